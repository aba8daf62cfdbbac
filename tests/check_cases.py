"""Rounds for the content-check tests (test_checks.py, test_gpu_checks.py): clean synthetic
rounds that exercise every rule, and offenders planted into them.

``ARRAY`` maps a rule to the RoundArrays field it reads; ``OFFENDERS`` to values that violate it
when stored there (rules 6 / 7: a table entry that drives the pair's sum out of range).
"""
import numpy as np

from pivot_place import _abi, synthetic

MODES = [_abi.PVT_CA_FF, _abi.PVT_CA_BF, _abi.PVT_OPP, _abi.PVT_VBP_FF, _abi.PVT_VBP_BF]
CA = (_abi.PVT_CA_FF, _abi.PVT_CA_BF)

ARRAY = {_abi.PVT_CHK_ZONE: "zone", _abi.PVT_CHK_AVAIL: "avail", _abi.PVT_CHK_DEM: "dem",
         _abi.PVT_CHK_GROUP: "task_group", _abi.PVT_CHK_ANCHOR: "group_anchor",
         _abi.PVT_CHK_COST: "cost", _abi.PVT_CHK_BW: "bw", _abi.PVT_CHK_RTBW: "rt_bw",
         _abi.PVT_CHK_DECAY: "decay", _abi.PVT_CHK_TIEBREAK: "tiebreak",
         _abi.PVT_CHK_MTPOS: "mt_state"}
# rules whose offender is a VALUE the kernels would only mis-order (never an index they follow)
VALUE_RULES = (_abi.PVT_CHK_AVAIL, _abi.PVT_CHK_DEM, _abi.PVT_CHK_COST, _abi.PVT_CHK_BW,
               _abi.PVT_CHK_DECAY)


def clean_round(mode, H, T, Z, seed=5, rt_bw=True):
    """A synthetic round of ``mode`` that reads every array its policy may: cost_aware rounds
    carry realtime bandwidth rows, cost_aware first-fit a host_decay column."""
    zones = 31     # locality.yml's; a wider table (the engine takes 32) repeats the last zone's row
    r = synthetic.make_round(mode, H, T, seed=seed, n_zones=min(Z, zones))
    if Z > zones:
        r.cost = np.pad(r.cost, (0, Z - zones), mode="edge")
        r.bw = np.pad(r.bw, (0, Z - zones), mode="edge")
        r.zone = (np.arange(H) % Z).astype(np.int32)
    if mode in CA and rt_bw:
        rs = np.random.RandomState(seed + 11)
        r.rt_bw = rs.uniform(0.5, 4.0, size=(max(r.n_groups, 1), H))
    if mode == _abi.PVT_CA_FF:
        r.decay = (1 + np.arange(H) % 3).astype(np.int32)
    return r


def grouped_round(mode, H, T, Z, G, seed=9):
    """A cost_aware round of exactly G groups (task t in group t % G, anchor g % Z) with
    realtime bandwidth rows (G, H)."""
    r = clean_round(mode, H, T, Z, seed=seed, rt_bw=False)
    r.task_group = (np.arange(T) % G).astype(np.int32)
    r.group_anchor = (np.arange(G) % Z).astype(np.int32)
    r.rt_bw = np.random.RandomState(seed).uniform(0.5, 4.0, size=(G, H))
    return r


def applicable(r):
    """The rules 1-10 that read an array of r (the table of include/pivot_place.h)."""
    T = r.n_tasks
    out = [_abi.PVT_CHK_ZONE, _abi.PVT_CHK_AVAIL]
    if T > 0:
        out.append(_abi.PVT_CHK_DEM)
    if r.task_group is not None and T > 0:
        out += [_abi.PVT_CHK_GROUP, _abi.PVT_CHK_ANCHOR]
    if r.mode in CA and T > 0:
        out += [_abi.PVT_CHK_COST, _abi.PVT_CHK_BW]
    if r.mode in CA and r.rt_bw is not None:
        out.append(_abi.PVT_CHK_RTBW)
    if r.decay is not None:
        out.append(_abi.PVT_CHK_DECAY)
    if r.mode == _abi.PVT_VBP_BF:
        out.append(_abi.PVT_CHK_TIEBREAK)
    return out


def length(r, rule):
    """Elements of the array rule ``rule`` reads."""
    if rule == _abi.PVT_CHK_RTBW:
        G = r.n_groups if r.task_group is not None else 0
        return max(G, 1) * r.n_hosts
    return getattr(r, ARRAY[rule]).size


def offender(r, rule, k=0):
    """The k-th kind of violating value for ``rule`` on round r."""
    H, Z = r.n_hosts, r.n_zones
    G = r.n_groups
    kinds = {
        _abi.PVT_CHK_ZONE: [Z, -1],
        _abi.PVT_CHK_AVAIL: [-0.0, np.nan, np.inf, -1.0],
        _abi.PVT_CHK_DEM: [np.nan, -0.0, -2.5, np.inf],
        _abi.PVT_CHK_GROUP: [G, -1],
        _abi.PVT_CHK_ANCHOR: [-1, Z],
        _abi.PVT_CHK_COST: [-1e6, np.nan],
        _abi.PVT_CHK_BW: [-1e12, np.nan],
        _abi.PVT_CHK_RTBW: [0.0, np.inf, np.nan, -1.0],
        _abi.PVT_CHK_DECAY: [0, -3],
        _abi.PVT_CHK_TIEBREAK: [H, 0xffffffff],
    }[rule]
    return kinds[k % len(kinds)]


def positions(n):
    """Index 0, the last index, and both sides of a 256-element block edge."""
    return sorted({i for i in (0, n - 1, 255, 256) if 0 <= i < n})


def plant(r, rule, index, value):
    """A copy of r with ``value`` stored at flat ``index`` of the rule's array."""
    out = r.copy()
    a = getattr(out, ARRAY[rule])
    a.reshape(-1)[index] = value
    return out
