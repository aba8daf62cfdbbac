"""The content rules of a round in numpy (``include/pivot_place.h``, enum pvt_check).

``check_arrays`` says whether a ``RoundArrays`` is a round the engine may be given. It restates
the rule table of the header and never calls the library, so it serves callers without a GPU,
and it is the checker the device check (``PlacementEngine.check``) is tested against.

A rule applies only where the engine reads the array:

==  =========  ================================  ==============================================
 1  zone       always                            zone[h] outside [0, Z)
 2  avail      always                            avail[i] not finite, or sign bit set (-0.0 too)
 3  dem        T > 0                             dem[i]: as rule 2
 4  group      task_group set, T > 0             task_group[t] outside [0, G)
 5  anchor     task_group set, T > 0             group_anchor[g] outside [0, Z)
 6  cost       cost_aware, T > 0                 not (cost[a][z] + cost[z][a] >= 0), index a*Z+z
 7  bw         cost_aware, T > 0                 not (bw[a][z] + bw[z][a] > 0)
 8  rt_bw      rt_bw set, cost_aware             rt_bw[i], i < max(G,1)*H, not finite or not > 0
 9  decay      decay set                         decay[h] < 1
10  tiebreak   vbp best-fit                      tiebreak[h] >= H, or an earlier host has the value
11  mt pos     opportunistic                     mt_state[624] > 624
==  =========  ================================  ==============================================
"""
import numpy as np

from . import _abi
from ._abi import CheckReport, RoundArrays


def _bad_amount(v):
    return ~np.isfinite(v) | np.signbit(v)


def check_arrays(r: RoundArrays) -> CheckReport:
    """The verdict ``pvt_check_round`` gives for the same arrays: the lowest-numbered violated
    rule, its lowest violating flat index, how many elements violate it, the element there, and
    the mask of every violated rule."""
    H, T, Z = r.n_hosts, r.n_tasks, r.n_zones
    grouped = r.task_group is not None
    G = r.n_groups if grouped else 0
    ca = r.mode in (_abi.PVT_CA_FF, _abi.PVT_CA_BF)
    found = []        # (rule, bad mask over the flat array, the flat values)

    def rule(code, bad, values):
        found.append((code, np.asarray(bad).ravel(), np.asarray(values).ravel()))

    rule(_abi.PVT_CHK_ZONE, (r.zone < 0) | (r.zone >= Z), r.zone)
    rule(_abi.PVT_CHK_AVAIL, _bad_amount(r.avail), r.avail)
    if T > 0:
        rule(_abi.PVT_CHK_DEM, _bad_amount(r.dem), r.dem)
    if grouped and T > 0:
        rule(_abi.PVT_CHK_GROUP, (r.task_group < 0) | (r.task_group >= G), r.task_group)
        if r.group_anchor is not None:
            rule(_abi.PVT_CHK_ANCHOR, (r.group_anchor < 0) | (r.group_anchor >= Z), r.group_anchor)
    if ca and T > 0:
        with np.errstate(invalid="ignore"):
            c = r.cost + r.cost.T
            b = r.bw + r.bw.T
            rule(_abi.PVT_CHK_COST, ~(c >= 0.0), c)
            rule(_abi.PVT_CHK_BW, ~(b > 0.0), b)
    if ca and r.rt_bw is not None:
        v = r.rt_bw.ravel()[:max(G, 1) * H]
        with np.errstate(invalid="ignore"):
            rule(_abi.PVT_CHK_RTBW, ~(np.isfinite(v) & (v > 0.0)), v)
    if r.decay is not None:
        rule(_abi.PVT_CHK_DECAY, r.decay < 1, r.decay)
    if r.mode == _abi.PVT_VBP_BF and r.tiebreak is not None:
        later = np.ones(H, dtype=bool)        # a host after the first one holding its value
        later[np.unique(r.tiebreak, return_index=True)[1]] = False
        rule(_abi.PVT_CHK_TIEBREAK, (r.tiebreak >= H) | later, r.tiebreak)
    if r.mode == _abi.PVT_OPP and r.mt_state is not None:
        bad = np.zeros(625, dtype=bool)
        bad[624] = r.mt_state[624] > 624
        rule(_abi.PVT_CHK_MTPOS, bad, r.mt_state)

    rep = CheckReport()
    for code, bad, values in found:
        if not bad.any():
            continue
        rep.mask |= 1 << code
        if rep.code == 0:
            i = int(np.flatnonzero(bad)[0])
            rep.code, rep.index, rep.count = code, i, int(bad.sum())
            rep.value = float(values[i])
    return rep
