"""Rounds for the frontier walk and the group epochs on clusters of 33 to 512 zones (DESIGN.md
§2.6), for test_wide_frontier_cases.py (CPU: the cases are what they claim to be) and
test_gpu_wide_frontier.py (the windowed engine equals the reference and takes the path it should).

``embed(r, Z, zmap)`` puts a round of up to 32 zones into a Z-zone cluster: zone and group_anchor
go through the injective ``zmap``, the original cost / bw block sits at ``np.ix_(zmap, zmap)``,
every other pair costs 1.0 (0.0 on the diagonal) at bandwidth 100.0, and no host lies in the added
zones. The added zones are singleton zero-cost components that no task is anchored in and no host
lives in, and zone ids only ever select table entries, so the reference places the embedded round
exactly as the original one. Expectations that exist for the narrow rounds (cert_cases.Expect)
therefore hold for the embedded ones.

References are computed once per case and shared; callers must not modify them."""
import functools

import numpy as np

import cert_cases as cc
from oracle import oracle
from pivot_place import _abi, synthetic

BF, FF = _abi.PVT_CA_BF, _abi.PVT_CA_FF
WIDE_Z = (33, 64, 65, 512)
# uncontended rounds: synthetic.make_round(mode, H, T, seed, n_zones=Z); every task is placed at
# zero cost
UNCONTENDED = {33: (3000, 400, 1), 64: (5000, 600, 2), 65: (5000, 600, 2), 512: (12000, 1500, 3)}


def embed(r, Z, zmap):
    zmap = np.asarray(zmap, dtype=np.int64)
    z0 = r.n_zones
    assert z0 <= 32 and len(zmap) >= z0 and len(set(zmap.tolist())) == len(zmap)
    assert zmap.min() >= 0 and zmap.max() < Z
    zm = zmap[:z0]
    e = r.copy()
    e.zone = zm[r.zone].astype(np.int32)
    e.group_anchor = zm[r.group_anchor].astype(np.int32)
    cost = np.ones((Z, Z), dtype=np.float64)
    np.fill_diagonal(cost, 0.0)
    bw = np.full((Z, Z), 100.0, dtype=np.float64)
    cost[np.ix_(zm, zm)] = r.cost
    bw[np.ix_(zm, zm)] = r.bw
    e.cost, e.bw = np.ascontiguousarray(cost), np.ascontiguousarray(bw)
    return e


def plain_zmap(Z):
    """The descending maps the embedding was checked with."""
    return (Z - 1 - np.arange(32)) if Z < 512 else (Z - 1 - 3 * np.arange(32)) % Z


def cert_zmap(Z):
    """Every zone a cert case uses above id 32, the zones of its two components {0, 1, 2} and
    {3, 4, 5} interleaved in global id (0, 3, 1, 4, 2, 5 ascending), so that a local id taken for a
    global one -- or the other way round -- picks a zone of the other component; the other zones
    follow in steps of 1 (Z = 64) or 7 (Z = 512)."""
    lo = 34 if Z == 64 else 301
    step = 1 if Z == 64 else 7
    m = np.empty(20, dtype=np.int64)            # (the cert cases have 20 zones)
    m[[0, 3, 1, 4, 2, 5]] = lo + step * np.arange(6)
    m[6:] = lo + step * np.arange(6, 20)
    assert m.max() < Z
    return m


def same_result(a, b):
    """NaN-aware equality of two results (window_cap_nan carries a NaN capacity)."""
    return (np.array_equal(a.placement, b.placement) and np.array_equal(a.order, b.order) and
            np.array_equal(a.avail, b.avail, equal_nan=True))


@functools.lru_cache(maxsize=None)
def cert_case(name, Z):
    """(embedded round, Expect, the reference of the NARROW round) of a cert_cases case."""
    r, e, ref = cc.reference(name)
    return embed(r, Z, cert_zmap(Z)), e, ref


def spill_round(seed=10):
    """The 20000 x 6000 round of test_gpu_epochs.test_epochs_groups_spill_and_collide."""
    r = synthetic.make_round(BF, 20_000, 6000, seed=seed)
    r.avail[:2, r.zone < 10] = 0.0
    return r


@functools.lru_cache(maxsize=None)
def spill_case(Z=64):
    r = spill_round()
    ref = oracle.place(r, threads=8)
    return embed(r, Z, plain_zmap(Z)), ref


# ---- a certificate only the wide walk has: zones outside the anchor's component ----------------
# The cert_cases skeleton at 64 zones with the planted host 4 moved into an ADDED zone X, a
# singleton component: X is outside A's component, not merely outside the chain's zone set, so the
# clause that guards it is the one over the zones outside the component (c >= 2^-300 and
# 0 < bw <= 2^300 on the anchor's row). Disk holds the separation 2^-288 on the planted host, so
# the separation certificate holds in every case and the score of the planted host for A is
# c * 2^-288 / bw.
#   out_c_bw    c = 2^-400, bw = 2^400: 2^-1088 underflows to 0 -- the reference takes the host.
#               (Either value alone cannot underflow while the separation holds: with bw <= 2^300
#               the score is >= 2^-988, with c >= 2^-300 and bw = 2^400 it is 2^-988 too. So the
#               two single-clause cases below go further out, as c_at_limits and bw_huge do.)
#   out_c       c = 2^-500, bw = 2^300: 2^-1088 -- `c` alone fails
#   out_bw      c = 2^-300, bw = 2^1023: underflows -- `bw` alone fails
#   out_limits  c = 2^-300, bw = 2^300: 2^-888 > 0 -- every clause at its limit, the walk may prove
OUT_Z = 64
OUT_X = 20                                      # an added zone (cert_zmap(64) starts at 34)
OUT_CASES = {"out_c_bw": (-400, 400, True), "out_c": (-500, 300, True),
             "out_bw": (-300, 1023, True), "out_limits": (-300, 300, False)}


@functools.lru_cache(maxsize=None)
def out_case(name):
    """(round, planted?, reference): A's first task is task 2."""
    ce, be, planted = OUT_CASES[name]
    r = cc.skeleton(BF, 6, 2)
    r.avail[:, cc.PLANTED] = (1.0, 2048.0, cc.p2(-288), 0.0)
    zmap = cert_zmap(OUT_Z)
    e = embed(r, OUT_Z, zmap)
    assert OUT_X not in zmap.tolist()
    e.zone = e.zone.copy()
    e.zone[cc.PLANTED] = OUT_X
    a = int(zmap[cc.A_ZONE])
    e.cost[a, OUT_X], e.cost[OUT_X, a] = cc.p2(ce - 1), cc.p2(ce - 1)
    if be == 1023:
        e.bw[a, OUT_X], e.bw[OUT_X, a] = cc.p2(1023), 0.0
    else:
        e.bw[a, OUT_X], e.bw[OUT_X, a] = cc.p2(be - 1), cc.p2(be - 1)
    return e, planted, oracle.place(e)


# ---- the component limit: 32 zones per zero-cost component --------------------------------------
def limit_round(mode=BF):
    """70 zones: zones 0..31 form a path (zero cost between consecutive zones only), zones 32..64 a
    path of 33, zones 65..69 are singletons. A chain's zone set stays small (an anchor reaches
    itself and its two neighbours) while its component is large. Groups are anchored in both paths
    and in singletons; hosts have room for everything at zero cost."""
    Z, H, T = 70, 7000, 700
    r = synthetic.make_round(mode, H, T, seed=4, n_zones=Z)
    cost = np.ones((Z, Z), dtype=np.float64)
    np.fill_diagonal(cost, 0.0)
    for lo, hi in ((0, 31), (32, 64)):
        for z in range(lo, hi):
            cost[z, z + 1] = cost[z + 1, z] = 0.0
    r.cost = np.ascontiguousarray(cost)
    r.bw = np.full((Z, Z), 100.0, dtype=np.float64)
    anchors = np.array([3, 40, 66, 17, 60, 68, 30, 33])[np.arange(T) % 8]
    first = {}
    for a in anchors:
        first.setdefault(int(a), len(first))
    r.task_group = np.array([first[int(a)] for a in anchors], dtype=np.int32)
    r.group_anchor = np.array(list(first.keys()), dtype=np.int32)
    return r


@functools.lru_cache(maxsize=None)
def limit_case():
    r = limit_round()
    return r, oracle.place(r)


def components(cost):
    """Zero-cost components of a cost table: list of sorted zone lists."""
    c = np.asarray(cost, dtype=np.float64)
    z0 = (c + c.T) == 0.0
    Z = len(c)
    root = list(range(Z))

    def find(z):
        while root[z] != z:
            root[z] = root[root[z]]
            z = root[z]
        return z
    for a, z in zip(*np.nonzero(z0)):
        root[find(int(a))] = find(int(z))
    out = {}
    for z in range(Z):
        out.setdefault(find(z), []).append(z)
    return list(out.values())


@functools.lru_cache(maxsize=None)
def uncontended(mode, Z):
    H, T, seed = UNCONTENDED[Z]
    r = synthetic.make_round(mode, H, T, seed=seed, n_zones=Z)
    return r, oracle.place(r, threads=4)


@functools.lru_cache(maxsize=None)
def stopped_chains_case():
    """The uncontended 64-zone best-fit round with zones 0-9 emptied (the narrow chain_stops round
    of test_gpu_epoch_tail.py at 64 zones): chains anchored there stop, while the chains of the
    other components complete and write their windows back -- a missed epoch with something to
    undo. (In wide_cases' contended rounds every chain stops, so nothing is written back.)"""
    H, T, seed = UNCONTENDED[64]
    r = synthetic.make_round(BF, H, T, seed=seed, n_zones=64)
    r.avail[:2, r.zone < 10] = 0.0
    return r, oracle.place(r, threads=4)


def zero_cost_fraction(r, ref):
    """(placed / tasks, zero-cost winners / placed)."""
    placed = ref.placement >= 0
    anc = r.group_anchor[r.task_group[placed]]
    z = r.zone[ref.placement[placed]]
    c = r.cost[anc, z] + r.cost[z, anc]
    return float(placed.mean()), float((c == 0).mean())
