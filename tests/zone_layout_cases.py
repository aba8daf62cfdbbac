"""cost_aware rounds on irregular host-zone layouts, for test_zone_layout_cases.py (CPU: the
reference's placements touch the boundaries each case aims at) and test_gpu_zone_layouts.py (every
engine path equals the reference).

``synthetic.make_round`` puts host h in zone h % Z: every zone's hosts are evenly strided, all zones
are equally large, none is empty, and a chain's zero-cost zone set U has the density |U| / Z
everywhere. The code that depends on WHERE a zone's hosts lie -- the window compaction
(csrc/pvt_zwin_dev.h), the host-sharded windows (zwin_build_kernel / zwin_merge_kernel of
csrc/pvt_zwalk.hip), the retry with the large window, the keyed first-fit zero-key prefix, the wide
walk's local zone ids -- never sees a dense pass, an empty pass, a window that fills in its first
row, or a hit in the last partial quad. The layouts here do that.

The geometry the cases aim at is named once below. Its source: csrc/pvt_kernels.h for ZW_M and
ZW_MBIG; csrc/pvt_zwin_dev.h for the passes (SCAN rows of NT threads x 4 hosts), which the walk
instantiates as <ZW_M, 256, 8> (csrc/pvt_zwalk.hip, ZW_THREADS / ZW_SCAN) and the order launch's
zone_window_block as <ZW_M, 1024, 2> (csrc/pvt_kernels.hip).

``CASES`` maps a name to its builder ``f(mode, sort_hosts=True)``; ``reference(name, mode,
sort_hosts)`` adds the CPU oracle's result, computed once and shared.
"""
import functools

import numpy as np

from oracle import oracle
from pivot_place import _abi, synthetic
from wide_frontier_cases import components

BF, FF = _abi.PVT_CA_BF, _abi.PVT_CA_FF
ZW_M = 1024             # window hosts
ZW_MBIG = 3072          # the large window of the retry
PASS = 8192             # hosts per pass, both instantiations: 8 x 256 x 4 = 2 x 1024 x 4
ROW_WALK = 1024         # hosts per row of the walk's instantiation (256 threads x 4)
ROW_ORDER = 4096        # ... of the order launch's (1024 threads x 4)
WAVE_WALK = 256         # hosts per wave and row (64 lanes x 4)

Z = 20
FAR = 19                # a singleton component: the zone of every host a case does not plant
WIDE_Z = 70
WIDE_FAR = 69
CAP = (16.0, 131072.0, 100.0, 1.0)
ROW = (1.0, 1024.0, 0.0, 0.0)
BLOCK_ANCHORS = ((0, 1100), (17, 700), (4, 300), (19, 100), (7, 1300))
BLOCKS_H = 12291
RESIDENT_H = 4093
WIDE_RESIDENT_H = 2045


def component_of(cost, z):
    """The zero-cost component (cost + cost.T == 0, transitively) of zone z, sorted."""
    return [c for c in components(cost) if z in c][0]


def wide_map():
    """Narrow zone k -> zone of the 70-zone cluster (synthetic.wide_zone_tables: zone i is base zone
    i % 31 in copy i // 31). Zones 0..18 go to copy 1 (31 + k: the same components, and {31, 32, 33}
    straddles local id 32); the far zone 19 goes to 69 (copy 2, whose component partner 68 holds no
    host)."""
    m = 31 + np.arange(Z)
    m[FAR] = WIDE_FAR
    return m


def _round(mode, H, T, seed, sort_hosts=True, wide=False):
    r = synthetic.make_round(mode, H, T, seed=seed, n_zones=WIDE_Z if wide else Z,
                             sort_hosts=sort_hosts)
    r.cost = np.array(r.cost, dtype=np.float64)
    r.bw = np.array(r.bw, dtype=np.float64)
    return r


def _regroup(r, anchors):
    """Tasks grouped by the given per-task anchors (first-seen group order)."""
    first = {}
    for a in anchors:
        first.setdefault(int(a), len(first))
    r.task_group = np.array([first[int(a)] for a in anchors], dtype=np.int32)
    r.group_anchor = np.array(list(first.keys()), dtype=np.int32)
    return r


def _fill(r, cap, row=ROW):
    for d in range(4):
        r.avail[d, :] = cap[d]
        r.dem[d, :] = row[d]


def one_task_cap(mode):
    """One task of ROW per host: an exact fit in cpus for best-fit (fit is >=), 1.5 cpus for
    first-fit (strict)."""
    return (1.0 if mode == BF else 1.5,) + CAP[1:]


def _zmap(r, zone, wide):
    r.zone = (wide_map()[zone] if wide else np.asarray(zone)).astype(np.int32)


def _anchors(counts, wide):
    a = np.concatenate([np.full(n, z, dtype=np.int64) for z, n in counts])
    return wide_map()[a] if wide else a


# ---- planted -------------------------------------------------------------------------------------
def planted_sets(H):
    """(A, B) host indices. A: eight hosts across the boundary of passes 0 and 1 and the three hosts
    of the partial last quad (H % 4 == 3). B: across the walk's first row boundary (1024, a wave
    boundary too), the order launch's first row boundary (4096) and a row boundary of pass 1 (the
    last one below H - 3 that both instantiations share where there is one)."""
    a = np.concatenate([np.arange(PASS - 4, PASS + 4), np.arange(H - 3, H)])
    edge = PASS + ROW_ORDER if PASS + ROW_ORDER + 1 < H - 3 else PASS + 2 * ROW_WALK
    b = np.concatenate([np.arange(ROW_WALK - 3, ROW_WALK + 2), np.arange(ROW_ORDER - 2, ROW_ORDER + 2),
                        [edge - 1, edge]])
    return a, b


def planted(mode, sort_hosts=True, wide=False):
    """H = 2 * 8192 + 3 (wide: 12291) hosts of (16, 131072, 100, 1), all in the far zone but the 11
    hosts of A (zones cycling 0, 1, 2) and the 11 of B (3, 4, 5), see planted_sets. Every task
    demands (1, 1024, 0, 0); five groups anchored at zones [0, 3, 1, 4, far] hold 88, 88, 88, 88 and
    40 tasks. The chains of {0, 1, 2} and {3, 4, 5} hold 176 tasks for 11 x 16 places: every planted
    host is filled (best-fit 16, first-fit 15: strict fit), in index order.

    Wide: A on zones 31, 32, 33, B on 34, 35, 36, far 69; B's last pair moves from 12287 / 12288 (the
    latter is of A's last quad at H = 12291) to 10239 / 10240, a row boundary of the walk's pass 1."""
    H = BLOCKS_H if wide else 2 * PASS + 3
    r = _round(mode, H, 392, 1, sort_hosts, wide)
    _fill(r, CAP)
    zone = np.full(H, FAR, dtype=np.int64)
    a, b = planted_sets(H)
    zone[a] = np.arange(len(a)) % 3
    zone[b] = 3 + np.arange(len(b)) % 3
    _zmap(r, zone, wide)
    return _regroup(r, _anchors(((0, 88), (3, 88), (1, 88), (4, 88), (FAR, 40)), wide))


# ---- window_edge ---------------------------------------------------------------------------------
def window_edge(mode, sort_hosts=True):
    """H = 3 * 8192 + 1, one task per host. Component {0, 1, 2} (zones cycling) owns hosts
    7168..8200: exactly ZW_M hits that end on the last host of pass 0, then nine more in the first
    quads of pass 1. A group of 1030 tasks anchored at zone 1 takes hosts 7168..8197 in order: the
    window fills on the very last host of a pass, and six tasks lie behind it. A group of 30 tasks
    anchored at the far zone follows."""
    H = 3 * PASS + 1
    r = _round(mode, H, 1060, 2, sort_hosts)
    _fill(r, one_task_cap(mode))
    zone = np.full(H, FAR, dtype=np.int64)
    own = np.arange(PASS - ZW_M, PASS + 9)
    zone[own] = np.arange(len(own)) % 3
    _zmap(r, zone, False)
    return _regroup(r, _anchors(((1, 1030), (FAR, 30)), False))


def window_edge_big(mode, sort_hosts=True):
    """The sibling for the large window: component {3, 4, 5} on hosts 0..3080 (3081 hosts), a chain
    of 3075 tasks (groups anchored at 3, 4 and 5: 1000 + 1000 + 1075) that crosses ZW_MBIG = 3072
    by three; 30 tasks anchored at the far zone. (Four groups: best-fit rounds run group epochs
    only with at most 1024 tasks per group on average.)"""
    H = 3 * PASS + 1
    r = _round(mode, H, 3105, 3, sort_hosts)
    _fill(r, one_task_cap(mode))
    zone = np.full(H, FAR, dtype=np.int64)
    own = np.arange(0, ZW_MBIG + 9)
    zone[own] = 3 + np.arange(len(own)) % 3
    _zmap(r, zone, False)
    return _regroup(r, _anchors(((3, 1000), (4, 1000), (5, 1075), (FAR, 30)), False))


# ---- blocks --------------------------------------------------------------------------------------
def block_counts(H):
    """BLOCK_ANCHORS' task counts scaled to H hosts (the stated counts at H = 12291)."""
    return tuple((z, n * H // BLOCKS_H) for z, n in BLOCK_ANCHORS)


def blocks(mode, sort_hosts=True, H=BLOCKS_H, desc=False, wide=False):
    """Contiguous zones: zone = h * 20 // H (desc: 19 - that), one task per host, H % 4 == 3 (the
    resident sizes: 1). Per-task anchors 0 x 1100, 17 x 700, 4 x 300, 19 x 100, 7 x 1300 (scaled by
    H / 12291 below that size) shuffled with RandomState(2).

    H = 12291: group 0's component {0, 1, 2} is hosts 0..1843, so the first pass is dense and the
    window overflows in the middle of row 0; the group takes hosts 0..1099. Group 7's component
    {6, 7} has 1229 hosts for 1300 tasks: 71 tasks spill at positive cost. Group 17's component
    starts at host 9833: pass 0 is empty. desc mirrors it: group 0's hosts start at 10448 behind an
    empty pass, group 7's 1229 hosts (7375..8603) straddle the pass boundary.

    Wide: the narrow zones through wide_map()."""
    T = sum(n for _, n in block_counts(H))
    r = _round(mode, H, T, 4, sort_hosts, wide)
    _fill(r, one_task_cap(mode))
    zone = np.arange(H, dtype=np.int64) * Z // H
    _zmap(r, (Z - 1 - zone) if desc else zone, wide)
    anchors = np.random.RandomState(2).permutation(_anchors(block_counts(H), wide))
    return _regroup(r, anchors)


def blocks_desc(mode, sort_hosts=True, H=BLOCKS_H):
    """blocks with the zones descending."""
    return blocks(mode, sort_hosts, H, desc=True)


# ---- skew ----------------------------------------------------------------------------------------
# The recipe as first stated (2 cpus per host, any seed) places every task at zero cost: the demands
# are 0.5 or 1 cpu and the smallest component still has room. Chosen on the CPU reference instead:
# seed 8 and one task per host (1 cpu best-fit, 1.5 first-fit), where the groups of the two smallest
# components spill at positive cost and the other 18 are placed wholly at zero cost.
SKEW_SEED = 8


def skew_zones(H, seed=SKEW_SEED):
    """Zones drawn with p ~ 1 / k^2, k = 1..20, through a random zone permutation."""
    rs = np.random.RandomState(seed)
    p = 1.0 / np.arange(1, Z + 1) ** 2
    perm = rs.permutation(Z)
    return perm[rs.choice(Z, size=H, p=p / p.sum())]


def skew(mode, sort_hosts=True, H=20003, T=1500):
    """H = 20003 hosts in zones of very different sizes (about 12 500 hosts down to about 20),
    make_round's demands (0.5 or 1 cpu), crowded: one task and 50000 of memory per host. Small
    components run dry and spill at positive cost while the large ones place everything at zero
    cost."""
    r = _round(mode, H, T, SKEW_SEED, sort_hosts)
    r.avail[0, :] = one_task_cap(mode)[0]
    r.avail[1, :] = 50000.0
    _zmap(r, skew_zones(H), False)
    return r


# ---- tail ----------------------------------------------------------------------------------------
TAIL_N = 37


def tail(mode, sort_hosts=True, H=9003, T=600):
    """Every host in zone 5 except the last 37, which cycle through the other 19 zones (H % 4 == 3
    at 9003, 1 at 4093): a group anchored outside {3, 4, 5} has at most six zero-cost hosts, all
    behind index H - 37, behind a pass (H = 9003) of no hit at all. make_round's demands; the tail
    hosts hold (4, 20000, 100, 1) so that every group fills its own and spills."""
    r = _round(mode, H, T, 6, sort_hosts)
    zone = np.full(H, 5, dtype=np.int64)
    others = np.array([z for z in range(Z) if z != 5])
    zone[H - TAIL_N:] = others[np.arange(TAIL_N) % len(others)]
    _zmap(r, zone, False)
    r.avail[0, H - TAIL_N:] = 4.0
    r.avail[1, H - TAIL_N:] = 20000.0
    return r


# ---- empty_zones ---------------------------------------------------------------------------------
def empty_zones(mode, sort_hosts=True, one=False, H=9001, T=600):
    """H = 9001 hosts in the even zones only (zone = 2 * (h % 10)); one: every host in zone 5.
    make_round's availability and demands, anchors over all 20 zones: groups whose anchor zone is
    empty while its component is not, and (one) groups whose whole component is empty -- U != 0 and
    an empty window."""
    r = _round(mode, H, T, 7, sort_hosts)
    _zmap(r, np.full(H, 5) if one else 2 * (np.arange(H) % 10), False)
    return r


def empty_zones_one(mode, sort_hosts=True):
    return empty_zones(mode, sort_hosts, one=True)


# ---- wide ----------------------------------------------------------------------------------------
def wide_blocks(mode, sort_hosts=True, H=BLOCKS_H):
    """blocks on the 70-zone cluster (wide_map): the dense component is {31, 32, 33}."""
    return blocks(mode, sort_hosts, H, wide=True)


def wide_planted(mode, sort_hosts=True):
    """planted on the 70-zone cluster at H = 12291: A on zones 31, 32, 33, B on 34, 35, 36."""
    return planted(mode, sort_hosts, wide=True)


CASES = {f.__name__: f for f in (planted, window_edge, window_edge_big, blocks, blocks_desc, skew,
                                 tail, empty_zones, empty_zones_one, wide_blocks, wide_planted)}
NAMES = list(CASES)
# resident-sized variants: name -> (builder, keyword arguments)
RESIDENT = {"blocks": (blocks, dict(H=RESIDENT_H)), "skew": (skew, dict(H=RESIDENT_H, T=1500)),
            "tail": (tail, dict(H=RESIDENT_H, T=600)),
            "wide_blocks": (wide_blocks, dict(H=WIDE_RESIDENT_H))}
# H % 4 of every case
RESIDUE = {"planted": 3, "window_edge": 1, "window_edge_big": 1, "blocks": 3, "blocks_desc": 3,
           "skew": 3, "tail": 3, "empty_zones": 1, "empty_zones_one": 1, "wide_blocks": 3,
           "wide_planted": 3}


@functools.lru_cache(maxsize=None)
def reference(name, mode, sort_hosts=True):
    """(round, oracle result) of the named case, computed once and shared; callers must not modify
    either."""
    r = CASES[name](mode, sort_hosts)
    return r, oracle.place(r, threads=4)


@functools.lru_cache(maxsize=None)
def resident_reference(name, mode, sort_hosts=True):
    f, kw = RESIDENT[name]
    r = f(mode, sort_hosts, **kw)
    return r, oracle.place(r, threads=4)


def zero_cost(r, ref):
    """Per task: True where it was placed at zero cost (anchor and host zone exchange for free)."""
    placed = ref.placement >= 0
    anc = r.group_anchor[r.task_group]
    z = r.zone[np.where(placed, ref.placement, 0)]
    return placed & ((r.cost[anc, z] + r.cost[z, anc]) == 0.0)
