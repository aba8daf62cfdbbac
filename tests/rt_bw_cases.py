"""cost_aware rounds with realtime bandwidths (pvt_round.rt_bw: one bandwidth per group and host
instead of the static bw[a][z] + bw[z][a]), for test_rt_bw_cases.py (CPU: on the oracle alone every
case does what it claims, and its placements depend on rt_bw) and test_gpu_rt_bw.py (every engine
path equals the oracle bit for bit).

Every builder returns a ``RoundArrays`` on ``synthetic.make_round``'s cluster. All but ``extreme``
and ``wide`` add 0.001 to every cost, so that no zone pair is free and every score depends on the
bandwidth.
Row g of rt_bw belongs to group g; a round without task_group has the one row 0.

``reference(name, *args)`` adds the oracle's result, computed once and shared: callers must not
modify either (``fresh`` copies a round for an entry point that takes host arrays).
"""
import functools

import numpy as np

import wide_cases
from oracle import oracle
from pivot_place import _abi, synthetic

BF, FF = _abi.PVT_CA_BF, _abi.PVT_CA_FF
MODES = [BF, FF]
IDS = ["bf", "ff"]

# the sizes, the smallest that still reach each path. The windowed task counts are odd and leave
# an odd last window at windows of 1, 3, 37 (297 = 8 * 37 + 1) and 1024 (1499 = 1024 + 475), so
# that the score kernel's 2- and 4-tasks-per-wave instances both meet a window tail.
TINY = (5, 40)              # more ranks than hosts
WINDOWED = (5000, 297)      # windowed; several windows at small window sizes
RESIDENT = (3000, 1500)     # resident kernel, host batch (and windowed with the resident limit at 0)
EPOCHS = (20000, 1499)      # windowed with group epochs, several segments

EXTREME_VALUES = (5e-324, 1e-300, 1e-160, 1e160, 1e300, 1.7e308)
TINY_COST = 2.0 ** -80      # extreme: the factor on the costs of every other zone
# tight, best-fit: tasks on 3000 hosts of which the oracle leaves some waiting (at 1500 it places all)
TIGHT_BF_TASKS = 4096


def _round(mode, H, T, seed, free=False, **kw):
    r = synthetic.make_round(mode, H, T, seed=seed, **kw)
    r.cost = np.array(r.cost, dtype=np.float64) if free else r.cost + 0.001
    return r


def queue_rows(r, seed):
    """The static bandwidth of every (group, host) divided by a queue factor randint(1, 4):
    bandwidths differ inside a zone, and equal values repeat (ties on the host index occur)."""
    rs = np.random.RandomState(seed)
    bsum = r.bw + r.bw.T
    a = r.group_anchor if r.group_anchor is not None else np.zeros(1, dtype=np.int32)
    return (bsum[a][:, r.zone] / rs.randint(1, 4, size=(len(a), r.n_hosts))).astype(np.float64)


def uniform_rows(r, seed):
    """U(0.5, 200) per (group, host), unrelated to the zone."""
    rs = np.random.RandomState(seed)
    return np.ascontiguousarray(rs.uniform(0.5, 200.0, size=(max(r.n_groups, 1), r.n_hosts)))


def queue(mode, H, T, seed, sort_hosts=True):
    r = _round(mode, H, T, seed, sort_hosts=sort_hosts)
    r.rt_bw = queue_rows(r, seed)
    return r


def uniform(mode, H, T, seed):
    r = _round(mode, H, T, seed)
    r.rt_bw = uniform_rows(r, seed)
    return r


def ungrouped(mode, H, T, seed):
    """task_group = group_anchor = NULL: one group of every task, anchored at zone 0, and the one
    row 0 of rt_bw (queue rows of zone 0)."""
    r = _round(mode, H, T, seed)
    r.task_group = r.group_anchor = None
    r.rt_bw = queue_rows(r, seed)
    assert r.rt_bw.shape == (1, H)
    return r


def few_groups(mode, H, T, seed, G):
    """``queue`` with make_round's groups folded into the first G (group g % G, the first G
    anchors): another number of rt_bw rows for the staging."""
    r = _round(mode, H, T, seed)
    assert r.n_groups >= G
    r.task_group = (r.task_group % G).astype(np.int32)
    r.group_anchor = r.group_anchor[:G].copy()
    r.rt_bw = queue_rows(r, seed)
    return r


def with_decay(H, T, seed):
    """First-fit with sort_hosts and host_decay: the key is c * decay / (||avail|| * rt_bw)."""
    r = queue(FF, H, T, seed)
    r.decay = np.random.RandomState(seed + 1).randint(1, 6, size=H).astype(np.int32)
    return r


def unsorted_ff(H, T, seed):
    """First-fit without sort_hosts: the reference reads no bandwidth there, rt_bw is ignored."""
    return queue(FF, H, T, seed, sort_hosts=False)


def tight(mode, H, T, seed):
    """One cpu per host, half a cpu on every seventh, 40000 of memory, uniform rows: hosts fill up
    and lists run dry (first-fit fits strictly: the half-cpu hosts never take a task)."""
    r = _round(mode, H, T, seed)
    r.avail[0] = 1.0
    r.avail[0, ::7] = 0.5
    r.avail[1] = 40000.0
    r.rt_bw = uniform_rows(r, seed)
    return r


def extreme_scaled_zones(r):
    """The zones whose costs ``extreme`` scales by TINY_COST: those of the other parity than group
    0's anchor."""
    return np.arange(r.n_zones) % 2 != int(r.group_anchor[0]) % 2


def extreme_planted(r):
    """The three hosts ``extreme`` plants for task 0: the first hosts at or behind H/8, H/2 and
    7H/8 in a zone of unscaled, positive cost to group 0's anchor."""
    a = int(r.group_anchor[0])
    c = r.cost[a] + r.cost[:, a]
    ok = (c[r.zone] > 0) & ~extreme_scaled_zones(r)[r.zone]
    H = r.n_hosts
    return [int(s + np.argmax(ok[s:])) for s in (H // 8, H // 2, 7 * H // 8)]


def extreme(mode, H, T, seed):
    """A ``queue`` round WITH its free zone pairs in which a seeded tenth of every row of rt_bw is
    replaced by values of EXTREME_VALUES, so that true zero scores (c == 0), scores that underflow
    to denormals or to exactly +0 with c > 0 and scores of +inf meet in one task's candidates.

    Two things the plain recipe does not give by itself are added. (1) With costs of 0.01 and more
    and residual norms of 100 and more (100 of disk is never demanded), a best-fit score
    c * ||avail - d|| / bw is at least 5e-309 at bw = 1.7e308: no underflow to 0. The costs between
    a zone of the other parity than group 0's anchor and any zone are therefore scaled by 2^-80
    (free pairs stay free): c * ||.|| is then about 1e-21, a denormal over 1e300 and exactly +0 over
    1.7e308, while the unscaled pairs still overflow to +inf over 5e-324. (2) A task whose every
    feasible host scores +inf: task 0 (of group 0, the first one processed) demands
    (15.5, 131000, 0, 0), no host keeps more than 130000 of memory except three planted ones of
    (16, 131072, 100, 1) in unscaled positive-cost zones, whose bandwidth to group 0 is 5e-324."""
    r = _round(mode, H, T, seed, free=True)
    rt = queue_rows(r, seed)
    rs = np.random.RandomState(seed + 2)
    n = max(H // 10, 1)
    for g in range(rt.shape[0]):
        rt[g, rs.choice(H, size=n, replace=False)] = rs.choice(EXTREME_VALUES, size=n)
    s = extreme_scaled_zones(r)
    r.cost[s[:, None] | s[None, :]] *= TINY_COST
    r.avail[1] = np.minimum(r.avail[1], 130000.0)
    r.dem[:, 0] = (15.5, 131000.0, 0.0, 0.0)
    for h in extreme_planted(r):
        r.avail[:, h] = (16.0, 131072.0, 100.0, 1.0)
        rt[0, h] = 5e-324
    r.rt_bw = rt
    return r


def wide(mode):
    """The contended 65-zone round of the wide-zone tests with uniform rows."""
    r = wide_cases.contended_round(mode, 65, *wide_cases.SMALL[65])
    r.rt_bw = uniform_rows(r, 17)
    return r


CASES = {f.__name__: f for f in (queue, uniform, ungrouped, few_groups, with_decay, unsorted_ff, tight,
                                 extreme, wide)}


def _plain(mode, H, T, seed, **kw):
    return synthetic.make_round(mode, H, T, seed=seed, **kw)


def batch_rounds():
    """[(label, round)] of a host batch of all five policies whose cost_aware rounds carry rt_bw
    in turn: 1 (ungrouped), 3 and 20 rows, 64, 1000 and 3000 hosts, one with decay, two extreme.
    Each sits next to a round without rt_bw. The batch's table cache holds the tables of its first
    round with tasks (``table_cache_hits``), here the +0.001 tables: the rt_bw rounds of 1, 3 and
    20 rows on those tables read the cached copy next to their staged rt_bw block, while the
    extreme rounds (scaled costs) and every round on make_round's own tables stage their own."""
    VF, VB, OPP = _abi.PVT_VBP_FF, _abi.PVT_VBP_BF, _abi.PVT_OPP
    return [("bf 20 rows 3000", queue(BF, 3000, 301, 607)),
            ("vbp_ff", _plain(VF, 1000, 90, 601)),
            ("bf ungrouped 64", ungrouped(BF, 64, 150, 602)),
            ("bf static, cached tables", without_rt(queue(BF, 1000, 120, 603))),
            ("opp", _plain(OPP, 1000, 77, 604)),
            ("ff 3 rows", few_groups(FF, 1000, 333, 605, 3)),
            ("ff static, other tables", _plain(FF, 1000, 140, 606)),
            ("ff decay", with_decay(1000, 257, 609)),
            ("vbp_bf", _plain(VB, 1000, 64, 608)),
            ("bf extreme", extreme(BF, 3000, 400, 610)),
            ("ff extreme", extreme(FF, 3000, 400, 610)),
            ("bf static after extreme", without_rt(uniform(BF, 1000, 99, 611))),
            ("ff ungrouped 1000", ungrouped(FF, 1000, 211, 612)),
            ("bf 3 rows 64", few_groups(BF, 64, 130, 613, 3)),
            ("opp again", _plain(OPP, 513, 40, 614)),
            ("ff 20 rows 3000", queue(FF, 3000, 299, 615))]


def wide_batch_rounds():
    """A host batch holding the 65-zone ``wide`` rounds: every round has at most 2048 hosts, so the
    whole batch runs on the wide resident kernels, the 20-zone rt_bw rounds included. Its first
    round is a wide one, so the cache holds the 65-zone tables: the wide rounds hit it, the
    20-zone rounds stage their own tables."""
    VF, VB, OPP = _abi.PVT_VBP_FF, _abi.PVT_VBP_BF, _abi.PVT_OPP
    return [("bf wide", wide(BF)),
            ("vbp_ff 2048", _plain(VF, 2048, 150, 622)),
            ("bf 20 zones", queue(BF, 1000, 203, 621)),
            ("opp", _plain(OPP, 700, 60, 623)),
            ("ff wide static", without_rt(wide(FF))),
            ("ff wide", wide(FF)),
            ("vbp_bf", _plain(VB, 333, 50, 625)),
            ("ff ungrouped", ungrouped(FF, 2047, 175, 624))]


def table_cache_hits(rounds):
    """Per round of a host batch, whether it reads the cached zone tables, by the engine's rule
    (csrc/pvt_resident.hip, zone_cache under pvt_place_host_batch): the first round with tasks
    that passes tables takes the cache (it finds its tables there or fills it), and a later round
    reads it exactly when its zone count, cost and bw equal that round's, whatever its policy;
    every other round stages its own tables."""
    first = next(r for r in rounds if r.n_tasks > 0)
    return [r.n_tasks > 0 and r.cost.shape == first.cost.shape and np.array_equal(r.cost, first.cost)
            and np.array_equal(r.bw, first.bw) for r in rounds]


def build(name, *args):
    return CASES[name](*args)


@functools.lru_cache(maxsize=None)
def reference(name, *args):
    """(round, oracle result) of ``CASES[name](*args)``, computed once and shared."""
    r = build(name, *args)
    return r, oracle.place(r, threads=4 if r.n_hosts >= 20000 else 0)


def fresh(r):
    return r.copy()


def without_rt(r):
    """The same round with the static bandwidths."""
    p = r.copy()
    p.rt_bw = None
    return p


def scores(r, avail, g, d=None):
    """Per host, the score the oracle gives group g's hosts in numpy, in its order of operations:
    best-fit (c * ||avail - d||) * 1.0 / bw for the demand d, first-fit the key
    c * decay / (||avail|| * bw) (d None). The norm's sum of squares is numpy's, not the oracle's
    FMA chain: the last bit can differ, which no test of +0 or +inf here is near to."""
    a = int(r.group_anchor[g]) if r.group_anchor is not None else 0
    c = (r.cost[a] + r.cost[:, a])[r.zone]
    bw = r.rt_bw[g] if r.rt_bw is not None else (r.bw[a] + r.bw[:, a])[r.zone]
    with np.errstate(over="ignore", under="ignore", divide="ignore", invalid="ignore"):
        if d is not None:
            x = avail - np.asarray(d)[:, None]
            return c, c * np.sqrt((x * x).sum(axis=0)) * 1.0 / bw
        df = r.decay.astype(np.float64) if r.decay is not None else 1.0
        return c, c * df / (np.sqrt((avail * avail).sum(axis=0)) * bw)


def replay(r, ref):
    """Walk the oracle's result in processing order; yields per task (t, winner or -1, feasible
    mask, c per host, score per host) with the availability of that moment (first-fit: the keys
    frozen at the group's start)."""
    avail = r.avail.copy()
    tg = r.task_group if r.task_group is not None else np.zeros(r.n_tasks, dtype=np.int32)
    cur, key = -1, None
    for t in ref.order:
        g = int(tg[t])
        d = r.dem[:, t]
        if r.mode == FF:
            if g != cur:
                cur, key = g, scores(r, avail, g)
            c, s = key
            feas = (avail > d[:, None]).all(axis=0)
        else:
            c, s = scores(r, avail, g, d)
            feas = (avail >= d[:, None]).all(axis=0)
        w = int(ref.placement[t])
        yield int(t), w, feas, c, s
        if w >= 0:
            avail[:, w] -= d
