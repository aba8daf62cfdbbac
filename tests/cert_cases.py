"""Rounds that pin the zero-score certificates ("Certificate thresholds"), for
test_cert_cases.py (CPU: the reference's answer depends on the clause) and test_gpu_zero_certs.py
(every engine path equals the reference).

A cost_aware host scores exactly 0 only in a zero-cost zone of the anchor or as an exact fit; the
fast paths skip scoring where a short list of thresholds (the certificates) proves that, and hand
over to the exact path otherwise. Each case here is a round of 2000 hosts in which one clause
alone decides a placement.

The skeleton. ``synthetic.make_round(mode, 2000, nA + nB, seed=1)`` regrouped into group B (anchor
zone 3, zero-cost component {3, 4, 5}; processed first) and group A (anchor zone 0, component
{0, 1, 2}): two chains, so the epoch takes the frontier walk. Every host holds (16, 131072, 100, 1),
every task demands (1, 2048, 0, 0), and the hosts of zones 0-2 below index 40 have no cpus. A's
first zero-cost fitting host is then host 40 and B's is host 3; with nothing planted the reference
gives [3, 3, 40, 40, ...]. Host 4 (zone 4: foreign to A, lower index than 40) is the planted host.

``NAMES`` lists the cases; ``build(name)`` returns ``(round, Expect)`` and ``reference(name)`` adds
the CPU oracle's result (computed once per case and shared; callers must not modify it).
"""
import collections
import functools
import os
import re

import numpy as np

from oracle import oracle
from pivot_place import _abi, synthetic

BF, FF = _abi.PVT_CA_BF, _abi.PVT_CA_FF
H = 2000
A_ZONE, B_ZONE = 0, 3
A_HOST, B_HOST = 40, 3                         # the groups' first zero-cost fitting hosts
PLANTED = 4
CAP = (16.0, 131072.0, 100.0, 1.0)
ROW = (1.0, 2048.0, 0.0, 0.0)
TINY = 5e-324                                   # the smallest subnormal


def p2(e):
    return float(np.ldexp(1.0, e))


# kind: what the reference does. "handover": it puts A's first task on the planted host, whose score
#       (first-fit: key) is 0 outside the anchor's zero-cost zones, so a path that skipped scoring
#       there would be wrong; "proven": it ignores the planted host, whose score is positive with
#       the clauses at their limits; "bound": certificate 3 / 3', equality only
# (walk and tail say which code must decide on the frontier paths)
# a0: the first task of A, in processing order, that some host fits; a0_host: where the reference must put it
# unplaced: tasks the reference cannot place
# tail: "none" (the epoch is accepted from the chains' words), "runs" (both chains complete and the
#       tail kernels decide), None (nothing pinned)
# walk: "both" (the frontier walk proves both chains), "left" (it leaves A's chain to the exact
#       path), "left_all" (the failing clause is read by both chains -- the separation is taken over
#       all hosts -- so the next epoch walks two chains with lists)
Expect = collections.namedtuple("Expect", "kind mode a0 a0_host unplaced tail walk")


def _regroup(r, anchors):
    """Tasks grouped by the given per-task anchors (first-seen group order)."""
    first = {}
    for a in anchors:
        first.setdefault(int(a), len(first))
    r.task_group = np.array([first[int(a)] for a in anchors], dtype=np.int32)
    r.group_anchor = np.array(list(first.keys()), dtype=np.int32)
    return r


def skeleton(mode, nA, nB, nC=0):
    """nC > 0: a third group C anchored in zone 1, the last one; it joins A's chain."""
    r = synthetic.make_round(mode, H, nA + nB + nC, seed=1)
    _regroup(r, [B_ZONE] * nB + [A_ZONE] * nA + [1] * nC)
    r.cost = np.array(r.cost, dtype=np.float64)
    r.bw = np.array(r.bw, dtype=np.float64)
    for d in range(4):
        r.avail[d, :] = CAP[d]
        r.dem[d, :] = ROW[d]
    r.avail[0, (r.zone < 3) & (np.arange(H) < A_HOST)] = 0.0
    return r


def _pair(r, c=None, bw=None, z=PLANTED):
    """The tables between anchor zone 0 and zone z: c = (cost[0, z], cost[z, 0]), bw likewise."""
    if c is not None:
        r.cost[A_ZONE, z], r.cost[z, A_ZONE] = c
    if bw is not None:
        r.bw[A_ZONE, z], r.bw[z, A_ZONE] = bw


def _host(r, h, cap):
    r.avail[:, h] = cap


def _exp(kind, mode, a0, host, unplaced=(), tail=None, walk=None):
    if walk is None:
        walk = "both" if kind == "proven" or tail == "runs" else "left"
    return Expect(kind, mode, a0, host, tuple(unplaced), tail, walk)


# ---- best-fit: hand-over cases (nA = 6, nB = 2) ------------------------------------------------
def c_subnormal():
    """c = 5e-324 and a residual of 0.25 in disk alone: c * r underflows to 0. bw is the table's and
    disk separates hosts from tasks (0.25 >= 2^-288): `c >= 2^-300` alone fails."""
    r = skeleton(BF, 6, 2)
    _pair(r, c=(TINY, 0.0))
    _host(r, PLANTED, (1.0, 2048.0, 0.25, 0.0))
    return r, _exp("handover", BF, 2, PLANTED)


def c_at_limits():
    """c = 2^-500 with bw = 2^300 and the separation 2^-288 exactly at their limits: the score
    2^-788 / 2^300 underflows. `c` alone fails."""
    r = skeleton(BF, 6, 2)
    _pair(r, c=(p2(-500), 0.0), bw=(p2(299), p2(299)))
    _host(r, PLANTED, (1.0, 2048.0, p2(-288), 0.0))
    return r, _exp("handover", BF, 2, PLANTED)


def bw_huge():
    """bw = 2^1023: the table's cost times a residual of 2^-60, divided by it, underflows.
    `bw <= 2^300` alone fails."""
    r = skeleton(BF, 6, 2)
    _pair(r, bw=(p2(1023), 0.0))
    _host(r, PLANTED, (1.0, 2048.0, p2(-60), 0.0))
    return r, _exp("handover", BF, 2, PLANTED)


def sep_fails():
    """c = 2^-300 and bw = 2^300 at their limits, a residual of 2^-500: no dimension separates hosts
    from tasks by 2^-288. The separation alone fails."""
    r = skeleton(BF, 6, 2)
    _pair(r, c=(p2(-301), p2(-301)), bw=(p2(299), p2(299)))
    _host(r, PLANTED, (1.0, 2048.0, p2(-500), 0.0))
    return r, _exp("handover", BF, 2, PLANTED, walk="left_all")


def _in_window(c02, cap, nC=0):
    r = skeleton(BF, 6, 2, nC)
    _pair(r, c=(c02, 0.0), z=2)                 # zone 2 stays in A's component through zone 1
    assert r.cost[1, 2] + r.cost[2, 1] == 0.0 and r.cost[0, 1] + r.cost[1, 0] == 0.0
    _host(r, 2, cap)
    return r


def in_window_underflow():
    """Zone 2 stays in anchor 0's zero-cost component (through zone 1) but costs c = 5e-324 from
    zone 0; host 2's exact score underflows to 0 and it must be taken as a zero (the underflow twin
    of a non-transitive zero-cost table). With these two groups the chain's zones are anchor 0's
    own, {0, 1}, so host 2 lies outside the window and the `c` clause fails; its row leaves no
    dimension separated either (memory 2048 - 2048, disk and gpus 0). The exact path decides."""
    return _in_window(TINY, (1.25, 2048.0, 0.0, 0.0)), _exp("handover", BF, 2, 2, walk="left_all")


def in_window_underflow_walked():
    """The same where the walk itself must pick host 2. A third group anchored in zone 1 joins A's
    chain, so the chain's zones are {0, 1, 2} and host 2 is a window host outside anchor 0's
    zero-cost zones, scored exactly; host 2 keeps 0.25 of disk (the norm of the residual
    (0.25, 0, 0.25, 0) is below 0.5, so 5e-324 times it still rounds to 0), so disk separates and
    every certificate holds."""
    return (_in_window(TINY, (1.25, 2048.0, 0.25, 0.0), nC=2),
            _exp("handover", BF, 2, 2, tail="none", walk="both"))


def verdict_mixed_dims():
    """B demands disk, A demands gpus; B's three commits leave host 3 at exactly A's row, an exact
    fit (score 0) for A's first task. Both walks complete, each chain has an undemanded dimension
    with a host minimum >= 2^-287, but no dimension is undemanded by both: only the AND across the
    chains' certificate words sends the epoch to the tail kernels."""
    nA, nB = 4, 3
    r = skeleton(BF, nA, nB)
    r.dem[:, :nB] = np.array([[1.0], [2048.0], [2.0], [0.0]])
    r.dem[:, nB:] = np.array([[1.0], [2048.0], [0.0], [0.25]])
    _host(r, B_HOST, (4.0, 8192.0, 6.0, 0.25))
    return r, _exp("handover", BF, nB, B_HOST, tail="runs")


# ---- best-fit: proven cases --------------------------------------------------------------------
def all_at_limits():
    """c = 2^-300, bw = 2^300, separation 2^-288: every clause of certificate 2 exactly at its
    limit, score 2^-888 > 0."""
    r = skeleton(BF, 6, 2)
    _pair(r, c=(p2(-301), p2(-301)), bw=(p2(299), p2(299)))
    _host(r, PLANTED, (1.0, 2048.0, p2(-288), 0.0))
    return r, _exp("proven", BF, 2, A_HOST)


def nontransitive_positive():
    """in_window_underflow with c = 0.03: host 2's exact score is positive. (No dimension is
    separated, as there: the exact path decides.)"""
    return _in_window(0.03, (1.25, 2048.0, 0.0, 0.0)), _exp("proven", BF, 2, A_HOST, walk="left_all")


def nontransitive_positive_walked():
    """in_window_underflow_walked with c = 0.03: every certificate holds and the walk scores the
    window host 2 exactly, > 0."""
    return (_in_window(0.03, (1.25, 2048.0, 0.25, 0.0), nC=2),
            _exp("proven", BF, 2, A_HOST, tail="none"))


def _verdict_min(e):
    """Disk holds 2^e on every host and gpus 0: both are undemanded by both chains, and with a
    gpu on every host the verdict would rest on gpus whatever disk holds."""
    r = skeleton(BF, 6, 2)
    r.avail[2, :] = p2(e)                       # disk: undemanded by both chains
    r.avail[3, :] = 0.0                         # gpus: undemanded too, so its minimum must not vouch
    return r


def verdict_min_at_limit():
    """The only dimension undemanded by both chains with a positive minimum holds exactly 2^-287."""
    return _verdict_min(-287), _exp("proven", BF, 2, A_HOST, tail="none")


def verdict_min_below():
    """2^-288: the walk's separation holds (memory) but the host's verdict must not accept."""
    return _verdict_min(-288), _exp("proven", BF, 2, A_HOST, tail="runs")


# ---- best-fit: bound cases (certificate 3) -----------------------------------------------------
def window_cap_2p501():
    r = skeleton(BF, 6, 2)
    _host(r, A_HOST, (p2(501),) + CAP[1:])
    return r, _exp("bound", BF, 2, A_HOST)


def window_cap_nan():
    """A NaN capacity fits nothing: the reference skips host 40 for host 41."""
    r = skeleton(BF, 6, 2)
    r.avail[2, A_HOST] = np.nan
    return r, _exp("bound", BF, 2, A_HOST + 1)


def dem_2p501():
    """One task of A demands 2^501 cpus: it is sorted to the front of its group and nothing fits it."""
    r = skeleton(BF, 6, 2)
    r.dem[0, 5] = p2(501)
    return r, _exp("bound", BF, 2, A_HOST, unplaced=(5,))


# ---- first-fit (sort_hosts; nA = nB = n >= the keyed walk's minimum group) ---------------------
def _ff_cap(n, e):
    r = skeleton(FF, n, n)
    _pair(r, c=(p2(-301), p2(-301)), bw=(p2(299), p2(299)))
    _host(r, PLANTED, (p2(e),) * 4)
    return r


def ff_cap_2p500(n):
    """Host 4 holds 2^500 in every dimension: its norm is 2^501 and its key for A,
    2^-300 / (2^501 * 2^300), underflows to 0, so it leads A's host order. `capacity <= 2^298`."""
    return _ff_cap(n, 500), _exp("handover", FF, n, PLANTED)


def ff_cap_inside(n):
    """2^297: norm 2^298, key 2^-898 > 0. Clause (2') exactly at its limits."""
    return _ff_cap(n, 297), _exp("proven", FF, n, A_HOST)


def ff_negative_demand(n):
    """One task of A demands -1 of disk (clause 3'); every host norm is > 0, so no key is 0 / 0."""
    r = skeleton(FF, n, n)
    r.dem[2, n + 7] = -1.0
    return r, _exp("bound", FF, n + 7, A_HOST)


BF_CASES = collections.OrderedDict((f.__name__, f) for f in (
    c_subnormal, c_at_limits, bw_huge, sep_fails, in_window_underflow, in_window_underflow_walked,
    verdict_mixed_dims, all_at_limits, nontransitive_positive, nontransitive_positive_walked,
    verdict_min_at_limit,
    verdict_min_below, window_cap_2p501, window_cap_nan, dem_2p501))
FF_CASES = collections.OrderedDict((f.__name__, f) for f in (
    ff_cap_2p500, ff_cap_inside, ff_negative_demand))
NAMES = list(BF_CASES) + list(FF_CASES)


def keyed_frontier_min():
    """KEYED_FRONTIER_MIN of csrc/pvt_driver.h: the group size from which first-fit groups take the
    keyed and chain walks."""
    path = os.path.join(os.path.dirname(os.path.abspath(synthetic.__file__)), "..", "csrc", "pvt_driver.h")
    with open(path) as f:
        m = re.search(r"constexpr\s+int\s+KEYED_FRONTIER_MIN\s*=\s*(\d+)\s*;", f.read())
    assert m, "KEYED_FRONTIER_MIN not found in %s" % path
    return int(m.group(1))


def build(name):
    """(round, Expect) of the named case; both groups of a first-fit case hold two tasks more than
    the keyed walk's minimum."""
    if name in BF_CASES:
        return BF_CASES[name]()
    return FF_CASES[name](keyed_frontier_min() + 2)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(round, Expect, oracle result) of the named case."""
    r, e = build(name)
    return r, e, oracle.place(r)
