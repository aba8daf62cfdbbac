"""Rounds with long runs of one demand row ("Run lengths from the order launch"),
for test_long_run_cases.py (CPU: every case has the shape it is named for) and
test_gpu_long_runs.py (the engine equals the reference on every switch).

The frontier walk places a stretch of bit-identical demand rows inside a group by run_bulk calls of
up to ZW_RMAX tasks, from run lengths the grouped-order launch wrote, and logs it in a ring of
ZW_LOGN chain positions. The cases put such stretches where that can go wrong: lengths on and next
to 64 and 128, every start offset in a 64-task batch that matters, whole batches covered by one
call, the cap, the ring's wrap, chunks that run out of fitting hosts, a segment start inside equal
rows, four demanded dimensions, counts that differ from the quotient, a negative demand.

The skeleton. 2000 hosts (zone = index % 20), every host (16, 131072, 100, 1), cost_aware best-fit.
The chain under test holds the groups anchored in the zero-cost component {0, 1, 2}; its window is
that component's 300 hosts in index order, so chunk c is window[64 c : 64 c + 64]. A last group of
two tasks anchored in zone 3 makes a second chain, so the epoch takes the frontier walk; every
segment is a whole group, so the fast prologue is eligible. Tasks before the run in its group
("fillers") are distinct rows of larger norm, so sorted order puts them first and each is a run of
one.

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

BF = _abi.PVT_CA_BF
H = 2000
CAP = (16.0, 131072.0, 100.0, 1.0)
ROW = (1.0, 2048.0, 0.0, 0.0)                   # 16 copies a host (cpus)
SMALL = (0.5, 1024.0, 0.0, 0.0)                 # sorted after ROW: keeps a chunk alive for tasks ahead
COMPONENT = (0, 1, 2)
OTHER = 3                                       # the second chain's anchor
BIG = 1000.0

# run: tasks of the stretch under test; group: its group; offset: its first task's chain position
# & 63; fit: per window chunk from 0, the hosts that can take a copy of the row when the run starts
# (the reference's state there); chain: tasks of the chain under test; row: the stretch's row;
# counts: copies the window's first hosts take of the run, where the case pins them
Expect = collections.namedtuple("Expect", "run group offset fit chain row counts")


def walk_constant(name):
    """ZW_RMAX / ZW_LOGN of csrc/pvt_zwalk.hip."""
    path = os.path.join(os.path.dirname(os.path.abspath(synthetic.__file__)), "..", "csrc", "pvt_zwalk.hip")
    with open(path) as f:
        src = f.read()
    pat = {"ZW_RMAX": r"#define\s+PVT_ZW_RMAX\s+(\d+)", "ZW_LOGN": r"constexpr\s+int\s+ZW_LOGN\s*=\s*(\d+)\s*;"}[name]
    m = re.search(pat, src)
    assert m, "%s not found in %s" % (name, path)
    return int(m.group(1))


def _regroup(r, anchors):
    """Tasks grouped by the given per-task anchors (first-seen group order)."""
    first = {}
    for a in anchors:
        first.setdefault(int(a), len(first))
    r.task_group = np.array([first[int(a)] for a in anchors], dtype=np.int32)
    r.group_anchor = np.array(list(first.keys()), dtype=np.int32)
    return r


def skeleton(sizes, anchors):
    """Contiguous groups of the given sizes and anchors, then the two tasks of the other chain;
    every task demands ROW, every host holds CAP."""
    sizes, anchors = tuple(sizes) + (2,), tuple(anchors) + (OTHER,)
    r = synthetic.make_round(BF, H, int(sum(sizes)), seed=1)
    _regroup(r, np.repeat(np.array(anchors), sizes))
    for d in range(4):
        r.avail[d, :] = CAP[d]
        r.dem[d, :] = ROW[d]
    return r


def window(r):
    """The chain's window: the component's hosts in index order."""
    return np.nonzero(np.isin(r.zone, COMPONENT))[0]


def _fillers(r, n):
    """Tasks [0, n): distinct rows of larger norm than ROW (a run of one each, sorted first)."""
    r.dem[1, :n] = 4096.0 + np.arange(n)


def _one_run(R, o, row=ROW, tail=0):
    """One group: o fillers, R tasks of the row, then `tail` tasks of SMALL."""
    r = skeleton((o + R + tail,), (0,))
    _fillers(r, o)
    for d in range(4):
        r.dem[d, o:o + R] = row[d]
        r.dem[d, o + R:o + R + tail] = SMALL[d]
    return r


def _exp(R, o, fit, chain, row=ROW, group=0, counts=None):
    return Expect(R, group, o & 63, tuple(fit), chain, tuple(row), counts)


def _fit_after_fillers(o):
    """Fillers take 16 a host (cpus), lowest index first: o // 16 hosts of chunk 0 are full."""
    return (64 - o // 16,)


def _exact(R, o):
    def case():
        return _one_run(R, o), _exp(R, o, _fit_after_fillers(o), o + R)
    case.__name__ = "run%d_at%d" % (R, o)
    case.__doc__ = "A run of exactly %d tasks whose first is task %d of its batch." % (R, o)
    return case


EXACT = [_exact(R, o) for R in (64, 65, 128, 129, 200) for o in (0, 1, 63)]


def covers_batches():
    """200 tasks from offset 10: the first call places ZW_RMAX of them and covers the next two
    batches whole (carry >= 64 twice)."""
    return _one_run(200, 10), _exp(200, 10, (64,), 210)


def ends_on_batch_end():
    """136 tasks from offset 56 end on position 192: one call, two batches covered whole and
    nothing carried into the fourth."""
    return _one_run(136, 56), _exp(136, 56, (61,), 192)


def over_the_cap():
    """400 tasks: more than ZW_RMAX, so the cap splits the run into further calls."""
    return _one_run(400, 5), _exp(400, 5, (64,), 405)


def ring_wraps():
    """300 single tasks, then a run of 150: the chain is longer than ZW_LOGN, the ring wraps under
    single entries and again under the run."""
    return _one_run(150, 300), _exp(150, 300, (64 - 18,), 450)


def _runout(R, cpus, tail):
    r = _one_run(R, 0, tail=tail)
    r.avail[0, window(r)] = cpus
    return r


def runout_chunk_moves():
    """Hosts of 2 cpus take two copies each and nothing ahead fits a used one: chunk 0 runs out
    after 128 tasks, is dead, and the register chunk moves on."""
    return _runout(200, 2.0, 0), _exp(200, 0, (64, 64, 64), 200)


def runout_on_pb():
    """Hosts of 2.5 cpus take two copies and keep half a cpu, which the group's last tasks (SMALL)
    fit: chunk 0 stays the register chunk and the run continues on chunk pb."""
    return _runout(200, 2.5, 4), _exp(200, 0, (64, 64, 64), 204)


def runout_on_lds():
    """The same with 300 tasks: chunk 0 and chunk pb take 128 each, the rest goes to chunk 2 in LDS."""
    return _runout(300, 2.5, 4), _exp(300, 0, (64, 64, 64), 304)


def segment_inside_equal_rows():
    """Two consecutive groups of one chain (anchors 0 and 1) with the same row: the stretch of 200
    equal rows is two runs, the first ends at the segment start."""
    return skeleton((100, 100), (0, 1)), _exp(100, 0, (64,), 200)


def four_dims():
    """Every dimension demanded: gpus bind (8 copies a host)."""
    row = (1.0, 2048.0, 1.0, 0.125)
    return _one_run(150, 3, row=row), _exp(150, 3, (64,), 153, row=row)


def rounding():
    """Demand 0.1 against 2.0 and 0.05 against 1.0: repeated subtraction gives 19 copies where the
    quotient says 20 (the values tests/test_gpu_run_bulk.py pins); the third host takes the rest."""
    row = (0.1, 0.05, 0.0, 0.0)
    r = _one_run(150, 0, row=row)
    w = window(r)
    r.avail[0, w] = 0.0
    for i, c in enumerate([(2.0, BIG, 100.0, 1.0), (BIG, 1.0, 100.0, 1.0), (BIG, BIG, 100.0, 1.0)]):
        r.avail[:, w[i]] = c
    return r, _exp(150, 0, (3, 0, 0), 150, row=row, counts=(19, 19, 112))


def negative_component():
    """A negative demand (disk): every call places one task."""
    row = (1.0, 2048.0, -1.0, 0.0)
    return _one_run(70, 0, row=row), _exp(70, 0, (64,), 70, row=row)


CASES = collections.OrderedDict((f.__name__, f) for f in EXACT + [
    covers_batches, ends_on_batch_end, over_the_cap, ring_wraps, runout_chunk_moves, runout_on_pb,
    runout_on_lds, segment_inside_equal_rows, four_dims, rounding, negative_component])
NAMES = list(CASES)


def build(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def reference(name):
    """(round, Expect, oracle result) of the named case."""
    r, e = build(name)
    return r, e, oracle.place(r)
