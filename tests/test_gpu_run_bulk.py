"""GPU tests of run_bulk (pvt_zwalk.hip): a run of tasks with one demand row is
placed on a 64-host chunk by counting, per host, the copies it takes (pass 1: the subtraction chain
in blocks of ZW_UNROLL = 8 copies, a snapshot of the capacities at each block start) and by giving
each taking host its capacities after its last copy (pass 2: from the snapshot plus at most a
block's copies, or from the start for a host that takes fewer copies than its snapshot holds).

Every case sets one demand row and the capacities of the first hosts of the chain's window (all
other hosts of its zero-cost component get no cpus, so they fit nothing), so that the hosts take
known numbers of copies: counts where copy-by-copy subtraction disagrees with the quotient, counts
on and around the block edges, every shape of the last taking host, all four dimensions, runs over
a batch end and across a segment start, and the other instances of the kernel (first-fit keyed,
ordered, a second epoch). The expected counts are checked on the CPU reference first; the engine
must then equal it bit for bit on placement, order and final availability with every chain on the
frontier walk. 20 000 hosts, at most a few hundred tasks (the second epoch apart)."""
import functools

import numpy as np
import pytest

from oracle import oracle
from pivot_place import _abi, synthetic

from test_gpu_epoch_tail import _engine_under, _round as _tail_round, _same, _zero_sets
from test_gpu_walk_pipe import H, ROW, _grouped, _place

pytestmark = pytest.mark.gpu

BIG = 1000.0                                    # a capacity no case exhausts
MEM = 2048.0 * 512                              # ROW's memory for 512 copies (exact)


@pytest.fixture(scope="module")
def engine_tail0():
    eng = _engine_under(PVT_EPOCH_TAIL="0")
    yield eng
    eng.close()


def _window(r, anchor):
    """The hosts of the anchor's zero-cost component, in index order: its chain's window."""
    return np.nonzero(np.isin(r.zone, sorted(_zero_sets(r)[anchor])))[0]


def _cpus(*counts):
    """Hosts that take the given numbers of ROW (1 cpu, 2048 MiB; best-fit: fit >=); None: a host
    that fits nothing."""
    return [None if c is None else (float(c), MEM, 100.0, 1.0) for c in counts]


def _bulk(mode, sizes, anchors, row, caps, seed):
    """Groups of the given sizes and anchors, every task with the demand row; the first hosts of
    anchor 0's window get the capacities caps, the component's other hosts no cpus."""
    r = _grouped(mode, sizes, anchors, seed)
    for d in range(4):
        r.dem[d, :] = row[d]
    w = _window(r, 0)
    r.avail[0, w] = 0.0
    for i, c in enumerate(caps):
        if c is not None:
            r.avail[:, w[i]] = c
    return r


# name -> (mode, group sizes, anchors, row, capacities of the window's first hosts, copies expected
# on them). The last group (two tasks, another component) makes the epoch a frontier epoch.
BF, FF = _abi.PVT_CA_BF, _abi.PVT_CA_FF
CASES = {
    # sequential rounding against floor(c / d): 2.0 / 0.1 -> 19 (20), 1.0 / 0.05 -> 19 (20),
    # 3.0 / 0.6 -> 4 (5), 3.0 / 0.2 -> 14 (15); the third host takes the rest (a partial lane)
    "rounding_two_a": (BF, (43, 2), (0, 3), (0.1, 0.05, 0.0, 0.0),
                       [(2.0, BIG, 100.0, 1.0), (BIG, 1.0, 100.0, 1.0), (BIG, BIG, 100.0, 1.0)], (19, 19, 5)),
    "rounding_two_b": (BF, (21, 2), (0, 3), (0.6, 0.2, 0.0, 0.0),
                       [(3.0, BIG, 100.0, 1.0), (BIG, 3.0, 100.0, 1.0), (BIG, BIG, 100.0, 1.0)], (4, 14, 3)),
    "rounding_four": (BF, (60, 2), (0, 3), (0.1, 0.05, 0.6, 0.2),
                      [(2.0, BIG, BIG, BIG), (BIG, 1.0, BIG, BIG), (BIG, BIG, 3.0, BIG), (BIG, BIG, BIG, 3.0),
                       (BIG, BIG, BIG, BIG)], (19, 19, 4, 14, 4)),
    # block edges of the unroll: 7, 8, 9, 15, 16, 17 and 24 copies; the run ends on the last
    # host's last copy (96 tasks: over a batch end too)
    "edges_all": (BF, (96, 2), (0, 3), ROW, _cpus(7, 8, 9, 15, 16, 17, 24), (7, 8, 9, 15, 16, 17, 24)),
    "edges_stop_on_block_end": (BF, (24, 2), (0, 3), ROW, _cpus(8, 16, 30), (8, 16, 0)),
    "edges_stop_in_block": (BF, (21, 2), (0, 3), ROW, _cpus(9, 24), (9, 12)),
    "edges_stop_after_block": (BF, (26, 2), (0, 3), ROW, _cpus(9, 24), (9, 17)),
    # shapes of the last taking lane
    "last_exact": (BF, (11, 2), (0, 3), ROW, _cpus(5, 6, 9), (5, 6, 0)),
    "last_one": (BF, (6, 2), (0, 3), ROW, _cpus(5, 6), (5, 1)),
    "last_all_but_one": (BF, (10, 2), (0, 3), ROW, _cpus(5, 6), (5, 5)),
    "single_host_partial": (BF, (30, 2), (0, 3), ROW, _cpus(40), (30,)),
    "single_host_exact": (BF, (40, 2), (0, 3), ROW, _cpus(40, 3), (40, 0)),
    "three_hosts_gap": (BF, (17, 2), (0, 3), ROW, _cpus(3, None, 4, None, None, 20), (3, 0, 4, 0, 0, 10)),
    # all four dimensions demanded: disk stops the first host (5 of 30 cpus used), gpus the second
    # (4), memory the third (6); the fourth takes part of its count
    "four_dims": (BF, (18, 2), (0, 3), (1.0, 2048.0, 1.0, 0.125),
                  [(30.0, MEM, 5.0, 1.0), (10.0, MEM, 100.0, 0.5), (20.0, 2048.0 * 6, 100.0, 1.0),
                   (20.0, MEM, 100.0, 1.0)], (5, 4, 6, 3)),
    # a run over a batch end: entries past position 63
    "carry_63": (BF, (63, 2), (0, 3), ROW, _cpus(60, 10), (60, 3)),
    "carry_64": (BF, (64, 2), (0, 3), ROW, _cpus(60, 10), (60, 4)),
    "carry_65": (BF, (65, 2), (0, 3), ROW, _cpus(60, 10), (60, 5)),
    "carry_100": (BF, (100, 2), (0, 3), ROW, _cpus(70, 40), (70, 30)),
    # a run cut by a segment start at task 40 (anchor 1 is of anchor 0's component): the second
    # host ends the first part and takes the whole second part
    "segment_cut": (BF, (40, 50, 2), (0, 1, 3), ROW, _cpus(30, 100), (30, 60)),
    "segment_cut_exact": (BF, (40, 50, 2), (0, 1, 3), ROW, _cpus(40, 100), (40, 50)),
    # cost_aware first-fit, the keyed instance: strict fit, a host left at exactly 0 does not count
    # (5 cpus: 4 copies; memory strict too); a group takes the keyed walk from 32 tasks on
    "ff_strict_exact": (FF, (38, 2), (0, 3), ROW, _cpus(5, 6, 30, 9), (4, 5, 29, 0)),
    "ff_strict_partial": (FF, (34, 2), (0, 3), ROW, _cpus(9, 17, 25), (8, 16, 10)),
    "ff_strict_memory": (FF, (33, 2), (0, 3), ROW,
                         [(40.0, 2048.0 * 8, 100.0, 1.0), (40.0, MEM, 100.0, 1.0)], (7, 26)),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """The round, its CPU reference (computed once, left unchanged) and the window's first hosts."""
    mode, sizes, anchors, row, caps, counts = CASES[name]
    r = _bulk(mode, sizes, anchors, row, caps, seed=100 + sorted(CASES).index(name))
    ref = oracle.place(r, threads=4)
    assert (ref.placement >= 0).all(), "the reference must place every task of %s" % name
    w = _window(r, 0)[:len(counts)]
    chain = ref.placement[:sum(sizes[:-1])]
    got = tuple(int((chain == h).sum()) for h in w)
    assert got == tuple(counts), "%s: the reference puts %s copies on the window's first hosts" % (name, got)
    return r, ref


def _proven(eng, name):
    r, ref = _case(name)
    res, st, n = _place(eng, r)
    _same(res, ref)
    assert n["zwalk_kernel"] > 0 and st["frontier_chains"] > 0 and st["list_chains"] == 0, (st, n)
    return st


@pytest.mark.parametrize("name", sorted(CASES))
def test_run(engine, name):
    _proven(engine, name)


@pytest.mark.parametrize("name", ["carry_100", "three_hosts_gap"])
def test_run_log_consumers(engine_tail0, name):
    """PVT_EPOCH_TAIL=0: the tail kernels rebuild the availability from the log alone, so a wrong
    entry of the batch log shows."""
    _proven(engine_tail0, name)


def test_ordered_walk(engine):
    """vbp first-fit (fit >=, index order over all hosts): the ordered instance of the walk."""
    counts = (7, 9, None, 30)                   # (the ordered walk starts from 32 tasks on)
    r = synthetic.make_round(_abi.PVT_VBP_FF, H, 40, seed=140)
    for d in range(4):
        r.dem[d, :] = ROW[d]
    r.avail[0, :] = 0.0
    for h, c in enumerate(_cpus(*counts)):
        if c is not None:
            r.avail[:, h] = c
    ref = oracle.place(r, threads=4)
    assert [int((ref.placement == h).sum()) for h in range(4)] == [7, 9, 0, 24]
    try:
        engine.set_resident(0)
        res = engine.place(r)
        st = engine.epoch_stats()
    finally:
        engine.set_resident(_abi.PVT_RESIDENT_MAX_HOSTS)
    _same(res, ref)
    assert st["frontier_chains"] > 0 and st["list_chains"] == 0, st


@functools.lru_cache(maxsize=None)
def _two_epochs():
    """The epoch-tail file's two_epochs (chains longer than CHAIN_MAX: the second epoch's walk takes
    the default prologue) with four demand rows that no capacity is a multiple of, in long runs."""
    r = _tail_round("two_epochs")
    k = np.arange(r.n_tasks) % 4
    r.dem[0, :] = np.array([0.1, 0.3, 0.6, 1.1])[k]
    r.dem[1, :] = np.array([100.1, 2048.0, 333.3, 1000.7])[k]
    return r, oracle.place(r, threads=4)


def test_second_epoch(engine):
    r, ref = _two_epochs()
    assert (ref.placement >= 0).all()
    res, st, n = _place(engine, r)
    _same(res, ref)
    assert st["epochs"] >= 2 and st["frontier_chains"] > 0 and st["list_chains"] == 0, st
