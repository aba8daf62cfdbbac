"""GPU tests of the frontier walk's log flush: the walk stores a batch's log --
the WinRec rows and the placement scatter -- at the head of the next batch and the last batch's
after its loop, from the batch buffer in LDS whose entries past 64 (a run carried over a batch end)
move down only after that store. The cases put batch ends, run ends, segment starts and chunk moves
where that order matters, at the smallest sizes that reach the code: 20 000 hosts, at most ~700
tasks (the two existing rounds of the epoch-tail file apart). Every case equals the CPU restatement
bit for bit, on the default engine and on one created under PVT_EPOCH_TAIL=0, whose tail kernels
rebuild the availability from the log alone, so that a wrong or missing WinRec row shows."""
import functools

import numpy as np
import pytest

from oracle import oracle
from pivot_place import _abi, synthetic

from test_gpu_epoch_tail import TAIL, UNDO, _engine_under, _regroup, _round as _tail_round, _same

pytestmark = pytest.mark.gpu

H = 20_000
RAGGED = (1, 63, 64, 65, 129)
RAGGED_ANCHORS = (0, 3, 6, 8, 11)               # one zone of five zero-cost components: a chain each
ROW = (1.0, 2048.0, 0.0, 0.0)                   # the single demand row of the run cases


@pytest.fixture(scope="module")
def engine_tail0():
    eng = _engine_under(PVT_EPOCH_TAIL="0")
    yield eng
    eng.close()


def _grouped(mode, sizes, anchors, seed):
    """20 000 hosts and sum(sizes) tasks in contiguous groups of the given sizes and anchors."""
    r = synthetic.make_round(mode, H, int(sum(sizes)), seed=seed)
    return _regroup(r, np.repeat(np.array(anchors), sizes))


def _one_row(r):
    for d in range(4):
        r.dem[d, :] = ROW[d]
    return r


def _round(name, mode=_abi.PVT_CA_BF):
    ff = mode == _abi.PVT_CA_FF
    if name == "ragged":                        # 1: chains of 1, 63, 64, 65 and 129 tasks
        return _grouped(mode, RAGGED, RAGGED_ANCHORS, 31)
    # (an epoch is walked on the frontier from two chains on: the one-component cases carry a
    # further group of two tasks in another component, a chain of its own)
    if name == "long_run":                      # 2: one run over three batch ends
        return _one_row(_grouped(mode, (200, 2), (0, 3), 32))
    if name == "segment_in_batch":              # 3: one row, a segment start at task 40 of a chain of 90
        return _one_row(_grouped(mode, (40, 50, 2), (0, 1, 3), 33))
    if name == "distinct_rows":                 # 4: no two tasks alike
        r = _grouped(mode, (128, 2), (0, 3), 34)
        r.dem[0, :] = 0.5
        r.dem[1, :] = 1024.0 + np.arange(130)
        return r
    if name == "one_copy_hosts":                # 5: a 150-task run, every host takes one copy
        r = _one_row(_grouped(mode, (150, 2), (0, 3), 35))
        r.avail[0, :] = ROW[0] + (0.5 if ff else 0.0)   # (first-fit: strict fit)
        r.avail[1, :] = np.maximum(r.avail[1], 4096.0)
        return r
    if name == "bound_exceeded":                # 7b: a certificate fails before the first task
        r = _tail_round("proven")
        r.dem[0, 17] = float.fromhex("0x1p501")
        return r
    return _tail_round(name)


@functools.lru_cache(maxsize=None)
def _case(name, mode=_abi.PVT_CA_BF):
    """The round and its CPU reference, computed once and left unchanged."""
    r = _round(name, mode)
    return r, oracle.place(r, threads=4)


def _place(eng, r):
    """The round on the windowed engine: result, epoch statistics, launches per named kernel."""
    try:
        eng.set_resident(0)
        eng.set_profiling(2)
        eng.reset_kstats()
        res = eng.place(r)
        st = eng.epoch_stats()
        n = {k: eng.kernel_kstats(k)["launches"] for k in TAIL + (UNDO, "zwalk_kernel")}
    finally:
        eng.set_profiling(False)
        eng.set_resident(_abi.PVT_RESIDENT_MAX_HOSTS)
    print(st, n)
    return res, st, n


def _proven(eng, name, mode=_abi.PVT_CA_BF):
    """A case the walk proves whole: the oracle alone places every task; the engine equals it with
    every chain on the frontier walk and none on the list walk."""
    r, ref = _case(name, mode)
    assert (ref.placement >= 0).all(), "the reference must place every task of %s" % name
    res, st, n = _place(eng, r)
    _same(res, ref)
    assert n["zwalk_kernel"] > 0 and st["frontier_chains"] > 0 and st["list_chains"] == 0, (st, n)
    return r, st, n


def test_ragged_chains(engine):
    r, st, n = _proven(engine, "ragged")
    assert st["epochs"] == 1 and st["frontier_chains"] == len(RAGGED), st
    assert all(n[k] == 0 for k in TAIL) and n[UNDO] == 0, n


def test_run_across_batch_ends(engine):
    r, st, n = _proven(engine, "long_run")
    assert (r.dem == r.dem[:, :1]).all()


def test_run_stops_at_segment_start(engine):
    r, st, n = _proven(engine, "segment_in_batch")
    assert st["segments"] == 3 and st["frontier_chains"] == 2, st


def test_singles_only(engine):
    r, st, n = _proven(engine, "distinct_rows")
    assert len({tuple(c) for c in r.dem.T}) == r.n_tasks


def test_run_over_lds_chunks(engine):
    r, st, n = _proven(engine, "one_copy_hosts")
    _, ref = _case("one_copy_hosts")
    assert np.unique(ref.placement).size == r.n_tasks          # a host per task: three chunks


@pytest.mark.parametrize("name", ["long_run", "segment_in_batch", "one_copy_hosts"])
def test_log_consumers(engine_tail0, name):
    """PVT_EPOCH_TAIL=0: the tail kernels rebuild the availability from the log."""
    r, st, n = _proven(engine_tail0, name)
    assert n[UNDO] == 0 and n["epoch_final_kernel"] >= 1 and n["epoch_accept_apply_kernel"] >= 1, n


@pytest.mark.parametrize("tail", ["default", "tail0"])
def test_miss_after_proven_prefix(engine, engine_tail0, tail):
    """Chains that stop after a proven prefix: their partial last batch is flushed after the loop
    and the tail kernels and the list walk go on from that log."""
    r, ref = _case("chain_stops")
    res, st, n = _place(engine if tail == "default" else engine_tail0, r)
    _same(res, ref)
    assert st["frontier_chains"] > 0 and st["list_chains"] > 0, st
    assert n["epoch_accept_apply_kernel"] >= 1, n


@pytest.mark.parametrize("tail", ["default", "tail0"])
def test_certificate_fails_before_first_task(engine, engine_tail0, tail):
    """A demand beyond the certificates' bound: that chain's walk ends before its loop with
    nothing logged; the other chains are walked as ever."""
    r, ref = _case("bound_exceeded")
    assert ref.placement[17] == -1
    res, st, n = _place(engine if tail == "default" else engine_tail0, r)
    _same(res, ref)
    assert st["frontier_chains"] > 0 and st["list_chains"] >= 1, st


@pytest.mark.parametrize("name", ["ragged", "long_run", "one_copy_hosts"])
def test_first_fit(engine, engine_tail0, name):
    """The FF instance of the walk on rounds 1, 2 and 5 (strict fit)."""
    r, st, n = _proven(engine, name, _abi.PVT_CA_FF)
    _, ref = _case(name, _abi.PVT_CA_FF)
    res0, st0, n0 = _place(engine_tail0, r)
    _same(res0, ref)
    assert st0["frontier_chains"] == st["frontier_chains"], (st, st0)


def test_two_epochs(engine, engine_tail0):
    """The epoch-tail file's two_epochs: the second epoch's walk takes the default prologue."""
    r, ref = _case("two_epochs")
    res, st, n = _place(engine, r)
    _same(res, ref)
    assert st["epochs"] >= 2 and st["frontier_chains"] > 0 and st["list_chains"] == 0, st
    res0, st0, n0 = _place(engine_tail0, r)
    _same(res0, ref)
