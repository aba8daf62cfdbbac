"""GPU tests of the frontier walk's fast prologue (PVT_CHAIN_CERT): in the round's
first cost_aware best-fit epoch the walk takes its chain's extremes, bound flag and batch minima
from the group certificates the order launch wrote and its window straight from the prebuilt one,
without a pass over the chain's demand rows; a missed optimistic apply is undone from that window.
Every case equals the CPU restatement bit for bit and an engine created under PVT_CHAIN_CERT=0;
launch counts come from the named profiling scopes, fast-prologue chains from
``prologue_stats``."""
import functools

import numpy as np
import pytest

from oracle import oracle
from pivot_place import _abi, synthetic

from test_gpu_epoch_tail import TAIL, UNDO, _engine_under, _regroup, _round as _tail_round, _same

pytestmark = pytest.mark.gpu

RAGGED = (63, 65, 129, 191, 1, 64)
RAGGED_ANCHORS = (0, 3, 1, 4, 2, 5)             # alternately the components {0, 1, 2} and {3, 4, 5}


@pytest.fixture(scope="module")
def engine_cert0():
    eng = _engine_under(PVT_CHAIN_CERT="0")
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def engine_plan0():
    eng = _engine_under(PVT_EPOCH_PLAN="0")
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def engine_plan0_cert0():
    eng = _engine_under(PVT_EPOCH_PLAN="0", PVT_CHAIN_CERT="0")
    yield eng
    eng.close()


def _sized(sizes, seed):
    """20 000 hosts and sum(sizes) tasks in six contiguous groups of the given sizes."""
    r = synthetic.make_round(_abi.PVT_CA_BF, 20_000, int(sum(sizes)), seed=seed)
    return _regroup(r, np.repeat(np.array(RAGGED_ANCHORS), sizes))


def _round(name):
    if name == "ragged":                        # 2: segment starts off the 64-task grid
        return _sized(RAGGED, 21)
    if name == "ragged_permuted":
        return _sized((64, 1, 191, 129, 65, 63), 21)
    if name == "signed_zeros":                  # 3
        r = _tail_round("proven")
        odd = (np.arange(r.n_tasks) % 2) == 1
        r.dem[2:, :] = 0.0
        r.dem[2:, odd] = -0.0
        return r
    if name == "bound_exceeded":                # 5
        r = _tail_round("proven")
        r.dem[0, 17] = float.fromhex("0x1p501")
        return r
    if name == "whole_then_later":              # 7
        # the first epoch holds whole groups only: the component {0, 1, 2} fills its chain exactly
        # (1024 + 1024 = CHAIN_MAX tasks), so the epoch ends before that component's third group
        # and the second epoch (tasks from 3648 on) takes the other prologue. (The epoch-tail
        # file's two_epochs cuts its fifth group, so no epoch of it is eligible.)
        return _sized((1024, 800, 1024, 800, 500, 500), 12)
    return _tail_round(name)


@functools.lru_cache(maxsize=None)
def _case(name):
    """The round and its CPU reference, computed once and left unchanged."""
    r = _round(name)
    return r, oracle.place(r, threads=4)


def _n_components(r):
    """Zero-cost components that hold a group anchor: the first epoch's chains."""
    c = np.asarray(r.cost, dtype=np.float64)
    z0 = (c + c.T) == 0.0
    Z = z0.shape[0]
    root = list(range(Z))

    def find(z):
        while root[z] != z:
            z = root[z]
        return z
    for a in range(Z):
        for z in range(Z):
            if z0[a, z]:
                root[find(a)] = find(z)
    return len({find(int(a)) for a in r.group_anchor})


def _place(eng, r):
    """Result, epoch statistics, launches per named kernel, fast-prologue chains."""
    try:
        eng.set_resident(0)
        eng.set_profiling(2)
        eng.reset_kstats()
        res = eng.place(r)
        st = eng.epoch_stats()
        fast = eng.prologue_stats()["fast_chains"]
        n = {k: eng.kernel_kstats(k)["launches"] for k in TAIL + (UNDO, "zwalk_kernel")}
    finally:
        eng.set_profiling(False)
        eng.set_resident(_abi.PVT_RESIDENT_MAX_HOSTS)
    print(st, n, fast)
    return res, st, n, fast


def _check(eng, eng0, name):
    """Parity with the oracle on the engine under test and on the PVT_CHAIN_CERT=0 engine, which
    never takes the fast prologue; both plan the same epochs and launch the same kernels."""
    r, ref = _case(name)
    res, st, n, fast = _place(eng, r)
    _same(res, ref)
    res0, st0, n0, fast0 = _place(eng0, r)
    _same(res0, ref)
    assert fast0 == 0, fast0
    assert st == st0, (st, st0)
    assert n == n0, (n, n0)
    return st, n, fast


def test_proven_epoch(engine, engine_cert0):
    st, n, fast = _check(engine, engine_cert0, "proven")
    assert st["frontier_chains"] > 0 and st["list_chains"] == 0, st
    assert fast == st["frontier_chains"], (fast, st)
    assert all(n[k] == 0 for k in TAIL) and n[UNDO] == 0 and n["zwalk_kernel"] == 1, n


@pytest.mark.parametrize("name", ["ragged", "ragged_permuted"])
def test_ragged_segments(engine, engine_cert0, name):
    r, _ = _case(name)
    assert _n_components(r) == 2
    st, n, fast = _check(engine, engine_cert0, name)
    assert st["epochs"] == 1 and st["frontier_chains"] == 2 and fast == 2, (st, fast)


def test_signed_zeros(engine, engine_cert0):
    r, _ = _case("signed_zeros")
    assert np.signbit(r.dem[2:, 1::2]).all() and not np.signbit(r.dem[2:, 0::2]).any()
    st, n, fast = _check(engine, engine_cert0, "signed_zeros")
    assert all(n[k] == 0 for k in TAIL) and n[UNDO] == 0 and n["zwalk_kernel"] == 1, n
    assert fast == st["frontier_chains"] > 0, (fast, st)


@pytest.mark.parametrize("name", ["all_demanded", "chain_stops"])
def test_undo_from_the_window(engine, engine_cert0, name):
    st, n, fast = _check(engine, engine_cert0, name)
    assert n[UNDO] >= 1 and all(n[k] >= 1 for k in TAIL if k != "epoch_validate_kernel"), n
    assert fast > 0, fast


def test_bound_exceeded(engine, engine_cert0):
    r, ref = _case("bound_exceeded")
    assert ref.placement[17] == -1
    st, n, fast = _check(engine, engine_cert0, "bound_exceeded")
    assert st["list_chains"] >= 1, st
    assert fast == _n_components(r) - 1, (fast, _n_components(r))


def test_shared_component(engine_plan0, engine_plan0_cert0):
    """PVT_EPOCH_PLAN=0: a chain per anchor zone, three chains on each component's window; nothing
    is written back and the tail kernels validate every pair."""
    st, n, fast = _check(engine_plan0, engine_plan0_cert0, "ragged")
    assert fast == 6, (st, fast)
    assert n[UNDO] == 0 and all(n[k] >= 1 for k in TAIL), n


def test_later_epoch(engine, engine_cert0):
    st, n, fast = _check(engine, engine_cert0, "whole_then_later")
    assert st["epochs"] >= 2, st
    assert 0 < fast < st["frontier_chains"], (fast, st)


def test_first_fit(engine, engine_cert0):
    """First-fit epochs keep their prologue."""
    st, n, fast = _check(engine, engine_cert0, "ff_proven")
    assert n["zwalk_kernel"] > 0 and fast == 0, (n, fast)
