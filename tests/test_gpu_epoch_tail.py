"""GPU tests of the epoch tail: a frontier-walked epoch whose chains all walk
to their end is applied by the chains themselves and accepted by the host from the chains' own
words, with no launch after the walk; any other epoch undoes the write-backs
(epoch_undo_kernel) and runs the tail kernels (epoch_final_kernel, epoch_validate_kernel,
epoch_accept_apply_kernel) as before. Every case equals the CPU restatement bit for bit and an
engine created under PVT_EPOCH_TAIL=0; launch counts come from the named profiling scopes."""
import functools
import os

import numpy as np
import pytest

from oracle import oracle
from pivot_place import _abi, synthetic
from pivot_place.engine import DeviceRound, PlacementEngine

pytestmark = pytest.mark.gpu

TAIL = ("epoch_final_kernel", "epoch_validate_kernel", "epoch_accept_apply_kernel")
UNDO = "epoch_undo_kernel"


def _engine_under(**env):
    """An engine whose context read the given PVT_* switches at creation."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return PlacementEngine(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def engine_tail0():
    eng = _engine_under(PVT_EPOCH_TAIL="0")
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def engine_plan0():
    eng = _engine_under(PVT_EPOCH_PLAN="0")
    yield eng
    eng.close()


def _regroup(r, anchors):
    """Tasks grouped by the given per-task anchors (first-seen group order)."""
    first = {}
    for a in anchors:
        first.setdefault(int(a), len(first))
    r.task_group = np.array([first[int(a)] for a in anchors], dtype=np.int32)
    r.group_anchor = np.array(list(first.keys()), dtype=np.int32)
    return r


def _round(name):
    if name == "proven":                        # 1
        return synthetic.make_round(_abi.PVT_CA_BF, 5000, 300, seed=1)
    if name == "all_demanded":                  # 2
        r = _round("proven")
        r.dem[2, :] = 1.0
        r.dem[3, :] = 0.125
        return r
    if name == "small_minima":                  # 3
        r = _round("proven")
        r.avail[2, :] = 0.0
        r.avail[3, :] = 0.0
        r.dem[2, :] = 0.0
        r.dem[3, :] = 0.0
        r.avail[0, :] += r.dem[0].max() + 1.0   # cpus separate hosts from tasks (certificate 2)
        return r
    if name == "chain_stops":                   # 4
        r = synthetic.make_round(_abi.PVT_CA_BF, 20_000, 1500, seed=10)
        r.avail[:2, r.zone < 10] = 0.0
        return r
    if name == "two_epochs":                    # 5
        # six groups of ~833 tasks anchored alternately in the components {0, 1, 2} and {3, 4, 5}
        # (groups of at most 1024 tasks on average keep the round on the epoch path)
        r = synthetic.make_round(_abi.PVT_CA_BF, 20_000, 5000, seed=12)
        return _regroup(r, np.array([0, 3, 1, 4, 2, 5])[np.arange(r.n_tasks) % 6])
    if name == "ff_proven":                     # 7
        return synthetic.make_round(_abi.PVT_CA_FF, 5000, 300, seed=1)
    if name == "ff_crowded":                    # 7
        r = synthetic.make_round(_abi.PVT_CA_FF, 8000, 6000, seed=5)
        r.avail[0, :] = 1.0
        r.avail[1, :] = 50000.0
        return r
    if name == "ff_mixed":                      # 7: zones 0-2 keep their cpus, so their chain completes
        r = _round("ff_crowded")
        keep = r.zone < 3
        r.avail[0, keep] = synthetic.make_round(_abi.PVT_CA_FF, 8000, 1, seed=5).avail[0, keep] + 4.0
        return r
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _case(name):
    """The round and its CPU reference, computed once and left unchanged."""
    r = _round(name)
    return r, oracle.place(r, threads=4)


def _same(res, ref):
    np.testing.assert_array_equal(res.placement, ref.placement)
    np.testing.assert_array_equal(res.order, ref.order)
    bad = np.nonzero((res.avail != ref.avail).any(axis=0))[0]
    assert bad.size == 0, "availability differs on hosts %s" % bad[:10]


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


def _check(eng, eng0, name, stats=True):
    """Parity with the oracle on the engine under test and on the PVT_EPOCH_TAIL=0 engine, which
    runs the tail kernels after every frontier walk and never undoes anything (stats: the two
    engines plan the same epochs, so their statistics agree too)."""
    r, ref = _case(name)
    res, st, n = _place(eng, r)
    _same(res, ref)
    res0, st0, n0 = _place(eng0, r)
    _same(res0, ref)
    assert n0[UNDO] == 0, n0
    assert n0["zwalk_kernel"] == 0 or all(n0[k] > 0 for k in TAIL if k != "epoch_validate_kernel"), n0
    for k in ("epochs", "segments", "rejected", "frontier_chains", "list_chains"):
        assert not stats or st[k] == st0[k], (k, st, st0)
    return st, n


def _zero_sets(r):
    """Anchor zone -> the set of zones it reaches at zero egress cost."""
    c = np.asarray(r.cost, dtype=np.float64)
    z0 = (c + c.T) == 0.0
    return {int(a): frozenset(np.nonzero(z0[int(a)])[0].tolist()) for a in np.unique(r.group_anchor)}


def test_proven_epoch_has_no_tail(engine, engine_tail0):
    st, n = _check(engine, engine_tail0, "proven")
    assert all(n[k] == 0 for k in TAIL) and n[UNDO] == 0, n
    assert n["zwalk_kernel"] > 0, n
    assert st["frontier_chains"] > 0 and st["list_chains"] == 0 and st["rejected"] == 0, st


def test_no_undemanded_dimension(engine, engine_tail0):
    """Every dimension is demanded: condition 3 fails whatever the walk proved."""
    st, n = _check(engine, engine_tail0, "all_demanded")
    assert n[UNDO] >= 1 and all(n[k] >= 1 for k in TAIL), n


def test_undemanded_dimensions_with_small_minima(engine, engine_tail0):
    """disk and gpus are undemanded but their host minima are 0; cpus carry the walk's
    separation certificate, so the chains complete and condition 3 alone fails."""
    st, n = _check(engine, engine_tail0, "small_minima")
    assert st["frontier_chains"] > 0, st
    assert n[UNDO] >= 1 and all(n[k] >= 1 for k in TAIL), n


def test_unfinished_chain_is_undone(engine, engine_tail0):
    """Zones 0-9 have no capacity: chains anchored there stop while others completed and wrote
    their windows back; the write-backs are undone before the tail decides."""
    st, n = _check(engine, engine_tail0, "chain_stops")
    assert n[UNDO] >= 1 and n["epoch_accept_apply_kernel"] >= 1, n


def test_two_epochs_without_tail(engine, engine_tail0):
    """Two zero-cost components anchor 2500 tasks each: each chain exceeds CHAIN_MAX = 2048, so
    the round takes more than one epoch, and every epoch is accepted from the walk alone."""
    st, n = _check(engine, engine_tail0, "two_epochs")
    assert st["epochs"] >= 2 and st["frontier_chains"] > 0, st
    assert all(n[k] == 0 for k in TAIL) and n[UNDO] == 0, n


def test_shared_zones_keep_the_tail(engine_plan0, engine_tail0):
    """PVT_EPOCH_PLAN=0: a chain per anchor zone, so chains of one zero-cost component share window
    hosts; no chain may write back and the tail kernels decide."""
    r, _ = _case("proven")
    sets = list(_zero_sets(r).values())
    shared = any(a & b for i, a in enumerate(sets) for b in sets[i + 1:])
    assert shared, "the round's anchors must share zero-cost zones"
    st, n = _check(engine_plan0, engine_tail0, "proven", stats=False)
    assert n["zwalk_kernel"] > 0 and all(n[k] >= 1 for k in TAIL), n
    assert n[UNDO] == 0, n                      # (nothing was written back)


def test_first_fit_proven_epoch_has_no_tail(engine, engine_tail0):
    st, n = _check(engine, engine_tail0, "ff_proven")
    assert n["zwalk_kernel"] > 0, n
    assert n["epoch_final_kernel"] == 0 and n["epoch_accept_apply_kernel"] == 0 and n[UNDO] == 0, n


def test_first_fit_crowded_chains_stop(engine, engine_tail0):
    """One cpu per host: no host strictly fits a task of one cpu, so chains stop and the tail
    decides (an undo only where some chain completed and wrote back)."""
    st, n = _check(engine, engine_tail0, "ff_crowded")
    assert n["epoch_final_kernel"] >= 1 and n["epoch_accept_apply_kernel"] >= 1, n
    assert n[UNDO] <= st["epochs"], (st, n)


def test_first_fit_crowded_chain_is_undone(engine, engine_tail0):
    """The same crowding outside zones 0-2: the chain of that component completes and writes back
    while others stop; undo, then the tail."""
    st, n = _check(engine, engine_tail0, "ff_mixed")
    assert n[UNDO] >= 1, n
    assert n["epoch_final_kernel"] >= 1 and n["epoch_accept_apply_kernel"] >= 1, n


def test_three_consecutive_steps(engine):
    """restore + run on one resident round: the restore reads the placement array the walk
    wrote, so every step starts from the same state and gives the same arrays."""
    r, ref = _case("proven")
    dr = DeviceRound(r, engine.device)
    try:
        engine.set_resident(0)
        for step in range(3):
            if step:
                engine.restore(dr)
            engine.run(dr)
            _same(dr.result(), ref)
    finally:
        engine.set_resident(_abi.PVT_RESIDENT_MAX_HOSTS)
