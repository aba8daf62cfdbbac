"""Realtime-bandwidth rounds (pvt_round.rt_bw; tests/rt_bw_cases.py) on every engine path: the
windowed engine under every window, pipeline and score-kernel setting, host-sharded rounds, mixed
host batches, the device-pointer entry points and the resident kernels. Placement, processing
order and final availability equal the CPU oracle bit for bit; test_rt_bw_cases.py shows on the
oracle alone that every case's placements depend on rt_bw (unsorted first-fit excepted, which must
ignore it).

A windowed or sharded rt_bw round walks no frontier chain (include/pivot_place.h): the zero-score
certificates reason about the static tables, so pvt_zero_walk_stats must count none."""
import contextlib

import numpy as np
import pytest

import golden_io
import rt_bw_cases as rc
from oracle import oracle
from pivot_place import _abi

pytestmark = pytest.mark.gpu

WORLDS = [1, 2, 3, 8]
SEEDS = {rc.TINY: 3, rc.WINDOWED: 1, rc.RESIDENT: 11, rc.EPOCHS: 41}


def _ref(name, *args):
    return rc.reference(name, *args)


def _sized(name, mode, size):
    return rc.reference(name, mode, *size, SEEDS[size])


def _same(got, ref, what=""):
    assert np.array_equal(got.order, ref.order), "%s: order differs" % what
    bad = np.flatnonzero(got.placement != ref.placement)
    assert bad.size == 0, "%s: %d placements differ, first task %d: %d for %d" % (
        what, bad.size, bad[0], got.placement[bad[0]], ref.placement[bad[0]])
    assert np.array_equal(got.avail, ref.avail), "%s: availability differs" % what
    if ref.mt_state is not None:
        assert np.array_equal(got.mt_state, ref.mt_state), "%s: MT19937 state differs" % what


@contextlib.contextmanager
def knobs(engines, resident=_abi.PVT_RESIDENT_MAX_HOSTS, window=0, pipeline=True, tw=0, epochs=True):
    try:
        for e in engines:
            e.set_resident(resident)
            e.set_window(window)
            e.set_pipeline(pipeline)
            e.set_score_tw(tw)
            e.set_epochs(epochs)
        yield
    finally:
        for e in engines:
            e.set_epochs(True)
            e.set_score_tw(0)
            e.set_pipeline(True)
            e.set_window(0)
            e.set_resident(_abi.PVT_RESIDENT_MAX_HOSTS)


@pytest.fixture(scope="module")
def engines():
    from pivot_place.engine import PlacementEngine
    return [PlacementEngine(0) for _ in range(8)]


def _windowed(engine, r, ref, what, **kw):
    with knobs([engine], resident=0, **kw):
        got = engine.place(rc.fresh(r))
        st = engine.epoch_stats()
        last = engine.last_stats()
    _same(got, ref, what)
    assert st["frontier_chains"] == 0, (what, st)
    return last


# ---- windowed knobs ------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", rc.MODES, ids=rc.IDS)
@pytest.mark.parametrize("name", ["queue", "uniform", "tight"])
def test_windowed_knobs(engine, name, mode):
    """pvt_place_host on the windowed engine: windows of 1, 3, 37 and the default (an odd last
    window each), the pipeline on and off, the 2- and the 4-tasks-per-wave score kernel. A
    best-fit round plans group epochs whatever the window (its list chains are scored per
    segment), so it runs the whole cross with the epochs off as well: then the windows are the
    list windows. First-fit has no epochs with rt_bw."""
    r, ref = _sized(name, mode, rc.WINDOWED)
    for epochs in (True, False) if mode == rc.BF else (True,):
        for window in (1, 3, 37, 0):
            for pipeline in (True, False):
                for tw in (2, 4):
                    _windowed(engine, r, ref, "%s epochs %d window %d pipeline %d tw %d"
                              % (name, epochs, window, pipeline, tw),
                              epochs=epochs, window=window, pipeline=pipeline, tw=tw)
    if mode == rc.FF:
        _windowed(engine, r, ref, "%s epochs off" % name, epochs=False)


@pytest.mark.parametrize("tw,epochs", [(0, True), (4, True), (4, False)])
@pytest.mark.parametrize("mode", rc.MODES, ids=rc.IDS)
def test_windowed_epochs_round(engine, mode, tw, epochs):
    """20000 hosts: best-fit plans group epochs (several segments, validated against the
    segment's row; epochs off: list windows of 1024 and 475 tasks), first-fit keys every group
    from its own row."""
    r, ref = _sized("queue", mode, rc.EPOCHS)
    _windowed(engine, r, ref, "queue 20000 tw %d epochs %d" % (tw, epochs), tw=tw, epochs=epochs)


@pytest.mark.parametrize("tasks", [rc.RESIDENT[1], rc.TIGHT_BF_TASKS])
@pytest.mark.parametrize("mode", rc.MODES, ids=rc.IDS)
def test_windowed_lists_run_dry(engine, mode, tasks):
    """3000 hosts that fill up (first-fit leaves 604 of 1500 tasks waiting, best-fit 172 of 4096)
    on the windowed engine: windows of 37 and the default, pipeline on and off, both score
    kernels, epochs on and off. At the default window best-fit lists run dry and are refilled
    (measured without epochs: 4 refills at 1500 tasks, 30 at 4096; asserted). Windows of 37 tasks
    and first-fit rounds need no refill (measured: 0): there the walk only rescores the hosts an
    earlier task of the window took, from the task's own row."""
    r, ref = rc.reference("tight", mode, rc.RESIDENT[0], tasks, 11)
    for epochs in (True, False) if mode == rc.BF else (True,):
        for window in (37, 0):
            for pipeline, tw in ((True, 4), (False, 2)):
                last = _windowed(engine, r, ref, "tight %d epochs %d window %d pipeline %d tw %d"
                                 % (tasks, epochs, window, pipeline, tw),
                                 epochs=epochs, window=window, pipeline=pipeline, tw=tw)
                if mode == rc.BF and window == 0:
                    assert last["refills"] > 0, last


# ---- host sharding -------------------------------------------------------------------------------
def _place_lockstep(engines, r):
    """pivot_place.sharded.place_lockstep, counting the windows and those that came back
    PVT_ESTALE (scored past a walk that stopped early, and scored again)."""
    import torch
    from pivot_place.engine import DeviceRound
    from pivot_place.sharded import shard_range
    world = len(engines)
    drs = [DeviceRound(r, e.device) for e in engines]
    mx = [e.shard_begin(dr, *shard_range(r.n_hosts, world, k, r.mode), world)
          for k, (e, dr) in enumerate(zip(engines, drs))]
    sends = [torch.empty(max(m, 1), dtype=torch.uint8, device=e.device) for m, e in zip(mx, engines)]
    recvs = [torch.empty(max(m, 1) * world, dtype=torch.uint8, device=e.device)
             for m, e in zip(mx, engines)]
    windows = stale = 0
    while True:
        got = [e.shard_score(s) for e, s in zip(engines, sends)]
        assert len(set(got)) == 1, "shards disagree on the window: %s" % (got,)
        nt, nb = got[0]
        if nt == 0:
            break
        for recv in recvs:
            for k, s in enumerate(sends):
                recv[k * nb:(k + 1) * nb].copy_(s[:nb])
        ok = [e.shard_commit(recv) for e, recv in zip(engines, recvs)]
        assert len(set(ok)) == 1, "shards disagree on a stale window: %s" % (ok,)
        windows += 1
        stale += not ok[0]
    return [dr.result() for dr in drs], windows, stale


def _no_frontier(engines, what):
    for e in engines:
        st = e.epoch_stats()
        assert st["frontier_chains"] == 0, (what, st)


def _lockstep(engines, world, r, ref, what):
    """Every rank equals rank 0, rank 0 equals ``ref``, no rank walked a frontier chain; returns
    (windows, stale windows)."""
    outs, windows, stale = _place_lockstep(engines[:world], r)
    for k, o in enumerate(outs[1:]):
        _same(o, outs[0], "%s: rank %d against rank 0" % (what, k + 1))
    _same(outs[0], ref, what)
    _no_frontier(engines[:world], what)
    return windows, stale


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("mode", rc.MODES, ids=rc.IDS)
@pytest.mark.parametrize("size", [rc.TINY, rc.WINDOWED, rc.EPOCHS], ids=["h5", "h5000", "h20000"])
def test_sharded_queue(engines, size, mode, world):
    """Every rank scores its hosts [lo, hi) against rows indexed by the global host; at 5 hosts
    ranks hold one host or none."""
    r, ref = _sized("queue", mode, size)
    _lockstep(engines, world, r, ref, "queue %s world %d" % (size, world))


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("mode", rc.MODES, ids=rc.IDS)
@pytest.mark.parametrize("name", ["ungrouped", "extreme"])
def test_sharded_cases(engines, name, mode, world):
    r, ref = _sized(name, mode, rc.RESIDENT)
    _lockstep(engines, world, r, ref, "%s world %d" % (name, world))


@pytest.mark.parametrize("world", WORLDS)
def test_sharded_with_decay(engines, world):
    r, ref = _ref("with_decay", *rc.RESIDENT, 11)
    _lockstep(engines, world, r, ref, "with_decay world %d" % world)


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("mode", rc.MODES, ids=rc.IDS)
def test_sharded_wide(engines, mode, world):
    r, ref = _ref("wide", mode)
    _lockstep(engines, world, r, ref, "wide world %d" % world)


@pytest.mark.parametrize("pipeline", [True, False])
@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("mode", rc.MODES, ids=rc.IDS)
def test_sharded_tight_small_windows(engines, mode, world, pipeline):
    """Windows of 37 tasks on hosts that fill up (41 windows best-fit, 51 first-fit: a first-fit
    window ends with its group): the replicated walk rescores the hosts that earlier tasks took
    from the merged packages. Windows this short never come back stale (measured: 0)."""
    r, ref = _sized("tight", mode, rc.RESIDENT)
    with knobs(engines, window=37, pipeline=pipeline):
        windows, _ = _lockstep(engines, world, r, ref, "tight world %d pipeline %d" % (world, pipeline))
    assert windows >= (r.n_tasks + 36) // 37


@pytest.mark.parametrize("world", WORLDS)
def test_sharded_tight_best_fit_stale_windows(engines, world):
    """Best-fit, 4096 tasks of which 172 stay waiting, the default window, the pipeline on: walks
    stop early on exhausted packages and the window scored ahead comes back PVT_ESTALE and is
    scored again (measured: 32, 19, 7 and 1 stale windows at worlds 1, 2, 3 and 8; asserted where
    there are several). With the pipeline off nothing is scored ahead."""
    r, ref = _ref("tight", rc.BF, rc.RESIDENT[0], rc.TIGHT_BF_TASKS, 11)
    what = "tight best-fit %d tasks world %d" % (r.n_tasks, world)
    _, stale = _lockstep(engines, world, r, ref, what)
    print("%s: %d stale windows" % (what, stale))
    if world <= 3:
        assert stale > 0
    with knobs(engines, pipeline=False):
        _, stale = _lockstep(engines, world, r, ref, what + " pipeline off")
    assert stale == 0


@pytest.mark.parametrize("name,idx", [x for x in golden_io.all_runs() if x[0] in ("rt_c1_h100", "rt_h12")])
def test_sharded_reference_golden(engines, name, idx):
    """The runs of the reference's realtime_bw fixtures at world 3 (each fixture's last run has
    no realtime_bw). A run that reads rt_bw (best-fit, or first-fit with sort_hosts) walks no
    frontier chain; the unsorted first-fit run ignores rt_bw and may take the ordered frontier as
    it does without."""
    case = golden_io.load(name)
    run = case["runs"][idx]
    r = golden_io.run_arrays(case, run)
    placement, order, avail, _ = golden_io.expected(case, run)
    outs, _, _ = _place_lockstep(engines[:3], r)
    for o in outs:
        assert np.array_equal(o.placement, placement)
        assert np.array_equal(o.order, order)
        assert np.array_equal(o.avail, avail)
    if r.rt_bw is not None and (r.mode == rc.BF or r.sort_hosts):
        _no_frontier(engines[:3], "%s run %d" % (name, idx))


# ---- host batch ----------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["narrow", "wide"])
def test_host_batch(engine, which):
    """pvt_place_host_batch: rounds with 1, 3 and 20 rows of rt_bw staged between rounds with none.
    The first round takes the zone-table cache, so in one launch rt_bw rounds of each row count
    read the cached tables beside their staged rt_bw block while other rt_bw rounds (extreme's
    scaled tables; wide: the 20-zone rounds) stage tables and rt_bw both
    (rt_bw_cases.table_cache_hits states the engine's rule; test_rt_bw_cases.py checks the mix).
    The wide batch runs every round on the wide kernels. Each round equals the oracle and the same
    round through place() alone."""
    rounds = rc.batch_rounds() if which == "narrow" else rc.wide_batch_rounds()
    hits = rc.table_cache_hits([r for _, r in rounds])
    assert any(h and r.rt_bw is not None and r.rt_bw.shape[0] > 1 for (_, r), h in zip(rounds, hits))
    assert any(not h and r.rt_bw is not None for (_, r), h in zip(rounds, hits))
    assert {r.mode for _, r in rounds} == {_abi.PVT_CA_FF, _abi.PVT_CA_BF, _abi.PVT_OPP,
                                           _abi.PVT_VBP_FF, _abi.PVT_VBP_BF}
    for _, r in rounds:
        assert engine.host_batch_fits(r)
        assert which == "narrow" or r.n_hosts <= _abi.PVT_RESIDENT_WIDE_MAX_HOSTS
    got = engine.place_host_batch([(rc.fresh(r), None) for _, r in rounds])
    assert len(got) == len(rounds)
    assert engine.resident_shape()["wide"] == (which == "wide")
    for (label, r), g in zip(rounds, got):
        ref = oracle.place(r)
        _same(g, ref, "batch round '%s'" % label)
        _same(engine.place(rc.fresh(r)), ref, "round '%s' alone" % label)


# ---- device entry points -------------------------------------------------------------------------
@pytest.mark.parametrize("mode", rc.MODES, ids=rc.IDS)
@pytest.mark.parametrize("size", [rc.RESIDENT, rc.WINDOWED], ids=["h3000", "h5000"])
def test_device_round_and_resident_cluster(engine, size, mode):
    """DeviceRound and ResidentCluster.place upload rt_bw themselves (3000 hosts: the resident
    kernel through pvt_place; 5000: the windowed engine)."""
    from pivot_place.engine import DeviceRound
    from pivot_place.hostops import ResidentCluster
    r, ref = _sized("queue", mode, size)
    dr = DeviceRound(r, engine.device)
    engine.run(dr)
    _same(dr.result(), ref, "DeviceRound")
    if size == rc.WINDOWED:
        assert engine.epoch_stats()["frontier_chains"] == 0
    cluster = ResidentCluster(engine, r.avail, r.zone, r.cost, r.bw)
    _same(cluster.place(r, want_avail=True), ref, "ResidentCluster")
    if size == rc.WINDOWED:
        assert engine.epoch_stats()["frontier_chains"] == 0


@pytest.mark.parametrize("mode", rc.MODES, ids=rc.IDS)
def test_place_batch(engine, mode):
    """pvt_place_batch over rounds of one policy with 20, 1, 20 and 3 rows of rt_bw."""
    cases = [_sized("queue", mode, rc.RESIDENT), _sized("ungrouped", mode, rc.RESIDENT),
             _sized("extreme", mode, rc.RESIDENT), _ref("few_groups", mode, 1000, 333, 605, 3)]
    for (r, ref), got in zip(cases, engine.place_batch([r for r, _ in cases])):
        _same(got, ref, "place_batch H=%d G=%d" % (r.n_hosts, r.n_groups))


# ---- resident and windowed, the cases of one group, decay, extreme values --------------------------
@pytest.mark.parametrize("path", ["resident", "windowed"])
@pytest.mark.parametrize("mode", rc.MODES, ids=rc.IDS)
@pytest.mark.parametrize("name", ["ungrouped", "extreme"])
def test_cases_both_engines(engine, name, mode, path):
    r, ref = _sized(name, mode, rc.RESIDENT)
    if path == "windowed":
        _windowed(engine, r, ref, name)
    else:
        _same(engine.place(rc.fresh(r)), ref, name)


@pytest.mark.parametrize("path", ["resident", "windowed"])
def test_with_decay_both_engines(engine, path):
    r, ref = _ref("with_decay", *rc.RESIDENT, 11)
    if path == "windowed":
        _windowed(engine, r, ref, "with_decay")
    else:
        _same(engine.place(rc.fresh(r)), ref, "with_decay")


@pytest.mark.parametrize("path", ["resident", "windowed"])
def test_unsorted_first_fit_ignores_rt_bw(engine, path):
    """First-fit without sort_hosts reads no bandwidth. It takes the ordered path (R.ordered: the
    ordered frontier walk over the first alive hosts, then the lists) exactly as the round without
    rt_bw does -- the switch on rt_bw in the round setup covers the keyed zero-key epochs only --
    so the windowed round walks as many frontier chains as its twin without rt_bw, and more than
    none."""
    r, ref = _ref("unsorted_ff", *rc.RESIDENT, 11)
    with knobs([engine], resident=_abi.PVT_RESIDENT_MAX_HOSTS if path == "resident" else 0):
        got = engine.place(rc.fresh(r))
        st = engine.epoch_stats()
        twin = engine.place(rc.without_rt(r))
        st_twin = engine.epoch_stats()
    _same(got, ref, "unsorted_ff")
    _same(twin, ref, "unsorted_ff without rt_bw")
    if path == "windowed":
        assert st["frontier_chains"] == st_twin["frontier_chains"] > 0, (st, st_twin)
