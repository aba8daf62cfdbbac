"""GPU tests of the fused cost_aware grouping (csrc/pvt_groups_dev.h ``ca_groups_round``) on each
of its three instantiations and at its size edges (tests/grouping_cases.py; the CPU checks of
those cases are tests/test_grouping_cases.py):

  single   ``ca_groups_kernel`` behind ``pvt_place_host``, then a resident or a windowed placement
           (what ``place_cost_aware`` calls for a round no one-round host batch takes)
  fused    ``ca_groups_round<256, 4096>`` inside ``resident_fused_kernel`` (``place_host_batch``)
  staged   ``ca_groups_batch_kernel`` (``place_host_batch`` on a context created under PVT_FUSED=0)

The truth is ``oracle.place`` of the round completed with ``group_reference``'s task_group /
group_anchor; placement, order, availability, the group count and the randomizer state after the
draws are compared bit for bit. Every run proves its path by the launches of the named kernels
(``resident_fused_kernel``, ``resident_kernel``) under profiling mode 2.
"""
import dataclasses

import numpy as np
import pytest

import grouping_cases as gc
from oracle import oracle
from pivot_place import _abi, synthetic

from test_gpu_epoch_tail import _engine_under

pytestmark = pytest.mark.gpu

PATHS = ("single", "fused", "staged")
NUMBERING = ("chunk_last", "chunk_first", "lanes_0_63", "last_wave", "reused_key", "one_group",
             "all_apps_4096")
DRAWS = tuple("storages_%d" % s for s in gc.STORAGES) + ("sparse_words", "full_word", "twist") + \
    tuple("position_%d" % p for p in gc.POSITIONS) + ("keys_8192",)


@pytest.fixture(scope="module")
def engine_staged():
    eng = _engine_under(PVT_FUSED="0")
    yield eng
    eng.close()


def _counted(eng, fn):
    """fn() and the launches of the two resident kernels during it."""
    eng.set_profiling(2)
    eng.reset_kstats()
    try:
        out = fn()
        n = {k: eng.kernel_kstats(k)["launches"] for k in ("resident_fused_kernel", "resident_kernel")}
    finally:
        eng.set_profiling(False)
    return out, n


def _place_host(eng, c):
    """pvt_place_host with the case's items: (result arrays, rc, randomizer state, status)."""
    it, keep, mt, status = eng._ca_items(*c.ca_args())
    res, rc = eng._place_host(c.r, it)
    del keep
    return res, rc, mt, status


def _single(eng, c):
    res, rc, mt, status = _place_host(eng, c)
    return eng._ca_result(res, rc, mt, status)


def _resident(eng, c):
    return c.r.n_tasks > 0 and eng.host_batch_fits(c.r, c.ca_args())


def _run(path, engine, engine_staged, c):
    """The case on the named path, with the proof that the path ran."""
    if path == "single":
        got, n = _counted(engine, lambda: _single(engine, c))
        assert n["resident_fused_kernel"] == 0, n
        if c.r.n_tasks:
            # (neither resident kernel: the windowed engine placed the round)
            assert n["resident_kernel"] == (1 if _resident(engine, c) else 0), n
        return got
    eng = engine if path == "fused" else engine_staged
    got, n = _counted(eng, lambda: eng.place_host_batch([(c.r, c.ca_args())])[0])
    if path == "fused":
        assert n["resident_fused_kernel"] == 1 and n["resident_kernel"] == 0, n
    else:
        assert n["resident_fused_kernel"] == 0 and n["resident_kernel"] == 1, n
    return got


def _same(got, want, what=""):
    """got: what place_cost_aware returns; want: grouping_cases.expected."""
    assert isinstance(got, tuple), "%s: %r" % (what, got)
    res, groups, mt = got
    tg, ga, G, mt_after, ref = want
    np.testing.assert_array_equal(res.order, ref.order, err_msg=what)
    np.testing.assert_array_equal(res.placement, ref.placement, err_msg=what)
    bad = np.nonzero((res.avail != ref.avail).any(axis=0))[0]
    assert bad.size == 0, "%s: availability differs on hosts %s" % (what, bad[:10])
    assert groups == G, what
    assert np.array_equal(mt, mt_after), "%s: randomizer state (position %d, expected %d)" % (
        what, mt[624], mt_after[624])


def _snapshot(c):
    return [a.copy() for a in (c.r.avail, c.r.dem, c.r.zone, c.task_item, c.pred_off, c.pred_host,
                               c.item_app, c.storage_zone, c.zone_storage, c.mt_state)]


def _untouched(c, snap):
    for a, b in zip(_snapshot(c), snap):
        assert a.tobytes() == b.tobytes()


# ---- task counts ---------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("T", gc.TASK_COUNTS)
def test_task_counts(engine, engine_staged, T, path):
    name = "tasks_%d" % T
    c = gc.case(name)
    assert engine.host_batch_fits(c.r, c.ca_args())
    _same(_run(path, engine, engine_staged, c), gc.expected(name), name)


@pytest.mark.parametrize("T", gc.BIG_TASK_COUNTS)
def test_task_counts_beyond_the_resident_kernel(engine, engine_staged, T):
    """More than 4096 tasks: the single path with the windowed placement (the status read back
    mid-round, n_groups set on the host); a host batch refuses the round and writes nothing."""
    name = "tasks_%d" % T
    c = gc.case(name)
    snap = _snapshot(c)
    assert not engine.host_batch_fits(c.r, c.ca_args())
    _same(_run("single", engine, engine_staged, c), gc.expected(name), name)
    got, n = _counted(engine, lambda: engine.place_cost_aware(c.r, *c.ca_args()))
    assert n["resident_fused_kernel"] == 0 and n["resident_kernel"] == 0, n
    _same(got, gc.expected(name), name + " place_cost_aware")
    for eng in (engine, engine_staged):
        with pytest.raises(RuntimeError, match="EUNSUPPORTED"):
            eng.place_host_batch([(gc.case("tasks_63").r, gc.case("tasks_63").ca_args()),
                                  (c.r, c.ca_args())])
    _untouched(c, snap)


def test_small_grouping_meets_the_windowed_engine(engine, engine_staged):
    """1024 tasks on 5000 hosts, and 1024 tasks on 96 hosts under set_resident(0)."""
    c = gc.case("hosts_5000")
    assert not engine.host_batch_fits(c.r, c.ca_args())
    _same(_run("single", engine, engine_staged, c), gc.expected("hosts_5000"), "hosts_5000")
    c = gc.case("tasks_1024")
    try:
        engine.set_resident(0)
        assert not engine.host_batch_fits(c.r, c.ca_args())
        got = _run("single", engine, engine_staged, c)
        pub, n = _counted(engine, lambda: engine.place_cost_aware(c.r, *c.ca_args()))
    finally:
        engine.set_resident(_abi.PVT_RESIDENT_MAX_HOSTS)
    assert n["resident_fused_kernel"] == 0 and n["resident_kernel"] == 0, n
    _same(got, gc.expected("tasks_1024"), "set_resident(0)")
    _same(pub, gc.expected("tasks_1024"), "set_resident(0) place_cost_aware")


# ---- group numbering across chunks ---------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", NUMBERING)
def test_group_numbering_across_chunks(engine, engine_staged, name, path):
    _same(_run(path, engine, engine_staged, gc.case(name)), gc.expected(name), name)


def test_every_task_its_own_group_at_the_key_limit(engine, engine_staged):
    """T = G = 8191 with one storage: S + n_apps = 8192 is accepted, and no draw is made."""
    c = gc.case("all_apps_8191")
    got = _run("single", engine, engine_staged, c)
    _same(got, gc.expected("all_apps_8191"), "all_apps_8191")
    assert got[1] == 8191 and np.array_equal(got[2], c.mt_state)


# ---- draws ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", DRAWS)
def test_draws(engine, engine_staged, name, path):
    c = gc.case(name)
    got = _run(path, engine, engine_staged, c)
    _same(got, gc.expected(name), name)
    if len(c.storage_zone) == 1:
        assert np.array_equal(got[2], c.mt_state), "a draw was made for one storage"
    else:
        assert not np.array_equal(got[2], c.mt_state)


# ---- limits --------------------------------------------------------------------------------------
def _refused(engine, c):
    snap = _snapshot(c)
    assert not engine.host_batch_fits(c.r, c.ca_args())
    assert engine.place_cost_aware(c.r, *c.ca_args()) is None
    res, rc, mt, status = _place_host(engine, c)
    assert rc == _abi.PVT_EUNSUPPORTED
    assert res.avail.tobytes() == c.r.avail.tobytes() and np.array_equal(mt, c.mt_state)
    assert status.tolist() == [0, 0]
    _untouched(c, snap)


def test_limits_are_refused_with_nothing_written(engine):
    ok = gc.case("keys_8192")
    assert len(ok.storage_zone) + ok.n_apps == 8192 and engine.host_batch_fits(ok.r, ok.ca_args())
    _refused(engine, dataclasses.replace(ok, n_apps=ok.n_apps + 1))
    _refused(engine, gc.build("tasks_16385", gc.mixed(16385, 4, 6, 1)))


# ---- anchors inside the grouping -----------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", ["lists", "lists_b"])
def test_tied_lists_at_the_anchor_edges(engine, engine_staged, name, path):
    """Lists of 64, 65, 1024, 1025, 8192 and 8193 tied entries (the first seen wins), at least
    three of them deferred to the block pass in one round."""
    _same(_run(path, engine, engine_staged, gc.case(name)), gc.expected(name), name)


def _plain(mode, seed):
    r = synthetic.make_round(mode, 200, 100, seed=seed)
    return r, oracle.place(r)


def _same_plain(res, ref, what):
    assert not isinstance(res, Exception), res
    np.testing.assert_array_equal(res.placement, ref.placement, err_msg=what)
    np.testing.assert_array_equal(res.order, ref.order, err_msg=what)
    assert np.array_equal(res.avail, ref.avail), what
    if ref.mt_state is not None:
        assert np.array_equal(res.mt_state, ref.mt_state), what


@pytest.mark.parametrize("path", ["fused", "staged"])
def test_deferred_lists_of_two_rounds_in_one_batch(engine, engine_staged, path):
    eng = engine if path == "fused" else engine_staged
    opp, opp_ref = _plain(_abi.PVT_OPP, 3)
    vbp, vbp_ref = _plain(_abi.PVT_VBP_BF, 4)
    a, b = gc.case("lists"), gc.case("lists_b")
    out, n = _counted(eng, lambda: eng.place_host_batch(
        [(a.r, a.ca_args()), (opp, None), (b.r, b.ca_args()), (vbp, None)]))
    assert n["resident_fused_kernel"] == (1 if path == "fused" else 0), n
    _same(out[0], gc.expected("lists"), "lists")
    _same_plain(out[1], opp_ref, "opportunistic")
    _same(out[2], gc.expected("lists_b"), "lists_b")
    _same_plain(out[3], vbp_ref, "vbp")


# ---- wide zones ----------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_forty_zones(engine, engine_staged, path):
    _same(_run(path, engine, engine_staged, gc.case("zones_40")), gc.expected("zones_40"), "zones_40")


# ---- errors --------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("at", [gc.ERROR_T - 1, 0], ids=["last", "first"])
@pytest.mark.parametrize("kind", gc.ERROR_KINDS)
def test_grouping_errors(engine, engine_staged, kind, at, path):
    """The reference's exception, with the round's arrays and randomizer state unchanged."""
    c, exc, pattern = gc.error_case(kind, at)
    snap = _snapshot(c)
    if path == "single":
        with pytest.raises(exc, match=pattern):
            _single(engine, c)
        res, rc, mt, status = _place_host(engine, c)
        assert rc == _abi.PVT_EINVAL and res.avail.tobytes() == c.r.avail.tobytes()
        assert np.array_equal(mt, c.mt_state)
    else:
        got = _run(path, engine, engine_staged, c)
        assert type(got) is exc and pattern in str(got), got
    _untouched(c, snap)


@pytest.mark.parametrize("kind", ["unplaced", "item_hi"])
def test_grouping_error_in_the_last_pass_of_a_windowed_round(engine, kind):
    """Task 16383 of 16384, the last of the single kernel's sixteenth pass: the error comes back
    with the status the windowed placement reads mid-round, and nothing is placed."""
    c, exc, pattern = gc.broken(gc.case("tasks_16384"), kind, 16383)
    assert type(c.groups()) is exc
    snap = _snapshot(c)
    with pytest.raises(exc, match=pattern):
        engine.place_cost_aware(c.r, *c.ca_args())
    res, rc, mt, status = _place_host(engine, c)
    assert rc == _abi.PVT_EINVAL and res.avail.tobytes() == c.r.avail.tobytes()
    assert np.array_equal(mt, c.mt_state)
    _untouched(c, snap)


HEALTHY = ("tasks_257", "storages_3", "sparse_words", "lists_b")


@pytest.mark.parametrize("path", ["fused", "staged"])
@pytest.mark.parametrize("kind,at", [(k, gc.ERROR_T - 1) for k in gc.ERROR_KINDS] + [("unplaced", 0)])
def test_a_bad_round_beside_healthy_rounds(engine, engine_staged, kind, at, path):
    eng = engine if path == "fused" else engine_staged
    bad, exc, pattern = gc.error_case(kind, at)
    good = [gc.case(n) for n in HEALTHY]
    reqs = [(c.r, c.ca_args()) for c in good]
    out = eng.place_host_batch(reqs[:2] + [(bad.r, bad.ca_args())] + reqs[2:])
    assert type(out[2]) is exc and pattern in str(out[2]), out[2]
    for got, name in zip(out[:2] + out[3:], HEALTHY):
        _same(got, gc.expected(name), name + " beside the bad round")
    for got, name in zip(eng.place_host_batch(reqs), HEALTHY):
        _same(got, gc.expected(name), name + " after the bad round")


# ---- several grouped rounds in one batch ---------------------------------------------------------
def _eight():
    names = ("tasks_1", "tasks_4096", None, "tasks_63", "tasks_257", "tasks_1025", "storages_33",
             "twist")
    out = []
    for i, name in enumerate(names):
        c = gc.build("empty", []) if name is None else gc.case(name)
        c = dataclasses.replace(c, mt_state=gc.mt_at(100 + i, 624 if i % 2 else 17 * i))
        out.append((c, gc.expected_of(c)))
    return out


@pytest.mark.parametrize("path", ["fused", "staged"])
def test_eight_grouped_rounds_in_one_batch(engine, engine_staged, path):
    """Different sizes (1 and 4096 tasks and an empty round among them), each round with its own
    randomizer state, each equal to the reference and to its single-path result."""
    eng = engine if path == "fused" else engine_staged
    eight = _eight()
    out, n = _counted(eng, lambda: eng.place_host_batch([(c.r, c.ca_args()) for c, _ in eight]))
    assert n["resident_fused_kernel"] == (1 if path == "fused" else 0), n
    for got, (c, want) in zip(out, eight):
        _same(got, want, c.name)
        one = _single(engine, c)
        _same(one, want, c.name + " single")
        assert got[0].placement.tobytes() == one[0].placement.tobytes()
