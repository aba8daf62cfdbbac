"""GPU parity on clusters of 33 to 512 zones (PVT_MAX_ZONES): every entry point that takes a
round, all five policies, against the CPU restatement -- placements, order, availability and
MT19937 state, bit for bit. The rounds are contended (wide_cases), so cost_aware winners reach
positive-cost zones. Zone counts: 33 is the first past the fast bound, 64 and 65 straddle the
one-lane-per-zone boundary of the wave64 row fills, 512 is the maximum (LDS budgets, table
sizes)."""
import ctypes

import numpy as np
import pytest

import wide_cases
from oracle import oracle
from pivot_place import _abi, policies, synthetic
from pivot_place.engine import DeviceBatch, DeviceRound
from test_sim_replay import OracleEngine

pytestmark = pytest.mark.gpu

ZONES = [33, 64, 65, 512]
ALL_MODES = wide_cases.ALL_MODES


def _same(got, ref, what=""):
    np.testing.assert_array_equal(got.placement, ref.placement, err_msg=what)
    np.testing.assert_array_equal(got.order, ref.order, err_msg=what)
    bad = np.nonzero((got.avail != ref.avail).any(axis=0))[0]
    assert bad.size == 0, "%s: availability differs on hosts %s" % (what, bad[:10])
    if ref.mt_state is not None:
        np.testing.assert_array_equal(got.mt_state, ref.mt_state, err_msg=what)


def _device_place(engine, r):
    """pvt_place on device arrays."""
    dr = DeviceRound(wide_cases.fresh(r), engine.device)
    engine.run(dr)
    return dr.result()


@pytest.mark.parametrize("mode", ALL_MODES)
@pytest.mark.parametrize("Z", ZONES)
def test_resident_round(engine, Z, mode):
    """Default routing, H = 2Z + 5: pvt_place_host (the fused resident launch) and pvt_place."""
    r, ref = wide_cases.case(mode, Z)
    _same(engine.place(wide_cases.fresh(r)), ref, "pvt_place_host")
    _same(_device_place(engine, r), ref, "pvt_place")


@pytest.mark.parametrize("mode", ALL_MODES)
@pytest.mark.parametrize("Z", ZONES)
def test_windowed_engine_on_the_small_round(engine, Z, mode):
    r, ref = wide_cases.case(mode, Z)
    try:
        engine.set_resident(0)
        _same(engine.place(wide_cases.fresh(r)), ref, "pvt_place_host")
        _same(_device_place(engine, r), ref, "pvt_place")
    finally:
        engine.set_resident(_abi.PVT_RESIDENT_MAX_HOSTS)


@pytest.mark.parametrize("mode", ALL_MODES)
@pytest.mark.parametrize("Z", ZONES)
def test_windowed_round_of_5000_hosts(engine, Z, mode):
    """Natural windowed routing, several windows."""
    r, ref = wide_cases.case(mode, Z, "large")
    _same(_device_place(engine, r), ref)
    if mode != _abi.PVT_OPP:
        assert engine.last_stats()["windows"] > 1


def test_wide_rounds_of_2049_to_4096_hosts(engine):
    """A cost_aware round of more than 32 zones is resident up to 2048 hosts and windowed above;
    a round of a policy that reads no zone tables stays resident up to 4096."""
    for mode in (_abi.PVT_CA_BF, _abi.PVT_CA_FF, _abi.PVT_VBP_BF, _abi.PVT_OPP):
        r = wide_cases.contended_round(mode, 65, 3000, 3500, 3500.0, 11)
        ref = oracle.place(r)
        wide_cases.assert_contended(r, ref)
        _same(engine.place(wide_cases.fresh(r)), ref, "mode %d host" % mode)
        _same(_device_place(engine, r), ref, "mode %d device" % mode)


@pytest.mark.parametrize("mode", [_abi.PVT_CA_FF, _abi.PVT_CA_BF])
@pytest.mark.parametrize("path", ["resident", "windowed"])
def test_realtime_bw_at_65_zones(engine, mode, path):
    H, T, mem_hi, seed = wide_cases.SMALL[65]
    r = wide_cases.contended_round(mode, 65, H, T, mem_hi, seed)
    rs = np.random.RandomState(17)
    r.rt_bw = np.ascontiguousarray(rs.uniform(0.5, 200.0, size=(r.n_groups, H)))
    ref = oracle.place(r)
    wide_cases.assert_contended(r, ref)
    try:
        engine.set_resident(_abi.PVT_RESIDENT_MAX_HOSTS if path == "resident" else 0)
        _same(engine.place(wide_cases.fresh(r)), ref)
    finally:
        engine.set_resident(_abi.PVT_RESIDENT_MAX_HOSTS)


@pytest.mark.parametrize("path", ["resident", "windowed"])
@pytest.mark.parametrize("sort_hosts", [True, False])
@pytest.mark.parametrize("decay", [True, False])
def test_first_fit_decay_and_sort_hosts(engine, decay, sort_hosts, path):
    H, T, mem_hi, seed = wide_cases.SMALL[65]
    r = wide_cases.contended_round(_abi.PVT_CA_FF, 65, H, T, mem_hi, seed, sort_hosts=sort_hosts)
    if decay:
        r.decay = np.random.RandomState(3).randint(1, 6, size=H).astype(np.int32)
    ref = oracle.place(r)
    wide_cases.assert_contended(r, ref, by_cost=sort_hosts)   # (unsorted first fit goes by index)
    try:
        engine.set_resident(_abi.PVT_RESIDENT_MAX_HOSTS if path == "resident" else 0)
        _same(engine.place(wide_cases.fresh(r)), ref)
    finally:
        engine.set_resident(_abi.PVT_RESIDENT_MAX_HOSTS)


@pytest.mark.parametrize("path", ["resident", "windowed"])
@pytest.mark.parametrize("mode", [_abi.PVT_CA_FF, _abi.PVT_CA_BF])
def test_sort_tasks_off(engine, mode, path):
    H, T, mem_hi, seed = wide_cases.SMALL[65]
    r = wide_cases.contended_round(mode, 65, H, T, mem_hi, seed, sort_tasks=False)
    ref = oracle.place(r)
    wide_cases.assert_contended(r, ref)
    try:
        engine.set_resident(_abi.PVT_RESIDENT_MAX_HOSTS if path == "resident" else 0)
        _same(engine.place(wide_cases.fresh(r)), ref)
    finally:
        engine.set_resident(_abi.PVT_RESIDENT_MAX_HOSTS)


@pytest.mark.parametrize("mode", ALL_MODES)
def test_place_batch_mixing_20_and_65_zones(engine, mode):
    rounds = []
    for i in range(8):
        Z = 65 if i % 2 else 20
        rounds.append(wide_cases.contended_round(mode, Z, 2 * Z + 5 + i, 300 + 9 * i, 40000.0, 40 + i))
    refs = [oracle.place(r) for r in rounds]
    got = engine.place_batch([wide_cases.fresh(r) for r in rounds])
    for i, (g, ref) in enumerate(zip(got, refs)):
        _same(g, ref, "round %d" % i)


@pytest.mark.parametrize("mode", ALL_MODES)
def test_place_batch_at_512_zones(engine, mode):
    r, ref = wide_cases.case(mode, 512)
    r2 = wide_cases.contended_round(mode, 512, 1029, 3500, 40000.0, 8)
    got = engine.place_batch([wide_cases.fresh(r), wide_cases.fresh(r2)])
    _same(got[0], ref, "round 0")
    _same(got[1], oracle.place(r2), "round 1")


class _Recorder(OracleEngine):
    """The oracle-backed engine that also records the fused request and declines it, so the
    policy goes on to anchor + place (on the oracle)."""

    def __init__(self):
        self.requests = []

    def place_cost_aware(self, r, *ca):
        self.requests.append((r, ca))
        return None


def _run_policy(cls, kwargs, cluster_args, eng):
    cluster, tasks = wide_cases.dropin_cluster(*cluster_args)
    sched = cls(None, cluster, seed=21, **kwargs)
    sched.engine = eng
    sched._update_resource_info()
    resc = sched.resource_info
    out = sched.schedule(list(tasks))
    hidx = {h.id: i for i, h in enumerate(cluster.hosts)}
    placement = [-1 if t.placement is None else hidx[t.placement] for t in tasks]
    pos = {id(t): i for i, t in enumerate(tasks)}
    after = np.array([resc[h.id] for h in cluster.hosts], dtype=np.float64).T
    st = sched.randomizer.get_state()
    return placement, [pos[id(t)] for t in out], after, (st[1].copy(), st[2])


def test_host_batch_of_mixed_policies_at_65_zones(engine):
    """pvt_place_host_batch: one round of every policy plus one fused cost_aware round (grouping,
    anchors and draws on the device), each against its own CPU result."""
    rec = _Recorder()
    want = _run_policy(policies.CostAwareGlobalScheduler, dict(bin_pack_algo="best-fit", sort_tasks=True),
                       (65, 135, 40, 800, 5), rec)
    (fr, fca), = rec.requests
    rounds = [wide_cases.contended_round(m, 65, 135 + i, 300 + 11 * i, 40000.0, 60 + i)
              for i, m in enumerate(ALL_MODES)]
    refs = [oracle.place(r) for r in rounds]
    got = engine.place_host_batch([(wide_cases.fresh(r), None) for r in rounds[:2]] + [(fr, fca)] +
                                  [(wide_cases.fresh(r), None) for r in rounds[2:]])
    fused = got.pop(2)
    for i, (g, ref) in enumerate(zip(got, refs)):
        _same(g, ref, "round %d mode %d" % (i, rounds[i].mode))
    assert not isinstance(fused, Exception), fused
    res, _, mt = fused
    assert res.placement.tolist() == want[0]
    assert np.array_equal(res.avail, want[2])
    assert np.array_equal(mt[:624], want[3][0]) and int(mt[624]) == want[3][1]
    assert 0.1 <= (res.placement >= 0).mean() <= 0.9


DROPIN = [
    (policies.CostAwareGlobalScheduler, dict(bin_pack_algo="first-fit", sort_hosts=True, sort_tasks=True)),
    (policies.CostAwareGlobalScheduler, dict(bin_pack_algo="best-fit", sort_tasks=True)),
    (policies.CostAwareGlobalScheduler, dict(bin_pack_algo="first-fit", host_decay=True)),
    (policies.OpportunisticGlobalScheduler, {}),
    (policies.FirstFitGlobalScheduler, dict(decreasing=True)),
    (policies.BestFitGlobalScheduler, dict(decreasing=True)),
]


class _TwoCall:
    """The GPU engine without the fused call: the policy takes anchor + place."""

    def __init__(self, eng):
        self.place, self.anchor = eng.place, eng.anchor


@pytest.mark.parametrize("cls,kwargs", DROPIN)
def test_dropin_policies_on_a_40_zone_cluster(engine, cls, kwargs):
    """The four policy classes on a 40-zone cluster of the fakes classes, through the engine (the
    fused place_cost_aware path, and the anchor + place path) and through the oracle-backed
    engine: placements, returned order, snapshot and RandomState must agree."""
    sched_kwargs = dict(kwargs)
    want = _run_policy(cls, sched_kwargs, (40, 85, 30, 400, 9), OracleEngine())
    assert 0.1 <= np.mean([p >= 0 for p in want[0]]) <= 0.9
    for eng in (engine, _TwoCall(engine)):
        got = _run_policy(cls, sched_kwargs, (40, 85, 30, 400, 9), eng)
        assert got[0] == want[0] and got[1] == want[1]
        assert np.array_equal(got[2], want[2])
        assert np.array_equal(got[3][0], want[3][0]) and got[3][1] == want[3][1]


@pytest.fixture(scope="module")
def engines(engine):
    from pivot_place.engine import PlacementEngine
    return [engine, PlacementEngine(0), PlacementEngine(0)]


@pytest.mark.parametrize("mode", ALL_MODES)
def test_sharded_lockstep_at_65_zones(engines, mode):
    """pvt_shard_begin / score / commit: three contexts on the one GPU, 5000 hosts."""
    from pivot_place.sharded import place_lockstep
    r, ref = wide_cases.case(mode, 65, "large")
    outs = place_lockstep(engines, wide_cases.fresh(r))
    for k, o in enumerate(outs):
        _same(o, ref, "shard %d" % k)


def test_content_checks_at_512_zones(engine):
    r, _ = wide_cases.case(_abi.PVT_CA_BF, 512)
    assert engine.check(DeviceRound(wide_cases.fresh(r), engine.device)).code == _abi.PVT_CHK_OK
    bad = wide_cases.fresh(r)
    bad.zone = r.zone.copy()
    bad.zone[777] = 512
    rep = engine.check(DeviceRound(bad, engine.device))
    assert (rep.code, rep.index, rep.count) == (_abi.PVT_CHK_ZONE, 777, 1)
    bad = wide_cases.fresh(r)
    bad.cost = r.cost.copy()
    bad.cost[300, 411] = -5.0                          # the pair (300, 411) and its mirror
    rep = engine.check(DeviceRound(bad, engine.device))
    assert (rep.code, rep.index, rep.count) == (_abi.PVT_CHK_COST, 300 * 512 + 411, 2)
    assert rep.value == bad.cost[300, 411] + bad.cost[411, 300]
    reps = engine.check_batch(DeviceBatch([wide_cases.fresh(r), bad], engine.device))
    assert [x.code for x in reps] == [_abi.PVT_CHK_OK, _abi.PVT_CHK_COST]
    assert reps[1].index == 300 * 512 + 411


def test_bounds(engine):
    assert engine.lib.pvt_max_zones() == 512 == _abi.PVT_MAX_ZONES
    Z = 513
    r = synthetic.make_round(_abi.PVT_CA_BF, 600, 50, seed=1, n_zones=40)
    rs = np.random.RandomState(0)
    r.cost = np.ascontiguousarray(rs.uniform(0.0, 1.0, size=(Z, Z)))
    r.bw = np.ascontiguousarray(rs.uniform(1.0, 2.0, size=(Z, Z)))
    assert r.n_zones == Z
    before = r.avail.copy()
    with pytest.raises(Exception, match="512"):
        engine.place(r)                                # pvt_place_host*
    assert np.array_equal(r.avail, before)
    dr = DeviceRound(r, engine.device)
    dr.placement.fill_(-7)
    dr.order.fill_(-7)
    rc = engine.lib.pvt_place(engine.ctx, ctypes.addressof(dr.struct))
    assert rc == _abi.PVT_EINVAL
    assert b"512" in engine.lib.pvt_last_error(engine.ctx)
    assert bool((dr.placement == -7).all()) and bool((dr.order == -7).all())
    assert np.array_equal(dr.avail.cpu().numpy(), before)
    rep = _abi.pvt_check_report()
    assert engine.lib.pvt_check_round(engine.ctx, ctypes.addressof(dr.struct), ctypes.byref(rep)) == _abi.PVT_EINVAL
