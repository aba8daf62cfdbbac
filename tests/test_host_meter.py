"""Metering the resident cluster on the CPU: ``apply_meter_ops`` against the reference meter's
recorded intervals, usage records and per-mark rows, the table row by row, the contract, the ABI
structs and a metered ``ResidentCluster`` over a fake engine."""
import ctypes

import numpy as np
import pytest

import host_meter_cases as mc
from pivot_place import _abi, hostops
from pivot_place.hostops import CHECK_IN, CHECK_OUT, HostMeterState, ResidentCluster, apply_meter_ops


def _assert_reference(name, state):
    ref = mc.reference()[name]["hosts"]
    assert sorted(h["host"] for h in ref) == [h for h in range(state.n_hosts) if state.usage[h]]
    for h in ref:
        i = h["host"]
        assert state.intervals[i] == h["intervals"], i
        assert [u[0] for u in state.usage[i]] == h["times"], i
        for r in range(4):
            assert [u[1 + r] for u in state.usage[i]] == h["usage"][r], (i, r)
    assert not any(state.intervals[i] for i in range(state.n_hosts)
                   if i not in {h["host"] for h in ref})


@pytest.mark.parametrize("name", mc.RUNS)
def test_fixture_log_gives_the_reference_meter(name):
    t = mc.fixture()[name]
    assert len(t["op_host"]) == 30536 and int((t["op_kind"] >= CHECK_IN).sum()) == 15268
    level, ok, state = mc.expected(t)
    assert ok.tobytes() == t["op_ok"].tobytes()
    _assert_reference(name, state)
    # cut into calls at the fixture's round counts: the same, bit for bit
    cuts = sorted({m for m in t["round_ops"] if 0 < m < len(t["op_host"])})
    assert len(cuts) > 100
    level2, ok2, state2 = mc.run(t, cuts)
    assert ok2.tobytes() == ok.tobytes() and level2.tobytes() == level.tobytes()
    assert state2.intervals == state.intervals and state2.usage == state.usage
    assert state2.last_time == state.last_time == t["op_time"][-1]
    f, f2 = state.finish(), state2.finish()
    assert all(f[k].tobytes() == f2[k].tobytes() for k in f)


def test_fixture_covers_the_table():
    """Every row but the check-out before any check-in occurs in the recorded runs."""
    for name in mc.RUNS:
        t = mc.fixture()[name]
        assert set(t["op_ok"][t["op_kind"] == CHECK_IN]) == {1, 2, 3, 4}
        assert set(t["op_ok"][t["op_kind"] == CHECK_OUT]) == {1, 2, 3}


def test_metered_log_leaves_the_levels_of_apply_ops():
    """The marks change no level: the ops alone through apply_ops give the same levels."""
    t = mc.fixture()["sim_h12_opportunistic"]
    level, ok, _ = mc.expected(t)
    ops = t["op_kind"] < CHECK_IN
    plain = t["capacity"].copy()
    ok0 = hostops.apply_ops(t["capacity"], plain, t["op_host"][ops], t["op_kind"][ops],
                            t["op_amt"][:, ops])
    assert plain.tobytes() == level.tobytes() and ok0.tobytes() == ok[ops].tobytes()


@pytest.mark.parametrize("name", mc.NAMES)
def test_synthetic_cases_build(name):
    c = mc.case(name)
    level, ok, state = mc.expected(c)
    marks = c["op_kind"] >= CHECK_IN
    assert state.n_usage == int(marks.sum())
    word, start, end = state.words()
    for h, ivs in enumerate(state.intervals):
        assert word[h] == (0 if not ivs else len(ivs[-1]))
        assert (start[h], end[h]) == ((0.0, 0.0) if not ivs else
                                      (ivs[-1][0], ivs[-1][1] if len(ivs[-1]) == 2 else 0.0))
    if name in mc.OPEN_AT_END:
        with pytest.raises(ValueError, match=r"1 host\(s\) with an open interval.*host 0"):
            state.finish()
        return
    f = state.finish()
    R = len(f["row_host"])
    assert f["row_host"].tolist() == [h for h in range(state.n_hosts) if state.usage[h]]
    assert f["iv_off"][R] == len(f["iv_start"]) == state.n_final + int((word == 2).sum())
    assert f["us_off"][R] == len(f["us_time"]) == state.n_usage
    assert f["us_frac"].shape == (4, state.n_usage)


def test_usage_is_used_over_total_at_that_point_of_the_log():
    c = mc.case("row_out_open")                  # check-in, subscribe D, check-out
    _, _, state = mc.expected(c)
    assert state.usage[0][0] == (1.0, 0.0, 0.0, 0.0, 0.0)
    want = tuple((mc.CAP[r] - (mc.CAP[r] - mc.D[r])) / mc.CAP[r] for r in range(4))
    assert state.usage[0][1] == (2.0,) + want and want[0] == 0.125


def test_finish_changes_nothing_and_may_be_repeated():
    c = mc.case("two_phases")
    K, cut = len(c["op_host"]), c["phase_cut"]
    one = mc.expected(c)[2].finish()
    level = c["level0"].copy()
    state = HostMeterState(c["capacity"].shape[1])
    apply_meter_ops(c["capacity"], level, state, c["op_host"][:cut], c["op_kind"][:cut],
                    c["op_amt"][:, :cut], c["op_time"][:cut])
    kept = ([list(map(list, v)) for v in state.intervals], [list(u) for u in state.usage])
    a, b = state.finish(), state.finish()
    assert all(a[k].tobytes() == b[k].tobytes() for k in a)
    assert kept == ([list(map(list, v)) for v in state.intervals], [list(u) for u in state.usage])
    assert len(a["iv_start"]) < len(one["iv_start"])
    apply_meter_ops(c["capacity"], level, state, c["op_host"][cut:], c["op_kind"][cut:],
                    c["op_amt"][:, cut:], c["op_time"][cut:])
    two = state.finish()
    assert all(one[k].tobytes() == two[k].tobytes() for k in one)


@pytest.mark.parametrize("what", [v[0] for v in mc.violations(mc.case("churn_5_600"))])
def test_contract_violations_raise_before_anything_changes(what):
    c = mc.case("churn_5_600")
    (k, bad), = [(v[1], v[2]) for v in mc.violations(c) if v[0] == what]
    level = c["level0"].copy()
    state = HostMeterState(5)
    with pytest.raises(ValueError, match=r"entry %d of the metered op log" % k):
        apply_meter_ops(bad["capacity"], level, state, bad["op_host"], bad["op_kind"],
                        bad["op_amt"], bad["op_time"])
    assert level.tobytes() == c["level0"].tobytes()
    assert state.n_usage == 0 and state.last_time == 0.0 and not any(state.intervals)


def test_time_below_the_last_call_and_bad_capacity_raise():
    c = mc.case("churn_5_600")
    level = c["level0"].copy()
    state = HostMeterState(5)
    cut = 300
    apply_meter_ops(c["capacity"], level, state, c["op_host"][:cut], c["op_kind"][:cut],
                    c["op_amt"][:, :cut], c["op_time"][:cut])
    assert state.last_time == c["op_time"][cut - 1] > 0
    before = (level.copy(), [list(map(list, v)) for v in state.intervals], state.n_usage)
    early = np.full(2, np.nextafter(state.last_time, -np.inf))
    with pytest.raises(ValueError, match="entry 0 of the metered op log"):
        apply_meter_ops(c["capacity"], level, state, c["op_host"][:2], c["op_kind"][:2],
                        c["op_amt"][:, :2], early)
    cap = c["capacity"].copy()
    k = int(np.flatnonzero(c["op_host"][cut:] != c["op_host"][cut])[0])
    cap[3, c["op_host"][cut + k]] = 0.0
    with pytest.raises(ValueError, match="entry %d of the metered op log" % k):
        apply_meter_ops(cap, level, state, c["op_host"][cut:], c["op_kind"][cut:],
                        c["op_amt"][:, cut:], c["op_time"][cut:])
    assert level.tobytes() == before[0].tobytes() and state.n_usage == before[2]
    assert [list(map(list, v)) for v in state.intervals] == before[1]
    # and the old entry point still refuses a mark
    with pytest.raises(ValueError, match="op 1 of the host op log"):
        hostops.apply_ops(c["capacity"], level, c["op_host"][:2], c["op_kind"][:2],
                          c["op_amt"][:, :2])


def test_struct_layout_and_constants():
    assert (_abi.CHECK_IN, _abi.CHECK_OUT) == (2, 3) == (CHECK_IN, CHECK_OUT)
    assert (_abi.METER_NONE, _abi.METER_OPEN, _abi.METER_CLOSED) == (0, 1, 2)
    assert _abi.PVT_ABI_VERSION == 3
    m = _abi.pvt_host_meter
    want = ["n_hosts", "reserved", "capacity", "level", "st_word", "st_start", "st_end", "iv_cap",
            "us_cap", "iv_host", "iv_start", "iv_end", "us_host", "us_time", "us_frac", "n_iv",
            "n_us", "last_time"]
    assert [f[0] for f in m._fields_] == want
    assert [getattr(m, n).offset for n in want] == [0, 4] + list(range(8, 8 * 17, 8))
    assert ctypes.sizeof(m) == 136
    o = _abi.pvt_host_meter_ops
    assert [f[0] for f in o._fields_] == ["n_ops", "reserved", "op_host", "op_kind", "op_amt",
                                          "op_time", "op_ok"]
    assert ctypes.sizeof(o) == 48 and o.op_host.offset == 8 and o.op_ok.offset == 40
    r = _abi.pvt_host_meter_out
    assert [f[0] for f in r._fields_] == ["row_host", "iv_off", "iv_start", "iv_end", "us_off",
                                          "us_time", "us_frac", "n_rows", "n_iv", "n_us"]
    assert ctypes.sizeof(r) == 80 and r.n_rows.offset == 56
    # the header declares what the binding mirrors
    import os
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                           "include", "pivot_place.h")) as f:
        text = f.read()
    for name in ("pvt_host_meter_apply", "pvt_host_meter_finish", "} pvt_host_meter;",
                 "} pvt_host_meter_ops;", "} pvt_host_meter_out;"):
        assert name in text, name
    assert "#define PVT_ABI_VERSION 3" in text.replace("  ", " ")
    # the header's field names, in order, are the binding's
    import re
    for name, struct in (("pvt_host_meter", m), ("pvt_host_meter_ops", o), ("pvt_host_meter_out", r)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [re.split(r"[\s*]+", n.strip(" *"))[-1] for decl in body.split(";")
                 if decl.strip() for n in decl.split(",")]
        assert names == [f[0] for f in struct._fields_], name
    # the built library exports the entry points and rejects NULL without a device
    from pivot_place import engine
    lib = engine.load_library()
    assert lib.pvt_host_meter_apply(None, None, None) == _abi.PVT_EINVAL
    assert lib.pvt_host_meter_finish(None, None, None) == _abi.PVT_EINVAL


def _cluster(engine, t, **kw):
    H = t["capacity"].shape[1]
    return ResidentCluster(engine, t["capacity"], np.zeros(H, np.int32), np.zeros((1, 1)),
                           np.ones((1, 1)), **kw)


def test_metered_resident_cluster_over_a_fake_engine():
    name = "sim_h12_opportunistic"
    t = mc.fixture()[name]
    K = len(t["op_host"])
    eng = mc.FakeMeterEngine()
    rc = _cluster(eng, t, meter=True, meter_log_capacity=64)
    start = rc.bytes_uploaded
    lo = 0
    oks = []
    for hi in mc.cuts_of(t) + [K]:
        oks.append(rc.apply(t["op_host"][lo:hi], t["op_kind"][lo:hi], t["op_amt"][:, lo:hi],
                            op_time=t["op_time"][lo:hi]))
        lo = hi
    assert np.concatenate(oks).tobytes() == t["op_ok"].tobytes()
    assert rc.bytes_uploaded - start == K * (4 + 4 + 32 + 8)          # the log and its times
    assert rc.meter.us_cap >= rc.meter.n_us == 15268 and eng.applied[0][1] > 64
    assert rc.levels().tobytes() == mc.expected(t)[0].tobytes()
    fin = rc.meter_log()
    want = mc.expected(t)[2].finish()
    assert all(fin[k].numpy().tobytes() == want[k].tobytes() for k in want)
    ref = mc.reference()[name]
    for s in (100, 7, 1000):
        mc.assert_series(rc.usage(s), ref["want"][str(s)])
    assert rc.instance_hours() == pytest.approx(mc.instance_hours(ref["hosts"]), rel=1e-9)
    assert rc.bytes_uploaded - start == K * 48 + 4 * 32                         # nothing more went up


def test_resident_cluster_without_meter_is_unchanged():
    t = mc.fixture()["sim_h12_opportunistic"]
    eng = mc.FakeMeterEngine()
    rc = _cluster(eng, t)
    assert rc.meter is None
    ops = t["op_kind"] < CHECK_IN
    with pytest.raises(ValueError, match="not metered"):
        rc.apply(t["op_host"][:4], t["op_kind"][:4], t["op_amt"][:, :4], op_time=t["op_time"][:4])
    with pytest.raises(ValueError, match="not metered"):
        rc.meter_log()
    first = int(np.flatnonzero(~ops)[0])
    with pytest.raises(ValueError, match="op %d of the host op log" % first):     # a mark: refused
        rc.apply(t["op_host"][:4], t["op_kind"][:4], t["op_amt"][:, :4])
    ok = rc.apply(t["op_host"][ops][:500], t["op_kind"][ops][:500], t["op_amt"][:, ops][:, :500])
    assert ok.tobytes() == t["op_ok"][ops][:500].tobytes()
    metered = _cluster(eng, t, meter=True)
    with pytest.raises(ValueError, match="needs op_time"):
        metered.apply(t["op_host"][:4], t["op_kind"][:4], t["op_amt"][:, :4])
    with pytest.raises(ValueError, match="sample_size"):
        metered.usage(2.5)
