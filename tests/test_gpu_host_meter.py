"""pvt_host_meter_apply / pvt_host_meter_finish (PlacementEngine.host_meter_apply, _finish) and a
metered ResidentCluster on the device, against ``pivot_place.hostops.apply_meter_ops`` byte for
byte, and against the reference meter's recorded series."""
import numpy as np
import pytest
import torch

import host_meter_cases as mc
from pivot_place import hostops
from pivot_place.meter import pack_usage, usage_series

pytestmark = pytest.mark.gpu

SENTINEL = -12345


def _dev(engine, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(engine.device)


class Run:
    """A case's state on the device: capacity, level and a DeviceMeter."""

    def __init__(self, engine, c, log_capacity=None):
        self.engine, self.c = engine, c
        H, K = c["capacity"].shape[1], len(c["op_host"])
        self.cap = _dev(engine, c["capacity"].ravel())
        self.level = _dev(engine, c["level0"].ravel())
        self.m = hostops.DeviceMeter(torch, engine.device, H, log_capacity or max(K, 1))

    def apply(self, lo=0, hi=None, c=None, ok=None):
        c = self.c if c is None else c
        hi = len(c["op_host"]) if hi is None else hi
        args = (self.m, self.cap, self.level, _dev(self.engine, c["op_host"][lo:hi]),
                _dev(self.engine, c["op_kind"][lo:hi]),
                _dev(self.engine, c["op_amt"][:, lo:hi].ravel()),
                _dev(self.engine, c["op_time"][lo:hi]))
        if ok is not None:
            return self.engine.host_meter_apply_into(*args, ok)
        self.m.reserve(hi - lo)
        return self.engine.host_meter_apply(*args).cpu().numpy()

    def finish(self):
        return {k: v.cpu().numpy() for k, v in self.engine.host_meter_finish(self.m).items()}

    def snapshot(self):
        """Everything a call may write, as bytes."""
        m = self.m
        return tuple(t.cpu().numpy().tobytes() for t in (
            self.level, m.st_word, m.st_start, m.st_end, m.iv_host, m.iv_start, m.iv_end,
            m.us_host, m.us_time, m.us_frac)) + (m.n_iv, m.n_us, m.last_time)


def _assert_state(run, level, state):
    m = run.m
    assert run.level.cpu().numpy().tobytes() == level.tobytes()
    word, start, end = state.words()
    assert m.st_word.cpu().numpy().tobytes() == word.tobytes()
    assert m.st_start.cpu().numpy().tobytes() == start.tobytes()
    assert m.st_end.cpu().numpy().tobytes() == end.tobytes()
    assert (m.n_iv, m.n_us, m.last_time) == (state.n_final, state.n_usage, state.last_time)
    # the raw logs: one host's records in its log order
    n = m.n_us
    us_host, us_time = m.us_host[:n].cpu().numpy(), m.us_time[:n].cpu().numpy()
    us_frac = m.us_frac[:4 * n].cpu().numpy().reshape(n, 4)
    iv_host = m.iv_host[:m.n_iv].cpu().numpy()
    iv = np.stack([m.iv_start[:m.n_iv].cpu().numpy(), m.iv_end[:m.n_iv].cpu().numpy()], axis=1)
    for h in range(state.n_hosts):
        recs = np.array(state.usage[h], dtype=np.float64).reshape(-1, 5)
        assert us_time[us_host == h].tobytes() == recs[:, 0].tobytes(), h
        assert us_frac[us_host == h].tobytes() == np.ascontiguousarray(recs[:, 1:]).tobytes(), h
        final = [v for v in state.intervals[h][:-1]]
        assert iv[iv_host == h].tolist() == final, h


def _assert_finished(got, want):
    for k in want:
        assert got[k].dtype == want[k].dtype, k
        assert got[k].tobytes() == want[k].tobytes(), k


@pytest.mark.parametrize("name", mc.NAMES)
def test_kernels_equal_apply_meter_ops(engine, name):
    c = mc.case(name)
    level, want_ok, state = mc.expected(c)
    run = Run(engine, c)
    ok = run.apply()
    assert ok.dtype == np.int32 and ok.tobytes() == want_ok.tobytes()
    _assert_state(run, level, state)
    if name in mc.OPEN_AT_END:
        before = run.snapshot()
        with pytest.raises(RuntimeError, match=r"EINVAL.*1 host\(s\) with an open interval.*host 0"):
            run.finish()
        assert run.snapshot() == before
        return
    _assert_finished(run.finish(), state.finish())


@pytest.mark.parametrize("name", ["churn_5_600", "churn_1_4097", "churn_40_3000", "table_mixed"])
def test_cut_into_two_calls(engine, name):
    """Cuts inside a host's segment and inside an open interval give the one-call result."""
    c = mc.case(name)
    level, want_ok, state = mc.expected(c)
    K = len(c["op_host"])
    trial = hostops.HostMeterState(state.n_hosts)
    opened = None
    for k in range(K):                       # the first entry after which an interval is open
        hostops.apply_meter_ops(c["capacity"], c["level0"].copy(), trial, c["op_host"][k:k + 1],
                                c["op_kind"][k:k + 1], np.zeros((4, 1)), c["op_time"][k:k + 1])
        if trial.words()[0].max() == 1 and k > 2:
            opened = k + 1
            break
    assert opened is not None
    inside = int(np.flatnonzero(c["op_host"] == c["op_host"][0])[1])
    want = state.finish()
    for cut in sorted({1, inside, opened, K // 2, K - 1}):
        run = Run(engine, c, log_capacity=64)
        a, b = run.apply(0, cut), run.apply(cut, K)
        assert np.concatenate([a, b]).tobytes() == want_ok.tobytes(), cut
        _assert_state(run, level, state)
        _assert_finished(run.finish(), want)


def test_finish_twice_and_finish_between_calls(engine):
    c = mc.case("two_phases")
    _, _, state = mc.expected(c)
    K, cut = len(c["op_host"]), c["phase_cut"]
    _, _, half = mc.run(dict(c, **{k: c[k][..., :cut] for k in ("op_host", "op_kind", "op_time",
                                                                 "op_amt")}))
    run = Run(engine, c, log_capacity=64)
    run.apply(0, cut)
    before = run.snapshot()
    first, second = run.finish(), run.finish()
    _assert_finished(first, half.finish())
    _assert_finished(second, first)
    assert run.snapshot() == before                           # finish writes nothing of the meter
    run.apply(cut, K)
    _assert_finished(run.finish(), state.finish())
    assert run.m.us_cap > 64                                  # the logs grew on the way


def test_same_run_twice_is_bit_identical(engine):
    c = mc.case("churn_40_3000")
    outs = []
    for _ in range(2):
        run = Run(engine, c)
        ok = run.apply()
        f = run.finish()
        outs.append((ok.tobytes(),) + tuple(f[k].tobytes() for k in sorted(f)))
    assert outs[0] == outs[1]


def test_full_log_is_refused_with_nothing_written(engine):
    c = mc.case("churn_5_600")
    run = Run(engine, c, log_capacity=64)
    run.m.reserve(64)
    run.apply(0, 64)
    before = run.snapshot()
    ok = torch.full((100,), SENTINEL, dtype=torch.int32, device=engine.device)
    with pytest.raises(RuntimeError, match=r"EINVAL.*logs are full"):
        run.apply(64, 164, ok=ok)                             # (apply_into does not grow them)
    assert run.snapshot() == before and (ok.cpu().numpy() == SENTINEL).all()


@pytest.mark.parametrize("what", [v[0] for v in mc.violations(mc.case("churn_5_600"))])
def test_contract_violation_writes_nothing(engine, what):
    c = mc.case("churn_5_600")
    (k, bad), = [(v[1], v[2]) for v in mc.violations(c) if v[0] == what]
    K = len(c["op_host"])
    run = Run(engine, c)
    before = run.snapshot()
    ok = torch.full((K,), SENTINEL, dtype=torch.int32, device=engine.device)
    with pytest.raises(RuntimeError, match=r"EINVAL.*entry %d of the metered op log" % k):
        run.apply(c=bad, ok=ok)
    assert run.snapshot() == before and (ok.cpu().numpy() == SENTINEL).all()
    # the context takes the valid log afterwards
    level, want_ok, state = mc.expected(c)
    assert run.apply().tobytes() == want_ok.tobytes()
    _assert_state(run, level, state)


def test_time_below_the_last_call_writes_nothing(engine):
    c = mc.case("churn_5_600")
    run = Run(engine, c)
    run.apply(0, 300)
    before = run.snapshot()
    early = dict(c, op_time=np.full(len(c["op_host"]), np.nextafter(run.m.last_time, -np.inf)))
    ok = torch.full((2,), SENTINEL, dtype=torch.int32, device=engine.device)
    with pytest.raises(RuntimeError, match=r"EINVAL.*entry 0 of the metered op log"):
        run.apply(0, 2, c=early, ok=ok)
    assert run.snapshot() == before and (ok.cpu().numpy() == SENTINEL).all()


def test_old_entry_point_refuses_marks(engine):
    c = mc.case("churn_5_600")
    K = len(c["op_host"])
    level = _dev(engine, c["level0"].ravel())
    ok = torch.full((K,), SENTINEL, dtype=torch.int32, device=engine.device)
    first = int(np.flatnonzero(c["op_kind"] >= hostops.CHECK_IN)[0])
    with pytest.raises(RuntimeError, match=r"EINVAL.*op %d " % first):
        engine.host_ops_into(_dev(engine, c["capacity"].ravel()), level, _dev(engine, c["op_host"]),
                             _dev(engine, c["op_kind"]), _dev(engine, c["op_amt"].ravel()), ok)
    assert level.cpu().numpy().tobytes() == c["level0"].tobytes()
    assert (ok.cpu().numpy() == SENTINEL).all()


def test_walk_is_timed_under_its_own_name(engine):
    c = mc.case("table_mixed")
    engine.set_profiling(2, "host_meter_kernel")
    engine.reset_kstats()
    try:
        Run(engine, c).apply()
        assert engine.kernel_kstats("host_meter_kernel")["launches"] == 1
    finally:
        engine.set_profiling(False)


def _cluster(engine, t, **kw):
    H = t["capacity"].shape[1]
    return hostops.ResidentCluster(engine, t["capacity"], np.zeros(H, np.int32), np.zeros((1, 1)),
                                   np.ones((1, 1)), **kw)


@pytest.mark.parametrize("name", mc.RUNS)
def test_metered_cluster_gives_the_reference_series(engine, name):
    t = mc.fixture()[name]
    ref = mc.reference()[name]
    K = len(t["op_host"])
    rc = _cluster(engine, t, meter=True, meter_log_capacity=64)
    start = rc.bytes_uploaded
    cuts = mc.cuts_of(t)
    assert 30 <= len(cuts) <= 60
    oks, lo = [], 0
    for hi in cuts + [K]:
        oks.append(rc.apply(t["op_host"][lo:hi], t["op_kind"][lo:hi], t["op_amt"][:, lo:hi],
                            op_time=t["op_time"][lo:hi]))
        lo = hi
    assert np.concatenate(oks).tobytes() == t["op_ok"].tobytes()
    assert rc.bytes_uploaded - start == K * (4 + 4 + 32 + 8)   # the log and its times, no more
    level, _, state = mc.expected(t)
    assert rc.levels().tobytes() == level.tobytes()
    fin = {k: v.cpu().numpy() for k, v in rc.meter_log().items()}
    want = state.finish()
    _assert_finished(dict(fin, us_frac=fin["us_frac"].reshape(4, -1)), want)
    rows = mc.rows_by_index(ref["hosts"])
    for s in (100, 7, 1000):
        got = rc.usage(s)
        mc.assert_series(got, ref["want"][str(s)])
        # the upload path on the same rows in host-index order: bit-identical
        up = usage_series(engine.meter_usage(pack_usage([rows], s)), s)[0]
        assert got["hosts"] == up["hosts"]
        for r in ("cpus", "mem", "disk", "gpus"):
            assert got[r][0] == up[r][0]
            assert np.array(got[r][1]).tobytes() == np.array(up[r][1]).tobytes(), (s, r)
        assert got["avg"].tobytes() == up["avg"].tobytes()
    hours = mc.instance_hours(ref["hosts"])
    assert abs(rc.instance_hours() - hours) <= 1e-9 * abs(hours)
    assert rc.bytes_uploaded - start == K * 48 + 4 * 32   # and four times a scenario's offsets
