"""pvt_host_ops_apply (PlacementEngine.host_ops) and ResidentCluster on the device, against
``pivot_place.hostops.apply_ops`` and the recorded reference simulations, byte for byte."""
import numpy as np
import pytest
import torch

import hostops_cases as hc
from pivot_place import hostops

pytestmark = pytest.mark.gpu

SENTINEL = -12345


def _dev(engine, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(engine.device)


def _log(engine, c, lo=0, hi=None):
    hi = len(c["op_host"]) if hi is None else hi
    return (_dev(engine, c["op_host"][lo:hi]), _dev(engine, c["op_kind"][lo:hi]),
            _dev(engine, c["op_amt"][:, lo:hi].ravel()))


def _apply(engine, c, level, lo=0, hi=None):
    ok = engine.host_ops(_dev(engine, c["capacity"].ravel()), level, *_log(engine, c, lo, hi))
    return ok.cpu().numpy()


@pytest.mark.parametrize("name", hc.NAMES)
def test_kernel_equals_apply_ops(engine, name):
    c = hc.case(name)
    want_level, want_ok = hc.expected(c)
    level = _dev(engine, c["level0"].ravel())
    ok = _apply(engine, c, level)
    assert ok.dtype == np.int32 and ok.tobytes() == want_ok.tobytes()
    assert level.cpu().numpy().tobytes() == want_level.tobytes()


@pytest.mark.parametrize("name", hc.TRACES)
def test_kernel_on_reference_log(engine, name):
    """The whole recorded log in one call, and round by round: the reference's results and
    every recorded snapshot."""
    import golden_io
    t = hc.fixture()[name]
    _, cases = golden_io.sim_rounds(name)
    c = dict(t, level0=t["capacity"])
    whole = _dev(engine, t["capacity"].ravel())
    ok = _apply(engine, c, whole)
    assert ok.tobytes() == t["op_ok"].tobytes()
    level = _dev(engine, t["capacity"].ravel())
    cap = _dev(engine, t["capacity"].ravel())
    host, kind = _dev(engine, t["op_host"]), _dev(engine, t["op_kind"])
    marks = [0] + t["round_ops"]
    step = max(1, len(cases) // 40)          # ~40 of the rounds' snapshots, the last one too
    picks = sorted(set(range(step - 1, len(cases), step)) | {len(cases) - 1})
    done = 0
    for k in picks:
        m = marks[k + 1]
        if m > done:
            amt = _dev(engine, t["op_amt"][:, done:m].ravel())
            got = engine.host_ops(cap, level, host[done:m], kind[done:m], amt).cpu().numpy()
            assert got.tobytes() == t["op_ok"][done:m].tobytes(), "round %d" % k
        done = m
        snap = hc.snapshot(cases[k])
        assert level.cpu().numpy().tobytes() == snap.tobytes(), "round %d" % k
    amt = _dev(engine, t["op_amt"][:, done:].ravel())
    engine.host_ops(cap, level, host[done:], kind[done:], amt)
    assert level.cpu().numpy().tobytes() == whole.cpu().numpy().tobytes()


@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("what", ["host_neg", "host_H", "kind_2"])
def test_invalid_log_writes_nothing(engine, what, where):
    c = hc.case("skewed_12_3000")
    K, H = len(c["op_host"]), c["capacity"].shape[1]
    k = 0 if where == "first" else K - 1
    host, kind = c["op_host"].copy(), c["op_kind"].copy()
    if what == "host_neg":
        host[k] = -1
    elif what == "host_H":
        host[k] = H
    else:
        kind[k] = 2
    level = _dev(engine, c["level0"].ravel())
    ok = torch.full((K,), SENTINEL, dtype=torch.int32, device=engine.device)
    with pytest.raises(RuntimeError, match=r"EINVAL.*op %d " % k):
        engine.host_ops_into(_dev(engine, c["capacity"].ravel()), level, _dev(engine, host),
                             _dev(engine, kind), _dev(engine, c["op_amt"].ravel()), ok)
    assert level.cpu().numpy().tobytes() == c["level0"].tobytes()
    assert (ok.cpu().numpy() == SENTINEL).all()
    # the context takes the valid log afterwards
    want_level, want_ok = hc.expected(c)
    assert _apply(engine, c, level).tobytes() == want_ok.tobytes()
    assert level.cpu().numpy().tobytes() == want_level.tobytes()


@pytest.mark.parametrize("name", ["long_4097", "order_sensitive", "skewed_100_20000"])
def test_cut_into_two_calls(engine, name):
    c = hc.case(name)
    want_level, want_ok = hc.expected(c)
    K = len(c["op_host"])
    inside = int(np.flatnonzero(c["op_host"] == c["op_host"][0])[1])    # inside a host's segment
    for cut in sorted({1, inside, K // 2, K - 1}):
        level = _dev(engine, c["level0"].ravel())
        a = _apply(engine, c, level, 0, cut)
        b = _apply(engine, c, level, cut, K)
        assert np.concatenate([a, b]).tobytes() == want_ok.tobytes(), cut
        assert level.cpu().numpy().tobytes() == want_level.tobytes(), cut


def test_same_call_twice(engine):
    c = hc.case("skewed_4096_50000")
    outs = []
    for _ in range(2):
        level = _dev(engine, c["level0"].ravel())
        ok = _apply(engine, c, level)
        outs.append((ok.tobytes(), level.cpu().numpy().tobytes()))
    assert outs[0] == outs[1]


def test_empty_log_launches_nothing(engine):
    c = hc.case("empty_h5")
    level = _dev(engine, c["level0"].ravel())
    engine.set_profiling(2, "host_ops_kernel")
    engine.reset_kstats()
    try:
        assert _apply(engine, c, level).shape == (0,)
        assert engine.kernel_kstats("host_ops_kernel")["launches"] == 0
        one = hc.case("single_sub")
        _apply(engine, one, _dev(engine, one["level0"].ravel()))
        assert engine.kernel_kstats("host_ops_kernel")["launches"] == 1
    finally:
        engine.set_profiling(False)
    assert level.cpu().numpy().tobytes() == c["level0"].tobytes()


@pytest.mark.parametrize("name", hc.TRACES)
def test_resident_cluster_replays_reference(engine, name):
    """The recorded simulation's round loop on the device: before every round the levels equal
    the recorded snapshot; the placement, the order and (opportunistic) the carried MT19937 state
    equal the recorded ones; a round uploads its task arrays and its log, never a snapshot."""
    rc, rounds = hc.replay_resident(engine, name)
    assert rounds > 100
    assert isinstance(rc, hostops.ResidentCluster)
