"""Host accounting between rounds, on the CPU: ``pivot_place.hostops.apply_ops`` against the ops
and snapshots of recorded reference simulations (tests/golden/host_ops.json.gz), the case
builders' own assertions, and ``ResidentCluster``'s round loop over a fake engine (apply_ops and
the CPU restatement of the policies)."""
import numpy as np
import pytest

import golden_io
import hostops_cases as hc
from pivot_place import hostops


def test_fixture_traces():
    fx = hc.fixture()
    assert tuple(fx) == hc.TRACES
    for name, t in fx.items():
        tr, cases = golden_io.sim_rounds(name)
        assert t["capacity"].shape == (4, tr["n_hosts"])
        assert len(t["round_ops"]) == len(cases)
        assert t["round_ops"] == sorted(t["round_ops"]) and t["round_ops"][-1] <= len(t["op_host"])
        # the reference's runs hold no refused subscribe (a refused one never finishes)
        assert t["op_ok"][t["op_kind"] == hostops.SUBSCRIBE].all()


@pytest.mark.parametrize("name", hc.TRACES)
def test_apply_ops_reproduces_reference(name):
    """Every op's result and every recorded round's snapshot, bit for bit; and the trace holds
    put-backs the reference skipped, so the rule differs from ``level += d`` on it."""
    t = hc.fixture()[name]
    _, cases = golden_io.sim_rounds(name)
    level = t["capacity"].copy()
    plain = t["capacity"].copy()            # what `level -= d` / `level += d` would give
    done = 0
    for k, (case, m) in enumerate(zip(cases, t["round_ops"])):
        ok = hostops.apply_ops(t["capacity"], level, t["op_host"][done:m], t["op_kind"][done:m],
                               t["op_amt"][:, done:m])
        assert np.array_equal(ok, t["op_ok"][done:m]), "round %d" % k
        assert np.array_equal(level, hc.snapshot(case)), "round %d" % k
        for j in range(done, m):
            sign = -1.0 if t["op_kind"][j] == hostops.SUBSCRIBE else 1.0
            plain[:, t["op_host"][j]] += sign * t["op_amt"][:, j]
        done = m
    rest = hostops.apply_ops(t["capacity"], level, t["op_host"][done:], t["op_kind"][done:],
                             t["op_amt"][:, done:])
    assert np.array_equal(rest, t["op_ok"][done:])
    un = t["op_kind"] == hostops.UNSUBSCRIBE
    missed = sum(int(((t["op_amt"][r] > 0) & un & (((t["op_ok"] >> r) & 1) == 0)).sum())
                 for r in range(4))
    assert missed == t["skipped_putbacks"] >= 1
    assert not np.array_equal(plain, hc.snapshot(cases[-1]))


@pytest.mark.parametrize("name", hc.NAMES)
def test_case_builders(name):
    """The builders' own assertions hold, and the checker is a function of its inputs."""
    c = hc.case(name)
    level, ok = hc.expected(c)
    again, ok2 = hc.run(c)
    assert level.tobytes() == again.tobytes() and ok.tobytes() == ok2.tobytes()
    assert ok.dtype == np.int32 and len(ok) == len(c["op_host"])
    if name == "rounding_skips":
        assert hc.skipped(c) >= 10


def test_apply_ops_cut_anywhere():
    c = hc.case("skewed_12_3000")
    level, ok = hc.expected(c)
    for cut in (0, 1, 1499, 3000):
        lv = c["level0"].copy()
        a = hostops.apply_ops(c["capacity"], lv, c["op_host"][:cut], c["op_kind"][:cut],
                              c["op_amt"][:, :cut])
        b = hostops.apply_ops(c["capacity"], lv, c["op_host"][cut:], c["op_kind"][cut:],
                              c["op_amt"][:, cut:])
        assert lv.tobytes() == level.tobytes()
        assert np.concatenate([a, b]).tobytes() == ok.tobytes()


@pytest.mark.parametrize("host,kind", [(-1, 0), (3, 1), (0, 2)])
def test_apply_ops_invalid_log_changes_nothing(host, kind):
    cap = hc._caps(3)
    level = cap * 0.5
    keep = level.copy()
    amt = np.ones((4, 2))
    with pytest.raises(ValueError, match="op 1 "):
        hostops.apply_ops(cap, level, [1, host], [0, kind], amt)
    assert level.tobytes() == keep.tobytes()


@pytest.mark.parametrize("name", hc.TRACES)
def test_resident_cluster_round_loop(name):
    """ResidentCluster over the fake engine: the recorded placements and orders from levels that
    only the logs change, and a scratch refreshed for just the hosts that can differ."""
    eng = hc.FakeEngine()
    rc, rounds = hc.replay_resident(eng, name)
    assert rounds > 100
    t = hc.fixture()[name]
    _, cases = golden_io.sim_rounds(name)
    # one restore per round after the first log, naming only placed-on or logged hosts
    assert 1 <= len(eng.restored) <= rounds
    done, prev = 0, np.zeros(0, dtype=np.int32)
    calls = iter(eng.restored)
    for case, m in zip(cases, t["round_ops"]):
        named = set(t["op_host"][done:m].tolist()) | set(prev[prev >= 0].tolist())
        if m > done or len(prev):
            got = next(calls)
            assert set(got[got >= 0].tolist()) == named
        prev = np.array(case["runs"][0]["placement"], dtype=np.int32)
        done = m


def test_resident_cluster_policy_commits_stay_in_scratch():
    """A placement changes ``work`` and not ``level``; ``want_avail`` returns the scratch."""
    name = "sim_h12_vbp_ff"
    tr, cases = golden_io.sim_rounds(name)
    t = hc.fixture()[name]
    cost, bw, _ = golden_io.zones()
    rc = hostops.ResidentCluster(hc.FakeEngine(), t["capacity"], tr["zone"], cost, bw,
                                 tiebreak=tr["id_rank"])
    m = t["round_ops"][0]
    rc.apply(t["op_host"][:m], t["op_kind"][:m], t["op_amt"][:, :m])
    r = golden_io.run_arrays(cases[0], cases[0]["runs"][0])
    res = rc.place(r, want_avail=True)
    _, _, avail, _ = golden_io.expected(cases[0], cases[0]["runs"][0])
    assert np.array_equal(res.avail, avail)
    assert np.array_equal(rc.levels(), hc.snapshot(cases[0]))
    assert not np.array_equal(res.avail, rc.levels())
    assert rc.apply([], [], np.zeros((4, 0))).shape == (0,)


def test_header_and_binding_agree():
    """include/pivot_place.h declares the entry point and the struct the ctypes mirror lays out;
    the built library exports it and rejects NULL without a device."""
    import ctypes
    import os
    import re
    from pivot_place import _abi, engine
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "pivot_place.h")).read()
    assert re.search(r"^int\s+pvt_host_ops_apply\(pvt_ctx\* ctx, const pvt_host_ops\* ops\);",
                     text, re.M)
    body = re.search(r"typedef struct pvt_host_ops \{(.*?)\} pvt_host_ops;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip(" *") for decl in body.split(";") if decl.strip()
             for n in decl.split(",")]
    names = [re.split(r"[\s*]+", n)[-1] for n in names]
    assert names == [f[0] for f in _abi.pvt_host_ops._fields_]
    assert ctypes.sizeof(_abi.pvt_host_ops) == 8 + 6 * ctypes.sizeof(ctypes.c_void_p)
    lib = engine.load_library()
    assert lib.pvt_host_ops_apply(None, None) == _abi.PVT_EINVAL
    assert "PVT_ABI_VERSION 3" in re.sub(r"\s+", " ", text)
