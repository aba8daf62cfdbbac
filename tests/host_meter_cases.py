"""Metered host-op logs (pvt_host_meter_apply / pvt_host_meter_finish), checked by
``pivot_place.hostops.apply_meter_ops``, and the reader of tests/golden/host_meter.json.gz.

A case is a hostops_cases case plus ``op_time`` (K,) float64. ``expected(case)`` is the checker's
verdict, computed once: (level after, op_ok, HostMeterState). A builder asserts what makes its
case worth having (that every row of the state machine is taken, that an interval is final).
"""
import functools
import gzip
import json
import os

import numpy as np

from pivot_place.hostops import (CHECK_IN as CIN, CHECK_OUT as COUT, SUBSCRIBE as SUB,
                                 UNSUBSCRIBE as UNSUB, HostMeterState, apply_meter_ops)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CAP = (16.0, 131072.0, 100.0, 1.0)
MEM_UNIT = 7864.32
Z = (0.0, 0.0, 0.0, 0.0)
RUNS = ("sim_c1_cost_aware", "sim_h12_opportunistic", "sim_c1_vbp_bf")


def _caps(H):
    return np.repeat(np.array(CAP)[:, None], H, axis=1)


def _case(name, H, ents):
    """``ents``: (host, kind, time[, amounts])."""
    K = len(ents)
    amt = np.array([e[3] if len(e) > 3 else Z for e in ents], dtype=np.float64).reshape(K, 4)
    return {"name": name, "capacity": _caps(H), "level0": _caps(H),
            "op_host": np.array([e[0] for e in ents], dtype=np.int32),
            "op_kind": np.array([e[1] for e in ents], dtype=np.int32),
            "op_time": np.array([e[2] for e in ents], dtype=np.float64),
            "op_amt": np.ascontiguousarray(amt.T)}


def run(case, cuts=()):
    """apply_meter_ops on a copy of the case's start, the log cut into calls at ``cuts``:
    (level after, op_ok, state)."""
    level = case["level0"].copy()
    state = HostMeterState(level.shape[1])
    K = len(case["op_host"])
    ok, lo = [], 0
    for hi in list(cuts) + [K]:
        ok.append(apply_meter_ops(case["capacity"], level, state, case["op_host"][lo:hi],
                                  case["op_kind"][lo:hi], case["op_amt"][:, lo:hi],
                                  case["op_time"][lo:hi]))
        lo = hi
    return level, np.concatenate(ok) if ok else np.zeros(0, np.int32), state


_EXPECTED = {}


def expected(case):
    if case["name"] not in _EXPECTED:
        _EXPECTED[case["name"]] = run(case)
    return _EXPECTED[case["name"]]


def demand(rng):
    return (float(rng.choice([0.5, 1.0, 1.0, 2.0, 4.0])),
            float(np.round(rng.uniform(0.01, 2.0), 2) * MEM_UNIT),
            float(rng.choice([0.0, 0.0, 1.0])), 0.0)


# ------------------------------------------------------------------------------- the table
D = (2.0, 4096.0, 1.0, 0.0)         # (exact in fp64: its put-back is not skipped by rounding)
# name -> (entries on host 0 of one host, the codes of the marks in order, intervals of host 0)
ROWS = {
    "in_none": ([(0, CIN, 5.0)], [1], [[5.0]]),
    "in_closed_later": ([(0, CIN, 1.0), (0, COUT, 2.0), (0, CIN, 3.0)], [1, 1, 2],
                        [[1.0, 2.0], [3.0]]),
    "in_closed_same": ([(0, CIN, 1.0), (0, COUT, 2.0), (0, CIN, 2.0)], [1, 1, 3], [[1.0]]),
    "in_open": ([(0, CIN, 1.0), (0, CIN, 4.0)], [1, 4], [[1.0]]),
    "out_open": ([(0, CIN, 1.0), (0, SUB, 1.5, D), (0, COUT, 2.0)], [1, 1], [[1.0, 2.0]]),
    "out_closed_later": ([(0, CIN, 1.0), (0, COUT, 2.0), (0, COUT, 2.5)], [1, 1, 2],
                         [[1.0, 2.5]]),
    "out_closed_same": ([(0, CIN, 1.0), (0, COUT, 2.0), (0, COUT, 2.0)], [1, 1, 3],
                        [[1.0, 2.0]]),
    "out_none": ([(0, COUT, 7.0)], [0], []),
}


def table_row(name):
    ents, codes, ivs = ROWS[name]
    c = _case("row_" + name, 1, ents)
    _, ok, st = expected(c)
    assert ok[c["op_kind"] >= CIN].tolist() == codes, (name, ok)
    assert st.intervals[0] == ivs, (name, st.intervals[0])
    assert len(st.usage[0]) == len(codes)
    return c


def table_mixed():
    """Every row of the table on three hosts, interleaved, with subscribes (two of them refused)
    and put-backs between the marks: usage follows the levels as they stand; host 1 checks out
    before any check-in and then never checks in (a row with usage and no interval)."""
    big = (17.0, 1.0, 0.0, 0.0)                     # more cpus than a host has: refused
    ents = [(0, CIN, 0.0), (1, COUT, 0.0), (2, CIN, 0.0),
            (0, SUB, 1.0, D), (2, SUB, 1.0, big), (0, CIN, 1.0),          # in_open
            (0, COUT, 2.0), (2, SUB, 2.0, D), (2, COUT, 2.0),             # out_open twice
            (0, SUB, 2.0, big), (0, CIN, 2.0),                            # in_closed_same
            (0, COUT, 3.0), (0, COUT, 3.0), (0, COUT, 4.0),               # open, same, later
            (2, CIN, 5.0), (2, UNSUB, 5.5, D), (2, COUT, 6.0),            # in_closed_later
            (1, COUT, 6.0), (0, UNSUB, 7.0, D), (0, CIN, 8.0), (0, COUT, 8.0)]
    c = _case("table_mixed", 3, ents)
    _, ok, st = expected(c)
    marks = c["op_kind"] >= CIN
    assert set(ok[marks & (c["op_kind"] == CIN)]) == {1, 2, 3, 4}
    assert set(ok[marks & (c["op_kind"] == COUT)]) == {0, 1, 2, 3}
    assert ok[~marks].tolist() == [1, 0, 1, 0, 0b0111, 0b0111]
    assert st.intervals == [[[0.0, 4.0], [8.0, 8.0]], [], [[0.0, 2.0], [5.0, 6.0]]]
    assert len(st.usage[1]) == 2 and st.usage[1][0][1:] == (0.0, 0.0, 0.0, 0.0)
    assert st.usage[0][1][1] == D[0] / CAP[0] and st.usage[2][2][1] == D[0] / CAP[0]
    return c


def churn(H, K, seed=5, name=None):
    """Hosts fill and drain with trace-like demands, checking in at every dispatch and out at
    every completion as the reference's hosts do; times advance in steps of 0, 0.25 or 3, so
    ``t == end`` and ``t > end`` both happen. Ends with no interval open."""
    rng = np.random.RandomState(seed + H + K)
    held = {h: [] for h in range(H)}
    ents, t = [], 0.0
    while len(ents) < K - 3 * H:
        t += float(rng.choice([0.0, 0.0, 0.25, 3.0]))
        h = int(rng.randint(H))
        q = held[h]
        if q and rng.rand() < 0.5:
            d = q.pop(int(rng.randint(len(q))))
            ents += [(h, UNSUB, t, d), (h, COUT, t)]
        else:
            d = demand(rng)
            q.append(d)
            ents += [(h, SUB, t, d), (h, CIN, t)]
    for h in range(H):                       # drain: the last mark of a host is a check-out
        t += 1.0
        ents += [(h, CIN, t), (h, COUT, t)]
    while len(ents) < K:
        ents.append((0, COUT, t))
    c = _case(name or "churn_%d_%d" % (H, K), H, ents[:K])
    _, ok, st = expected(c)
    st.finish()
    assert st.n_final > 0
    return c


def two_phases(H=7, K=500):
    """Two churns one after the other on the same hosts, the second later in time: at
    ``phase_cut`` every host's last interval is closed (a finish there is valid), and each host's
    first check-in of the second phase makes that interval final."""
    a = churn(H, K, seed=11, name="phase_a")
    b = churn(H, K, seed=12, name="phase_b")
    shift = float(a["op_time"][-1]) + 10.0
    c = {"name": "two_phases", "capacity": a["capacity"], "level0": a["level0"], "phase_cut": K,
         "op_host": np.concatenate([a["op_host"], b["op_host"]]),
         "op_kind": np.concatenate([a["op_kind"], b["op_kind"]]),
         "op_time": np.concatenate([a["op_time"], b["op_time"] + shift]),
         "op_amt": np.ascontiguousarray(np.concatenate([a["op_amt"], b["op_amt"]], axis=1))}
    _, _, half = expected(a)
    _, _, st = expected(c)
    assert (half.words()[0] == 2).all() and st.n_final >= half.n_final + H
    return c


def one_mark_each(H):
    """Host h checks in at time h // 7 and is checked out at the end: H rows of one or two usage
    records, the closed intervals all in the tail. Hosts 3 and H - 2 stay without a record."""
    skip = {3, H - 2}
    order = np.random.RandomState(H).permutation(H)
    ents = sorted([(int(h), CIN, float(h // 7)) for h in order if h not in skip],
                  key=lambda e: e[2])
    t = float(H)
    ents += [(int(h), COUT, t) for h in order[::2] if h not in skip]
    ents += [(int(h), COUT, t + 1) for h in order[1::2] if h not in skip]
    c = _case("one_mark_each_%d" % H, H, ents)
    _, _, st = expected(c)
    f = st.finish()
    assert len(f["row_host"]) == H - 2 and st.n_final == 0 and len(f["iv_start"]) == H - 2
    return c


BUILDERS = (
    [("row_" + n, functools.partial(table_row, n)) for n in ROWS] +
    [("table_mixed", table_mixed),
     ("churn_5_600", functools.partial(churn, 5, 600)),
     ("churn_1_4097", functools.partial(churn, 1, 4097)),
     ("churn_1_40", functools.partial(churn, 1, 40)),
     ("churn_40_3000", functools.partial(churn, 40, 3000)),
     ("two_phases", two_phases),
     ("one_mark_each_65", functools.partial(one_mark_each, 65)),
     ("one_mark_each_257", functools.partial(one_mark_each, 257))])
NAMES = [n for n, _ in BUILDERS]
OPEN_AT_END = ("row_in_none", "row_in_closed_later", "row_in_closed_same", "row_in_open")


@functools.lru_cache(maxsize=None)
def case(name):
    c = dict(BUILDERS)[name]()
    assert c["name"] == name
    return c


def violations(c):
    """(name, entry index, case) per contract violation of the metered log, built on ``c``
    (at its middle entry, and for the times also at entry 0 against a last time)."""
    K, H = len(c["op_host"]), c["capacity"].shape[1]
    k = K // 2
    assert c["op_time"][k] > 0 and K > 4
    out = []

    def vary(name, field, value, at=k):
        v = dict(c, name="%s_%s" % (c["name"], name))
        v[field] = c[field].copy()
        v[field][at] = value
        out.append((name, at, v))

    vary("time_decreasing", "op_time", np.nextafter(c["op_time"][k - 1], -np.inf))
    vary("time_nan", "op_time", np.nan)
    vary("time_2p52", "op_time", 2.0 ** 52)
    vary("time_negative", "op_time", -1.0, at=0)
    vary("kind_4", "op_kind", 4)
    vary("kind_neg", "op_kind", -1)
    vary("host_H", "op_host", H)
    vary("host_neg", "op_host", -1)
    return out


# ------------------------------------------------------------------------------- fixture
@functools.lru_cache(maxsize=None)
def fixture():
    """tests/golden/host_meter.json.gz: per run name ``capacity`` (4, H), the log (``op_host``,
    ``op_kind``, ``op_time``, ``op_amt`` (4, K), the reference's ``op_ok``) and ``round_ops``
    (entries logged before each recorded round)."""
    with gzip.open(os.path.join(GOLDEN, "host_meter.json.gz"), "rt") as f:
        raw = json.load(f)
    out = {}
    for t in raw:
        K = len(t["op_host"])
        cap = np.ascontiguousarray(np.array(t["capacity"], dtype=np.float64).T)
        out[t["name"]] = {
            "name": t["name"], "capacity": cap, "level0": cap,
            "op_host": np.array(t["op_host"], dtype=np.int32),
            "op_kind": np.array(t["op_kind"], dtype=np.int32),
            "op_time": np.array(t["op_time"], dtype=np.float64),
            "op_amt": np.array(t["op_amt"], dtype=np.float64).reshape(4, K),
            "op_ok": np.array(t["op_ok"], dtype=np.int32),
            "round_ops": [int(m) for m in t["round_ops"]]}
    return out


@functools.lru_cache(maxsize=None)
def reference():
    """tests/golden/meter_usage.json.gz by run name: the reference meter's ``hosts`` (its dict
    order: host index, intervals, record times, four value lists) and ``want`` series."""
    with gzip.open(os.path.join(GOLDEN, "meter_usage.json.gz"), "rt") as f:
        return {t["name"]: t for t in json.load(f)}


def cuts_of(t, n=40):
    """About ``n`` of the run's round counts, increasing and inside the log."""
    K = len(t["op_host"])
    marks = sorted({m for m in t["round_ops"] if 0 < m < K})
    step = max(1, len(marks) // n)
    return marks[step - 1::step]


def rows_by_index(ref_hosts):
    """The reference's host records as ``pack_usage`` scenario in host-index order."""
    hs = sorted(ref_hosts, key=lambda h: h["host"])
    return {"hosts": [h["intervals"] for h in hs], "routes": [],
            "usage": [(h["times"], tuple(h["usage"])) for h in hs]}


def instance_hours(ref_hosts):
    """Meter.cumulative_instance_hours (:31-33), in the meter's own order."""
    return sum([sum([v[1] - v[0] for v in h["intervals"]]) for h in ref_hosts]) / 3600


# ------------------------------------------------------------------------------- fake engine
class FakeMeterEngine:
    """What a metered ResidentCluster asks of an engine, on CPU tensors, by the checker. It
    keeps a HostMeterState beside the DeviceMeter and refuses a log the meter cannot take."""

    def __init__(self):
        import torch
        self.torch = torch
        self.device = torch.device("cpu")
        self.states = {}
        self.applied = []           # per call: (K, iv_cap, us_cap)

    def host_ops(self, capacity, level, op_host, op_kind, op_amt):
        from pivot_place.hostops import apply_ops
        return self.torch.from_numpy(apply_ops(capacity.numpy(), level.numpy(), op_host.numpy(),
                                               op_kind.numpy(), op_amt.numpy()))

    def host_meter_apply(self, m, capacity, level, op_host, op_kind, op_amt, op_time):
        st = self.states.setdefault(id(m), HostMeterState(m.n_hosts))
        K = op_host.numel()
        assert m.n_iv + K <= m.iv_cap and m.n_us + K <= m.us_cap, "the logs were not grown"
        assert m.iv_host.numel() == m.iv_cap and m.us_frac.numel() == 4 * m.us_cap
        self.applied.append((K, m.iv_cap, m.us_cap))
        ok = apply_meter_ops(capacity.numpy(), level.numpy(), st, op_host.numpy(),
                             op_kind.numpy(), op_amt.numpy(), op_time.numpy())
        m.n_iv, m.n_us, m.last_time = st.n_final, st.n_usage, st.last_time
        return self.torch.from_numpy(ok)

    def host_meter_finish(self, m):
        st = self.states.setdefault(id(m), HostMeterState(m.n_hosts))
        return {k: self.torch.from_numpy(np.ascontiguousarray(v).ravel())
                for k, v in st.finish().items()}

    def meter_usage_device(self, fin, sample_size, last_time):
        """numpy's statement of pvt_meter_usage's outputs for one scenario."""
        f = {k: v.numpy() for k, v in fin.items()}
        s, n_us = int(sample_size), len(f["us_time"])
        NB = int(last_time // s) + 1 if n_us else 0
        R = len(f["row_host"])
        n_hosts, res_hosts = np.zeros(NB, np.int32), np.zeros(NB, np.int32)
        res_mean = np.zeros((4, NB))
        frac = f["us_frac"].reshape(4, n_us)
        per = [dict() for _ in range(NB)]
        for i in range(R):
            seen = set()
            for v in range(f["iv_off"][i], f["iv_off"][i + 1]):
                seen |= set(range(int(f["iv_start"][v] // s), int(f["iv_end"][v] // s)))
            for b in seen:
                n_hosts[b] += 1
            for u in range(f["us_off"][i], f["us_off"][i + 1]):
                per[int(f["us_time"][u] // s)].setdefault(i, []).append(frac[:, u])
        for b, hosts in enumerate(per):
            res_hosts[b] = len(hosts)
            if hosts:
                res_mean[:, b] = np.mean([np.mean(v, axis=0) for v in hosts.values()], axis=0)
        avg = np.full((1, 5), np.nan)
        if (n_hosts > 0).any():
            avg[0, 0] = n_hosts[n_hosts > 0].mean()
        if (res_hosts > 0).any():
            avg[0, 1:] = res_mean[:, res_hosts > 0].mean(axis=1)
        return {"bucket_off": np.array([0, NB], dtype=np.int64), "n_hosts": n_hosts,
                "res_hosts": res_hosts, "res_mean": res_mean, "avg": avg}

    def meter_device(self, fin):
        f = {k: v.numpy() for k, v in fin.items()}
        hours = sum(float((f["iv_end"][a:b] - f["iv_start"][a:b]).sum())
                    for a, b in zip(f["iv_off"][:-1], f["iv_off"][1:])) / 3600
        return {"instance_hours": np.array([hours]), "egress_cost": np.zeros(1),
                "congestion_delay": np.zeros(1)}


def assert_series(got, want, rel=1e-9):
    """``got``: ResidentCluster.usage's dict; ``want``: the reference's series of one sample size
    from meter_usage.json.gz. Bucket positions and host counts exact, means within ``rel``."""
    assert [list(k) for k in got["hosts"][0]] == want["hosts"][0]
    assert list(got["hosts"][1]) == want["hosts"][1]
    for r in ("cpus", "mem", "disk", "gpus"):
        assert list(got[r][0]) == want[r][0], r
        np.testing.assert_allclose(np.array(got[r][1], dtype=np.float64), want[r][1], rtol=rel,
                                   atol=0, err_msg=r)
    assert got["avg"][0] == want["avg"][0]
    np.testing.assert_allclose(got["avg"][1:], want["avg"][1:], rtol=rel, atol=0)
