"""Seeded host-op logs for the resident cluster state (pvt_host_ops_apply), checked by
``pivot_place.hostops.apply_ops``, and the reader of tests/golden/host_ops.json.gz.

A case is a dict: ``name``, ``capacity`` and ``level0`` (4, H) float64, ``op_host`` / ``op_kind``
(K,) int32, ``op_amt`` (4, K) float64. ``expected(case)`` is apply_ops' verdict, computed once:
(level after, op_ok). A builder asserts what makes its case worth having (that a refusal is a
refusal, that put-backs are skipped by rounding, that the order of a host's ops shows).
"""
import functools
import gzip
import json
import os

import numpy as np

from pivot_place.hostops import SUBSCRIBE as SUB, UNSUBSCRIBE as UNSUB, apply_ops

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CAP = (16.0, 131072.0, 100.0, 1.0)      # the reference's hosts (alibaba/sim.py: 16, 131072, 100, 1)
MEM_UNIT = 7864.32                       # the trace's memory demands are mem x 7864.32


def _case(name, capacity, ops, level0=None):
    capacity = np.ascontiguousarray(capacity, dtype=np.float64).reshape(4, -1)
    K = len(ops)
    return {"name": name, "capacity": capacity,
            "level0": capacity.copy() if level0 is None else
            np.ascontiguousarray(level0, dtype=np.float64).reshape(4, -1),
            "op_host": np.array([o[0] for o in ops], dtype=np.int32),
            "op_kind": np.array([o[1] for o in ops], dtype=np.int32),
            "op_amt": np.ascontiguousarray(
                np.array([o[2] for o in ops], dtype=np.float64).reshape(K, 4).T)}


def _caps(H):
    return np.repeat(np.array(CAP)[:, None], H, axis=1)


def run(case):
    """apply_ops on a copy of the case's start: (level after, op_ok)."""
    level = case["level0"].copy()
    ok = apply_ops(case["capacity"], level, case["op_host"], case["op_kind"], case["op_amt"])
    return level, ok


_EXPECTED = {}


def expected(case):
    if case["name"] not in _EXPECTED:
        _EXPECTED[case["name"]] = run(case)
    return _EXPECTED[case["name"]]


def demand(rng):
    """A trace-like demand: cpus of a few halves, memory a multiple of 0.01 x 7864.32."""
    return (float(rng.choice([0.5, 1.0, 1.0, 2.0, 4.0])),
            float(np.round(rng.uniform(0.01, 2.0), 2) * MEM_UNIT),
            float(rng.choice([0.0, 0.0, 1.0])), 0.0)


def skipped(case):
    """Put-backs of a positive amount that apply_ops did not make."""
    _, ok = expected(case)
    amt, un = case["op_amt"], case["op_kind"] == UNSUB
    return int(sum(((amt[r] > 0) & un & (((ok >> r) & 1) == 0)).sum() for r in range(4)))


# ------------------------------------------------------------------------------- builders
def empty(H):
    return _case("empty_h%d" % H, _caps(H), [])


def single(kind):
    lvl = _caps(1)
    lvl[:, 0] = (10.0, 100000.0, 100.0, 1.0)
    c = _case("single_%s" % ("sub", "unsub")[kind], _caps(1),
              [(0, kind, (2.0, 3.5 * MEM_UNIT, 1.0, 0.0))], level0=lvl)
    level, ok = expected(c)
    assert ok[0] == (1 if kind == SUB else 0b011)       # disk is full: nothing to put back
    assert not np.array_equal(level, lvl)
    return c


def long_segment(n, seed=1):
    """Host 2 of 5 takes n alternating ops; its neighbours stay untouched."""
    rng = np.random.RandomState(seed + n)
    ops, last = [], None
    for i in range(n):
        if i % 2 == 0:
            last = demand(rng)
            ops.append((2, SUB, last))
        else:
            ops.append((2, UNSUB, last))
    c = _case("long_%d" % n, _caps(5), ops)
    level, ok = expected(c)
    assert np.array_equal(level[:, [0, 1, 3, 4]], c["level0"][:, [0, 1, 3, 4]])
    return c


def all_distinct(n=1025, seed=2):
    rng = np.random.RandomState(seed)
    hosts = rng.permutation(n)
    ops = [(int(h), SUB if i % 3 else UNSUB, demand(rng)) for i, h in enumerate(hosts)]
    lvl = _caps(n) * 0.5
    return _case("distinct_%d" % n, _caps(n), ops, level0=lvl)


def high_keys(H, seed=3):
    """9 ops on each of the hosts 0, 65535, 65536 and H-1, interleaved: key bits above 16 (and,
    for H > 2^20, bit 20) decide the order."""
    rng = np.random.RandomState(seed)
    hosts = [0, 65535, 65536, H - 1]
    ops, held = [], {h: [] for h in hosts}
    for i in range(9):
        for h in hosts:
            if i % 3 == 2:
                ops.append((h, UNSUB, held[h].pop(0)))
            else:
                held[h].append(demand(rng))
                ops.append((h, SUB, held[h][-1]))
    c = _case("high_keys_%d" % H, _caps(H), ops)
    level, _ = expected(c)
    changed = np.flatnonzero((level != c["level0"]).any(axis=0))
    assert changed.tolist() == sorted(set(hosts))
    return c


def refusals():
    """One host per scenario, each with the levels (4, 1000.5, 10, 1) under the capacity CAP;
    the scenario's op, then a put-back that shows what the op left."""
    base = (4.0, 1000.5, 10.0, 1.0)
    small = (1.0, 10.0, 1.0, 0.0)
    scen, want = [], []
    for r in range(4):
        def at(v, rest=small):
            d = list(rest)
            d[r] = v
            return tuple(d)
        scen += [(SUB, at(float(np.nextafter(base[r], np.inf)))), (SUB, at(base[r])),
                 (SUB, at(-1.0)), (SUB, at(float("nan"))), (SUB, at(float("inf"))),
                 (SUB, at(float("-inf"))), (UNSUB, at(float("nan"))), (UNSUB, at(float("inf"))),
                 (UNSUB, at(-1.0)), (UNSUB, at(float(np.nextafter(CAP[r] - base[r], np.inf))))]
        rest_mask = sum(1 << q for q in range(4) if q != r and small[q] > 0)
        want += [0, 1, 0, 1, 0, 0, rest_mask, rest_mask, rest_mask, rest_mask]
    scen.append((SUB, (0.0, 0.0, 0.0, 0.0)))
    want.append(1)
    scen.append((UNSUB, (0.0, 0.0, 0.0, 0.0)))
    want.append(0)
    H = len(scen)
    lvl = np.repeat(np.array(base)[:, None], H, axis=1)
    ops = [(h, k, d) for h, (k, d) in enumerate(scen)]
    c = _case("refusals", _caps(H), ops, level0=lvl)
    level, ok = expected(c)
    assert ok.tolist() == want, (ok.tolist(), want)
    for r in range(4):
        h = 10 * r + 1                      # amount == level: taken, and the level is +0.0
        assert level[r, h] == 0.0 and not np.signbit(level[r, h])
        h = 10 * r + 3                      # a NaN amount passes and changes nothing itself
        assert level[r, h] == base[r]
    for h, (k, d) in enumerate(scen):       # a refused subscribe changes nothing
        if k == SUB and ok[h] == 0:
            assert np.array_equal(level[:, h], lvl[:, h])
    return c


def putbacks():
    """Put-backs of more than is used, and on an idle host."""
    ops = [(0, SUB, (3.0, 4096.0, 2.0, 1.0)),
           (0, UNSUB, (5.0, 4096.0, 3.0, 1.0)),      # cpus and disk: more than is used
           (1, UNSUB, (1.0, MEM_UNIT, 1.0, 1.0)),    # an idle host: nothing is used
           (0, UNSUB, (3.0, 4096.0, 2.0, 1.0))]      # mem and gpus are back already
    c = _case("putbacks", _caps(2), ops)
    level, ok = expected(c)
    assert ok.tolist() == [1, 0b1010, 0, 0b0101]
    assert np.array_equal(level, c["level0"])
    return c


def rounding_skips(min_skips=10):
    """Hosts that fill up with a few tasks and drain again, with the trace's memory amounts. A
    put-back that follows its own accepted subscribe asks for no more than is in use, so when it
    is skipped it is skipped by the rounding of ``capacity - level`` alone: typically the last
    put-back of a draining host, whose level carries the rounding of the subtractions before it
    (the memory then never returns). Searches seeds for a log with >= min_skips such
    put-backs."""
    for seed in range(200):
        rng = np.random.RandomState(1000 + seed)
        H, ops, own = 16, [], []
        for _ in range(6):                       # cycles: every host fills, then drains
            held = {h: [] for h in range(H)}
            for h in rng.permutation(H):
                for _ in range(int(rng.randint(2, 7))):
                    d = (0.25, float(np.round(rng.uniform(0.01, 1.0), 2) * MEM_UNIT), 0.0, 0.0)
                    held[int(h)].append((d, len(ops)))
                    own.append(-1)
                    ops.append((int(h), SUB, d))
            left = [h for h in range(H) for _ in held[h]]
            for h in rng.permutation(left):
                d, k = held[int(h)].pop(int(rng.randint(len(held[int(h)]))))
                own.append(k)
                ops.append((int(h), UNSUB, d))
        c = _case("rounding_skips", _caps(H), ops)
        level, ok = run(c)
        own = np.array(own)
        n = int(((own >= 0) & (ok[np.maximum(own, 0)] == 1) & ((ok & 2) == 0)).sum())
        if n >= min_skips:
            return c
    raise AssertionError("no seed gave %d put-backs skipped by rounding" % min_skips)


def order_sensitive():
    """Three hosts, interleaved; each host's ops give another result when reversed, so a sort
    that does not keep a host's log order shows."""
    per = [(SUB, (10.0, 0.0, 0.0, 0.0)), (SUB, (10.0, 0.0, 0.0, 0.0)), (UNSUB, (10.0, 0.0, 0.0, 0.0)),
           (UNSUB, (3.0, 0.0, 0.0, 0.0)), (SUB, (5.0, 0.0, 0.0, 0.0))] * 60
    ops = [(h, k, d) for (k, d) in per for h in (2, 0, 1)]
    c = _case("order_sensitive", _caps(3), ops)
    level, ok = expected(c)
    for h in range(3):
        idx = np.flatnonzero(c["op_host"] == h)
        rev = dict(c, name="order_sensitive_rev%d" % h, op_kind=c["op_kind"].copy(),
                   op_amt=c["op_amt"].copy())
        rev["op_kind"][idx] = c["op_kind"][idx[::-1]]
        rev["op_amt"][:, idx] = c["op_amt"][:, idx[::-1]]
        level_r, ok_r = run(rev)
        assert not np.array_equal(level_r, level) or not np.array_equal(ok_r[idx][::-1], ok[idx])
    return c


def skewed(H, K, seed=4):
    """Trace-like amounts; half the ops fall on 3 hosts. A host's put-backs name amounts it was
    asked for earlier, whether or not that subscribe was taken."""
    rng = np.random.RandomState(seed + H)
    hot = rng.choice(H, 3, replace=False)
    held = {}
    ops = []
    for _ in range(K):
        h = int(hot[rng.randint(3)]) if rng.rand() < 0.5 else int(rng.randint(H))
        q = held.setdefault(h, [])
        if q and rng.rand() < 0.5:
            ops.append((h, UNSUB, q.pop(int(rng.randint(len(q))))))
        else:
            q.append(demand(rng))
            ops.append((h, SUB, q[-1]))
    c = _case("skewed_%d_%d" % (H, K), _caps(H), ops)
    assert np.isin(c["op_host"], hot).sum() >= K // 2 - K // 20
    return c


BUILDERS = (
    [("empty_h%d" % H, functools.partial(empty, H)) for H in (1, 5)] +
    [("single_sub", functools.partial(single, SUB)), ("single_unsub", functools.partial(single, UNSUB))] +
    [("long_%d" % n, functools.partial(long_segment, n)) for n in (65, 257, 1025, 4097)] +
    [("distinct_1025", all_distinct)] +
    [("high_keys_%d" % H, functools.partial(high_keys, H)) for H in (70000, 1048577)] +
    [("refusals", refusals), ("putbacks", putbacks), ("rounding_skips", rounding_skips),
     ("order_sensitive", order_sensitive)] +
    [("skewed_%d_%d" % hk, functools.partial(skewed, *hk))
     for hk in ((12, 3000), (100, 20000), (4096, 50000))])
NAMES = [n for n, _ in BUILDERS]


@functools.lru_cache(maxsize=None)
def case(name):
    c = dict(BUILDERS)[name]()
    assert c["name"] == name
    return c


# ------------------------------------------------------------------------------- fixture
@functools.lru_cache(maxsize=None)
def fixture():
    """tests/golden/host_ops.json.gz: per trace name a dict with ``capacity`` (4, H), the log
    (``op_host``, ``op_kind``, ``op_amt`` (4, K), the reference's ``op_ok``), ``round_ops`` (ops
    logged before each recorded round's snapshot) and ``skipped_putbacks``."""
    with gzip.open(os.path.join(GOLDEN, "host_ops.json.gz"), "rt") as f:
        raw = json.load(f)
    out = {}
    for t in raw:
        K = len(t["op_host"])
        out[t["name"]] = {
            "name": t["name"],
            "capacity": np.ascontiguousarray(np.array(t["capacity"], dtype=np.float64).T),
            "op_host": np.array(t["op_host"], dtype=np.int32),
            "op_kind": np.array(t["op_kind"], dtype=np.int32),
            "op_amt": np.array(t["op_amt"], dtype=np.float64).reshape(4, K),
            "op_ok": np.array(t["op_ok"], dtype=np.int32),
            "round_ops": [int(m) for m in t["round_ops"]],
            "skipped_putbacks": int(t["skipped_putbacks"])}
    return out


TRACES = ("sim_h12_opportunistic", "sim_h12_vbp_ff", "sim_h12_vbp_bf", "sim_h12_cost_aware",
          "sim_h12_cost_aware_bf", "sim_c1_cost_aware")


def snapshot(case_):
    """(4, H) availability of a round of golden_io.sim_rounds."""
    return np.ascontiguousarray(np.array(case_["avail"], dtype=np.float64).reshape(-1, 4).T)


# ------------------------------------------------------------------------------- replay
class FakeEngine:
    """What ResidentCluster asks of an engine, on CPU tensors: apply_ops for the log and the
    CPU restatement of the policies for the round."""

    def __init__(self):
        import torch
        self.torch = torch
        self.device = torch.device("cpu")
        self.restored = []          # per restore_hosts call: the hosts it named

    def host_ops(self, capacity, level, op_host, op_kind, op_amt):
        ok = apply_ops(capacity.numpy(), level.numpy(), op_host.numpy(), op_kind.numpy(),
                       op_amt.numpy())
        return self.torch.from_numpy(ok)

    def restore_hosts(self, avail, avail0, hosts):
        a, a0 = avail.numpy().reshape(4, -1), avail0.numpy().reshape(4, -1)
        hs = hosts.numpy()
        self.restored.append(hs.copy())
        for h in hs:
            if 0 <= h < a.shape[1]:
                a[:, h] = a0[:, h]

    def run(self, dr):
        import dataclasses
        from oracle import oracle
        r = dataclasses.replace(
            dr.arrays, avail=dr.avail.numpy().reshape(4, -1).copy(), zone=dr.zone.numpy(),
            cost=dr.cost.numpy().reshape(dr.n_zones, dr.n_zones),
            bw=dr.bw.numpy().reshape(dr.n_zones, dr.n_zones),
            tiebreak=None if dr.tiebreak is None else dr.tiebreak.numpy().view(np.uint32),
            mt_state=dr.mt)
        res = oracle.place(r)
        T = r.n_tasks
        dr.placement.numpy()[:T] = res.placement
        dr.order.numpy()[:T] = res.order
        dr.avail.numpy()[:] = res.avail.ravel()
        if dr.mt is not None:
            dr.mt[:] = res.mt_state


def replay_resident(engine, name, check_levels=True):
    """The round loop of a recorded reference simulation on a ResidentCluster: the log up to
    each round's snapshot, then the round. Asserts, per round: the reference's results of the
    ops, (``check_levels``) its snapshot, its placement, order and carried MT19937 state, and
    that no more went up than the round's task arrays, its log and 4 KiB. The rounds' ``avail``
    is NaN: it is not read. Returns (cluster, rounds replayed)."""
    import dataclasses
    import golden_io
    from pivot_place import _abi
    from pivot_place.hostops import ResidentCluster
    fx = fixture()[name]
    tr, cases = golden_io.sim_rounds(name)
    cost, bw, _ = golden_io.zones()
    vbp = tr["policy"] in ("vbp_ff", "vbp_bf")
    rc = ResidentCluster(engine, fx["capacity"], np.array(tr["zone"], dtype=np.int32), cost, bw,
                         tiebreak=np.array(tr["id_rank"], dtype=np.uint32) if vbp else None)
    H = rc.n_hosts
    assert len(cases) == len(fx["round_ops"])
    opp = tr["policy"] == "opportunistic"
    mt = golden_io.mt_state(tr["seed"]) if opp else None
    shadow = np.random.RandomState(tr["seed"])
    done = 0
    for k, (case, m) in enumerate(zip(cases, fx["round_ops"])):
        run_ = case["runs"][0]
        before = rc.bytes_uploaded
        ok = rc.apply(fx["op_host"][done:m], fx["op_kind"][done:m], fx["op_amt"][:, done:m])
        assert np.array_equal(ok, fx["op_ok"][done:m]), "round %d: op results" % k
        if check_levels:
            assert np.array_equal(rc.levels(), snapshot(case)), "round %d: snapshot" % k
        r = golden_io.run_arrays(case, run_)
        r = dataclasses.replace(r, avail=np.full((4, H), np.nan), mt_state=mt)
        res = rc.place(r)
        placement, order, _, _ = golden_io.expected(case, run_)
        assert np.array_equal(res.placement, placement), "round %d: placement" % k
        assert np.array_equal(res.order, order), "round %d: order" % k
        assert res.avail is None
        if opp:
            for _ in range(run_["rng_draws"]):
                shadow.randint(0, 1 << 32, dtype=np.uint32)
            st = shadow.get_state()
            assert np.array_equal(res.mt_state[:624], st[1]) and res.mt_state[624] == st[2], \
                "round %d: MT19937 state" % k
            mt = res.mt_state
        tasks = sum(a.nbytes for a in (r.dem, r.decay, r.task_group, r.group_anchor, r.rt_bw,
                                       r.mt_state) if a is not None)
        log_bytes = (m - done) * (4 + 4 + 32)
        assert rc.bytes_uploaded - before <= tasks + log_bytes + 4096, "round %d: upload" % k
        done = m
    return rc, len(cases)
