"""pivot_place.routes on the CPU: the rule of pvt_rt_rows against the reference's recorded realtime
bandwidths (tests/golden/route_queues.json.gz), the list's contract, queues_of on a fake cluster,
the binding's struct and ResidentCluster.place(routes=...) over a fake engine."""
import ctypes
import os
import re

import numpy as np
import pytest

import rt_rows_cases as rr
from pivot_place import _abi, routes
from pivot_place.hostops import ResidentCluster
from pivot_place.routes import IN, OUT, RouteQueues, realtime_rows, realtime_value


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


STATES = [s["name"] for s in rr.fixture()["states"]]


def _state(name):
    return next(s for s in rr.fixture()["states"] if s["name"] == name)


# ---- the rule against the reference ---------------------------------------------------------------
@pytest.mark.parametrize("name", STATES)
def test_rows_equal_the_reference_bit_for_bit(name):
    """Every storage and host of the state: in + out of the reference's realtime_bw properties."""
    bw = rr.fixture()["bw"]
    st = _state(name)
    rq = rr.state_queues(st, len(bw))
    rows = realtime_rows(st["zone"], bw, st["storage_zone"], rq)
    want = rr.state_rows(st)
    assert rows.shape == want.shape == (len(st["storage_zone"]), len(st["zone"]))
    assert _bits(rows) == _bits(want)
    # and route by route, through the scalar statement of the rule
    sz = st["storage_zone"]
    for r in st["routes"]:
        ref = (st["rt_in"] if r["dir"] == IN else st["rt_out"])[r["k"]][r["h"]]
        assert realtime_value(r["bw"], r["mbs"]) == ref
    listed = {(r["k"], r["h"], r["dir"]) for r in st["routes"]}
    for k, a in enumerate(sz):
        for h, z in enumerate(st["zone"]):
            if (k, h, IN) not in listed:
                assert realtime_value(bw[a, z], []) == st["rt_in"][k][h]
            if (k, h, OUT) not in listed:
                assert realtime_value(bw[z, a], []) == st["rt_out"][k][h]


def test_fixture_holds_the_states_it_was_made_for():
    names = set(STATES)
    assert {"queued_h12", "queued_h100", "replaced_h12"} <= names
    assert names & {"sim_h12_contention", "requeued_h12"}
    req = _state("requeued_h12") if "requeued_h12" in names else _state("sim_h12_contention")
    assert any(len(r["mbs"]) >= 2 for r in req["routes"])
    if req["name"] == "requeued_h12":           # 2500 MB sent 1000, queued again behind the 700
        assert [r["mbs"] for r in req["routes"]] == [[700, 1500]]
    rep, base = _state("replaced_h12"), _state("queued_h12")
    extra = [r for r in rep["routes"] if not r["mbs"]]
    assert len(extra) == 1 and len(rep["routes"]) == len(base["routes"]) + 1
    bw = rr.fixture()["bw"]
    r = extra[0]
    a, z = rep["storage_zone"][r["k"]], rep["zone"][r["h"]]
    assert r["bw"] != (bw[a, z] if r["dir"] == IN else bw[z, a])
    assert max(len(r["mbs"]) for r in _state("queued_h100")["routes"]) == 6


def test_the_sum_runs_in_queue_order():
    """Order-sensitivity guard: of the fixture's routes with two or more packets, at least 10 %
    change bits in realtime_value when the queue is rotated by one (measured here: printed), so
    a sum in another order cannot pass test_rows_equal_the_reference_bit_for_bit unnoticed."""
    n = changed = 0
    for st in rr.fixture()["states"]:
        for r in st["routes"]:
            if len(r["mbs"]) >= 2:
                n += 1
                changed += realtime_value(r["bw"], r["mbs"]) != realtime_value(
                    r["bw"], r["mbs"][1:] + r["mbs"][:1])
    print("rotated queues that change realtime_value: %d of %d (%.1f %%)" % (changed, n, 100.0 * changed / n))
    assert n >= 1000
    assert changed >= 0.10 * n


def test_an_idle_route_is_not_its_static_bandwidth():
    """Idle-route guard: some zone pair of the fixture's table has 1 / (1 / b) != b."""
    bw = rr.fixture()["bw"]
    idle = np.array([[realtime_value(b, []) for b in row] for row in bw])
    share = float((idle != bw).mean())
    print("zone pairs whose idle value differs from the table: %.1f %%" % (100 * share))
    assert (idle != bw).any()
    used = {(st["storage_zone"][k], z) for st in rr.fixture()["states"]
            for k in range(len(st["storage_zone"])) for z in st["zone"]}
    assert any(idle[a, z] != bw[a, z] or idle[z, a] != bw[z, a] for a, z in used)
    t = rr.table(64, 3)
    assert _bits(routes._idle(t)) == _bits([[realtime_value(b, []) for b in row] for row in t])
    assert 0.05 < float((routes._idle(t) != t).mean()) < 0.2


def test_values_vectorised_equal_the_scalar_rule():
    t, z = rr.table(7, 1), rr.zones(65, 7, 2)
    es = rr.random_entries(np.random.RandomState(3), [0, 3, 6], 65, t, z, 0.5, own_bw=0.3)
    es += [e for e in rr.edge_entries(65, 7, [1], t, z)]
    rq = RouteQueues.pack(es, 65, 7)
    want = [realtime_value(rq.bw[i], rq.mbs[rq.off[i]:rq.off[i + 1]]) for i in range(rq.n_routes)]
    assert _bits(rq.values()) == _bits(want)
    # extremes follow IEEE
    assert realtime_value(np.inf, [5.0]) == np.inf                  # est == 0: the value is bw
    assert realtime_value(5e-324, []) == 0.0                        # est = inf
    assert realtime_value(3.0, [1e308, 1e308]) == 0.0               # the packets sum to inf
    assert realtime_value(1e-310, [2.0]) == 1.0 / (3.0 / 1e-310)


def test_rows_convention_and_shared_anchors():
    t, z = rr.table(5, 4), rr.zones(33, 5, 5)
    rq = RouteQueues.pack(rr.random_entries(np.random.RandomState(6), [0, 2], 33, t, z, 0.5), 33, 5)
    one = realtime_rows(z, t, None, rq)
    assert one.shape == (1, 33)
    assert _bits(one) == _bits(realtime_rows(z, t, [0], rq)) == _bits(realtime_rows(z, t, np.zeros(0, np.int32), rq))
    rows = realtime_rows(z, t, [2, 0, 2, 4], rq)
    assert _bits(rows[0]) == _bits(rows[2]) and _bits(rows[1]) == _bits(one[0])
    assert _bits(rows[3]) == _bits(routes._idle(t[4, z]) + routes._idle(t[z, 4]))     # no entry names zone 4
    with pytest.raises(ValueError, match=r"group_anchor\[1\] = 5"):
        realtime_rows(z, t, [0, 5], rq)
    with pytest.raises(ValueError, match=r"zone\[%d\] = 4" % int(np.flatnonzero(z == 4)[0])):
        realtime_rows(z, t[:4, :4], [0], routes.empty_queues())


# ---- pack and the contract ------------------------------------------------------------------------
def test_pack_sorts_and_refuses_duplicates():
    es = [(2, 5, 1, 10.0, [1.0]), (0, 7, 0, 11.0, []), (2, 5, 0, 12.0, [3.0, 2.0]), (0, 1, 1, 13.0, [4.0])]
    rq = RouteQueues.pack(es, 8, 3)
    assert list(zip(rq.anchor, rq.host, rq.dir)) == [(0, 1, 1), (0, 7, 0), (2, 5, 0), (2, 5, 1)]
    assert list(rq.bw) == [13.0, 11.0, 12.0, 10.0]
    assert list(rq.off) == [0, 1, 1, 3, 4] and list(rq.mbs) == [4.0, 3.0, 2.0, 1.0]
    assert (rq.anchor.dtype, rq.off.dtype, rq.mbs.dtype) == (np.int32, np.int64, np.float64)
    assert rq.nbytes == 4 * (4 + 4 + 4 + 8) + 5 * 8 + 4 * 8
    with pytest.raises(ValueError, match="listed twice"):
        RouteQueues.pack(es + [(0, 7, 0, 1.0, [])], 8, 3)
    assert RouteQueues.pack([], 8, 3).n_routes == 0


BAD_ENTRIES = {
    "anchor high": (3, 0, 0, 1.0, [1.0]), "anchor negative": (-1, 0, 0, 1.0, [1.0]),
    "host high": (0, 8, 0, 1.0, [1.0]), "host negative": (0, -1, 0, 1.0, [1.0]),
    "dir": (0, 0, 2, 1.0, [1.0]), "bw zero": (0, 0, 0, 0.0, [1.0]), "bw negative": (0, 0, 0, -2.0, []),
    "bw nan": (0, 0, 0, float("nan"), []), "packet zero": (0, 0, 0, 1.0, [1.0, 0.0]),
    "packet negative": (0, 0, 0, 1.0, [-1.0]), "packet nan": (0, 0, 0, 1.0, [float("nan"), 2.0]),
}


@pytest.mark.parametrize("what", sorted(BAD_ENTRIES))
def test_pack_refuses_each_violation(what):
    good = [(1, 3, 0, 5.0, [2.0]), (1, 3, 1, 5.0, [])]
    with pytest.raises(ValueError):
        RouteQueues.pack(good + [BAD_ENTRIES[what]], 8, 3)


def test_first_bad_names_the_entry():
    """Arrays that never went through pack: the entry pvt_rt_rows names."""
    def rq(**kw):
        d = dict(anchor=[0, 0, 1, 1], host=[0, 0, 2, 3], dir=[0, 1, 0, 0], bw=[1.0, 2.0, 3.0, 4.0],
                 off=[0, 1, 1, 3, 4], mbs=[1.0, 2.0, 3.0, 4.0])
        d.update(kw)
        return RouteQueues(**d)
    assert rq().first_bad(4, 2) == -1
    assert rq(host=[0, 0, 3, 2]).first_bad(4, 2) == 3                # unsorted
    assert rq(host=[0, 0, 2, 2]).first_bad(4, 2) == 3                # duplicate
    assert rq(dir=[1, 0, 0, 0]).first_bad(4, 2) == 1
    assert rq().first_bad(3, 2) == 3 and rq().first_bad(4, 1) == 2
    assert rq(off=[0, 2, 1, 3, 4]).first_bad(4, 2) == 1              # off decreasing
    assert rq(off=[1, 1, 1, 3, 4]).first_bad(4, 2) == 0              # off[0] != 0
    assert rq(off=[0, 1, 1, 3, 3]).first_bad(4, 2) == 3              # off[R] != P
    assert rq(off=[0, 1, 1, 3, 5]).first_bad(4, 2) == 3
    assert rq(mbs=[1.0, 2.0, 0.0, 4.0]).first_bad(4, 2) == 2
    assert rq(bw=[1.0, float("nan"), 3.0, 4.0]).first_bad(4, 2) == 1
    with pytest.raises(ValueError, match="entry 2 of the route queues"):
        rq(mbs=[1.0, 2.0, -1.0, 4.0]).check(4, 2)
    assert rq(bw=[1.0, float("inf"), 3.0, 4.0], mbs=[float("inf"), 2.0, 3.0, 4.0]).first_bad(4, 2) == -1
    with pytest.raises(ValueError, match="one length"):
        RouteQueues([0], [0, 1], [0], [1.0], [0, 0], [])


# ---- queues_of on a fake cluster --------------------------------------------------------------------
class Packet:
    def __init__(self, num_mbs):
        self.num_mbs = num_mbs


class Store:
    def __init__(self):
        self.items = []


class NetworkRoute:
    """A route as the reference keeps it: ``bw`` and a private store of packets."""

    def __init__(self, bw, mbs=()):
        self.bw = bw
        self.__pkts = Store()
        self.__pkts.items.extend(Packet(m) for m in mbs)

    @property
    def realtime_bw(self):       # network.py:70-73
        est = (sum([p.num_mbs for p in self.__pkts.items]) + 1) / self.bw
        return 1 / est if est else self.bw


class Node:
    def __init__(self, id, locality):
        self.id, self.locality = id, locality


class FakeCluster:
    def __init__(self, H, Z, seed):
        rs = np.random.RandomState(seed)
        self.zones = ["z%d" % i for i in range(Z)]
        self.bw = rr.table(Z, seed)
        self.hosts = [Node("h%d" % i, self.zones[rs.randint(Z)]) for i in range(H)]
        self.storage = [Node("s%d" % i, z) for i, z in enumerate(self.zones)]
        self.routes = {}
        for s in self.storage:
            a = self.zones.index(s.locality)
            for h in self.hosts:
                z = self.zones.index(h.locality)
                for key, b in (((s.id, h.id), self.bw[a, z]), ((h.id, s.id), self.bw[z, a])):
                    u = rs.random_sample()
                    mbs = list(rs.uniform(1, 4000, size=rs.randint(1, 5))) if u < 0.3 else []
                    own = float(b) * 0.5 if 0.3 <= u < 0.35 or u < 0.03 else float(b)
                    self.routes[key] = NetworkRoute(own, mbs)

    def get_route(self, src, dst):
        return self.routes.get((src, dst))

    def get_storage_by_locality(self, l):
        return next((s for s in self.storage if s.locality == l), None)


class FakeTables:
    """The part of the policies' per-cluster tables queues_of reads."""

    def __init__(self, cl):
        from pivot_place.policies import _ClusterTables
        self.zones, self.bw = cl.zones, cl.bw
        self.host_ids = [h.id for h in cl.hosts]
        self.zone = np.array([cl.zones.index(h.locality) for h in cl.hosts], dtype=np.int32)
        self.routes_of = lambda cluster, anchor: _ClusterTables.routes_of(self, cluster, anchor)


def test_queues_of_lists_exactly_the_routes_that_are_not_idle():
    cl = FakeCluster(23, 4, 9)
    tab = FakeTables(cl)
    anchors = [2, 0, 2]
    rq = routes.queues_of(cl, tab, anchors)
    want = set()
    for a in (0, 2):
        for h, host in enumerate(cl.hosts):
            z = int(tab.zone[h])
            for d, key, b in ((IN, ("s%d" % a, host.id), cl.bw[a, z]), (OUT, (host.id, "s%d" % a), cl.bw[z, a])):
                r = cl.routes[key]
                if r._NetworkRoute__pkts.items or r.bw != b:
                    want.add((a, h, d))
    assert set(zip(rq.anchor.tolist(), rq.host.tolist(), rq.dir.tolist())) == want
    assert 0 < len(want) < 4 * 23 and any(rq.off[i] == rq.off[i + 1] for i in range(rq.n_routes))
    # the rows are what _realtime_row's formula gives over all 2 * H routes
    rows = realtime_rows(tab.zone, tab.bw, anchors, rq)
    for g, a in enumerate(anchors):
        ins, outs = tab.routes_of(cl, cl.storage[a])
        row = (np.array([x.realtime_bw for x in ins], dtype=np.float64)
               + np.array([x.realtime_bw for x in outs], dtype=np.float64))
        assert _bits(rows[g]) == _bits(row)
    gone = cl.storage.pop(3)                                            # zone 3 has no storage now
    with pytest.raises(AttributeError, match="'NoneType' object has no attribute 'id'"):
        routes.queues_of(cl, tab, [3])
    cl.storage.insert(3, gone)
    del cl.routes[("s0", "h5")]
    with pytest.raises(AttributeError, match="realtime_bw"):
        routes.queues_of(cl, tab, [0])
    assert routes.queues_of(cl, tab, [1, 3]).n_routes > 0              # other anchors: untouched


# ---- the binding ---------------------------------------------------------------------------------
def test_struct_layout():
    q = _abi.pvt_route_queues
    want = ["n_hosts", "n_zones", "n_groups", "n_routes", "zone", "bw", "group_anchor", "rq_anchor",
            "rq_host", "rq_dir", "rq_bw", "rq_off", "rq_mbs", "n_packets", "rt_bw"]
    assert [f[0] for f in q._fields_] == want
    assert [getattr(q, n).offset for n in want] == [0, 4, 8, 12] + list(range(16, 16 + 8 * 11, 8))
    assert ctypes.sizeof(q) == 104
    assert q.n_packets.size == 8 and q.n_routes.size == 4
    assert _abi.PVT_ABI_VERSION == 3
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                           "include", "pivot_place.h")) as f:
        text = f.read()
    assert "int  pvt_rt_rows(pvt_ctx* ctx, const pvt_route_queues* q);" in text
    assert "#define PVT_ABI_VERSION 3" in text.replace("  ", " ")
    body = re.search(r"typedef struct pvt_route_queues \{(.*?)\} pvt_route_queues;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    names = [re.split(r"[\s*]+", n.strip(" *"))[-1] for d in decls for n in d.split(",")]
    assert names == want
    ctype = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}
    fields = dict(q._fields_)
    for d in decls:
        for n in d.split(","):
            name = re.split(r"[\s*]+", n.strip(" *"))[-1]
            base = d.replace("const", "").split()[0].strip("*")
            assert fields[name] is (ctypes.c_void_p if "*" in d else ctype[base]), name
    from pivot_place import engine
    lib = engine.load_library()
    assert lib.pvt_rt_rows(None, None) == _abi.PVT_EINVAL


# ---- ResidentCluster.place(routes=...) over a fake engine --------------------------------------------
class FakeRowsEngine:
    """What place(routes=...) asks of an engine, on CPU tensors: rt_rows by the checker, run by
    the oracle on the rows the struct points at."""

    def __init__(self):
        import torch
        self.torch = torch
        self.device = torch.device("cpu")
        self.asked = []             # per rt_rows call: (anchors or None, RouteQueues, out's elements)
        self.ran = []               # per run: the rows the round pointed at, or None

    def restore_hosts(self, work, level, hosts):
        assert int(hosts.max()) == -1           # run() places nothing: no host is stale

    def rt_rows(self, zone, bw, group_anchor, rq, out=None):
        got = RouteQueues(*(getattr(rq, n).numpy() for n in ("anchor", "host", "dir", "bw", "off", "mbs")))
        anchors = None if group_anchor is None else group_anchor.numpy()
        H = zone.numel()
        Z = int(round(bw.numel() ** 0.5))
        rows = realtime_rows(zone.numpy(), bw.numpy().reshape(Z, Z), anchors, got)
        self.asked.append((anchors, got, out.numel()))
        out[:rows.size] = self.torch.from_numpy(rows.ravel())
        return out[:rows.size].view(-1, H)

    def run(self, dr):
        s = dr.struct
        n = max(s.n_groups if s.task_group else 0, 1) * s.n_hosts
        self.ran.append(None if not s.rt_bw else np.ctypeslib.as_array(
            ctypes.cast(s.rt_bw, ctypes.POINTER(ctypes.c_double)), (n,)).copy())


def _cluster(r):
    eng = FakeRowsEngine()
    return eng, ResidentCluster(eng, r.avail, r.zone, r.cost, r.bw)


def test_place_with_routes_over_a_fake_engine():
    import rt_bw_cases
    r, rq = rr.e2e_round(_abi.PVT_CA_BF, rr.E2E_RESIDENT)
    full, _, _ = rr.e2e_reference(_abi.PVT_CA_BF, rr.E2E_RESIDENT)
    eng, rc = _cluster(r)
    start = rc.bytes_uploaded
    rc.place(r, routes=rq)
    assert rc.bytes_uploaded - start == rr.round_upload_bytes(r, rq)            # the sparse arrays only
    assert rq.nbytes == rq.n_routes * 28 + 8 + rq.n_packets * 8
    assert rr.round_upload_bytes(r, rq) < r.n_groups * r.n_hosts * 8
    (anchors, got, cap), = eng.asked
    assert anchors.tobytes() == r.group_anchor.tobytes()                          # the round's anchors
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got.arrays(), rq.arrays()))
    assert _bits(eng.ran[0]) == _bits(full.rt_bw)
    # a smaller round reuses the buffer; a larger one grows it
    ff = rr.e2e_round(_abi.PVT_CA_FF, rr.E2E_RESIDENT)[0]
    small = rt_bw_cases.few_groups(_abi.PVT_CA_BF, r.n_hosts, 50, 5, 3)
    small.rt_bw = None
    rc.place(small, routes=routes.empty_queues())
    assert eng.asked[-1][2] == cap and len(eng.ran[-1]) == 3 * r.n_hosts
    # a round without task_group: one row, anchored at zone 0
    single = r.copy()
    single.task_group = single.group_anchor = None
    rc.place(single, routes=rq)
    assert eng.asked[-1][0] is None
    assert _bits(eng.ran[-1]) == _bits(realtime_rows(r.zone, r.bw, None, rq))
    # rt_bw and routes together, routes on another policy
    with pytest.raises(ValueError, match="rt_bw"):
        rc.place(full, routes=rq)
    vbp = rt_bw_cases._plain(_abi.PVT_VBP_FF, r.n_hosts, 10, 1)
    with pytest.raises(ValueError, match="cost_aware"):
        rc.place(vbp, routes=rq)
    # unsorted first-fit reads no route: no rows asked for, nothing of the list uploaded, no rt_bw
    n, before = len(eng.asked), rc.bytes_uploaded
    unsorted = ff.copy()
    unsorted.sort_hosts = False
    rc.place(unsorted, routes=rq)
    assert len(eng.asked) == n and eng.ran[-1] is None
    assert rc.bytes_uploaded - before == rr.round_upload_bytes(unsorted, routes.empty_queues()) - 8
    # sorted first-fit asks for them; the default call is unchanged
    rc.place(ff, routes=rq)
    assert len(eng.asked) == n + 1 and eng.ran[-1] is not None
    rc.place(full)
    assert len(eng.asked) == n + 1 and _bits(eng.ran[-1]) == _bits(full.rt_bw)
    rc.place(r)
    assert eng.ran[-1] is None


@pytest.mark.parametrize("kind", sorted(rr.E2E_KINDS))
@pytest.mark.parametrize("size", [rr.E2E_RESIDENT, rr.E2E_WINDOWED], ids=["h600", "h5000"])
@pytest.mark.parametrize("mode", [_abi.PVT_CA_BF, _abi.PVT_CA_FF], ids=["bf", "ff"])
def test_end_to_end_rounds_depend_on_their_queues(mode, size, kind):
    """On the oracle alone: the end-to-end rounds of test_gpu_rt_rows.py place differently with
    their queues than with idle rows, and their list is the smaller upload."""
    r, rq = rr.e2e_round(mode, size, kind)
    full, ref, idle = rr.e2e_reference(mode, size, kind)
    assert len(set(r.group_anchor.tolist())) == (rr.E2E_ANCHORS if kind == "shared" else r.n_groups)
    assert int((ref.placement >= 0).sum()) > 0
    assert not np.array_equal(ref.placement, idle.placement)
    assert rr.round_upload_bytes(r, rq) < r.n_groups * r.n_hosts * 8
    assert np.isfinite(full.rt_bw).all() and (full.rt_bw > 0).all()
