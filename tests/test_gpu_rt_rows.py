"""pvt_rt_rows on the device: the realtime-bandwidth rows built from route queues equal
``pivot_place.routes.realtime_rows`` bit for bit (infinities and zeros included) at the smallest
shapes that reach each edge of the kernels, a list that breaks the contract is refused with the
output untouched, calls are deterministic, and ``ResidentCluster.place(r, routes=rq)`` equals the
oracle on the same round with the dense rows (tests/rt_rows_cases.py; test_routes.py shows on the
CPU that the checker equals the reference and that the end-to-end rounds depend on their queues)."""
import types

import numpy as np
import pytest

import rt_rows_cases as rr
from pivot_place import _abi, routes
from pivot_place.routes import RouteQueues, realtime_rows

pytestmark = pytest.mark.gpu

HOSTS = [1, 2, 63, 64, 65, 127, 1000, 4097]      # 4097: three tiles of the fill, a tail of one host
ZONES = [1, 20, 31, 33, 512]
GROUPS = [0, 1, 3, 20, 64]                        # 20 and 64: three and eight chunks of rows
SENTINEL = -12345.678


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def _up(engine, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(engine.device)


def _dev(engine, rq):
    return types.SimpleNamespace(**{n: _up(engine, a) for n, a in zip(
        ("anchor", "host", "dir", "bw", "off", "mbs"), rq.arrays())})


def _rows(engine, zone, bw, anchors, rq, out=None):
    got = engine.rt_rows(_up(engine, zone), _up(engine, bw.ravel()),
                         None if anchors is None else _up(engine, anchors), _dev(engine, rq), out=out)
    return got.cpu().numpy()


def _same(engine, zone, bw, anchors, rq, what):
    want = realtime_rows(zone, bw, anchors, rq)
    got = _rows(engine, zone, bw, anchors, rq)
    assert got.shape == want.shape, what
    if _bits(got) != _bits(want):
        bad = np.argwhere(got.view(np.uint64) != want.view(np.uint64))
        g, h = bad[0]
        raise AssertionError("%s: %d of %d elements differ, first row %d host %d: %r for %r"
                             % (what, len(bad), want.size, g, h, got[g, h], want[g, h]))


def _lists(H, Z, anchors, bw, zone, seed):
    """{R: entries}: none, one, about H, the listed edges, every route of every anchor."""
    named = [0] if anchors is None else sorted(set(int(a) for a in anchors))
    rs = np.random.RandomState(seed)
    pool = named + [(named[0] + 1) % Z]                   # and a zone that may be no group's
    keys = {(pool[rs.randint(len(pool))], int(rs.randint(H)), int(rs.randint(2))) for _ in range(H)}
    about_h = [(a, h, d, float(rs.uniform(1.0, 2e5)),
                [float(x) for x in rs.uniform(1.0, 4000.0, size=rs.randint(0, 5))]) for a, h, d in sorted(keys)]
    out = {"R=0": [], "R=1": [(named[-1], H - 1, 1, 3.5, [2.0, 1.0])], "R~H": about_h,
           "edges": rr.edge_entries(H, Z, named, bw, zone)}
    if len(named) <= 2 or H <= 65:                        # (small H: with 20 and 64 groups too)
        out["every route"] = rr.full_entries(H, Z, named, bw, zone, seed + 1)
    return out


@pytest.mark.parametrize("H", HOSTS)
def test_rows_equal_the_checker(engine, H):
    """Five (Z, G) pairs per H, rotated so that the eight H cover every pair; every list of
    ``_lists`` on each. Odd H with G >= 2 starts rows on odd doubles."""
    k = HOSTS.index(H)
    for i, Z in enumerate(ZONES):
        G = GROUPS[(i + k) % len(GROUPS)]
        bw, zone = rr.table(Z, 100 + Z), rr.zones(H, Z, 200 + H)
        anchors = rr.anchors_of(G, Z, 300 + G + H)
        for name, es in _lists(H, Z, anchors, bw, zone, 400 + H + Z).items():
            rq = RouteQueues.pack(es, H, Z)
            _same(engine, zone, bw, anchors, rq, "H=%d Z=%d G=%d %s (R=%d)" % (H, Z, G, name, rq.n_routes))


def test_every_zone_and_group_pair_is_covered():
    pairs = {(Z, GROUPS[(i + k) % len(GROUPS)]) for k in range(len(HOSTS)) for i, Z in enumerate(ZONES)}
    assert len(pairs) == len(ZONES) * len(GROUPS)
    a = rr.anchors_of(20, 33, 1)
    assert len(set(a.tolist())) < 20 and len(set(a.tolist())) < 33       # shared anchors, unnamed zones


def test_extreme_values(engine):
    """bw = inf (est == 0: the value is bw), subnormal bw, packets that sum to inf, bw = 5e-324,
    in the list and in the table; bits compared, infinities and zeros included."""
    H, Z = 65, 3
    bw = rr.table(Z, 7)
    bw[0, 1], bw[1, 0], bw[2, 2], bw[0, 2] = np.inf, 5e-324, 1e-310, 1e308
    zone = rr.zones(H, Z, 8)
    anchors = np.array([0, 2, 0, 1], dtype=np.int32)
    es = [(0, 0, 0, np.inf, [5.0]), (0, 0, 1, np.inf, []), (0, 1, 0, 1e-310, [1.0, 2.0]),
          (0, 2, 1, 3.0, [1e308, 1e308]), (0, 3, 0, 5e-324, []), (0, 4, 0, 5e-324, [4000.0]),
          (1, 5, 0, 1.7e308, [1e-300]), (2, 64, 1, 2.5e-308, [np.inf]), (2, 63, 0, np.inf, [np.inf])]
    rq = RouteQueues.pack(es, H, Z)
    want = realtime_rows(zone, bw, anchors, rq)
    assert np.isinf(want).any() and (want == 0).any()
    _same(engine, zone, bw, anchors, rq, "extreme values")


def _good(H=40, Z=5):
    bw, zone = rr.table(Z, 11), rr.zones(H, Z, 12)
    rq = RouteQueues.pack(rr.random_entries(np.random.RandomState(13), [1, 3], H, bw, zone, 0.3), H, Z)
    return H, Z, bw, zone, np.array([3, 1, 3], dtype=np.int32), rq


def _mutations():
    H, Z, _, _, _, rq = _good()
    R, P = rq.n_routes, rq.n_packets
    i = R // 2
    assert rq.off[i + 1] > rq.off[i] or rq.off[i + 2] > rq.off[i + 1]
    j = i if rq.off[i + 1] > rq.off[i] else i + 1             # an entry with a packet
    swap = lambda a: np.concatenate((a[:i], a[i + 1:i + 2], a[i:i + 1], a[i + 2:]))
    dup = lambda a: np.concatenate((a[:i + 1], a[i:i + 1], a[i + 2:]))

    def put(name, idx, v):
        def f(d):
            d[name] = d[name].copy()
            d[name][idx] = v
        return f

    def keys(g):
        def f(d):
            for n in ("anchor", "host", "dir"):
                d[n] = g(d[n])
        return f

    def grow(d):
        d["mbs"] = np.concatenate((d["mbs"], [1.0]))

    return {"unsorted keys": keys(swap), "a duplicate key": keys(dup),
            "host high": put("host", 3, H), "host negative": put("host", 0, -1),
            "anchor high": put("anchor", R - 1, Z), "anchor negative": put("anchor", 0, -2),
            "dir": put("dir", 5, 2), "off decreasing": put("off", j + 1, int(rq.off[j]) - 1 if rq.off[j] else P + 1),
            "off[R] != P": grow, "off[0] != 0": put("off", 0, 1),
            "bw zero": put("bw", 7, 0.0), "bw negative": put("bw", 7, -3.0), "bw nan": put("bw", R - 1, np.nan),
            "packet zero": put("mbs", int(rq.off[j]), 0.0), "packet negative": put("mbs", P - 1, -1.0),
            "packet nan": put("mbs", 0, np.nan)}


@pytest.mark.parametrize("what", sorted(_mutations()))
def test_contract_violations_are_refused_and_write_nothing(engine, what):
    import torch
    H, Z, bw, zone, anchors, rq = _good()
    d = dict(zip(("anchor", "host", "dir", "bw", "off", "mbs"), rq.arrays()))
    _mutations()[what](d)
    bad = RouteQueues(**d)
    first = bad.first_bad(H, Z)
    assert first >= 0, "the mutation broke nothing"
    out = torch.full((len(anchors) * H,), SENTINEL, dtype=torch.float64, device=engine.device)
    with pytest.raises(RuntimeError, match=r"EINVAL.*entry %d of the route queues" % first):
        _rows(engine, zone, bw, anchors, bad, out=out)
    assert (out.cpu().numpy() == SENTINEL).all()
    with pytest.raises(ValueError, match="entry %d of the route queues" % first):
        realtime_rows(zone, bw, anchors, bad)
    _same(engine, zone, bw, anchors, rq, "the list as it was")          # the context goes on


def test_group_anchor_and_zone_out_of_range(engine):
    import torch
    H, Z, bw, zone, anchors, rq = _good()
    out = torch.full((len(anchors) * H,), SENTINEL, dtype=torch.float64, device=engine.device)
    for a in (Z, -1):
        with pytest.raises(RuntimeError, match=r"EINVAL.*group_anchor\[1\] = %d" % a):
            _rows(engine, zone, bw, np.array([3, a, 3], dtype=np.int32), rq, out=out)
    z = zone.copy()
    z[17] = Z
    with pytest.raises(RuntimeError, match=r"EINVAL.*zone\[17\] = %d" % Z):
        _rows(engine, z, bw, anchors, rq, out=out)
    assert (out.cpu().numpy() == SENTINEL).all()
    with pytest.raises(ValueError, match="at least"):
        _rows(engine, zone, bw, anchors, rq, out=out[:-1])


def test_calls_are_deterministic_and_write_exactly_their_rows(engine):
    import torch
    H, Z = 1001, 20
    bw, zone = rr.table(Z, 21), rr.zones(H, Z, 22)
    a5 = np.array([4, 9, 4, 0, 19], dtype=np.int32)
    rq = RouteQueues.pack(rr.random_entries(np.random.RandomState(23), [0, 4, 9, 19], H, bw, zone, 0.2), H, Z)
    want = realtime_rows(zone, bw, a5, rq)
    buf = torch.full((5 * H + 7,), SENTINEL, dtype=torch.float64, device=engine.device)
    first = _rows(engine, zone, bw, a5, rq, out=buf)
    again = _rows(engine, zone, bw, a5, rq, out=buf)
    assert _bits(first) == _bits(again) == _bits(want)
    assert (buf.cpu().numpy()[5 * H:] == SENTINEL).all()
    buf.fill_(SENTINEL)
    two = _rows(engine, zone, bw, a5[:2], rq, out=buf)
    host = buf.cpu().numpy()
    assert _bits(two) == _bits(want[:2]) == _bits(host[:2 * H])
    assert (host[2 * H:] == SENTINEL).all()
    buf.fill_(SENTINEL)
    one = _rows(engine, zone, bw, None, rq, out=buf)                      # G = 0: the row of zone 0
    assert _bits(one) == _bits(want[3:4]) and (buf.cpu().numpy()[H:] == SENTINEL).all()
    # a view that starts on an odd double: every row start's alignment flips
    buf.fill_(SENTINEL)
    odd = _rows(engine, zone, bw, a5, rq, out=buf[1:])
    assert _bits(odd) == _bits(want) and buf.cpu().numpy()[0] == SENTINEL


@pytest.mark.parametrize("kind", sorted(rr.E2E_KINDS))
@pytest.mark.parametrize("size", [rr.E2E_RESIDENT, rr.E2E_WINDOWED], ids=["h600", "h5000"])
@pytest.mark.parametrize("mode", [_abi.PVT_CA_BF, _abi.PVT_CA_FF], ids=["bf", "ff"])
def test_resident_cluster_places_from_route_queues(engine, mode, size, kind):
    """Best-fit, and first-fit with sort_hosts; 600 hosts on the resident kernels, 5000 on the
    windowed engine; queues on 40 % of the routes of 2 anchors that 20 groups share, and on 5 %
    of the routes of 20 distinct anchors (rt_rows_cases.e2e_round says why). Placement, order and final availability equal the oracle's on the dense
    rows of the checker; the oracle places differently on idle rows, so the queues count; and
    the round's upload stays below the dense rows' G * H * 8 bytes."""
    from pivot_place.hostops import ResidentCluster
    r, rq = rr.e2e_round(mode, size, kind)
    full, ref, idle = rr.e2e_reference(mode, size, kind)
    assert not np.array_equal(ref.placement, idle.placement)
    cluster = ResidentCluster(engine, r.avail, r.zone, r.cost, r.bw)
    before = cluster.bytes_uploaded
    got = cluster.place(r, want_avail=True, routes=rq)
    sent = cluster.bytes_uploaded - before
    print("uploaded %d bytes for the round, dense rows %d" % (sent, r.n_groups * r.n_hosts * 8))
    assert np.array_equal(got.order, ref.order)
    assert np.array_equal(got.placement, ref.placement)
    assert np.array_equal(got.avail, ref.avail)
    assert sent == rr.round_upload_bytes(r, rq) < r.n_groups * r.n_hosts * 8
    if size == rr.E2E_WINDOWED:
        assert engine.epoch_stats()["frontier_chains"] == 0
    # the same rows through the dense path, and the cluster goes on
    again = ResidentCluster(engine, r.avail, r.zone, r.cost, r.bw).place(full, want_avail=True)
    assert np.array_equal(again.placement, ref.placement) and np.array_equal(again.avail, ref.avail)
