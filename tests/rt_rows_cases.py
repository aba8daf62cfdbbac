"""Route queues for test_routes.py (CPU: ``pivot_place.routes`` against the reference's recorded
realtime bandwidths) and test_gpu_rt_rows.py (``pvt_rt_rows`` against ``routes.realtime_rows``, bit
for bit, and ``ResidentCluster.place(routes=...)`` against the oracle).

``fixture()`` is tests/golden/route_queues.json.gz (made by tests/golden/make_route_queues.py from
the reference): states with their listed routes and ``rt_in`` / ``rt_out`` as the reference's
property returned them. Everything else here is seeded and synthetic. Shared results are computed
once: callers must not modify them.
"""
import functools
import gzip
import json
import os

import numpy as np

import rt_bw_cases
from oracle import oracle
from pivot_place import routes
from pivot_place.routes import RouteQueues

HERE = os.path.dirname(os.path.abspath(__file__))

# the end-to-end rounds: (hosts, tasks) on the resident kernels and on the windowed engine
E2E_RESIDENT = (600, 300)
E2E_WINDOWED = rt_bw_cases.WINDOWED
E2E_ANCHORS = 2         # distinct anchor zones of an end-to-end round (see e2e_round)
E2E_SEED = {E2E_RESIDENT: 71, E2E_WINDOWED: 72}


@functools.lru_cache(maxsize=None)
def fixture():
    with gzip.open(os.path.join(HERE, "golden", "route_queues.json.gz"), "rt") as f:
        d = json.load(f)
    d["bw"] = np.array(d["bw"], dtype=np.float64)
    return d


def state_queues(st, n_zones):
    """The RouteQueues of a fixture state: a storage is named by its zone."""
    sz = st["storage_zone"]
    return RouteQueues.pack([(sz[r["k"]], r["h"], r["dir"], r["bw"], r["mbs"]) for r in st["routes"]],
                            len(st["zone"]), n_zones)


def state_rows(st):
    """Per storage, in + out as the reference's policy adds them (cost_aware.py:79,112)."""
    return np.array(st["rt_in"], dtype=np.float64) + np.array(st["rt_out"], dtype=np.float64)


def table(Z, seed):
    """A seeded U(1, 2e5) bandwidth table: 1 / (1 / b) != b for about one entry in nine."""
    return np.random.RandomState(seed).uniform(1.0, 2e5, size=(Z, Z))


def zones(H, Z, seed):
    """Host zones, irregular, every zone < Z; the last zone is used when H allows."""
    z = np.random.RandomState(seed).randint(0, Z, size=H).astype(np.int32)
    z[-1] = Z - 1
    return z


def random_entries(rs, anchors, H, table_bw, zone, frac, max_pkts=6, own_bw=0.0):
    """Entries on a seeded ``frac`` of the 2 * H routes of every anchor in ``anchors``: 1 to
    ``max_pkts`` packets of U(1, 4000) MB on the table's bandwidth; a share ``own_bw`` of them
    get a bandwidth of their own instead."""
    es = []
    for a in anchors:
        for h in range(H):
            for d in (0, 1):
                if rs.random_sample() < frac:
                    b = table_bw[a, zone[h]] if d == 0 else table_bw[zone[h], a]
                    if rs.random_sample() < own_bw:
                        b = float(rs.uniform(1.0, 2e5))
                    es.append((int(a), h, d, float(b),
                               [float(x) for x in rs.uniform(1.0, 4000.0, size=rs.randint(1, max_pkts + 1))]))
    return es


def edge_entries(H, Z, anchors, table_bw, zone):
    """The edges the issue lists, on the first anchor (and one entry on a zone that may be no
    group's): both directions on one pair, only in, only out, the first and the last host, an
    empty queue with a bandwidth of its own, one queue of 300 packets."""
    a = int(anchors[0])
    rs = np.random.RandomState(5)
    es = {}

    def put(an, h, d, b, mbs):
        es[(an, h, d)] = (an, h, d, b, mbs)

    put(a, 0, 0, float(table_bw[a, zone[0]]), [1500.0, 700.0])               # first host, both
    put(a, 0, 1, float(table_bw[zone[0], a]), [12.5])
    put(a, H - 1, 1, 77.25, [])                                               # last host: own bw, empty
    if H > 2:
        put(a, 1, 0, float(table_bw[a, zone[1]]), [3999.0])                   # only in
        put(a, H // 2, 1, float(table_bw[zone[H // 2], a]), [0.5, 0.25])      # only out
    if H > 4:
        put(a, 3, 0, 1234.5, [float(x) for x in rs.uniform(1.0, 4000.0, size=300)])
    other = (a + 1) % Z                                                       # maybe no group's anchor
    put(other, H - 1, 0, 9.0, [1.0, 2.0, 3.0])
    return list(es.values())


def full_entries(H, Z, anchors, table_bw, zone, seed):
    """Every route of every distinct anchor, 1 to 3 packets each."""
    rs = np.random.RandomState(seed)
    return random_entries(rs, sorted(set(int(a) for a in anchors)), H, table_bw, zone, 2.0, max_pkts=3)


def anchors_of(G, Z, seed):
    """G group anchors (None for G = 0) in which anchors repeat when G > 2 and, when Z allows,
    some zone stays without a group."""
    if G == 0:
        return None
    rs = np.random.RandomState(seed)
    pool = rs.permutation(Z)[:max(1, min(Z - 1, (G + 1) // 2))]
    a = pool[rs.randint(0, len(pool), size=G)].astype(np.int32)
    a[0] = pool[0]
    return a


# ---- end to end ----------------------------------------------------------------------------------
E2E_KINDS = {"shared": (0.4, True), "distinct": (0.05, False)}    # queue fraction, anchors folded


@functools.lru_cache(maxsize=None)
def e2e_round(mode, size, kind="shared"):
    """(round without rt_bw, RouteQueues): ``rt_bw_cases._round`` (costs + 0.001: every score
    depends on the bandwidth), first-fit with sort_hosts, and seeded queues on the anchors' routes.

    ``shared``: make_round's groups anchored at E2E_ANCHORS zones in turn, queues on 40 % of the
    anchors' routes. Why the groups share anchors: an entry costs 28 bytes and 8 per packet (1 to
    6: 56 on average), so queues on 40 % of the 2 * A * H routes of A distinct anchors upload about
    45 * A * H bytes against the 8 * G * H of the dense rows. The upload is the smaller one only
    for G > 5.6 * A: with every group on its own anchor (A = G) the list pays off below 7 % of
    the routes queued, not at 40 %. Several groups on one anchor are what the reference's rounds
    have (source tasks are grouped by application, cost_aware.py:45-58, and every such group
    has an anchor storage), so the round keeps make_round's 20 groups and folds their anchors
    onto E2E_ANCHORS zones.

    ``distinct``: make_round's own anchors, one zone per group (20 of them), and queues on 5 % of
    their routes, below that break-even: the fill's three chunks of rows and the patch's scan of
    the anchors run through ``place`` with every anchor different."""
    frac, fold = E2E_KINDS[kind]
    H, T = size
    r = rt_bw_cases._round(mode, H, T, E2E_SEED[size], sort_hosts=True)
    if fold:
        r.group_anchor = (r.group_anchor % E2E_ANCHORS).astype(np.int32)
    else:
        assert len(set(r.group_anchor.tolist())) == r.n_groups > 8
    rs = np.random.RandomState(E2E_SEED[size] + 1)
    es = random_entries(rs, sorted(set(r.group_anchor.tolist())), H, r.bw, r.zone, frac)
    return r, RouteQueues.pack(es, H, r.n_zones)


@functools.lru_cache(maxsize=None)
def e2e_reference(mode, size, kind="shared"):
    """(round with the dense rows, its oracle result, the oracle result on idle rows)."""
    r, rq = e2e_round(mode, size, kind)
    full, idle = r.copy(), r.copy()
    full.rt_bw = routes.realtime_rows(r.zone, r.bw, r.group_anchor, rq)
    idle.rt_bw = routes.realtime_rows(r.zone, r.bw, r.group_anchor, routes.empty_queues())
    return full, oracle.place(full), oracle.place(idle)


def round_upload_bytes(r, rq):
    """What ResidentCluster.place(r, routes=rq) sends: the task arrays and the list."""
    n = r.dem.nbytes + rq.nbytes
    for a in (r.decay, r.task_group, r.group_anchor):
        n += 0 if a is None else a.nbytes
    return n
