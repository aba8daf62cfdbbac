"""Realtime-bandwidth rows from route queues: the rule of ``pvt_rt_rows`` in plain Python.

A cost_aware round with ``realtime_bw`` reads, per group and host, ``in_route.realtime_bw +
out_route.realtime_bw`` of the two routes between the group's anchor storage and the host
(reference ``scheduler/cost_aware.py:73-79,106-112``). A route's realtime bandwidth is
``1 / ((Q + 1) / bw)`` with ``Q`` the sum of the MB of the packets queued on it
(``resources/network.py:70-73``), so an idle route on the zone table's bandwidth
(``resources/gen.py:70-73``) has a value that depends on its zone pair alone. ``RouteQueues`` lists
the routes that carry more than that -- those that hold packets, or whose own ``bw`` is not the
table's -- and ``realtime_rows`` builds the dense ``(G, H)`` rows of ``RoundArrays.rt_bw`` from the
list and the table.

This module never calls the library: it serves callers without a GPU and it is the checker
``pvt_rt_rows`` is tested against (the role ``hostops.apply_ops`` has for ``pvt_host_ops_apply``).

Two things are part of the rule and not to be simplified away. ``1 / ((0 + 1) / b)`` is not ``b``
for about one ``b`` in nine: the two divisions are performed for idle routes too. And ``Q`` is the
sequential left-to-right fp64 sum in queue order, starting from 0, as ``sum()`` of the reference's
list is: the queue is rotated when a partly sent packet is queued again (``network.py:99-100``),
and a rotated queue's sum differs in its last bits in a quarter of the cases.
"""
import numpy as np

IN, OUT = 0, 1      # RouteQueues.dir: storage -> host (in_route), host -> storage (out_route)


def realtime_value(bw, mbs):
    """``NetworkRoute.realtime_bw`` (network.py:70-73) of a route of bandwidth ``bw`` whose queue
    holds packets of ``mbs`` MB, in queue order. IEEE throughout (a zero ``bw`` gives what the
    divisions give, where the reference raises)."""
    s = np.float64(0.0)
    with np.errstate(all="ignore"):
        for m in mbs:
            s = s + np.float64(m)
        bw = np.float64(bw)
        est = (s + np.float64(1.0)) / bw
        return float(np.float64(1.0) / est if est else bw)


def _idle(b):
    """``realtime_value(b, [])`` elementwise."""
    b = np.asarray(b, dtype=np.float64)
    with np.errstate(all="ignore"):
        est = (np.float64(0.0) + np.float64(1.0)) / b
        return np.where(est != 0.0, np.float64(1.0) / est, b)


class RouteQueues:
    """The sparse list: per listed route its key ``anchor`` (the zone of its storage end),
    ``host`` and ``dir`` (``IN`` / ``OUT``), (R,) int32 each, sorted by (anchor, host, dir) without
    duplicates; the route object's own ``bw`` (R,) float64; and its queued packets' remaining MB
    ``mbs`` (P,) float64 in queue order, entry i's at ``off[i]:off[i+1]`` (``off`` (R+1,) int64).
    An entry without packets is legal (a replaced route whose bandwidth is not the table's).

    The constructor takes arrays that are already in that form and checks only what needs no
    cluster; ``check`` tests the whole contract; ``pack`` builds a checked list from entries in
    any order."""

    def __init__(self, anchor, host, dir, bw, off, mbs):
        self.anchor = np.ascontiguousarray(anchor, dtype=np.int32).ravel()
        self.host = np.ascontiguousarray(host, dtype=np.int32).ravel()
        self.dir = np.ascontiguousarray(dir, dtype=np.int32).ravel()
        self.bw = np.ascontiguousarray(bw, dtype=np.float64).ravel()
        self.off = np.ascontiguousarray(off, dtype=np.int64).ravel()
        self.mbs = np.ascontiguousarray(mbs, dtype=np.float64).ravel()
        R = len(self.anchor)
        if not (len(self.host) == len(self.dir) == len(self.bw) == R and len(self.off) == R + 1):
            raise ValueError("RouteQueues: anchor, host, dir and bw of one length R, off of R + 1")

    @property
    def n_routes(self):
        return len(self.anchor)

    @property
    def n_packets(self):
        return len(self.mbs)

    @property
    def nbytes(self):
        """The bytes of the six arrays, which is what an upload of the list costs."""
        return sum(a.nbytes for a in self.arrays())

    def arrays(self):
        return (self.anchor, self.host, self.dir, self.bw, self.off, self.mbs)

    def first_bad(self, n_hosts, n_zones):
        """The first entry that breaks the contract, or -1: the entry ``pvt_rt_rows`` names.
        Entry i is bad when its anchor, host or dir is out of range, its key is not above its
        predecessor's, its bw is not > 0, ``0 <= off[i] <= off[i+1] <= P`` fails (entry 0:
        ``off[0] == 0``; the last: ``off[R] == P``) or one of its packets is not > 0."""
        R, P = self.n_routes, self.n_packets
        if R == 0:
            return -1
        a, h, d = (x.astype(np.int64) for x in (self.anchor, self.host, self.dir))
        bad = (a < 0) | (a >= n_zones) | (h < 0) | (h >= n_hosts) | ((d != 0) & (d != 1))
        bad[1:] |= ~((a[1:] > a[:-1]) | ((a[1:] == a[:-1]) & (
            (h[1:] > h[:-1]) | ((h[1:] == h[:-1]) & (d[1:] > d[:-1])))))
        with np.errstate(invalid="ignore"):
            bad |= ~(self.bw > 0)
            lo, hi = self.off[:-1], self.off[1:]
            rng = (lo >= 0) & (lo <= hi) & (hi <= P)
            rng[0] &= lo[0] == 0
            rng[-1] &= hi[-1] == P
            bad |= ~rng
            pkt_bad = ~(self.mbs > 0)
        if pkt_bad.any():
            for i in np.flatnonzero(rng):
                if pkt_bad[lo[i]:hi[i]].any():
                    bad[i] = True
        nz = np.flatnonzero(bad)
        return int(nz[0]) if len(nz) else -1

    def check(self, n_hosts, n_zones):
        """Raise ValueError naming the first entry that breaks the contract."""
        i = self.first_bad(n_hosts, n_zones)
        if i >= 0:
            raise ValueError(
                "entry %d of the route queues: anchor %d (of %d), host %d (of %d), dir %d, bw %r, "
                "packets [%d, %d) of %d (keys ascend strictly, bw and packets are > 0)"
                % (i, self.anchor[i], n_zones, self.host[i], n_hosts, self.dir[i],
                   float(self.bw[i]), self.off[i], self.off[i + 1], self.n_packets))
        return self

    @classmethod
    def pack(cls, entries, n_hosts, n_zones):
        """A checked list from ``entries``, an iterable of ``(anchor, host, dir, bw, packets)``
        in any order: sorted by (anchor, host, dir); a key listed twice raises, and so does
        every other violation of the contract, before the list is returned."""
        es = sorted(((int(a), int(h), int(d), float(b), [float(m) for m in pk])
                     for a, h, d, b, pk in entries), key=lambda e: e[:3])
        for x, y in zip(es, es[1:]):
            if x[:3] == y[:3]:
                raise ValueError("route queues: route (anchor %d, host %d, dir %d) is listed twice"
                                 % x[:3])
        off = np.zeros(len(es) + 1, dtype=np.int64)
        if es:
            off[1:] = np.cumsum([len(e[4]) for e in es])
        for name, col, hi in (("anchor", 0, n_zones), ("host", 1, n_hosts), ("dir", 2, 2)):
            for e in es:
                if not 0 <= e[col] < hi:       # (before the int32 conversion can wrap it)
                    raise ValueError("route queues: %s %d of route (anchor %d, host %d, dir %d) "
                                     "is outside [0, %d)" % ((name, e[col]) + e[:3] + (hi,)))
        rq = cls([e[0] for e in es], [e[1] for e in es], [e[2] for e in es], [e[3] for e in es],
                 off, [m for e in es for m in e[4]])
        return rq.check(n_hosts, n_zones)

    def values(self):
        """``realtime_value`` of every entry, (R,) float64: the sums run left to right, one
        packet position of every queue at a time."""
        n = np.diff(self.off)
        s = np.zeros(self.n_routes, dtype=np.float64)
        with np.errstate(all="ignore"):
            for j in range(int(n.max()) if len(n) else 0):
                m = n > j
                s[m] = s[m] + self.mbs[self.off[:-1][m] + j]
            est = (s + np.float64(1.0)) / self.bw
            return np.where(est != 0.0, np.float64(1.0) / est, self.bw)


def empty_queues():
    """A list without entries: every route idle on the table."""
    return RouteQueues([], [], [], [], [0], [])


def realtime_rows(zone, bw_table, group_anchor, rq):
    """The rows of ``RoundArrays.rt_bw``, (max(G, 1), H) float64: ``row[g][h] = in + out``, with
    ``in`` the value of the listed route (a, h, IN) or ``realtime_value(bw_table[a][zone[h]],
    [])``, ``out`` likewise with (a, h, OUT) and ``bw_table[zone[h]][a]``, and
    ``a = group_anchor[g]`` -- or zone 0 and one row when ``group_anchor`` is None or empty
    (``pvt_round.rt_bw``'s convention for a round without groups). Raises ValueError when the
    list breaks the contract or an anchor or a zone is out of range."""
    zone = np.asarray(zone, dtype=np.int64).ravel()
    bw_table = np.asarray(bw_table, dtype=np.float64)
    Z, H = bw_table.shape[0], len(zone)
    if bw_table.shape != (Z, Z) or H < 1:
        raise ValueError("realtime_rows: a (Z, Z) table and at least one host")
    anchors = (np.zeros(1, dtype=np.int64) if group_anchor is None or len(group_anchor) == 0
               else np.asarray(group_anchor, dtype=np.int64).ravel())
    rq.check(H, Z)
    for name, v in (("group_anchor", anchors), ("zone", zone)):
        out = np.flatnonzero((v < 0) | (v >= Z))
        if len(out):
            raise ValueError("%s[%d] = %d of the route queues' round (of %d zones)"
                             % (name, out[0], v[out[0]], Z))
    val = rq.values()
    rows = np.empty((len(anchors), H), dtype=np.float64)
    done = {}
    for g, a in enumerate(anchors):
        a = int(a)
        if a not in done:
            inn, out = _idle(bw_table[a, zone]), _idle(bw_table[zone, a])
            mine = rq.anchor == a
            for d, side in ((IN, inn), (OUT, out)):
                sel = mine & (rq.dir == d)
                side[rq.host[sel]] = val[sel]
            done[a] = inn + out
        rows[g] = done[a]
    return rows


def _packets(route):
    """The route's queue, as the reference keeps it (``NetworkRoute.__pkts``, a Store)."""
    return route._NetworkRoute__pkts.items


def queues_of(cluster, tables, anchor_zones):
    """The ``RouteQueues`` of a reference-shaped cluster for the given anchor zones (zone
    indices of ``tables``, the policies' per-cluster tables: ``zones``, ``zone``, ``bw``,
    ``host_ids`` and ``routes_of``): of the routes between each zone's storage
    (``cluster.get_storage_by_locality``) and every host, those that are not idle on the table's
    bandwidth -- a route whose queue holds packets, or whose own ``bw`` differs in bits from the
    table's entry for its zone pair. Read from the objects' own attributes (the queue's
    ``items``, a packet's ``num_mbs``, the route's ``bw``). A missing route, or a zone without a
    storage, raises what ``routes_of`` raises."""
    entries = []
    for a in sorted({int(z) for z in anchor_zones}):
        # (a zone without a storage: routes_of reads None.id and raises, as the reference does)
        ins, outs = tables.routes_of(cluster, cluster.get_storage_by_locality(tables.zones[a]))
        for d, routes in ((IN, ins), (OUT, outs)):
            for h, route in enumerate(routes):
                z = int(tables.zone[h])
                tab = tables.bw[a, z] if d == IN else tables.bw[z, a]
                items = _packets(route)
                own = np.float64(route.bw)
                if items or own.tobytes() != np.float64(tab).tobytes():
                    entries.append((a, h, d, own, [p.num_mbs for p in items]))
    return RouteQueues.pack(entries, len(tables.host_ids), len(tables.zones))
