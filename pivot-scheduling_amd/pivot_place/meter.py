"""Meter aggregates on the GPU (reference resources/meter.py:31-53).

The reference Meter logs host check-ins / check-outs and per-route packet transfers during a
simulation, and its three aggregate properties fold those logs with Python sums:

    cumulative_instance_hours    sum_h sum_intervals (end - start) / 3600        (:31-33)
    total_network_traffic_cost   sum_routes cost[src, dst] * sum sizes / 8000     (:35-42)
    average_congestion_delay     mean gap between a packet's consecutive transfers (:44-53)

``MeterLog`` packs the logs of any number of scenarios into nested CSR arrays (the layout of
``pvt_meter_log`` in include/pivot_place.h); ``PlacementEngine.meter`` reduces a whole batch
in one launch (one workgroup per scenario). ``MeterAggregatesMixin`` is the drop-in: mixed in
front of the reference's Meter, its three properties come from the GPU. fp64 throughout;
within 1e-9 relative of the reference's left-to-right sums (tests/test_meter.py).

The usage series are the other half of the reference meter (:135-179): per time bucket of
``sample_size`` seconds the number of hosts in use (``plot_host_usage``, which ``Meter.save``
writes to host_usage.json on every run) and the mean utilisation of each resource
(``plot_resource_usage``), with their averages (``get_avg_*_usage``). ``UsageLog`` /
``pack_usage`` pack the host intervals and the usage records of any number of scenarios (the
layout of ``pvt_usage_log``), ``PlacementEngine.meter_usage`` computes every series of a batch
in one launch, ``usage_series`` turns its dense output into the reference's ``(x, y)`` lists and
``MeterUsageMixin`` is the drop-in. The host series and its average are exact; the resource
means are within 1e-9 relative of numpy's (tests/test_gpu_meter_usage.py).
"""
import dataclasses

import numpy as np

from . import _abi


@dataclasses.dataclass
class MeterLog:
    host_off: np.ndarray    # [S+1] int64
    iv_off: np.ndarray      # [n_host_rows+1] int64
    iv_start: np.ndarray    # [n_iv] float64
    iv_end: np.ndarray
    route_off: np.ndarray   # [S+1] int64
    route_cost: np.ndarray  # [n_routes] float64
    pkt_off: np.ndarray     # [n_routes+1] int64
    tr_off: np.ndarray      # [n_pkts+1] int64
    tr_start: np.ndarray    # [n_tr] float64
    tr_end: np.ndarray
    tr_size: np.ndarray

    @property
    def n_scen(self):
        return len(self.host_off) - 1

    def arrays(self):
        return [(f.name, getattr(self, f.name)) for f in dataclasses.fields(self)]

    def fill(self, ptr, out):
        """A pvt_meter_log over this log; ``ptr(array)`` gives each array's address and
        ``out`` holds the three [S] float64 result arrays' addresses."""
        m = _abi.pvt_meter_log()
        m.n_scen = self.n_scen
        m.reserved = 0
        m.n_host_rows = len(self.iv_off) - 1
        m.n_iv = len(self.iv_start)
        m.n_routes = len(self.route_cost)
        m.n_pkts = len(self.tr_off) - 1
        m.n_tr = len(self.tr_size)
        for name, a in self.arrays():
            setattr(m, name, ptr(a))
        m.instance_hours, m.egress_cost, m.congestion_delay = out
        return m


def pack(scenarios) -> MeterLog:
    """``scenarios``: one dict per scenario with ``hosts`` = [[[start, end], ...] per host] and
    ``routes`` = [(cost, [[(start, end, size), ...] per packet]) per route], both in the
    reference meter's dict order."""
    host_off, iv_off, iv_s, iv_e = [0], [0], [], []
    route_off, rcost, pkt_off, tr_off, ts, te, tz = [0], [], [0], [0], [], [], []
    for sc in scenarios:
        for ivs in sc["hosts"]:
            for v in ivs:
                iv_s.append(v[0])
                iv_e.append(v[1])
            iv_off.append(len(iv_s))
        host_off.append(len(iv_off) - 1)
        for cost, pkts in sc["routes"]:
            rcost.append(cost)
            for trans in pkts:
                for t in trans:
                    ts.append(t[0])
                    te.append(t[1])
                    tz.append(t[2])
                tr_off.append(len(tz))
            pkt_off.append(len(tr_off) - 1)
        route_off.append(len(rcost))
    i64 = lambda x: np.array(x, dtype=np.int64)
    f64 = lambda x: np.array(x, dtype=np.float64)
    return MeterLog(i64(host_off), i64(iv_off), f64(iv_s), f64(iv_e), i64(route_off), f64(rcost),
                    i64(pkt_off), i64(tr_off), f64(ts), f64(te), f64(tz))


def scenario_of(meter):
    """The logs of a reference ``resources.meter.Meter`` (its private dicts, in their order)."""
    meta = meter._Meter__meta
    hosts = [[list(v) for v in vals] for vals in meter._Meter__hosts.values()]
    routes = [(meta.cost[r.src.locality, r.dst.locality],
               [[tuple(t) for t in trans] for trans in pkts.values()])
              for r, pkts in meter._Meter__routes.items()]
    return {"hosts": hosts, "routes": routes}


class MeterAggregatesMixin:
    """Mixed in front of the reference's ``Meter``: the three aggregates come from the GPU."""

    engine = None

    def _pvt_aggregates(self):
        if self.engine is None:
            from .engine import default_engine
            eng = default_engine(0)
        else:
            eng = self.engine
        return eng.meter(pack([scenario_of(self)]))

    @property
    def cumulative_instance_hours(self):
        return float(self._pvt_aggregates()["instance_hours"][0])

    @property
    def total_network_traffic_cost(self):
        return float(self._pvt_aggregates()["egress_cost"][0])

    @property
    def average_congestion_delay(self):
        return float(self._pvt_aggregates()["congestion_delay"][0])


# ------------------------------------------------------------------ usage series (:135-179)
RESOURCES = _abi.USAGE_RESOURCES


@dataclasses.dataclass
class UsageLog:
    sample_size: int
    host_off: np.ndarray    # [S+1] int64
    iv_off: np.ndarray      # [n_host_rows+1] int64
    iv_start: np.ndarray    # [n_iv] float64
    iv_end: np.ndarray
    us_off: np.ndarray      # [n_host_rows+1] int64, or None: no scenario has usage records
    us_time: np.ndarray     # [n_us] float64 (None with us_off)
    us_frac: np.ndarray     # [4, n_us] float64, rows in RESOURCES order (None with us_off)
    bucket_off: np.ndarray  # [S+1] int64: scenario s owns output buckets [off[s], off[s+1])

    @property
    def n_scen(self):
        return len(self.host_off) - 1

    def arrays(self):
        return [(f.name, getattr(self, f.name)) for f in dataclasses.fields(self)
                if f.name != "sample_size"]

    def fill(self, ptr, out):
        """A pvt_usage_log over this log; ``ptr(array)`` gives each array's address and ``out``
        holds the addresses of n_hosts, res_hosts, res_mean and avg."""
        m = _abi.pvt_usage_log()
        m.n_scen = self.n_scen
        m.reserved = 0
        m.sample_size = int(self.sample_size)
        m.n_host_rows = len(self.iv_off) - 1
        m.n_iv = len(self.iv_start)
        m.n_us = 0 if self.us_time is None else len(self.us_time)
        m.n_buckets = int(self.bucket_off[-1])
        for name, a in self.arrays():
            setattr(m, name, None if a is None else ptr(a))
        m.n_hosts, m.res_hosts, m.res_mean, m.avg = out
        return m


def integral_sample_size(sample_size):
    """``sample_size`` as the int the engine takes (1 .. 2^31 - 1), or None when it is not one
    (the engine divides in int64, which is Python's float ``//`` only for an integral size)."""
    if isinstance(sample_size, (bool, np.bool_)):
        return None
    try:
        s = int(sample_size)
    except (TypeError, ValueError, OverflowError):
        return None
    return s if s == sample_size and 1 <= s <= _abi.USAGE_MAX_SAMPLE else None


def pack_usage(scenarios, sample_size) -> UsageLog:
    """``scenarios``: dicts as for ``pack`` (only ``hosts`` is read) with an optional ``usage``
    entry: per host, in ``hosts`` order, ``(times, (cpus, mem, disk, gpus))`` -- the timestamps
    of the host's usage records and the four value lists. A scenario gets
    ``max time // sample_size + 1`` output buckets, 0 without any interval or record."""
    s = integral_sample_size(sample_size)
    if s is None:
        raise ValueError("sample_size must be an integer in [1, 2^31 - 1], got %r" % (sample_size,))
    with_usage = any(sc.get("usage") is not None for sc in scenarios)
    host_off, iv_off, iv_s, iv_e, us_off, us_t, bucket_off = [0], [0], [], [], [0], [], [0]
    us_f = [[], [], [], []]
    for sc in scenarios:
        usage = sc.get("usage")
        if usage is not None and len(usage) != len(sc["hosts"]):
            raise ValueError("usage lists %d hosts, hosts %d" % (len(usage), len(sc["hosts"])))
        t_max = None
        for i, ivs in enumerate(sc["hosts"]):
            for v in ivs:
                iv_s.append(v[0])
                iv_e.append(v[1])
                t_max = max(v[0], v[1]) if t_max is None else max(t_max, v[0], v[1])
            iv_off.append(len(iv_s))
            if usage is not None:
                times, vals = usage[i]
                if any(len(v) != len(times) for v in vals) or len(vals) != 4:
                    raise ValueError("host %d: four value lists as long as its times" % i)
                us_t.extend(times)
                for r in range(4):
                    us_f[r].extend(vals[r])
                if len(times):
                    t_max = max(times) if t_max is None else max(t_max, max(times))
            us_off.append(len(us_t))
        host_off.append(len(iv_off) - 1)
        bucket_off.append(bucket_off[-1] + (0 if t_max is None else int(t_max // s) + 1))
    i64 = lambda x: np.array(x, dtype=np.int64)
    f64 = lambda x: np.array(x, dtype=np.float64)
    return UsageLog(s, i64(host_off), i64(iv_off), f64(iv_s), f64(iv_e),
                    i64(us_off) if with_usage else None, f64(us_t) if with_usage else None,
                    f64(us_f).reshape(4, -1) if with_usage else None, i64(bucket_off))


def usage_of(meter):
    """Host intervals and usage records of a reference ``resources.meter.Meter`` (its private
    ``__hosts`` and ``__usage`` dicts; both list the hosts in check-in order, :59-81,181-187).
    Without any record the ``usage`` entry is None: only the host series exists."""
    hosts = meter._Meter__hosts
    usage = meter._Meter__usage
    sc = {"hosts": [[list(v) for v in vals] for vals in hosts.values()], "routes": [],
          "usage": None}
    if any(len(usage.get(r, ())) for r in RESOURCES):
        rows = []
        for h in hosts:
            recs = [usage.get(r, {}).get(h, ()) for r in RESOURCES]
            rows.append(([t for t, _ in recs[0]], tuple([v for _, v in rr] for rr in recs)))
        sc["usage"] = rows
    return sc


def usage_series(out, sample_size):
    """Per scenario of a ``PlacementEngine.meter_usage`` result the reference's series: a dict
    with ``hosts`` = (x, y) as ``plot_host_usage`` returns it (x the bucket ranges as tuples, y
    the host counts), each of ``RESOURCES`` = (x, y) as ``plot_resource_usage`` does (x the
    bucket starts) and ``avg`` = the five ``get_avg_*_usage`` values (hosts, then RESOURCES).
    Empty buckets are dropped, as the reference's dicts never hold them."""
    s = sample_size
    off = out["bucket_off"]
    series = []
    for i in range(len(off) - 1):
        lo, hi = int(off[i]), int(off[i + 1])
        nh = out["n_hosts"][lo:hi]
        bs = np.flatnonzero(nh).tolist()
        sc = {"hosts": ([(b * s, (b + 1) * s) for b in bs], [int(nh[b]) for b in bs])}
        bs = np.flatnonzero(out["res_hosts"][lo:hi]).tolist()
        for r, name in enumerate(RESOURCES):
            y = out["res_mean"][r, lo:hi]
            sc[name] = ([b * s for b in bs], [y[b] for b in bs])
        sc["avg"] = out["avg"][i]
        series.append(sc)
    return series


class MeterUsageMixin:
    """Mixed in front of the reference's ``Meter``: ``plot_host_usage``, ``plot_resource_usage``
    and the five ``get_avg_*_usage`` come from the GPU, so the reference's own ``save()`` runs
    unchanged on top of it. A ``sample_size`` that is not an integer in [1, 2^31 - 1] goes to
    the class behind the mixin. Every call packs the meter's log and launches once; a sweep that
    wants all series of many meters calls ``usage_series(engine.meter_usage(pack_usage(...)))``
    once instead."""

    engine = None

    def _pvt_usage(self, s, sample_size):
        """The series at the integral size ``s``; x is built from the caller's own
        ``sample_size`` (``b * sample_size``: a float size gives float bounds)."""
        if self.engine is None:
            from .engine import default_engine
            eng = default_engine(0)
        else:
            eng = self.engine
        return usage_series(eng.meter_usage(pack_usage([usage_of(self)], s)), sample_size)[0]

    def plot_host_usage(self, sample_size=100):
        s = integral_sample_size(sample_size)
        if s is None:
            return super().plot_host_usage(sample_size=sample_size)
        return self._pvt_usage(s, sample_size)["hosts"]

    def plot_resource_usage(self, resource, sample_size=100):
        s = integral_sample_size(sample_size)
        if s is None:
            return super().plot_resource_usage(resource, sample_size=sample_size)
        if resource not in RESOURCES:
            return [], []      # the reference's defaultdict: an unknown resource has no records
        return self._pvt_usage(s, sample_size)[resource]

    def _pvt_avg(self, k, name, sample_size):
        s = integral_sample_size(sample_size)
        if s is None:
            return getattr(super(), name)(sample_size=sample_size)
        return self._pvt_usage(s, sample_size)["avg"][k]

    def get_avg_host_usage(self, sample_size=100):
        return self._pvt_avg(0, "get_avg_host_usage", sample_size)

    def get_avg_cpu_usage(self, sample_size=100):
        return self._pvt_avg(1, "get_avg_cpu_usage", sample_size)

    def get_avg_mem_usage(self, sample_size=100):
        return self._pvt_avg(2, "get_avg_mem_usage", sample_size)

    def get_avg_disk_usage(self, sample_size=100):
        return self._pvt_avg(3, "get_avg_disk_usage", sample_size)

    def get_avg_gpus_usage(self, sample_size=100):
        return self._pvt_avg(4, "get_avg_gpus_usage", sample_size)
