"""Host accounting between rounds: the reference's ``HostResource.subscribe`` / ``unsubscribe``
(``resources/__init__.py:433-461``, over SimPy containers) as a log of ops on resident levels.

``apply_ops`` states the rules in plain Python, op by op, and never calls the library: it serves
callers without a GPU and it is the checker ``pvt_host_ops_apply`` is tested against (the role
``checks.py`` has for the content rules). ``ResidentCluster`` keeps a cluster's capacities and
levels on the device from round to round: the caller's event loop sends the ops that happened
since the last round (``apply``) and places the next round on the device's own state (``place``),
so no 4 x H snapshot is assembled or uploaded.

Layout: ``capacity`` and ``level`` are (4, H) float64, rows cpus, mem, disk, gpus (the layout of
``RoundArrays.avail``); a log is ``op_host`` (K,) int32, ``op_kind`` (K,) int32 (``SUBSCRIBE`` or
``UNSUBSCRIBE``) and ``op_amt`` (4, K) float64, in event order.

Metering (``resources/meter.py:59-81,181-187``): the reference's ``Meter`` records, at every
``host_check_in`` / ``host_check_out``, the host's ``used / total`` of the four resources and runs
a small state machine over the host's [check-in, check-out] intervals. ``used`` is
``capacity - level``, so a metered log carries a time per entry (``op_time`` (K,) float64) and two
more kinds, ``CHECK_IN`` and ``CHECK_OUT``, whose amounts are ignored. ``apply_meter_ops`` states
those rules op by op on a ``HostMeterState``; ``ResidentCluster(..., meter=True)`` runs them on
the device (``pvt_host_meter_apply`` / ``pvt_host_meter_finish``) and feeds the finished arrays
to ``pvt_meter_usage`` and ``pvt_meter`` without a download.

Realtime bandwidths (``scheduler/cost_aware.py:73-79``, ``resources/network.py:70-73``):
``ResidentCluster.place(r, routes=rq)`` takes a ``routes.RouteQueues`` -- the routes that hold
packets or have a bandwidth of their own -- instead of a dense ``r.rt_bw`` and builds the rows on
the device (``pvt_rt_rows``); ``pivot_place/routes.py`` states that rule in plain Python.
"""
import numpy as np

from . import _abi
from ._abi import RoundArrays, RoundResult

SUBSCRIBE, UNSUBSCRIBE = _abi.HOST_OP_SUBSCRIBE, _abi.HOST_OP_UNSUBSCRIBE
CHECK_IN, CHECK_OUT = _abi.CHECK_IN, _abi.CHECK_OUT
METER_NONE, METER_OPEN, METER_CLOSED = _abi.METER_NONE, _abi.METER_OPEN, _abi.METER_CLOSED
_SCENARIO_OFFSETS = 32             # bytes: the four int64 offsets of one scenario, per reduction
TIME_LIMIT = float(2 ** 52)        # times are finite with 0 <= t < 2^52 (pvt_usage_log's contract)


def _subscribe(level, h, d):
    """HostResource.subscribe (:433-449): refused as a whole when an amount exceeds what is
    available or is negative; otherwise every positive amount is taken (Container.get)."""
    for r in range(4):
        if d[r] > level[r, h] or d[r] < 0:
            return 0
    for r in range(4):
        if d[r] > 0:
            level[r, h] = level[r, h] - d[r]
    return 1


def _unsubscribe(capacity, level, h, d):
    """HostResource.unsubscribe (:451-461): each resource on its own is put back when
    ``0 < d <= used``, with ``used = capacity - level`` (:401-415) rounded once."""
    mask = 0
    for r in range(4):
        used = capacity[r, h] - level[r, h]
        if 0 < d[r] <= used:
            level[r, h] = level[r, h] + d[r]
            mask |= 1 << r
    return mask


def apply_ops(capacity, level, op_host, op_kind, op_amt):
    """Apply the log to ``level`` in place, in log order; returns ``op_ok`` (K,) int32: 0 / 1 for
    a subscribe (refused / taken), the mask of the resources put back (bit r) for an
    unsubscribe. Raises ValueError, before anything is changed, when an op names a host outside
    [0, H) or a kind other than 0 or 1."""
    if not (isinstance(level, np.ndarray) and level.dtype == np.float64):
        raise TypeError("level: a float64 numpy array (it is updated in place)")
    lv = level.reshape(4, -1)
    if lv.size and not np.shares_memory(lv, level):
        raise ValueError("level: not reshapeable to (4, H) in place")
    H = lv.shape[1]
    cap = np.asarray(capacity, dtype=np.float64).reshape(4, H)
    host = np.asarray(op_host, dtype=np.int64).ravel()
    kind = np.asarray(op_kind, dtype=np.int64).ravel()
    K = len(host)
    amt = np.asarray(op_amt, dtype=np.float64).reshape(4, K)
    if len(kind) != K:
        raise ValueError("op_host and op_kind differ in length")
    bad = np.flatnonzero((host < 0) | (host >= H) | ((kind != SUBSCRIBE) & (kind != UNSUBSCRIBE)))
    if len(bad):
        k = int(bad[0])
        raise ValueError("op %d of the host op log: host %d (of %d), kind %d"
                         % (k, host[k], H, kind[k]))
    ok = np.zeros(K, dtype=np.int32)
    with np.errstate(all="ignore"):
        for k in range(K):
            h, d = int(host[k]), amt[:, k]
            if kind[k] == SUBSCRIBE:
                ok[k] = _subscribe(lv, h, d)
            else:
                ok[k] = _unsubscribe(cap, lv, h, d)
    return ok


# ------------------------------------------------------------------------------- metering
class HostMeterState:
    """What the reference ``Meter`` holds per host, by host index: ``intervals[h]`` is
    ``Meter.__hosts[h]`` (lists ``[start]`` or ``[start, end]``), ``usage[h]`` the host's records
    ``(time, cpus, mem, disk, gpus)`` of ``Meter.__usage`` (the four resources share the time).
    ``last_time`` is the time of the last entry applied."""

    def __init__(self, n_hosts):
        self.n_hosts = int(n_hosts)
        self.intervals = [[] for _ in range(self.n_hosts)]
        self.usage = [[] for _ in range(self.n_hosts)]
        self.last_time = 0.0

    def words(self):
        """The per-host state as the device keeps it: (word (H,) int32, start, end (H,)
        float64). ``METER_NONE``: (0, 0); ``METER_OPEN``: (start, 0); ``METER_CLOSED``:
        (start, end) of the host's last interval."""
        H = self.n_hosts
        word, start, end = np.zeros(H, np.int32), np.zeros(H), np.zeros(H)
        for h, ivs in enumerate(self.intervals):
            if ivs:
                word[h] = METER_OPEN if len(ivs[-1]) == 1 else METER_CLOSED
                start[h] = ivs[-1][0]
                end[h] = ivs[-1][1] if len(ivs[-1]) == 2 else 0.0
        return word, start, end

    @property
    def n_final(self):
        """Intervals that no later mark can change: all but each host's last."""
        return sum(max(len(ivs) - 1, 0) for ivs in self.intervals)

    @property
    def n_usage(self):
        return sum(len(u) for u in self.usage)

    def finish(self):
        """The arrays ``pvt_host_meter_finish`` returns, as numpy: rows are the hosts with at
        least one usage record in host-index order (``row_host`` (R,) int32), with ``iv_off``
        (R+1,) int64, ``iv_start`` / ``iv_end``, ``us_off`` (R+1,) int64, ``us_time`` and
        ``us_frac`` (4, n_us). Raises ValueError when a host's last interval is open, as the
        reference's own properties do. Changes nothing."""
        is_open = [h for h, ivs in enumerate(self.intervals) if ivs and len(ivs[-1]) == 1]
        if is_open:
            raise ValueError("%d host(s) with an open interval at finish, the first is host %d"
                             % (len(is_open), is_open[0]))
        rows = [h for h in range(self.n_hosts) if self.usage[h]]
        iv_off, us_off, iv_s, iv_e, us_t = [0], [0], [], [], []
        us_f = [[], [], [], []]
        for h in rows:
            for v in self.intervals[h]:
                iv_s.append(v[0])
                iv_e.append(v[1])
            iv_off.append(len(iv_s))
            for rec in self.usage[h]:
                us_t.append(rec[0])
                for r in range(4):
                    us_f[r].append(rec[1 + r])
            us_off.append(len(us_t))
        return {"row_host": np.array(rows, dtype=np.int32),
                "iv_off": np.array(iv_off, dtype=np.int64),
                "iv_start": np.array(iv_s, dtype=np.float64),
                "iv_end": np.array(iv_e, dtype=np.float64),
                "us_off": np.array(us_off, dtype=np.int64),
                "us_time": np.array(us_t, dtype=np.float64),
                "us_frac": np.array(us_f, dtype=np.float64).reshape(4, -1)}


def _mark(capacity, level, state, h, kind, t):
    """Meter.host_check_in (:59-69) / host_check_out (:71-81) of host ``h`` at time ``t``: the
    usage record first (:181-187), then the interval state machine. Returns the row's code."""
    state.usage[h].append((t,) + tuple(
        float((capacity[r, h] - level[r, h]) / capacity[r, h]) for r in range(4)))
    ivs = state.intervals[h]
    last = ivs[-1] if ivs else None
    if kind == CHECK_IN:
        if last is None:
            ivs.append([t])
            return 1
        if len(last) == 2:
            if t > last[1]:
                ivs.append([t])         # the closed interval is final from here on
                return 2
            last.pop()                  # the reference pops the end: open(start) again
            return 3
        return 4
    if last is None:
        return 0                        # (the reference raises here, after recording usage)
    if len(last) == 1:
        last.append(t)
        return 1
    if t > last[1]:
        last[1] = t
        return 2
    return 3


def apply_meter_ops(capacity, level, state, op_host, op_kind, op_amt, op_time):
    """``apply_ops`` for a metered log: kinds ``SUBSCRIBE`` / ``UNSUBSCRIBE`` as there, and
    ``CHECK_IN`` / ``CHECK_OUT`` of ``op_host[k]`` at ``op_time[k]`` on ``state`` (a
    ``HostMeterState``), whose amounts are ignored. Returns ``op_ok`` (K,) int32: as ``apply_ops``
    for the two ops; for a mark 1..4 (check-in: opened / opened after a closed interval / the end
    popped / already open) or 0..3 (check-out: none before / closed / end moved / end kept).

    Raises ValueError, before anything is changed, naming the first entry with a host outside
    [0, H), a kind outside 0..3, a time that is not finite in [0, 2^52), below its predecessor's
    or below ``state.last_time``, or a host with a capacity that is not positive."""
    if not (isinstance(level, np.ndarray) and level.dtype == np.float64):
        raise TypeError("level: a float64 numpy array (it is updated in place)")
    lv = level.reshape(4, -1)
    if lv.size and not np.shares_memory(lv, level):
        raise ValueError("level: not reshapeable to (4, H) in place")
    H = lv.shape[1]
    if state.n_hosts != H:
        raise ValueError("state holds %d hosts, level %d" % (state.n_hosts, H))
    cap = np.asarray(capacity, dtype=np.float64).reshape(4, H)
    host = np.asarray(op_host, dtype=np.int64).ravel()
    kind = np.asarray(op_kind, dtype=np.int64).ravel()
    time = np.asarray(op_time, dtype=np.float64).ravel()
    K = len(host)
    amt = np.asarray(op_amt, dtype=np.float64).reshape(4, K)
    if len(kind) != K or len(time) != K:
        raise ValueError("op_host, op_kind and op_time differ in length")
    with np.errstate(all="ignore"):
        prev = np.concatenate(([state.last_time], time[:-1]))
        bad = (host < 0) | (host >= H) | (kind < 0) | (kind > CHECK_OUT)
        bad |= ~(np.isfinite(time) & (time >= 0) & (time < TIME_LIMIT) & (time >= prev))
        bad |= ~(cap[:, np.clip(host, 0, H - 1)] > 0).all(axis=0)
    bad = np.flatnonzero(bad)
    if len(bad):
        k = int(bad[0])
        raise ValueError("entry %d of the metered op log: host %d (of %d), kind %d, time %r "
                         "(after %r)" % (k, host[k], H, kind[k], float(time[k]),
                                         float(prev[k])))
    ok = np.zeros(K, dtype=np.int32)
    with np.errstate(all="ignore"):
        for k in range(K):
            h, d = int(host[k]), amt[:, k]
            if kind[k] == SUBSCRIBE:
                ok[k] = _subscribe(lv, h, d)
            elif kind[k] == UNSUBSCRIBE:
                ok[k] = _unsubscribe(cap, lv, h, d)
            else:
                ok[k] = _mark(cap, lv, state, h, int(kind[k]), float(time[k]))
    if K:
        state.last_time = float(time[-1])
    return ok


class DeviceMeter:
    """The caller-owned device state of ``pvt_host_meter``: per host the state word and two
    doubles, and the two append logs -- final intervals (``iv_host``, ``iv_start``, ``iv_end``)
    and usage records (``us_host``, ``us_time``, ``us_frac`` record-major, (capacity, 4)) -- with
    their counts ``n_iv`` / ``n_us`` and ``last_time`` on the host. ``reserve(k)`` grows a log
    that cannot take ``k`` more records by a plain copy."""

    def __init__(self, torch, device, n_hosts, log_capacity=4096):
        self._torch, self.device, self.n_hosts = torch, device, int(n_hosts)
        z = lambda n, dt: torch.zeros(n, dtype=dt, device=device)
        self.st_word = z(self.n_hosts, torch.int32)
        self.st_start, self.st_end = z(self.n_hosts, torch.float64), z(self.n_hosts, torch.float64)
        self.n_iv = self.n_us = 0
        self.last_time = 0.0
        self.iv_cap = self.us_cap = 0
        self.iv_host = self.iv_start = self.iv_end = None
        self.us_host = self.us_time = self.us_frac = None
        self._grow("iv", max(int(log_capacity), 1))
        self._grow("us", max(int(log_capacity), 1))

    def _grow(self, which, cap):
        torch, n = self._torch, getattr(self, "n_" + which)
        for name, dt, w in ((which + "_host", torch.int32, 1),
                            (which + ("_start" if which == "iv" else "_time"), torch.float64, 1),
                            (which + ("_end" if which == "iv" else "_frac"), torch.float64,
                             1 if which == "iv" else 4)):
            new = torch.zeros(cap * w, dtype=dt, device=self.device)
            old = getattr(self, name)
            if old is not None and n:
                new[:n * w].copy_(old[:n * w])
            setattr(self, name, new)
        setattr(self, which + "_cap", cap)

    def reserve(self, k):
        for which in ("iv", "us"):
            need = getattr(self, "n_" + which) + k
            if need > getattr(self, which + "_cap"):
                self._grow(which, max(need, 2 * getattr(self, which + "_cap")))


class ResidentCluster:
    """A cluster whose capacities stay on the device between rounds.

    On the device: ``capacity``, the true ``level`` (it starts as a copy of ``capacity``) and a
    round scratch ``work``. ``apply`` changes the truth, by the reference's rules, as the caller's
    event loop subscribes dispatched tasks and unsubscribes finished ones. ``place`` places a
    round on ``work``: the policy's commits land there only, as the reference's policies commit
    to their snapshot and not to ``HostResource``. Before a round, ``work`` is brought up to date
    from ``level`` for exactly the hosts that can differ -- the hosts of the previous placement
    and the hosts named by the logs applied since -- in one ``pvt_restore_hosts``.

    ``engine``: a ``PlacementEngine`` (or an object with its ``device``, ``host_ops``,
    ``restore_hosts`` and ``run``; ``rt_rows`` as well for ``place(routes=...)``). ``zone``
    (H,), ``cost`` / ``bw`` (Z, Z) and the optional ``tiebreak`` (H,) are the cluster's
    constants, uploaded once. ``bytes_uploaded`` counts every host-to-device byte this object
    sends.

    ``meter=True`` meters the cluster on the device as the reference's ``Meter`` does
    (``resources/meter.py:59-81,181-187``): ``apply`` then requires ``op_time`` and accepts
    ``CHECK_IN`` / ``CHECK_OUT`` entries, ``meter_log`` finishes the run's intervals and usage
    records into device tensors, and ``usage`` / ``instance_hours`` reduce them there. The
    engine then also needs ``host_meter_apply``, ``host_meter_finish``, ``meter_usage_device``
    and ``meter_device``. ``meter_log_capacity``: the append logs' first size (they grow)."""

    def __init__(self, engine, capacity, zone, cost, bw, tiebreak=None, meter=False,
                 meter_log_capacity=4096):
        import torch
        self._torch = torch
        self.engine = engine
        self.device = engine.device
        self.bytes_uploaded = 0
        cap = np.ascontiguousarray(capacity, dtype=np.float64).reshape(4, -1)
        self.n_hosts = cap.shape[1]
        if self.n_hosts < 1:
            raise ValueError("ResidentCluster: at least one host")
        self.capacity = self._up(cap.ravel())
        self.level = self.capacity.clone()
        self.work = self.capacity.clone()
        self.zone = self._up(np.ascontiguousarray(zone, dtype=np.int32))
        self.cost = self._up(np.ascontiguousarray(cost, dtype=np.float64))
        self.bw = self._up(np.ascontiguousarray(bw, dtype=np.float64))
        self.n_zones = int(np.asarray(cost).shape[0])
        self.tiebreak = None if tiebreak is None else self._up(
            np.ascontiguousarray(tiebreak, dtype=np.uint32).view(np.int32))
        if self.zone.numel() != self.n_hosts:
            raise ValueError("ResidentCluster: zone must name every host")
        self._stale = []        # device int32 tensors of hosts where work may differ from level
        self._rt_rows = None    # place(routes=...): the rows built on the device (grows)
        self.meter = (DeviceMeter(torch, self.device, self.n_hosts, meter_log_capacity)
                      if meter else None)

    def _up(self, a):
        """One host-to-device copy of a contiguous numpy array, counted."""
        self.bytes_uploaded += a.nbytes
        return self._torch.from_numpy(a).to(self.device)

    def apply(self, op_host, op_kind, op_amt, op_time=None):
        """Upload a log and apply it to ``level`` (``pvt_host_ops_apply``); returns ``op_ok`` as
        a numpy array. An invalid log raises and changes nothing. A metered cluster takes the
        entries' times ``op_time`` (K,) as well, accepts marks (``pvt_host_meter_apply``) and
        grows its append logs to take the call's records."""
        host = np.ascontiguousarray(op_host, dtype=np.int32).ravel()
        kind = np.ascontiguousarray(op_kind, dtype=np.int32).ravel()
        K = len(host)
        amt = np.ascontiguousarray(op_amt, dtype=np.float64).reshape(4, K)
        if len(kind) != K:
            raise ValueError("op_host and op_kind differ in length")
        if self.meter is None:
            if op_time is not None:
                raise ValueError("op_time: this cluster is not metered (meter=True)")
        else:
            if op_time is None:
                raise ValueError("a metered cluster needs op_time")
            time = np.ascontiguousarray(op_time, dtype=np.float64).ravel()
            if len(time) != K:
                raise ValueError("op_host and op_time differ in length")
        if K == 0:
            return np.zeros(0, dtype=np.int32)
        d_host = self._up(host)
        if self.meter is None:
            ok = self.engine.host_ops(self.capacity, self.level, d_host, self._up(kind),
                                      self._up(amt.ravel()))
        else:
            self.meter.reserve(K)
            ok = self.engine.host_meter_apply(self.meter, self.capacity, self.level, d_host,
                                              self._up(kind), self._up(amt.ravel()),
                                              self._up(time))
        self._stale.append(d_host)
        return ok.cpu().numpy()

    def _metered(self):
        if self.meter is None:
            raise ValueError("this cluster is not metered (meter=True)")
        return self.meter

    def meter_log(self):
        """Finish the metered run so far (``pvt_host_meter_finish``; the cluster may go on and
        finish again): a dict of device tensors ``row_host`` (R,) int32 -- the hosts with a
        usage record, in host-index order -- ``iv_off`` (R+1,) int64, ``iv_start``, ``iv_end``,
        ``us_off`` (R+1,) int64, ``us_time`` and ``us_frac`` (4 * n_us, resource-major), the
        layout ``pvt_meter_log`` and ``pvt_usage_log`` take. Raises when a host's last interval
        is open."""
        return self.engine.host_meter_finish(self._metered())

    def usage(self, sample_size):
        """The usage series of the run so far, the dict ``meter.usage_series`` returns for one
        scenario (``hosts``, the four resources, ``avg``)."""
        from .meter import integral_sample_size, usage_series
        s = integral_sample_size(sample_size)
        if s is None:
            raise ValueError("sample_size must be an integer in [1, 2^31 - 1], got %r"
                             % (sample_size,))
        m = self._metered()
        out = self.engine.meter_usage_device(self.meter_log(), s, m.last_time)
        self.bytes_uploaded += _SCENARIO_OFFSETS
        return usage_series(out, sample_size)[0]

    def instance_hours(self):
        """``Meter.cumulative_instance_hours`` (:31-33) of the run so far, through
        ``pvt_meter`` with no routes."""
        hours = self.engine.meter_device(self.meter_log())["instance_hours"][0]
        self.bytes_uploaded += _SCENARIO_OFFSETS
        return float(hours)

    def refresh(self):
        """Bring ``work`` up to date from ``level`` (``place`` does it before every round)."""
        if not self._stale:
            return
        hosts = self._stale[0] if len(self._stale) == 1 else self._torch.cat(self._stale)
        self.engine.restore_hosts(self.work, self.level, hosts)
        self._stale = []

    def place(self, r: RoundArrays, want_avail=False, routes=None) -> RoundResult:
        """Place ``r``'s tasks on the resident state. ``r.avail`` is neither read nor uploaded,
        and ``r.zone``, ``r.cost``, ``r.bw`` and ``r.tiebreak`` give way to the cluster's own.
        The result's ``avail`` (the scratch after the policy's commits) is None unless
        ``want_avail``.

        ``routes``: a ``routes.RouteQueues`` of a cost_aware round with ``realtime_bw``, in place
        of a dense ``r.rt_bw`` (passing both raises ValueError, and so does ``routes`` on another
        policy). The list is uploaded -- its six arrays, counted in ``bytes_uploaded`` -- and the
        rows of the round's anchors are built on the device (``pvt_rt_rows``) in a buffer the
        cluster keeps and grows. First-fit without ``sort_hosts`` reads no route (reference
        ``scheduler/cost_aware.py:118-119``): nothing is uploaded or built for it."""
        torch = self._torch
        if routes is not None:
            if r.rt_bw is not None:
                raise ValueError("place: routes and r.rt_bw are two sources of the same rows")
            if r.mode not in (_abi.PVT_CA_FF, _abi.PVT_CA_BF):
                raise ValueError("place: routes belong to a cost_aware round, not to %s"
                                 % _abi.MODE_NAMES.get(r.mode, r.mode))
            if r.mode == _abi.PVT_CA_FF and not r.sort_hosts:
                routes = None
        self.refresh()
        T = r.n_tasks
        dr = _ResidentRound()
        dr.arrays, dr.n_hosts, dr.n_zones, dr.avail = r, self.n_hosts, self.n_zones, self.work
        dr.zone, dr.cost, dr.bw, dr.tiebreak = self.zone, self.cost, self.bw, self.tiebreak
        dr.placement = torch.full((max(T, 1),), -1, dtype=torch.int32, device=self.device)
        dr.order = torch.empty(max(T, 1), dtype=torch.int32, device=self.device)
        dr.mt = None if r.mt_state is None else np.array(r.mt_state, dtype=np.uint32)
        if dr.mt is not None:
            self.bytes_uploaded += dr.mt.nbytes          # (the library stages the state itself)
        s = _abi.fill_struct(r)
        s.n_hosts, s.n_zones = self.n_hosts, self.n_zones
        s.avail, s.zone = dr.avail.data_ptr(), dr.zone.data_ptr()
        s.cost, s.bw = dr.cost.data_ptr(), dr.bw.data_ptr()
        s.tiebreak = None if dr.tiebreak is None else dr.tiebreak.data_ptr()
        keep = {}
        for name in ("dem", "decay", "task_group", "group_anchor", "rt_bw"):
            a = getattr(r, name)
            t = None if a is None or a.size == 0 else self._up(np.ascontiguousarray(a).ravel())
            keep[name] = t
            setattr(s, name, None if t is None else t.data_ptr())
        if routes is not None:
            # (rows per group only when the round has groups: pvt_round.rt_bw's convention)
            anchors = keep["group_anchor"] if keep["task_group"] is not None else None
            s.rt_bw = self._route_rows(routes, anchors).data_ptr()
        s.placement, s.order = dr.placement.data_ptr(), dr.order.data_ptr()
        s.mt_state = None if dr.mt is None else dr.mt.ctypes.data
        dr.struct = s
        self.engine.run(dr)
        placement = dr.placement[:T]
        self._stale.append(placement)                    # -1 entries are ignored by the restore
        return RoundResult(placement=placement.cpu().numpy(), order=dr.order[:T].cpu().numpy(),
                           avail=(self.work.cpu().numpy().reshape(4, -1).copy()
                                  if want_avail else None),
                           mt_state=dr.mt)

    def _route_rows(self, routes, anchors):
        """Upload ``routes`` and build the rows of ``anchors`` (a device tensor, or None for the
        one row of zone 0) in the cluster's grow-only buffer; returns the rows."""
        rq = _DeviceQueues()
        for name, a in zip(("anchor", "host", "dir", "bw", "off", "mbs"), routes.arrays()):
            setattr(rq, name, self._up(a))
        need = (1 if anchors is None else anchors.numel()) * self.n_hosts
        if self._rt_rows is None or self._rt_rows.numel() < need:
            self._rt_rows = self._torch.empty(need, dtype=self._torch.float64, device=self.device)
        return self.engine.rt_rows(self.zone, self.bw.view(-1), anchors, rq, out=self._rt_rows)

    def levels(self):
        """The true levels, (4, H) float64, downloaded."""
        return self.level.cpu().numpy().reshape(4, self.n_hosts).copy()


class _DeviceQueues:
    """The six arrays of a ``routes.RouteQueues`` as device tensors (``PlacementEngine.rt_rows``)."""


class _ResidentRound:
    """What ``PlacementEngine.run`` takes: ``struct``, a pvt_round over device arrays (and the
    tensors behind it, kept alive for the call)."""
