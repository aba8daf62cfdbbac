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
"""
import numpy as np

from . import _abi
from ._abi import RoundArrays, RoundResult

SUBSCRIBE, UNSUBSCRIBE = _abi.HOST_OP_SUBSCRIBE, _abi.HOST_OP_UNSUBSCRIBE


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
    ``restore_hosts`` and ``run``). ``zone`` (H,), ``cost`` / ``bw`` (Z, Z) and the optional
    ``tiebreak`` (H,) are the cluster's constants, uploaded once. ``bytes_uploaded`` counts every
    host-to-device byte this object sends."""

    def __init__(self, engine, capacity, zone, cost, bw, tiebreak=None):
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

    def _up(self, a):
        """One host-to-device copy of a contiguous numpy array, counted."""
        self.bytes_uploaded += a.nbytes
        return self._torch.from_numpy(a).to(self.device)

    def apply(self, op_host, op_kind, op_amt):
        """Upload a log and apply it to ``level`` (``pvt_host_ops_apply``); returns ``op_ok`` as
        a numpy array. An invalid log raises and changes nothing."""
        host = np.ascontiguousarray(op_host, dtype=np.int32).ravel()
        kind = np.ascontiguousarray(op_kind, dtype=np.int32).ravel()
        K = len(host)
        amt = np.ascontiguousarray(op_amt, dtype=np.float64).reshape(4, K)
        if len(kind) != K:
            raise ValueError("op_host and op_kind differ in length")
        if K == 0:
            return np.zeros(0, dtype=np.int32)
        d_host = self._up(host)
        ok = self.engine.host_ops(self.capacity, self.level, d_host, self._up(kind),
                                  self._up(amt.ravel()))
        self._stale.append(d_host)
        return ok.cpu().numpy()

    def refresh(self):
        """Bring ``work`` up to date from ``level`` (``place`` does it before every round)."""
        if not self._stale:
            return
        hosts = self._stale[0] if len(self._stale) == 1 else self._torch.cat(self._stale)
        self.engine.restore_hosts(self.work, self.level, hosts)
        self._stale = []

    def place(self, r: RoundArrays, want_avail=False) -> RoundResult:
        """Place ``r``'s tasks on the resident state. ``r.avail`` is neither read nor uploaded,
        and ``r.zone``, ``r.cost``, ``r.bw`` and ``r.tiebreak`` give way to the cluster's own.
        The result's ``avail`` (the scratch after the policy's commits) is None unless
        ``want_avail``."""
        torch = self._torch
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
        keep = []
        for name in ("dem", "decay", "task_group", "group_anchor", "rt_bw"):
            a = getattr(r, name)
            t = None if a is None or a.size == 0 else self._up(np.ascontiguousarray(a).ravel())
            keep.append(t)
            setattr(s, name, None if t is None else t.data_ptr())
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

    def levels(self):
        """The true levels, (4, H) float64, downloaded."""
        return self.level.cpu().numpy().reshape(4, self.n_hosts).copy()


class _ResidentRound:
    """What ``PlacementEngine.run`` takes: ``struct``, a pvt_round over device arrays (and the
    tensors behind it, kept alive for the call)."""
