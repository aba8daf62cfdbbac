"""A plain reference of the cost_aware grouping and the rounds that pin the device grouping
(csrc/pvt_groups_dev.h ``ca_groups_round``) on every path and at its size edges. No GPU and no
engine: numpy, ``collections`` and the CPU restatement of the placement (``oracle``) only.
tests/test_grouping_cases.py checks this module on the CPU, tests/test_gpu_grouping.py runs its
cases on the device.

``group_reference`` is written straight from the reference's scheduler/cost_aware.py:30-58:
per item the mode of its predecessor placements by ``max(Counter(list).items(), key=...)``,
the group key the storage of that host's zone (the application for an item without
predecessors), groups in an ``OrderedDict`` in first-seen task order, one
``RandomState.randint(0, S)`` per application group in group order.

Every case lives on a small cluster of its own: zone[h] = h % Z, cost 0 on the diagonal and
0.01 * (1 + |a - z|) off it, positive bandwidths, one storage per zone unless the case says
otherwise, and so much room in every zone that each task lands in its group's anchor zone (the
hosts of that zone score zero, best-fit and first-fit with sorted hosts take the first of them
with room). So a wrong anchor moves its group's tasks to another zone, and a wrong group number
shows in ``order``.
"""
import dataclasses
import functools
from collections import Counter, OrderedDict

import numpy as np

from oracle import oracle
from pivot_place import _abi
from pivot_place._abi import RoundArrays

BF, FF = _abi.PVT_CA_BF, _abi.PVT_CA_FF
CHUNK_FUSED, CHUNK_SINGLE = 256, 1024      # tasks per pass: fused instance; single and staged
TASK_COUNTS = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096)
BIG_TASK_COUNTS = (4097, 8193, 16384)      # single path only (the windowed placement)
STORAGES = (1, 2, 3, 31, 32, 33)
POSITIONS = (624, 0, 1, 561, 623)
LIST_LENGTHS = (64, 65, 1024, 1025, 8192, 8193)


def group_reference(task_item, pred_off, pred_host, item_app, storage_zone, zone_storage, zone,
                    mt_state, n_apps=None):
    """(task_group, group_anchor, n_groups, mt_after) of a round's items, or the exception the
    reference raises (returned, not raised): AttributeError for a mode placement that is no
    host and for an anchor zone without storage, RuntimeError("EINVAL") for arrays no reference
    object could have produced (an item or application index out of range)."""
    task_item = np.asarray(task_item)
    C, S = len(pred_off) - 1, len(storage_zone)
    rs = np.random.RandomState(0)
    rs.set_state(("MT19937", np.array(mt_state[:624], dtype=np.uint32), int(mt_state[624]), 0, 0.0))
    groups = OrderedDict()
    modes = {}
    for t, it in enumerate(task_item.tolist()):
        if not 0 <= it < C:
            return RuntimeError("EINVAL: task %d names item %d of %d" % (t, it, C))
        preds = pred_host[pred_off[it]:pred_off[it + 1]]
        if len(preds):
            if it not in modes:
                modes[it] = max(Counter(preds.tolist()).items(), key=lambda x: x[1])[0]
            placement = modes[it]
            if placement < 0:            # cluster.get_host(placement) is None
                return AttributeError("'NoneType' object has no attribute 'locality'")
            s = int(zone_storage[zone[placement]])
            if s < 0:                    # get_storage_by_locality(locality) is None
                return AttributeError("'NoneType' object has no attribute 'locality'")
            key = ("storage", s)
        else:
            ap = int(item_app[it])
            if ap < 0 or (n_apps is not None and ap >= n_apps):
                return RuntimeError("EINVAL: item %d names application %d" % (it, ap))
            key = ("app", ap)
        groups.setdefault(key, []).append(t)
    task_group = np.zeros(len(task_item), dtype=np.int32)
    anchors = []
    for g, ((kind, k), members) in enumerate(groups.items()):
        task_group[members] = g
        anchors.append(int(storage_zone[rs.randint(0, S) if kind == "app" else k]))
    st = rs.get_state()
    mt_after = np.empty(625, dtype=np.uint32)
    mt_after[:624] = st[1]
    mt_after[624] = st[2]
    return task_group, np.array(anchors, dtype=np.int32), len(anchors), mt_after


def mt_at(seed, pos):
    """(625,) MT19937 state at position ``pos``: the key of RandomState(seed) advanced by that
    many 32-bit draws (624: the fresh seed; 0: the key after the first twist, nothing taken)."""
    rs = np.random.RandomState(seed)
    if pos != 624:
        for _ in range(max(pos, 1)):
            rs.randint(0, 1 << 32, dtype=np.uint32)
    out = np.empty(625, dtype=np.uint32)
    out[:624] = rs.get_state()[1]
    out[624] = pos
    return out


def tables(Z):
    a = np.arange(Z)
    d = np.abs(a[:, None] - a[None, :])
    cost = np.where(d == 0, 0.0, 0.01 * (1 + d))
    bw = 10.0 + a[:, None] + 2.0 * a[None, :]
    return cost.astype(np.float64), bw.astype(np.float64)


@dataclasses.dataclass
class Case:
    """A cost_aware round without task_group / group_anchor, and its item arrays."""
    name: str
    r: RoundArrays
    task_item: np.ndarray
    pred_off: np.ndarray
    pred_host: np.ndarray
    item_app: np.ndarray
    n_apps: int
    storage_zone: np.ndarray
    zone_storage: np.ndarray
    mt_state: np.ndarray

    def ca_args(self):
        """The arguments of PlacementEngine.place_cost_aware after the round."""
        return (self.task_item, self.pred_off, self.pred_host, self.item_app, self.n_apps,
                self.storage_zone, self.zone_storage, self.mt_state)

    def groups(self):
        return group_reference(self.task_item, self.pred_off, self.pred_host, self.item_app,
                               self.storage_zone, self.zone_storage, self.r.zone, self.mt_state,
                               n_apps=self.n_apps)

    def completed(self, task_group, group_anchor):
        return dataclasses.replace(self.r, task_group=task_group,
                                   group_anchor=group_anchor if len(group_anchor) else
                                   np.zeros(1, dtype=np.int32))


def tied_list(n, first, second, third):
    """``n`` entries, ``first`` and ``second`` alternating with equal counts (``first`` seen
    first: it must win); an odd list ends with one entry of ``third``."""
    lst = np.where(np.arange(n) % 2 == 0, first, second).astype(np.int32)
    if n % 2:
        lst[-1] = third
    return lst


def build(name, specs, mode=BF, S=4, Z=None, H=None, n_apps=None, pos=624, seed=11, lists=None,
          storage_zone=None, zone_storage=None):
    """The case of tasks with the group keys ``specs``: k >= 0 the storage k, -1 - j the
    application j. Two items per key (tasks take them by the parity of their index), short
    predecessor lists whose mode host lies in the storage's zone; ``lists``: {storage key: n}
    gives that key one item with a tied list of n entries instead."""
    specs = np.asarray(specs, dtype=np.int64)
    T = len(specs)
    if storage_zone is None:
        Z = Z or S
        storage_zone = np.arange(S) % Z
    storage_zone = np.asarray(storage_zone, dtype=np.int32)
    S = len(storage_zone)
    Z = Z or int(storage_zone.max()) + 1
    if zone_storage is None:             # dict semantics: the last storage of a zone answers
        zone_storage = np.full(Z, -1, dtype=np.int32)
        zone_storage[storage_zone] = np.arange(S)
    zone_storage = np.asarray(zone_storage, dtype=np.int32)
    if H is None:
        H = Z * max(2, min(300 // Z, 24))
    Hz = H // Z
    zone = (np.arange(H) % Z).astype(np.int32)
    lists = lists or {}
    items, task_item, off, lst, item_app = {}, [], [0], [], []
    for t, k in enumerate(specs.tolist()):
        ik = (k, 0 if k in lists else t & 1)
        i = items.get(ik)
        if i is None:
            i = items[ik] = len(items)
            if k >= 0:
                zk = int(storage_zone[k])
                assert zone_storage[zk] == k, "storage %d does not answer for its zone" % k
                zo, z3 = (zk + 1) % Z, (zk + 2) % Z
                if k in lists:
                    # the first-seen host is the zone's last one, the other the lowest host of
                    # the next zone: a sort by host index puts the loser in front
                    lst.extend(tied_list(lists[k], zk + Z * (Hz - 1), zo, z3 if Z > 2 else -1))
                else:
                    hk, ho = zk + Z * ((k + ik[1]) % Hz), zo + Z * (k % Hz)
                    lst.extend([hk, ho, hk] if ik[1] == 0 else [ho, -1, hk, hk])
                item_app.append(0)
            else:
                item_app.append(-1 - k)
            off.append(len(lst))
        task_item.append(i)
    if n_apps is None:
        n_apps = max([-k for k in specs.tolist() if k < 0] + [0])
    cost, bw = tables(Z)
    tt = np.arange(T)
    dem = np.zeros((4, T))
    dem[0] = (1 + tt % 3) / 64.0
    dem[1] = (1 + (tt // 3) % 2) / 64.0
    avail = np.ones((4, H))
    avail[:2] = (-(-T // Hz) + 2) * 3 / 64.0 + 1 / 128.0     # every zone holds the whole round
    r = RoundArrays(mode=mode, avail=avail, zone=zone, dem=dem, cost=cost, bw=bw,
                    sort_tasks=mode == FF, sort_hosts=mode == FF)
    return Case(name, r, np.array(task_item, dtype=np.int32), np.array(off, dtype=np.int64),
                np.array(lst, dtype=np.int32), np.array(item_app, dtype=np.int32), int(n_apps),
                storage_zone, zone_storage, mt_at(seed, pos))


def mixed(T, S, n_apps, seed):
    """Random keys, storages and applications interleaved."""
    rs = np.random.RandomState(seed)
    return np.where(rs.randint(0, 2, T) == 0, rs.randint(0, S, T), -1 - rs.randint(0, n_apps, T))


def fresh_keys(T, at, S=8, first_new=1):
    """Storage 0 everywhere (a key first seen in task 0 and used again in every chunk), and at
    each task of ``at`` a key not seen before: storages 1..S-1, then applications."""
    specs = np.zeros(T, dtype=np.int64)
    for n, t in enumerate(sorted(at)):
        k = first_new + n
        specs[t] = k if k < S else -1 - (k - S)
    return specs


def _numbering():
    T = 4096
    out = []
    f, s = CHUNK_FUSED, CHUNK_SINGLE
    out.append(("chunk_last", fresh_keys(T, [c * f - 1 for c in range(1, T // f + 1)])))
    out.append(("chunk_first", fresh_keys(T, [c * f for c in range(1, T // f)])))
    lanes = {c * f + (c % 4) * 64 + l for c in range(1, T // f) for l in (0, 63)}
    lanes |= {c * s + 64 * w + l for c in range(1, T // s) for w in (5, 15) for l in (0, 63)}
    out.append(("lanes_0_63", fresh_keys(T, lanes)))
    # lanes 960..1023 of a 1024-task pass are lanes 192..255 of a 256-task pass
    last = {c * s + 960 + 9 * j for c in range(T // s) for j in range(8)} | {T - 1}
    out.append(("last_wave", fresh_keys(T, last)))
    # an application first seen in chunk 0, used again in every later chunk of either size
    specs = fresh_keys(T, [c * f + 7 for c in range(1, T // f)])
    specs[3] = -1 - 4000
    specs[[c * f + 100 for c in range(1, T // f)]] = -1 - 4000
    out.append(("reused_key", specs))
    out.append(("one_group", np.zeros(T, dtype=np.int64)))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """Every case by name (built once; the arrays are shared: copy before changing one)."""
    out = []
    for n, T in enumerate(TASK_COUNTS + BIG_TASK_COUNTS):
        out.append(build("tasks_%d" % T, mixed(T, 4, 6, T), mode=(BF, FF)[n % 2]))
    out.append(build("hosts_5000", mixed(1024, 4, 6, 5), H=5000))
    for n, (name, specs) in enumerate(_numbering()):
        out.append(build(name, specs, mode=(FF, BF)[n % 2], S=8))
    out.append(build("all_apps_4096", -1 - np.arange(4096), S=4))
    # S + n_apps = 8192, the key limit, and S = 1: no draw for 8191 application groups
    out.append(build("all_apps_8191", -1 - np.arange(8191), storage_zone=[0], Z=2, mode=FF))
    for n, S in enumerate(STORAGES):
        kw = dict(mode=(BF, FF)[n % 2])
        if S == 1:
            kw.update(storage_zone=[0], Z=2)         # zone 1 has hosts and no storage
        elif S == 33:
            kw.update(storage_zone=np.arange(33) % 11)   # three storages per zone
        specs = mixed(300, S, 20, 100 + S)
        if S == 33:                                  # (only a zone's last storage answers)
            specs = np.where(specs >= 0, 22 + specs % 11, specs)
        out.append(build("storages_%d" % S, specs, S=S, **kw))
    # application groups at every other group number: sparse 32-group words
    alt = np.empty(64, dtype=np.int64)
    alt[0::2], alt[1::2] = np.arange(32), -1 - np.arange(32)
    out.append(build("sparse_words", np.concatenate([alt, mixed(200, 32, 32, 8)]), S=32))
    # groups 0..31 all applications (one full word), then a storage, then alternating
    out.append(build("full_word", np.concatenate([-1 - np.arange(32), [0], alt + 0,
                                                  mixed(200, 32, 64, 9)]), S=32, mode=FF))
    # 700 application groups, S = 33 (a rejection mask of 63): the twist runs inside the draws
    out.append(build("twist", -1 - np.arange(700), S=33, storage_zone=np.arange(33) % 11))
    for pos in POSITIONS:
        out.append(build("position_%d" % pos, mixed(300, 3, 40, 7), S=3, pos=pos, seed=5,
                         mode=(BF, FF)[pos % 2]))
    out.append(build("keys_8192", mixed(300, 4, 50, 3), S=4, n_apps=8188))
    # tied lists at every edge of the anchor kernels; 1025, 8192 and 8193 are deferred
    specs = np.concatenate([np.arange(40) % 6, -1 - np.arange(3), np.arange(6)])
    out.append(build("lists", specs, S=6, lists=dict(zip(range(6), LIST_LENGTHS))))
    out.append(build("lists_b", specs[::-1].copy(), S=6, mode=FF, seed=12,
                     lists={0: 1025, 2: 8193, 3: 1500, 5: 64}))
    out.append(build("zones_40", mixed(300, 40, 20, 40), S=40))
    return OrderedDict((c.name, c) for c in out)


def case(name):
    return cases()[name]


# ---- rounds with a grouping error -------------------------------------------------------------
ERROR_KINDS = ("unplaced", "no_storage", "item_hi", "item_neg", "app_range")
ERROR_T = 4096


@functools.lru_cache(maxsize=None)
def error_base():
    """The healthy round the error cases break: zone 4 has hosts and no storage."""
    return build("error_base", mixed(ERROR_T, 4, 6, 21), S=4, Z=5, zone_storage=[0, 1, 2, 3, -1])


@functools.lru_cache(maxsize=None)
def error_case(kind, at):
    """error_base with task ``at`` made the offender. Returns (case, exception type, pattern)."""
    return broken(error_base(), kind, at)


def broken(b, kind, at):
    """The case ``b`` with task ``at`` made the offender (no_storage: zone 4 must have none)."""
    ti, off, ph, ia = b.task_item.copy(), b.pred_off, b.pred_host, b.item_app
    C = len(ia)
    new = None
    if kind == "unplaced":               # the mode placement is -1
        new, app, exc = [-1, 7, -1], 0, AttributeError
    elif kind == "no_storage":           # the mode host lies in zone 4
        new, app, exc = [4, 9, 4], 0, AttributeError
    elif kind == "app_range":
        new, app, exc = [], b.n_apps, RuntimeError
    elif kind == "item_hi":
        ti[at], exc = C, RuntimeError
    elif kind == "item_neg":
        ti[at], exc = -1, RuntimeError
    if new is not None:
        ti[at] = C
        ph = np.concatenate([ph, np.array(new, dtype=np.int32)])
        off = np.concatenate([off, [len(ph)]]).astype(np.int64)
        ia = np.concatenate([ia, [app]]).astype(np.int32)
    c = dataclasses.replace(b, name="%s_%s_%d" % (b.name, kind, at), task_item=ti, pred_off=off,
                            pred_host=ph, item_app=ia)
    return c, exc, "EINVAL" if exc is RuntimeError else "locality"


# ---- expected results ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def expected(name):
    """(task_group, group_anchor, n_groups, mt_after, oracle.place of the completed round) of a
    case of ``cases()``; computed once and left unchanged."""
    return expected_of(case(name))


def expected_of(c):
    tg, ga, G, mt = c.groups()
    return tg, ga, G, mt, oracle.place(c.completed(tg, ga))


def other_zone(c, z, n=0):
    """Another storage zone than ``z`` (with one storage: another zone of the cluster)."""
    zs = [int(x) for x in sorted(set(c.storage_zone.tolist())) if x != z]
    if not zs:
        zs = [x for x in range(c.r.n_zones) if x != z]
    return zs[n % len(zs)]
