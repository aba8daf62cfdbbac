"""Contended rounds on clusters of more than 32 zones, for the wide-zone tests.

``contended_round`` is ``synthetic.make_round`` (hosts ``zone = h % Z``, tables from
``wide_zone_tables``) with scarce availability, so the zero-cost hosts of an anchor run out and
cost_aware placements reach positive-cost zones: cpus = 0.5 * randint(0, 9), mem = U(0, mem_hi),
from RandomState(seed + 1000). ``reference`` is the CPU oracle's placement of it (computed once
per case and shared; callers must not modify it), after asserting on the oracle's result that
the round is a contended one: 10-90 % of the tasks placed and, for cost_aware, at least 15 % of
the winners at zero cost and at least 15 % at positive cost."""
import functools

import numpy as np

from oracle import oracle
from pivot_place import _abi, synthetic

ALL_MODES = [_abi.PVT_CA_FF, _abi.PVT_CA_BF, _abi.PVT_OPP, _abi.PVT_VBP_FF, _abi.PVT_VBP_BF]
CA_MODES = (_abi.PVT_CA_FF, _abi.PVT_CA_BF)

# (hosts, tasks, upper memory bound, seed) of the small round per zone count: H = 2Z + 5; T = 400
# up to 65 zones; at 512 zones (1029 hosts) the same availability places 400 tasks at zero cost,
# so the round has more tasks
SMALL = {33: (71, 400, 40000.0, 3), 64: (133, 400, 40000.0, 3), 65: (135, 400, 40000.0, 3),
         512: (1029, 4000, 40000.0, 3)}
# the windowed round: 5000 hosts, several windows of tasks, scarcer memory so a third is placed
LARGE = {33: (5000, 6000, 3000.0, 5), 64: (5000, 6000, 3000.0, 5), 65: (5000, 6000, 3000.0, 5),
         512: (5000, 6000, 3000.0, 5)}


def contended_round(mode, Z, H, T, mem_hi, seed, **kw):
    r = synthetic.make_round(mode, H, T, seed=seed, n_zones=Z, **kw)
    rs = np.random.RandomState(seed + 1000)
    r.avail[0] = 0.5 * rs.randint(0, 9, size=H)
    r.avail[1] = rs.uniform(0, mem_hi, size=H)
    return r


def fractions(r, ref):
    """(placed / tasks, zero-cost winners / placed, positive-cost winners / placed)."""
    placed = ref.placement >= 0
    n = int(placed.sum())
    if r.mode not in CA_MODES or n == 0:
        return n / max(r.n_tasks, 1), 0.0, 0.0
    anc = r.group_anchor[r.task_group[placed]]
    z = r.zone[ref.placement[placed]]
    c = r.cost[anc, z] + r.cost[z, anc]
    return n / r.n_tasks, float((c == 0).sum()) / n, float((c > 0).sum()) / n


def assert_contended(r, ref, by_cost=True):
    """by_cost = False: a policy that does not look at costs (first fit by host index)."""
    p, z0, zp = fractions(r, ref)
    assert 0.10 <= p <= 0.90, "placed fraction %.3f" % p
    if r.mode in CA_MODES and by_cost:
        assert z0 >= 0.15 and zp >= 0.15, "zero-cost %.3f, positive-cost %.3f of the winners" % (z0, zp)


@functools.lru_cache(maxsize=None)
def case(mode, Z, size="small"):
    """(round, oracle result) of the contended round of ``mode`` at ``Z`` zones."""
    H, T, mem_hi, seed = (SMALL if size == "small" else LARGE)[Z]
    r = contended_round(mode, Z, H, T, mem_hi, seed)
    ref = oracle.place(r)
    assert_contended(r, ref)
    return r, ref


def fresh(r):
    """A copy of a shared round: the engine writes avail and mt_state of the round it is given."""
    return r.copy()


def dropin_cluster(Z, H, n_containers, T, seed):
    """(cluster, tasks) of the ``fakes`` classes on ``Z`` zones (``wide_zone_tables``): hosts in
    zone ``h % Z`` with contended availability, a storage in every zone, and ready tasks of
    containers with recorded predecessor placements (every fourth container has none: its
    application's group draws its anchor)."""
    import fakes
    rs = np.random.RandomState(seed)
    cost, bw = synthetic.wide_zone_tables(Z, seed)
    zones = [fakes.Locality("cloud%d/region%02d/z%03d" % (z // 31, z % 31, z)) for z in range(Z)]
    ids = ["h%05d" % x for x in rs.permutation(H)]
    hosts = [fakes.Host(ids[h], zones[h % Z],
                        (0.5 * rs.randint(0, 9), rs.uniform(0, 40000.0), 100.0, 1.0), int(rs.randint(0, 4)))
             for h in range(H)]
    storage = [fakes.Storage("s%03d" % z, zones[z]) for z in range(Z)]
    cluster = fakes.Cluster(hosts, storage, fakes.Meta(zones, cost, bw))
    cpus, mem, cum = synthetic.demand_rows()
    rows = np.searchsorted(cum, rs.randint(0, int(cum[-1]), size=T), side="right")
    case = {"containers": [{"app": int(k % 7), "pred_hosts": [] if k % 4 == 3 else
                            [int(x) for x in rs.randint(0, H, size=1 + k % 3)]}
                           for k in range(n_containers)],
            "tasks": {"dem": [[float(cpus[i]), float(mem[i] * synthetic.MEM_SCALE_FACTOR), 0.0, 0.0]
                              for i in rows],
                      "container": [int(x) for x in rs.randint(0, n_containers, size=T)]}}
    return cluster, fakes.build_tasks(case, cluster)
