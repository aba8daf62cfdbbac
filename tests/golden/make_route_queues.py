#!/usr/bin/env python3
"""Record route queues and the REFERENCE's realtime bandwidths of them (test-only).

Writes ``tests/golden/route_queues.json.gz`` for ``tests/test_routes.py``: per state the hosts'
zones, the storages' zones, every storage<->host route that is not idle on the zone table's
bandwidth -- its key, its own ``bw`` and its queued packets' ``num_mbs`` in ``Store.items`` order
-- and ``rt_in`` / ``rt_out``, every such route's ``realtime_bw`` exactly as the reference's
property returned it (resources/network.py:70-73). The zone table is written once.

Run by hand where the reference is mounted (``make_golden.py`` says how it is imported); the
tests never run it. The states:
  (a) 12 and 100 hosts with ``make_golden.queue_packets(frac=0.4, max_pkts=6)``;
  (b) the 12-host contention simulation of ``make_golden_sim.py`` (cost_aware), stopped at the
      first round in which a route holds two or more packets, one of them queued again after a
      partial send (``NetworkRoute._transfer``, network.py:99-100, rotates the queue); when no
      round has such a route, a 2500-MB and a 700-MB packet are sent over one route of a fresh
      12-host cluster and the event core is stepped until the first has been queued again;
  (c) the 12-host state of (a) with one route replaced through ``cluster.add_route`` by a route
      of another ``bw`` and an empty queue.
The event core is ``pivot_place.des`` registered as ``simpy``, as in ``make_golden_sim.py``.
"""
import collections
import gzip
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "pivot-scheduling_amd"))
sys.path.insert(0, HERE)

JOBS = "jobs-5000-200-172800-259200.yaml"


class Found(Exception):
    """Raised out of schedule() to stop the simulation at the round that was looked for."""


def _items(route):
    return route._NetworkRoute__pkts.items


def record(world, name, cluster, note):
    """One state. Hosts by their index in cluster.hosts, storages by theirs in cluster.storage."""
    import make_golden as mg
    hosts, storage = cluster.hosts, cluster.storage
    zone = [world.zone_index(h.locality) for h in hosts]
    szone = [world.zone_index(s.locality) for s in storage]
    assert len(set(szone)) == len(szone)          # one storage per zone: the zone names it
    bw = world.meta.bw
    routes = []
    for k, s in enumerate(storage):
        for h, host in enumerate(hosts):
            for d, r, tab in ((0, cluster.get_route(s.id, host.id), bw[(s.locality, host.locality)]),
                              (1, cluster.get_route(host.id, s.id), bw[(host.locality, s.locality)])):
                mbs = [p.num_mbs for p in _items(r)]
                if mbs or r.bw != tab:
                    routes.append({"k": k, "h": h, "dir": d, "bw": r.bw, "mbs": mbs})
    rt_in, rt_out = mg.record_realtime(cluster)
    return {"name": name, "note": note, "zone": zone, "storage_zone": szone, "routes": routes,
            "rt_in": rt_in, "rt_out": rt_out}


def queued_state(world, mg, name, n_hosts, seed):
    env = world.simpy.Environment()
    cluster = world.cluster(env, n_hosts, False)
    rs = world.np.random.RandomState(seed)
    mg.queue_packets(world, cluster, rs, frac=0.4, max_pkts=6)
    return cluster, record(world, name, cluster, "queue_packets(frac=0.4, max_pkts=6), seed %d" % seed)


def contention_state(world, mg, sim):
    """(b): the contention run, stopped inside schedule() at the first qualifying round."""
    from resources.network import Packet
    decrement = Packet.decrement

    def marked(self):
        decrement(self)
        if not self.is_transferred:
            self._sent_part = True              # it goes back to the end of its queue

    Packet.decrement = marked
    out = {}
    policy, kwargs = "cost_aware", dict(sim.SIM_POLICIES[2][2])

    class Watch(mg.POLICIES[policy](world)):
        def schedule(self, tasks):
            cl = self.cluster
            for s in cl.storage:
                for h in cl.hosts:
                    for r in (cl.get_route(s.id, h.id), cl.get_route(h.id, s.id)):
                        it = _items(r)
                        if len(it) >= 2 and any(getattr(p, "_sent_part", False) for p in it):
                            out["state"] = record(
                                world, "sim_h12_contention", cl,
                                "make_golden_sim's 12-host cost_aware run at t=%r: a route with "
                                "%d packets, one queued again after a partial send" % (self.env.now, len(it)))
                            raise Found()
            # (make_golden_sim's recorder wraps _first_fit and notes the groups there)
            self._groups, self._tpos = [], collections.defaultdict(int)
            return super().schedule(tasks)

    try:
        sim.setup(mg, world, "route_queues_h12", policy, kwargs, 12, 100, JOBS, cls=Watch)()
    except Found:
        pass
    finally:
        Packet.decrement = decrement
    return out.get("state")


def requeued_state(world, mg):
    """(b)'s fallback: 2500 MB and 700 MB over one route until the first is queued again."""
    env = world.simpy.Environment()
    cluster = world.cluster(env, 12, False)
    r = cluster.get_route(cluster.storage[0].id, cluster.hosts[0].id)
    env.process(r.send(2500, env.event()))
    env.process(r.send(700, env.event()))
    for _ in range(10000):
        if [p.num_mbs for p in _items(r)] == [700, 1500]:
            break
        env.step()
    assert [p.num_mbs for p in _items(r)] == [700, 1500]
    return record(world, "requeued_h12", cluster,
                  "2500 MB then 700 MB sent over one route; stepped until the first was queued again")


def replaced_state(world, mg, cluster):
    """(c): one idle route of the queued 12-host state replaced by one of another bandwidth."""
    s, h = cluster.storage[-1], cluster.hosts[-1]
    for host in reversed(cluster.hosts):
        if not _items(cluster.get_route(host.id, s.id)):
            h = host
            break
    old = cluster.get_route(h.id, s.id)
    assert not _items(old)
    env = world.simpy.Environment()
    cluster.add_route(world.NetworkRoute(env, h, s, old.bw * 0.37))
    assert cluster.get_route(h.id, s.id).bw != old.bw
    return record(world, "replaced_h12", cluster,
                  "the queued 12-host state with one idle route replaced through add_route "
                  "(bw * 0.37, empty queue)")


def main():
    if os.environ.get("PYTHONHASHSEED") != "0":
        env = dict(os.environ, PYTHONHASHSEED="0")
        sys.exit(subprocess.call([sys.executable] + sys.argv, env=env))
    from pivot_place import des
    des.install(force=True)
    import make_golden as mg
    import make_golden_sim as sim
    mg._install_compat()
    mg._seed_uuid(20261021)
    import logging
    logging.disable(logging.CRITICAL)
    world = mg.World()
    states = []
    c12, st = queued_state(world, mg, "queued_h12", 12, 46)
    states.append(st)
    states.append(queued_state(world, mg, "queued_h100", 100, 47)[1])
    states.append(contention_state(world, mg, sim) or requeued_state(world, mg))
    states.append(replaced_state(world, mg, c12))
    _, bw = world.tables()
    fn = os.path.join(HERE, "route_queues.json.gz")
    with gzip.open(fn, "wt") as f:
        json.dump({"bw": bw, "states": states}, f, separators=(",", ":"))
    for s in states:
        print("%-20s H=%-4d S=%-3d routes=%-5d packets=%-6d longest=%d  %s"
              % (s["name"], len(s["zone"]), len(s["storage_zone"]), len(s["routes"]),
                 sum(len(r["mbs"]) for r in s["routes"]),
                 max([len(r["mbs"]) for r in s["routes"]] or [0]), s["note"]))
    print("%s: %d KB" % (fn, os.path.getsize(fn) // 1024))


if __name__ == "__main__":
    main()
