#!/usr/bin/env python3
"""Host accounting ops of REFERENCE simulations (test-only; HostResource.subscribe /
unsubscribe, resources/__init__.py:433-461).

Re-runs, under their labels, the simulations behind six of the recorded traces (``TRACES``;
make_golden_sim.py's ``CONFIGS``) with ``HostResource.subscribe`` / ``unsubscribe`` wrapped, in
this process only, to log every op when it has finished (the host's lock serialises the ops of a
host, so that is the order its levels change in): host index, kind, the four amounts, and the
reference's result -- what ``subscribe`` returned, and for ``unsubscribe`` the mask of the
resources whose level it changed. At every recorded (non-empty) round the number of ops logged
so far is noted when the round's state is recorded, which is when the scheduler takes its
snapshot (scheduler/__init__.py:100-103).

An op is not atomic in simulated time: a container's level changes when ``get`` / ``put`` is
called, and the op's process resumes only after the events already queued for that instant, the
scheduler's snapshot among them. A snapshot can therefore fall inside an op (a dozen or so per
run do): it sees the resources the op has moved so far and not the rest. Such an op is logged in
two entries, the part before the snapshot (the amounts moved so far, zeros elsewhere) and the
rest after it. By the rules this is the same op: a subscribe that was accepted as a whole is
accepted in parts, since the host's lock keeps every other op of that host out, and an
unsubscribe treats each resource on its own anyway.

Before anything is written the log is replayed with ``pivot_place.hostops.apply_ops`` against the
simulation's own snapshots and results, and the put-backs the reference skipped are counted.

Output: tests/golden/host_ops.json.gz -- per trace the capacity, the op log (columns), the
per-round op counts and the count of skipped put-backs. Only the fixture travels.
"""
import gzip
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TRACES = ("sim_h12_opportunistic", "sim_h12_vbp_ff", "sim_h12_vbp_bf", "sim_h12_cost_aware",
          "sim_h12_cost_aware_bf", "sim_c1_cost_aware")


def main():
    if os.environ.get("PYTHONHASHSEED") != "0":
        env = dict(os.environ, PYTHONHASHSEED="0")
        sys.exit(subprocess.call([sys.executable] + sys.argv, env=env))
    sys.path.insert(0, HERE)
    import numpy as np
    import make_golden_sim as mgs
    from pivot_place import des, hostops
    des.install(force=True)
    import make_golden as mg
    mg._install_compat()
    import logging
    logging.disable(logging.CRITICAL)
    world = mg.World()
    import resources
    HR = resources.HostResource
    sub0, unsub0 = HR.subscribe, HR.unsubscribe
    log, marks, owner, inflight, split = [], [], {}, [], [0]

    def levels(res):
        return (res.cpus_available, res.mem_available, res.disk_available, res.gpus_available)

    def emit(st, now, ret, final):
        """Log what op ``st`` has done since its last entry: at a snapshot the resources whose
        level it has changed so far, at its end the rest, with the reference's result."""
        left = [r for r in range(4) if not st["done"][r]]
        moved = [r for r in left if now[r] != st["before"][r]]
        part = moved if not final else left
        if not part or (final and len(left) < 4 and all(st["amt"][r] == 0 for r in left)):
            return
        amt = [st["amt"][r] if r in part else 0.0 for r in range(4)]
        if st["kind"] == 0:
            res = int(bool(ret)) if final else 1
        else:
            res = sum(1 << r for r in moved)
        for r in part:
            st["done"][r] = True
        log.append((id(st["res"]), st["kind"]) + tuple(amt) + (res,))

    def wrap(kind, orig):
        def op(self, cpus, mem, disk, gpus):
            gen = orig(self, cpus, mem, disk, gpus)
            st = {"res": self, "kind": kind, "before": None, "done": [False] * 4,
                  "amt": [float(cpus), float(mem), float(disk), float(gpus)]}
            ret = None
            try:
                ev = next(gen)
                while True:
                    got = yield ev
                    if st["before"] is None:     # the lock is held from here on: the op begins
                        st["before"] = levels(self)
                        inflight.append(st)
                    ev = gen.send(got)
            except StopIteration as e:
                ret = e.value
            inflight.remove(st)
            emit(st, levels(self), ret, True)
            return ret
        return op

    subscribe, unsubscribe = wrap(0, sub0), wrap(1, unsub0)
    record0 = mg.record_state

    def record_state(*a, **k):
        for st in inflight:          # an op the snapshot falls into: its part so far
            emit(st, levels(st["res"]), None, False)
            split[0] += 1
        marks.append(len(log))
        return record0(*a, **k)

    HR.subscribe, HR.unsubscribe, mg.record_state = subscribe, unsubscribe, record_state
    specs = {}
    for cfg, n_hosts, n_apps, job_file, pols in mgs.CONFIGS:
        for label, policy, kwargs in pols:
            specs["sim_%s_%s" % (cfg, label)] = (policy, kwargs, n_hosts, n_apps, job_file)
    out = []
    for name in TRACES:
        policy, kwargs, n_hosts, n_apps, job_file = specs[name]
        del log[:], marks[:], inflight[:]
        split[0] = 0
        owner.clear()
        got = []
        tr = mgs.simulate(mg, world, name, policy, kwargs, n_hosts, n_apps, job_file,
                          meter_out=got)
        _, cluster = got[0]
        # the wrapped methods see HostResource objects: find each host's by identity
        for i, h in enumerate(cluster.hosts):
            owner[id(h.resource)] = i
        ops = [(owner[o[0]],) + o[1:] for o in log]
        cap = [[float(h.resource.total_cpus), float(h.resource.total_mem),
                float(h.resource.total_disk), float(h.resource.total_gpus)]
               for h in cluster.hosts]
        assert len(marks) == len(tr["rounds"]), (name, len(marks), len(tr["rounds"]))
        # replay: every snapshot and every result, by the project's own statement of the rules
        H, K = len(cap), len(ops)
        capacity = np.array(cap, dtype=np.float64).T.copy()
        level = capacity.copy()
        host = np.array([o[0] for o in ops], dtype=np.int32)
        kind = np.array([o[1] for o in ops], dtype=np.int32)
        amt = np.array([o[2:6] for o in ops], dtype=np.float64).reshape(K, 4).T.copy()
        want = np.array([o[6] for o in ops], dtype=np.int32)
        avail, done = [None] * H, 0
        for r, m in zip(tr["rounds"], marks):
            ok = hostops.apply_ops(capacity, level, host[done:m], kind[done:m], amt[:, done:m])
            assert np.array_equal(ok, want[done:m]), (name, done, m)
            done = m
            for row in r["avail_delta"]:
                avail[row[0]] = row[1:]
            assert np.array_equal(level, np.array(avail, dtype=np.float64).T), (name, m)
        full = np.where(kind == 1, ((amt > 0).astype(np.int32) << np.arange(4)[:, None]).sum(0), 0)
        skipped = int(sum(bin(int(f) & ~int(w)).count("1") for f, w in zip(full[:done], want[:done])))
        ops_all_skipped = int(sum(bin(int(f) & ~int(w)).count("1") for f, w in zip(full, want)))
        out.append({"name": name, "capacity": cap, "op_host": host.tolist(),
                    "op_kind": kind.tolist(), "op_amt": amt.tolist(), "op_ok": want.tolist(),
                    "round_ops": list(marks), "skipped_putbacks": ops_all_skipped})
        print(name, "hosts", H, "ops", K, "rounds", len(marks), "skipped put-backs",
              ops_all_skipped, "(%d before the last recorded round)" % skipped,
              "refused subscribes", int(((kind == 0) & (want == 0)).sum()),
              "ops in flight at a snapshot", split[0], flush=True)
    path = os.path.join(HERE, "host_ops.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as g:
        g.write(json.dumps(out, separators=(",", ":")).encode())
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
