#!/usr/bin/env python3
"""Metered host-op logs of REFERENCE simulations (test-only; HostResource.subscribe /
unsubscribe, resources/__init__.py:433-461, and Meter.host_check_in / host_check_out,
resources/meter.py:59-81,181-187).

Re-runs the three simulations of meter_usage.json.gz (make_meter_logs.py's ``RUNS``) with
``HostResource.subscribe`` / ``unsubscribe`` wrapped as make_host_ops.py wraps them, and with
``Meter.host_check_in`` / ``host_check_out`` wrapped to log a mark: host, kind (2 check-in,
3 check-out), ``env.now`` and the row of the meter's state machine the reference took, read off
the host's interval list before and after the call (the codes of
``pivot_place.hostops.apply_meter_ops``). Every entry carries ``env.now`` at the moment it is
logged.

An op of the marked host that is in flight at a mark holds the lock and has moved some of its
resources: the meter sees those. Such an op is logged in two entries around the mark, the rule
make_host_ops.py applies at round snapshots.

Before anything is written the log is replayed with ``apply_meter_ops``; the replay's intervals
and usage records must equal the meter's ``__hosts`` and ``__usage`` bit for bit, its codes the
observed ones, and the hosts' records those of meter_usage.json.gz for the same run (whose
``want`` series are therefore not stored twice).

Output: tests/golden/host_meter.json.gz -- per run the capacity, the log (columns), the number
of entries logged before each recorded round and the number of ops split at a mark. Only the
fixture travels.
"""
import gzip
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
RESOURCES = ("cpus", "mem", "disk", "gpus")


def main():
    if os.environ.get("PYTHONHASHSEED") != "0":
        env = dict(os.environ, PYTHONHASHSEED="0")
        sys.exit(subprocess.call([sys.executable] + sys.argv, env=env))
    sys.path.insert(0, HERE)
    import numpy as np
    from make_meter_logs import RUNS
    import make_golden_sim as mgs
    from pivot_place import des, hostops
    des.install(force=True)
    import make_golden as mg
    mg._install_compat()
    import logging
    logging.disable(logging.CRITICAL)
    world = mg.World()
    import resources
    from resources.meter import Meter
    HR = resources.HostResource
    sub0, unsub0 = HR.subscribe, HR.unsubscribe
    in0, out0 = Meter.host_check_in, Meter.host_check_out
    # a log entry: (environment, id of the HostResource, kind, time, four amounts, result)
    log, rounds, inflight, split = [], [], [], [0]

    def levels(res):
        return (res.cpus_available, res.mem_available, res.disk_available, res.gpus_available)

    def emit(st, now, ret, final):
        """make_host_ops.py's emit: what op ``st`` has done since its last entry."""
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
        env = st["res"]._HostResource__env
        log.append((env, id(st["res"]), st["kind"], float(env.now)) + tuple(amt) + (res,))

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

    def row(kind, before, after, raised):
        """The state machine's row, from the host's interval list before and after the call."""
        last = before[-1] if before else None
        if kind == hostops.CHECK_IN:
            if last is None:
                return 1
            if len(last) == 2:
                return 2 if len(after) > len(before) else 3
            return 4
        if last is None:
            assert raised
            return 0
        if len(last) == 1:
            return 1
        return 2 if after[-1][1] != last[1] else 3

    def mark(kind, orig):
        def m(self, h):
            for st in inflight:      # an op of this host the mark falls into: its part so far
                if st["res"] is h.resource:
                    emit(st, levels(st["res"]), None, False)
                    split[0] += 1
            env = self._Meter__env
            hosts = self._Meter__hosts
            before = [list(v) for v in hosts[h]] if h in hosts else []
            raised = None
            try:
                orig(self, h)
            except Exception as e:      # a check-out before any check-in: usage is recorded
                raised = e
            after = [list(v) for v in hosts[h]] if h in hosts else []
            log.append((env, id(h.resource), kind, float(env.now), 0.0, 0.0, 0.0, 0.0,
                        row(kind, before, after, raised is not None)))
            if raised is not None:
                raise raised
        return m

    record0 = mg.record_state

    def record_state(*a, **k):
        rounds.append(len(log))
        return record0(*a, **k)

    HR.subscribe, HR.unsubscribe = wrap(0, sub0), wrap(1, unsub0)
    Meter.host_check_in = mark(hostops.CHECK_IN, in0)
    Meter.host_check_out = mark(hostops.CHECK_OUT, out0)
    mg.record_state = record_state
    with gzip.open(os.path.join(HERE, "meter_usage.json.gz"), "rt") as f:
        recorded = {t["name"]: t for t in json.load(f)}
    out = []
    for name, policy, kwargs, n_hosts, n_apps, job_file in RUNS:
        del log[:], rounds[:], inflight[:]
        split[0] = 0
        got = []
        mgs.simulate(mg, world, name, policy, kwargs, n_hosts, n_apps, job_file, meter_out=got)
        meter, cluster = got[0]
        env = meter._Meter__env
        owner = {id(h.resource): i for i, h in enumerate(cluster.hosts)}
        # (entries of the environment the cluster was generated in are not this run's; the
        # round counts are corrected for them)
        mine = [e[0] is env for e in log]
        before = np.concatenate(([0], np.cumsum(mine)))
        marks = [int(before[m]) for m in rounds]
        ops = [(owner[e[1]],) + e[2:] for e, keep in zip(log, mine) if keep]
        cap = [[float(h.resource.total_cpus), float(h.resource.total_mem),
                float(h.resource.total_disk), float(h.resource.total_gpus)]
               for h in cluster.hosts]
        H, K = len(cap), len(ops)
        capacity = np.array(cap, dtype=np.float64).T.copy()
        level = capacity.copy()
        host = np.array([o[0] for o in ops], dtype=np.int32)
        kind = np.array([o[1] for o in ops], dtype=np.int32)
        time = np.array([o[2] for o in ops], dtype=np.float64)
        amt = np.array([o[3:7] for o in ops], dtype=np.float64).reshape(K, 4).T.copy()
        want = np.array([o[7] for o in ops], dtype=np.int32)
        assert (np.diff(time) >= 0).all(), name
        # replay by the project's own statement of the rules, cut at the rounds
        state = hostops.HostMeterState(H)
        done = 0
        for m in marks + [K]:
            ok = hostops.apply_meter_ops(capacity, level, state, host[done:m], kind[done:m],
                                         amt[:, done:m], time[done:m])
            assert np.array_equal(ok, want[done:m]), (name, done, m)
            done = m
        hidx = {id(h): i for i, h in enumerate(cluster.hosts)}
        usage = meter._Meter__usage
        seen = set()
        for h, vals in meter._Meter__hosts.items():
            i = hidx[id(h)]
            seen.add(i)
            assert state.intervals[i] == [list(v) for v in vals], (name, i)
        for r, res in enumerate(RESOURCES):
            for h, recs in usage[res].items():
                i = hidx[id(h)]
                assert [(u[0], u[1 + r]) for u in state.usage[i]] == [tuple(x) for x in recs], \
                    (name, res, i)
                seen.add(i)
        assert all(not state.usage[i] and not state.intervals[i]
                   for i in range(H) if i not in seen), name
        assert not any(ivs and len(ivs[-1]) == 1 for ivs in state.intervals), name
        rec = recorded[name]["hosts"]
        assert sorted(h["host"] for h in rec) == sorted(i for i in range(H) if state.usage[i]), name
        for h in rec:
            i = h["host"]
            assert h["intervals"] == state.intervals[i], (name, i)
            assert h["times"] == [u[0] for u in state.usage[i]], (name, i)
            assert h["usage"] == [[u[1 + r] for u in state.usage[i]] for r in range(4)], (name, i)
        out.append({"name": name, "capacity": cap, "op_host": host.tolist(),
                    "op_kind": kind.tolist(), "op_time": time.tolist(), "op_amt": amt.tolist(),
                    "op_ok": want.tolist(), "round_ops": marks, "split_at_mark": split[0]})
        print(name, "hosts", H, "entries", K, "marks", int((kind >= 2).sum()), "rounds",
              len(marks), "final intervals", state.n_final, "usage records", state.n_usage,
              "codes", np.bincount(want[kind == 2], minlength=5).tolist(),
              np.bincount(want[kind == 3], minlength=4).tolist(),
              "ops in flight at a mark", split[0], flush=True)
    path = os.path.join(HERE, "host_meter.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as g:
        g.write(json.dumps(out, separators=(",", ":")).encode())
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
