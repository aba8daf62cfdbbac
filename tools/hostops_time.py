"""Time of the resident cluster state (pvt_host_ops_apply; reference
resources/__init__.py:433-461) against the upload it replaces.

At --hosts hosts (default 1e6) and for each log length of --ops (default 1e3, 2e4, 2e5), seeded
trace-like ops on hosts drawn uniformly (segments of a few ops), from data generated here only:
  log_ms       ``ResidentCluster.apply`` of the log plus the refresh of the round scratch for
               the hosts it names: the log's upload, keys, sort and segment walk, the download of
               the results, then one pvt_restore_hosts; a host clock from a device synchronise to
               a device synchronise.
  snapshot_ms  ``torch.from_numpy(avail).to(device)`` of the 4 x H float64 snapshot, which is what
               a caller of the placement entry points pays per round today (without assembling
               it), synchronise to synchronise.
The two are measured in the same run, alternating, each the median of --calls (>= 20) after
--warmup (>= 3); then, in a pass of its own with the engine's HIP events on, the mean time of
the segment walk alone. Logs up to --check-ops ops are checked against apply_ops. Prints one
JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pivot-scheduling_amd"))

CAP = (16.0, 131072.0, 100.0, 1.0)


def make_log(np, H, K, seed):
    rng = np.random.RandomState(seed)
    host = rng.randint(0, H, size=K).astype(np.int32)
    kind = (rng.rand(K) < 0.4).astype(np.int32)
    amt = np.zeros((4, K))
    amt[0] = rng.choice([0.5, 1.0, 2.0], size=K)
    amt[1] = np.round(rng.uniform(0.01, 2.0, size=K), 2) * 7864.32
    return host, kind, amt


def measure(eng, torch, np, H, K, warmup, calls, check):
    from pivot_place import hostops
    cap = np.repeat(np.array(CAP)[:, None], H, axis=1)
    rc = hostops.ResidentCluster(eng, cap, np.zeros(H, dtype=np.int32), np.zeros((1, 1)),
                                 np.ones((1, 1)))
    start = rc.capacity * 0.5                       # half-used hosts: both kinds of op take
    host, kind, amt = make_log(np, H, K, K)
    snap = np.ascontiguousarray(cap)
    dev = eng.device
    t_log, t_snap = [], []
    ok = None
    for i in range(warmup + calls):
        rc.level.copy_(start)
        rc.work.copy_(start)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        ok = rc.apply(host, kind, amt)
        rc.refresh()
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        up = torch.from_numpy(snap).to(dev)
        torch.cuda.synchronize(dev)
        t2 = time.perf_counter()
        del up
        if i >= warmup:
            t_log.append(t1 - t0)
            t_snap.append(t2 - t1)
    assert torch.equal(rc.level, rc.work)
    checked = False
    if K <= check:
        level = start.cpu().numpy().reshape(4, H).copy()
        want = hostops.apply_ops(cap, level, host, kind, amt)
        assert want.tobytes() == ok.tobytes() and level.tobytes() == rc.levels().tobytes()
        checked = True
    eng.set_profiling(2, "host_ops_kernel")
    eng.reset_kstats()
    for _ in range(calls):
        rc.level.copy_(start)
        rc.apply(host, kind, amt)
    k = eng.kernel_kstats("host_ops_kernel")
    eng.set_profiling(False)
    return {"ops": K, "log_bytes": 40 * K, "snapshot_bytes": 32 * H,
            "log_ms_median": statistics.median(t_log) * 1e3, "log_ms_min": min(t_log) * 1e3,
            "log_ms_max": max(t_log) * 1e3,
            "snapshot_ms_median": statistics.median(t_snap) * 1e3,
            "snapshot_ms_min": min(t_snap) * 1e3, "snapshot_ms_max": max(t_snap) * 1e3,
            "walk_kernel_ms_mean": k["ms"] / max(k["launches"], 1), "walk_launches": k["launches"],
            "refused": int(((kind == 0) & (ok == 0)).sum()), "checked_against_apply_ops": checked}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hosts", type=int, default=1000000)
    ap.add_argument("--ops", type=int, nargs="+", default=[1000, 20000, 200000])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--check-ops", type=int, default=20000)
    args = ap.parse_args()
    if args.warmup < 3 or args.calls < 20:
        ap.error("at least 3 warm-up calls and 20 timed calls")
    import numpy as np
    import torch
    from pivot_place.engine import PlacementEngine
    eng = PlacementEngine(0)
    res = {"metric": "resident host levels (pvt_host_ops_apply)", "hosts": args.hosts,
           "warmup": args.warmup, "calls": args.calls,
           "logs": [measure(eng, torch, np, args.hosts, K, args.warmup, args.calls,
                            args.check_ops) for K in args.ops],
           "note": "log_ms: host clock, synchronise to synchronise, around ResidentCluster.apply "
                   "(upload of the log, keys, sort, walk, results back) and the scratch refresh; "
                   "snapshot_ms: the same clock around torch.from_numpy(avail).to(device) of the "
                   "4 x H snapshot, alternating with it; walk_kernel_ms: HIP events around the "
                   "segment walk, separate pass"}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
