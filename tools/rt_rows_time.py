"""Time of the realtime-bandwidth rows built on the device (pvt_rt_rows; reference
resources/network.py:70-73, scheduler/cost_aware.py:73-79) against the dense upload they replace.

At --hosts hosts (default 1e6), --zones zones (20) and --groups groups (20, one anchor each) and
for each list length of --routes (default 0, 1e4, 1e6), seeded queues of 1 to 6 packets on routes
drawn uniformly from the anchors' 2 * G * H, from data generated here only:
  dense_upload_ms  (A) ``torch.from_numpy(rows).to(device)`` of the dense (G, H) float64 rows, which
                   is what a caller of ``ResidentCluster.place`` pays per realtime round without
                   ``routes=`` -- the rows already built on the CPU; synchronise to synchronise.
  sparse_ms        (B) the upload of the list's six arrays plus ``pvt_rt_rows`` into a buffer that
                   exists (what ``place(routes=...)`` adds to a round); the same clock.
  cpu_build_ms     building the dense rows on the CPU with ``routes.realtime_rows`` (numpy), the
                   median of three: the cheapest a caller of (A) can build them; the reference's
                   own way is 2 * H Python property reads per anchor, which is slower.
(A) and (B) alternate in one process, each --calls (>= 20) times after --warmup (>= 3); median and
minimum are reported. Then, in a pass of its own with the engine's HIP events bound to the
dispatch, the mean time of ``rt_fill_kernel`` alone, its bytes by the model in csrc/pvt_rtrows.hip
(G*H*8 written + ceil(G/8)*H*4 read) and their rate as a share of the achievable HBM rate
(--hbm-tbs, default 6.3). The device rows are checked against ``realtime_rows`` bit for bit.
Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pivot-scheduling_amd"))


def make_queues(np, routes, H, Z, anchors, bw, zone, R, seed):
    rs = np.random.RandomState(seed)
    A = len(anchors)
    key = np.unique(rs.randint(0, 2 * A * H, size=int(R * 1.05) + 16))
    key = np.sort(rs.permutation(key)[:R])
    R = len(key)
    a = anchors[key // (2 * H)].astype(np.int32)
    h = ((key // 2) % H).astype(np.int32)
    d = (key % 2).astype(np.int32)
    order = np.lexsort((d, h, a))
    a, h, d = a[order], h[order], d[order]
    z = zone[h]
    b = np.where(d == 0, bw[a, z], bw[z, a])
    n = rs.randint(1, 7, size=R)
    off = np.concatenate(([0], np.cumsum(n))).astype(np.int64)
    mbs = rs.uniform(1.0, 4000.0, size=int(off[-1]))
    rq = routes.RouteQueues(a, h, d, b, off, mbs)
    assert rq.first_bad(H, Z) == -1
    return rq


def measure(eng, torch, np, routes, H, Z, G, R, warmup, calls, hbm_tbs):
    rs = np.random.RandomState(R + 1)
    bw = rs.uniform(1.0, 2e5, size=(Z, Z))
    zone = rs.randint(0, Z, size=H).astype(np.int32)
    anchors = rs.permutation(Z)[:G].astype(np.int32) if G <= Z else rs.randint(0, Z, size=G).astype(np.int32)
    rq = make_queues(np, routes, H, Z, anchors, bw, zone, R, R + 2)
    t_cpu = []
    for _ in range(3):
        t0 = time.perf_counter()
        dense = routes.realtime_rows(zone, bw, anchors, rq)
        t_cpu.append(time.perf_counter() - t0)
    dense = np.ascontiguousarray(dense)
    dev = eng.device
    d_zone, d_bw = torch.from_numpy(zone).to(dev), torch.from_numpy(bw.ravel()).to(dev)
    d_anchor = torch.from_numpy(anchors).to(dev)
    out = torch.empty(G * H, dtype=torch.float64, device=dev)
    names = ("anchor", "host", "dir", "bw", "off", "mbs")

    def sparse():
        q = types.SimpleNamespace(**{n: torch.from_numpy(a).to(dev) for n, a in zip(names, rq.arrays())})
        return eng.rt_rows(d_zone, d_bw, d_anchor, q, out=out)

    t_a, t_b = [], []
    for i in range(warmup + calls):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        up = torch.from_numpy(dense).to(dev)
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        got = sparse()
        torch.cuda.synchronize(dev)
        t2 = time.perf_counter()
        if i == 0:
            assert got.cpu().numpy().tobytes() == dense.tobytes(), "device rows differ from realtime_rows"
        del up
        if i >= warmup:
            t_a.append(t1 - t0)
            t_b.append(t2 - t1)
    eng.set_profiling(2, "rt_fill_kernel")
    eng.reset_kstats()
    for _ in range(calls):
        sparse()
    k = eng.kernel_kstats("rt_fill_kernel")
    eng.set_profiling(False)
    fill_ms = k["ms"] / max(k["launches"], 1)
    fill_bytes = k["bytes"] / max(k["launches"], 1)
    rate = fill_bytes / (fill_ms * 1e-3) / 1e12 if fill_ms > 0 else 0.0
    return {"routes": rq.n_routes, "packets": rq.n_packets, "sparse_bytes": rq.nbytes,
            "dense_bytes": dense.nbytes,
            "dense_upload_ms_median": statistics.median(t_a) * 1e3, "dense_upload_ms_min": min(t_a) * 1e3,
            "sparse_ms_median": statistics.median(t_b) * 1e3, "sparse_ms_min": min(t_b) * 1e3,
            "cpu_build_ms_median": statistics.median(t_cpu) * 1e3,
            "fill_kernel_ms_mean": fill_ms, "fill_launches": k["launches"], "fill_model_bytes": fill_bytes,
            "fill_tb_per_s": rate, "fill_share_of_hbm": rate / hbm_tbs,
            "checked_against_realtime_rows": True}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hosts", type=int, default=1000000)
    ap.add_argument("--zones", type=int, default=20)
    ap.add_argument("--groups", type=int, default=20)
    ap.add_argument("--routes", type=int, nargs="+", default=[0, 10000, 1000000])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--hbm-tbs", type=float, default=6.3)
    args = ap.parse_args()
    if args.warmup < 3 or args.calls < 20:
        ap.error("at least 3 warm-up calls and 20 timed calls")
    import numpy as np
    import torch
    from pivot_place import routes
    from pivot_place.engine import PlacementEngine
    eng = PlacementEngine(0)
    res = {"metric": "realtime-bandwidth rows from route queues (pvt_rt_rows)", "hosts": args.hosts,
           "zones": args.zones, "groups": args.groups, "warmup": args.warmup, "calls": args.calls,
           "hbm_tb_per_s": args.hbm_tbs,
           "lists": [measure(eng, torch, np, routes, args.hosts, args.zones, args.groups, R,
                             args.warmup, args.calls, args.hbm_tbs) for R in args.routes],
           "note": "dense_upload_ms (A): host clock, synchronise to synchronise, around "
                   "torch.from_numpy(rows).to(device) of the dense (G, H) rows built beforehand; "
                   "sparse_ms (B): the same clock around the upload of the list's six arrays and "
                   "pvt_rt_rows, alternating with (A); cpu_build_ms: routes.realtime_rows on the "
                   "CPU, apart; fill_kernel_ms: HIP events bound to rt_fill_kernel's dispatch, "
                   "separate pass"}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
