"""Time of the metered resident cluster (pvt_host_meter_apply / pvt_host_meter_finish; reference
resources/meter.py:59-81,181-187), from data generated here only. Three measurements, each the
median of --calls (>= 20) after --warmup (>= 3) with the range, a host clock from a device
synchronise to the call's own synchronisation, the columns of a row alternating in one session:

  old     ``pvt_host_ops_apply`` on mark-free logs of --ops ops at --hosts hosts, device arrays in
          place: the library of --parent-lib (the parent commit's build) against this tree's.
  marks   ``pvt_host_meter_apply`` on the same ops with one mark after each op (2K entries, the
          logs sized before), beside ``old``; and the walk kernel alone by HIP events, in a pass
          of its own.
  finish  one cluster of --rows hosts holding --records usage records (the host rows and records
          of DESIGN §4.2's 4096 synthetic scenarios): ``host_meter_finish`` + the device-tensor
          ``meter_usage_device`` against ``engine.meter_usage`` of the same arrays from host
          memory (what ``pack_usage`` hands it; the packing itself is not timed on either side).
Prints one JSON line.
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


def stats(ts):
    return {"median_ms": statistics.median(ts) * 1e3, "min_ms": min(ts) * 1e3, "max_ms": max(ts) * 1e3}


def make_ops(np, H, K, seed):
    rng = np.random.RandomState(seed)
    host = rng.randint(0, H, size=K).astype(np.int32)
    kind = (rng.rand(K) < 0.4).astype(np.int32)
    amt = np.zeros((4, K))
    amt[0] = rng.choice([0.5, 1.0, 2.0], size=K)
    amt[1] = np.round(rng.uniform(0.01, 2.0, size=K), 2) * 7864.32
    return host, kind, amt


def with_marks(np, host, kind, amt):
    """A mark after each op, as the reference's hosts check in after a dispatch and out after a
    completion; entry k at time k // 2."""
    K = len(host)
    h2 = np.repeat(host, 2)
    k2 = np.empty(2 * K, dtype=np.int32)
    k2[0::2], k2[1::2] = kind, 2 + kind
    a2 = np.zeros((4, 2 * K))
    a2[:, 0::2] = amt
    return h2, k2, a2, (np.arange(2 * K) // 2).astype(np.float64)


class ParentLibrary:
    """``host_ops_into`` on another build of the library (the parent's knows no metering, so it
    is bound by hand: context, stream, pvt_host_ops_apply)."""

    def __init__(self, path, torch, device):
        import ctypes
        from pivot_place import _abi
        self._abi, self._ct = _abi, ctypes
        self.lib = ctypes.CDLL(path)
        self.lib.pvt_ctx_create.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
        self.lib.pvt_ctx_set_stream.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        self.lib.pvt_host_ops_apply.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        self.ctx = ctypes.c_void_p()
        assert self.lib.pvt_ctx_create(device.index or 0, ctypes.byref(self.ctx)) == 0
        stream = torch.cuda.current_stream(device).cuda_stream
        assert self.lib.pvt_ctx_set_stream(self.ctx, ctypes.c_void_p(stream)) == 0

    def host_ops_into(self, capacity, level, op_host, op_kind, op_amt, op_ok):
        o = self._abi.pvt_host_ops()
        o.n_hosts, o.n_ops = level.numel() // 4, op_host.numel()
        o.capacity, o.level = capacity.data_ptr(), level.data_ptr()
        o.op_host, o.op_kind = op_host.data_ptr(), op_kind.data_ptr()
        o.op_amt, o.op_ok = op_amt.data_ptr(), op_ok.data_ptr()
        assert self.lib.pvt_host_ops_apply(self.ctx, self._ct.addressof(o)) == 0


def old_and_marks(engs, torch, np, H, K, warmup, calls):
    from pivot_place import hostops
    dev = engs["new"].device
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    cap = up(np.repeat(np.array(CAP)[:, None], H, axis=1).ravel())
    start = cap * 0.5
    host, kind, amt = make_ops(np, H, K, K)
    d_ops = (up(host), up(kind), up(amt.ravel()))
    h2, k2, a2, t2 = with_marks(np, host, kind, amt)
    d_marked = (up(h2), up(k2), up(a2.ravel()), up(t2))
    level = start.clone()
    ok = torch.empty(K, dtype=torch.int32, device=dev)
    ok2 = torch.empty(2 * K, dtype=torch.int32, device=dev)
    meter = hostops.DeviceMeter(torch, dev, H, 2 * K)
    times = {name: [] for name in list(engs) + ["marks"]}

    def marked():
        meter.st_word.zero_()
        meter.n_iv = meter.n_us = 0
        meter.last_time = 0.0
        level.copy_(start)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        engs["new"].host_meter_apply_into(meter, cap, level, *d_marked, ok2)
        return time.perf_counter() - t0

    for i in range(warmup + calls):
        for name, eng in engs.items():
            level.copy_(start)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            eng.host_ops_into(cap, level, *d_ops, ok)      # synchronises before it returns
            dt = time.perf_counter() - t0
            if i >= warmup:
                times[name].append(dt)
        dt = marked()
        if i >= warmup:
            times["marks"].append(dt)
    walk = {}
    for kname, fn in (("host_ops_kernel", lambda: engs["new"].host_ops_into(cap, level, *d_ops, ok)),
                      ("host_meter_kernel", marked)):
        engs["new"].set_profiling(2, kname)
        engs["new"].reset_kstats()
        for _ in range(calls):
            level.copy_(start)
            fn()
        k = engs["new"].kernel_kstats(kname)
        engs["new"].set_profiling(False)
        walk[kname + "_ms_mean"] = k["ms"] / max(k["launches"], 1)
    out = {"ops": K, "entries_with_marks": 2 * K, "usage_records": meter.n_us,
           "final_intervals": meter.n_iv}
    for name, ts in times.items():
        out[name] = stats(ts)
    out["marks_over_old"] = out["marks"]["median_ms"] / out["new"]["median_ms"]
    out.update(walk)
    return out


def finish(eng, torch, np, rows, records, s, warmup, calls):
    from pivot_place import hostops, meter as pm
    dev = eng.device
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    H = rows
    rng = np.random.RandomState(rows)
    per = np.minimum(2 * rng.poisson(records / (2.0 * rows), size=H), 24)    # even: none left open
    J = int(per.max())
    hosts, kinds, times = [], [], []
    for j in range(J):
        hs = np.flatnonzero(per > j).astype(np.int32)
        hosts.append(hs)
        kinds.append(np.full(len(hs), 2 + (j & 1), dtype=np.int32))
        times.append(130.0 * j + 129.0 * hs / H)
    host, kind, t = np.concatenate(hosts), np.concatenate(kinds), np.concatenate(times)
    K = len(host)
    cap = up(np.repeat(np.array(CAP)[:, None], H, axis=1).ravel())
    level = cap * 0.5
    m = hostops.DeviceMeter(torch, dev, H, K)
    eng.host_meter_apply(m, cap, level, up(host), up(kind), torch.zeros(4 * K, dtype=torch.float64,
                                                                        device=dev), up(t))
    fin = eng.host_meter_finish(m)
    f = {k: v.cpu().numpy() for k, v in fin.items()}
    R = len(f["row_host"])
    NB = int(m.last_time // s) + 1
    log = pm.UsageLog(s, np.array([0, R], dtype=np.int64), f["iv_off"], f["iv_start"], f["iv_end"],
                      f["us_off"], f["us_time"], f["us_frac"].reshape(4, -1),
                      np.array([0, NB], dtype=np.int64))
    t_dev, t_fin, t_up = [], [], []
    for i in range(warmup + calls):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fin = eng.host_meter_finish(m)
        t1 = time.perf_counter()
        a = eng.meter_usage_device(fin, s, m.last_time)
        t2 = time.perf_counter()
        b = eng.meter_usage(log)
        t3 = time.perf_counter()
        if i >= warmup:
            t_fin.append(t1 - t0)
            t_dev.append(t2 - t0)
            t_up.append(t3 - t2)
    same = all(a[k].tobytes() == b[k].tobytes() for k in ("n_hosts", "res_hosts", "res_mean", "avg"))
    return {"hosts": H, "rows": R, "usage_records": m.n_us, "intervals": len(f["iv_start"]),
            "logged_intervals": m.n_iv, "buckets": NB, "sample_size": s,
            "finish": stats(t_fin), "finish_plus_device_usage": stats(t_dev),
            "upload_usage": stats(t_up), "device_equals_upload": bool(same)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hosts", type=int, default=1000000)
    ap.add_argument("--ops", type=int, nargs="+", default=[1000, 20000, 200000])
    ap.add_argument("--rows", type=int, default=616318)
    ap.add_argument("--records", type=int, default=3690000)
    ap.add_argument("--sample-size", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libpivot_place.so")
    args = ap.parse_args()
    if args.warmup < 3 or args.calls < 20:
        ap.error("at least 3 warm-up calls and 20 timed calls")
    import numpy as np
    import torch
    from pivot_place.engine import PlacementEngine
    engs = {"new": PlacementEngine(0)}
    if args.parent_lib:
        engs = {"parent": ParentLibrary(args.parent_lib, torch, engs["new"].device), **engs}
    res = {"metric": "metered resident cluster (pvt_host_meter_apply / _finish)",
           "hosts": args.hosts, "warmup": args.warmup, "calls": args.calls,
           "logs": [old_and_marks(engs, torch, np, args.hosts, K, args.warmup, args.calls)
                    for K in args.ops],
           "finish": finish(engs["new"], torch, np, args.rows, args.records, args.sample_size,
                            args.warmup, args.calls)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
