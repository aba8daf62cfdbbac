"""Time of the meter usage series (pvt_meter_usage; reference resources/meter.py:135-179).

Two workloads, both from data in the tree only:
  synthetic   --scen seeded scenarios of tests/usage_cases.py (0-300 hosts, 0-5 intervals and
              0-12 usage records per host) as one batch at --sample-size;
  reference   the three recorded reference runs of tests/golden/meter_usage.json.gz (12-72 hosts,
              15 268 records each) as one batch at --sample-size.
For each: the median over --calls calls (after --warmup) of ``PlacementEngine.meter_usage`` on
the packed log -- a host clock around the whole call, which stages the arrays, launches once,
synchronises and copies the series back -- then, in a pass of its own with the engine's HIP
events on, the mean time of the launch alone; and beside them the plain-Python checker of
the series (tests/usage_cases.py) on the same scenarios, one core. Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pivot-scheduling_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def measure(eng, torch, scen, s, warmup, calls):
    import usage_cases as uc
    from pivot_place import _abi, meter
    log = meter.pack_usage(scen, s)
    for _ in range(warmup):
        out = eng.meter_usage(log)
    torch.cuda.synchronize()
    times = []
    for _ in range(calls):
        t0 = time.perf_counter()
        out = eng.meter_usage(log)          # synchronises before it returns
        times.append(time.perf_counter() - t0)
    eng.set_profiling(True)
    eng.reset_kstats()
    for _ in range(calls):
        eng.meter_usage(log)
    k = eng.kstats(_abi.PVT_K_OTHER)
    eng.set_profiling(False)
    t0 = time.perf_counter()
    want = [uc.series(sc, s) for sc in scen]
    cpu_s = time.perf_counter() - t0
    for g, w in zip(meter.usage_series(out, s), want):
        uc.check_series(g, w)
    return {"scenarios": len(scen), "host_rows": len(log.iv_off) - 1, "intervals": len(log.iv_start),
            "records": len(log.us_time), "buckets": int(log.bucket_off[-1]),
            "call_ms_median": statistics.median(times) * 1e3,
            "call_ms_min": min(times) * 1e3, "call_ms_max": max(times) * 1e3,
            "kernel_ms_mean": k["ms"] / max(k["launches"], 1), "kernel_launches": k["launches"],
            "python_helper_ms": cpu_s * 1e3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scen", type=int, default=4096)
    ap.add_argument("--sample-size", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    if args.warmup < 3 or args.calls < 20:
        ap.error("at least 3 warm-up calls and 20 timed calls")
    import torch
    import usage_cases as uc
    from pivot_place.engine import PlacementEngine
    eng = PlacementEngine(0)
    s = args.sample_size
    res = {"metric": "meter usage series (pvt_meter_usage)", "sample_size": s,
           "warmup": args.warmup, "calls": args.calls,
           "synthetic": measure(eng, torch, uc.synthetic(args.scen, 0, s), s, args.warmup,
                                args.calls),
           "reference_runs": measure(eng, torch, uc.fixture()[1], s, args.warmup, args.calls),
           "note": "call_ms: host clock around engine.meter_usage (staging, one launch, "
                   "synchronise, copy back); kernel_ms: HIP events around the launch, separate "
                   "pass; python_helper_ms: the same series in plain Python, one core"}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
