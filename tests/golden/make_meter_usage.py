#!/usr/bin/env python3
"""Usage series of REFERENCE simulations (test-only; the second half of resources/meter.py).

Runs the three reference simulations of make_meter_logs.py (its ``RUNS``) and writes, per run:

* ``hosts``: the meter's ``__hosts`` dict in its order — per host its [check-in, check-out]
  intervals, the timestamps of its usage records (``__usage``, one record per resource at every
  host_check_in / host_check_out, :181-187; the four resources share the timestamps, stored
  once) and the four value lists in the order cpus, mem, disk, gpus;
* ``want``: per sample size in ``SAMPLE_SIZES`` the reference meter's own ``plot_host_usage``
  (:135-148), ``plot_resource_usage`` of each resource (:150-159) and the five
  ``get_avg_*_usage`` (:161-179), as the reference computes them.

Output: tests/golden/meter_usage.json.gz. Only the fixture travels.
"""
import gzip
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
RESOURCES = ("cpus", "mem", "disk", "gpus")
SAMPLE_SIZES = (100, 7, 1000)


def main():
    if os.environ.get("PYTHONHASHSEED") != "0":
        env = dict(os.environ, PYTHONHASHSEED="0")
        sys.exit(subprocess.call([sys.executable] + sys.argv, env=env))
    sys.path.insert(0, HERE)
    from make_meter_logs import RUNS
    import make_golden_sim as mgs
    from pivot_place import des
    des.install(force=True)
    import make_golden as mg
    mg._install_compat()
    import logging
    logging.disable(logging.CRITICAL)
    world = mg.World()
    out = []
    for label, policy, kwargs, n_hosts, n_apps, job in RUNS:
        got = []
        mgs.simulate(mg, world, label, policy, kwargs, n_hosts, n_apps, job, meter_out=got)
        meter, cluster = got[0]
        hidx = {id(h): i for i, h in enumerate(cluster.hosts)}
        usage = meter._Meter__usage
        order = list(meter._Meter__hosts)
        hosts = []
        for r in RESOURCES:
            assert list(usage[r]) == order, (label, r)
        for h, vals in meter._Meter__hosts.items():
            times = [t for t, _ in usage["cpus"][h]]
            for r in RESOURCES:
                assert [t for t, _ in usage[r][h]] == times, (label, r)
            hosts.append({"host": hidx[id(h)], "intervals": [list(v) for v in vals],
                          "times": times,
                          "usage": [[v for _, v in usage[r][h]] for r in RESOURCES]})
        want = {}
        for s in SAMPLE_SIZES:
            x, y = meter.plot_host_usage(sample_size=s)
            w = {"hosts": [[list(k) for k in x], y]}
            for r in RESOURCES:
                x, y = meter.plot_resource_usage(r, sample_size=s)
                w[r] = [list(x), [float(v) for v in y]]
            w["avg"] = [float(meter.get_avg_host_usage(sample_size=s)),
                        float(meter.get_avg_cpu_usage(sample_size=s)),
                        float(meter.get_avg_mem_usage(sample_size=s)),
                        float(meter.get_avg_disk_usage(sample_size=s)),
                        float(meter.get_avg_gpus_usage(sample_size=s))]
            want[str(s)] = w
        out.append({"name": label, "hosts": hosts, "want": want})
        print(label, len(hosts), sum(len(h["times"]) for h in hosts),
              {s: (len(w["hosts"][1]), w["avg"]) for s, w in want.items()})
    path = os.path.join(HERE, "meter_usage.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as g:
        g.write(json.dumps(out, separators=(",", ":")).encode())
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
