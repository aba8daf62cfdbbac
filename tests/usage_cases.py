"""Shared cases of the meter usage series tests (test_meter_usage.py, test_gpu_meter_usage.py).

``host_series`` / ``resource_series`` compute what the reference's plot_host_usage and
plot_resource_usage (resources/meter.py:135-159) compute, in plain Python and in this project's
own terms (dicts keyed by bucket index), over a scenario dict as
``pivot_place.meter.pack_usage`` takes it; they are the CPU checker of the GPU series. The
fixture tests/golden/meter_usage.json.gz (make_meter_usage.py) holds three reference runs with
the reference meter's own series, which pins the checker to the reference.
"""
import gzip
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RESOURCES = ("cpus", "mem", "disk", "gpus")
SAMPLE_SIZES = (100, 7, 1000)
RTOL = 1e-9     # BASELINE.json north star, as RTOL in tests/test_meter.py

_FIXTURE = []


def fixture():
    """(runs, scenarios) of the fixture, loaded once and never modified."""
    if not _FIXTURE:
        with gzip.open(os.path.join(GOLDEN, "meter_usage.json.gz"), "rt") as f:
            runs = json.load(f)
        scen = [{"hosts": [h["intervals"] for h in r["hosts"]], "routes": [],
                 "usage": [(h["times"], tuple(h["usage"])) for h in r["hosts"]]} for r in runs]
        _FIXTURE.append((runs, scen))
    return _FIXTURE[0]


def mean(vals):
    return sum(vals) / len(vals) if len(vals) else float("nan")


def host_series(sc, s):
    """Hosts in use per bucket: an interval [start, end] puts its host into the buckets
    start // s .. end // s - 1 (the bucket that holds `end` is left out; the fixture pins this
    to the reference). x: the non-empty buckets as (b * s, (b + 1) * s), y: distinct hosts."""
    in_use = {}
    for h, intervals in enumerate(sc["hosts"]):
        for start, end in intervals:
            for b in range(int(start // s), int(end // s)):
                in_use.setdefault(b, set()).add(h)
    buckets = sorted(in_use)
    return [(b * s, (b + 1) * s) for b in buckets], [len(in_use[b]) for b in buckets]


def resource_series(sc, resource, s):
    """Mean utilisation per bucket: a record falls in bucket t // s; y is the mean over the hosts
    with a record there of each host's own mean. x: the bucket starts b * s."""
    r = RESOURCES.index(resource)
    per_bucket = {}
    for h, (times, vals) in enumerate(sc.get("usage") or []):
        for t, v in zip(times, vals[r]):
            per_bucket.setdefault(int(t // s), {}).setdefault(h, []).append(v)
    buckets = sorted(per_bucket)
    return ([b * s for b in buckets],
            [mean([mean(v) for v in per_bucket[b].values()]) for b in buckets])


def series(sc, sample_size):
    """All series of a scenario in the shape of ``pivot_place.meter.usage_series``."""
    out = {"hosts": host_series(sc, sample_size)}
    for r in RESOURCES:
        out[r] = resource_series(sc, r, sample_size)
    out["avg"] = [mean(out["hosts"][1])] + [mean(out[r][1]) for r in RESOURCES]
    return out


def check_series(got, want, with_usage=True):
    """``got`` (usage_series of a GPU result, or the helper) against ``want`` (the helper, or a
    fixture entry): host series and its average exactly, resource x exactly, means at RTOL."""
    gx, gy = got["hosts"]
    wx, wy = want["hosts"]
    assert [tuple(k) for k in gx] == [tuple(k) for k in wx]
    assert list(gy) == list(wy)
    np.testing.assert_array_equal(got["avg"][0], want["avg"][0])
    if not with_usage:
        return
    for k, r in enumerate(RESOURCES):
        assert list(got[r][0]) == list(want[r][0]), r
        np.testing.assert_allclose(np.array(got[r][1], dtype=np.float64),
                                   np.array(want[r][1], dtype=np.float64), rtol=RTOL, atol=0)
        np.testing.assert_allclose(got["avg"][1 + k], want["avg"][1 + k], rtol=RTOL, atol=0)


def synthetic(n_scen, seed, sample_size, max_hosts=300):
    """Seeded scenarios: 0..max_hosts hosts, 0-5 ordered intervals and 0-12 time-ordered records
    per host; gaps of up to three buckets, integral and fractional times, some gaps zero."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_scen):
        H = int(rng.integers(0, max_hosts + 1))
        frac = bool(rng.integers(0, 2))
        t = np.cumsum(rng.integers(0, 3 * sample_size + 1, size=(H, 10)), axis=1)
        ut = np.cumsum(rng.integers(0, sample_size + 1, size=(H, 12)), axis=1)
        t, ut = t.astype(np.float64), ut.astype(np.float64)
        if frac:
            t = np.sort(t + rng.integers(0, 4, size=t.shape) * 0.25, axis=1)
            ut = np.sort(ut + rng.integers(0, 4, size=ut.shape) * 0.25, axis=1)
        n_iv, n_us = rng.integers(0, 6, size=H).tolist(), rng.integers(0, 13, size=H).tolist()
        t, ut, vals = t.reshape(H, 5, 2).tolist(), ut.tolist(), rng.random((H, 4, 12)).tolist()
        hosts = [t[h][:n_iv[h]] for h in range(H)]
        usage = [(ut[h][:n_us[h]], tuple(v[:n_us[h]] for v in vals[h])) for h in range(H)]
        out.append({"hosts": hosts, "routes": [], "usage": usage})
    return out


def records(times):
    n = len(times)
    return (list(times), tuple([((7 * i + 3 * r) % 11) / 10.0 for i in range(n)] for r in range(4)))


def edge_cases(s=100):
    """One batch of the corner cases, times scaled by s / 100 (s = 100: the values named in the
    comments). Every scenario lists usage records, some of them none."""
    k = s / 100.0 if s % 100 else s // 100
    T = lambda *ts: [t * k for t in ts]
    span = lambda nb: [[T(0, (nb - 1) * 100 + 5)], [T(25500, 25700)] if nb > 257 else [],
                       [T((nb - 2) * 100, (nb - 1) * 100)]]
    cases = [
        ("no hosts", [], []),
        ("host without intervals", [[]], [records([])]),
        ("inside one bucket", [[T(10, 50)]], [records(T(10, 50))]),
        ("[0,100]", [[T(0, 100)]], [records(T(0, 100))]),
        ("[100,100]", [[T(100, 100)]], [records(T(100, 100))]),
        ("[0,150],[150,420]", [[T(0, 150), T(150, 420)]], [records(T(0, 150, 150, 420))]),
        ("multiples as ints", [[[200 * k, 400 * k]], [[0, 300 * k]]],
         [records([200 * k, 400 * k]), records([0, 300 * k])]),
        ("multiples as floats", [[[float(200 * k), float(400 * k)]], [[0.0, float(300 * k)]]],
         [records([float(200 * k), float(400 * k)]), records([0.0, float(300 * k)])]),
        ("records without intervals", [[], []], [records(T(5, 105, 110, 350)), records(T(100))]),
    ]
    for nb in (255, 256, 257, 513):
        hosts = span(nb)
        cases.append(("nb %d" % nb, hosts,
                      [records([v for iv in h for v in iv]) for h in hosts]))
    for n in (257, 300):
        hosts = [[T(100 * (i % 7), 100 * (i % 7) + 60 * (i % 5) + 30)] for i in range(n)]
        cases.append(("%d host rows" % n, hosts,
                      [records(T(100 * (i % 7), 100 * (i % 7) + 20, 100 * (i % 7) + 60 * (i % 5) + 30))
                       for i in range(n)]))
    return ([c[0] for c in cases],
            [{"hosts": c[1], "routes": [], "usage": c[2]} for c in cases])
