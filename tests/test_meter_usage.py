"""Meter usage series, CPU side (reference resources/meter.py:135-179).

tests/golden/make_meter_usage.py ran the three reference simulations of make_meter_logs.py and
recorded the host intervals, the usage records and the reference meter's own series at sample
sizes 100, 7 and 1000. The plain-Python checker of the two series
(tests/usage_cases.py), which checks the GPU series in test_gpu_meter_usage.py, reproduces them
here: host series and host average exactly, resource means within 1e-9 relative (numpy sums
pairwise, the checker left to right; every term is a non-negative fraction).
"""
import gzip
import json
import math
import os
import re

import numpy as np
import pytest

import usage_cases as uc
from pivot_place import _abi, meter

HEADER = os.path.join(os.path.dirname(uc.GOLDEN), "..", "include", "pivot_place.h")


@pytest.mark.parametrize("s", uc.SAMPLE_SIZES)
def test_helper_reproduces_reference_series(s):
    runs, scen = uc.fixture()
    for r, sc in zip(runs, scen):
        want = r["want"][str(s)]
        assert len(want["hosts"][1]) > 0 and len(want["cpus"][1]) > 0
        uc.check_series(uc.series(sc, s), want)


def test_helper_quirks():
    """The bucket that holds `end` is not counted; an interval inside one bucket counts nowhere."""
    hs = lambda ivs, s=100: uc.host_series({"hosts": [ivs]}, s)
    assert hs([[0, 100]]) == ([(0, 100)], [1])
    assert hs([[100, 100]]) == ([], [])
    assert hs([[10, 50]]) == ([], [])
    assert hs([[0, 150], [150, 420]]) == ([(0, 100), (100, 200), (200, 300), (300, 400)],
                                          [1, 1, 1, 1])
    sc = {"hosts": [[[0, 250]], [[120, 130], [199, 200]]],
          "usage": [([0, 250], ([0.5, 1.0], [0, 0], [0, 0], [0, 0])),
                    ([120, 130, 199, 200], ([0.25, 0.75, 0.5, 0.125], [0] * 4, [0] * 4, [0] * 4))]}
    assert uc.host_series(sc, 100) == ([(0, 100), (100, 200)], [1, 2])
    assert uc.resource_series(sc, "cpus", 100) == ([0, 100, 200], [0.5, 0.5, (1.0 + 0.125) / 2])
    assert math.isnan(uc.series({"hosts": []}, 100)["avg"][0])


def test_fixture_intervals_equal_the_meter_logs():
    runs, _ = uc.fixture()
    with gzip.open(os.path.join(uc.GOLDEN, "meter_logs.json.gz"), "rt") as f:
        logs = json.load(f)
    assert [r["name"] for r in runs] == [r["name"] for r in logs]
    for r, l in zip(runs, logs):
        assert [(h["host"], h["intervals"]) for h in r["hosts"]] == \
               [(h["host"], h["intervals"]) for h in l["hosts"]]
        for h in r["hosts"]:
            assert all(len(v) == len(h["times"]) for v in h["usage"]) and len(h["usage"]) == 4


def test_pack_usage_layout():
    log = meter.pack_usage([
        {"hosts": [[[0, 150], [150, 420]], []],
         "usage": [([0, 150, 150, 420], ([.1, .2, .3, .4], [.5] * 4, [0] * 4, [1] * 4)),
                   ([777.5], ([.9], [.8], [.7], [.6]))]},
        {"hosts": [], "routes": []}], 100)
    assert log.sample_size == 100 and log.n_scen == 2
    assert log.host_off.tolist() == [0, 2, 2] and log.iv_off.tolist() == [0, 2, 2]
    assert log.iv_start.tolist() == [0, 150] and log.iv_end.tolist() == [150, 420]
    assert log.us_off.tolist() == [0, 4, 5]
    assert log.us_time.tolist() == [0, 150, 150, 420, 777.5]
    assert log.us_frac.shape == (4, 5)
    assert log.us_frac[0].tolist() == [.1, .2, .3, .4, .9]
    assert log.us_frac[3].tolist() == [1, 1, 1, 1, .6]
    assert log.bucket_off.tolist() == [0, 8, 8]          # 777.5 // 100 + 1, then no data
    for name, a in log.arrays():
        assert a.dtype == (np.float64 if name in ("iv_start", "iv_end", "us_time", "us_frac")
                           else np.int64), name
    m = log.fill(lambda a: a.ctypes.data, [1, 2, 3, 4])
    assert (m.n_scen, m.reserved, m.sample_size, m.n_host_rows, m.n_iv, m.n_us, m.n_buckets) == \
           (2, 0, 100, 2, 2, 5, 8)
    assert m.us_frac == log.us_frac.ctypes.data and m.avg == 4
    # without any usage entry there is no resource series: the three arrays are absent
    bare = meter.pack_usage([{"hosts": [[[0, 100]]]}], 7)
    assert bare.us_off is None and bare.us_time is None and bare.us_frac is None
    assert bare.bucket_off.tolist() == [0, 15]
    m = bare.fill(lambda a: a.ctypes.data, [1, 2, 3, 4])
    assert m.n_us == 0 and m.us_off is None and m.us_time is None and m.us_frac is None
    for bad in (0, -3, 2.5, 2 ** 31, None, "100"):
        with pytest.raises(ValueError):
            meter.pack_usage([], bad)
    assert meter.pack_usage([], 100.0).sample_size == 100


def test_usage_of_reads_a_meters_private_dicts():
    """A Meter-shaped object with the reference's ``__hosts`` / ``__usage`` dicts packs to the
    same arrays as the fixture scenario it was built from."""
    import collections
    runs, scen = uc.fixture()
    run, sc = runs[2], scen[2]

    class Fake:
        pass

    m = Fake()
    keys = [object() for _ in run["hosts"]]
    m._Meter__hosts = collections.defaultdict(list)
    m._Meter__usage = collections.defaultdict(dict)
    for k, h in zip(keys, run["hosts"]):
        m._Meter__hosts[k] = [list(v) for v in h["intervals"]]
        for r, name in enumerate(uc.RESOURCES):
            m._Meter__usage[name][k] = list(zip(h["times"], h["usage"][r]))
    a, b = meter.pack_usage([meter.usage_of(m)], 100), meter.pack_usage([sc], 100)
    for (name, x), (_, y) in zip(a.arrays(), b.arrays()):
        assert x.tobytes() == y.tobytes(), name
    m._Meter__usage = collections.defaultdict(dict)
    bare = meter.usage_of(m)
    assert bare["usage"] is None and bare["hosts"] == sc["hosts"]
    assert meter.pack_usage([bare], 100).us_off is None


def test_usage_series_drops_empty_buckets():
    out = {"bucket_off": np.array([0, 3, 3, 5]), "n_hosts": np.array([2, 0, 1, 0, 4], np.int32),
           "res_hosts": np.array([0, 1, 1, 0, 0], np.int32),
           "res_mean": np.arange(20, dtype=np.float64).reshape(4, 5),
           "avg": np.arange(15, dtype=np.float64).reshape(3, 5)}
    a, b, c = meter.usage_series(out, 7)
    assert a["hosts"] == ([(0, 7), (14, 21)], [2, 1])
    assert a["cpus"] == ([7, 14], [1.0, 2.0]) and a["gpus"] == ([7, 14], [16.0, 17.0])
    assert b["hosts"] == ([], []) and b["mem"] == ([], [])
    assert c["hosts"] == ([(7, 14)], [4]) and c["disk"] == ([], [])
    assert c["avg"].tolist() == [10, 11, 12, 13, 14]


def test_usage_struct_layout_matches_header():
    text = open(HEADER).read()
    body = re.search(r"typedef struct pvt_usage_log \{(.*?)\} pvt_usage_log;", text,
                     flags=re.S).group(1)
    fields = re.findall(r"\b(\w+)\s*(?:,|;)", body)
    assert [f for f, _ in _abi.pvt_usage_log._fields_] == fields
    import ctypes
    assert ctypes.sizeof(_abi.pvt_usage_log) == 2 * 4 + 5 * 8 + 12 * 8


def test_header_declares_pvt_meter_usage():
    text = open(HEADER).read()
    assert re.search(r"^int\s+pvt_meter_usage\(pvt_ctx\* ctx, const pvt_usage_log\* u\);", text,
                     flags=re.M)
    assert int(re.search(r"#define\s+PVT_ABI_VERSION\s+(\d+)", text).group(1)) == 3
    from pivot_place import engine
    assert hasattr(engine.load_library(), "pvt_meter_usage")
