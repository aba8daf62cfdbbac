"""Meter usage series on the GPU (pvt_meter_usage; reference resources/meter.py:135-179).

The GPU series against the reference meter's own values recorded in
tests/golden/meter_usage.json.gz, and against the plain-Python checker of the two series
(tests/usage_cases.py) on corner cases and seeded batches. Host counts, bucket positions and the
host average must be equal; the resource means are within 1e-9 relative (the project's bound,
RTOL of tests/test_meter.py: the kernel sums a host's run in record order, hosts in a shuffle
tree and buckets per wave, numpy sums pairwise; every term is a non-negative fraction).
"""
import numpy as np
import pytest

import usage_cases as uc
from pivot_place import meter

pytestmark = pytest.mark.gpu


def _run(engine, scen, s):
    return meter.usage_series(engine.meter_usage(meter.pack_usage(scen, s)), s)


@pytest.mark.parametrize("s", uc.SAMPLE_SIZES)
def test_gpu_usage_reference_runs(engine, s):
    runs, scen = uc.fixture()
    got = _run(engine, scen, s)
    for r, g in zip(runs, got):
        uc.check_series(g, r["want"][str(s)])


@pytest.mark.parametrize("s", [100, 1])
def test_gpu_usage_edge_cases(engine, s):
    names, scen = uc.edge_cases(s)
    got = _run(engine, scen, s)
    for name, sc, g in zip(names, scen, got):
        try:
            uc.check_series(g, uc.series(sc, s))
        except AssertionError as e:
            raise AssertionError("%s (s = %d): %s" % (name, s, e))
    by = dict(zip(names, got))
    assert by["no hosts"]["hosts"] == ([], []) and np.isnan(by["no hosts"]["avg"]).all()
    assert by["inside one bucket"]["hosts"] == ([], [])
    assert by["[0,100]"]["hosts"] == ([(0, s)], [1])
    assert by["[100,100]"]["hosts"] == ([], [])
    assert by["[0,150],[150,420]"]["hosts"] == ([(b * s, (b + 1) * s) for b in range(4)], [1] * 4)
    assert by["multiples as ints"]["hosts"] == by["multiples as floats"]["hosts"] == \
           ([(0, s), (s, 2 * s), (2 * s, 3 * s), (3 * s, 4 * s)], [1, 1, 2, 1])
    assert by["records without intervals"]["hosts"] == ([], [])
    assert by["records without intervals"]["cpus"][0] == [0, s, 3 * s]
    for nb in (255, 256, 257, 513):
        x, y = by["nb %d" % nb]["hosts"]
        assert len(y) == nb - 1 and y[-1] == 2 and x[-1] == ((nb - 2) * s, (nb - 1) * s)


@pytest.mark.parametrize("n_scen,seed,s", [(1, 0, 100), (1, 1, 1), (7, 2, 7), (7, 3, 1),
                                           (7, 4, 100), (512, 5, 7)])
def test_gpu_usage_batches(engine, n_scen, seed, s):
    scen = uc.synthetic(n_scen, seed, s)
    out = engine.meter_usage(meter.pack_usage(scen, s))
    assert out["n_hosts"].dtype == np.int32 and out["res_hosts"].dtype == np.int32
    assert out["res_mean"].shape == (4, out["bucket_off"][-1]) and out["avg"].shape == (n_scen, 5)
    assert (out["n_hosts"] >= 0).all() and (out["res_mean"][:, out["res_hosts"] == 0] == 0).all()
    for sc, g in zip(scen, meter.usage_series(out, s)):
        uc.check_series(g, uc.series(sc, s))


def test_gpu_usage_is_deterministic(engine):
    scen = uc.synthetic(7, 11, 7)
    log = meter.pack_usage(scen, 7)
    a, b = engine.meter_usage(log), engine.meter_usage(log)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    off = a["bucket_off"]
    for i, sc in enumerate(scen):
        one = engine.meter_usage(meter.pack_usage([sc], 7))
        lo, hi = off[i], off[i + 1]
        assert one["bucket_off"].tolist() == [0, hi - lo]
        assert one["n_hosts"].tobytes() == a["n_hosts"][lo:hi].tobytes()
        assert one["res_hosts"].tobytes() == a["res_hosts"][lo:hi].tobytes()
        assert one["res_mean"].tobytes() == np.ascontiguousarray(a["res_mean"][:, lo:hi]).tobytes()
        assert one["avg"].tobytes() == a["avg"][i:i + 1].tobytes()


def _valid_log():
    scen = [{"hosts": [[[0, 150], [150, 420]], [[30, 900.5]]],
             "usage": [uc.records([0, 150, 150, 420]), uc.records([30, 900.5])]},
            {"hosts": [[[5, 250]]], "usage": [uc.records([5, 250])]}]
    return meter.pack_usage(scen, 100)


def _set(name, index, value):
    def change(log):
        a = getattr(log, name).copy()
        a[index] = value
        setattr(log, name, a)
    return change


VIOLATIONS = {
    "bad offset": _set("iv_off", 1, 10 ** 9),
    "end < start": _set("iv_start", 2, 1000.0),
    "overlapping intervals": _set("iv_start", 1, 149.0),
    "negative time": _set("iv_start", 0, -1.0),
    "NaN time": _set("iv_end", 3, float("nan")),
    "time 2^52": _set("iv_end", 3, 2.0 ** 52),
    "bucket_off one short": _set("bucket_off", slice(1, None), np.array([9, 12])),
    "sample_size 0": lambda log: setattr(log, "sample_size", 0),
    "decreasing us_time": _set("us_time", 3, 100.0),
}


@pytest.mark.parametrize("what", list(VIOLATIONS))
def test_gpu_usage_contract_violation(engine, what):
    log = _valid_log()
    assert log.bucket_off.tolist() == [0, 10, 13]
    engine.meter_usage(log)                      # the log is valid before the change
    VIOLATIONS[what](log)
    with pytest.raises(RuntimeError, match="EINVAL"):
        engine.meter_usage(log)


class _Base:
    """What stands behind the mixin (the reference Meter's place): it records that it was
    reached."""

    def plot_host_usage(self, sample_size=100):
        return ("base plot_host_usage", sample_size)

    def plot_resource_usage(self, resource, sample_size=100):
        return ("base plot_resource_usage", resource, sample_size)

    def get_avg_host_usage(self, sample_size=100):
        return ("base get_avg_host_usage", sample_size)

    def get_avg_gpus_usage(self, sample_size=100):
        return ("base get_avg_gpus_usage", sample_size)


class FakeMeter(meter.MeterUsageMixin, _Base):
    def __init__(self, engine, run, with_usage=True):
        self.engine = engine
        keys = [("h", i) for i in range(len(run["hosts"]))]
        self._Meter__hosts = {k: [list(v) for v in h["intervals"]]
                              for k, h in zip(keys, run["hosts"])}
        self._Meter__usage = {}
        if with_usage:
            for r, name in enumerate(uc.RESOURCES):
                self._Meter__usage[name] = {k: list(zip(h["times"], h["usage"][r]))
                                            for k, h in zip(keys, run["hosts"])}


def test_gpu_usage_dropin_mixin(engine):
    runs, _ = uc.fixture()
    avg_names = ("host", "cpu", "mem", "disk", "gpus")
    for run in runs:
        m = FakeMeter(engine, run)
        for s in (100, 1000):
            want = run["want"][str(s)]
            got = {"hosts": m.plot_host_usage(sample_size=s),
                   "avg": [getattr(m, "get_avg_%s_usage" % n)(sample_size=s) for n in avg_names]}
            for r in uc.RESOURCES:
                got[r] = m.plot_resource_usage(r, sample_size=s)
            uc.check_series(got, want)
            x, y = got["hosts"]
            assert isinstance(x, list) and isinstance(x[0], tuple) and type(y[0]) is int
            assert isinstance(got["cpus"][0], list) and isinstance(got["cpus"][1], list)
        assert m.plot_host_usage() == m.plot_host_usage(sample_size=100)     # the default
        assert m.plot_resource_usage("no such resource") == ([], [])
    run = runs[1]
    bare = FakeMeter(engine, run, with_usage=False)
    want = run["want"]["100"]
    x, y = bare.plot_host_usage()
    assert [tuple(k) for k in want["hosts"][0]] == x and want["hosts"][1] == y
    assert bare.get_avg_host_usage() == want["avg"][0]
    assert bare.plot_resource_usage("cpus") == ([], []) and np.isnan(bare.get_avg_cpu_usage())
    m = FakeMeter(engine, run)
    # x is b * sample_size with the caller's own sample_size: a float size gives float bounds
    xf, yf = m.plot_host_usage(sample_size=100.0)
    assert (xf, yf) == m.plot_host_usage(sample_size=100) and type(xf[0][0]) is float
    assert type(m.plot_host_usage(sample_size=100)[0][0][0]) is int
    assert type(m.plot_resource_usage("cpus", sample_size=100.0)[0][0]) is float
    assert m.plot_host_usage(sample_size=2.5) ==("base plot_host_usage", 2.5)
    assert m.plot_resource_usage("mem", sample_size=2.5) == ("base plot_resource_usage", "mem", 2.5)
    assert m.get_avg_host_usage(sample_size=2.5) == ("base get_avg_host_usage", 2.5)
    assert m.get_avg_gpus_usage(sample_size=2.5) == ("base get_avg_gpus_usage", 2.5)
