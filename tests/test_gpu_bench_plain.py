"""A plain bench.py run (no --full): the headline line alone -- no parity, CPU baseline, roofline
or extra legs -- with --steps timed steps, and --dump-outputs writing the round the last timed
step placed: equal, value for value, to the CPU restatement's result on the same seeded round."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, T = 20000, 300


@pytest.mark.parametrize("mode", ["ca_bf", "opp"])
def test_plain_run_is_lean_and_dumps_the_placed_round(tmp_path, mode):
    sys.path.insert(0, ROOT)
    import bench
    from oracle import oracle
    from pivot_place import synthetic
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3",
           "--warmup", "1", "--hosts", str(H), "--tasks", str(T), "--mode", mode,
           "--dump-outputs", str(tmp_path / "out")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=110, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    res = json.loads(lines[0])
    assert res["metric"] == bench.METRIC and res["unit"] == "candidates/s"
    assert res["higher_is_better"] is True and res["dtype"] == "f64"
    assert res["steps"] == 3 and res["warmup"] == 1 and res["ms_per_step"] > 0
    assert res["value"] == pytest.approx(float(T) * H / (res["ms_per_step"] * 1e-3), rel=1e-9)
    for k in ("parity", "cpu_baseline", "extra", "roofline", "kernel_ms_per_step", "full_results"):
        assert k not in res, k
    assert "parity against the oracle" not in out.stderr and "cpu baseline" not in out.stderr
    ref = oracle.place(synthetic.make_round(bench.MODES[mode], H, T, seed=bench.DEFAULT_SEED))
    names = ["placement", "order", "avail"] + (["mt_state"] if ref.mt_state is not None else [])
    assert sorted(os.listdir(tmp_path / "out")) == sorted(n + ".npy" for n in names)
    for n in names:
        got = np.load(tmp_path / "out" / (n + ".npy"))
        want = np.asarray(getattr(ref, n), dtype=np.float64).ravel()
        assert got.dtype == np.float64 and np.array_equal(got, want), n
    assert res["outputs"] == {n: int(np.asarray(getattr(ref, n)).size) for n in names}
