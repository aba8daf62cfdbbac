"""GPU tests of the frontier walk's long runs ("Run lengths from the order
launch"): the rounds of long_run_cases.py, each checked for its shape on the CPU reference
(test_long_run_cases.py), equal the reference bit for bit on placement, order and availability on

  default   run lengths from the grouped-order launch, the log's ring, the fast prologue
  runrem0   an engine created under PVT_ZW_RUNREM=0 (the walk finds its runs itself, 64 at the most)
  cert0     an engine created under PVT_CHAIN_CERT=0 (the walk's own prologue, no run lengths)
  tail0     an engine created under PVT_EPOCH_TAIL=0 (the tail kernels rebuild the availability
            from the log alone, so a wrong or missing ring entry shows)

The default run must report fast-prologue chains: the instance that reads the run lengths ran."""
import pytest

import long_run_cases as lc

from test_gpu_epoch_tail import _engine_under, _same
from test_gpu_walk_pipe import _place

pytestmark = pytest.mark.gpu

PATHS = ("default", "runrem0", "cert0", "tail0")


@pytest.fixture(scope="module")
def engines(engine):
    made = {"runrem0": _engine_under(PVT_ZW_RUNREM="0"), "cert0": _engine_under(PVT_CHAIN_CERT="0"),
            "tail0": _engine_under(PVT_EPOCH_TAIL="0")}
    yield dict(made, default=engine)
    for eng in made.values():
        eng.close()


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", lc.NAMES)
def test_case(engines, name, path):
    r, e, ref = lc.reference(name)
    eng = engines[path]
    res, st, n = _place(eng, r)
    fast = eng.prologue_stats()["fast_chains"]
    print(name, path, "fast chains", fast)
    _same(res, ref)
    assert n["zwalk_kernel"] >= 1 and st["frontier_chains"] == 2 and st["list_chains"] == 0, (st, n)
    if path == "default":
        assert fast >= 1, fast
    if path == "cert0":
        assert fast == 0, fast
