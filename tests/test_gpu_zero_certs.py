"""GPU tests of the zero-score certificates ("Certificate thresholds"): the rounds
of cert_cases.py, in each of which one clause alone decides a placement on the CPU reference
(test_cert_cases.py), on every engine path. Placement, order and final availability equal the
reference bit for bit on

  frontier        the windowed engine, frontier walk with the fast prologue
  frontier_cert0  an engine created under PVT_CHAIN_CERT=0 (the walk's own prologue)
  frontier_tail0  an engine created under PVT_EPOCH_TAIL=0 (the tail kernels decide every epoch)
  lists           set_zero_walk(False): list chains, validation and finality
  sequential      set_epochs(False): the sequential list walk
  resident        all cases of a mode in one place_batch call

and on the three frontier paths the epoch statistics, fast-prologue chains and launches of the
named kernels say which code decided.

What "left to the exact path" can assert at this size. The cases put group B (one chain) before
group A (the other). Where only A's chain fails a certificate, the epoch accepts B's segment, and
the next epoch holds A's group alone: a single chain takes the plain list walk, which
``list_chains`` does not count. ``list_chains >= 1`` holds only where the failing clause is one
both chains read (the separation and the first-fit capacity bound are taken over all hosts). So
for every case whose chain must be left, the tests assert what the driver guarantees in both
situations: the frontier walk did not prove both chains (``frontier_chains < 2``) and a further
epoch ran (``epochs >= 2``). In first-fit rounds the groups a chain walk refuses go to the keyed
path, whose own per-group walks count as frontier chains too; there the tests assert that the
chain walk rejected a group (``rejected >= 1``) and that further walks were launched.

The in-window cases: with groups anchored in zones 3 and 0 only, the chain's zone set is
anchor 0's own zero-cost zones, so a host of zone 2 is never a window host; the _walked variants
add a group anchored in zone 1 to A's chain, which puts zone 2 in the window, and keep a
separating dimension. They are the ones in which the walk itself scores host 2 exactly."""
import dataclasses

import numpy as np
import pytest

import cert_cases as cc
from pivot_place import _abi

from test_gpu_epoch_tail import TAIL, UNDO, _engine_under, _same as _same_numbers

pytestmark = pytest.mark.gpu

KERNELS = TAIL + (UNDO, "zwalk_kernel")
FRONTIER = ("frontier", "frontier_cert0", "frontier_tail0")


@pytest.fixture(scope="module")
def engine_cert0():
    eng = _engine_under(PVT_CHAIN_CERT="0")
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def engine_tail0():
    eng = _engine_under(PVT_EPOCH_TAIL="0")
    yield eng
    eng.close()


@pytest.fixture
def engines(engine, engine_cert0, engine_tail0):
    return {"frontier": engine, "frontier_cert0": engine_cert0, "frontier_tail0": engine_tail0,
            "lists": engine, "sequential": engine}


def _same(res, ref):
    """test_gpu_epoch_tail._same; a NaN capacity (window_cap_nan) must be a NaN in the same place."""
    nan = np.isnan(ref.avail)
    if nan.any():
        np.testing.assert_array_equal(np.isnan(res.avail), nan)
        res = dataclasses.replace(res, avail=np.where(nan, 0.0, res.avail))
        ref = dataclasses.replace(ref, avail=np.where(nan, 0.0, ref.avail))
    _same_numbers(res, ref)


def _place(eng, path, r):
    """The round on the windowed engine: result, epoch statistics, launches per named kernel,
    fast-prologue chains."""
    try:
        eng.set_resident(0)
        if path == "lists":
            eng.set_zero_walk(False)
        if path == "sequential":
            eng.set_epochs(False)
        eng.set_profiling(2)
        eng.reset_kstats()
        res = eng.place(r)
        st = eng.epoch_stats()
        fast = eng.prologue_stats()["fast_chains"]
        n = {k: eng.kernel_kstats(k)["launches"] for k in KERNELS}
    finally:
        eng.set_profiling(False)
        eng.set_zero_walk(True)
        eng.set_epochs(True)
        eng.set_resident(_abi.PVT_RESIDENT_MAX_HOSTS)
    print(path, st, n, fast)
    return res, st, n, fast


def _check_stats(name, path, e, st, n, fast):
    ff = e.mode == cc.FF
    tail_ran = n["epoch_final_kernel"] >= 1 and n["epoch_accept_apply_kernel"] >= 1
    if e.walk in ("left", "left_all"):
        # (the module docstring: why list_chains >= 1 only where both chains read the clause)
        assert n["zwalk_kernel"] >= 1 and st["epochs"] >= 2, (name, path, st, n)
        if ff:
            assert st["rejected"] >= 1 and n["zwalk_kernel"] >= 2, (name, path, st, n)
        else:
            assert st["frontier_chains"] < 2, (name, path, st)
            assert e.walk == "left" or st["list_chains"] >= 1, (name, path, st)
        return
    assert st["frontier_chains"] == 2, (name, path, st)
    assert n["zwalk_kernel"] >= 1, (name, path, n)
    if e.tail == "runs":
        # both chains complete; the host's verdict refuses and the tail kernels decide
        assert tail_ran, (name, path, n)
        assert (n[UNDO] == 0) if path == "frontier_tail0" else (n[UNDO] >= 1), (name, path, n)
    if e.kind == "proven" or e.tail == "none":
        assert st["list_chains"] == 0 and st["epochs"] == 1 and st["rejected"] == 0, (name, path, st)
        if path != "frontier_tail0":
            assert fast == (0 if ff or path == "frontier_cert0" else 2), (name, path, fast)
    if e.tail == "none" and path == "frontier":
        assert n[UNDO] == 0 and all(n[k] == 0 for k in TAIL), (name, path, n)
    if path == "frontier_tail0" and not ff:
        assert tail_ran and n[UNDO] == 0, (name, path, n)


@pytest.mark.parametrize("path", FRONTIER + ("lists", "sequential"))
@pytest.mark.parametrize("name", cc.NAMES)
def test_case(engines, name, path):
    r, e, ref = cc.reference(name)
    res, st, n, fast = _place(engines[path], path, r)
    _same(res, ref)
    if path in FRONTIER:
        _check_stats(name, path, e, st, n, fast)
    elif path == "lists":
        assert n["zwalk_kernel"] == 0, (name, path, n)


@pytest.mark.parametrize("mode", [cc.BF, cc.FF])
def test_resident_batch(engine, mode):
    """All cases of a mode in one place_batch call: the resident kernel's fast winner."""
    names = [k for k in cc.NAMES if cc.reference(k)[1].mode == mode]
    got = engine.place_batch([cc.reference(k)[0] for k in names])
    for k, res in zip(names, got):
        print(k, res.placement[:8].tolist())
    for k, res in zip(names, got):
        _same(res, cc.reference(k)[2])
