"""GPU tests of the frontier walk and the group epochs on clusters of 33 to 512 zones (DESIGN.md
§2.6): the rounds of wide_frontier_cases.py on the windowed engine. Placement, order and final
availability equal the CPU reference bit for bit, and the epoch statistics and the launches of the
named kernels say which path ran: the wide instances of the walk (pvt_zwalk_wide.hip) where the
chain's zero-cost component has at most 32 zones and every certificate holds, the exact list path
otherwise -- and always under PVT_ZW_WIDE=0.

The embedded certificate cases reuse cert_cases.Expect. What differs from test_gpu_zero_certs.py:
wide chains take the ordinary prologue (no fast-prologue chains), a PVT_CHAIN_CERT=0 engine is
therefore the same path as the default one, and the keyed path of a wide first-fit round runs no
per-group walk, so there ``frontier_chains`` counts chain walks alone and `< 2` holds for
first-fit hand-overs too."""
import numpy as np
import pytest

import cert_cases as cc
import wide_cases
import wide_frontier_cases as wf
from pivot_place import _abi, policies

from test_gpu_epoch_tail import TAIL, UNDO, _engine_under
from test_gpu_wide_zones import DROPIN, _run_policy
from test_sim_replay import OracleEngine

pytestmark = pytest.mark.gpu

KERNELS = TAIL + (UNDO, "zwalk_kernel")
BF, FF = wf.BF, wf.FF


@pytest.fixture(scope="module")
def engine_tail0():
    eng = _engine_under(PVT_EPOCH_TAIL="0")
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def engine_wide0():
    eng = _engine_under(PVT_ZW_WIDE="0")
    yield eng
    eng.close()


def _same(res, ref):
    """Bit-for-bit; a NaN capacity (window_cap_nan) must be a NaN in the same place."""
    np.testing.assert_array_equal(res.placement, ref.placement)
    np.testing.assert_array_equal(res.order, ref.order)
    nan = np.isnan(ref.avail)
    np.testing.assert_array_equal(np.isnan(res.avail), nan)
    bad = np.nonzero((np.where(nan, 0.0, res.avail) != np.where(nan, 0.0, ref.avail)).any(axis=0))[0]
    assert bad.size == 0, "availability differs on hosts %s" % bad[:10]


def _place(eng, r, path="frontier"):
    """The round on the windowed engine: result, epoch statistics, launches per named kernel,
    fast-prologue chains, list windows."""
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
        st["fast"] = eng.prologue_stats()["fast_chains"]
        st["windows"] = eng.last_stats()["windows"]
        n = {k: eng.kernel_kstats(k)["launches"] for k in KERNELS}
    finally:
        eng.set_profiling(False)
        eng.set_zero_walk(True)
        eng.set_epochs(True)
        eng.set_resident(_abi.PVT_RESIDENT_MAX_HOSTS)
    print(path, st, n)
    return res, st, n


# ---- 2. every zero-score certificate, wide -------------------------------------------------------
def _check_cert_stats(name, path, e, st, n):
    tail_ran = n["epoch_final_kernel"] >= 1 and n["epoch_accept_apply_kernel"] >= 1
    assert st["fast"] == 0, (name, path, st)             # (wide chains: the ordinary prologue)
    if e.walk in ("left", "left_all"):
        assert n["zwalk_kernel"] >= 1 and st["epochs"] >= 2, (name, path, st, n)
        assert st["frontier_chains"] < 2, (name, path, st)
        if e.mode == FF:
            assert st["rejected"] >= 1, (name, path, st)
        else:
            assert e.walk == "left" or st["list_chains"] >= 1, (name, path, st)
        return
    assert st["frontier_chains"] == 2, (name, path, st)
    assert n["zwalk_kernel"] >= 1, (name, path, n)
    if e.tail == "runs":
        assert tail_ran, (name, path, n)
        assert (n[UNDO] == 0) if path == "frontier_tail0" else (n[UNDO] >= 1), (name, path, n)
    if e.kind == "proven" or e.tail == "none":
        assert st["list_chains"] == 0 and st["epochs"] == 1 and st["rejected"] == 0, (name, path, st)
    if e.tail == "none" and path == "frontier":
        assert n[UNDO] == 0 and all(n[k] == 0 for k in TAIL), (name, path, n)
    if path == "frontier_tail0" and e.mode != FF:
        assert tail_ran and n[UNDO] == 0, (name, path, n)


@pytest.mark.parametrize("path", ["frontier", "frontier_tail0", "lists", "sequential"])
@pytest.mark.parametrize("Z", [64, 512])
@pytest.mark.parametrize("name", cc.NAMES)
def test_cert_case(engine, engine_tail0, name, Z, path):
    r, e, ref = wf.cert_case(name, Z)
    res, st, n = _place(engine_tail0 if path == "frontier_tail0" else engine, r, path)
    _same(res, ref)
    if path in ("frontier", "frontier_tail0"):
        _check_cert_stats(name, path, e, st, n)
    elif path == "lists":
        assert n["zwalk_kernel"] == 0, (name, path, n)


@pytest.mark.parametrize("Z", [64, 512])
@pytest.mark.parametrize("mode", [BF, FF])
def test_cert_cases_resident_batch(engine, mode, Z):
    names = [k for k in cc.NAMES if cc.reference(k)[1].mode == mode]
    got = engine.place_batch([wf.cert_case(k, Z)[0] for k in names])
    for k, res in zip(names, got):
        _same(res, wf.cert_case(k, Z)[2])


# ---- 3. a certificate only the wide walk has -----------------------------------------------------
@pytest.mark.parametrize("name", list(wf.OUT_CASES))
def test_zone_outside_the_component(engine, name):
    r, planted, ref = wf.out_case(name)
    res, st, n = _place(engine, r)
    _same(res, ref)
    assert n["zwalk_kernel"] >= 1, n
    if planted:                                 # A's chain is left to the exact path
        assert st["frontier_chains"] < 2 and st["epochs"] >= 2, st
    else:                                       # every clause at its limit: both chains proven
        assert st["frontier_chains"] == 2 and st["epochs"] == 1 and st["list_chains"] == 0, st


# ---- 4. the component limit ----------------------------------------------------------------------
def test_component_limit(engine):
    """A chain of the 32-zone component is walked; a chain of the 33-zone component reports no
    walk and its epoch goes to the list walk."""
    r, ref = wf.limit_case()
    res, st, n = _place(engine, r)
    _same(res, ref)
    assert st["frontier_chains"] > 0 and st["list_chains"] > 0, st


# ---- 5. uncontended wide rounds ------------------------------------------------------------------
@pytest.mark.parametrize("mode", [BF, FF])
@pytest.mark.parametrize("Z", wf.WIDE_Z)
def test_uncontended_round_takes_the_fast_path(engine, engine_wide0, Z, mode):
    r, ref = wf.uncontended(mode, Z)
    res, st, n = _place(engine, r)
    _same(res, ref)
    assert st["epochs"] >= 1 and st["frontier_chains"] > 0 and st["list_chains"] == 0, st
    assert n["zwalk_kernel"] >= 1, n
    res0, st0, n0 = _place(engine_wide0, r)
    _same(res0, ref)
    assert st0["frontier_chains"] == 0 and n0["zwalk_kernel"] == 0, (st0, n0)


# ---- 6. contended wide rounds --------------------------------------------------------------------
@pytest.mark.parametrize("mode", [BF, FF])
@pytest.mark.parametrize("Z", wf.WIDE_Z)
def test_contended_round(engine, Z, mode):
    r, ref = wide_cases.case(mode, Z, "large")
    res, st, n = _place(engine, wide_cases.fresh(r))
    _same(res, ref)
    if mode == BF:
        assert st["epochs"] >= 1, st


def test_embedded_spill_round_rejects(engine):
    r, ref = wf.spill_case(64)
    res, st, n = _place(engine, r)
    _same(res, ref)
    assert st["rejected"] > 0, st


# ---- 7. the epoch tail ---------------------------------------------------------------------------
def test_accepted_epoch_has_no_tail(engine):
    r, ref = wf.uncontended(BF, 64)
    res, st, n = _place(engine, r)
    _same(res, ref)
    assert n["zwalk_kernel"] >= 1 and n[UNDO] == 0 and all(n[k] == 0 for k in TAIL), n


def test_missed_epoch_is_undone_then_decided_by_the_tail(engine, engine_tail0):
    """Zones 0-9 have no capacity: chains anchored there stop while others completed and wrote
    their windows back; the write-backs are undone (epoch_undo_kernel is launched only when some
    chain wrote back) before the tail kernels decide."""
    r, ref = wf.stopped_chains_case()
    res, st, n = _place(engine, r)
    _same(res, ref)
    assert n["zwalk_kernel"] >= 1 and n[UNDO] >= 1 and all(n[k] >= 1 for k in TAIL), n
    res0, st0, n0 = _place(engine_tail0, r, "frontier_tail0")
    _same(res0, ref)
    assert n0[UNDO] == 0 and all(n0[k] >= 1 for k in TAIL), n0


def test_contended_epochs_are_decided_by_the_tail(engine):
    """wide_cases' contended round: every chain stops, nothing is written back, the tail decides."""
    r, ref = wide_cases.case(BF, 64, "large")
    res, st, n = _place(engine, wide_cases.fresh(r))
    _same(res, ref)
    assert n["zwalk_kernel"] >= 1 and all(n[k] >= 1 for k in TAIL), n


# ---- 8. drop-in ----------------------------------------------------------------------------------
@pytest.mark.parametrize("cls,kwargs", DROPIN[:2])
def test_dropin_cost_aware_on_a_65_zone_cluster_of_3000_hosts(engine, cls, kwargs):
    """Above PVT_RESIDENT_WIDE_MAX_HOSTS: the windowed engine takes the rounds."""
    assert cls is policies.CostAwareGlobalScheduler
    args = (65, 3000, 40, 800, 5)
    want = _run_policy(cls, dict(kwargs), args, OracleEngine())
    got = _run_policy(cls, dict(kwargs), args, engine)
    assert got[0] == want[0] and got[1] == want[1]
    assert np.array_equal(got[2], want[2])
    assert np.array_equal(got[3][0], want[3][0]) and got[3][1] == want[3][1]
