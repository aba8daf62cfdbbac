"""Every instance of the resident kernel (csrc/pvt_batch.hip: 1, 2, 4 and 8 waves per round, 1 to
16 hosts per lane) and every switch of its one-wave walks against the CPU restatement, on the
batches of resident_shape_cases.py (whose premises test_resident_shape_cases.py checks on the CPU).

An instance is chosen from the batch's largest round and PVT_RES_WAVES, a walk switch from
PVT_RWALK, both read when the context is created; so each preference has an engine of its own. Every
test also asserts what ran -- ``engine.resident_shape()``, the plan of the last resident launch --
so a preference or a switch that is dropped on the way to the launch cannot pass by comparing the
default instance with the reference.

Placement, order, final availability and (opportunistic) MT19937 state equal the reference bit
for bit in every round."""
import numpy as np
import pytest

import resident_shape_cases as rc
from oracle import oracle
from pivot_place import synthetic
from pivot_place.engine import DeviceBatch, DeviceRound

from test_gpu_epoch_tail import _engine_under

pytestmark = pytest.mark.gpu

POLICY_NAMES = [p[0] for p in rc.POLICIES]
PREF_H = [(pref, H) for pref in rc.PREFS for H in rc.EDGES[pref]]


@pytest.fixture(scope="module")
def engines():
    """One engine per preference, closed after the module."""
    made = {pref: _engine_under(PVT_RES_WAVES=str(pref)) for pref in rc.PREFS}
    yield made
    for eng in made.values():
        eng.close()


@pytest.fixture(scope="module")
def staged_engines():
    """Engines whose host batches take the staged launches (PVT_FUSED=0), per preference."""
    made = {pref: _engine_under(PVT_RES_WAVES=str(pref), PVT_FUSED="0") for pref in (1, 2, 8)}
    yield made
    for eng in made.values():
        eng.close()


def _same(res, ref, what):
    np.testing.assert_array_equal(res.placement, ref.placement, err_msg=what)
    np.testing.assert_array_equal(res.order, ref.order, err_msg=what)
    bad = np.nonzero((res.avail != ref.avail).any(axis=0))[0]
    assert bad.size == 0, "%s: availability differs on hosts %s" % (what, bad[:10])
    if ref.mt_state is not None:
        np.testing.assert_array_equal(res.mt_state, ref.mt_state, err_msg=what)


def _ran(eng, waves, hpl, switches=None):
    s = eng.resident_shape()
    assert (s["waves"], s["hosts_per_lane"], s["wide"]) == (waves, hpl, 0), s
    if switches is not None:
        assert s["switches"] == switches, s


def _batch_equals(eng, rounds, refs, what):
    got = eng.place_batch(rounds)
    assert len(got) == len(refs)
    for i, (res, ref) in enumerate(zip(got, refs)):
        _same(res, ref, "%s round %d" % (what, i))


def test_no_launch_reports_zeros():
    eng = _engine_under(PVT_RES_WAVES="8")
    try:
        assert eng.resident_shape() == {"waves": 0, "hosts_per_lane": 0, "wide": 0, "switches": 0}
    finally:
        eng.close()


@pytest.mark.parametrize("family", rc.FAMILIES)
@pytest.mark.parametrize("policy", POLICY_NAMES)
@pytest.mark.parametrize("pref,H", PREF_H)
def test_shape_matches_oracle(engines, pref, H, policy, family):
    shape = rc.expected_shape(pref, H)
    rounds, refs = rc.reference(family, policy, H, shape if family == "boundary" else None)
    _batch_equals(engines[pref], rounds, refs, "PVT_RES_WAVES=%d H=%d %s %s" % (pref, H, policy, family))
    _ran(engines[pref], *shape, switches=rc.expected_switches(9, H))


@pytest.mark.parametrize("H", rc.SUFFIX_H)
@pytest.mark.parametrize("pref", rc.PREFS)
def test_suffix_maxima(engines, pref, H):
    """The zero-cost window's separation is taken against the largest demands of every remaining
    block: the big task of a later block goes to the exact fit outside the window."""
    rounds, refs = rc.reference("suffix", "ca_bf", H)
    got = engines[pref].place_batch(rounds)
    _ran(engines[pref], *rc.expected_shape(pref, H), switches=9)
    for i, (r, res, ref) in enumerate(zip(rounds, got, refs)):
        if r.n_hosts > 1:
            pos = rc.suffix_facts(r)[3]
            print("round %d: the big task (position %d) on host %d, the reference on host %d"
                  % (i, pos, res.placement[pos], ref.placement[pos]))
    for i, (res, ref) in enumerate(zip(got, refs)):
        _same(res, ref, "PVT_RES_WAVES=%d H=%d suffix round %d" % (pref, H, i))


RWALK = ("10", "13", "73", "585")


@pytest.mark.parametrize("rwalk", RWALK)
@pytest.mark.parametrize("pref", rc.PREFS)
def test_rwalk_switches(pref, rwalk):
    """The rotating walker (10: with 16 rounds every wave index walks), the walks without bulk
    runs (13), run lists for every policy (73) and from two remaining tasks on (585)."""
    policies = ["ca_bf", "ca_ff_keyed", "ca_ff", "vbp_ff"] + (["vbp_bf"] if rwalk in ("73", "585") else [])
    eng = _engine_under(PVT_RES_WAVES=str(pref), PVT_RWALK=rwalk)
    try:
        for H in rc.SUFFIX_H:
            shape = rc.expected_shape(pref, H)
            word = rc.expected_switches(int(rwalk), H)
            assert word == int(rwalk)
            for policy in policies:
                for family in ("plain", "runs") + (("suffix",) if policy == "ca_bf" else ()):
                    rounds, refs = rc.reference(family, policy, H, None, 16)
                    assert len(rounds) == 16
                    _batch_equals(eng, rounds, refs, "PVT_RES_WAVES=%d PVT_RWALK=%s H=%d %s %s"
                                  % (pref, rwalk, H, policy, family))
                    _ran(eng, *shape, switches=word)
    finally:
        eng.close()


# ---- entry points (H = 600: <1,16>, <2,8>, <8,2>; four waves: <4,4>)
ENTRY_H = 600


def _entry_rounds(policy, n=3):
    return [synthetic.make_round(rc.POLICY[policy][0], ENTRY_H - 7 * i, 150 + i, seed=700 + i,
                                 sort_hosts=rc.POLICY[policy][1]) for i in range(n)]


@pytest.mark.parametrize("policy", POLICY_NAMES)
@pytest.mark.parametrize("pref", [1, 2, 8])
def test_single_round(engines, staged_engines, pref, policy):
    """pvt_place on a device round takes the preferred shape; ``place`` is a one-round host batch:
    four waves where host batches are fused, the preferred shape where they are staged."""
    r = _entry_rounds(policy, 1)[0]
    ref = oracle.place(r)
    eng = engines[pref]
    dr = DeviceRound(r, eng.device)
    eng.run(dr)
    _same(dr.result(), ref, "pvt_place")
    _ran(eng, *rc.expected_shape(pref, ENTRY_H), switches=9)
    _same(eng.place(r), ref, "place (fused)")
    _ran(eng, *rc.expected_shape(4, ENTRY_H), switches=9)
    _same(staged_engines[pref].place(r), ref, "place (staged)")
    _ran(staged_engines[pref], *rc.expected_shape(pref, ENTRY_H), switches=9)


@pytest.mark.parametrize("policy", POLICY_NAMES)
@pytest.mark.parametrize("pref", [1, 2, 8])
def test_host_batch(engines, staged_engines, pref, policy):
    rounds = _entry_rounds(policy)
    refs = [oracle.place(r) for r in rounds]
    for eng, shape in ((staged_engines[pref], rc.expected_shape(pref, ENTRY_H)),
                       (engines[pref], rc.expected_shape(4, ENTRY_H))):
        got = eng.place_host_batch([(r, None) for r in rounds])
        for i, (res, ref) in enumerate(zip(got, refs)):
            _same(res, ref, "host batch round %d" % i)
        _ran(eng, *shape, switches=9)


@pytest.mark.parametrize("pref", [1, 2, 8])
def test_mixed_host_batch_takes_four_waves(engines, staged_engines, pref):
    rounds = [_entry_rounds(policy, 1)[0] for policy in POLICY_NAMES]
    refs = [oracle.place(r) for r in rounds]
    for eng in (staged_engines[pref], engines[pref]):
        got = eng.place_host_batch([(r, None) for r in rounds])
        for i, (res, ref) in enumerate(zip(got, refs)):
            _same(res, ref, "mixed host batch round %d" % i)
        _ran(eng, *rc.expected_shape(4, ENTRY_H), switches=9)


@pytest.mark.parametrize("pref", [1, 2, 8])
def test_device_resident_mt_states(engines, pref):
    """Opportunistic rounds whose MT19937 states stay on the device (pvt_place_batch_mt): placed,
    reset and placed again, the same results and states both times."""
    rounds = _entry_rounds("opp", 5)
    refs = [oracle.place(r) for r in rounds]
    eng = engines[pref]
    b = DeviceBatch(rounds, eng.device)
    assert b.mt_dev is not None
    for again in range(2):
        eng.run_batch(b)
        for i, (res, ref) in enumerate(zip(b.results(), refs)):
            _same(res, ref, "run %d round %d" % (again, i))
        _ran(eng, *rc.expected_shape(pref, ENTRY_H), switches=9)
        b.reset()
