"""The wide frontier cases (wide_frontier_cases.py) on the CPU reference alone: every round the
GPU tests use is what it claims to be. An embedded round is placed exactly as the round it embeds,
the planted rounds' answers depend on the clause over the zones outside the component, the
component-limit table has the components it says, and the uncontended rounds place everything at
zero cost."""
import numpy as np
import pytest

import cert_cases as cc
import wide_cases
import wide_frontier_cases as wf
from oracle import oracle
from pivot_place import synthetic


@pytest.mark.parametrize("Z", [64, 512])
@pytest.mark.parametrize("name", cc.NAMES)
def test_embedded_cert_case_equals_the_narrow_one(name, Z):
    r, e, ref = wf.cert_case(name, Z)
    assert r.n_zones == Z and r.n_hosts == cc.H
    assert wf.same_result(oracle.place(r), ref)
    # every zone the case uses lies above id 32, and the two components interleave in global id
    zm = wf.cert_zmap(Z)
    assert zm.min() > 32 and sorted(np.unique(r.zone).tolist()) == sorted(zm[:20].tolist())
    a, b = sorted(zm[[0, 1, 2]].tolist()), sorted(zm[[3, 4, 5]].tolist())
    assert a[0] < b[0] < a[1] < b[1] < a[2] < b[2]
    comps = [c for c in wf.components(r.cost) if len(c) > 1]
    assert a in comps and b in comps and max(len(c) for c in comps) <= 3


@pytest.mark.parametrize("Z", [33, 64, 512])
def test_embedding_with_the_descending_maps(Z):
    """The maps the embedding was checked with, on a case of every kind and both modes."""
    for name in ("c_subnormal", "all_at_limits", "window_cap_nan", "ff_cap_2p500"):
        r, e, ref = cc.reference(name)
        assert wf.same_result(oracle.place(wf.embed(r, Z, wf.plain_zmap(Z))), ref), (name, Z)


def test_embedded_spill_round():
    r, ref = wf.spill_case(64)
    assert r.n_zones == 64 and wf.same_result(oracle.place(r, threads=8), ref)
    # groups anchored in the emptied zones spill: a good part of the winners cost something
    placed, zero = wf.zero_cost_fraction(r, ref)
    assert placed > 0.5 and zero < 0.9, (placed, zero)


@pytest.mark.parametrize("name", list(wf.OUT_CASES))
def test_outside_component_cases(name):
    """The planted host lies in an added zone X, a singleton component: outside A's component. In
    the planted cases the reference puts A's first task on it (its score underflows to 0) and
    exactly the named clause of the row (A, X) fails; in the control every clause holds with
    equality and the reference ignores it."""
    r, planted, ref = wf.out_case(name)
    ce, be, _ = wf.OUT_CASES[name]
    a = int(r.group_anchor[1])
    comp = [c for c in wf.components(r.cost) if a in c][0]
    assert len(comp) == 3 and wf.OUT_X not in comp
    assert [c for c in wf.components(r.cost) if wf.OUT_X in c] == [[wf.OUT_X]]
    assert r.zone[cc.PLANTED] == wf.OUT_X and (r.zone == wf.OUT_X).sum() == 1
    c = r.cost[a, wf.OUT_X] + r.cost[wf.OUT_X, a]
    bw = r.bw[a, wf.OUT_X] + r.bw[wf.OUT_X, a]
    assert c == cc.p2(ce) and bw == cc.p2(be)
    assert (c >= cc.p2(-300)) == (ce >= -300) and (0 < bw <= cc.p2(300)) == (be <= 300)
    assert (c >= cc.p2(-300) and bw <= cc.p2(300)) == (not planted)
    # the separation certificate holds: disk keeps 2^-288 on the planted host, 100 elsewhere
    assert (r.avail.min(axis=1) - r.dem.max(axis=1)).max() == cc.p2(-288)
    assert ref.placement[:2].tolist() == [cc.B_HOST] * 2
    assert ref.placement[2] == (cc.PLANTED if planted else cc.A_HOST)
    # every other row of A's chain and all of B's pass the clause: only (A, X) can decide
    for g in (0, 1):
        an = int(r.group_anchor[g])
        for z in range(r.n_zones):
            if z in comp or (g == 1 and z == wf.OUT_X):
                continue
            cz, bz = r.cost[an, z] + r.cost[z, an], r.bw[an, z] + r.bw[z, an]
            assert cz == 0.0 or (cz >= cc.p2(-300) and 0 < bz <= cc.p2(300))


def test_component_limit_table():
    r, ref = wf.limit_case()
    sizes = sorted(len(c) for c in wf.components(r.cost))
    assert r.n_zones == 70 and sizes == [1] * 5 + [32, 33]
    comps = {min(c): c for c in wf.components(r.cost)}
    assert comps[0] == list(range(32)) and comps[32] == list(range(32, 65))
    anchors = set(r.group_anchor.tolist())
    assert anchors & set(comps[0]) and anchors & set(comps[32]) and anchors & set(range(65, 70))
    # zero cost between consecutive zones only: an anchor's zero-cost zones are at most three
    z0 = (r.cost + r.cost.T) == 0.0
    assert z0.sum(axis=1).max() == 3
    placed, zero = wf.zero_cost_fraction(r, ref)
    assert placed == 1.0 and zero == 1.0


@pytest.mark.parametrize("mode", [wf.BF, wf.FF])
@pytest.mark.parametrize("Z", wf.WIDE_Z)
def test_uncontended_rounds_place_everything_at_zero_cost(Z, mode):
    r, ref = wf.uncontended(mode, Z)
    assert r.n_zones == Z
    assert wf.zero_cost_fraction(r, ref) == (1.0, 1.0)
    assert max(len(c) for c in wf.components(r.cost)) == 3


@pytest.mark.parametrize("Z,n", [(33, 12), (64, 23), (65, 23), (512, 182)])
def test_wide_tables_have_small_components(Z, n):
    cost, _ = synthetic.wide_zone_tables(Z)
    comps = wf.components(cost)
    assert max(len(c) for c in comps) == 3
    assert len(comps) == n


@pytest.mark.parametrize("Z", wf.WIDE_Z)
def test_contended_rounds_stop_chains(Z):
    """wide_cases' large rounds: zero-cost hosts run out, so chains stop and hand over."""
    for mode in (wf.BF, wf.FF):
        r, ref = wide_cases.case(mode, Z, "large")
        p, z0, zp = wide_cases.fractions(r, ref)
        assert 0.25 <= p <= 0.45 and 0.5 <= z0 <= 0.85, (Z, mode, p, z0)
