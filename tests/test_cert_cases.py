"""The certificate cases (cert_cases.py) on the CPU reference alone: every case still does what it
exists for. A hand-over case is one in which the reference puts A's first task on the planted host
(so an engine that ignored the failing clause would place it elsewhere); a proven case one in which
the reference ignores the planted host although every clause sits at its limit. A later edit to
synthetic.py or to a builder cannot silently turn a discriminating case into a vacuous one."""
import os
import re

import numpy as np
import pytest

import cert_cases as cc
from oracle import oracle


def _sum(t, a, z):
    return t[a, z] + t[z, a]


@pytest.mark.parametrize("name", cc.NAMES)
def test_precondition(name):
    r, e, ref = cc.reference(name)
    assert r.n_hosts == cc.H and r.n_tasks <= 68
    assert r.group_anchor.tolist()[:2] == [cc.B_ZONE, cc.A_ZONE]    # (a third group: anchor 1, A's chain)
    assert r.group_anchor.tolist()[2:] in ([], [1])
    assert r.task_group[e.a0] == 1
    a_first = int(np.nonzero(r.task_group == 1)[0][0])
    assert ref.order[a_first] == (e.unplaced[0] if e.unplaced else e.a0)   # A's first in processing order
    unplaced = np.nonzero(ref.placement < 0)[0].tolist()
    assert unplaced == list(e.unplaced), unplaced
    assert ref.placement[0] == cc.B_HOST
    assert ref.placement[e.a0] == e.a0_host, (ref.placement[e.a0], e.a0_host)
    if e.kind == "handover":
        assert e.a0_host != cc.A_HOST and e.a0_host < cc.A_HOST
        # the winner lies outside the anchor's zero-cost zones: its score is 0 by underflow or as
        # an exact fit (first-fit: its key), the cases the certificates exist for
        assert _sum(r.cost, cc.A_ZONE, r.zone[e.a0_host]) > 0.0
    elif e.kind == "proven":
        assert e.a0_host == cc.A_HOST
    else:
        assert e.kind == "bound"


def test_skeleton_without_a_plant():
    """Nothing planted: [3, 3, 40, 40, ...]; hosts 3 and 40 are the groups' first zero-cost fits."""
    r = cc.skeleton(cc.BF, 6, 2)
    ref = oracle.place(r)
    assert ref.placement.tolist() == [3, 3] + [40] * 6
    assert _sum(r.cost, cc.A_ZONE, r.zone[cc.PLANTED]) > 0.0
    assert _sum(r.cost, cc.B_ZONE, r.zone[cc.PLANTED]) == 0.0
    for z in (0, 1, 2):
        assert _sum(r.cost, cc.A_ZONE, z) == 0.0


@pytest.mark.parametrize("name,c_ok,bw_ok,sep_ok", [
    ("c_subnormal", False, True, True), ("c_at_limits", False, True, True),
    ("bw_huge", True, False, True), ("sep_fails", True, True, False),
    ("all_at_limits", True, True, True)])
def test_one_clause_fails(name, c_ok, bw_ok, sep_ok):
    """Certificate 2 recomputed in numpy for anchor zone 0: exactly the named clause fails, and in
    all_at_limits each holds with equality."""
    r, e, _ = cc.reference(name)
    out = [z for z in range(r.n_zones) if _sum(r.cost, cc.A_ZONE, z) != 0.0]
    c = np.array([_sum(r.cost, cc.A_ZONE, z) for z in out])
    bw = np.array([_sum(r.bw, cc.A_ZONE, z) for z in out])
    sep = (r.avail.min(axis=1) - r.dem.max(axis=1)).max()
    assert bool((c >= cc.p2(-300)).all()) == c_ok
    assert bool(((bw > 0) & (bw <= cc.p2(300))).all()) == bw_ok
    assert bool(sep >= cc.p2(-288)) == sep_ok
    if name == "all_at_limits":
        assert c.min() == cc.p2(-300) and bw.max() == cc.p2(300) and sep == cc.p2(-288)


def test_verdict_mixed_dims_needs_the_and():
    """Each chain leaves a dimension undemanded whose host minimum is >= 2^-287, but the two sets
    are disjoint: accepted by an OR across the chains' certificate words, refused by the AND."""
    r, e, ref = cc.reference("verdict_mixed_dims")
    hmin = r.avail.min(axis=1)
    und = [set(np.nonzero((r.dem[:, r.task_group == g] == 0.0).all(axis=1))[0].tolist()) for g in (0, 1)]
    ok = [{d for d in u if hmin[d] >= cc.p2(-287)} for u in und]
    assert ok[0] and ok[1] and not (ok[0] & ok[1]), (und, hmin)
    assert ref.placement.tolist() == [3, 3, 3, 3, 40, 40, 40]
    # the walk's own certificates hold: memory separates hosts from tasks
    assert (hmin - r.dem.max(axis=1)).max() >= cc.p2(-288)


@pytest.mark.parametrize("name,e2", [("verdict_min_at_limit", -287), ("verdict_min_below", -288)])
def test_verdict_minimum(name, e2):
    r, e, _ = cc.reference(name)
    hmin = r.avail.min(axis=1)
    und = np.nonzero((r.dem == 0.0).all(axis=1))[0].tolist()
    assert und == [2, 3]
    assert max(hmin[d] for d in und) == cc.p2(e2)
    assert (hmin - r.dem.max(axis=1)).max() >= cc.p2(-288)


@pytest.mark.parametrize("name,sep_ok", [
    ("in_window_underflow", False), ("nontransitive_positive", False),
    ("in_window_underflow_walked", True), ("nontransitive_positive_walked", True)])
def test_in_window_cases(name, sep_ok):
    """Zone 2 joins anchor 0's component through zone 1 but is not a zero-cost zone of anchor 0.
    Only in the _walked variants is host 2 a window host (the union of the chain's anchors'
    zero-cost zones holds zone 2, through the group anchored in zone 1) with a separating
    dimension left."""
    r, e, _ = cc.reference(name)
    assert _sum(r.cost, 0, 2) > 0.0 and _sum(r.cost, 0, 1) == 0.0 and _sum(r.cost, 1, 2) == 0.0
    chain = [int(a) for a in r.group_anchor if a in (0, 1, 2)]
    U = {z for a in chain for z in range(r.n_zones) if _sum(r.cost, a, z) == 0.0}
    assert (2 in U) == sep_ok and U <= {0, 1, 2}
    sep = (r.avail.min(axis=1) - r.dem.max(axis=1)).max()
    assert bool(sep >= cc.p2(-288)) == sep_ok


def test_first_fit_sizes_and_keys():
    n = cc.keyed_frontier_min() + 2
    for name, zero_key in (("ff_cap_2p500", True), ("ff_cap_inside", False)):
        r, e, ref = cc.reference(name)
        assert r.n_tasks == 2 * n and r.sort_hosts
        a = r.avail[:, cc.PLANTED]
        key = _sum(r.cost, 0, 4) / (np.sqrt((a * a).sum()) * _sum(r.bw, 0, 4))
        assert (key == 0.0) == zero_key, key
        on_planted = (ref.placement[n:] == cc.PLANTED)
        assert on_planted.all() if zero_key else not on_planted.any()
    r, e, ref = cc.reference("ff_negative_demand")
    assert (r.dem < 0).sum() == 1 and r.dem[2, e.a0] == -1.0
    assert (np.sqrt((r.avail * r.avail).sum(axis=0)) > 0).all()


def test_fixtures_sit_at_the_header_constants():
    """The thresholds of csrc/pvt_cert.h, read from its `constexpr double NAME = 0x1p...;` lines, are
    the values the cases are planted at: the limit itself where a case must hold, one step (a factor
    of two) past it where it must fail."""
    path = os.path.join(os.path.dirname(os.path.abspath(cc.synthetic.__file__)), "..", "csrc", "pvt_cert.h")
    with open(path) as f:
        K = {n: float.fromhex(v) for n, v in
             re.findall(r"^constexpr\s+double\s+(\w+)\s*=\s*(0x1p[-+]?\d+)\s*;", f.read(), re.M)}
    assert sorted(K) == ["CERT_BOUND", "CERT_BW_MAX", "CERT_C_MIN", "CERT_FF_CAP", "CERT_MARGIN",
                         "CERT_RES_MIN", "CERT_S2_MIN", "CERT_SEP"], sorted(K)
    assert K["CERT_S2_MIN"] == K["CERT_RES_MIN"] ** 2 and K["CERT_MARGIN"] == 2 * K["CERT_SEP"]

    def clause2(name):
        r = cc.reference(name)[0]
        z = r.zone[cc.PLANTED]
        return (_sum(r.cost, cc.A_ZONE, z), _sum(r.bw, cc.A_ZONE, z),
                (r.avail.min(axis=1) - r.dem.max(axis=1)).max())

    # *_at_limits: every clause that holds, holds with equality; sep_fails: c and bw likewise
    assert clause2("all_at_limits") == (K["CERT_C_MIN"], K["CERT_BW_MAX"], K["CERT_SEP"])
    c, bw, sep = clause2("c_at_limits")
    assert c < K["CERT_C_MIN"] and (bw, sep) == (K["CERT_BW_MAX"], K["CERT_SEP"])
    c, bw, sep = clause2("sep_fails")
    assert (c, bw) == (K["CERT_C_MIN"], K["CERT_BW_MAX"]) and sep < K["CERT_SEP"]
    # the verdict's minimum: accepted at the margin, refused one step below, where the walk's
    # separation still holds
    for name, v in (("verdict_min_at_limit", K["CERT_MARGIN"]), ("verdict_min_below", K["CERT_MARGIN"] / 2)):
        r = cc.reference(name)[0]
        assert r.avail[2].min() == r.avail[2].max() == v and v >= K["CERT_SEP"]
    # certificate 3: one step past the bound, in a window capacity and in a demand
    assert cc.reference("window_cap_2p501")[0].avail[0, cc.A_HOST] == 2 * K["CERT_BOUND"]
    assert cc.reference("dem_2p501")[0].dem.max() == 2 * K["CERT_BOUND"]
    # first-fit: the planted host's norm at the capacity bound (its capacities inside it), and a
    # capacity past it that certificate 3 still admits
    a = cc.reference("ff_cap_inside")[0].avail[:, cc.PLANTED]
    assert a.max() <= K["CERT_FF_CAP"] and np.sqrt((a * a).sum()) == K["CERT_FF_CAP"]
    a = cc.reference("ff_cap_2p500")[0].avail[:, cc.PLANTED]
    assert K["CERT_FF_CAP"] < a.min() == a.max() <= K["CERT_BOUND"]
