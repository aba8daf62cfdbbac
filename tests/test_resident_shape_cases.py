"""The resident shape cases (resident_shape_cases.py) on the CPU reference alone: every family
still has the property it exists for, every round is one the engine may be given
(checks.check_arrays), and ``expected_shape`` / ``EDGES`` agree with the rule and the
static_asserts of csrc/pvt_kernels.h. A later edit to synthetic.py or to a builder cannot silently
turn a discriminating case into a vacuous one."""
import os
import re

import numpy as np
import pytest

import resident_shape_cases as rc
from pivot_place import _abi, checks

POLICY_NAMES = [p[0] for p in rc.POLICIES]
# (preference, largest round) of every shape test, and the sizes any of them uses
PREF_H = [(pref, H) for pref in rc.PREFS for H in rc.EDGES[pref]]
ALL_H = sorted({H for _, H in PREF_H})


def test_expected_shape_at_every_edge():
    want = {8: {1: (8, 1), 65: (8, 1), 512: (8, 1), 513: (8, 2), 1024: (8, 2), 1025: (8, 4),
                2048: (8, 4), 2049: (8, 8), 4096: (8, 8)},
            2: {512: (4, 2), 513: (2, 8), 1024: (2, 8), 1025: (2, 16), 2048: (2, 16), 2049: (4, 16)},
            1: {512: (4, 2), 513: (1, 16), 1024: (1, 16), 1025: (4, 8)},
            4: {256: (4, 1), 257: (4, 2)}}
    for pref in rc.PREFS:
        assert sorted(want[pref]) == list(rc.EDGES[pref])
        for H, shape in want[pref].items():
            assert rc.expected_shape(pref, H) == shape, (pref, H)
    # the 12 instances per policy, each reached by a shape test or by the entry-point tests (600)
    inst = {rc.expected_shape(p, H) for p, H in PREF_H} | {rc.expected_shape(4, 600)}
    assert inst == {(4, 1), (4, 2), (4, 4), (4, 8), (4, 16), (8, 1), (8, 2), (8, 4), (8, 8), (2, 8),
                    (2, 16), (1, 16)}
    for pref, H in PREF_H:
        waves, hpl = rc.expected_shape(pref, H)
        assert waves * hpl * rc.WAVE >= H
        # an edge is the last size of its instance or the first
        assert hpl == 1 or rc.expected_shape(pref, H - 1) != (waves, hpl) or \
            rc.expected_shape(pref, H + 1) != (waves, hpl) or H == 4096, (pref, H)


def test_header_asserts_the_same_shapes():
    """Every resident_shape(pref, H) == ResidentShape{w, h} clause of pvt_kernels.h's static_asserts
    agrees with expected_shape, and every edge of EDGES stands in one."""
    path = os.path.join(os.path.dirname(os.path.abspath(rc.synthetic.__file__)), "..", "csrc", "pvt_kernels.h")
    with open(path) as f:
        text = f.read().replace("RES_MAX_HOSTS)", "4096)")
    seen = set()
    for pref, H, w, h in re.findall(r"resident_shape\((\d+), (\d+)\) == ResidentShape\{(\d+), (\d+)\}", text):
        assert rc.expected_shape(int(pref), int(H)) == (int(w), int(h)), (pref, H)
        seen.add((int(pref), int(H)))
    assert set(PREF_H) <= seen, sorted(set(PREF_H) - seen)
    m = re.search(r"constexpr\s+int\s+RW_MAXH\s*=\s*(\d+)\s*;", text)
    assert m and int(m.group(1)) == rc.RW_MAXH


def test_expected_switches():
    for word in (9, 10, 13, 73, 585, 0, 16, 32):
        assert rc.expected_switches(word, 600) == word and rc.expected_switches(word, 1024) == word
    assert rc.expected_switches(3, 1024) == 1 and rc.expected_switches(4, 1024) == 0
    assert rc.expected_switches(9, 1025) == 0 and rc.expected_switches(585, 1025) == 576


@pytest.mark.parametrize("H", ALL_H)
def test_batch_sizes(H):
    for n in (7, 16):
        sz = rc.sizes(H, n)
        assert len(sz) == n and 6 <= n
        hs = [h for h, _ in sz]
        assert max(hs) == H == hs[0] and 1 in hs and max(1, H - 63) in hs
        assert all(130 <= t <= 300 and t % 64 for _, t in sz)


@pytest.mark.parametrize("policy", POLICY_NAMES)
@pytest.mark.parametrize("family", ["plain", "tied", "runs", "dry"])
def test_rounds_are_valid(family, policy):
    """Every round of the batches at the smallest and the largest size, and at 600 (the 16-round
    batches of the switch tests), passes the content rules."""
    for H, n in ((1, 7), (4096, 7), (600, 16)):
        for r in rc._BUILD[family](policy, H, n):
            assert checks.check_arrays(r).ok, (family, policy, H)
            assert r.n_hosts <= H and r.n_tasks <= 300
        assert max(r.n_hosts for r in rc._BUILD[family](policy, H, n)) == H


@pytest.mark.parametrize("policy", POLICY_NAMES)
def test_plain_places_on_many_hosts(policy):
    rounds, refs = rc.reference("plain", policy, 513)
    assert any((ref.placement >= 0).sum() > 100 for ref in refs)
    mode, sort_hosts = rc.POLICY[policy]
    assert all(r.mode == mode and bool(r.sort_hosts) == (sort_hosts and mode in (rc.CA_FF, rc.CA_BF))
               for r in rounds)


def test_alternating_ranks():
    for H in (1, 2, 65, 513, 600, 1024, 1025, 4096):
        rank = rc.alternating_ranks(H)
        assert sorted(rank.tolist()) == list(range(H))
        if H > 64:
            order = np.argsort(rank)
            half = 1 << ((H - 1).bit_length() - 1)
            # no two consecutive ranks on the upper side of the largest power of two below H, so
            # every upper host is a crossing there and back; and consecutive ranks lie at least an
            # eighth of the index range apart
            up = order >= half
            assert not (up[1:] & up[:-1]).any()
            assert (np.diff(up.astype(int)) != 0).sum() >= 2 * (H - half) - 1
            assert np.abs(np.diff(order)).min() >= half // 4


@pytest.mark.parametrize("policy", POLICY_NAMES)
@pytest.mark.parametrize("H", [1024, 2048])
def test_tied_hosts_and_crossings(policy, H):
    """Hosts of two kinds only, each taking at most two tasks, so the winner moves on all the time:
    over more than one 64-host span in every policy, and (vbp best-fit, by the ranks) between the
    waves of every multi-wave shape that runs this size."""
    rounds, refs = rc.reference("tied", policy, H)
    for r in rounds:
        assert checks.check_arrays(r).ok
        assert set(np.unique(r.avail[0]).tolist()) <= {0.5, 1.0} and (r.avail[1] == 40000.0).all()
        assert r.dem[0].min() >= 0.5
    r, ref = rounds[0], refs[0]
    placed = ref.placement[ref.order]
    placed = placed[placed >= 0]
    assert np.unique(placed).size >= 65
    if policy == "vbp_bf":
        assert (r.tiebreak == rc.alternating_ranks(H)).all()
        shapes = [rc.expected_shape(pref, H) for pref in rc.PREFS if H in rc.EDGES[pref]]
        assert len([s for s in shapes if s[0] > 1]) >= 2
        for waves, hpl in shapes:
            if waves > 1:
                assert (np.diff(placed // (rc.WAVE * hpl)) != 0).sum() >= 50, (waves, hpl)


@pytest.mark.parametrize("policy", POLICY_NAMES)
@pytest.mark.parametrize("pref,H", PREF_H)
def test_boundary_slots_fill(policy, pref, H):
    shape = rc.expected_shape(pref, H)
    rounds, refs = rc.reference("boundary", policy, H, shape)
    for r, ref in zip(rounds, refs):
        assert checks.check_arrays(r).ok
        slots = rc.boundary_slots(r.n_hosts, *shape)
        assert slots[0] == 0 and slots[-1] == r.n_hosts - 1
        span = rc.WAVE * shape[1]
        assert all(s % span in (0, span - 1) or s == r.n_hosts - 1 for s in slots)
        got = np.bincount(ref.placement[ref.placement >= 0], minlength=r.n_hosts)
        assert (got[slots] == 2).all() and got.sum() == 2 * len(slots)
        assert (ref.placement < 0).sum() == r.n_tasks - 2 * len(slots) > 0
        left = ref.avail[:, slots]
        assert (left[0] == 0.5).all() and (left[1] == 1024.0).all()


@pytest.mark.parametrize("policy", POLICY_NAMES)
def test_runs_are_the_sticky_edits(policy):
    rounds, refs = rc.reference("runs", policy, 1024)
    for i, (r, ref) in enumerate(zip(rounds, refs)):
        assert checks.check_arrays(r).ok
        s = (0, 3, 4)[i % 3]
        rows = {(a, b) for a, b in zip(r.dem[0].tolist(), r.dem[1].tolist())}
        assert rows <= {0: {(0.5, 2048.0), (0.25, 1024.0)}, 3: {(1.5, 3000.0)}, 4: {(0.5, 2048.0)}}[s]
        if s == 3:
            assert r.avail[0].max() <= 4.5
        if s == 4 and r.n_hosts > 1:
            # exact fits: some host ends with no cpus or no memory left
            hit = np.unique(ref.placement[ref.placement >= 0])
            assert ((ref.avail[0, hit] == 0.0) | (ref.avail[1, hit] == 0.0)).any() or \
                r.mode in (rc.CA_FF, rc.VBP_BF)    # (strict fit: the last copy fails)


@pytest.mark.parametrize("policy", POLICY_NAMES)
def test_dry_rounds(policy):
    rounds, refs = rc.reference("dry", policy, 1025)
    assert [r.n_tasks == 0 for r in rounds] == [False, False, True, False, False, False, False]
    for r, ref in zip(rounds, refs):
        assert checks.check_arrays(r).ok
        big = np.nonzero(r.dem[0] == rc.DRY_CPUS)[0]
        assert big.tolist() == list(range(0, r.n_tasks, 7)) and rc.DRY_CPUS > r.avail[0].max()
        assert (ref.placement[big] == -1).all()
        if r.n_tasks:
            assert ref.placement.shape == (r.n_tasks,)
        if r.n_hosts > 100 and r.n_tasks:
            assert (ref.placement >= 0).any()


@pytest.mark.parametrize("H", rc.SUFFIX_H)
def test_suffix_rounds(H):
    """Certificate (ii) holds against the first block's largest demands and fails against the
    round's; the reference puts the big task on the outside host, a first fit over the window
    alone elsewhere."""
    rounds, refs = rc.reference("suffix", "ca_bf", H)
    assert len(rounds) == 7 and max(r.n_hosts for r in rounds) == H
    blocks = set()
    for r, ref in zip(rounds, refs):
        assert checks.check_arrays(r).ok
        if r.n_hosts == 1:
            continue
        assert r.mode == rc.CA_BF and not r.sort_tasks and r.n_groups == 1
        assert (ref.order == np.arange(r.n_tasks)).all()
        assert 512 < r.n_hosts <= rc.RW_MAXH
        safe, sep0, sep, pos, out, where = rc.suffix_facts(r)
        assert safe and sep0 and not sep
        assert pos >= 64 and tuple(r.dem[:, pos]) == rc.SUFFIX_BIG
        assert tuple(r.avail[:, out]) == rc.SUFFIX_BIG
        a = int(r.group_anchor[0])
        inside = (r.cost[a, r.zone] + r.cost[r.zone, a]) == 0.0
        assert (r.avail[0, ~inside] >= 2.0).all() and (r.avail[0, :out] == 1.5).all()
        assert ref.placement[pos] == out
        assert where >= 0 and where != out and inside[where]
        assert (ref.placement >= 0).all()
        blocks.add(pos // 64)
    assert blocks == {1, 2}
    # the issue's round: task 70 on host 3 (zone 3, anchor 0)
    if H == 600:
        r, ref = rounds[0], refs[0]
        assert (r.n_tasks, int(r.group_anchor[0]), int(ref.placement[70])) == (130, 0, 3)
    r, ref = rounds[1], refs[1]
    assert r.n_tasks == 200 and rc.suffix_facts(r)[3] == 150


def test_policies_cover_the_five_modes():
    assert {m for _, m, _ in rc.POLICIES} == {_abi.PVT_CA_FF, _abi.PVT_CA_BF, _abi.PVT_OPP,
                                              _abi.PVT_VBP_FF, _abi.PVT_VBP_BF}
    assert [s for _, m, s in rc.POLICIES if m == _abi.PVT_CA_FF] == [True, False]
