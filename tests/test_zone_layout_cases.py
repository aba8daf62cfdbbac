"""The irregular zone layouts (zone_layout_cases.py) on the CPU reference alone: every round that
test_gpu_zone_layouts.py places is what its docstring claims, and the reference's placements touch
the hosts at the compaction's boundaries -- the pass boundary, the row and wave boundaries of both
instantiations, the partial last quad, the last slot of the window. A GPU parity test on a case is
only worth something if the answer depends on those hosts."""
import numpy as np
import pytest

import zone_layout_cases as zl
from pivot_place import synthetic

MODES = [zl.BF, zl.FF]
IDS = ["bf", "ff"]


def _by_anchor(r, ref, anchor):
    """(placements in processing order, zero-cost flags) of the tasks of the group anchored there."""
    g = int(np.nonzero(r.group_anchor == anchor)[0][0])
    t = ref.order[r.task_group[ref.order] == g]
    return ref.placement[t], zl.zero_cost(r, ref)[t]


def _common(name, r, ref, placed_share=1.0):
    assert r.n_hosts % 4 == zl.RESIDUE[name]
    assert sorted(ref.order.tolist()) == list(range(r.n_tasks))
    assert (ref.placement >= 0).mean() >= placed_share
    assert r.zone.min() >= 0 and r.zone.max() < r.n_zones


def test_geometry_and_components():
    assert zl.PASS == 8 * 256 * 4 == 2 * 1024 * 4
    assert zl.ROW_WALK == 256 * 4 and zl.ROW_ORDER == 1024 * 4 and zl.WAVE_WALK == 64 * 4
    assert zl.ROW_WALK == zl.ZW_M and zl.ZW_MBIG == 3 * zl.ZW_M
    cost = zl._round(zl.BF, 8, 1, 1).cost
    assert zl.components(cost) == [[0, 1, 2], [3, 4, 5], [6, 7], [8, 9, 10], [11, 12], [13, 14, 15],
                                   [16, 17, 18], [19]]
    s = cost + cost.T
    assert s[s > 0].min() == 0.02
    wide, _ = synthetic.wide_zone_tables(zl.WIDE_Z)
    comps = zl.components(wide)
    for c in ([31, 32, 33], [34, 35, 36], [68, 69]):
        assert c in comps
    a = zl.component_of(wide, 31)
    assert a[0] < 32 <= a[-1]                  # straddles the narrow paths' zone bound
    # wide_map keeps the component structure of the narrow zones
    m = zl.wide_map()
    for c in zl.components(cost):
        assert [z for z in zl.component_of(wide, int(m[c[0]])) if z in m.tolist()] == m[c].tolist()


# ---- planted -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["planted", "wide_planted"])
@pytest.mark.parametrize("mode", MODES, ids=IDS)
def test_planted(name, mode):
    r, ref = zl.reference(name, mode)
    wide = name == "wide_planted"
    H = r.n_hosts
    assert H == (zl.BLOCKS_H if wide else 2 * zl.PASS + 3)
    _common(name, r, ref)
    m = zl.wide_map() if wide else np.arange(zl.Z)
    a, b = zl.planted_sets(H)
    assert a.tolist() == list(range(8188, 8196)) + [H - 3, H - 2, H - 1]
    assert b.tolist() == [1021, 1022, 1023, 1024, 1025, 4094, 4095, 4096, 4097] + (
        [10239, 10240] if wide else [12287, 12288])
    assert not set(a) & set(b)
    # the histogram: 11 hosts of A over its three zones, 11 of B, everything else far
    hist = np.bincount(r.zone, minlength=r.n_zones)
    assert hist[m[[0, 1, 2]]].tolist() == [4, 4, 3] and hist[m[[3, 4, 5]]].tolist() == [4, 4, 3]
    assert hist[m[zl.FAR]] == H - 22 and hist.sum() == H
    assert np.isin(r.zone[a], m[[0, 1, 2]]).all() and np.isin(r.zone[b], m[[3, 4, 5]]).all()
    # the boundaries the sets straddle
    assert a[3] == zl.PASS - 1 and a[4] == zl.PASS and (H - 3) % 4 == 0
    assert b[2] == zl.ROW_WALK - 1 and b[3] == zl.ROW_WALK and zl.ROW_WALK % zl.WAVE_WALK == 0
    assert b[6] == zl.ROW_ORDER - 1 and b[7] == zl.ROW_ORDER
    assert b[10] > zl.PASS and (b[10] - zl.PASS) % zl.ROW_WALK == 0
    assert r.group_anchor.tolist() == m[[0, 3, 1, 4, zl.FAR]].tolist()
    assert np.bincount(r.task_group).tolist() == [88, 88, 88, 88, 40]
    # every planted host is filled
    per_host = np.bincount(ref.placement, minlength=H)
    full = 16 if mode == zl.BF else 15
    assert (per_host[a] == full).all() and (per_host[b] == full).all()
    # the groups anchored at A's zones use A in index order, and only A at zero cost
    p0, z0 = _by_anchor(r, ref, m[0])
    p1, z1 = _by_anchor(r, ref, m[1])
    used = np.concatenate([p0[z0], p1[z1]])
    assert z0.all() and (np.diff(used) >= 0).all()
    assert sorted(set(used.tolist())) == a.tolist()
    assert np.bincount(used, minlength=H)[a].tolist() == [full] * len(a)
    assert z1.sum() == len(a) * full - 88


# ---- window_edge ---------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=IDS)
def test_window_edge(mode):
    r, ref = zl.reference("window_edge", mode)
    H = r.n_hosts
    assert H == 3 * zl.PASS + 1
    _common("window_edge", r, ref)
    own = np.nonzero(np.isin(r.zone, [0, 1, 2]))[0]
    assert own.tolist() == list(range(7168, 8201))
    assert own[zl.ZW_M - 1] == zl.PASS - 1      # the window's last slot is the pass's last host
    assert np.bincount(r.zone, minlength=zl.Z)[:3].tolist() == [345, 344, 344]
    assert (r.zone == zl.FAR).sum() == H - 1033
    p, z = _by_anchor(r, ref, 1)
    assert z.all() and p.tolist() == list(range(7168, 8198))
    assert len(p) > zl.ZW_M
    pf, zf = _by_anchor(r, ref, zl.FAR)
    assert zf.all() and pf.tolist() == list(range(30))


@pytest.mark.parametrize("mode", MODES, ids=IDS)
def test_window_edge_big(mode):
    r, ref = zl.reference("window_edge_big", mode)
    assert r.n_hosts == 3 * zl.PASS + 1
    _common("window_edge_big", r, ref)
    own = np.nonzero(np.isin(r.zone, [3, 4, 5]))[0]
    assert own.tolist() == list(range(3081))
    assert np.bincount(r.zone, minlength=zl.Z)[3:6].tolist() == [1027, 1027, 1027]
    assert np.bincount(r.task_group).tolist() == [1000, 1000, 1075, 30]
    assert r.n_tasks <= r.n_groups * 1024           # (MAX_WINDOW: the round runs group epochs)
    parts = [_by_anchor(r, ref, a) for a in (3, 4, 5)]
    chain = np.concatenate([p for p, _ in parts])
    assert all(z.all() for _, z in parts) and chain.tolist() == list(range(3075))
    assert len(chain) > zl.ZW_MBIG


# ---- blocks --------------------------------------------------------------------------------------
def _check_blocks(name, r, ref, H, desc, m):
    assert r.n_hosts == H
    blk = np.arange(H) * zl.Z // H
    narrow = (zl.Z - 1 - blk) if desc else blk
    assert np.array_equal(r.zone, m[narrow])
    hist = np.bincount(narrow, minlength=zl.Z)
    assert hist.min() >= H // zl.Z and hist.max() <= H // zl.Z + 1
    assert (np.diff(r.zone) != 0).sum() == zl.Z - 1          # 20 contiguous blocks
    counts = dict(zl.block_counts(H))
    got = {int(a): int((r.task_group == g).sum()) for g, a in enumerate(r.group_anchor)}
    assert got == {int(m[z]): n for z, n in counts.items()}
    first = np.random.RandomState(2).permutation(
        np.concatenate([np.full(n, z) for z, n in zl.block_counts(H)]))
    seen = list(dict.fromkeys(m[first].tolist()))
    assert r.group_anchor.tolist() == seen
    return counts


@pytest.mark.parametrize("name", ["blocks", "blocks_desc", "wide_blocks"])
@pytest.mark.parametrize("mode", MODES, ids=IDS)
def test_blocks(name, mode):
    r, ref = zl.reference(name, mode)
    desc, wide = name == "blocks_desc", name == "wide_blocks"
    m = zl.wide_map() if wide else np.arange(zl.Z)
    H = zl.BLOCKS_H
    _common(name, r, ref)
    _check_blocks(name, r, ref, H, desc, m)
    comp = lambda z: np.nonzero(np.isin(r.zone, m[zl.component_of(zl._round(zl.BF, 8, 1, 1).cost, z)]))[0]
    p0, z0 = _by_anchor(r, ref, m[0])
    p7, z7 = _by_anchor(r, ref, m[7])
    p17, z17 = _by_anchor(r, ref, m[17])
    c0, c7, c17 = comp(0), comp(7), comp(17)
    assert len(c7) == 1229 and z7.sum() == 1229 and (~z7).sum() == 71
    assert sorted(p7[z7].tolist()) == c7.tolist() and p7[z7].tolist() == c7.tolist()
    assert z0.all() and z17.all()
    if not desc:
        # a dense first pass: the window overflows in the middle of row 0 of either instantiation
        assert c0[0] == 0 and len(c0) > zl.ZW_M and c0[-1] < zl.ROW_ORDER
        assert p0.tolist() == list(range(1100))
        assert c17[0] == 9833 and c17[0] >= zl.PASS                 # an empty pass 0
        assert p17.tolist() == list(range(9833, 9833 + 700))
        assert c7[0] == 3688 and c7[-1] < zl.PASS
    else:
        assert c0[0] == 10448 and c0[0] >= zl.PASS                  # an empty pass 0
        assert p0.tolist() == list(range(10448, 10448 + 1100))
        assert c17[0] == 615 and p17.tolist() == list(range(615, 615 + 700))
        assert c7[0] == 7375 and c7[0] < zl.PASS <= c7[-1] == 8603  # across the pass boundary
    # the 71 spilled tasks pay at least the smallest positive cost
    t = ref.order[r.task_group[ref.order] == int(np.nonzero(r.group_anchor == m[7])[0][0])][~z7]
    zt = r.zone[ref.placement[t]]
    assert (r.cost[m[7], zt] + r.cost[zt, m[7]] >= 0.02).all()


# ---- skew ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=IDS)
def test_skew(mode):
    r, ref = zl.reference("skew", mode)
    assert r.n_hosts == 20003 and r.n_tasks == 1500
    _common("skew", r, ref, placed_share=0.9)
    hist = np.sort(np.bincount(r.zone, minlength=zl.Z))[::-1]
    assert hist.min() > 0 and 12000 < hist[0] < 13000 and 2800 < hist[1] < 3400 and hist[-1] < 40
    ideal = 20003 / np.arange(1, zl.Z + 1) ** 2 / (1.0 / np.arange(1, zl.Z + 1) ** 2).sum()
    assert (np.abs(hist - ideal) <= 4 * np.sqrt(ideal) + 1).all()
    assert (r.avail[0] == zl.one_task_cap(mode)[0]).all() and (r.avail[1] == 50000.0).all()
    zc, placed = zl.zero_cost(r, ref), ref.placement >= 0
    mixed = whole = 0
    for g in range(r.n_groups):
        t = r.task_group == g
        mixed += 0 < zc[t].sum() < placed[t].sum()
        whole += zc[t].all()
    assert mixed >= 1 and whole >= 1, (mixed, whole)


# ---- tail ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [9003, zl.RESIDENT_H])
@pytest.mark.parametrize("mode", MODES, ids=IDS)
def test_tail(mode, H):
    if H == 9003:
        r, ref = zl.reference("tail", mode)
        _common("tail", r, ref)
        assert H - zl.TAIL_N > zl.PASS              # a whole pass without a hit for 17 anchors
        assert (H - zl.TAIL_N) % 4 != 0             # the tail starts inside a quad
    else:
        r, ref = zl.resident_reference("tail", mode)
        assert r.n_hosts % 4 == 1 and (ref.placement >= 0).all()
    assert r.n_hosts == H and r.n_tasks == 600
    hist = np.bincount(r.zone, minlength=zl.Z)
    assert hist[5] == H - zl.TAIL_N and sorted(np.delete(hist, 5).tolist()) == [1] + [2] * 18
    assert (r.zone[:H - zl.TAIL_N] == 5).all() and (r.zone[H - zl.TAIL_N:] != 5).all()
    zc = zl.zero_cost(r, ref)
    assert sorted(r.group_anchor.tolist()) == list(range(zl.Z))
    per_host = np.bincount(ref.placement, minlength=H)
    full = 0
    for c in zl.components(r.cost):
        if 5 in c:
            continue
        own = np.nonzero(np.isin(r.zone, c))[0]
        assert 1 <= len(own) <= 6 and own.min() >= H - zl.TAIL_N
        assert (per_host[own] > 0).all()            # each of them is used
        t = np.isin(r.group_anchor[r.task_group], c) & zc
        used = sorted(set(ref.placement[t].tolist()))
        assert set(used) <= set(own.tolist())
        full += used == own.tolist()
    # ... and by a group of its own component, unless another group's spill filled it first (the
    # reference: all 7 components under best-fit at 9003 hosts, 5 or 6 otherwise)
    assert full >= (7 if (H, mode) == (9003, zl.BF) else 5), full
    last = np.arange(H & ~3, H)                     # the partial last quad: every host is used
    assert 1 <= len(last) <= 3 and np.isin(last, ref.placement[zc]).all()
    assert 0.2 < zc.mean() < 0.6                    # and most groups spill


# ---- empty_zones ---------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=IDS)
def test_empty_zones(mode):
    r, ref = zl.reference("empty_zones", mode)
    assert r.n_hosts == 9001
    _common("empty_zones", r, ref)
    hist = np.bincount(r.zone, minlength=zl.Z)
    assert (hist[1::2] == 0).all() and hist[0] == 901 and (hist[2::2] == 900).all()
    assert sorted(r.group_anchor.tolist()) == list(range(zl.Z))
    zc = zl.zero_cost(r, ref)
    # an empty anchor zone in a component that has hosts: placed at zero cost in the neighbours
    for a in (1, 3, 5, 7, 9, 11, 13, 15, 17):
        p, z = _by_anchor(r, ref, a)
        assert hist[a] == 0 and z.all() and np.isin(r.zone[p], zl.component_of(r.cost, a)).all()
    # zone 19 is a component of its own: nothing at zero cost
    p, z = _by_anchor(r, ref, 19)
    assert len(p) > 0 and not z.any() and (p >= 0).all()


@pytest.mark.parametrize("mode", MODES, ids=IDS)
def test_empty_zones_one(mode):
    r, ref = zl.reference("empty_zones_one", mode)
    assert r.n_hosts == 9001
    _common("empty_zones_one", r, ref)
    assert np.bincount(r.zone, minlength=zl.Z).tolist() == [0] * 5 + [9001] + [0] * 14
    assert sorted(r.group_anchor.tolist()) == list(range(zl.Z))
    empty = 0
    for a in range(zl.Z):
        p, z = _by_anchor(r, ref, a)
        assert (p >= 0).all() and z.all() == (a in (3, 4, 5)) and z.any() == (a in (3, 4, 5))
        empty += a not in (3, 4, 5)
    assert empty == 17                               # 17 groups whose whole component is empty


# ---- the resident sizes --------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(zl.RESIDENT))
@pytest.mark.parametrize("mode", MODES, ids=IDS)
def test_resident_sizes(name, mode):
    from pivot_place import _abi
    r, ref = zl.resident_reference(name, mode)
    wide = name == "wide_blocks"
    assert r.n_hosts == (zl.WIDE_RESIDENT_H if wide else zl.RESIDENT_H)
    assert r.n_hosts <= (_abi.PVT_RESIDENT_WIDE_MAX_HOSTS if wide else _abi.PVT_RESIDENT_MAX_HOSTS)
    assert r.n_hosts % 4 == 1 and r.n_tasks <= 1500
    assert (ref.placement >= 0).mean() >= (0.9 if name == "skew" else 1.0)
    zc = zl.zero_cost(r, ref).mean()
    assert zc < 1.0                                  # every one of them spills somewhere
    if name in ("blocks", "wide_blocks"):
        m = zl.wide_map() if wide else np.arange(zl.Z)
        counts = _check_blocks(name, r, ref, r.n_hosts, False, m)
        p0, z0 = _by_anchor(r, ref, m[0])
        assert z0.all() and p0.tolist() == list(range(counts[0]))
        p7, z7 = _by_anchor(r, ref, m[7])
        assert 0 < (~z7).sum() < len(p7)
