"""GPU parity of cost_aware rounds on irregular host-zone layouts (zone_layout_cases.py;
test_zone_layout_cases.py shows on the CPU that the reference's placements touch the boundary hosts
each case aims at). The truth is ``oracle.place(r)``: placement, order and final availability are
compared bit for bit on every cost_aware path -- the windowed engine with the frontier walk, with
the lists alone, with sequential groups, with short list windows, the resident kernels, host-sharded
rounds over uneven ranges, a zone array that is not 16-byte aligned, decay and realtime bandwidths.

Every synthetic round elsewhere in the suite has zone[h] = h % Z, so the window compaction
(csrc/pvt_zwin_dev.h) never saw a dense pass, an empty pass, a window that fills inside row 0 or on
the last host of a pass, a hit in the partial last quad or a range that starts inside a quad.
"""
import functools

import numpy as np
import pytest

import zone_layout_cases as zl
from oracle import oracle
from pivot_place import _abi

pytestmark = pytest.mark.gpu

BF, FF = zl.BF, zl.FF
VARIANTS = {"bf": (BF, True), "ff": (FF, True), "ff_unsorted": (FF, False)}
# cases whose chains the frontier walk must serve (plenty of zero-cost capacity behind the
# boundaries they aim at); tail and the empty_zones cases are checked for parity alone
WALKED = ("planted", "window_edge", "window_edge_big", "blocks", "blocks_desc", "wide_blocks",
          "wide_planted")
PATHS = ("windowed", "lists", "sequential", "short", "short_unpipelined")


def _same(res, ref):
    np.testing.assert_array_equal(res.placement, ref.placement)
    np.testing.assert_array_equal(res.order, ref.order)
    bad = np.nonzero((res.avail != ref.avail).any(axis=0))[0]
    assert bad.size == 0, "availability differs on hosts %s" % bad[:10]


# best-fit: every chain fits its window's hosts (176 tasks on the 11 x 16 places of A or B, the
# partial last quad among them): a window that lacked one of them would hand its chain to the lists,
# which place it right -- parity alone would not see that
ALL_WALKED = ("planted", "wide_planted")


def _all_walked(st):
    assert st["epochs"] == 1 and st["frontier_chains"] == 3 and st["list_chains"] == 0 and \
        st["rejected"] == 0, st


def _case(name, variant):
    mode, sort_hosts = VARIANTS[variant]
    return zl.reference(name, mode, sort_hosts)


def _place(engine, r, path="windowed"):
    """The round on the windowed engine by the named path: (result, epoch statistics)."""
    try:
        engine.set_resident(0)
        if path == "lists":
            engine.set_zero_walk(False)
        elif path == "sequential":
            engine.set_epochs(False)
        elif path.startswith("short"):
            engine.set_window(96)
            engine.set_pipeline(path == "short")
        res = engine.place(r)
        st = engine.epoch_stats()
    finally:
        engine.set_pipeline(True)
        engine.set_window(0)
        engine.set_epochs(True)
        engine.set_zero_walk(True)
        engine.set_resident(_abi.PVT_RESIDENT_MAX_HOSTS)
    return res, st


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", zl.NAMES)
def test_windowed_engine(engine, name, variant, path):
    """Every case on the windowed engine: defaults (the frontier walk and its compaction), the
    lists alone, sequential groups, list windows of 96 tasks with the pipeline on and off.

    tail and the empty_zones cases assert parity alone. Observed ``frontier_chains`` /
    ``list_chains`` of the default path on the first run (best-fit; first-fit; first-fit unsorted):
    tail 7 / 75; 13 / 0; 1 / 0 -- empty_zones 7 / 7; 19 / 0; 1 / 0 -- empty_zones_one 2 / 72;
    4 / 0; 1 / 0."""
    r, ref = _case(name, variant)
    res, st = _place(engine, r, path)
    print(name, variant, path, st)
    _same(res, ref)
    if path == "windowed" and name in WALKED:
        assert st["frontier_chains"] > 0, st
    if path == "windowed" and variant == "bf" and name in ALL_WALKED:
        _all_walked(st)
    if path == "lists":
        assert st["frontier_chains"] == 0, st
    if path == "sequential":
        assert st["epochs"] == 0, st


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", list(zl.RESIDENT))
def test_resident_kernels(engine, name, variant):
    """The resident-sized variants (4093 hosts; 2045 on the 70-zone cluster) with the defaults."""
    mode, sort_hosts = VARIANTS[variant]
    r, ref = zl.resident_reference(name, mode, sort_hosts)
    assert engine.host_batch_fits(r) and r.n_hosts <= _abi.resident_max_hosts(r.n_zones)
    _same(engine.place(r), ref)
    _same(engine.place_batch([r, r])[1], ref)


# ---- host-sharded rounds over uneven ranges ------------------------------------------------------
@pytest.fixture(scope="module")
def engines():
    from pivot_place.engine import PlacementEngine
    return [PlacementEngine(0) for _ in range(5)]


def _lockstep(engines, r, bounds):
    """pivot_place.sharded.place_lockstep's loop with explicit ascending bounds: rank k owns hosts
    [bounds[k], bounds[k + 1])."""
    import torch
    from pivot_place.engine import DeviceRound
    world = len(bounds) - 1
    engines = engines[:world]
    drs = [DeviceRound(r, e.device) for e in engines]
    mx = [e.shard_begin(dr, bounds[k], bounds[k + 1], world)
          for k, (e, dr) in enumerate(zip(engines, drs))]
    sends = [torch.empty(max(m, 1), dtype=torch.uint8, device=e.device) for m, e in zip(mx, engines)]
    recvs = [torch.empty(max(m, 1) * world, dtype=torch.uint8, device=e.device)
             for m, e in zip(mx, engines)]
    while True:
        got = [e.shard_score(s) for e, s in zip(engines, sends)]
        assert len(set(got)) == 1, "shards disagree on the window: %s" % (got,)
        nt, nb = got[0]
        if nt == 0:
            break
        for recv in recvs:
            for k, s in enumerate(sends):
                recv[k * nb:(k + 1) * nb].copy_(s[:nb])
        ok = [e.shard_commit(recv) for e, recv in zip(engines, recvs)]
        assert len(set(ok)) == 1, "shards disagree on a stale window: %s" % (ok,)
    return [dr.result() for dr in drs]


def _bounds(name, which):
    H = 2 * zl.PASS + 3 if name == "planted" else zl.BLOCKS_H
    if name == "planted":
        # an empty rank, a cut inside the quad 8188..8191 (which holds hits), a three-host rank, a
        # last rank that is only the partial quad; and a one-host first rank
        return {"five": [0, 8190, 8190, 8193, H - 3, H], "one_host": [0, 1, H]}[which]
    # rank 0 holds all 1844 hosts of {0, 1, 2}: it fills ZW_M alone for the group anchored at 0
    # and ranks 1 to 3 hold no host of that component
    return [0, 1846, 3001, 9002, H]


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name,which", [("planted", "five"), ("planted", "one_host"),
                                        ("blocks", "rank0_fills")])
def test_host_sharded_uneven_ranges(engines, name, which, variant):
    """Explicit ascending ranges instead of place_lockstep's even split; every rank equals rank 0
    and rank 0 the reference.

    blocks, first-fit: the ranks disagree on the keyed order's shape. Rank 2 holds all 1229 hosts
    of {6, 7} (a zero-key prefix, the rest unsorted), the others hold none (a full sort). When the
    1300 tasks anchored at 7 run that prefix dry, the replicated walk places nothing; the ranks
    with a full sort used to fail there ("commit walk made no progress") while rank 2 sorted its
    rest -- with zone = h % Z every rank's prefix runs dry at once, so no test saw it."""
    r, ref = _case(name, variant)
    bounds = _bounds(name, which)
    assert bounds[0] == 0 and bounds[-1] == r.n_hosts and (np.diff(bounds) >= 0).all()
    if name == "blocks":
        own = np.nonzero(np.isin(r.zone, [0, 1, 2]))[0]
        assert own.max() < bounds[1] and len(own) >= zl.ZW_M and bounds[1] % 4 != 0
    outs = _lockstep(engines, r, bounds)
    st = engines[0].epoch_stats()
    print(name, which, variant, st)
    for o in outs[1:]:                      # every rank holds the same result
        _same(o, outs[0])
    _same(outs[0], ref)
    if variant == "bf":
        assert st["frontier_chains"] > 0, st


# ---- a zone array that is not 16-byte aligned ----------------------------------------------------
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", ["planted", "blocks", "wide_planted"])
def test_zone_pointer_that_is_not_16_byte_aligned(engine, name, variant):
    """zone four bytes past a 16-byte boundary: the compaction takes its element loads and must
    list the same hosts. (Checked by reading before the first run: in csrc/ only the guarded
    ``load`` of pvt_zwin_dev.h reads zone wider than four bytes -- no other kernel casts a zone
    pointer to a vector type.)"""
    import torch
    from pivot_place.engine import DeviceRound
    r, ref = _case(name, variant)
    H = r.n_hosts
    dr = DeviceRound(r, engine.device)
    buf = torch.zeros(H + 1, dtype=torch.int32, device=engine.device)
    assert buf.data_ptr() % 16 == 0
    buf[1:].copy_(torch.from_numpy(r.zone))
    dr.struct.zone = buf.data_ptr() + 4
    try:
        engine.set_resident(0)
        engine.run(dr)
        st = engine.epoch_stats()
    finally:
        engine.set_resident(_abi.PVT_RESIDENT_MAX_HOSTS)
    _same(dr.result(), ref)
    assert st["frontier_chains"] > 0, st
    if variant == "bf" and name in ALL_WALKED:
        _all_walked(st)
    del buf


# ---- decay and realtime bandwidths ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _decay_case(name, sort_hosts):
    r = zl.CASES[name](FF, sort_hosts).copy()
    r.decay = np.random.RandomState(3).randint(1, 6, r.n_hosts).astype(np.int32)
    return r, oracle.place(r, threads=4)


@pytest.mark.parametrize("sort_hosts", [True, False], ids=["ff", "ff_unsorted"])
@pytest.mark.parametrize("name", ["blocks", "skew"])
def test_with_decay(engine, name, sort_hosts):
    r, ref = _decay_case(name, sort_hosts)
    res, st = _place(engine, r)
    _same(res, ref)


@functools.lru_cache(maxsize=None)
def _rt_bw_case(variant):
    """The recipe of test_gpu_parity.test_realtime_bw_synthetic on the skewed layout."""
    mode, sort_hosts = VARIANTS[variant]
    r = zl.skew(mode, sort_hosts).copy()
    r.cost = r.cost + 0.001            # no free-egress zone: every score depends on the bandwidth
    rs = np.random.RandomState(41)
    bsum = r.bw + r.bw.T
    a = r.group_anchor
    r.rt_bw = (bsum[a][:, r.zone] / rs.randint(1, 4, size=(len(a), r.n_hosts))).astype(np.float64)
    return r, oracle.place(r, threads=4)


@pytest.mark.parametrize("epochs", [True, False], ids=["epochs", "sequential"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_with_realtime_bw(engine, variant, epochs):
    r, ref = _rt_bw_case(variant)
    res, st = _place(engine, r, "windowed" if epochs else "sequential")
    _same(res, ref)
