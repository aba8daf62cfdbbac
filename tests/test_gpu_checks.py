"""The device content check (csrc/pvt_check.hip; pvt_check_round, pvt_check_batch, pvt_set_checks)
against ``pivot_place.checks.check_arrays``, the numpy restatement of the rule table: every
report field equal, ``value`` bit for bit.

Rounds that break an INDEX rule (zone, task_group, group_anchor, tiebreak) go through
check / check_batch only, which never place; only value violations (rules 2, 3, 6, 7, 9) are sent
to placement calls, and only with the switch on, where the check must stop them."""
import ctypes
import re
import struct

import numpy as np
import pytest

import check_cases as cc
from oracle import oracle
from pivot_place import _abi, checks
from pivot_place.engine import DeviceBatch, DeviceRound

pytestmark = pytest.mark.gpu

HOSTS = (1, 63, 64, 65, 257, 1000, 70001)
TASKS = (0, 1, 300)
ZONES = (1, 20, 32)


def _bits(v):
    return struct.pack("<d", v)


def _same(dev, ref, what):
    assert (dev.code, dev.mask, dev.index, dev.count, _bits(dev.value)) == \
        (ref.code, ref.mask, ref.index, ref.count, _bits(ref.value)), "%s: device %r, numpy %r" % (what, dev, ref)


def _poke(t, i, value, dtype):
    """Store one element of a device tensor (bytes, so unsigned and -0.0 / NaN go in as they are)."""
    import torch
    raw = np.array([value]).astype(dtype).view(np.uint8)
    n = raw.size
    t.view(-1).view(torch.uint8)[i * n:(i + 1) * n].copy_(torch.from_numpy(raw.copy()))


class Planted:
    """r and its resident copy with one element replaced; both are restored on exit."""

    def __init__(self, r, dr, rule, index, value):
        self.host = getattr(r, cc.ARRAY[rule]).reshape(-1)
        self.dev = getattr(dr, cc.ARRAY[rule])
        self.i, self.value = index, value

    def __enter__(self):
        self.old = self.host[self.i].copy()
        self.host[self.i] = self.value
        _poke(self.dev, self.i, self.value, self.host.dtype)

    def __exit__(self, *exc):
        self.host[self.i] = self.old
        _poke(self.dev, self.i, self.old, self.host.dtype)


@pytest.mark.parametrize("mode", cc.MODES)
def test_clean_and_planted_rounds_match_numpy(engine, mode):
    """Every size at which the kernel changes shape (one lane, a wave's edge, a block's edge,
    several blocks, a grid that strides) x no / one / many tasks x 1, 20 and 32 zones: the clean
    round, then one offender of every rule its policy reads at index 0, at the last index and on
    both sides of element 256."""
    kind = 0
    for H in HOSTS:
        for T in TASKS:
            for Z in ZONES:
                what = "mode %d H=%d T=%d Z=%d" % (mode, H, T, Z)
                r = cc.clean_round(mode, H, T, Z)
                dr = DeviceRound(r, engine.device)
                ref = checks.check_arrays(r)
                assert ref.code == 0, what
                _same(engine.check(dr), ref, what)
                for rule in cc.applicable(r):
                    for i in cc.positions(cc.length(r, rule)):
                        kind += 1
                        v = cc.offender(r, rule, kind)
                        with Planted(r, dr, rule, i, v):
                            ref = checks.check_arrays(r)
                            assert ref.code == rule, (what, rule, i, v)
                            _same(engine.check(dr), ref, "%s rule %d at %d = %r" % (what, rule, i, v))
                _same(engine.check(dr), checks.check_arrays(r), what + " restored")


@pytest.mark.parametrize("mode", [_abi.PVT_CA_FF, _abi.PVT_VBP_BF])
def test_two_offenders_give_lowest_index_and_count(engine, mode):
    r = cc.clean_round(mode, 1000, 300, 20)
    dr = DeviceRound(r, engine.device)
    for rule in cc.applicable(r):
        n = cc.length(r, rule)
        i, j = n // 3, n - 2
        if rule == _abi.PVT_CHK_TIEBREAK:
            vi, vj = 1000, 1001          # two ranks out of range (duplicates: the test below)
        else:
            vi, vj = cc.offender(r, rule, 0), cc.offender(r, rule, 1)
        with Planted(r, dr, rule, j, vj), Planted(r, dr, rule, i, vi):
            ref = checks.check_arrays(r)
            assert ref.code == rule and ref.index <= i and ref.count >= 2, (rule, ref)
            if rule not in (_abi.PVT_CHK_COST, _abi.PVT_CHK_BW):
                assert (ref.index, ref.count) == (i, 2), (rule, ref)
            _same(engine.check(dr), ref, "rule %d at %d and %d" % (rule, i, j))


def test_tiebreak_duplicate_and_out_of_range(engine):
    for H in (2, 65, 1000, 70001):
        r = cc.clean_round(_abi.PVT_VBP_BF, H, 1, 20)
        dr = DeviceRound(r, engine.device)
        for i, j in ((0, H - 1), (H - 1, 0), (H // 2, H // 3)):
            if i == j:
                continue
            with Planted(r, dr, _abi.PVT_CHK_TIEBREAK, i, int(r.tiebreak[j])):   # a duplicate
                ref = checks.check_arrays(r)
                assert (ref.code, ref.index, ref.count) == (10, max(i, j), 1)
                _same(engine.check(dr), ref, "H=%d rank of %d also at %d" % (H, j, i))
        with Planted(r, dr, _abi.PVT_CHK_TIEBREAK, H // 2, H), \
                Planted(r, dr, _abi.PVT_CHK_TIEBREAK, 0, 0xffffffff):              # out of range
            ref = checks.check_arrays(r)
            assert (ref.code, ref.index, ref.count) == (10, 0, 2)
            _same(engine.check(dr), ref, "H=%d ranks out of range" % H)
    # three holders of one rank: every one but the first is counted
    r = cc.clean_round(_abi.PVT_VBP_BF, 1000, 1, 20)
    r.tiebreak[[900, 300]] = r.tiebreak[10]
    ref = checks.check_arrays(r)
    assert (ref.code, ref.index, ref.count) == (10, 300, 2)
    _same(engine.check(DeviceRound(r, engine.device)), ref, "three holders")


@pytest.mark.parametrize("mode", [_abi.PVT_CA_FF, _abi.PVT_CA_BF])
def test_rt_bw_rows_of_three_groups(engine, mode):
    H, G = 257, 3
    r = cc.grouped_round(mode, H, 40, 20, G)
    dr = DeviceRound(r, engine.device)
    _same(engine.check(dr), checks.check_arrays(r), "clean")
    for i, v in ((0, 0.0), (H, np.inf), (2 * H + 5, np.nan), (G * H - 1, -1.0), (256, -0.0)):
        with Planted(r, dr, _abi.PVT_CHK_RTBW, i, v):
            ref = checks.check_arrays(r)
            assert (ref.code, ref.index, ref.count) == (8, i, 1)
            _same(engine.check(dr), ref, "rt_bw[%d] = %r" % (i, v))
    with Planted(r, dr, _abi.PVT_CHK_GROUP, 7, G), Planted(r, dr, _abi.PVT_CHK_RTBW, 3, 0.0):
        ref = checks.check_arrays(r)
        assert ref.code == 4 and ref.mask == (1 << 4) | (1 << 8)
        _same(engine.check(dr), ref, "group and rt_bw")


def test_pointer_that_is_not_16_byte_aligned(engine):
    """The fp64 arrays are read 16 bytes at a time: an array that starts 8 bytes past a 16-byte
    boundary is read through the scalar head and tail, with the same indices."""
    import torch
    r = cc.clean_round(_abi.PVT_VBP_FF, 1000, 300, 20)
    dr = DeviceRound(r, engine.device)
    n = r.avail.size
    buf = torch.zeros(n + 1, dtype=torch.float64, device=engine.device)
    assert buf.data_ptr() % 16 == 0
    dr.struct.avail = buf.data_ptr() + 8
    for i in (0, 1, 255, 256, n - 2, n - 1):
        a = r.avail.copy()
        a.reshape(-1)[i] = -0.0
        buf[1:].copy_(torch.from_numpy(a.reshape(-1)))
        bad = r.copy()
        bad.avail = a
        ref = checks.check_arrays(bad)
        assert (ref.code, ref.index, ref.count) == (2, i, 1)
        _same(engine.check(dr), ref, "avail[%d] behind an odd pointer" % i)


def test_batch_reports_equal_single_rounds(engine):
    """Five rounds of mixed sizes and policies in one launch, two of them bad: one report per
    round, equal to the round's own check. The packed buffers leave the later rounds' zone tables
    and realtime rows 8 bytes off a 16-byte boundary."""
    rounds = [cc.clean_round(_abi.PVT_CA_BF, 63, 1, 1), cc.grouped_round(_abi.PVT_CA_FF, 257, 41, 20, 3),
              cc.clean_round(_abi.PVT_VBP_BF, 70001, 300, 20), cc.clean_round(_abi.PVT_OPP, 1, 0, 32),
              cc.grouped_round(_abi.PVT_CA_BF, 1001, 300, 32, 5)]
    rounds[1] = cc.plant(rounds[1], _abi.PVT_CHK_ANCHOR, 2, 20)
    rounds[4] = cc.plant(cc.plant(rounds[4], _abi.PVT_CHK_RTBW, 5 * 1001 - 1, 0.0), _abi.PVT_CHK_BW, 33, -1e9)
    refs = [checks.check_arrays(r) for r in rounds]
    assert [p.code for p in refs] == [0, 5, 0, 0, 7]
    got = engine.check_batch(DeviceBatch(rounds, engine.device))
    assert len(got) == 5
    for i, (r, g, ref) in enumerate(zip(rounds, got, refs)):
        _same(g, ref, "batch round %d" % i)
        _same(engine.check(DeviceRound(r, engine.device)), ref, "single round %d" % i)
    assert engine.check_batch(DeviceBatch([], engine.device)) == []


def test_mt_position_is_read_on_the_host(engine):
    r = cc.clean_round(_abi.PVT_OPP, 65, 1, 20)
    r.mt_state[624] = 625
    _same(engine.check(DeviceRound(r, engine.device)), checks.check_arrays(r), "mt pos 625")
    assert checks.check_arrays(r).code == 11


# ---------------------------------------------------------------- the switch
def _value_violations():
    """(rule, a round that violates only it by VALUE): rules 2, 3, 6, 7, 9."""
    bf = cc.clean_round(_abi.PVT_CA_BF, 500, 60, 20, rt_bw=False)
    ff = cc.clean_round(_abi.PVT_CA_FF, 500, 60, 20, rt_bw=False)
    return [(2, cc.plant(bf, _abi.PVT_CHK_AVAIL, 700, -0.0)),
            (3, cc.plant(bf, _abi.PVT_CHK_DEM, 61, np.nan)),
            (6, cc.plant(bf, _abi.PVT_CHK_COST, 45, -50.0)),
            (7, cc.plant(ff, _abi.PVT_CHK_BW, 21, -1e12)),
            (9, cc.plant(ff, _abi.PVT_CHK_DECAY, 499, 0))]


@pytest.fixture
def checked(engine):
    engine.set_checks(True)
    try:
        yield engine
    finally:
        engine.set_checks(False)
        engine.set_profiling(False)


def _snapshot(*tensors):
    return [t.cpu().numpy().copy().view(np.uint8) for t in tensors]


def test_switch_stops_value_violations_before_anything_is_placed(checked):
    engine = checked
    for rule, r in _value_violations():
        ref = checks.check_arrays(r)
        assert ref.code == rule
        text = r"rule %d \(%s\) at index %d, " % (rule, _abi.CHECK_NAMES[rule], ref.index)
        with pytest.raises(RuntimeError, match=text):
            engine.place(r)                               # host arrays (pvt_place_host*)
        dr = DeviceRound(r, engine.device)
        dr.placement.fill_(-7)
        dr.order.fill_(-9)
        before = _snapshot(dr.placement, dr.order, dr.avail)
        with pytest.raises(RuntimeError, match=text):
            engine.run(dr)                                # pvt_place
        for a, b in zip(before, _snapshot(dr.placement, dr.order, dr.avail)):
            assert np.array_equal(a, b), "rule %d: pvt_place wrote an output" % rule
        good = cc.clean_round(r.mode, 300, 20, 20, rt_bw=False)
        with pytest.raises(RuntimeError, match="round 1: check failed: " + text):
            engine.place_batch([good, r, good])
        b = DeviceBatch([good, r, good], engine.device)
        b.placement.fill_(-7)
        b.order.fill_(-9)
        before = _snapshot(b.placement, b.order, b.bufs["avail"])
        with pytest.raises(RuntimeError, match="round 1: check failed: " + text):
            engine.run_batch(b)                           # pvt_place_batch
        for a, c in zip(before, _snapshot(b.placement, b.order, b.bufs["avail"])):
            assert np.array_equal(a, c), "rule %d: pvt_place_batch wrote an output" % rule


@pytest.mark.parametrize("mode", cc.MODES)
def test_clean_rounds_place_as_before_with_the_switch_on(checked, mode):
    engine = checked
    for H in (700, 20000):                                 # resident kernel, windowed engine
        r = cc.clean_round(mode, H, 120, 20, rt_bw=False)
        ref = oracle.place(r)
        dr = DeviceRound(r, engine.device)
        engine.run(dr)
        for got in (dr.result(), engine.place(r)):
            assert np.array_equal(got.placement, ref.placement) and np.array_equal(got.order, ref.order)
            assert np.array_equal(got.avail, ref.avail)
    rounds = [cc.clean_round(mode, 400, 50 + s, 20, seed=s, rt_bw=False) for s in range(4)]
    for r, got in zip(rounds, engine.place_batch(rounds)):
        ref = oracle.place(r)
        assert np.array_equal(got.placement, ref.placement) and np.array_equal(got.avail, ref.avail)


def test_switch_guards_sharded_rounds(checked):
    """pvt_shard_begin checks first: a violating round starts no sharded round and writes no
    output; a clean one is placed as the oracle places it."""
    from pivot_place.sharded import place_lockstep
    engine = checked
    for mode in (_abi.PVT_CA_BF, _abi.PVT_VBP_BF, _abi.PVT_OPP):
        r = cc.clean_round(mode, 20000, 150, 20, rt_bw=False)
        got, ref = place_lockstep([engine], r)[0], oracle.place(r)
        assert np.array_equal(got.placement, ref.placement) and np.array_equal(got.order, ref.order)
        assert np.array_equal(got.avail, ref.avail)
        bad = cc.plant(r, _abi.PVT_CHK_DEM, 3, -0.0)
        dr = DeviceRound(bad, engine.device)
        dr.placement.fill_(-7)
        dr.order.fill_(-9)
        before = _snapshot(dr.placement, dr.order, dr.avail)
        with pytest.raises(RuntimeError, match=r"rule 3 \(dem\) at index 3, value -0 "):
            engine.shard_begin(dr, 0, bad.n_hosts, 1)
        for a, b in zip(before, _snapshot(dr.placement, dr.order, dr.avail)):
            assert np.array_equal(a, b), "mode %d: pvt_shard_begin wrote an output" % mode


def test_no_check_launch_unless_the_switch_is_on(engine, checked):
    engine.set_checks(False)
    engine.set_profiling(2)
    dr = DeviceRound(cc.clean_round(_abi.PVT_VBP_BF, 2000, 100, 20), engine.device)
    b = DeviceBatch([cc.clean_round(_abi.PVT_VBP_FF, 300, 40, 20, seed=s) for s in range(3)], engine.device)
    engine.reset_kstats()
    engine.run(dr)
    engine.run_batch(b)
    assert engine.kernel_kstats("check_kernel")["launches"] == 0
    assert engine.kernel_kstats("resident_kernel")["launches"] == 2
    engine.set_checks(True)
    dr.reset()
    b.reset()
    engine.reset_kstats()
    engine.run(dr)
    engine.run_batch(b)
    assert engine.kernel_kstats("check_kernel")["launches"] == 2
    assert engine.kernel_kstats("resident_kernel")["launches"] == 2


def test_host_round_verdict_equals_the_device_one(checked):
    engine = checked
    r = cc.plant(cc.clean_round(_abi.PVT_CA_BF, 5000, 50, 20, rt_bw=False), _abi.PVT_CHK_COST, 7 * 20 + 3, -3.5)
    res, rc = engine._place_host(r, None)                 # pvt_place_host itself
    assert rc == _abi.PVT_EINVAL
    m = re.search(r"rule (\d+) \((\w+)\) at index (\d+), value (\S+) \((\d+) violating",
                  engine.lib.pvt_last_error(engine.ctx).decode())
    assert m, engine.lib.pvt_last_error(engine.ctx)
    dev = engine.check(DeviceRound(r, engine.device))
    _same(dev, checks.check_arrays(r), "device")
    assert (int(m.group(1)), int(m.group(3)), int(m.group(5))) == (dev.code, dev.index, dev.count) == (6, 67, 2)
    assert _bits(float(m.group(4))) == _bits(dev.value)
    assert np.array_equal(res.avail, r.avail)             # outputs untouched
    # the host batch: every round its own result, nothing placed
    good = cc.clean_round(_abi.PVT_VBP_FF, 300, 20, 20)
    n = 3
    structs = (_abi.pvt_round * n)()
    keep = []
    for i, q in enumerate((good, r, good)):
        s, rr = engine._host_struct(q)
        structs[i] = s
        keep.append(rr)
    rcs = (ctypes.c_int32 * n)()
    items = (ctypes.POINTER(_abi.pvt_ca_items) * n)()
    assert engine.lib.pvt_place_host_batch(engine.ctx, structs, items, n, rcs) == _abi.PVT_EINVAL
    assert list(rcs) == [_abi.PVT_OK, _abi.PVT_EINVAL, _abi.PVT_OK]
    assert "host batch round 1: check failed: rule 6 (cost) at index 67" in engine.lib.pvt_last_error(engine.ctx).decode()
