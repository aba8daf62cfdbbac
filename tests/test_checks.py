"""Content checks without a device: the ABI additions (pvt_check_round, pvt_check_batch,
pvt_set_checks, pvt_check_report, enum pvt_check) agree with the header and reject NULL
arguments, and ``pivot_place.checks.check_arrays`` -- the numpy restatement of the rule table,
and the checker the device check is tested against (test_gpu_checks.py) -- passes every round
the project ships and names the right rule, index, count, value and mask on violating ones."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import check_cases as cc
import golden_io
from pivot_place import _abi, checks, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pivot_place.h")


def test_report_struct_and_enum_match_header():
    text = open(HEADER).read()
    body = re.search(r"typedef struct pvt_check_report \{(.*?)\} pvt_check_report;", text,
                     flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b(\w+);", body) == [f for f, _ in _abi.pvt_check_report._fields_]
    assert ctypes.sizeof(_abi.pvt_check_report) == 4 * 2 + 8 * 3
    assert _abi.pvt_check_report.index.offset == 8 and _abi.pvt_check_report.value.offset == 24
    enum = re.search(r"enum pvt_check \{(.*?)\};", text, flags=re.S).group(1)
    names = re.findall(r"(PVT_CHK_\w+)\s*=\s*(\d+)", enum)
    assert len(names) == 12
    for name, value in names:
        assert getattr(_abi, name) == int(value), name
    assert int(re.search(r"#define\s+PVT_ABI_VERSION\s+(\d+)", text).group(1)) == 3


def test_new_symbols_are_exported_and_reject_null():
    lib = engine.load_library()
    for name in ("pvt_check_round", "pvt_check_batch", "pvt_set_checks"):
        assert hasattr(lib, name), name
    rep = _abi.pvt_check_report()
    rnd = _abi.pvt_round()
    assert lib.pvt_check_round(None, ctypes.addressof(rnd), ctypes.byref(rep)) == _abi.PVT_EINVAL
    assert lib.pvt_check_round(None, None, None) == _abi.PVT_EINVAL
    assert lib.pvt_check_batch(None, ctypes.addressof(rnd), 1, ctypes.byref(rep)) == _abi.PVT_EINVAL
    assert lib.pvt_set_checks(None, 1) == _abi.PVT_EINVAL


def _clean(rep, what):
    assert rep == _abi.CheckReport(0, 0, -1, 0, 0.0), "%s: %r" % (what, rep)


@pytest.mark.parametrize("mode", cc.MODES)
def test_synthetic_rounds_are_clean(mode):
    for H, T, Z in ((1, 0, 1), (1, 1, 1), (65, 1, 20), (257, 300, 32), (1000, 300, 20)):
        _clean(checks.check_arrays(cc.clean_round(mode, H, T, Z)), "mode %d H=%d T=%d Z=%d" % (mode, H, T, Z))
    _clean(checks.check_arrays(cc.clean_round(mode, 2000, 300, 20, rt_bw=False)), "no rt_bw")


def test_golden_runs_are_clean():
    runs = golden_io.all_runs()
    assert runs
    for name, i in runs:
        case = golden_io.load(name)
        _clean(checks.check_arrays(golden_io.run_arrays(case, case["runs"][i])), "%s run %d" % (name, i))


@pytest.mark.parametrize("name", golden_io.sim_traces())
def test_sim_trace_rounds_are_clean(name):
    tr, cases = golden_io.sim_rounds(name)
    assert cases
    for k, case in enumerate(cases):
        for run in case["runs"]:
            _clean(checks.check_arrays(golden_io.run_arrays(case, run)), "%s round %d" % (name, k))


def _round_for(rule):
    mode = {_abi.PVT_CHK_DECAY: _abi.PVT_CA_FF, _abi.PVT_CHK_TIEBREAK: _abi.PVT_VBP_BF,
            _abi.PVT_CHK_MTPOS: _abi.PVT_OPP}.get(rule, _abi.PVT_CA_BF)
    return cc.clean_round(mode, 300, 40, 20)


def _same_value(a, b):
    return (math.isnan(a) and math.isnan(b)) or (a == b and math.copysign(1, a) == math.copysign(1, b))


@pytest.mark.parametrize("rule", range(1, 11))
def test_each_rule_is_reported(rule):
    r = _round_for(rule)
    n = cc.length(r, rule)
    i = n // 2 + 1
    for k in range(4):
        v = cc.offender(r, rule, k)
        rep = checks.check_arrays(cc.plant(r, rule, i, v))
        assert rep.code == rule and rep.mask == 1 << rule, (rule, k, rep)
        if rule in (_abi.PVT_CHK_COST, _abi.PVT_CHK_BW):
            a, z = divmod(i, r.n_zones)       # the pair (a, z) and its mirror both carry the sum
            tab = getattr(r, cc.ARRAY[rule])
            assert rep.index == min(i, z * r.n_zones + a) and rep.count == (1 if a == z else 2)
            assert _same_value(rep.value, float(v + tab[z, a]))
        else:
            assert rep.index == i and rep.count == 1, (rule, k, rep)
            assert _same_value(rep.value, float(np.array(v).astype(getattr(r, cc.ARRAY[rule]).dtype)))


def test_duplicate_rank_blames_the_later_host():
    r = _round_for(_abi.PVT_CHK_TIEBREAK)
    bad = r.copy()
    bad.tiebreak[200] = bad.tiebreak[7]
    rep = checks.check_arrays(bad)
    assert (rep.code, rep.index, rep.count, rep.value) == (10, 200, 1, float(r.tiebreak[7]))
    bad.tiebreak[3] = bad.tiebreak[7]         # now host 7 is the later holder too
    rep = checks.check_arrays(bad)
    assert (rep.code, rep.index, rep.count) == (10, 7, 2)


def test_mt_position_is_rule_11():
    r = _round_for(_abi.PVT_CHK_MTPOS)
    r.mt_state[624] = 624
    _clean(checks.check_arrays(r), "pos 624")
    r.mt_state[624] = 625
    assert checks.check_arrays(r) == _abi.CheckReport(11, 1 << 11, 624, 1, 625.0)


def test_lower_rule_wins_and_mask_has_both():
    r = _round_for(_abi.PVT_CHK_COST)
    bad = cc.plant(cc.plant(r, _abi.PVT_CHK_DEM, 5, np.nan), _abi.PVT_CHK_ZONE, 9, -1)
    bad = cc.plant(bad, _abi.PVT_CHK_ZONE, 4, 20)
    rep = checks.check_arrays(bad)
    assert rep == _abi.CheckReport(1, (1 << 1) | (1 << 3), 4, 2, 20.0)


def test_rules_apply_only_where_the_engine_reads():
    r = cc.clean_round(_abi.PVT_VBP_FF, 100, 0, 20)
    r.dem = np.full((4, 0), np.nan)
    r.cost = -np.ones((20, 20))               # vbp never reads the zone tables
    _clean(checks.check_arrays(r), "vbp_ff, no tasks")
    r = cc.clean_round(_abi.PVT_CA_BF, 100, 0, 20, rt_bw=False)
    r.cost = -np.ones((20, 20))               # cost_aware without tasks: rules 4-7 do not apply
    r.task_group = np.zeros(0, dtype=np.int32)
    r.group_anchor = np.array([99], dtype=np.int32)
    _clean(checks.check_arrays(r), "cost_aware, no tasks")
