"""Clusters of more than 32 zones, without a GPU: the synthetic wide zone tables meet the
engine's content rules, rounds of up to 31 zones are unchanged, the CPU restatement places a
round at the bound, and the bindings carry the bound."""
import hashlib

import numpy as np
import pytest

import wide_cases
from oracle import oracle
from pivot_place import _abi, checks, policies, synthetic


def _digest(r):
    h = hashlib.sha256()
    for name in ("avail", "zone", "dem", "cost", "bw", "task_group", "group_anchor", "tiebreak", "mt_state"):
        a = getattr(r, name, None)
        h.update(name.encode())
        if a is not None:
            a = np.ascontiguousarray(a)
            h.update(str(a.dtype).encode())
            h.update(str(a.shape).encode())
            h.update(a.tobytes())
    h.update(repr((r.mode, bool(r.sort_tasks), bool(r.sort_hosts))).encode())
    return h.hexdigest()


# make_round(mode, 300, 200, seed=5, n_zones=...) before wide zone tables existed
RECORDED = {
    (_abi.PVT_CA_FF, 20): "6ec567053b97f7877a93f28eb17dbc4d79eb362b775cc43a6b603ead5cf97c76",
    (_abi.PVT_CA_BF, 20): "ee068a471766bd090664217bd784100430fcee010c8a56eaaf148a85a5040b5b",
    (_abi.PVT_OPP, 20): "d4627aba240c8915e4fc28d26805c4238022444599af968fb0fcd0bf65f3124a",
    (_abi.PVT_VBP_FF, 20): "91e646b440e3cf431a56c80d3ca9796b86d2ce548f19cff227192f3e2673d925",
    (_abi.PVT_VBP_BF, 20): "0af75461764116f1747e040998dd4fdfe35cec7a981c12168d4de5175e5f675a",
    (_abi.PVT_CA_BF, 31): "f3b9fad04bac6f2f00c372287c4bcca10ff6612a9518e04a0f6621812541eeea",
}


@pytest.mark.parametrize("mode,Z", sorted(RECORDED))
def test_rounds_of_up_to_31_zones_are_unchanged(mode, Z):
    assert _digest(synthetic.make_round(mode, 300, 200, seed=5, n_zones=Z)) == RECORDED[(mode, Z)]


@pytest.mark.parametrize("Z", [32, 33, 64, 65, 512])
def test_wide_zone_tables_meet_the_content_rules(Z):
    cost, bw = synthetic.wide_zone_tables(Z, 7)
    assert cost.shape == bw.shape == (Z, Z) and cost.dtype == bw.dtype == np.float64
    r = synthetic.make_round(_abi.PVT_CA_BF, 2 * Z + 5, 50, seed=1, n_zones=Z)
    r.cost, r.bw = cost, bw
    rep = checks.check_arrays(r)                       # rules 6 and 7 among them
    assert rep.code == _abi.PVT_CHK_OK and rep.mask == 0
    csum = cost + cost.T
    off = ~np.eye(Z, dtype=bool)
    assert (np.diag(csum) == 0.0).all()                # the same zone
    assert (csum[off] == 0.0).any()                    # zones of one region
    assert (csum > 0.0).any() and (csum >= 0.0).all()
    assert ((bw + bw.T) > 0.0).all()
    for tab in (np.hstack([cost, bw]), bw):            # pairwise distinct rows
        assert len({row.tobytes() for row in tab}) == Z
    if Z > 31:                                         # cross-copy pairs are never free
        assert (csum[:31, 31:] > 0.0).all()


def test_wide_zone_tables_are_seeded_and_extend_the_base():
    a = synthetic.wide_zone_tables(70, 3)
    b = synthetic.wide_zone_tables(70, 3)
    c = synthetic.wide_zone_tables(70, 4)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(a[0], c[0]) and not np.array_equal(a[1], c[1])
    base_cost, _ = synthetic.zone_tables(0)
    assert np.array_equal(a[0][:31, :31], base_cost)
    assert np.array_equal(a[0][31:62, 31:62], base_cost)
    with pytest.raises(ValueError):
        synthetic.wide_zone_tables(_abi.PVT_MAX_ZONES + 1, 0)


def test_make_round_beyond_31_zones_has_that_many_zones():
    r = synthetic.make_round(_abi.PVT_CA_FF, 200, 300, seed=2, n_zones=40)
    assert r.n_zones == 40 and r.cost.shape == (40, 40)
    assert int(r.zone.max()) == 39 and int(r.group_anchor.max()) > 30
    assert checks.check_arrays(r).code == _abi.PVT_CHK_OK


@pytest.mark.parametrize("mode", wide_cases.ALL_MODES)
def test_oracle_places_a_contended_round_at_512_zones(mode):
    r, ref = wide_cases.case(mode, 512)               # (asserts the contention on the result)
    assert r.n_zones == _abi.PVT_MAX_ZONES == 512
    placed = ref.placement[ref.placement >= 0]
    assert placed.size and int(placed.max()) < r.n_hosts
    assert sorted(ref.order.tolist()) == list(range(r.n_tasks))
    assert (ref.avail >= 0).all() and (ref.avail <= r.avail).all()


@pytest.mark.parametrize("Z", [33, 64, 65, 512])
@pytest.mark.parametrize("size", ["small", "large"])
def test_contended_cases_hold_for_every_mode(Z, size):
    for mode in wide_cases.ALL_MODES:
        wide_cases.case(mode, Z, size)


def test_cluster_tables_at_40_zones():
    """The drop-in policies take Z = len(cluster.meta.zones) with no bound of their own."""
    cluster, tasks = wide_cases.dropin_cluster(40, 85, 30, 120, seed=9)
    tab = policies._ClusterTables(cluster)
    cost, bw = synthetic.wide_zone_tables(40, 9)
    assert tab.cost.shape == (40, 40) and np.array_equal(tab.cost, cost) and np.array_equal(tab.bw, bw)
    assert np.array_equal(tab.zone, np.arange(85) % 40)
    storage_zone, zone_storage = tab.storage_tables(cluster)
    assert np.array_equal(storage_zone, np.arange(40)) and np.array_equal(zone_storage, np.arange(40))


def test_bindings_carry_the_bound():
    assert _abi.PVT_MAX_ZONES == 512
    assert _abi.resident_max_hosts(32) == _abi.PVT_RESIDENT_MAX_HOSTS
    assert _abi.resident_max_hosts(33) == _abi.PVT_RESIDENT_WIDE_MAX_HOSTS == 2048


def test_library_exports_the_bound():
    from pivot_place import engine
    assert engine.max_zones() == 512                   # (loads the library; no GPU call)
