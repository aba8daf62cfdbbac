"""CPU checks of tests/grouping_cases.py, the reference and the rounds of test_gpu_grouping.py:
``group_reference`` reproduces the grouping of every recorded cost_aware run, numpy's
``choice`` is the ``randint`` the reference restates, and every case can tell a wrong grouping
from a right one (a moved anchor moves a placement, swapped group numbers change the order)."""
import numpy as np
import pytest

import fakes
import golden_io
import grouping_cases as gc
from oracle import oracle
from pivot_place import policies


def _recorded_runs():
    out = []
    for name, idx in golden_io.all_runs(skip_errors=False):
        run = golden_io.load(name)["runs"][idx]
        if run["policy"] == "cost_aware" and "groups" in run:
            out.append((name, idx))
    return out


@pytest.mark.parametrize("name,idx", _recorded_runs())
def test_group_reference_reproduces_recorded_runs(name, idx):
    """Partition, group order, anchor zones and the RandomState after the draws of every golden
    cost_aware run that records ``groups``. The only errors recorded are the TypeError of
    best-fit with host_decay, which the reference raises while it places its first group, after
    the grouping (cost_aware.py:36-42): such a run records that one group, which must be the
    reference's first, and the grouping itself must return no error. A run that recorded a
    grouping error (AttributeError) would have to return that type."""
    case = golden_io.load(name)
    run = case["runs"][idx]
    cluster, tasks = fakes.build(case)
    sched = policies.CostAwareGlobalScheduler(None, cluster, seed=run["seed"], **run["kwargs"])
    tab = sched._tables()
    items, item_of, off, lst = sched._items(tasks)
    apps = {}
    item_app = [apps.setdefault(id(c.application), len(apps)) for c in items]
    storage_zone, zone_storage = tab.storage_tables(cluster)
    got = gc.group_reference(np.array(item_of, dtype=np.int32), np.array(off, dtype=np.int64),
                             np.array(lst, dtype=np.int32), np.array(item_app, dtype=np.int32),
                             storage_zone, zone_storage, tab.zone,
                             golden_io.mt_state(run["seed"]), n_apps=len(apps))
    if run["error"] == "AttributeError":
        assert type(got).__name__ == run["error"]
        return
    assert run["error"] in (None, "TypeError")
    task_group, group_anchor, G, mt_after = got
    rec = run["groups"]
    if run["error"] is None:
        assert G == len(rec)
        assert np.array_equal(mt_after, golden_io.mt_state(run["seed"], run["rng_draws"]))
    else:
        assert len(rec) == 1 and G >= 1
    for g, grp in enumerate(rec):
        assert sorted(grp["tasks"]) == np.nonzero(task_group == g)[0].tolist()
        assert grp["anchor_zone"] == group_anchor[g]


@pytest.mark.parametrize("S,draws", [(37, 2000), (1, 2000)])
def test_choice_is_randint(S, draws):
    """RandomState.choice(list of objects) and randint(0, len): the same indices and the same
    final state; with one element no draw is made."""
    objs = [object() for _ in range(S)]
    a, b = np.random.RandomState(9), np.random.RandomState(9)
    ia = [objs.index(a.choice(objs)) for _ in range(draws)]
    ib = [int(b.randint(0, S)) for _ in range(draws)]
    assert ia == ib

    def same(x, y):
        return x[0] == y[0] and np.array_equal(x[1], y[1]) and x[2:] == y[2:]

    assert same(a.get_state(), b.get_state())
    assert same(a.get_state(), np.random.RandomState(9).get_state()) == (S == 1)


@pytest.mark.parametrize("pos", gc.POSITIONS)
def test_positions_are_what_they_say(pos):
    st = gc.mt_at(5, pos)
    assert st[624] == pos
    want = np.random.RandomState(5)
    skip = 0 if pos == 624 else pos
    for _ in range(skip):
        want.randint(0, 1 << 32, dtype=np.uint32)
    rs = np.random.RandomState(0)
    rs.set_state(("MT19937", st[:624], int(st[624]), 0, 0.0))
    assert [int(rs.randint(0, 1 << 32, dtype=np.uint32)) for _ in range(700)] == \
        [int(want.randint(0, 1 << 32, dtype=np.uint32)) for _ in range(700)]


def test_cases_reach_the_edges_they_name():
    cs = gc.cases()
    for T in gc.TASK_COUNTS + gc.BIG_TASK_COUNTS:
        assert cs["tasks_%d" % T].r.n_tasks == T
    for name, c in cs.items():
        assert c.r.n_hosts <= 300 or name == "hosts_5000", name
        assert c.r.n_tasks <= 16384 and len(c.storage_zone) + c.n_apps <= 8192, name
        assert (c.r.cost.diagonal() == 0).all() and (c.r.cost + c.r.cost.T)[~np.eye(c.r.n_zones, dtype=bool)].min() > 0
        assert c.r.bw.min() > 0
        tg, ga, G, mt, ref = gc.expected(name)
        assert (ref.placement >= 0).all(), name            # every task is placed
        # ... in its group's anchor zone: the anchor decides the placement
        assert np.array_equal(c.r.zone[ref.placement], ga[tg]), name
    assert cs["hosts_5000"].r.n_hosts == 5000
    for name in ("all_apps_4096", "all_apps_8191"):
        assert gc.expected(name)[2] == cs[name].r.n_tasks
    assert len(cs["all_apps_8191"].storage_zone) + cs["all_apps_8191"].n_apps == 8192
    assert len(cs["keys_8192"].storage_zone) + cs["keys_8192"].n_apps == 8192
    assert gc.expected("one_group")[2] == 1
    # with one storage no draw is made
    for name in ("storages_1", "all_apps_8191"):
        assert np.array_equal(gc.expected(name)[3], cs[name].mt_state)
    # the twist runs inside the draws of one round
    c = cs["twist"]
    assert gc.expected("twist")[2] == 700 > 624 and len(c.storage_zone) == 33
    # application bits: every other group, and one full word
    tg, ga, G, _, _ = gc.expected("sparse_words")
    first = [int(cs["sparse_words"].task_item[np.nonzero(tg == g)[0][0]]) for g in range(64)]
    app = [cs["sparse_words"].pred_off[i] == cs["sparse_words"].pred_off[i + 1] for i in first]
    assert app == [False, True] * 32
    c = cs["full_word"]
    tg = gc.expected("full_word")[0]
    first = [int(c.task_item[np.nonzero(tg == g)[0][0]]) for g in range(33)]
    assert [c.pred_off[i] == c.pred_off[i + 1] for i in first] == [True] * 32 + [False]
    # deferred lists (more than 1024 entries): three in one round, and in a second round
    for name, n in (("lists", 3), ("lists_b", 3)):
        assert (np.diff(cs[name].pred_off) > 1024).sum() >= n
    assert sorted(np.diff(cs["lists"].pred_off)[np.diff(cs["lists"].pred_off) >= 64].tolist()) == \
        sorted(gc.LIST_LENGTHS)
    assert cs["zones_40"].r.n_zones == 40


@pytest.mark.parametrize("name", ["chunk_last", "chunk_first", "lanes_0_63", "last_wave",
                                  "reused_key"])
def test_new_keys_fall_where_the_case_says(name):
    """The first tasks of the groups, against the pass sizes of the fused instance (256 tasks)
    and of the single and staged kernels (1024)."""
    c = gc.case(name)
    tg, _, G, _, _ = gc.expected(name)
    firsts = np.array([np.nonzero(tg == g)[0][0] for g in range(G)])
    assert firsts[0] == 0 and (np.diff(firsts) > 0).all()
    new = firsts[1:]
    for chunk in (gc.CHUNK_FUSED, gc.CHUNK_SINGLE):
        later = new[new >= chunk]
        assert len(later), "no key first seen past the first pass of %d" % chunk
        if name == "chunk_last":
            assert ((later + 1) % chunk == 0).any()
        if name == "chunk_first":
            assert (later % chunk == 0).any()
        if name == "lanes_0_63":
            assert (later % 64 == 0).any() and (later % 64 == 63).any()
        if name == "last_wave":
            assert (later % chunk >= chunk - 64).any()
        # group 0's key comes back in every pass
        assert all((tg[k:k + chunk] == 0).any() for k in range(0, c.r.n_tasks, chunk))
    if name == "reused_key":
        g = tg[3]
        assert g > 0 and all((tg[k:k + 256] == g).any() for k in range(0, c.r.n_tasks, 256))


def _instances(name):
    """The groups whose anchor the sensitivity test moves: all of a case up to 1100 tasks, 64
    picked with a fixed seed of a larger one."""
    G = gc.expected(name)[2]
    if gc.case(name).r.n_tasks <= 1100 or G <= 64:
        return list(range(G))
    return sorted(np.random.RandomState(1).choice(G, 64, replace=False).tolist())


def test_a_moved_anchor_moves_a_placement():
    """Every instance: one group's anchor moved to another storage zone (with a single storage:
    to the cluster's other zone) gives another placement. None is left out."""
    tried = same = 0
    for name, c in gc.cases().items():
        tg, ga, G, _, ref = gc.expected(name)
        for g in _instances(name):
            moved = ga.copy()
            moved[g] = gc.other_zone(c, int(ga[g]), g)
            assert moved[g] != ga[g]
            res = oracle.place(c.completed(tg, moved))
            tried += 1
            if np.array_equal(res.placement, ref.placement):
                same += 1
                print("not told apart:", name, "group", g)
    print("instances:", tried, "left out: 0, not told apart:", same)
    assert tried > 0 and same == 0


def test_swapped_adjacent_groups_change_the_order():
    for name, c in gc.cases().items():
        tg, ga, G, _, ref = gc.expected(name)
        if G < 2:
            continue
        for g in sorted({0, G // 2 - 1 if G >= 4 else 0, G - 2}):
            sw = tg.copy()
            sw[tg == g], sw[tg == g + 1] = g + 1, g
            gs = ga.copy()
            gs[g], gs[g + 1] = ga[g + 1], ga[g]
            res = oracle.place(c.completed(sw, gs))
            assert not np.array_equal(res.order, ref.order), (name, g)


@pytest.mark.parametrize("at", [gc.ERROR_T - 1, 0])
@pytest.mark.parametrize("kind", gc.ERROR_KINDS)
def test_error_cases_raise_in_the_reference(kind, at):
    c, exc, pattern = gc.error_case(kind, at)
    got = c.groups()
    assert type(got) is exc and pattern in str(got)
    assert isinstance(gc.error_base().groups(), tuple)
