"""The long-run cases (long_run_cases.py) on the CPU reference alone: each really has the shape it
is named for -- the run's length, the batch offset of its first task and the hosts per window
chunk that can take a copy when it starts -- read from the oracle's order and the demand rows, so
that a later edit to synthetic.py or to a builder cannot silently make a case vacuous."""
import numpy as np
import pytest

import long_run_cases as lc


def _chain(r, ref):
    """The chain under test in processing order: tasks (caller indices) of every group but the last."""
    last = int(r.task_group.max())
    order = np.asarray(ref.order)
    return order[r.task_group[order] != last]


def _stretches(r, chain):
    """Maximal stretches of bit-identical demand rows inside a group, as (start, length)."""
    rows = np.ascontiguousarray(r.dem[:, chain].T).view(np.uint64)
    grp = r.task_group[chain]
    cut = np.ones(len(chain), dtype=bool)
    cut[1:] = (rows[1:] != rows[:-1]).any(axis=1) | (grp[1:] != grp[:-1])
    starts = np.nonzero(cut)[0]
    return list(zip(starts.tolist(), np.diff(np.append(starts, len(chain))).tolist()))


def _state_before(r, ref, chain, pos):
    """Availability after the chain's first `pos` commits (the other chain's hosts are disjoint)."""
    a = r.avail.copy()
    for t in chain[:pos]:
        a[:, ref.placement[t]] -= r.dem[:, t]
    return a


def _target(r, e, chain):
    """The first stretch of the case's row in its group."""
    row = np.array(e.row)
    for s, n in _stretches(r, chain):
        t = chain[s]
        if r.task_group[t] == e.group and (r.dem[:, t].view(np.uint64) == row.view(np.uint64)).all():
            return s, n
    raise AssertionError("no stretch of %s" % (e.row,))


@pytest.mark.parametrize("name", lc.NAMES)
def test_shape(name):
    r, e, ref = lc.reference(name)
    assert r.n_hosts == lc.H and r.n_tasks <= 702
    assert (ref.placement >= 0).all()
    # groups in order: segments of the chain are whole groups, the other chain's two tasks last
    assert (np.diff(r.task_group) >= 0).all() and r.group_anchor[-1] == lc.OTHER
    assert set(r.group_anchor[:-1].tolist()) <= set(lc.COMPONENT)
    assert (r.task_group == r.task_group.max()).sum() == 2
    c = np.asarray(r.cost, dtype=np.float64)
    z0 = (c + c.T) == 0.0
    for a in r.group_anchor[:-1]:
        assert set(np.nonzero(z0[int(a)])[0].tolist()) == set(lc.COMPONENT)
    assert not z0[lc.OTHER][list(lc.COMPONENT)].any()
    chain = _chain(r, ref)
    assert len(chain) == e.chain
    s, n = _target(r, e, chain)
    assert n == e.run, (s, n)
    assert s & 63 == e.offset, (s, n)
    w = lc.window(r)
    assert len(w) == 300
    a = _state_before(r, ref, chain, s)
    fits = (a[:, w] >= np.array(e.row)[:, None]).all(axis=0)
    got = tuple(int(fits[64 * k:64 * k + 64].sum()) for k in range(len(e.fit)))
    assert got == e.fit, got
    # every task of the chain lands in the window, the run in index order
    assert np.isin(ref.placement[chain], w).all()
    run_hosts = ref.placement[chain[s:s + n]]
    if min(e.row) >= 0:
        assert (np.diff(run_hosts) >= 0).all()
    if e.counts:
        assert tuple(int((run_hosts == h).sum()) for h in w[:len(e.counts)]) == e.counts


def test_lengths_and_offsets_cover_the_issue():
    got = {(lc.reference(k)[1].run, lc.reference(k)[1].offset) for k in lc.NAMES if "_at" in k}
    assert got == {(R, o) for R in (64, 65, 128, 129, 200) for o in (0, 1, 63)}


def test_cap_and_ring():
    rmax, logn = lc.walk_constant("ZW_RMAX"), lc.walk_constant("ZW_LOGN")
    assert rmax >= 192 and logn >= 64 + rmax and logn & (logn - 1) == 0
    assert lc.reference("over_the_cap")[1].run > rmax
    e = lc.reference("ring_wraps")[1]
    assert e.chain > logn and e.chain - e.run > logn           # wraps under singles, then under the run
    # a whole batch covered by one call: at least 64 tasks left after the rest of the first batch
    e = lc.reference("covers_batches")[1]
    assert e.run >= 200 and min(e.run, rmax) - (64 - e.offset) >= 128
    e = lc.reference("ends_on_batch_end")[1]
    assert (e.offset + e.run) % 64 == 0 and e.run <= rmax and e.run - (64 - e.offset) >= 64


def test_runout_cases():
    """Two copies a host: a chunk gives out after 128 tasks. Where the used hosts keep half a cpu
    and smaller tasks follow, chunk 0 can still take a task ahead (it stays the register chunk)."""
    for name, alive, chunks in (("runout_chunk_moves", False, 2), ("runout_on_pb", True, 2),
                                ("runout_on_lds", True, 3)):
        r, e, ref = lc.reference(name)
        chain = _chain(r, ref)
        s, n = _target(r, e, chain)
        w = lc.window(r)
        hosts = ref.placement[chain[s:s + n]]
        per_chunk = [int(np.isin(hosts, w[64 * k:64 * k + 64]).sum()) for k in range(4)]
        assert per_chunk[:2] == [128, 128 if n > 200 else n - 128], per_chunk
        assert sum(1 for x in per_chunk if x) == chunks, per_chunk
        assert all(int((hosts == h).sum()) == 2 for h in w[:64])
        after = _state_before(r, ref, chain, s + 128)
        ahead = r.dem[:, chain[s + n:]]
        can = ahead.size > 0 and (after[:, w[:64]] >= ahead.min(axis=1)[:, None]).all(axis=0).any()
        assert bool(can) == alive


def test_segment_case():
    r, e, ref = lc.reference("segment_inside_equal_rows")
    chain = _chain(r, ref)
    assert _stretches(r, chain) == [(0, 100), (100, 100)]
    assert (r.dem[:, chain] == r.dem[:, chain[:1]]).all()      # one row throughout
    assert r.group_anchor.tolist() == [0, 1, lc.OTHER]


def test_negative_case():
    r, e, ref = lc.reference("negative_component")
    assert min(e.row) < 0 and (r.dem[2, _chain(r, ref)] == -1.0).all()
