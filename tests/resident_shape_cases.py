"""Batches that pin every instance of the resident kernel (csrc/pvt_batch.hip), for
test_resident_shape_cases.py (CPU: each family still has the property it exists for, on the
reference) and test_gpu_resident_shapes.py (every instance equals the reference).

The kernel is compiled for 1, 2, 4 and 8 waves per round and 1 to 16 hosts per lane;
``resident_shape`` (csrc/pvt_kernels.h) picks the instance from the batch's largest round and the
preference PVT_RES_WAVES. ``expected_shape`` restates that rule, ``EDGES[pref]`` lists the largest
round sizes at which an instance begins or ends, and the families below are the rounds in which a
mistake in the wave count's share of the kernel -- the posts between the waves, the per-wave
lists and MT19937 copies, the reductions in front of the one-wave walks, the padding slots after
the last host -- changes a placement:

  plain     ``synthetic.make_round`` as it is
  tied      identical nearly full hosts: every comparison is a tie, so the winner is the lowest
            index, or (vbp best-fit) the lowest rank of a permutation whose consecutive ranks lie
            in different halves, quarters, ... of the hosts: in different waves, whatever the shape
  boundary  capacity only on the first and the last host of every wave, and on the last host
  runs      the demand edits 0, 3 and 4 of ``edit``: long runs, winners that run out, exact fits
  suffix    cost_aware best-fit rounds in which the zero-cost window's separation (DESIGN.md §2.3,
            certificate (ii)) fails only against a demand of a later 64-task block
  dry       every 7th task fits no host, and one round of the batch has no task

Every batch holds 6 or 7 rounds (``n=16``: for the rotating walker), the largest of ``H`` hosts,
one of a single host and one of ``H - 63``, with 130 to 300 tasks, never a multiple of 64.
``reference`` adds the CPU oracle's results, computed once per batch and shared; callers must not
modify them.
"""
import functools

import numpy as np

from oracle import oracle
from pivot_place import _abi, synthetic

CA_FF, CA_BF, OPP = _abi.PVT_CA_FF, _abi.PVT_CA_BF, _abi.PVT_OPP
VBP_FF, VBP_BF = _abi.PVT_VBP_FF, _abi.PVT_VBP_BF
# (name, mode, sort_hosts): the five policies, cost_aware first-fit both ways
POLICIES = (("ca_ff_keyed", CA_FF, True), ("ca_ff", CA_FF, False), ("ca_bf", CA_BF, True),
            ("opp", OPP, True), ("vbp_ff", VBP_FF, True), ("vbp_bf", VBP_BF, True))
POLICY = {name: (mode, sort_hosts) for name, mode, sort_hosts in POLICIES}
FAMILIES = ("plain", "tied", "boundary", "runs", "dry")

WAVE = 64
RW_MAXH = 1024          # csrc/pvt_kernels.h: the one-wave walks' limit
PREFS = (8, 2, 1, 4)
# the largest round of a batch: the last size of an instance (the last lane's last slot is a real
# host) or the first (the most padding slots); 2 and 1 fall back to four waves at their ends
EDGES = {8: (1, 65, 512, 513, 1024, 1025, 2048, 2049, 4096),
         2: (512, 513, 1024, 1025, 2048, 2049),
         1: (512, 513, 1024, 1025),
         4: (256, 257)}
SUFFIX_H = (600, 1024)


def expected_shape(pref, max_hosts):
    """(waves, hosts per lane) of a batch whose largest round has ``max_hosts`` hosts on an engine
    created under PVT_RES_WAVES=pref."""
    H = int(max_hosts)
    if pref == 8:
        waves = 8
    elif pref == 2 and 512 < H <= 2048:
        waves = 2
    elif pref == 1 and 512 < H <= 1024:
        waves = 1
    else:
        waves = 4
    hpl = 1
    while hpl * waves * WAVE < H:
        hpl *= 2
    return waves, hpl


def expected_switches(word, max_hosts):
    """PVT_RWALK=word as it takes effect in a batch whose largest round has ``max_hosts`` hosts (of
    at most 32 zones), in the documented bit values: 3 is 1, and no walk bit above RW_MAXH."""
    w = int(word)
    out = w & (16 | 32 | 64 | 0xff00)
    if max_hosts <= RW_MAXH and (w & 11):
        out |= (2 if w & 3 == 2 else 1 if w & 3 else 0) | (w & 8) | (w & 4)
    return out


def edit(r, rs, s):
    """The demand edit `s` of test_gpu_sticky_runs.test_sticky_runs_match_oracle on round r."""
    if s == 0:                               # two rows only: runs of hundreds of tasks
        rows = np.array([[0.5, 2048.0], [0.25, 1024.0]])
        pick = rs.randint(0, 2, size=r.n_tasks)
        r.dem[0], r.dem[1] = rows[pick, 0], rows[pick, 1]
    elif s == 1:                             # not exactly representable, tight hosts
        r.dem[0] = 0.1
        r.dem[1] = 0.3 * 1024.0
        r.avail[0] = 0.1 * rs.randint(1, 30, size=r.n_hosts) + 0.05 * (s % 2)
    elif s == 2:                             # all-zero rows between the others
        r.dem[:, ::3] = 0.0
    elif s == 3:                             # one row, few hosts: winners run out mid-run
        r.dem[0], r.dem[1] = 1.5, 3000.0
        r.avail[0] = np.minimum(r.avail[0], 4.5)
    elif s == 4:                             # exact fits (strict modes: the last copy fails)
        r.dem[0], r.dem[1] = 0.5, 2048.0
        r.avail[0] = 0.5 * rs.randint(0, 6, size=r.n_hosts)
        r.avail[1] = 2048.0 * rs.randint(0, 6, size=r.n_hosts)
    else:                                    # fewer distinct rows: longer runs
        r.dem[0] = np.round(r.dem[0] * 4) / 4
        r.dem[1] = np.round(r.dem[1] / 4096.0) * 4096.0


_TASKS = (130, 131, 200, 257, 300, 193, 150)


def sizes(H, n=7):
    """(hosts, tasks) of a batch's n rounds: the largest first and again later, one host, H - 63."""
    hs = (H, 1, max(1, H - 63), H, max(1, (H + 1) // 2), max(1, H - 1), H)
    return [(hs[i % 7], _TASKS[(i + i // 7) % 7]) for i in range(n)]


def _round(policy, H, T, seed):
    mode, sort_hosts = POLICY[policy]
    return synthetic.make_round(mode, H, T, seed=seed, sort_hosts=sort_hosts)


def alternating_ranks(H):
    """A rank per host, a permutation: the hosts in bit-reversed index order, so hosts of
    consecutive ranks lie on different sides of the largest power of two below H (a wave's first
    host in every shape with more than one wave of real hosts), of its half, and so on."""
    bits = max(1, (H - 1).bit_length())
    order = [int(format(i, "0%db" % bits)[::-1], 2) for i in range(1 << bits)]
    order = [h for h in order if h < H]
    rank = np.empty(H, dtype=np.uint32)
    rank[order] = np.arange(H, dtype=np.uint32)
    return rank


def boundary_slots(H, waves, hpl):
    """The first and the last host slot of every wave that holds real hosts, and the last host."""
    span = WAVE * hpl
    slots = {H - 1}
    for w in range(waves):
        if w * span < H:
            slots.update((w * span, min((w + 1) * span, H) - 1))
    return sorted(slots)


BOUNDARY_ROW = (1.0, 2048.0, 0.0, 0.0)
BOUNDARY_CAP = (2.5, 5120.0, 100.0, 1.0)     # two copies of the row under >= and under >


def plain(policy, H, n=7):
    return [_round(policy, h, t, 100 + i) for i, (h, t) in enumerate(sizes(H, n))]


def tied(policy, H, n=7):
    rounds = []
    for i, (h, t) in enumerate(sizes(H, n)):
        r = _round(policy, h, t, 200 + i)
        r.avail[0, :] = 1.0
        r.avail[1, :] = 40000.0
        r.avail[0, i::7] = 0.5
        if r.mode == VBP_BF:
            r.tiebreak = alternating_ranks(h)
        rounds.append(r)
    return rounds


def boundary(policy, H, shape, n=7):
    waves, hpl = shape
    rounds = []
    for i, (h, t) in enumerate(sizes(H, n)):
        r = _round(policy, h, t, 300 + i)
        for d in range(4):
            r.dem[d, :] = BOUNDARY_ROW[d]
        r.avail[0, :] = 0.0
        for s in boundary_slots(h, waves, hpl):
            r.avail[:, s] = BOUNDARY_CAP
        rounds.append(r)
    return rounds


def runs(policy, H, n=7):
    rounds = []
    for i, (h, t) in enumerate(sizes(H, n)):
        r = _round(policy, h, t, 400 + i)
        edit(r, np.random.RandomState(900 + i), (0, 3, 4)[i % 3])
        rounds.append(r)
    return rounds


DRY_CPUS = 1000.0       # above every host's (at most 16)


def dry(policy, H, n=7):
    rounds = []
    for i, (h, t) in enumerate(sizes(H, n)):
        r = _round(policy, h, 0 if i == 2 else t, 500 + i)
        r.dem[0, ::7] = DRY_CPUS
        rounds.append(r)
    return rounds


SUFFIX_BIG = (2.0, 4096.0, 100.0, 1.0)
SUFFIX_ROW = (1.0, 1024.0, 0.0, 0.0)


def suffix_round(H, T, pos, seed=1, a=0):
    """One group anchored in zone a; every task demands SUFFIX_ROW but the one at position
    ``pos`` (not in the first 64-task block), which demands SUFFIX_BIG. The lowest-index host
    outside a's zero-cost zones holds exactly SUFFIX_BIG (a score of 0 as an exact fit), every
    other outside host at least 2 cpus, and the window hosts below it 1.5 cpus: the outside hosts
    are separated from the first block's demands (2 - 1 cpus) but not from the round's."""
    r = synthetic.make_round(CA_BF, H, T, seed=seed, sort_tasks=False)
    r.task_group = np.zeros(T, dtype=np.int32)
    r.group_anchor = np.array([a], dtype=np.int32)
    for d in range(4):
        r.dem[d, :] = SUFFIX_ROW[d]
    r.dem[:, pos] = SUFFIX_BIG
    inside = (r.cost[a, r.zone] + r.cost[r.zone, a]) == 0.0
    out = int(np.nonzero(~inside)[0][0])
    r.avail[0, ~inside] = np.maximum(r.avail[0, ~inside], 2.0)
    r.avail[:, out] = SUFFIX_BIG
    r.avail[0, :out][inside[:out]] = 1.5
    return r


def suffix(H, n=6):
    """The suffix rounds: the big task in the second block (T = 130) and in the third (T = 200)."""
    # (hosts, tasks, the big task's position, seed, anchor zone)
    spec = ((H, 130, 70, 1, 0), (H, 200, 150, 1, 0), (H - 63, 130, 100, 2, 0), (H, 200, 190, 4, 3),
            (H, 257, 64, 5, 0), (H, 193, 191, 6, 7))
    rounds = [suffix_round(*spec[i % 6][:3], seed=spec[i % 6][3] + 10 * (i // 6), a=spec[i % 6][4])
              for i in range(n)]
    rounds.insert(3, synthetic.make_round(CA_BF, 1, 131, seed=3))
    return rounds


def suffix_facts(r):
    """What the suffix family rests on, recomputed in numpy for one of its rounds: (every zone is
    safe for the anchor, a dimension separates against block 0's maxima, one does against the
    round's, the big task's position, the lowest-index outside host, where a first fit over the
    window hosts alone puts the big task)."""
    a = int(r.group_anchor[0])
    c = r.cost[a] + r.cost[:, a]
    bw = r.bw[a] + r.bw[:, a]
    safe = bool(((bw > 0) & (bw <= 2.0 ** 300) & ((c == 0) | (c >= 2.0 ** -300))).all())
    inside = c[r.zone] == 0.0
    hmin = r.avail[:, ~inside].min(axis=1)
    sep0 = bool((hmin - r.dem[:, :64].max(axis=1) >= 2.0 ** -288).any())
    sep = bool((hmin - r.dem.max(axis=1) >= 2.0 ** -288).any())
    pos = int(np.argmax(r.dem[0]))
    av = r.avail[:, inside].copy()
    ids = np.nonzero(inside)[0]
    where = -1
    for t in range(pos + 1):
        fit = np.nonzero((av >= r.dem[:, t:t + 1]).all(axis=0))[0]
        if fit.size == 0:
            break
        av[:, fit[0]] -= r.dem[:, t]
        if t == pos:
            where = int(ids[fit[0]])
    return safe, sep0, sep, pos, int(np.nonzero(~inside)[0][0]), where


_BUILD = {"plain": plain, "tied": tied, "runs": runs, "dry": dry}


@functools.lru_cache(maxsize=None)
def reference(family, policy, H, shape=None, n=7):
    """(rounds, oracle results) of a family's batch. ``shape``: (waves, hosts per lane) for
    "boundary", None otherwise; "suffix" is cost_aware best-fit only."""
    if family == "suffix":
        assert policy == "ca_bf"
        rounds = suffix(H, n - 1)
    elif family == "boundary":
        rounds = boundary(policy, H, shape, n)
    else:
        rounds = _BUILD[family](policy, H, n)
    return rounds, [oracle.place(r) for r in rounds]
