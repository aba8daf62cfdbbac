// pvt_zwalk.hip — the zero-cost frontier walk of an epoch chain (cost_aware best-fit).
//
// A cost_aware best-fit task takes the host of minimum key (score, index), score =
// (c * ||avail - d||) / bw (scheduler/cost_aware.py:85-97). Hosts in a zone its anchor reaches
// at zero egress cost (csum = 0) score exactly +0, the smallest key, so while one of them fits,
// the winner is simply the LOWEST-INDEX fitting host of those zones. An epoch chain
// (pvt_epoch.hip) holds the groups anchored in one zero-cost component, whose tasks pile onto
// the first hosts of the component's zones (config 5: the 1500 tasks of the longest chain use
// fewer than 200 of them). This kernel walks such a chain without candidate lists:
//
//   window   the first ZW_M hosts, in index order, of the zones U = the union of the chain's
//            anchors' zero-cost zones, with their capacities at the epoch start, in LDS;
//   task     the first window host (index order) that fits and scores exactly 0 -- found 64
//            hosts per step by one wave (a ballot) -- is committed in LDS and logged (WinRec);
//
// exactly the host the sequential reference picks, given three certificates checked here
// (any failure: the chain is left to the list-based walk, which then runs for it):
//
//   (1) a winner exists in the window: every zero-cost host of lower index is in the window
//       (U contains the anchor's zero-cost zones; the window is U's index-order prefix);
//   (2) no host outside U scores 0: for every zone z outside U, c = csum[a][z] >= 2^-300 and
//       bw = bsum[a][z] <= 2^300, and some capacity dimension r separates hosts from tasks,
//       min_h avail[r][h] - max_t d[r] >= 2^-288 (so s2 >= fl(x_r^2) >= 2^-578 for every such
//       pair and the score is >= 2^-900 > 0 -- the same bound ca_score_bits uses); hosts outside
//       U are never committed to by this walk, so their epoch-start state is their state;
//   (3) zero-cost scores are exactly +0: bw > 0 for the anchor's zero-cost zones and every
//       window capacity and chain demand is finite with |x| <= 2^500 (s2 finite);
//
// and window hosts of U outside the anchor's zero-cost zones are scored exactly (ca_score_bits,
// a key of 0 only when the score's bits are 0). The log and the chain's progress have the
// format of the list walk's chain mode, so validation, finality and apply are unchanged.
//
// Optimistic apply (ZwalkArgs.undo, the driver's epoch tail): a chain that walked all its tasks
// holds each of its hosts' final state in its window and writes it to global availability
// itself; with every chain's report in the host's mapped words, an epoch whose chains all
// completed needs no kernel after this one. The prologue saves the window's start rows (ZwUndo)
// for the epochs the host does not accept whole; the fast prologue (FAST below: the round's first
// epoch, from the order launch's group certificates) saves nothing, its start rows are those of
// the prebuilt window it walks.
//
// FF: the same chain walk for cost_aware FIRST-fit with sort_hosts (scheduler/cost_aware.py:
// 99-127). A group's hosts are taken in the order of the frozen key c*df/(||avail||*bw); hosts
// of the anchor's zero-cost zones have key exactly 0 and lead that order in index order, so
// while one of them strictly fits, the winner is the lowest-index such host -- the same window,
// with strict fit, and fitting U hosts of other zones simply skipped (their key is > 0).
// Certificates: (1) as above; (2') every zone has c == 0 with bw > 0 (key exactly 0 for r > 0)
// or c >= 2^-300 with bw <= 2^300, and every host capacity is at most 2^298 (so r <= 2^299 and
// a positive key is >= 2^-899, never 0); (3') as (3), and the chain's demands are >= 0 (a host
// that strictly fits then has r > 0). Chains of different zero-cost components commit to
// disjoint hosts, none of which is zero-key for another component's anchors, so every chain's
// proven prefix is exact in the sequential order too (the driver's ff_epoch: no validation).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pivot_place.h"
#include "pvt_device.h"
#include "pvt_kernels.h"
#include "pvt_zwalk_stamps.h"
#include "pvt_zwin_dev.h"

namespace pvt {

constexpr int ZW_THREADS = 256;
constexpr int ZW_WAVES = ZW_THREADS / 64;
constexpr int ZW_SCAN = 8;                 // 16-byte zone loads (4 hosts) per thread per window-build pass
constexpr int ZW_MINB = ZW_MIN_PARTS;      // blocks of the host-minimum pass
constexpr int ZW_PR = 8;                   // chain task rows per thread per prologue pass

#ifndef PVT_ZW_UNROLL
#define PVT_ZW_UNROLL 8
#endif
constexpr int ZW_UNROLL = PVT_ZW_UNROLL;   // run_bulk pass 1: copies per stop check
constexpr int ZW_SB = 64;                  // suffix-minimum batches (the last one holds the rest)
constexpr int32_t ZW_SAME = -1;            // batch log, host entry: the host of the position before
#ifndef PVT_ZW_RMAX
#define PVT_ZW_RMAX 192
#endif
#ifndef PVT_ZW_RMIN
// the hot loop places a run through run_bulk from this many tasks on (2, 4 and 8 measured against
// each other: EXPERIMENTS.md, round 11)
#define PVT_ZW_RMIN 2
#endif
constexpr int ZW_RMAX = PVT_ZW_RMAX;       // tasks one run_bulk call places at the most (run lengths from the order launch)
constexpr int ZW_RMIN = PVT_ZW_RMIN;
constexpr int ZW_LOGN = 256;               // positions of the batch log's ring
static_assert((ZW_LOGN & (ZW_LOGN - 1)) == 0 && ZW_LOGN >= 64 + ZW_RMAX && ZW_RMAX >= 64 && ZW_RMIN >= 2,
              "a run from the current batch writes at most 64 + ZW_RMAX positions past the oldest unflushed one");
template <int WM>
struct ZwalkLDS {
  double wa[4][WM];                        // window capacities (live)
  int32_t wid[WM];                         // window hosts (ascending index)
  int32_t wz[WM];                          // their zones
  uint64_t zm[WM / 64];                    // current anchor: zero-cost window hosts, per chunk
  double csum[ZMAX * ZMAX], bsum[ZMAX * ZMAX];
  int32_t cnt[ZW_SCAN][ZW_WAVES];          // window build: hits per (pass row, wave)
  double red[ZW_WAVES][12];                // block reductions: max d, min d, min avail
  double smin[ZW_SB][4];                   // suffix minima of the demands, per 64-task batch
  double lg[ZW_LOGN][4];                   // the log's ring, by chain position & (ZW_LOGN - 1): capacities after each commit
  int32_t lgid[ZW_LOGN];                   //   and the host, or ZW_SAME (a run writes ahead of its batch)
  int32_t rwho[64], rstart[64];            // fast prologue: an entry's chain-local range [rstart, rwho)
  uint64_t sbits[CHAIN_MAX / 64];          // chain mode: bit i = a group segment starts at task i
  uint32_t amask[ZMAX];                    // anchor -> its zero-cost zones
  uint32_t umask;
  int32_t nwin, bail;
  int32_t touch[WM / 64];                  // optimistic apply: chunks committed to in LDS (past p0 / pb)
};

// NaN-propagating maximum (fmax drops a NaN operand): the FF certificate (2') must fail on a NaN
// capacity, whose frozen key would break the reference's sorted() order (cost_aware.py:116).
__device__ __forceinline__ double nan_max(double a, double b) {
  return (a != a || b <= a) ? a : b;
}
__device__ __forceinline__ double wave_nmax_d(double v) {
  return wave_reduce_d(v, [](double a, double b) { return nan_max(a, b); });
}

// The wide instance's own LDS (rounds of more than ZMAX zones, pvt_zwalk_wide.hip): the zones of
// the chain's zero-cost component renumbered 0..k-1 in ascending zone id. After the prologue the
// walk runs on local ids alone (S.csum / S.bsum hold the component's k x k block, anchors and
// window zones are local), exactly as a round of k zones.
struct ZwWideLDS {
  uint8_t zl[ZWIDE];                       // zone -> local id, ZL_NONE: not in the component
  int16_t gl[ZMAX];                        // local id -> zone
  int32_t seg[2 * ZW_WAVES];               // component zones per (pass, wave) of the numbering
  int32_t root;                            // the component (its root in ZwalkArgs.zcomp), < 0: none
  uint32_t aset;                           // the chain's anchors (local ids)
};

#ifndef PVT_ZWALK_WIDE_TU
// Per-dimension minimum capacity over hosts [lo, hi) (certificate 2), ZW_MINB partials.
__global__ __launch_bounds__(256) void host_min_kernel(const double* avail, int H, int lo, int hi,
                                                       double* part) {
  __shared__ double red[4][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double m[4] = {DINF, DINF, DINF, DINF};
  for (int h = lo + blockIdx.x * 256 + tid; h < hi; h += gridDim.x * 256)
#pragma unroll
    for (int r = 0; r < 4; r++) m[r] = fmin(m[r], avail[(size_t)r * H + h]);
#pragma unroll
  for (int r = 0; r < 4; r++) {
    m[r] = wave_min_d(m[r]);
    if (lane == 0) red[wave][r] = m[r];
  }
  __syncthreads();
  if (tid < 4) {
    double v = red[0][tid];
    for (int w = 1; w < 4; w++) v = fmin(v, red[w][tid]);
    part[blockIdx.x * 4 + tid] = v;
  }
}
#endif

// A compile-time integer as a function argument (run_bulk: the dimensions a run updates).
template <int N> struct IntC { static constexpr int value = N; };

// A branch condition the wave holds uniformly: through readfirstlane, so that the compiler's
// divergence analysis (which loses track across this walk's nested loops) keeps the branch scalar
// instead of building exec-mask loops around it.
#define UNI(c) (__builtin_amdgcn_readfirstlane((int)(c)) != 0)

// Fit from the minimum residual min(a - d): a >= d (best-fit) or a > d (first-fit, strict) in
// every dimension; exact in sign for finite values (certificate 3).
template <bool STRICT>
__device__ __forceinline__ bool fit_res(double m) { return STRICT ? (m > 0.0) : (m >= 0.0); }

// One wave orders its LDS stores before its later loads (compiler fence + lgkmcnt(0)).
__device__ __forceinline__ void wave_lds_sync() {
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
  __builtin_amdgcn_s_waitcnt(0xc07f);
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
}

// The first WM hosts of [h_lo, h_hi), in index order, whose zone is in the mask U
// (pvt_zwin_dev.h, with this walk's workgroup and ZW_SCAN rows per pass).
template <int WM = ZW_M>
__device__ __forceinline__ void compact_zone_window(const int32_t* zone, int Z, uint32_t U,
                                                    int h_lo, int h_hi, int32_t* wid, int32_t* wz,
                                                    int32_t (*cnt)[ZW_WAVES], int32_t* nwin) {
  compact_zone_window_t<WM, ZW_THREADS, ZW_SCAN>(zone, Z, U, h_lo, h_hi, wid, wz, cnt, nwin);
}

// The winner's log entry: its host and its capacities after the commit, at the task's ring slot.
template <int WM>
__device__ __forceinline__ void zw_log_entry(ZwalkLDS<WM>& S, int q, int32_t id, double a0, double a1,
                                             double a2, double a3) {
  S.lg[q][0] = a0; S.lg[q][1] = a1; S.lg[q][2] = a2; S.lg[q][3] = a3;
  S.lgid[q] = id;
}

// A run of R tasks with the same demand d from batch task k, placed on one 64-host chunk
// (registers c0..c3, host cid; m0 = its lanes that fit d, all of them zero-cost). Sequentially
// each task takes the lowest fitting lane; a lane that no longer fits d never fits it again
// (capacities only fall), and the lanes that do not fit now never will, so the run fills the
// fitting lanes in index order, each until it cannot take another copy of d. Pass 1: every
// lane subtracts d again and again in parallel (cnt = copies taken; the active set only
// shrinks), until the lanes up to the lowest active one u have taken R copies (fb = copies of
// the finished lanes below u, u itself has taken t) or no lane takes another. Lane l then takes
// asg = clamp(R - (copies of the lanes before it), 0, cnt) tasks; pass 2 leaves the chunk's
// registers at the capacities after exactly those subtractions (from pass 1's snapshot of the
// lane plus at most a block's copies, or replayed from the start) and logs them at the batch
// position of the lane's last task. Returns the tasks placed (>= 1; fewer than R when the chunk runs
// out). Bit-exact: the same sequential subtractions as one task after the other.
// (One body for all four call sites; the closed-form counts of c05054d were compiled into the
// hot loop's call only: a copy at each of the four call sites ran the walk out of scalar registers)
template <bool STRICT, int WM>
__device__ __forceinline__ int zw_run_bulk(ZwalkLDS<WM>& S, ZwStamps& st, double& c0, double& c1, double& c2,
                                           double& c3, int32_t cid, double d0, double d1, double d2,
                                           double d3, uint64_t m0, int R, int k) {
  st.bulk_enter(k);
  // (Dimensions of demand +0 keep their capacity, x - +0 == x bit for bit, and fit as they did
  // for m0: with d2 = d3 = +0, the trace's disk and gpus, only cpus and memory are counted and
  // updated.)
  if (!(d0 >= 0.0 && d1 >= 0.0 && d2 >= 0.0 && d3 >= 0.0)) R = 1;   // (then one task only)
  const bool on1 = __builtin_amdgcn_inverse_ballot_w64(m0);
  const bool two = __double_as_longlong(d2) == 0 && __double_as_longlong(d3) == 0;
  R = __builtin_amdgcn_readfirstlane(R);
  int cnt = 0;
  st.bulk_setup_done();
  double s0 = c0, s1 = c1, s2 = c2, s3 = c3;   // pass 1's snapshots (below; c until a block start takes one)
  int t = 0;                               // copies pass 1 has subtracted
  // Pass 1: without per-lane masks: with d >= 0 a lane that fails a copy fails every later
  // one (its residual only falls further), so every lane just keeps subtracting, counting
  // the copies that fit (= the copies it takes); lanes outside m0 start at -inf.
  // ZW_UNROLL copies per check (a check past the stop only raises counts of lanes that get no
  // task or no more tasks: asg clamps them).
  // The loop is bound by issue, not by latency (tools/f64_chain.hip: a dependent v_add_f64
  // link is 9 cycles, an instruction of a lone wave issues every ~5), so a copy costs its
  // instructions: the subtractions, the minima, one compare and one carry add -- a copy that
  // fits adds one to cnt (exact: a lane that fails a copy fails every later one, so its
  // count is the number of copies that fit). The copies of a block are software-pipelined in
  // the source (subtractions of copy j, pair minima of j - 1, last minimum of j - 2, test of
  // j - 3) and pinned by scheduling barriers, so that no instruction waits for the one
  // before it. Left alone the compiler puts each minimum and compare right behind what it
  // reads.
  // Snapshots for pass 2: s = the capacities at the last block start at which the lane still
  // fit every copy so far (two selects per changing dimension per block, not per copy).
  double x0 = on1 ? c0 : -DINF, x1 = on1 ? c1 : -DINF, x2 = on1 ? c2 : -DINF, x3 = on1 ? c3 : -DINF;
  auto pass1 = [&](auto dims) {
    constexpr int D = decltype(dims)::value;
    constexpr int U = ZW_UNROLL;
    int u = __builtin_ctzll(m0), fb = 0;
    bool f = false;
    for (;;) {
      t = __builtin_amdgcn_readfirstlane(t);
      u = __builtin_amdgcn_readfirstlane(u);
      fb = __builtin_amdgcn_readfirstlane(fb);
      if (t > 0) {                           // (f: the lane took the last block's last copy)
        s0 = f ? x0 : s0; s1 = f ? x1 : s1;
        if (D == 4) { s2 = f ? x2 : s2; s3 = f ? x3 : s3; }
      }
      double a0[U], a1[U], a2[U], a3[U], mp[U], mq[U], mm[U];
#pragma unroll
      for (int j = 0; j < U + 3; j++) {
        if (j < U) {
          a0[j] = (j ? a0[j - 1] : x0) - d0;
          a1[j] = (j ? a1[j - 1] : x1) - d1;
          if (D == 4) { a2[j] = (j ? a2[j - 1] : x2) - d2; a3[j] = (j ? a3[j - 1] : x3) - d3; }
        }
        if (j >= 1 && j - 1 < U) {
          mp[j - 1] = fmin(a0[j - 1], a1[j - 1]);
          if (D == 4) mq[j - 1] = fmin(a2[j - 1], a3[j - 1]);
        }
        if (j >= 2 && j - 2 < U) mm[j - 2] = D == 4 ? fmin(mp[j - 2], mq[j - 2]) : mp[j - 2];
        if (j >= 3) {
          f = fit_res<STRICT>(mm[j - 3]);
          cnt += f ? 1 : 0;
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      x0 = a0[U - 1]; x1 = a1[U - 1];
      if (D == 4) { x2 = a2[U - 1]; x3 = a3[U - 1]; }
      t += ZW_UNROLL;
      // (the stop tests on scalars: a ballot through rfl_u64, t / u / fb / R through
      // readfirstlane -- plain scalar compares, no round trip through a vector register)
      const uint64_t an = rfl_u64(__ballot(f));   // lanes that took copy t
      if (an == 0) break;
      const int un = __builtin_ctzll(an);
      if (un != u) {                         // (u only rises: every lane below un is done)
        u = un;
        fb = __builtin_amdgcn_readlane(wave_incl_scan_dpp(cnt), u - 1);
      }
      if (fb + t >= R) break;
    }
  };
  if (two) pass1(IntC<2>{});
  else pass1(IntC<4>{});
  st.bulk_pass1_done(t);
  const int incl = wave_incl_scan_dpp(cnt);
  const int pre = incl - cnt;
  const int asg = max(0, min(cnt, R - pre));
  const int covered = min(R, __builtin_amdgcn_readlane(incl, 63));
  st.bulk_counted();
  // Pass 2: a taking lane marks its host and ends at its capacities after asg copies: the same
  // sequential subtractions as task after task, so bit-exact. Pass 1 held most of them: the
  // snapshot s is the lane's value after sbc copies, sbc = the last block start it was still
  // whole at (the largest multiple of ZW_UNROLL up to cnt, at most the last block's start).
  // A lane with asg >= sbc -- every lane that takes all its copies, and the last taking lane
  // when the run ends in the block that stopped pass 1 -- goes on from s with asg - sbc copies,
  // at most a block's (x - d by v_add_f64 and fma(-1, d, x) round once to the same value);
  // a lane that takes fewer copies than its snapshot holds (at most one per call: the last
  // taking lane) replays its asg copies from c. A lane that takes nothing has sbc > 0 = asg or
  // s == c: it keeps c. The log keeps the host of
  // every copy and the capacities after a lane's last one only: a host's earlier entries in a
  // segment are never final (epoch_final_kernel marks them; validation and apply read the
  // capacities of final entries only, and the keyed / ordered walks read no log).
  // (each taking lane writes its host at its first run position only; the positions after it
  // keep the batch's "as before" mark, ZW_SAME, and the flush gives each the host of the last
  // written position at or before it -- once per batch, not once per run)
  if (asg > 0) S.lgid[(k + pre) & (ZW_LOGN - 1)] = cid;
  const int sbc = min(cnt / ZW_UNROLL * ZW_UNROLL, max(t - ZW_UNROLL, 0));
  const bool snap = asg >= sbc;
  const int nrep = snap ? asg - sbc : asg;
  c0 = snap ? s0 : c0; c1 = snap ? s1 : c1;
  c2 = snap ? s2 : c2; c3 = snap ? s3 : c3;  // (two: s2 == c2, s3 == c3)
  // the copies left, a scalar: at most a block's from a snapshot (4 or 8: one ballot), and the
  // count of the one lane that starts over, if any
  const uint64_t over = rfl_u64(__ballot(asg > 0 && !snap));
  int nmax = rfl_u64(__ballot(snap && nrep > 4)) ? ZW_UNROLL : rfl_u64(__ballot(snap && nrep > 0)) ? 4 : 0;
  if (over) nmax = max(nmax, __builtin_amdgcn_readlane(asg, __builtin_ctzll(over)));
  st.bulk_assigned(asg, cnt, over);
  // (c - d as fma(-1, d, c), rounded once, the same bits; fma(-0, d, c) == c for the finite d
  // and c of a proven chain: one 0/1 factor per copy for every dimension)
  if (two) {
    for (int m = 0; m < nmax; m += 4) {
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const double o = m + u < nrep ? -1.0 : -0.0;
        c0 = __builtin_fma(o, d0, c0);
        c1 = __builtin_fma(o, d1, c1);
      }
      st.bulk_replay_block();
    }
  } else {
    for (int m = 0; m < nmax; m += 4) {
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const double o = m + u < nrep ? -1.0 : -0.0;
        c0 = __builtin_fma(o, d0, c0);
        c1 = __builtin_fma(o, d1, c1);
        c2 = __builtin_fma(o, d2, c2);
        c3 = __builtin_fma(o, d3, c3);
      }
      st.bulk_replay_block();
    }
  }
  st.bulk_replayed();
  if (asg > 0) {
    const int q = (k + pre + asg - 1) & (ZW_LOGN - 1);
    S.lg[q][0] = c0; S.lg[q][1] = c1; S.lg[q][2] = c2; S.lg[q][3] = c3;
  }
  st.bulk_exit();
  return covered;
}

// KEYED: cost_aware first-fit with sort_hosts (the driver's round_next_window): one group, its
// window the first ZW_M hosts of the group's zero-key prefix (perm, index order), strict fit,
// no zone certificates (the order is the keyed path's own); the window's capacities are written
// back at the end and status[0] = tasks walked.
// KEYED with STRICT = false: vbp first-fit (index order, fit >=) over a window of the first
// alive hosts (the driver's ordered_frontier), same mechanics.
// FAST: the fast prologue of the round's first best-fit epoch (below), a template flag so that
// neither instance carries both prologues.
// WMP: the window's hosts; negative for the WIDE instance of that window (rounds of more than ZMAX
// zones, instantiated in pvt_zwalk_wide.hip): chain mode, the ordinary prologue, and in it the
// chain's component renumbered (ZwWideLDS); everything wide is discarded from the other instances.
template <bool KEYED, bool STRICT, bool FF = false, int WMP = ZW_M, bool FAST = false>
__global__ __launch_bounds__(ZW_THREADS) void zwalk_kernel(ZwalkArgs A) {
  constexpr bool WIDE = WMP < 0;
  constexpr int WM = WIDE ? -WMP : WMP;
  static_assert(!FF || (!KEYED && STRICT), "FF: chain mode, strict fit");
  static_assert(WM == ZW_M || !KEYED, "keyed / ordered / sharded windows: ZW_M hosts");
  static_assert(!WIDE || (!KEYED && !FAST), "wide: chain mode, the ordinary prologue");
  __shared__ ZwalkLDS<WM> S;
  [[maybe_unused]] ZwWideLDS* W = nullptr;
  if constexpr (WIDE) {
    __shared__ ZwWideLDS wide_lds;
    W = &wide_lds;
  }
  ZwStamps st;
  st.start();
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // chain tables: by value in the arguments (A.tab; the host sends them only for chains of at
  // most CHAIN_MAX tasks, as the epoch planner builds them), or device arrays (uploaded)
  const bool tabm = !KEYED && A.tab.nch > 0;
  const int base = KEYED ? 0 : tabm ? A.tab.coff[b] : A.coff[b];
  const int nt = KEYED ? A.knt : tabm ? A.tab.coff[b + 1] - A.tab.coff[b] : A.coff[b + 1] - base;
  // chain-local position -> epoch task (A.cmap, global): with the tables by value, this block
  // writes its chain's range of it from the segments first (read back by the same block after the
  // barrier below; the prologue's first positions come from the segments directly). (Neither a map in LDS -- the select between an LDS and a global map became a
  // flat load per access -- nor one computed from the segments per access: the walk ran 4-7 %
  // slower either way.)
  const int32_t* gcmap = KEYED ? nullptr : A.cmap + base;
  const bool segm = !KEYED && (tabm || A.cseg);   // group segment starts break runs
  int32_t* status = A.status + 2 * b;
  // (WIDE: Z becomes the zones of the chain's component in the prologue; ZG stays the round's)
  int Z = A.Z;
  const int H = A.H;
  [[maybe_unused]] const int ZG = A.Z;
  // the chain's report (one thread): the device words the epoch kernels read and, with the
  // optimistic apply, the host's mapped words -- no later kernel copies them
  auto report = [&](int s0, int s1) {
    status[0] = s0; status[1] = s1;
    if (!KEYED && A.hstat) { A.hstat[2 * b] = s0; A.hstat[2 * b + 1] = s1; }
  };

  // the chain's range of the position map from the segments, and block 0's publication of the
  // tables for the epoch kernels after the walk (tables by value; either prologue)
  auto publish_map = [&]() {
    if (tabm) {
      int32_t* wmap = const_cast<int32_t*>(A.cmap) + base;
      for (int k = A.tab.csoff[b]; k < A.tab.csoff[b + 1]; k++) {
        const int sg = A.tab.csegid[k], c0 = A.tab.seg_cstart[sg], o0 = A.tab.seg_off[sg];
        const int len = A.tab.seg_off[sg + 1] - o0;
        for (int i = tid; i < len; i += ZW_THREADS) wmap[c0 + i] = o0 + i;
      }
      // block 0 publishes the tables for the epoch kernels after the walk
      if (b == 0) {
        const int ns = A.tab.nseg, nc = A.tab.nch;
        for (int i = tid; i <= ns; i += ZW_THREADS) {
          A.tab.o_seg_off[i] = A.tab.seg_off[i];
          if (i < ns) { A.tab.o_seg_chain[i] = A.tab.seg_chain[i]; A.tab.o_seg_cstart[i] = A.tab.seg_cstart[i]; }
        }
        for (int i = tid; i <= nc; i += ZW_THREADS) A.tab.o_coff[i] = A.tab.coff[i];
      }
    }
  };
  double mn[4];                              // (the walk: the batch's minima ahead)
  uint32_t U;                                // the window's zone set (certificate 2)
  int nwin;
  if constexpr (FAST) {
    // ---- The fast prologue (ChainCert): an unsharded best-fit chain of the
    // round's first epoch, tables by value, every segment a whole group with a certificate
    // (GroupCert) from the order launch, its window prebuilt (ZoneWindows). Every load is issued
    // here, before the first barrier, all in flight together: the zone tables, the host-minimum
    // partials, the window the host names (its zone set, n, bad, ids, zones, capacities, straight
    // to LDS) and the records of this chain's segments -- wave w takes segments w, w + 4, ..., a
    // lane per 64-task sub-batch. No pass over demand rows or anchors, no finiteness scan of the
    // capacities (ZoneWindow::bad), no ZwUndo stores (epoch_undo_kernel reads the window itself).
    // Exactness:
    //  * extremes, bound flag: fmax / fmin over the records equal the scan's over the rows (fmax
    //    and fmin drop a NaN either way) up to the sign of a zero, which no consumer distinguishes
    //    (the certificate word and sep compare with <=, >=; cmax is only subtracted from);
    //  * window: the host's zone set of the chain must lie in the window's U' (else (0, 1): the
    //    list walk decides); U' takes U's place in certificate 2, as in the other prologue;
    //  * batch minima: S.smin[q] is the minimum over the (segment, sub-batch) entries, in chain
    //    order, from the first whose chain-local range reaches past 64 q -- a lower bound of the
    //    demands at positions >= 64 q (a straddling sub-batch brings up to 63 earlier tasks). The
    //    walk uses it (mn) only to decide that a chunk can still take a task ahead, so a lower
    //    bound only keeps a chunk alive longer; slots no entry owns stay at -inf.
    static_assert(!KEYED && !FF && WM == ZW_M && ZW_M == 4 * ZW_THREADS, "fast prologue: best-fit chains");
    static_assert(ZW_ENT <= 64 && ZW_ENT <= ZW_SB, "entries: a lane each, in rwho / rstart / lg");
    const int j = min((int)A.cert.cwin[b], ZMAX - 1);
    const ZoneWindow* const zw = &A.zpre->w[j];
    const int ZZ = Z * Z;
    double cs[4], bs[4], ha[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int i = tid + u * ZW_THREADS;
      cs[u] = i < ZZ ? A.csum[i] : 0.0;
      bs[u] = i < ZZ ? A.bsum[i] : 0.0;
    }
#pragma unroll
    for (int r = 0; r < 4; r++) ha[r] = A.hmin[tid * 4 + r];
    const uint32_t zu = A.zpre->U[j];
    const int zn = zw->n, zbad = zw->bad;
    int32_t wi[4], wzv[4];
    double wv[4][4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int p = tid + u * ZW_THREADS;
      wi[u] = zw->id[p];
      wzv[u] = zw->z[p];
#pragma unroll
      for (int r = 0; r < 4; r++) wv[u][r] = zw->a[r][p];
    }
    const int k0 = A.tab.csoff[b], k1 = A.tab.csoff[b + 1];
    // a segment's record: lane l its sub-batch l's minima, lanes 0-3 the maxima; entries at
    // seg_ent + l of the chain's list (values in S.lg, chain-local range in S.rstart / S.rwho)
    double mxv = -DINF;
    bool badv = false;
    for (int k = k0 + wave; k < k1; k += ZW_WAVES) {
      const int sg = A.tab.csegid[k], c0 = A.tab.seg_cstart[sg];
      const int len = A.tab.seg_off[sg + 1] - A.tab.seg_off[sg];
      const GroupCert* const gc = A.cert.rec + min((int)A.cert.seg_grp[sg], GCOMPACT_MAX - 1);
      const int ne = (len + 63) >> 6, e = A.cert.seg_ent[sg] + lane;
      const bool on = lane < ne && lane < GC_SUB && e < ZW_ENT;
      double sm[4];
#pragma unroll
      for (int r = 0; r < 4; r++) sm[r] = on ? gc->smin[lane][r] : DINF;
      const double gm = lane < 4 ? gc->mx[lane] : -DINF;
      badv |= gc->bad != 0 || gc->n != len;
      mxv = fmax(mxv, gm);
      if (on) {
#pragma unroll
        for (int r = 0; r < 4; r++) S.lg[e][r] = sm[r];
        S.rstart[e] = c0 + 64 * lane;
        S.rwho[e] = c0 + min(64 * lane + 64, len);
      }
    }
    publish_map();
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int i = tid + u * ZW_THREADS;
      if (i < ZZ) { S.csum[i] = cs[u]; S.bsum[i] = bs[u]; }
    }
    if (tid < CHAIN_MAX / 64) S.sbits[tid] = 0;
    if (tid < WM / 64) S.touch[tid] = 0;
    if (tid < ZW_SB) {
#pragma unroll
      for (int r = 0; r < 4; r++) S.smin[tid][r] = -DINF;
    }
    nwin = min(zn, ZW_M);
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int p = tid + u * ZW_THREADS;
      if (p < nwin) {
        S.wid[p] = wi[u];
        S.wz[p] = wzv[u];
#pragma unroll
        for (int r = 0; r < 4; r++) S.wa[r][p] = wv[u][r];
      }
    }
#pragma unroll
    for (int r = 0; r < 4; r++) ha[r] = wave_min_d(ha[r]);
    const bool wbadv = __ballot(badv) != 0;
    if (lane < 4) S.red[wave][lane] = mxv;
    if (lane == 0) {
#pragma unroll
      for (int r = 0; r < 4; r++) S.red[wave][8 + r] = ha[r];
      S.cnt[0][wave] = wbadv ? 1 : 0;
    }
    st.loaded();
    __syncthreads();
    if (tid < Z) {                             // anchor row -> zero-cost zone mask
      uint32_t m = 0;
      for (int z = 0; z < Z; z++) m |= (S.csum[tid * Z + z] == 0.0) ? (1u << z) : 0u;
      S.amask[tid] = m;
    }
    for (int k = k0 + tid; k < k1; k += ZW_THREADS) {   // segment starts (chain-local positions)
      const int p = A.tab.seg_cstart[A.tab.csegid[k]];
      if (p > 0 && p < CHAIN_MAX) atomicOr(&S.sbits[p >> 6], 1ull << (p & 63));
    }
    double mx[4];
    bool bad = false;
#pragma unroll
    for (int w = 0; w < ZW_WAVES; w++) bad |= S.cnt[0][w] != 0;
#pragma unroll
    for (int r = 0; r < 4; r++) {
      mx[r] = fmax(fmax(S.red[0][r], S.red[1][r]), fmax(S.red[2][r], S.red[3][r]));
      ha[r] = fmin(fmin(S.red[0][8 + r], S.red[1][8 + r]), fmin(S.red[2][8 + r], S.red[3][8 + r]));
    }
    // the entries' suffix minima, wave r for dimension r, a lane per entry; an entry owns the
    // slot q whose boundary 64 q lies in its range [start, end) (at most one: 64 tasks or fewer)
    const int ne = min((int)A.cert.cent[b], ZW_ENT);
    {
      double v = lane < ne ? S.lg[lane][wave] : DINF;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) v = fmin(v, __shfl_down(v, off));
      if (lane < ne) {
        const int q = (S.rstart[lane] + 63) >> 6;
        if (q * 64 < S.rwho[lane] && q < ZW_SB) S.smin[q][wave] = v;
      }
      if (lane == 0) S.red[0][4 + wave] = v;   // (the chain's minimum: the certificate word)
    }
    bool sep = false;                          // (cert_separates, written out: pvt_cert.h)
#pragma unroll
    for (int r = 0; r < 4; r++) sep |= (ha[r] - mx[r] >= CERT_SEP);
    U = zu;
    // (it never walks a window it has not verified: the host's zone set inside the window's)
    const bool cover = zu != 0 && (A.cert.cu[b] & ~zu) == 0;
    const bool stop = bad || !sep || nt <= 0 || nt > CHAIN_MAX || !cover || zbad != 0 || nwin <= 0;
    st.certified_fast();
    __syncthreads();
    if (tid == 0) {
      int cert = stop ? 0 : ZW_CERT_FAST;
#pragma unroll
      for (int r = 0; r < 4; r++) cert |= zw_cert_dim(mx[r], S.red[0][4 + r], ha[r], r);
      if (A.hcert) A.hcert[b] = cert;
      if (stop) report(0, nt <= 0 ? 0 : 1);
    }
    if (A.cmax && tid < 4) A.cmax[b * 4 + tid] = mx[tid];   // (the validation's fast path)
    if (stop) return;
  } else {
    // Every load the prologue needs that depends on nothing else is issued first (the zone
    // tables, the host minima, the chain's first task positions, its segment range), so the
    // prologue waits for about two HBM latencies, not one per step.
    static_assert(ZMAX * ZMAX <= 4 * ZW_THREADS && ZW_MINB == ZW_THREADS, "prologue loads");
    const int ZZ = (KEYED || WIDE) ? 0 : Z * Z;   // (WIDE: the component's block, gathered below)
    double cs[4], bs[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int i = tid + u * ZW_THREADS;
      cs[u] = i < ZZ ? A.csum[i] : 0.0;
      bs[u] = i < ZZ ? A.bsum[i] : 0.0;
    }
    // host minima (FF: maxima of |capacity|) from the partials
    double ha[4] = {FF ? -DINF : DINF, FF ? -DINF : DINF, FF ? -DINF : DINF, FF ? -DINF : DINF};
    if (!KEYED) {
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const double x = A.hmin[tid * 4 + r];
        ha[r] = FF ? nan_max(ha[r], x) : fmin(ha[r], x);
      }
    }
    publish_map();
    int wv[ZW_PR];
    if (tabm) {
      // the first positions straight from the segments (no dependent load of the map before the
      // demand rows: one HBM latency less in the prologue)
      const int k0 = A.tab.csoff[b], k1 = A.tab.csoff[b + 1];
#pragma unroll
      for (int u = 0; u < ZW_PR; u++) {
        const int i = u * ZW_THREADS + tid;
        int v = -1;
        for (int k = k0; k < k1; k++) {
          const int sg = A.tab.csegid[k], c0 = A.tab.seg_cstart[sg];
          if (i >= c0) v = A.tab.seg_off[sg] + (i - c0);
        }
        wv[u] = i < nt ? v : -1;
      }
    } else {
#pragma unroll
      for (int u = 0; u < ZW_PR; u++) {
        const int i = u * ZW_THREADS + tid;
        wv[u] = i < nt ? (KEYED ? i : gcmap[i]) : -1;
      }
    }
    const int sg0 = tabm ? A.tab.csoff[b] : (!KEYED && A.cseg) ? A.csoff[b] : 0;
    const int sg1 = tabm ? A.tab.csoff[b + 1] : (!KEYED && A.cseg) ? A.csoff[b + 1] : 0;
    // prebuilt windows' zone sets (ZoneWindows; lane j: zone j's, 0 = none)
    const uint32_t zpu = (!KEYED && !WIDE && WM == ZW_M && A.zpre && lane < Z) ? A.zpre->U[lane] : 0u;
    // WIDE: the zones' components (two zones per thread), and the chain's component from its
    // first task's anchor
    static_assert(ZWIDE == 2 * ZW_THREADS, "wide prologue: two zones per thread");
    [[maybe_unused]] int zc0 = -1, zc1 = -1;
    if constexpr (WIDE) {
      zc0 = tid < ZG ? A.zcomp[tid] : -1;
      zc1 = tid + ZW_THREADS < ZG ? A.zcomp[tid + ZW_THREADS] : -1;
      W->zl[tid] = ZL_NONE;
      W->zl[tid + ZW_THREADS] = ZL_NONE;
      if (tid == 0) {
        const int a0 = nt > 0 ? A.anc[max(wv[0], 0)] : -1;
        W->root = (a0 >= 0 && a0 < ZG) ? A.zcomp[a0] : -2;
        W->aset = 0;
      }
    }

#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int i = tid + u * ZW_THREADS;
      if (i < ZZ) { S.csum[i] = cs[u]; S.bsum[i] = bs[u]; }
    }
    if (tid == 0) { S.umask = 0; S.nwin = 0; S.bail = 0; }
    if (tid < CHAIN_MAX / 64) S.sbits[tid] = 0;
    if (tid < WM / 64) S.touch[tid] = 0;
    st.loaded();
    __syncthreads();
    if constexpr (WIDE) {
      // The component's zones numbered in ascending zone id (pass p, thread t: zone 256 p + t; a
      // ballot per wave, the waves' counts through LDS), the local -> zone list, and the
      // component's k x k block of the sum tables gathered into S.csum / S.bsum: the same
      // doubles the walk of a k-zone round would read. More than ZMAX zones: no walk.
      const int root = W->root;
      const bool m0 = root >= 0 && zc0 == root, m1 = root >= 0 && zc1 == root;
      const uint64_t b0 = __ballot(m0), b1 = __ballot(m1);
      if (lane == 0) { W->seg[wave] = __popcll(b0); W->seg[ZW_WAVES + wave] = __popcll(b1); }
      __syncthreads();
      int base0 = 0, base1 = 0, k = 0;
#pragma unroll
      for (int w = 0; w < 2 * ZW_WAVES; w++) {
        const int c = W->seg[w];
        base0 += w < wave ? c : 0;
        base1 += w < ZW_WAVES + wave ? c : 0;
        k += c;
      }
      const uint64_t below = (1ull << lane) - 1ull;
      const int l0 = base0 + __popcll(b0 & below), l1 = base1 + __popcll(b1 & below);
      if (m0 && l0 < ZMAX) { W->zl[tid] = (uint8_t)l0; W->gl[l0] = (int16_t)tid; }
      if (m1 && l1 < ZMAX) { W->zl[tid + ZW_THREADS] = (uint8_t)l1; W->gl[l1] = (int16_t)(tid + ZW_THREADS); }
      if (k < 1 || k > ZMAX) S.bail = 1;       // benign race: every writer stores 1
      Z = min(k, ZMAX);
      __syncthreads();
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int i = tid + u * ZW_THREADS;
        if (i < Z * Z) {
          const int la = i / Z, lz = i - la * Z;
          const int g = (int)W->gl[la] * ZG + (int)W->gl[lz];
          S.csum[i] = A.csum[g];
          S.bsum[i] = A.bsum[g];
        }
      }
      __syncthreads();
    }
    if (!KEYED && tid < Z) {                   // anchor row -> zero-cost zone mask
      uint32_t m = 0;
      for (int z = 0; z < Z; z++) m |= (S.csum[tid * Z + z] == 0.0) ? (1u << z) : 0u;
      S.amask[tid] = m;
    }
    if (tabm) {                                // segment starts (chain-local positions)
      for (int k = sg0 + tid; k < sg1; k += ZW_THREADS) {
        const int p = A.tab.seg_cstart[A.tab.csegid[k]];
        if (p > 0 && p < CHAIN_MAX) atomicOr(&S.sbits[p >> 6], 1ull << (p & 63));
      }
    } else {
      for (int k = sg0 + tid; k < sg1; k += ZW_THREADS) {
        const int p = A.cseg[k];
        if (p > 0 && p < CHAIN_MAX) atomicOr(&S.sbits[p >> 6], 1ull << (p & 63));
      }
    }

    // the chain's anchors (-> its zones U below), demand extremes and finiteness (certificates 2,
    // 3), and the minima of the demands per 64-task batch (for the suffix minima below: a wave's
    // 64 lanes of one pass are one batch); ZW_PR rows per thread in flight at once, the next pass's
    // positions loaded while this one is reduced
    uint32_t abits = 0;                        // anchors seen (Z <= 32)
    double mx[4] = {-DINF, -DINF, -DINF, -DINF};
    mn[0] = mn[1] = mn[2] = mn[3] = DINF;
    bool bad = false;
    for (int i0 = 0; i0 < nt; i0 += ZW_PR * ZW_THREADS) {
      int av[ZW_PR], wn[ZW_PR];
      double dv[ZW_PR][4];
#pragma unroll
      for (int u = 0; u < ZW_PR; u++) {
        const int w = max(wv[u], 0);
        av[u] = A.anc[w];
#pragma unroll
        for (int r = 0; r < 4; r++) dv[u][r] = A.dem[(size_t)w * 4 + r];
      }
#pragma unroll
      for (int u = 0; u < ZW_PR; u++) {
        const int i = i0 + ZW_PR * ZW_THREADS + u * ZW_THREADS + tid;
        wn[u] = i < nt ? (KEYED ? i : gcmap[i]) : -1;
      }
#pragma unroll
      for (int u = 0; u < ZW_PR; u++) {
        const bool ok = wv[u] >= 0;
        double bm[4];
#pragma unroll
        for (int r = 0; r < 4; r++) bm[r] = ok ? dv[u][r] : DINF;
        if (ok) {
          int a = av[u];
          // (WIDE: the anchor's local id; a zone of another component is no anchor of this chain)
          if constexpr (WIDE) a = (a >= 0 && a < ZG) ? (int)W->zl[a] : (int)ZL_NONE;
          if (a < 0 || a >= Z) {
            bad = true;
          } else {
            abits |= 1u << a;
#pragma unroll
            for (int r = 0; r < 4; r++) {
              bad |= !cert_bounded(dv[u][r]);
              mx[r] = fmax(mx[r], dv[u][r]);
              mn[r] = fmin(mn[r], dv[u][r]);
            }
          }
        }
        const int blk = (i0 + u * ZW_THREADS) / 64 + wave;   // (uniform: the wave's batch)
        if (blk < ZW_SB - 1 && blk * 64 < nt) {
#pragma unroll
          for (int r = 0; r < 4; r++) bm[r] = wave_min_d(bm[r]);
          if (lane == 0) {
#pragma unroll
            for (int r = 0; r < 4; r++) S.smin[blk][r] = bm[r];
          }
        }
      }
#pragma unroll
      for (int u = 0; u < ZW_PR; u++) wv[u] = wn[u];
    }
    __syncthreads();                           // (amask)
    uint32_t um = 0;
    if (!KEYED)
      for (uint32_t m = abits; m; m &= m - 1) um |= S.amask[__builtin_ctz(m)];
#pragma unroll
    for (int r = 0; r < 4; r++) {
      mx[r] = wave_max_d(mx[r]);
      mn[r] = wave_min_d(mn[r]);
      ha[r] = FF ? wave_nmax_d(ha[r]) : wave_min_d(ha[r]);
    }
    if (lane == 0) {
#pragma unroll
      for (int r = 0; r < 4; r++) { S.red[wave][r] = mx[r]; S.red[wave][4 + r] = mn[r]; S.red[wave][8 + r] = ha[r]; }
    }
    if (bad) S.bail = 1;                        // benign race: every writer stores 1
    if (um) atomicOr(&S.umask, um);
    if constexpr (WIDE) {
      if (abits) atomicOr(&W->aset, abits);
    }
    __syncthreads();
    if constexpr (WIDE) {
      // Certificate 2 / 2' for the zones outside the component, on every anchor row of the chain
      // (coalesced along the row): c >= 2^-300 and 0 < bw <= 2^300, the clause the walk applies per
      // anchor to the component's own zones outside U. Taken here over all of the chain's anchors
      // at once: a failure leaves the whole chain to the exact path (stricter than the per-anchor
      // test, never wrong). c != 0 there by the component's definition.
      bool out_bad = false;
      for (uint32_t m = W->aset; m; m &= m - 1) {
        const int ga = W->gl[__builtin_ctz(m)];
        for (int z = tid; z < ZG; z += ZW_THREADS) {
          const double c = A.csum[ga * ZG + z], bw = A.bsum[ga * ZG + z];
          if (W->zl[z] == ZL_NONE) out_bad |= !((c >= CERT_C_MIN) && (bw > 0.0) && (bw <= CERT_BW_MAX));
        }
      }
      if (out_bad) S.bail = 1;
      __syncthreads();
    }
    st.certified();
#pragma unroll
    for (int r = 0; r < 4; r++) {
      for (int w = 1; w < ZW_WAVES; w++) {
        mx[r] = fmax(mx[r], S.red[w][r]);
        mn[r] = fmin(mn[r], S.red[w][4 + r]);
        ha[r] = FF ? nan_max(ha[r], S.red[w][8 + r]) : fmin(ha[r], S.red[w][8 + r]);
      }
      mx[r] = fmax(mx[r], S.red[0][r]);
      mn[r] = fmin(mn[r], S.red[0][4 + r]);
      ha[r] = FF ? nan_max(ha[r], S.red[0][8 + r]) : fmin(ha[r], S.red[0][8 + r]);
    }
    if (!KEYED && A.cmax && tid < 4) A.cmax[b * 4 + tid] = mx[tid];   // (the validation's fast path)
    if (!KEYED && A.hcert && tid == 0) {       // the certificate word of the host's verdict
      int cert = 0;
      if (!FF) {                               // (zw_cert_dim, written out: pvt_cert.h)
#pragma unroll
        for (int r = 0; r < 4; r++)
          cert |= ((mx[r] <= 0.0 && mn[r] >= 0.0) ? (ZW_CERT_UNDEMANDED << r) : 0) |
                  ((ha[r] >= CERT_MARGIN) ? (ZW_CERT_HOSTMIN << r) : 0);
      }
      A.hcert[b] = cert;
    }
    bool sep = KEYED;
    if (FF) {                                  // certificates (2') and (3'): bounded capacities,
      sep = true;                              // demands >= 0
#pragma unroll
      for (int r = 0; r < 4; r++) sep &= cert_ff_bounded(ha[r], mn[r]);
    } else {                                   // (cert_separates, written out)
#pragma unroll
      for (int r = 0; r < 4; r++) sep |= (ha[r] - mx[r] >= CERT_SEP);
    }
    U = S.umask;
    if (S.bail || !sep || nt <= 0 || (!KEYED && nt > CHAIN_MAX)) {
      if (tid == 0) report(0, (KEYED || nt <= 0) ? 0 : 1);
      return;
    }
    const FrontierSlot* pw = (!WIDE && A.pwin) ? A.pwin + (KEYED ? 0 : b) : nullptr;   // (wide rounds: unsharded)
    // the round's first epoch: the window the grouped order's launch prebuilt for the component of
    // the chain's anchors (its zone set U' covers U; a window over U' is exact, with U' in the
    // certificates)
    const ZoneWindow* zw = nullptr;
    if (!KEYED && WM == ZW_M && !pw && A.zpre && U != 0) {
      const uint64_t cover = __ballot(zpu != 0 && (U & ~zpu) == 0);
      if (cover) {
        const int j = __builtin_ctzll(cover);
        zw = &A.zpre->w[j];
        U = (uint32_t)__builtin_amdgcn_readlane((int)zpu, j);
      }
    }
    if (pw) {                                  // host-sharded: the merged window, capacities too
      const int nw = min(pw->n, ZW_M);
      for (int p = tid; p < nw; p += ZW_THREADS) {
        const int32_t h = pw->id[p];
        S.wid[p] = h;
        S.wz[p] = KEYED ? 0 : A.zone[h];
      }
      if (tid == 0) S.nwin = nw;
      __syncthreads();
    } else if (zw) {                           // prebuilt: ids and zones (capacities below)
      const int nw = min(zw->n, ZW_M);
      for (int p = tid; p < nw; p += ZW_THREADS) { S.wid[p] = zw->id[p]; S.wz[p] = zw->z[p]; }
      if (tid == 0) S.nwin = nw;
      __syncthreads();
    } else if (KEYED) {                        // window: the zero-key prefix's first hosts
      const int nw = min(A.kn_dev ? *A.kn_dev : A.kn, ZW_M);
      for (int p = tid; p < nw; p += ZW_THREADS) { S.wid[p] = A.lo + A.kperm[p]; S.wz[p] = 0; }
      if (tid == 0) S.nwin = nw;
      __syncthreads();
    } else if constexpr (WIDE) {               // window: U's hosts in index order, zones through
      // the table (membership and S.wz by local id: a zone of another component never enters)
      compact_zone_window_local_t<WM, ZW_THREADS, ZW_SCAN>(A.zone, ZoneLocal{ZG, W->zl, U}, 0, H, S.wid,
                                                           S.wz, S.cnt, &S.nwin);
    } else {                                   // window: U's hosts in index order
      compact_zone_window<WM>(A.zone, Z, U, 0, H, S.wid, S.wz, S.cnt, &S.nwin);
    }
    nwin = S.nwin;
    st.window_built();
    bool wbad = false;
    // optimistic apply: the window's hosts and start capacities, saved for an undo (plain stores
    // nothing waits for)
    ZwUndo* const ud = (!KEYED && A.undo) ? A.undo + b : nullptr;
    if (ud && tid == 0) ud->count = nwin;
    static_assert(WM <= ZW_MBIG, "ZwUndo holds every window");
    static_assert(WM % (4 * ZW_THREADS) == 0, "window capacities: four hosts per thread per pass");
    for (int p0 = 0; p0 < WM && p0 < nwin; p0 += 4 * ZW_THREADS) {
      double v[4][4];                          // every gather of the pass in flight at once
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int p = p0 + u * ZW_THREADS + tid;
        const int h = p < nwin ? S.wid[p] : 0;   // (host 0: a valid address, never used)
#pragma unroll
        for (int r = 0; r < 4; r++)
          v[u][r] = p >= nwin ? 0.0 : (pw ? pw->a[r][p] : zw ? zw->a[r][p] : A.avail[(size_t)r * H + h]);
      }
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int p = p0 + u * ZW_THREADS + tid;
        if (p < nwin) {
#pragma unroll
          for (int r = 0; r < 4; r++) {
            wbad |= !cert_bounded(v[u][r]);
            S.wa[r][p] = v[u][r];
          }
          if (ud) {
            ud->id[p] = S.wid[p];
#pragma unroll
            for (int r = 0; r < 4; r++) ud->a[r][p] = v[u][r];
          }
        }
      }
    }
    if (wbad) S.bail = 1;
    __syncthreads();
    st.capacities_loaded();
    if (S.bail || nwin == 0) {
      if (tid == 0) report(0, KEYED ? 0 : 1);
      return;
    }
    // suffix minima of the chain's demands per 64-task batch: a chunk no host of which fits the
    // smallest demand still ahead is dead (the walk moves its register chunk past it)
    const int nsb = min((nt + 63) >> 6, ZW_SB);
    // (batches before the last were reduced with the certificates above; the last holds the rest)
    for (int blk = ZW_SB - 1 + wave; blk < nsb; blk += ZW_WAVES) {
      const int i1 = blk == ZW_SB - 1 ? nt : min(nt, blk * 64 + 64);
      double bm[4] = {DINF, DINF, DINF, DINF};
      for (int i = blk * 64 + lane; i < i1; i += 64) {
        const int w = KEYED ? i : gcmap[i];
#pragma unroll
        for (int r = 0; r < 4; r++) bm[r] = fmin(bm[r], A.dem[(size_t)w * 4 + r]);
      }
#pragma unroll
      for (int r = 0; r < 4; r++) bm[r] = wave_min_d(bm[r]);
      if (lane == 0) {
#pragma unroll
        for (int r = 0; r < 4; r++) S.smin[blk][r] = bm[r];
      }
    }
    __syncthreads();
    static_assert(ZW_SB == 64 && ZW_WAVES == 4, "suffix minima: one wave per dimension, a lane per batch");
    {                                          // suffix minima: wave r scans dimension r
      double v = lane < nsb ? S.smin[lane][wave] : DINF;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) v = fmin(v, __shfl_down(v, off));
      if (lane < nsb) S.smin[lane][wave] = v;
    }
    __syncthreads();
  }
  if (wave != 0) return;
  st.walk_begins();

  // ---- the walk (one wave). Lane l of chunk c holds window host c * 64 + l. Chunk p0 (the
  // first that can still fit a chain task) stays in registers, where nearly every task finds its
  // winner: a task is then four compares, a ballot and a one-lane update, with no memory access
  // on its path. Otherwise the chunk is written back and the later chunks are scanned in LDS.
  // The winning lane writes the task's log entry into an LDS batch buffer, flushed to HBM every
  // 64 tasks.
  const int nch = (nwin + 63) >> 6;
  int p0 = 0;                                // chunks before p0 cannot fit any chain task
  int cur = -1;                              // anchor the zero-cost masks are for
  int done = 0;
  bool failed = false, exhausted = false;
  // chunk p0 in registers
  double ra0, ra1, ra2, ra3;
  int32_t rid;
  uint64_t rzm = 0, rvalid = 0;              // its zero-cost lanes (anchor cur), its real lanes
  bool dirty = false;
  auto load_chunk = [&](int c) {
    const int p = c * 64 + lane;
    const int q = min(p, nwin - 1);
    ra0 = S.wa[0][q]; ra1 = S.wa[1][q]; ra2 = S.wa[2][q]; ra3 = S.wa[3][q];
    rid = S.wid[q];
    rvalid = __ballot(p < nwin);
    dirty = false;
    __builtin_amdgcn_s_waitcnt(0xc07f);   // loads landed here, so the hot loop carries no wait
  };
  auto store_chunk = [&](int c) {
    const int p = c * 64 + lane;
    if (dirty && p < nwin) { S.wa[0][p] = ra0; S.wa[1][p] = ra1; S.wa[2][p] = ra2; S.wa[3][p] = ra3; }
    dirty = false;
  };
  // chunk pb = p0 + 1 in registers too (pb < 0: none): a task whose demand no host of chunk p0
  // fits usually finds its winner there
  double rb0 = 0.0, rb1 = 0.0, rb2 = 0.0, rb3 = 0.0;
  int32_t bid = 0;
  uint64_t bzm = 0, bvalid = 0;
  bool bdirty = false;
  int pb = -1;
  auto load_b = [&](int c) {
    bdirty = false;
    if (c >= nch) { pb = -1; bvalid = 0; bzm = 0; return; }
    pb = c;
    const int p = c * 64 + lane;
    const int q = min(p, nwin - 1);
    rb0 = S.wa[0][q]; rb1 = S.wa[1][q]; rb2 = S.wa[2][q]; rb3 = S.wa[3][q];
    bid = S.wid[q];
    bvalid = __ballot(p < nwin);
    bzm = cur >= 0 ? rfl_u64(S.zm[c]) : 0;
    __builtin_amdgcn_s_waitcnt(0xc07f);
  };
  auto store_b = [&]() {
    const int p = pb * 64 + lane;
    if (bdirty && pb >= 0 && p < nwin) { S.wa[0][p] = rb0; S.wa[1][p] = rb1; S.wa[2][p] = rb2; S.wa[3][p] = rb3; }
    bdirty = false;
  };
  load_chunk(0);
  load_b(1);
  // task records, software-pipelined across 64-task batches: while batch b is walked, batch
  // b + 1's records and batch b + 2's chain positions are in flight (no HBM latency at a batch
  // start)
  auto task_at = [&](int i) { return i < nt ? (KEYED ? i : gcmap[i]) : 0; };
  // a task's anchor (WIDE: its local id; the prologue checked every chain task's anchor, and a
  // lane past the chain's end reads task 0's, which no test looks at)
  auto anc_at = [&](int w) -> int {
    const int a = A.anc[w];
    if constexpr (WIDE) return W->zl[min((uint32_t)a, (uint32_t)(ZWIDE - 1))];
    else return a;
  };
  int nw = task_at(lane);
  double nd0 = A.dem[(size_t)nw * 4 + 0], nd1 = A.dem[(size_t)nw * 4 + 1];
  double nd2 = A.dem[(size_t)nw * 4 + 2], nd3 = A.dem[(size_t)nw * 4 + 3];
  int nanc = anc_at(nw), ncal = A.ord[nw];
  // run lengths from the order launch (the fast prologue's instance, where the driver has them):
  // loaded with the batch's records
  const bool rrm = FAST && A.run_rem != nullptr;
  int nrr = rrm ? A.run_rem[nw] : 0;
  int nw1 = task_at(64 + lane);
  int carry = 0;                             // tasks from this batch on that a run of an earlier one placed (64 and more: whole batches)
  // The batch's log (WinRec; sup: epoch_final_kernel) goes to HBM at the head of the NEXT batch,
  // between the copy of that batch's prefetched records and the loads for the one after it (the
  // last batch's after the loop): the record wait at a batch head then has only operations a
  // whole batch old before it. Stored right after its batch, behind the loads just issued, the
  // log's stores were what the next head's vmcnt wait stood on.
  // The log is a ring of ZW_LOGN positions, a task's entry at its chain position & (ZW_LOGN - 1):
  // a run writes ahead of its batch, at most 64 + ZW_RMAX positions past the oldest unflushed one
  // (everything before the current batch is flushed at its head), so it never laps the ring. A
  // batch that a run covered whole walks nothing and is flushed like any other.
  // Hosts: a single task's winner writes its host at the task's position, a run's taking lanes at
  // their first positions (run_bulk); every other position of the ring holds ZW_SAME (a batch's
  // slots are reset after its flush) and takes the host of the last written position at or before
  // it -- the run's taking lanes fill consecutive ranges in lane order, so that is its host.
  // Positions before the batch's first written one continue a run from an earlier batch: the
  // host of the last batch's position 63 (fprev, handed on from batch to batch).
  int fk = 0, ftw = 0, fcal = 0, fkb = 0;    // the unflushed batch: entries, its tasks' tw / tcal, its ring slots
  int32_t fprev = 0;
  static_assert(ZW_LOGN % 64 == 0, "the ring holds whole batches");
#pragma unroll
  for (int q = 0; q < ZW_LOGN; q += 64) S.lgid[q + lane] = ZW_SAME;
  auto flush_log = [&]() {
    if (UNI(fk > 0)) {
      const int32_t raw = S.lgid[fkb + lane];
      const uint64_t upto = __ballot(raw != ZW_SAME) & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull));
      const int32_t from = __shfl(raw, upto ? 63 - __builtin_clzll(upto) : 0);
      const int32_t id = upto ? from : fprev;
      fprev = __builtin_amdgcn_readlane(id, 63);
      if (lane < fk) {
        WinRec& e = A.wlog[ftw];
        e.s = 0.0;
        e.id = id;
        e.a[0] = S.lg[fkb + lane][0]; e.a[1] = S.lg[fkb + lane][1];
        e.a[2] = S.lg[fkb + lane][2]; e.a[3] = S.lg[fkb + lane][3];
        A.placement[fcal] = id;
      }
      S.lgid[fkb + lane] = ZW_SAME;          // (the slots' next batch starts from "as before")
    }
  };
  for (int i0 = 0; UNI(i0 < nt && !failed); i0 += 64) {
    st.batch_part_begins();
#pragma unroll
    for (int r = 0; r < 4; r++) mn[r] = S.smin[min(i0 >> 6, ZW_SB - 1)][r];
    const int tw = nw;
    const double td[4] = {nd0, nd1, nd2, nd3};
    const int tanc = nanc;
    const int tcal = ncal;
    const int trr = nrr;
    const int kb = i0 & (ZW_LOGN - 1);       // the batch's ring slots [kb, kb + 64)
    // (the record wait, explicit and ahead of the stores: left to the compiler it lands at the
    // records' first use, behind the flush, and waits for the stores just issued)
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    __builtin_amdgcn_s_waitcnt(0x0f70);      // vmcnt(0)
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    flush_log();
    __atomic_signal_fence(__ATOMIC_SEQ_CST);   // (this batch's runs may write the slots just flushed)
    if (i0 + 64 < nt) {                     // (uniform) batch b + 1's records, b + 2's positions
      nw = nw1;
      nd0 = A.dem[(size_t)nw * 4 + 0]; nd1 = A.dem[(size_t)nw * 4 + 1];
      nd2 = A.dem[(size_t)nw * 4 + 2]; nd3 = A.dem[(size_t)nw * 4 + 3];
      nanc = anc_at(nw); ncal = A.ord[nw];
      if (rrm) nrr = A.run_rem[nw];
      nw1 = task_at(i0 + 128 + lane);
    }
    const int kn = min(64, nt - i0);
    // (uniform) every task of the batch has the anchor the zero-cost masks are for: the tasks
    // need no anchor test (a chain's groups are long, so nearly every batch)
    bool uni = __ballot(lane < kn && tanc != cur) == 0;
    // runs: bit i is set iff task i of the batch has task i - 1's demand vector, bit for bit (the
    // trace has few distinct demand rows, and sorted order puts equal ones next to each other)
    // (not evaluated where the run lengths come with the records)
    uint64_t E = 0;
    if (!rrm) {
      bool same = lane > 0 && lane < kn;
#pragma unroll
      for (int r = 0; r < 4; r++)
        same &= __double_as_longlong(__shfl_up(td[r], 1)) == __double_as_longlong(td[r]);
      E = __ballot(same);
      // (chain mode: a run stops at a group segment start -- pass 2 logs a host's capacities
      // at its last copy of the run only, and the segment before must hold its own last copy)
      if (segm) E &= ~rfl_u64(S.sbits[i0 >> 6]);
    }
    st.batch_runs(E, i0, kn, lane, td[0], td[1], td[2], td[3], tanc, trr, rrm, segm, S.sbits);
    // A run that reaches the end of a full batch goes on into the next one while those tasks
    // have the same demand vector and anchor and no segment starts (their records are already in
    // registers, nd*): at most 64 tasks per run on this path, the ones past the batch logged
    // ahead in the ring and counted in carry.
    int extc = -1;
    auto ext_len = [&]() -> int {
      if (extc < 0) {
        extc = 0;
        if (kn == 64 && i0 + 64 < nt && uni) {
          const int kn2 = min(64, nt - i0 - 64);
          const double l0 = readlane_d(td[0], 63), l1 = readlane_d(td[1], 63);
          const double l2 = readlane_d(td[2], 63), l3 = readlane_d(td[3], 63);
          bool eq = lane < kn2 && readlane_i(tanc, 63) == nanc &&
                    __double_as_longlong(nd0) == __double_as_longlong(l0) &&
                    __double_as_longlong(nd1) == __double_as_longlong(l1) &&
                    __double_as_longlong(nd2) == __double_as_longlong(l2) &&
                    __double_as_longlong(nd3) == __double_as_longlong(l3);
          if (segm) eq = eq && !((rfl_u64(S.sbits[(i0 >> 6) + 1]) >> lane) & 1ull);
          const uint64_t m = __ballot(eq);
          extc = m == ~0ull ? 64 : __builtin_ctzll(~m);
        }
        extc = __builtin_amdgcn_readfirstlane(extc);
      }
      return extc;
    };
    // With the order launch's run lengths a run is the rest of its stretch of identical rows
    // inside its group (so it ends at a segment start: the fast prologue's segments are whole
    // groups, all of one anchor), ZW_RMAX tasks at the most; a longer one takes another call.
    auto run_len = [&](int k) {
      if (rrm) return min(min(readlane_i(trr, k), ZW_RMAX), nt - i0 - k);
      int r = k < 63 ? min(kn - k, 1 + __builtin_ctzll(~(E >> (k + 1)))) : 1;
      if (k + r == 64) r = min(64, r + ext_len());
      return r;
    };
    // The run step, for a task k of a uniform batch that the register chunk p0 cannot take: its
    // run (R tasks with its demand, R >= 1) is placed by run_bulk on the first chunk that can
    // take a copy of it -- chunk p0 (moved on past chunks no task ahead can use), chunk pb, then
    // the LDS chunks in index order -- with the per-task path's exactness conditions: every
    // chunk before it fits no copy (for the chunks before p0: no task ahead), and no fitting
    // host of a chunk it looks at is outside the anchor's zero-cost zones (else 0: the per-task
    // path decides, with exact scores). Returns the tasks placed (0: none).
    auto run_step = [&](int k) -> int {
      st.search_begins();
      const double d0 = readlane_d(td[0], k), d1 = readlane_d(td[1], k);
      const double d2 = readlane_d(td[2], k), d3 = readlane_d(td[3], k);
      const int R = run_len(k);
      for (;;) {
        const double n0 = ra0 - d0, n1 = ra1 - d1, n2 = ra2 - d2, n3 = ra3 - d3;
        uint64_t fm = __ballot(fit_res<STRICT>(fmin(fmin(n0, n1), fmin(n2, n3)))) & rvalid;
        if (FF) fm &= rzm;                     // (FF: other fitting hosts have key > 0)
        if (!FF && UNI((fm & ~rzm) != 0)) return 0;
        if (UNI(fm != 0)) {
          dirty = true;
          st.search_ends();
          return zw_run_bulk<STRICT>(S, st, ra0, ra1, ra2, ra3, rid, d0, d1, d2, d3, fm, R, kb + k);
        }
        if (__ballot(((rvalid >> lane) & 1ull) && fits<STRICT>(ra0, ra1, ra2, ra3, mn[0], mn[1], mn[2], mn[3])))
          break;                               // chunk p0 can still take a task ahead
        if (p0 + 1 >= nch) return 0;
        store_b();                             // dead: move the register chunks on
        store_chunk(p0);
        ++p0;
        rzm = rfl_u64(S.zm[p0]);
        load_chunk(p0);
        load_b(p0 + 1);
      }
      if (pb >= 0) {
        const double q0 = rb0 - d0, q1 = rb1 - d1, q2 = rb2 - d2, q3 = rb3 - d3;
        uint64_t fb = __ballot(fit_res<STRICT>(fmin(fmin(q0, q1), fmin(q2, q3)))) & bvalid;
        if (FF) fb &= bzm;
        if (!FF && UNI((fb & ~bzm) != 0)) return 0;
        if (UNI(fb != 0)) {
          bdirty = true;
          st.search_ends();
          return zw_run_bulk<STRICT>(S, st, rb0, rb1, rb2, rb3, bid, d0, d1, d2, d3, fb, R, kb + k);
        }
      }
      for (int c = (pb >= 0 ? pb : p0) + 1; c < nch; c++) {
        const int p = c * 64 + lane;
        const int q = min(p, nwin - 1);
        double x0 = S.wa[0][q], x1 = S.wa[1][q], x2 = S.wa[2][q], x3 = S.wa[3][q];
        const int32_t xid = S.wid[q];
        const uint64_t xzm = rfl_u64(S.zm[c]);
        st.probe();
        uint64_t fm = __ballot(p < nwin && fit_res<STRICT>(fmin(fmin(x0 - d0, x1 - d1),
                                                                fmin(x2 - d2, x3 - d3))));
        if (FF) fm &= xzm;
        if (!FF && UNI((fm & ~xzm) != 0)) return 0;
        if (UNI(fm != 0)) {
          st.search_ends();
          const int got = zw_run_bulk<STRICT>(S, st, x0, x1, x2, x3, xid, d0, d1, d2, d3, fm, R, kb + k);
          if (p < nwin) { S.wa[0][p] = x0; S.wa[1][p] = x1; S.wa[2][p] = x2; S.wa[3][p] = x3; }
          if (!KEYED && lane == 0) S.touch[c] = 1;
          return got;
        }
      }
      st.search_ends();
      return 0;
    };
    st.batch_part_ends();
    int k = carry;                           // (>= kn: a run covered the batch whole, nothing to walk)
    while (UNI(k < kn)) {
      // (wave-uniform state the compiler cannot prove uniform: keeps the loops below scalar)
      k = __builtin_amdgcn_readfirstlane(k);
      p0 = __builtin_amdgcn_readfirstlane(p0);
      pb = __builtin_amdgcn_readfirstlane(pb);
      done = __builtin_amdgcn_readfirstlane(done);
      rzm = rfl_u64(rzm);
      bzm = rfl_u64(bzm);
      // The hot loop: the batch's tasks while each finds a fitting zero-cost host in the
      // register chunk and every fitting host of it is zero-cost for the anchor. Per task: the
      // demand from registers, four subtractions, three minima, one ballot, the winner's mask
      // bit (lowest set bit, scalar), four selects on it and the winner lane's log entry -- no
      // compare of a lane id and no branch back to the vector unit. Any other task leaves it for
      // the general step below, then the hot loop goes on.
      if (uni) {
        for (; k < kn;) {
          k = __builtin_amdgcn_readfirstlane(k);
          const double d0 = readlane_d(td[0], k), d1 = readlane_d(td[1], k);
          const double d2 = readlane_d(td[2], k), d3 = readlane_d(td[3], k);
          const double n0 = ra0 - d0, n1 = ra1 - d1, n2 = ra2 - d2, n3 = ra3 - d3;
          const uint64_t fm0 = __ballot(fit_res<STRICT>(fmin(fmin(n0, n1), fmin(n2, n3)))) & rvalid;
          const uint64_t m0 = fm0 & rzm;
          if (UNI(m0 == 0 || (!FF && (fm0 & ~rzm) != 0))) break;
          // a run of tasks with this demand: placed in one pass over the chunk (run_bulk)
          const int R = run_len(k);
          if (UNI(R >= ZW_RMIN)) {
            const int c = zw_run_bulk<STRICT>(S, st, ra0, ra1, ra2, ra3, rid, d0, d1, d2, d3, m0, R, kb + k);
            k += c;
            done += c;
            dirty = true;
            st.run_placed(c);
            continue;
          }
          const bool win = __builtin_amdgcn_inverse_ballot_w64(m0 & (0ull - m0));
          ra0 = win ? n0 : ra0; ra1 = win ? n1 : ra1; ra2 = win ? n2 : ra2; ra3 = win ? n3 : ra3;
          if (win) {
            zw_log_entry(S, kb + k, rid, n0, n1, n2, n3);
          }
          dirty = true;
          st.single_placed();
          done++;
          k++;
        }
        if (UNI(k >= kn)) break;
        const int got = run_step(k);
        st.run_placed(got);                    // (0: none, not counted)
        if (UNI(got > 0)) {
          k += got;
          done += got;
          continue;
        }
      }
      const double d0 = readlane_d(td[0], k), d1 = readlane_d(td[1], k);
      const double d2 = readlane_d(td[2], k), d3 = readlane_d(td[3], k);
      const int a = uni ? cur : readlane_i(tanc, k);
      if (a != cur) {
        // certificates 2 / 3 for this anchor's zone row
        bool ok = true;
        if (!KEYED && lane < Z) {
          const double c = S.csum[a * Z + lane], bw = S.bsum[a * Z + lane];
          if (c == 0.0) ok = bw > 0.0;
          // (bw > 0: a negative bandwidth would give a negative key, ahead of every zero key)
          else if (FF || !((U >> lane) & 1u)) ok = (c >= CERT_C_MIN) && (bw > 0.0) && (bw <= CERT_BW_MAX);
        }
        if (__ballot(!ok)) { failed = true; break; }
        const uint32_t am = KEYED ? ~0u : S.amask[a];   // keyed: every prefix host is zero-key
        for (int c = 0; c < nch; c++) {
          const int p = c * 64 + lane;
          const uint64_t m = __ballot(p < nwin && (KEYED || ((am >> S.wz[min(p, nwin - 1)]) & 1u)));
          if (lane == 0) S.zm[c] = m;
          if (c == p0) rzm = m;
          if (c == pb) bzm = m;
        }
        cur = a;
        uni = __ballot(lane >= k && lane < kn && tanc != cur) == 0;   // the rest of the batch
        __builtin_amdgcn_s_waitcnt(0xc07f);
        st.anchor_switched();
      }
      // exact scores for this lane's host when it fits but is not zero-cost for `a`
      auto zero_exact = [&](bool f, bool k0, double a0, double a1, double a2, double a3, int q) {
        if (FF) return k0;                   // (first-fit: a fitting host of another zone has key > 0)
        if (__builtin_expect(__ballot(f && !k0) != 0, 0)) {
          if (f && !k0) {
            const int z = S.wz[q];
            const double s2 = norm2_seq(a0 - d0, a1 - d1, a2 - d2, a3 - d3);
            const double sc = (S.csum[a * Z + z] * __builtin_sqrt(s2)) / S.bsum[a * Z + z];
            k0 = __double_as_longlong(sc) == 0;
          }
        }
        return k0;
      };
      // Hot path, straight-line: the register chunk holds a fitting zero-cost host and every
      // fitting host of it is zero-cost for this anchor. The fit test is the minimum residual:
      // every window capacity and chain demand is finite with |x| <= 2^500 (certificate 3), so
      // a - d is exact in sign (a >= d iff a - d >= +-0) and is the capacity after a commit.
      const double n0 = ra0 - d0, n1 = ra1 - d1, n2 = ra2 - d2, n3 = ra3 - d3;
      // (keyed first-fit: strict fit, a > d iff a - d > 0)
      const uint64_t fm0 = __ballot(fit_res<STRICT>(fmin(fmin(n0, n1), fmin(n2, n3)))) & rvalid;
      bool found = true;
      st.chunk_scanned();
      // Each path commits in place (no shared commit block: merging the paths made the compiler
      // copy the chunk registers on every task). commit: resc[h] -= t_demand
      // (cost_aware.py:95) on the lowest such lane, which logs.
      // (the winner's lane from its mask bit in scalar registers: no lane-id compare, and the
      // commit is four selects on that mask)
      const uint64_t m0 = fm0 & rzm;
      if (__builtin_expect(m0 != 0 && (FF || (fm0 & ~rzm) == 0), 1)) {
        const bool win = __builtin_amdgcn_inverse_ballot_w64(m0 & (0ull - m0));
        ra0 = win ? n0 : ra0; ra1 = win ? n1 : ra1; ra2 = win ? n2 : ra2; ra3 = win ? n3 : ra3;
        if (win) {
          zw_log_entry(S, kb + k, rid, n0, n1, n2, n3);
        }
        dirty = true;
      } else {
        bool inb = false;
        if (fm0 == 0 && pb >= 0) {
          // no host of chunk p0 fits this task: its winner is chunk pb's first fitting zero-cost
          // host, from registers (a dead chunk p0 is moved on by the general path below)
          const double q0 = rb0 - d0, q1 = rb1 - d1, q2 = rb2 - d2, q3 = rb3 - d3;
          const uint64_t fb = __ballot(fit_res<STRICT>(fmin(fmin(q0, q1), fmin(q2, q3)))) & bvalid;
          const uint64_t mb = fb & bzm;
          if (mb != 0 && (FF || (fb & ~bzm) == 0)) {
            const bool win = __builtin_amdgcn_inverse_ballot_w64(mb & (0ull - mb));
            rb0 = win ? q0 : rb0; rb1 = win ? q1 : rb1; rb2 = win ? q2 : rb2; rb3 = win ? q3 : rb3;
            if (win) {
              zw_log_entry(S, kb + k, bid, q0, q1, q2, q3);
            }
            bdirty = true;
            inb = true;
          }
        }
        if (!inb) {                            // the general path
          found = false;
          store_b();                           // it works on LDS from p0 + 1 on
          double g0 = n0, g1 = n1, g2 = n2, g3 = n3;
          uint64_t fm = fm0, m = fm0 & rzm;
          for (;;) {                           // the register chunk (advancing past dead ones)
            if (fm & ~rzm)                     // fitting hosts of U outside the anchor's
              m = __ballot(zero_exact((fm >> lane) & 1ull, (rzm >> lane) & 1ull, ra0, ra1, ra2,
                                      ra3, min(p0 * 64 + lane, nwin - 1))) & fm;   // zero-cost zones
            if (m) {
              const bool win = lane == __builtin_ctzll(m);
              ra0 = win ? g0 : ra0; ra1 = win ? g1 : ra1; ra2 = win ? g2 : ra2; ra3 = win ? g3 : ra3;
              if (win) {
                zw_log_entry(S, kb + k, rid, g0, g1, g2, g3);
              }
              dirty = true;
              found = true;
              break;
            }
            if (__ballot(((rvalid >> lane) & 1ull) && fits<STRICT>(ra0, ra1, ra2, ra3, mn[0], mn[1], mn[2], mn[3])))
              break;                           // chunk p0 still useful: look further in LDS
            store_chunk(p0);                   // dead: move the register chunk on
            if (++p0 >= nch) break;
            rzm = rfl_u64(S.zm[p0]);
            load_chunk(p0);
            g0 = ra0 - d0; g1 = ra1 - d1; g2 = ra2 - d2; g3 = ra3 - d3;
            fm = __ballot(fit_res<STRICT>(fmin(fmin(g0, g1), fmin(g2, g3)))) & rvalid;
            m = fm & rzm;
            st.chunk_scanned();
          }
          if (!found && p0 < nch) {
            store_chunk(p0);
            for (int c = p0 + 1; c < nch; c++) {
              st.chunk_scanned();
              const int p = c * 64 + lane;
              const int q = min(p, nwin - 1);
              const double a0 = S.wa[0][q], a1 = S.wa[1][q], a2 = S.wa[2][q], a3 = S.wa[3][q];
              const int32_t id = S.wid[q];
              const uint64_t zm = rfl_u64(S.zm[c]);
              const bool f = p < nwin && fits<STRICT>(a0, a1, a2, a3, d0, d1, d2, d3);
              const bool k0 = zero_exact(f, (zm >> lane) & 1ull, a0, a1, a2, a3, q);
              const uint64_t mc = __ballot(f && k0);
              if (mc) {
                if (lane == __builtin_ctzll(mc)) {
                  const double c0 = a0 - d0, c1 = a1 - d1, c2 = a2 - d2, c3 = a3 - d3;
                  S.wa[0][q] = c0; S.wa[1][q] = c1; S.wa[2][q] = c2; S.wa[3][q] = c3;
                  zw_log_entry(S, kb + k, id, c0, c1, c2, c3);
                  if (!KEYED) S.touch[c] = 1;
                }
                found = true;
                break;
              }
            }
          }
          wave_lds_sync();
          load_b(p0 + 1);
        }
      }
      if (UNI(!found)) {                     // certificate 1 fails: the list walk decides --
        failed = true;                       // or, when the window is full, a larger one may do
        exhausted = nwin >= WM;
        break;
      }
      done++;
      k++;
    }
    st.batch_part_begins();
    fk = __builtin_amdgcn_readfirstlane(min(k, kn));
    fkb = kb;
    ftw = tw;
    fcal = tcal;
    carry = __builtin_amdgcn_readfirstlane(k > kn ? k - kn : 0);
    st.batch_part_ends();
  }
  flush_log();                               // the last batch walked
  if (KEYED) {   // the window's capacities to global availability: the keyed path goes on there
    store_chunk(p0);
    store_b();
    wave_lds_sync();
    for (int p = lane; p < nwin; p += 64) {
      const int h = S.wid[p];
#pragma unroll
      for (int r = 0; r < 4; r++) A.wb[(size_t)r * H + h] = S.wa[r][p];
    }
  }
  if (!KEYED && A.undo && !failed && done == nt) {
    // optimistic apply: the chain walked all its tasks, so its window holds each host's state after
    // the chain's last commit to it -- what the epoch's apply would rebuild from the log. The
    // chunks the walk committed to (the register chunks' range, and those marked in LDS) go to
    // global availability; the driver undoes it (ZwUndo) if the epoch is not accepted whole.
    store_chunk(p0);
    store_b();
    wave_lds_sync();
    const int top = max(p0, pb);
    for (int c = 0; c < nch; c++) {
      if (c > top && !S.touch[c]) continue;
      const int p = c * 64 + lane;
      if (p < nwin) {
        const int h = S.wid[p];
#pragma unroll
        for (int r = 0; r < 4; r++) A.wb[(size_t)r * H + h] = S.wa[r][p];
      }
    }
  }
  // status[0]: tasks proven (their log entries are exact; validation accepts them), status[1]:
  // 1 when a certificate failed there (the rest of the chain is left to the list walk)
  if (lane == 0) report(done, (failed && !KEYED) ? (exhausted ? 2 : 1) : 0);
  if (lane == 0) st.add_to(A.stamps, b, done, nt);
}

#ifdef PVT_ZWALK_WIDE_TU
// ---- rounds of more than ZMAX zones (this section alone is compiled into pvt_zwalk_wide.hip)
void launch_zwalk_wide(const ZwalkArgs& a, int nchains, bool big, hipStream_t st) {
  if (big) PVT_LAUNCH((zwalk_kernel<false, false, false, -ZW_MBIG>), dim3(nchains), dim3(ZW_THREADS), 0, st, a);
  else PVT_LAUNCH((zwalk_kernel<false, false, false, -ZW_M>), dim3(nchains), dim3(ZW_THREADS), 0, st, a);
}
void launch_zwalk_ff_wide(const ZwalkArgs& a, int nchains, hipStream_t st) {
  PVT_LAUNCH((zwalk_kernel<false, true, true, -ZW_M>), dim3(nchains), dim3(ZW_THREADS), 0, st, a);
}

// The zero pairs of the sum table (the driver's components of a wide round): block a scans row a
// for z > a; a pair takes a slot from the counter in pairs[0].
__global__ __launch_bounds__(256) void zero_pairs_kernel(const double* csum, int Z, int32_t* pairs,
                                                         int cap) {
  const int a = blockIdx.x;
  for (int z = a + 1 + threadIdx.x; z < Z; z += 256) {
    if (csum[a * Z + z] == 0.0) {
      const int slot = atomicAdd(&pairs[0], 1);
      if (slot < cap) pairs[1 + slot] = (a << 16) | z;
    }
  }
}
void launch_zero_pairs(const double* csum, int Z, int32_t* pairs, int cap, hipStream_t st) {
  (void)hipMemsetAsync(pairs, 0, sizeof(int32_t), st);
  PVT_LAUNCH(zero_pairs_kernel, dim3(Z), dim3(256), 0, st, csum, Z, pairs, cap);
}
#else
void launch_host_min(const double* avail, int H, int lo, int hi, double* part, hipStream_t st) {
  PVT_LAUNCH(host_min_kernel, dim3(ZW_MINB), dim3(256), 0, st, avail, H, lo, hi, part);
}

void launch_zwalk(const ZwalkArgs& a, int nchains, hipStream_t st) {
  if (a.cert.fast && a.tab.nch > 0 && a.zpre && !a.pwin)
    PVT_LAUNCH((zwalk_kernel<false, false, false, ZW_M, true>), dim3(nchains), dim3(ZW_THREADS), 0, st, a);
  else
    PVT_LAUNCH((zwalk_kernel<false, false>), dim3(nchains), dim3(ZW_THREADS), 0, st, a);
}
void launch_zwalk_big(const ZwalkArgs& a, int nchains, hipStream_t st) {
  PVT_LAUNCH((zwalk_kernel<false, false, false, ZW_MBIG>), dim3(nchains), dim3(ZW_THREADS), 0, st, a);
}
void launch_zwalk_ff(const ZwalkArgs& a, int nchains, hipStream_t st) {
  PVT_LAUNCH((zwalk_kernel<false, true, true>), dim3(nchains), dim3(ZW_THREADS), 0, st, a);
}

// Per-dimension maxima of |avail| over hosts [lo, hi) (the FF walk's certificate 2'), in
// host_min_kernel's partial layout.
__global__ __launch_bounds__(256) void host_absmax_kernel(const double* avail, int H, int lo, int hi,
                                                          double* part) {
  __shared__ double red[4][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double m[4] = {0.0, 0.0, 0.0, 0.0};
  for (int h = lo + blockIdx.x * 256 + tid; h < hi; h += gridDim.x * 256)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      m[r] = nan_max(m[r], __builtin_fabs(avail[(size_t)r * H + h]));   // (NaN propagates:
    }                                                                     //  no certificate)
#pragma unroll
  for (int r = 0; r < 4; r++) {
    m[r] = wave_nmax_d(m[r]);
    if (lane == 0) red[wave][r] = m[r];
  }
  __syncthreads();
  if (tid < 4) {
    double v = red[0][tid];
    for (int w = 1; w < 4; w++) v = nan_max(v, red[w][tid]);
    part[blockIdx.x * 4 + tid] = v;
  }
}
void launch_host_absmax(const double* avail, int H, int lo, int hi, double* part, hipStream_t st) {
  PVT_LAUNCH(host_absmax_kernel, dim3(ZW_MINB), dim3(256), 0, st, avail, H, lo, hi, part);
}
void launch_zwalk_keyed(const ZwalkArgs& a, bool strict, hipStream_t st) {
  if (strict) PVT_LAUNCH((zwalk_kernel<true, true>), dim3(1), dim3(ZW_THREADS), 0, st, a);
  else PVT_LAUNCH((zwalk_kernel<true, false>), dim3(1), dim3(ZW_THREADS), 0, st, a);
}

// Ordered frontier: the smallest demand (per dimension) of tasks [0, n), then the hosts that
// fit it (the alive hosts: no other can fit any of those tasks), as flags for a compaction.
__global__ __launch_bounds__(1024) void dem_min_kernel(const double* dem, int n, double* out) {
  __shared__ double red[16][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double m[4] = {DINF, DINF, DINF, DINF};
  for (int i = tid; i < n; i += 1024)
#pragma unroll
    for (int r = 0; r < 4; r++) m[r] = fmin(m[r], dem[(size_t)i * 4 + r]);
#pragma unroll
  for (int r = 0; r < 4; r++) {
    m[r] = wave_min_d(m[r]);
    if (lane == 0) red[wave][r] = m[r];
  }
  __syncthreads();
  if (tid < 4) {
    double v = red[0][tid];
    for (int w = 1; w < 16; w++) v = fmin(v, red[w][tid]);
    out[tid] = v;
  }
}
__global__ void alive_flags_kernel(const double* avail, int H, int lo, int hs, const double* dmin,
                                   int strict, uint8_t* flags) {
  const int h = lo + blockIdx.x * blockDim.x + threadIdx.x;
  if (h >= hs) return;
  const double a0 = avail[h], a1 = avail[(size_t)H + h], a2 = avail[2 * (size_t)H + h],
               a3 = avail[3 * (size_t)H + h];
  flags[h - lo] = strict ? fits<true>(a0, a1, a2, a3, dmin[0], dmin[1], dmin[2], dmin[3])
                    : fits<false>(a0, a1, a2, a3, dmin[0], dmin[1], dmin[2], dmin[3]);
}
void launch_alive_flags(const double* avail, int H, int lo, int hs, const double* dem, int n,
                        int strict, double* dmin, uint8_t* flags, hipStream_t st) {
  PVT_LAUNCH(dem_min_kernel, dim3(1), dim3(1024), 0, st, dem, n, dmin);
  if (hs <= lo) return;
  PVT_LAUNCH(alive_flags_kernel, dim3((hs - lo + 255) / 256), dim3(256), 0, st, avail, H,
                     lo, hs, dmin, strict, flags);
}

// ---- host-sharded frontier walks: a rank's window candidates, and their merge

// Chain b of the epoch: its zero-cost zones U (the union of its anchors' zero-cost zones, as the
// walk computes them) and the first ZW_M hosts of U in this rank's range [lo, hi), index order,
// with their capacities; block 0 also stamps the package header.
__global__ __launch_bounds__(ZW_THREADS) void zwin_build_kernel(ZwinArgs A) {
  __shared__ uint32_t amask[ZMAX];
  __shared__ uint32_t umask;
  __shared__ int32_t cnt[ZW_SCAN][ZW_WAVES];
  __shared__ int32_t nwin;
  const int b = blockIdx.x, tid = threadIdx.x, Z = A.Z;
  FrontierSlot* out = A.out + b;
  if (tid == 0) { umask = 0; nwin = 0; }
  if (tid < Z) {
    uint32_t m = 0;
    for (int z = 0; z < Z; z++) m |= (A.csum[tid * Z + z] == 0.0) ? (1u << z) : 0u;
    amask[tid] = m;
  }
  __syncthreads();
  uint32_t um = 0;
  for (int i = A.coff[b] + tid; i < A.coff[b + 1]; i += ZW_THREADS) {
    const int a = A.anc[A.cmap[i]];
    if (a >= 0 && a < Z) um |= amask[a];    // (a bad anchor: the walk bails on it)
  }
  if (um) atomicOr(&umask, um);
  __syncthreads();
  compact_zone_window(A.zone, Z, umask, A.lo, A.hi, out->id, nullptr, cnt, &nwin);
  const int n = nwin;
  for (int p = tid; p < n; p += ZW_THREADS) {
    const int h = out->id[p];
#pragma unroll
    for (int r = 0; r < 4; r++) out->a[r][p] = A.avail[(size_t)r * A.H + h];
  }
  if (tid == 0) { out->n = n; out->total = n; }
}

__global__ __launch_bounds__(256) void zwin_gather_kernel(const double* avail, int H, int lo,
                                                          const int32_t* perm, const int32_t* count,
                                                          FrontierSlot* out) {
  const int c = *count, n = min(c, ZW_M);
  for (int p = threadIdx.x; p < n; p += 256) {
    const int h = lo + perm[p];
    out->id[p] = h;
#pragma unroll
    for (int r = 0; r < 4; r++) out->a[r][p] = avail[(size_t)r * H + h];
  }
  if (threadIdx.x == 0) { out->n = n; out->total = c; }
}

// Block b < nslots: slot b of every rank, concatenated in rank order and cut at ZW_M (ranks own
// ascending ranges, so this is the index-order window); block nslots: the host-minimum partials,
// the minimum over ranks.
__global__ __launch_bounds__(256) void zwin_merge_kernel(const uint8_t* pkgs, int64_t pkg_bytes,
                                                         int world, int nslots, FrontierSlot* out,
                                                         double* hmin) {
  __shared__ int32_t off[PVT_SHARD_MAX_WORLD + 1];
  const int b = blockIdx.x, tid = threadIdx.x;
  auto hdr = [&](int k) { return reinterpret_cast<const FrontierHdr*>(pkgs + (size_t)k * pkg_bytes); };
  if (b == nslots) {               // (keyed / ordered walks: hmin NULL, no minima exchanged)
    for (int i = tid; hmin && i < ZW_MIN_PARTS * 4; i += 256) {
      double m = DINF;
      for (int k = 0; k < world; k++) m = fmin(m, (&hdr(k)->hmin[0][0])[i]);
      (&hmin[0])[i] = m;
    }
    return;
  }
  auto slot = [&](int k) { return reinterpret_cast<const FrontierSlot*>(hdr(k) + 1) + b; };
  if (tid == 0) {
    int o = 0, tot = 0;
    for (int k = 0; k < world; k++) { off[k] = o; o += slot(k)->n; tot += slot(k)->total; }
    off[world] = o;
    out[b].n = min(o, ZW_M);
    out[b].total = tot;
  }
  __syncthreads();
  for (int k = 0; k < world && off[k] < ZW_M; k++) {
    const FrontierSlot* s = slot(k);
    const int n = min(s->n, ZW_M - off[k]);
    for (int p = tid; p < n; p += 256) {
      const int q = off[k] + p;
      out[b].id[q] = s->id[p];
#pragma unroll
      for (int r = 0; r < 4; r++) out[b].a[r][q] = s->a[r][p];
    }
  }
}

void launch_zwin_build(const ZwinArgs& a, int nchains, hipStream_t st) {
  PVT_LAUNCH(zwin_build_kernel, dim3(nchains), dim3(ZW_THREADS), 0, st, a);
}
void launch_zwin_gather(const double* avail, int H, int lo, const int32_t* perm,
                        const int32_t* count, FrontierSlot* out, hipStream_t st) {
  PVT_LAUNCH(zwin_gather_kernel, dim3(1), dim3(256), 0, st, avail, H, lo, perm, count, out);
}
void launch_zwin_merge(const uint8_t* pkgs, int64_t pkg_bytes, int world, int nslots,
                       FrontierSlot* out, double* hmin, hipStream_t st) {
  PVT_LAUNCH(zwin_merge_kernel, dim3(nslots + 1), dim3(256), 0, st, pkgs, pkg_bytes, world,
                     nslots, out, hmin);
}
#endif  // PVT_ZWALK_WIDE_TU

}  // namespace pvt
