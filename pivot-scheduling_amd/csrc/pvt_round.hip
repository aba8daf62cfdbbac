// pvt_round.hip — the windowed round (pvt_capi.hip describes a round): the processing order,
// round_begin, and per window the candidate lists, the commit walk and the ordered frontier;
// place_pipelined overlaps scoring and walking, place_windowed is the entry for a checked round.
// Also the builders of the walks' and epochs' kernel arguments, shared with the epoch and
// sharded paths. The only driver file that instantiates hipcub.
#include <hipcub/hipcub.hpp>

#include <limits>

#include "pvt_driver.h"
#include "pvt_opp.h"
#include "pvt_groups.h"

// ---------------------------------------------------------------- round driver
// Host segments per task for the score pass: enough waves to fill 256 CUs (~16 per CU) when
// the window is short, at least 4096 hosts per segment, a multiple of 8 (one XCD per
// blockIdx % 8), capped by the segment-list scratch.
static constexpr size_t SEG_ENTRIES_MAX = (size_t)MAX_WINDOW * MAX_SEG * KL;
// vbp best-fit scores are continuous, so a segment's list keeps improving while it streams:
// about KL * (1 + ln(H / (S * KL))) serial insertions per segment, S times per task. Fewer,
// longer segments halve those insertions at 16 (measured: 29.7 -> 26.2 ms of score per
// 1M x 10k round); cost_aware's zero-cost zone fills its lists at once and wants the waves.
static int choose_segments(int H, int nt, int mode, int force_tw, bool epoch, int force_S, int Z) {
  const int tw = score_tasks_per_wave(mode, H, force_tw, Z);
  const int task_waves = (nt + tw - 1) / tw;
  int S = (4096 + task_waves - 1) / task_waves;
  if (mode == PVT_VBP_BF) S = std::min(S, 16);
  // cost_aware best-fit over many tasks (epochs): each segment fills its list from the zero-cost
  // zones' lowest-index hosts and exits early, so fewer, longer segments stream fewer hosts per
  // task -- but a merged list of S x 64 entries must stay deep enough for a whole group's walk
  // (config 5 ca_bf epoch of 10k tasks: S = 2 -> 5.6 ms, 4 -> 4.1, 8 -> 4.8; S = 2 refills;
  // config 3, 1k tasks: 8 -> 0.82 ms, 4 -> 0.73)
  if (mode == PVT_CA_BF && epoch) S = 4;
  if (force_S > 0) S = force_S;   // (PVT_SEGMENTS, read at context creation)
  S = std::min(S, std::max(1, H / 4096));
  S = std::min(S, std::max(MAX_SEG, (int)(SEG_ENTRIES_MAX / ((size_t)nt * KL))));
  S = std::max(1, std::min(S, 256));
  if (S >= 8) S = S / 8 * 8;
  return S;
}
// keyed first-fit scan depth: entries per task list (deeper lists, fewer refills)
static constexpr int KSCAN_DEPTH = 256;
// zero-key prefix used alone (no sort) when it holds at least this many hosts
static constexpr int KPREFIX_MIN = 1024;
double pvt::bytes_per_candidate(int mode) {
  // cost_aware 36 B (4 x fp64 avail + int32 zone); vbp best-fit 36 B
  // (+ host-id rank); opportunistic / vbp first-fit 32 B.
  return (mode == PVT_CA_FF || mode == PVT_CA_BF || mode == PVT_VBP_BF) ? 36.0 : 32.0;
}

// a2: processing order. Group-major (stable by group id), within a group caller order or, with
// sort_tasks, stable descending ||d||2. Two LSD passes of a stable radix sort.
// Processing order (a2). Grouped rounds take the optimistic path: group counts, offsets and the
// pinned copies of counts / anchors / cost table, then the per-group sorts, all launched with no
// synchronisation (*pending = true); the caller syncs once, later, and calls build_order_check.
// Spin on the count kernel's flag (the staged counts are visible once it holds flag_seq). Every
// 4096 polls the stream is queried: an idle stream with no flag is an error, never a hang.
static int wait_host_flag(pvt_ctx* ctx, volatile int32_t* f, int32_t seq, const char* what) {
  for (uint32_t n = 1;; n++) {
    if (__atomic_load_n(f, __ATOMIC_ACQUIRE) == seq) return PVT_OK;
    __builtin_ia32_pause();                   // (yield the core's pipeline to its sibling thread)
    if (n >= (1u << 18)) {
      // a long wait (the GPU is shared or the round is large): stop spinning and block on the
      // stream -- everything queued behind the kernel runs without the host
      HIPCHK(hipStreamSynchronize(ctx->stream));
      if (__atomic_load_n(f, __ATOMIC_ACQUIRE) == seq) return PVT_OK;
      return fail(ctx, PVT_EHIP, "%s: kernel finished without its flag", what);
    }
    if ((n & 4095) == 0) {
      const hipError_t e = hipStreamQuery(ctx->stream);
      if (e == hipSuccess) {
        if (__atomic_load_n(f, __ATOMIC_ACQUIRE) == seq) return PVT_OK;
        return fail(ctx, PVT_EHIP, "%s: kernel finished without its flag", what);
      }
      if (e != hipErrorNotReady) return fail(ctx, PVT_EHIP, "%s: %s", what, hipGetErrorString(e));
    }
  }
}
static int wait_stage_flag(pvt_ctx* ctx) {
  return wait_host_flag(ctx, ctx->flag_host, ctx->flag_seq, "grouped order");
}

static int build_order_radix(pvt_ctx* ctx, const pvt_round* r, int32_t** ord_out);
// hmin (or NULL): the frontier walk's host minima, written by the order's launch when it can
// (*hmin_done); stage_flag: the host then waits on ctx->flag_host instead of ev_stage.
static int build_order(pvt_ctx* ctx, const pvt_round* r, int32_t** ord_out, bool* pending,
                       double* hmin = nullptr, bool* hmin_done = nullptr,
                       ZoneWindows* zwin = nullptr) {
  *pending = false;
  if (hmin_done) *hmin_done = false;
  ctx->rs.stage_flag = false;
  const int T = r->n_tasks;
  hipStream_t st = ctx->stream;
  ENSURE(ctx->ord, sizeof(int32_t) * T);
  ENSURE(ctx->ord2, sizeof(int32_t) * T);
  int32_t* cur = P<int32_t>(ctx->ord);
  const bool grouped = r->task_group != nullptr && r->n_groups > 1;
  RoundState& R = ctx->rs;
  R.ginfo = false;
  R.zpre = false;
  R.gcert = false;
  R.runrem = false;
  if (grouped && r->n_groups <= (1 << 20)) {
    // one synchronisation: group counts, group anchors and the cost table to the host
    const int G = r->n_groups;
    const bool fused = T <= PREP_T_MAX && G <= GAGG_MAX;   // (launch_order_prep: two launches)
    if (!fused) {
      ENSURE(ctx->gcnt, sizeof(int32_t) * (G + 1));
      HIPCHK(hipMemsetAsync(ctx->gcnt.p, 0, sizeof(int32_t) * (G + 1), st));
      launch_group_hist(r->task_group, T, G, P<int32_t>(ctx->gcnt), st);
    }
    // staged in pinned memory: pageable destinations made each copy a ~20 us synchronous
    // staging step (profiles/r02q kernel trace)
    const bool ca = r->mode == PVT_CA_FF || r->mode == PVT_CA_BF;
    const size_t nz2 = ca ? (size_t)r->n_zones * r->n_zones : 0;
    const size_t need = sizeof(double) * nz2 + sizeof(int32_t) * (2 * (size_t)G + 1);
    if (ctx->gstage_cap < need) {
      if (ctx->gstage) (void)hipHostFree(ctx->gstage);
      ctx->gstage = nullptr;
      ctx->gstage_cap = 0;
      HIPCHK(hipHostMalloc(&ctx->gstage, need));
      ctx->gstage_cap = need;
    }
    // counts, anchors and cost table written into the pinned buffer by one kernel, which also
    // leaves the groups' offsets and scatter cursors on the device
    ENSURE(ctx->goff, sizeof(int32_t) * 2 * (G + 1));
    void* dstage = nullptr;
    HIPCHK(hipHostGetDevicePointer(&dstage, ctx->gstage, 0));
    double* dcst = reinterpret_cast<double*>(dstage);
    int32_t* dcnt = reinterpret_cast<int32_t*>(dcst + nz2);
    // the per-group sorts, optimistically (a group over GSORT_MAX tasks is left unsorted by the
    // kernel; build_order_check then redoes the order with radix passes)
    ENSURE(ctx->gskey, sizeof(uint64_t) * T);
    ENSURE(ctx->gsidx, sizeof(int32_t) * T);
    if (fused) {
      // placement fill and (cost_aware) zone tables too: round_begin skips its own
      if (ca) {
        ENSURE(ctx->csum, sizeof(double) * r->n_zones * r->n_zones);
        ENSURE(ctx->bsum, sizeof(double) * r->n_zones * r->n_zones);
      }
      PrepArgs pa{r->task_group, T, G, r->group_anchor, r->cost, r->bw, r->n_zones, (int)nz2,
                  r->dem, r->sort_tasks ? 1 : 0, r->placement, P<int32_t>(ctx->goff), dcnt,
                  dcnt + G + 1, dcst, ca ? P<double>(ctx->csum) : nullptr,
                  ca ? P<double>(ctx->bsum) : nullptr, P<uint64_t>(ctx->gskey), P<int32_t>(ctx->gsidx),
                  nullptr, 0};
      R.prep_fused = true;
      if (G <= GCOMPACT_MAX) {   // one launch: the counts (block 0) beside the sorted, gathered order
        // the host polls a flag the count block stores (no event: a marker on the stream cost
        // ~5 us of idle GPU between launches)
        pa.hflag = ctx->flag_hdev;
        pa.seq = ++ctx->flag_seq;
        R.stage_flag = true;
        const bool zw = hmin && zwin && ca && r->n_zones <= ZMAX;
        // (the groups' certificates for the first epoch's frontier walk, with its windows)
        const bool gc = zw && ctx->t_chain_cert;
        if (gc) ENSURE(ctx->gcert, sizeof(GroupCert) * (size_t)GCOMPACT_MAX);
        const bool rr = gc && ctx->t_zw_runrem;   // (run lengths for that walk, from the same rows)
        if (rr) ENSURE(ctx->run_rem, sizeof(int32_t) * (size_t)T);
        launch_group_sort_gather(pa, GatherOut{cur, P<double>(ctx->dem_ord), P<int32_t>(ctx->anc_ord),
                                               P<int32_t>(ctx->grp_ord), r->order, r->avail,
                                               r->n_hosts, hmin, ctx->stamps, r->zone,
                                               zw ? zwin : nullptr,
                                               gc ? P<GroupCert>(ctx->gcert) : nullptr,
                                               rr ? P<int32_t>(ctx->run_rem) : nullptr}, st);
        if (hmin_done) *hmin_done = hmin != nullptr;
        R.zpre = zw;
        R.gcert = gc;
        R.runrem = rr;
        R.gathered = true;
        R.ginfo = ca;
        *pending = true;
        *ord_out = cur;
        return PVT_OK;
      }
      launch_order_prep(pa, st, ctx->ev_stage);
    } else {
      launch_group_stage(P<int32_t>(ctx->gcnt), G, r->group_anchor, r->cost, (int)nz2,
                         P<int32_t>(ctx->goff), dcnt, dcnt + G + 1, dcst, st);
      HIPCHK(hipGetLastError());
      const uint64_t* keys = nullptr;
      if (r->sort_tasks) {
        ENSURE(ctx->keys64a, sizeof(uint64_t) * T);
        launch_norm_keys(r->dem, T, nullptr, P<uint64_t>(ctx->keys64a), st);
        keys = P<uint64_t>(ctx->keys64a);
      }
      launch_group_scatter(r->task_group, keys, T, G, P<int32_t>(ctx->goff) + G + 1,
                           P<uint64_t>(ctx->gskey), P<int32_t>(ctx->gsidx), st);
      HIPCHK(hipEventRecord(ctx->ev_stage, st));
    }
    // the host waits for the staged counts only (ev_stage), not for the scatter, sorts and
    // gathers queued after them: it plans the round while they run
    launch_group_sort(P<int32_t>(ctx->goff), G, P<uint64_t>(ctx->gskey), P<int32_t>(ctx->gsidx),
                      cur, st);
    R.ginfo = ca;
    *pending = true;
    *ord_out = cur;
    return PVT_OK;
  }
  return build_order_radix(ctx, r, ord_out);
}

// After the caller's synchronisation: the group counts, anchors and cost table the optimistic
// path staged; *redo = a group exceeded the LDS sort (the order must be rebuilt by radix passes).
static int build_order_check(pvt_ctx* ctx, const pvt_round* r, bool* redo) {
  RoundState& R = ctx->rs;
  const int G = r->n_groups;
  const bool ca = r->mode == PVT_CA_FF || r->mode == PVT_CA_BF;
  const size_t nz2 = ca ? (size_t)r->n_zones * r->n_zones : 0;
  const double* cst = reinterpret_cast<const double*>(ctx->gstage);
  const int32_t* cnt = reinterpret_cast<const int32_t*>(cst + nz2);
  const int32_t* gan = cnt + G + 1;
  R.gcnt.assign(cnt, cnt + G + 1);
  R.ga_host.assign(gan, gan + G);
  R.cost_host.assign(cst, cst + nz2);
  if (R.gcnt[G] != 0) return fail(ctx, PVT_EINVAL, "task_group out of range");
  int mx = 0;
  for (int g = 0; g < G; g++) mx = std::max(mx, R.gcnt[g]);
  *redo = mx > GSORT_MAX;
  return PVT_OK;
}

// Processing order by radix passes: stable by descending norm (sort_tasks), then stable by group.
static int build_order_radix(pvt_ctx* ctx, const pvt_round* r, int32_t** ord_out) {
  const int T = r->n_tasks;
  hipStream_t st = ctx->stream;
  int32_t* cur = P<int32_t>(ctx->ord);
  int32_t* alt = P<int32_t>(ctx->ord2);
  const bool grouped = r->task_group != nullptr && r->n_groups > 1;
  launch_iota(cur, T, st);
  if (r->sort_tasks) {
    ENSURE(ctx->keys64a, sizeof(uint64_t) * T);
    ENSURE(ctx->keys64b, sizeof(uint64_t) * T);
    launch_norm_keys(r->dem, T, nullptr, P<uint64_t>(ctx->keys64a), st);
    size_t tmp = 0;
    HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp, P<uint64_t>(ctx->keys64a),
                                              P<uint64_t>(ctx->keys64b), cur, alt, T, 0, 64, st));
    ENSURE(ctx->sorttmp, tmp);
    HIPCHK(hipcub::DeviceRadixSort::SortPairs(ctx->sorttmp.p, tmp, P<uint64_t>(ctx->keys64a),
                                              P<uint64_t>(ctx->keys64b), cur, alt, T, 0, 64, st));
    std::swap(cur, alt);
  }
  if (grouped) {
    ENSURE(ctx->keys32a, sizeof(uint32_t) * T);
    ENSURE(ctx->keys32b, sizeof(uint32_t) * T);
    launch_group_keys(r->task_group, cur, T, P<uint32_t>(ctx->keys32a), st);
    int bits = 1;
    while ((1 << bits) < r->n_groups && bits < 31) bits++;
    size_t tmp = 0;
    HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp, P<uint32_t>(ctx->keys32a),
                                              P<uint32_t>(ctx->keys32b), cur, alt, T, 0, bits, st));
    ENSURE(ctx->sorttmp, tmp);
    HIPCHK(hipcub::DeviceRadixSort::SortPairs(ctx->sorttmp.p, tmp, P<uint32_t>(ctx->keys32a),
                                              P<uint32_t>(ctx->keys32b), cur, alt, T, 0, bits, st));
    std::swap(cur, alt);
  }
  *ord_out = cur;
  return PVT_OK;
}

void pvt::lists_from(pvt_ctx* ctx, Lists& L, int b) {
  L.e = P<ListEntry>(ctx->l_e[b]);
  L.ids = P<int32_t>(ctx->l_ids[b]);
  L.t = P<TaskRec>(ctx->l_t[b]);
}

// Opportunistic: windows of OPP_MAXW tasks in caller order; count pass then commit walk. The
// MT19937 state travels host -> device -> host around the round.
static int opp_round(pvt_ctx* ctx, const pvt_round* r) {
  const int T = r->n_tasks, H = r->n_hosts;
  hipStream_t st = ctx->stream;
  // Window: longer windows cut the per-window launches and hand-offs; the walk's touched-host
  // tables bound them (OPP_MAXW, LDS). (bench sweeps at 1M hosts x 10k tasks: round 2 with the
  // speculative-range walk, profiles/r02h: pipelined 64 -> 20.1 ms, 128 -> 18.5, 256 -> 19.4;
  // round 4 with the register-row walk: 128 -> 10.0, 256 -> 9.6)
  const int wdef = ctx->pipeline ? OPP_WINDOW_PIPE : OPP_WINDOW_DEFAULT;
  const int W = std::max(1, std::min(ctx->window > 0 ? ctx->window : wdef, OPP_MAXW));
  const int nq = (H + OPP_CH - 1) / OPP_CH, nsq = (nq + OPP_SUP - 1) / OPP_SUP;
  ENSURE(ctx->dem_ord, sizeof(double) * 4 * T);
  ENSURE(ctx->anc_ord, sizeof(int32_t) * T);
  launch_gather_tasks(r->dem, r->order, nullptr, nullptr, T, P<double>(ctx->dem_ord),
                      P<int32_t>(ctx->anc_ord), nullptr, st);
  // Pipelined windows (a walk's inherited + own touched hosts, 2 x OPP_MAXW, fit its LDS):
  // window k+1's count pass runs on the side stream while window k is walked. Walk k leaves
  // global availability untouched and hands its hosts to walk k+1, which applies them on entry
  // and then releases count k+2; so every count pass reads the capacities its walk's
  // predecessor started from, and the hosts that walk touched are touched for the next walk.
  const int nwin = (T + W - 1) / W;
  const bool pipe = ctx->pipeline && nwin > 1;
  const int nbuf = pipe ? 2 : 1;
  const size_t bm_bytes = sizeof(uint64_t) * 4 * (size_t)nq * W;
  const size_t sc_bytes = sizeof(int32_t) * (size_t)nsq * W;
  const size_t tl_bytes = pipe ? sizeof(OppTouched) : 0;
  const size_t slot = (bm_bytes + sc_bytes + tl_bytes + 255) / 256 * 256;
  ENSURE(ctx->opp, slot * nbuf + sizeof(uint32_t) * 640);
  ENSURE(ctx->oppfault, 16);
  int32_t* fault = P<int32_t>(ctx->oppfault);
  HIPCHK(hipMemsetAsync(fault, 0, sizeof(int32_t), st));
  char* base = reinterpret_cast<char*>(ctx->opp.p);
  auto bm_of = [&](int b) { return reinterpret_cast<uint64_t*>(base + slot * b); };
  auto sc_of = [&](int b) { return reinterpret_cast<int32_t*>(base + slot * b + bm_bytes); };
  auto tl_of = [&](int b) { return reinterpret_cast<OppTouched*>(base + slot * b + bm_bytes + sc_bytes); };
  uint32_t* mt = reinterpret_cast<uint32_t*>(base + slot * nbuf);
  HIPCHK(hipMemcpyAsync(mt, r->mt_state, sizeof(uint32_t) * 625, hipMemcpyHostToDevice, st));
  const double bpc = bytes_per_candidate(r->mode);
  auto count = [&](int k, hipStream_t s) {
    const int t0 = k * W, nt = std::min(W, T - t0);
    OppCountArgs ca{r->avail, P<double>(ctx->dem_ord) + (size_t)t0 * 4, H, nt, 0, 0, nq, nsq,
                    W, bm_of(k % nbuf), sc_of(k % nbuf), 0, nsq, nq, nsq};
    Scope sc(ctx, PVT_K_SCORE, (double)nt * H, (double)nt * H * bpc, s, "opp_count_kernel");
    launch_opp_count(ca, s);
  };
  if (nwin > 0) count(0, st);
  for (int k = 0; k < nwin; k++) {
    const int t0 = k * W, nt = std::min(W, T - t0);
    const bool next = pipe && k + 1 < nwin;
    ctx->windows++;
    if (!pipe && k > 0) count(k, st);   // sequential: window k counted after walk k-1 wrote back
    const OppTouched* in = (pipe && k > 0) ? tl_of((k - 1) % nbuf) : nullptr;
    if (in) launch_opp_apply(in, r->avail, H, st);   // walk k-1's commits, before count k+1
    if (next) {
      HIPCHK(hipEventRecord(ctx->ev_walk, st));
      HIPCHK(hipStreamWaitEvent(ctx->side, ctx->ev_walk, 0));
      count(k + 1, ctx->side);
      HIPCHK(hipEventRecord(ctx->ev_lists, ctx->side));
    }
    OppCommitArgs oa{r->avail, P<double>(ctx->dem_ord) + (size_t)t0 * 4, bm_of(k % nbuf),
                     sc_of(k % nbuf), H, nt, nq, nsq, W, r->placement + t0, mt, ctx->stamps,
                     in, next ? tl_of(k % nbuf) : nullptr, next ? 0 : 1, fault};
    {
      Scope s(ctx, PVT_K_COMMIT, 0, 0, nullptr, "opp_commit_kernel");
      launch_opp_commit(oa, st);
    }
    if (next) HIPCHK(hipStreamWaitEvent(st, ctx->ev_lists, 0));
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(r->mt_state, mt, sizeof(uint32_t) * 625, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(ctx->next_host + 3, fault, sizeof(int32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (ctx->next_host[3])
    return fail(ctx, PVT_EHIP, "opportunistic walk: inconsistent feasible counts (a range's first "
                "task, window-local %d, failed its verification)", ctx->next_host[3] - 1);
  return PVT_OK;
}

// vbp best-fit band lists: hosts [lo, hi) sorted by snapshot memory (stable radix sort of the
// orderable bits of avail[1]) and their snapshot state gathered in that order; no host touched.
// (rocPRIM's onesweep sort measured slower than the default dispatch's merge sort at config 5's
// 1M hosts: 8 passes of ~25 us plus two fill launches each, against ~0.19 ms; the memory values
// of uniform random hosts vary in ~63 key bits, so no pass can be skipped.)
static int band_snapshot(pvt_ctx* ctx) {
  RoundState& R = ctx->rs;
  const pvt_round* r = &R.r;
  hipStream_t st = ctx->stream;
  const int n = R.hi - R.lo;
  ENSURE(ctx->bkey, sizeof(uint64_t) * 2 * (size_t)n);
  ENSURE(ctx->bidx, sizeof(int32_t) * 2 * (size_t)n);
  ENSURE(ctx->bsa, sizeof(double) * 4 * (size_t)n);
  ENSURE(ctx->bstb, sizeof(uint32_t) * (size_t)n);
  ENSURE(ctx->btouch, (size_t)R.H);
  ENSURE(ctx->btlist, sizeof(int32_t) * (size_t)R.H);
  ENSURE(ctx->btcnt, 16);
  ENSURE(ctx->bpos, sizeof(int32_t) * (size_t)R.H);
  ENSURE(ctx->bptouch, (size_t)n);
  ENSURE(ctx->brec, sizeof(BandRec) * (size_t)n);
  uint64_t* k0 = P<uint64_t>(ctx->bkey);
  int32_t* i0 = P<int32_t>(ctx->bidx);
  size_t tmp = 0;
  HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp, k0, k0 + n, i0, i0 + n, n, 0, 64, st));
  ENSURE(ctx->bsorttmp, tmp);
  const int bs = ctx->t_band_segs ? ctx->t_band_segs : BAND_SEGS;   // (PVT_BAND_SEGS: 2 ... 32)
  R.band_S = (bs == 1 || bs == 2 || bs == 4 || bs == 8 || bs == 16 || bs == 32) ? bs : BAND_SEGS;
  Scope sc(ctx, PVT_K_OTHER, 0, 0);
  launch_band_keys(r->avail, r->tiebreak, R.H, R.lo, n, k0, i0, P<BandRec>(ctx->brec), st);
  HIPCHK(hipcub::DeviceRadixSort::SortPairs(ctx->bsorttmp.p, tmp, k0, k0 + n, i0, i0 + n, n, 0, 64, st));
  launch_band_gather(P<BandRec>(ctx->brec), R.lo, n, i0 + n, P<double>(ctx->bsa),
                     P<uint32_t>(ctx->bstb), P<int32_t>(ctx->bpos), st);
  HIPCHK(hipMemsetAsync(ctx->btouch.p, 0, (size_t)R.H, st));
  HIPCHK(hipMemsetAsync(ctx->bptouch.p, 0, (size_t)n, st));
  HIPCHK(hipMemsetAsync(ctx->btcnt.p, 0, 16, st));
  HIPCHK(hipGetLastError());
  return PVT_OK;
}

// The last walk's committed hosts flagged and listed as touched (band lists), on the context's
// stream. Called only where no band score pass is in flight (it would read the touched table).
void pvt::flush_touched(pvt_ctx* ctx) {
  RoundState& R = ctx->rs;
  if (!R.band || R.touch_lb < 0) return;
  launch_touch_update(P<int32_t>(ctx->owned[R.touch_lb]),
                      R.touch_status ? R.touch_status : P<int32_t>(ctx->next),
                      P<uint8_t>(ctx->btouch), P<int32_t>(ctx->btlist), P<int32_t>(ctx->btcnt),
                      P<int32_t>(ctx->bpos), R.lo, R.hi, P<uint8_t>(ctx->bptouch), ctx->stream);
  R.touch_lb = -1;
}

// ---------------------------------------------------------------- round state machine
// pvt_place() and the sharded calls share one round: begin (order, gathers, zone tables, group
// boundaries), then per window: candidate lists over this context's host range (optionally
// exchanged between ranks), then the commit walk, which decides where the next window starts.

int pvt::round_begin(pvt_ctx* ctx, const pvt_round* rin, int lo, int hi, int world) {
  RoundState& R = ctx->rs;
  R.active = false;
  int rc = check_round(ctx, rin);
  if (rc) return rc;
  R.r = *rin;
  const pvt_round* r = &R.r;
  ctx->windows = ctx->refills = 0;
  HIPCHK(hipSetDevice(ctx->device));
  const int T = r->n_tasks, H = r->n_hosts, Z = r->n_zones;
  R.T = T; R.H = H; R.Z = Z; R.lo = lo; R.hi = hi; R.world = world;
  R.t0 = 0; R.g = 0; R.nt = 0; R.lb = 0;
  R.gstart.assign(1, 0);
  R.ganchor.clear();
  R.gid.clear();
  if (T == 0) { R.ngroups = 0; R.active = true; return PVT_OK; }
  hipStream_t st = ctx->stream;

  bool pending = false;
  R.prep_fused = false;
  R.gathered = false;
  ENSURE(ctx->dem_ord, sizeof(double) * 4 * T);
  ENSURE(ctx->anc_ord, sizeof(int32_t) * T);
  ENSURE(ctx->grp_ord, sizeof(int32_t) * T);
  // a cost_aware best-fit round of epochs (epoch_groups) starts with the frontier walk's host
  // minima: written by the grouped order's launch, or queued below, they are ready while the
  // host waits for the grouped order's counts
  const bool want_hmin = ctx->epochs && ctx->zwalk && r->mode == PVT_CA_BF && r->task_group &&
                         r->n_groups >= 2 && T >= 2 && !r->rt_bw && (Z <= ZMAX || wide_fast(ctx)) &&
                         world == 1;
  // (rounds of more than ZMAX zones: the minima only -- no prebuilt windows, no group certificates)
  const bool want_zwin = want_hmin && ctx->t_zpre && Z <= ZMAX;
  if (want_hmin) {
    ENSURE(ctx->hmin, sizeof(double) * 4 * ZW_MIN_PARTS);
    if (want_zwin) ENSURE(ctx->zwin, sizeof(ZoneWindows));
  }
  bool hmin_done = false;
  if ((rc = build_order(ctx, r, &R.ord, &pending, want_hmin ? P<double>(ctx->hmin) : nullptr,
                        &hmin_done, want_zwin ? P<ZoneWindows>(ctx->zwin) : nullptr)))
    return rc;
  if (!R.prep_fused) HIPCHK(hipMemsetAsync(r->placement, 0xff, sizeof(int32_t) * T, st));
  auto order_out = [&]() -> int {   // (the gather also writes the caller's order)
    launch_gather_tasks(r->dem, R.ord, r->task_group, r->group_anchor, T, P<double>(ctx->dem_ord),
                        P<int32_t>(ctx->anc_ord), P<int32_t>(ctx->grp_ord), st, r->n_groups, r->order);
    return PVT_OK;
  };
  if (!R.gathered && (rc = order_out())) return rc;
  const bool ca = r->mode == PVT_CA_FF || r->mode == PVT_CA_BF;
  if (ca) {
    ENSURE(ctx->csum, sizeof(double) * Z * Z);
    ENSURE(ctx->bsum, sizeof(double) * Z * Z);
    if (!R.prep_fused)
      launch_zone_tables(r->cost, r->bw, Z, P<double>(ctx->csum), P<double>(ctx->bsum), st);
  }
  R.hmin_pre = false;
  if (want_hmin) {
    if (!hmin_done) {
      Scope sc(ctx, PVT_K_OTHER, 0, 0);
      launch_host_min(r->avail, H, 0, H, P<double>(ctx->hmin), st);
    }
    R.hmin_pre = true;
  }
  if (pending) {   // the one synchronisation of the grouped order: counts, anchors, cost table
    if (R.stage_flag) {
      if ((rc = wait_stage_flag(ctx))) return rc;
    } else {
      HIPCHK(hipEventSynchronize(ctx->ev_stage));
    }
    bool redo = false;
    if ((rc = build_order_check(ctx, r, &redo))) return rc;
    if (redo) {
      R.gcert = false;                        // (a group had no record)
      R.runrem = false;
      if ((rc = build_order_radix(ctx, r, &R.ord))) return rc;
      if ((rc = order_out())) return rc;
    }
  }

  // group boundaries in processing order (only cost_aware first-fit with sort_hosts needs them)
  R.keyed = r->mode == PVT_CA_FF && r->sort_hosts;
  R.kscan = false;
  R.kmode = 0; R.kn = 0; R.kstall = false; R.kstall_t0 = -1;
  R.ordered = (r->mode == PVT_VBP_FF) || (r->mode == PVT_CA_FF && !r->sort_hosts);
  if (R.keyed) {
    std::vector<int32_t> tg, ga;
    if (r->task_group) {
      std::vector<int> cnt(r->n_groups, 0);
      if (R.ginfo) {                          // copied by build_order
        for (int g = 0; g < r->n_groups; g++) cnt[g] = R.gcnt[g];
        ga = R.ga_host;
      } else {
        tg.resize(T);
        ga.resize(r->n_groups);
        HIPCHK(hipMemcpyAsync(tg.data(), r->task_group, sizeof(int32_t) * T, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(ga.data(), r->group_anchor, sizeof(int32_t) * r->n_groups,
                              hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (int t = 0; t < T; t++) {
          if (tg[t] < 0 || tg[t] >= r->n_groups) return fail(ctx, PVT_EINVAL, "task_group out of range");
          cnt[tg[t]]++;
        }
      }
      int off = 0;
      R.gstart.clear();
      for (int g = 0; g < r->n_groups; g++) {
        if (cnt[g] == 0) continue;
        R.gstart.push_back(off);
        R.ganchor.push_back(ga[g]);
        R.gid.push_back(g);
        off += cnt[g];
      }
    } else {
      R.ganchor.push_back(0);
      R.gid.push_back(0);
    }
    ENSURE(ctx->key, sizeof(double) * H);
    ENSURE(ctx->next, sizeof(int32_t) * 4);
    R.kscan = ctx->keyed_scan != 0;
    if (ctx->t_keyed_scan >= 0) R.kscan = ctx->t_keyed_scan != 0;   // (PVT_KEYED_SCAN)
    if (R.kscan && hi > lo) {
      const int n = hi - lo;
      ENSURE(ctx->kskey, sizeof(uint64_t) * 2 * (size_t)std::max(n, 1));
      ENSURE(ctx->kperm, sizeof(int32_t) * (size_t)std::max(n, 1));
      ENSURE(ctx->kiota, sizeof(int32_t) * (size_t)std::max(n, 1));
      size_t tmp = 0;
      HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp, P<uint64_t>(ctx->kskey),
                                                P<uint64_t>(ctx->kskey) + n, P<int32_t>(ctx->kiota),
                                                P<int32_t>(ctx->kperm), n, 0, 64, st));
      size_t tmp2 = 0;
      HIPCHK(hipcub::DeviceSelect::Flagged(nullptr, tmp2, P<int32_t>(ctx->kiota),
                                           P<uint8_t>(ctx->kflag), P<int32_t>(ctx->kperm),
                                           P<int32_t>(ctx->next) + 2, n, st));
      ENSURE(ctx->ksorttmp, std::max(tmp, tmp2));
      ENSURE(ctx->kflag, (size_t)n);
      launch_iota(P<int32_t>(ctx->kiota), n, st);
    }
  }
  // vbp first-fit / unsorted cost_aware first-fit: the frontier walk over the first alive hosts
  // (ordered_frontier); its scratch is the keyed path's (the modes exclude each other)
  R.sh_epochs = false;
  R.list_until = 0;
  R.ofront = ctx->zwalk && R.ordered && T >= ORDERED_FRONTIER_MIN && H >= 64;
  R.of_try = R.ofront;
  R.of_tasks = ctx->of_tasks;
  R.kf_pending = false;
  if (R.ofront) {
    R.ofh = ORDERED_FRONTIER_HOSTS;
    if (ctx->t_of_hosts) R.ofh = ctx->t_of_hosts;   // (PVT_OF_HOSTS)
    ENSURE(ctx->next, sizeof(int32_t) * 4);
    ENSURE(ctx->kperm, sizeof(int32_t) * (size_t)H);
    ENSURE(ctx->kiota, sizeof(int32_t) * (size_t)H);
    ENSURE(ctx->kflag, (size_t)H);
    ENSURE(ctx->hmin, sizeof(double) * 4 * ZW_MIN_PARTS);
    size_t tmp2 = 0;
    HIPCHK(hipcub::DeviceSelect::Flagged(nullptr, tmp2, P<int32_t>(ctx->kiota), P<uint8_t>(ctx->kflag),
                                         P<int32_t>(ctx->kperm), P<int32_t>(ctx->next) + 2, H, st));
    ENSURE(ctx->ksorttmp, tmp2);
    launch_iota(P<int32_t>(ctx->kiota), H, st);
  }
  R.gstart.push_back(T);
  R.ngroups = R.keyed ? R.ganchor.size() : 1;
  // keyed first-fit: zero-key epochs (ff_epoch) over the groups, unsharded rounds
  R.ffe = false;
  R.ffe_skip = -1;
  R.wide_misses = 0;
  R.ep_to_lists = false;
  if (R.keyed && !R.sharded && ctx->zwalk && ctx->epochs && !r->rt_bw && (Z <= ZMAX || wide_fast(ctx)) &&
      T >= KEYED_FRONTIER_MIN) {
    R.egs = R.gstart;
    R.ega = R.ganchor;
    if ((rc = zero_cost_components(ctx))) return rc;
    R.ffe = true;
  }
  R.key_group = -1;
  R.touch_lb = -1;
  R.band = r->mode == PVT_VBP_BF && ctx->band_min > 0 && hi - lo >= ctx->band_min;
  if (R.band && (rc = band_snapshot(ctx))) return rc;
  R.runs.clear();
  if (R.band && ctx->lwalk && !R.sharded) {
    // representative list rows: the round's runs of equal demands, once (their ids on the host
    // size each window's rows; one synchronisation per round instead of a launch per window)
    ENSURE(ctx->brun, sizeof(int32_t) * (size_t)T);
    ENSURE(ctx->brdem, sizeof(double) * 4 * (size_t)T);
    launch_band_runs(P<double>(ctx->dem_ord), T, P<int32_t>(ctx->brun), P<double>(ctx->brdem), st);
    HIPCHK(hipGetLastError());
    R.runs.resize(T);
    HIPCHK(hipMemcpyAsync(R.runs.data(), ctx->brun.p, sizeof(int32_t) * (size_t)T,
                          hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  }

  // Windows adapt to how far commit walks get before a list is exhausted: a walk that stops
  // early means the next window only needs about that many tasks (the score pass costs the
  // same per task either way, so short windows waste less on tasks that get re-scored).
  // default window: MAX_WINDOW for every policy. (vbp best-fit had 512: its walks search deeper
  // lists as a window's touched hosts pile up at the top of every task's ranking; with the
  // merge-path merge the longer windows win -- config 5: 3.33 ms at 512, 3.26 at 768, 3.07 at
  // 1024, round 4 sweep.)
  const int wdef = MAX_WINDOW;
  R.Wmax = std::max(1, std::min(ctx->window > 0 ? ctx->window : wdef, MAX_WINDOW));
  R.W = R.Wmax;
  ENSURE(ctx->seg, sizeof(SegEntry) * (size_t)SEG_ENTRIES_MAX);
  ENSURE(ctx->seg_feas, sizeof(int32_t) * (size_t)SEG_ENTRIES_MAX / KL);
  for (int b = 0; b < 2; b++) {
    ENSURE(ctx->l_e[b], sizeof(ListEntry) * (size_t)R.Wmax * LMAX);
    ENSURE(ctx->l_ids[b], sizeof(int32_t) * (size_t)R.Wmax * LMAX);
    ENSURE(ctx->l_t[b], sizeof(TaskRec) * (size_t)R.Wmax);
    ENSURE(ctx->owned[b], sizeof(int32_t) * MAX_WINDOW);
  }
  ENSURE(ctx->next, sizeof(int32_t) * 4);
  R.active = true;
  return PVT_OK;
}

// End of the group holding task t0 (keyed first-fit: windows never cross a group).
int pvt::group_end(const RoundState& R, int t0) {
  if (!R.keyed) return R.T;
  size_t g = 0;
  while (g < R.ngroups && t0 >= R.gstart[g + 1]) g++;
  return g < R.ngroups ? R.gstart[g + 1] : R.T;
}

// ---- kernel argument builders: every field is set by name, so a field added to one of the
// structs (pvt_kernels.h) shifts nothing. Each returns the fields its callers share; a caller
// then sets its own, by name.

// The list walk of window [t0, t0 + nt) on list buffer lb, inheriting n_prev hosts from the
// other buffer's walk. Callers add: walk_launch hflag / hseq; place_epochs' chain mode coff /
// cmap / csoff / cseg / wlog / skip_done and prev_ids = nullptr.
CommitArgs pvt::commit_args(pvt_ctx* ctx, int t0, int nt, int lb, int n_prev, int32_t* status) {
  RoundState& R = ctx->rs;
  const pvt_round* r = &R.r;
  CommitArgs a{};
  a.avail = r->avail; a.zone = r->zone; a.tb = r->tiebreak; a.placement = r->placement;
  a.dem = P<double>(ctx->dem_ord) + (size_t)t0 * 4;
  a.grp = P<int32_t>(ctx->grp_ord) + t0;
  a.csum = P<double>(ctx->csum); a.bsum = P<double>(ctx->bsum);
  lists_from(ctx, a.L, lb);
  a.H = R.H; a.Z = R.Z; a.nt = nt; a.mode = r->mode;
  a.prev_ids = P<int32_t>(ctx->owned[1 - lb]); a.n_prev = n_prev;
  a.own_ids = P<int32_t>(ctx->owned[lb]);
  a.status = status;
  a.rtb = r->mode == PVT_CA_BF ? r->rt_bw : nullptr;
  a.stamps = ctx->stamps;
  if (R.band && R.reps[lb]) {      // representative rows (window_lists)
    a.rowmap = P<int32_t>(ctx->brun) + t0; a.rowbase = R.rbase[lb]; a.ordw = R.ord + t0;
  }
  return a;
}

// What every frontier walk of tasks from t0 reads (pvt_zwalk.hip).
static ZwalkArgs zwalk_common_args(pvt_ctx* ctx, int t0) {
  RoundState& R = ctx->rs;
  ZwalkArgs a{};
  a.avail = R.r.avail; a.zone = R.r.zone; a.placement = R.r.placement;
  a.H = R.H; a.Z = R.Z;
  a.dem = P<double>(ctx->dem_ord) + (size_t)t0 * 4;
  a.anc = P<int32_t>(ctx->anc_ord) + t0;
  a.ord = R.ord + t0;
  a.wlog = P<WinRec>(ctx->wres);
  a.stamps = ctx->stamps;
  return a;
}

// Chain mode: the chains of the epoch at t0, tables and status in ctx->ep_dev, host minima (or
// absolute maxima, ff_epoch) in ctx->hmin. Callers add: ff_epoch tab; place_epochs cmax, zpre,
// tab; shard_frontier_commit cmax, pwin.
ZwalkArgs pvt::zwalk_chain_args(pvt_ctx* ctx, int t0) {
  int32_t* dev = P<int32_t>(ctx->ep_dev);
  ZwalkArgs a = zwalk_common_args(ctx, t0);
  a.csum = P<double>(ctx->csum); a.bsum = P<double>(ctx->bsum);
  a.coff = dev + EP_COFF; a.cmap = dev + EP_CMAP; a.csoff = dev + EP_CSOFF; a.cseg = dev + EP_CSEG;
  a.status = dev + EP_STATUS;
  a.hmin = P<double>(ctx->hmin);
  if (ctx->rs.Z > ZMAX) a.zcomp = P<int32_t>(ctx->zcomp);   // (the wide walk's components)
  return a;
}

// Keyed mode: one walk of n tasks from t0, status in ctx->next, capacities written back to the
// round. Callers add: round_next_window (keyed group start) csum / bsum, kperm, lo, kn_dev;
// ordered_frontier kperm, kn_dev (lo stays 0); shard_frontier_commit lo, pwin. Only the
// unsharded keyed walk passes csum / bsum: the ordered and the sharded walks pass NULL.
ZwalkArgs pvt::zwalk_keyed_args(pvt_ctx* ctx, int t0, int n) {
  ZwalkArgs a = zwalk_common_args(ctx, t0);
  a.status = P<int32_t>(ctx->next);
  a.knt = n;
  a.wb = ctx->rs.r.avail;
  return a;
}

// Validation / finality / apply of the epoch of nt tasks in nseg segments at t0 (pvt_epoch.hip).
// Callers add: ff_epoch whole; place_epochs and shard_frontier_commit rtb, and for a
// frontier-walked epoch cmax / coff / nch / safe.
EpochArgs pvt::epoch_args(pvt_ctx* ctx, int t0, int nt, int nseg) {
  RoundState& R = ctx->rs;
  int32_t* dev = P<int32_t>(ctx->ep_dev);
  EpochArgs a{};
  a.dem = P<double>(ctx->dem_ord) + (size_t)t0 * 4;
  a.anc = P<int32_t>(ctx->anc_ord) + t0;
  a.grp = P<int32_t>(ctx->grp_ord) + t0;
  a.csum = P<double>(ctx->csum); a.bsum = P<double>(ctx->bsum);
  a.zone = R.r.zone; a.avail = R.r.avail;
  a.seg_off = dev + EP_SEG_OFF; a.seg_chain = dev + EP_SEG_CHAIN; a.seg_cstart = dev + EP_SEG_CSTART;
  a.status = dev + EP_STATUS; a.bad = dev + EP_BAD;
  a.wlog = P<WinRec>(ctx->wres);
  a.H = R.H; a.Z = R.Z; a.nt = nt; a.nseg = nseg;
  return a;
}

// The flagged hosts of kiota[0, n) compacted into kperm, their count to ctx->next[2].
int pvt::compact_flags(pvt_ctx* ctx, int n, hipStream_t st) {
  size_t tmp = ctx->ksorttmp.n;
  HIPCHK(hipcub::DeviceSelect::Flagged(P<void>(ctx->ksorttmp), tmp, P<int32_t>(ctx->kiota),
                                       P<uint8_t>(ctx->kflag), P<int32_t>(ctx->kperm),
                                       P<int32_t>(ctx->next) + 2, n, st));
  return PVT_OK;
}

// A keyed-mode frontier walk's report: `done` of n tasks placed (what: the path, for the error).
int pvt::frontier_walked(pvt_ctx* ctx, const char* what, int done, int n) {
  if (done < 0 || done > n)
    return fail(ctx, PVT_EHIP, "%s frontier walk returned %d of %d", what, done, n);
  ctx->n_zchains += done > 0;
  return PVT_OK;
}

// The ordered frontier's decision after an attempt that placed `done` of n tasks on a window
// taken from the first hs hosts (its candidate count in ctx->next_host[2]): a short window that
// stopped the walk doubles the span; *again = the frontier is tried again (a short window that
// placed nothing, or an attempt that placed at least ORDERED_FRONTIER_MIN tasks), else one list
// window comes next.
int pvt::ordered_verdict(pvt_ctx* ctx, const char* what, int done, int n, int hs, bool* again) {
  RoundState& R = ctx->rs;
  int rc = frontier_walked(ctx, what, done, n);
  if (rc) return rc;
  *again = done >= ORDERED_FRONTIER_MIN;
  const bool short_window = ctx->next_host[2] < ZW_M && hs < R.H;
  if (done < n && short_window) {
    R.ofh = (int)std::min<int64_t>((int64_t)R.ofh * 2, R.H);
    if (done == 0) *again = true;
  }
  return PVT_OK;
}

// Full stable radix sort of the frozen keys of this context's hosts (cost_aware.py:118-119).
static int keyed_full_sort(pvt_ctx* ctx) {
  RoundState& R = ctx->rs;
  const int n = R.hi - R.lo;
  size_t tmp = ctx->ksorttmp.n;
  const uint64_t* kin = reinterpret_cast<const uint64_t*>(P<double>(ctx->key) + R.lo);
  HIPCHK(hipcub::DeviceRadixSort::SortPairs(P<void>(ctx->ksorttmp), tmp, kin,
                                            P<uint64_t>(ctx->kskey) + n, P<int32_t>(ctx->kiota),
                                            P<int32_t>(ctx->kperm), n, 0, 64, ctx->stream));
  R.kmode = 2;
  R.kn = n;
  return PVT_OK;
}

// Size of the next window at R.t0 (0: the round is done). Computes the frozen first-fit key of
// this context's hosts at a group start (cost_aware.py:118-119, on the current capacities).
// Keyed rounds first try zero-key epochs at each group start (ff_epoch): whole groups proven by
// the first-fit chain walk need no key at all.
int pvt::round_next_window(pvt_ctx* ctx, int* nt_out) {
  RoundState& R = ctx->rs;
  *nt_out = 0;
  if (!R.active) return fail(ctx, PVT_EINVAL, "no round in progress");
  for (;;) {                      // (a group the keyed frontier walk completed: the next one)
  while (R.g < R.ngroups && R.t0 >= (R.keyed ? R.gstart[R.g + 1] : R.T)) R.g++;
  if (R.g >= R.ngroups || R.T == 0) return PVT_OK;
  const int ge = R.keyed ? R.gstart[R.g + 1] : R.T;
  int rc = 0;
  if (R.ffe && R.t0 == R.gstart[R.g] && R.key_group != (int)R.g && R.ffe_skip != (int)R.g) {
    int adv = 0;
    if ((rc = ff_epoch(ctx, &adv))) return rc;
    if (adv > 0) { R.t0 += adv; continue; }
    R.ffe_skip = (int)R.g;          // (this group goes to the keyed path below)
    // (a wide round whose zero-key epochs keep accepting nothing plans no more of them)
    if (R.Z > ZMAX && ++R.wide_misses >= WIDE_MISS_MAX) R.ffe = false;
  }
  if (R.kstall) {                 // same group, frozen keys: complete the order
    R.kstall = false;
    if (R.key_group == (int)R.g && R.kmode == 1 && (rc = keyed_full_sort(ctx))) return rc;
  }
  if (R.keyed && R.key_group != (int)R.g && R.hi == R.lo && R.kscan && R.sharded) {
    // a rank with no hosts: no key, an empty prefix -- but the group start's frontier walk is a
    // collective step every rank takes (round_next_window decides it the same way everywhere)
    R.kf_pending = ctx->zwalk && R.t0 == R.gstart[R.g] && ge - R.t0 >= KEYED_FRONTIER_MIN &&
                   !R.r.rt_bw && R.Z <= ZMAX;
    HIPCHK(hipMemsetAsync(P<int32_t>(ctx->next) + 2, 0, sizeof(int32_t), ctx->stream));
    R.key_group = (int)R.g;
  }
  if (R.keyed && R.key_group != (int)R.g && R.hi > R.lo) {
    KeyArgs ka{R.r.avail, R.r.zone, R.r.decay, P<double>(ctx->csum), P<double>(ctx->bsum), R.H, R.Z,
               R.ganchor[R.g], R.lo, R.hi, P<double>(ctx->key),
               R.r.rt_bw ? R.r.rt_bw + (size_t)R.gid[R.g] * R.H : nullptr};
    {
      Scope sc(ctx, PVT_K_OTHER, 0, 0);
      launch_key(ka, ctx->stream);
    }
    if (R.kscan) {
      // The group's host order (cost_aware.py:118-119). Hosts of zero key (the anchor zone's:
      // no egress cost) come first, in host order; when there are enough of them the rest is
      // sorted only if a walk ever exhausts that prefix (kstall).
      const int n = R.hi - R.lo;
      const double* kin = P<double>(ctx->key) + R.lo;
      {
        Scope sc(ctx, PVT_K_OTHER, 0, 0);
        launch_zero_key_flags(kin, n, P<uint8_t>(ctx->kflag), ctx->stream);
        if ((rc = compact_flags(ctx, n, ctx->stream))) return rc;
      }
      // The frontier walk (pvt_zwalk.hip, keyed mode) takes the group's first tasks from the
      // group start: each takes the first prefix host, in host order, that strictly fits, which
      // is the keyed order's answer whatever the prefix length (zero-key hosts lead it in both
      // modes below); it stops at the first task no host of the prefix's first ZW_M fits, and
      // the windowed list path goes on from there with the same frozen key. Launched on the
      // prefix length as the device holds it, read back with it in one synchronisation.
      const int n_g = ge - R.t0;
      const bool zk_any = ctx->zwalk && R.t0 == R.gstart[R.g] && n_g >= KEYED_FRONTIER_MIN &&
                          !R.r.rt_bw && R.Z <= ZMAX;
      const bool zk = zk_any && !R.sharded;
      // host-sharded: the walk runs on the merged window of every rank's first prefix hosts
      // (pvt_shard_score packs this rank's, PK_KEYED), after the prefix lengths are known
      R.kf_pending = zk_any && R.sharded;
      if (zk) {
        ENSURE(ctx->wres, sizeof(WinRec) * (size_t)n_g);
        ZwalkArgs za = zwalk_keyed_args(ctx, R.t0, n_g);
        za.csum = P<double>(ctx->csum);
        za.bsum = P<double>(ctx->bsum);
        za.kperm = P<int32_t>(ctx->kperm);
        za.lo = R.lo;
        za.kn_dev = P<int32_t>(ctx->next) + 2;
        Scope sc(ctx, PVT_K_COMMIT, 0, 0, nullptr, "zwalk_kernel");
        launch_zwalk_keyed(za, true, ctx->stream);
      }
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(ctx->next_host, P<int32_t>(ctx->next), sizeof(int32_t) * 3,
                            hipMemcpyDeviceToHost, ctx->stream));
      HIPCHK(hipStreamSynchronize(ctx->stream));
      const int nz = ctx->next_host[2];
      if (zk) {
        const int done = ctx->next_host[0];
        if ((rc = frontier_walked(ctx, "keyed", done, n_g))) return rc;
        R.t0 += done;
      }
      if (nz >= KPREFIX_MIN && nz < n) {
        R.kmode = 1;
        R.kn = nz;
        HIPCHK(hipMemsetAsync(P<uint64_t>(ctx->kskey) + n, 0, sizeof(uint64_t) * nz, ctx->stream));
      } else {
        if ((rc = keyed_full_sort(ctx))) return rc;
      }
    }
    R.key_group = (int)R.g;
  }
  if (R.t0 >= ge) continue;       // the frontier walk took the whole group
  R.nt = std::min(R.W, ge - R.t0);
  *nt_out = R.nt;
  return PVT_OK;
  }
}

// Exact candidate lists of tasks [t0, t0 + nt) over hosts [lo, hi) into list buffer `lb`, on
// stream `st`.
int pvt::window_lists(pvt_ctx* ctx, int t0, int nt, int lb, hipStream_t st) {
  RoundState& R = ctx->rs;
  const pvt_round* r = &R.r;
  const int Hl = R.hi - R.lo;
  ctx->windows++;
  Lists L;
  lists_from(ctx, L, lb);
  const double bpc = bytes_per_candidate(r->mode);
  const double* dem_w = P<double>(ctx->dem_ord) + (size_t)t0 * 4;
  const int32_t* anc_w = P<int32_t>(ctx->anc_ord) + t0;
  if (R.kscan) {
    const int n = R.hi - R.lo;
    PermArgs pa{r->avail, r->zone, P<uint64_t>(ctx->kskey) + n, P<int32_t>(ctx->kperm), dem_w,
                anc_w, R.ord + t0, R.H, nt, n > 0 ? R.kn : 0, KSCAN_DEPTH, R.lo,
                R.kmode == 1 ? 1 : 0, std::numeric_limits<double>::denorm_min(), L};
    Scope sc(ctx, PVT_K_SCORE, (double)nt * Hl, (double)nt * Hl * bpc, st, "perm_scan_kernel");
    launch_perm_scan(pa, st);
  } else if (R.ordered) {
    OrderedArgs oa{r->avail, r->zone, dem_w, anc_w, R.ord + t0, R.H, nt,
                   r->mode == PVT_CA_FF ? 1 : 0, R.lo, R.hi, L};
    Scope sc(ctx, PVT_K_SCORE, (double)nt * Hl, (double)nt * Hl * bpc, st, "ordered_kernel");
    launch_ordered(oa, st);
  } else if (R.band) {
    const int S = R.band_S;
    ENSURE(ctx->seg, sizeof(SegEntry) * (size_t)nt * S * KL);
    ENSURE(ctx->seg_feas, sizeof(int32_t) * (size_t)nt * S);
    const int n = R.hi - R.lo;
    // Representative rows (unsharded rounds, walked by the one-wave list walk, which maps each
    // task to its row): one list per run of equal demands instead of one per task.
    const bool reps = !R.runs.empty() && !R.full_lists;
    R.reps[lb] = reps;
    const double* dem_l = dem_w;
    const int32_t* nt_dev = nullptr;
    int nt_l = nt;
    if (reps) {                   // the rows: the runs the window spans
      const int b0 = R.runs[t0];
      R.rbase[lb] = b0;
      nt_l = R.runs[t0 + nt - 1] - b0 + 1;
      dem_l = P<double>(ctx->brdem) + (size_t)b0 * 4;
    }
    BandArgs ba{P<uint64_t>(ctx->bkey) + n, P<double>(ctx->bsa), P<uint32_t>(ctx->bstb),
                P<int32_t>(ctx->bidx) + n, n, R.lo, R.hi, P<uint8_t>(ctx->btouch),
                P<int32_t>(ctx->btlist), P<int32_t>(ctx->btcnt), r->avail, r->tiebreak, R.H, dem_l,
                nt_l, S, P<SegEntry>(ctx->seg), P<int32_t>(ctx->seg_feas), nt_dev,
                P<uint8_t>(ctx->bptouch)};
    {
      Scope sc(ctx, PVT_K_SCORE, (double)nt * Hl, (double)nt * Hl * bpc, st, "band_score_kernel");
      launch_band_score(ba, st);
    }
    MergeArgs ma{P<SegEntry>(ctx->seg), P<int32_t>(ctx->seg_feas), r->avail, r->zone, dem_l,
                 anc_w, R.ord + t0, R.H, nt_l, S, KL, L, nt_dev, ctx->t_merge_bitonic};
    Scope sc(ctx, PVT_K_MERGE, 0, 0, st, merge_kernel_name(ma));
    launch_merge(ma, st);
  } else {
    const int S = choose_segments(Hl, nt, r->mode, ctx->score_tw, R.in_epoch, ctx->t_segments, R.Z);
    ENSURE(ctx->seg, sizeof(SegEntry) * (size_t)nt * S * KL);
    ENSURE(ctx->seg_feas, sizeof(int32_t) * (size_t)nt * S);
    ScoreArgs sa{r->avail, r->zone, r->tiebreak, R.keyed ? P<double>(ctx->key) : nullptr,
                 dem_w, anc_w, P<double>(ctx->csum), P<double>(ctx->bsum), R.H, R.Z, nt, S,
                 R.lo, R.hi, P<SegEntry>(ctx->seg), P<int32_t>(ctx->seg_feas), ctx->score_tw,
                 r->mode == PVT_CA_BF ? r->rt_bw : nullptr, P<int32_t>(ctx->grp_ord) + t0};
    {
      Scope sc(ctx, PVT_K_SCORE, (double)nt * Hl, (double)nt * Hl * bpc, st, "score_kernel");
      launch_score(r->mode, sa, st);
    }
    MergeArgs ma{P<SegEntry>(ctx->seg), P<int32_t>(ctx->seg_feas), r->avail, r->zone, dem_w,
                 anc_w, R.ord + t0, R.H, nt, S, KL, L, nullptr, ctx->t_merge_bitonic};
    Scope sc(ctx, PVT_K_MERGE, 0, 0, st, merge_kernel_name(ma));
    launch_merge(ma, st);
  }
  HIPCHK(hipGetLastError());
  return PVT_OK;
}

// Launch the commit walk of tasks [t0, t0 + nt) on list buffer `lb` (inheriting n_prev hosts
// from the other buffer's walk); status -> ctx->next_host after a sync.
int pvt::walk_launch(pvt_ctx* ctx, int t0, int nt, int lb, int n_prev) {
  RoundState& R = ctx->rs;
  const pvt_round* r = &R.r;
  hipStream_t st = ctx->stream;
  int32_t* status = P<int32_t>(ctx->next);
  CommitArgs ca_ = commit_args(ctx, t0, nt, lb, n_prev, status);
  R.lw_last = r->mode == PVT_VBP_BF && ctx->lwalk && n_prev <= 2048;
  R.lw_lb = lb;
  R.lw_prev = n_prev;
  if (ca_.rowmap && !R.lw_last)
    return fail(ctx, PVT_EHIP, "representative lists need the one-wave list walk");
  R.lw_flag = R.lw_last;
  if (R.lw_flag) {               // the walk reports to mapped pinned words: the host polls them
    ca_.hflag = ctx->flag_hdev + 4;
    ca_.hseq = ++ctx->walk_seq;
  }
  {
    Scope sc(ctx, PVT_K_COMMIT, 0, 0, nullptr, R.lw_last ? "lwalk_kernel" : "commit_kernel");
    if (R.lw_last) launch_lwalk(ca_, st);
    else launch_commit(ca_, st);
  }
  HIPCHK(hipGetLastError());
  if (!R.lw_flag)
    HIPCHK(hipMemcpyAsync(ctx->next_host, status, sizeof(int32_t) * 2, hipMemcpyDeviceToHost, st));
  if (R.band) { R.touch_lb = lb; R.touch_status = status; }   // its hosts become touched before
                                                              // the next band score
  return PVT_OK;
}

// Window-size adaptation after a walk that advanced `adv` of `nt` tasks.
void pvt::adapt_window(pvt_ctx* ctx, int adv, int nt) {
  RoundState& R = ctx->rs;
  if (adv < nt) {
    ctx->refills++;
    R.W = std::max(std::min(64, R.Wmax), std::min(R.Wmax, adv + adv / 2));
  } else if (nt == R.W) {
    R.W = std::min(R.Wmax, 2 * R.W);
  }
}

// The one-wave list walk could not start the window [t0, t0 + nt) (R.lw_lb, R.lw_prev): the
// list walk walks it instead; *adv = where it stopped (after a synchronisation).
static int lw_fallback(pvt_ctx* ctx, int t0, int nt, int* adv) {
  // the one-wave list walk could not start this window (its first task's list ends before
  // its bound, or too many inherited hosts): the list walk walks it, on the same lists
  RoundState& R = ctx->rs;
  if (R.reps[R.lw_lb]) {
    // representative rows: the list walk reads one list per task, so the window is scored
    // again with one (on the current state: capacities only fall, and the inherited hosts are
    // rescored as touched). The side stream's scoring shares the segment scratch: wait for it.
    if (ctx->side) HIPCHK(hipStreamSynchronize(ctx->side));
    R.full_lists = true;
    const int rc = window_lists(ctx, t0, nt, R.lw_lb, ctx->stream);
    R.full_lists = false;
    if (rc) return rc;
  }
  // (one list per task by now: no representative-row fields)
  const CommitArgs ca_ = commit_args(ctx, t0, nt, R.lw_lb, R.lw_prev, P<int32_t>(ctx->next));
  R.lw_last = false;
  {
    Scope sc(ctx, PVT_K_COMMIT, 0, 0, nullptr, "commit_kernel");
    launch_commit(ca_, ctx->stream);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(ctx->next_host, P<int32_t>(ctx->next), sizeof(int32_t) * 2,
                        hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  *adv = ctx->next_host[0];
  return PVT_OK;
}

int pvt::walk_status(pvt_ctx* ctx, int t0, int nt, bool inherited, int* adv) {
  if (ctx->rs.lw_flag) {
    ctx->rs.lw_flag = false;
    int rc = wait_host_flag(ctx, ctx->flag_host + 4, ctx->walk_seq, "list walk");
    if (rc) return rc;
    ctx->next_host[0] = __atomic_load_n(ctx->flag_host + 5, __ATOMIC_ACQUIRE);
    ctx->next_host[1] = __atomic_load_n(ctx->flag_host + 6, __ATOMIC_ACQUIRE);
  } else {
    HIPCHK(hipStreamSynchronize(ctx->stream));
  }
  *adv = ctx->next_host[0];
  if (*adv == 0 && ctx->rs.lw_last) {
    int rc = lw_fallback(ctx, t0, nt, adv);
    if (rc) return rc;
  }
  if (*adv == -1) return fail(ctx, PVT_EHIP, "commit walk: ring hand-off timed out at task %d", t0);
  if (*adv < 0 || *adv > nt) return fail(ctx, PVT_EHIP, "commit walk returned %d of %d", *adv, nt);
  if (*adv == 0 && !inherited) {
    RoundState& R = ctx->rs;
    // a zero-key prefix ran dry: sort the rest. Host-sharded, the prefix may be another rank's:
    // each rank chooses prefix or full sort by the zero-key hosts of its own range, while the walk
    // and its report are the same everywhere. A rank whose own order is complete (or that has no
    // host) takes the same step, once per task, and scores the window again.
    const bool others = R.sharded && R.world > 1 && R.kstall_t0 != t0;
    if (R.kscan && (R.kmode == 1 || others)) {
      R.kstall = true;
      R.kstall_t0 = t0;
      return PVT_OK;
    }
    return fail(ctx, PVT_EHIP, "commit walk made no progress at task %d", t0);
  }
  return PVT_OK;
}

// vbp first-fit and unsorted cost_aware first-fit (host index order; fit >= / strict): the
// frontier walk (pvt_zwalk.hip, keyed mode) over the first ZW_M alive hosts -- those fitting the
// smallest demand of the remaining tasks, in index order; no other host can take any of them --
// takes tasks until one fits no window host; the window is rebuilt from the current capacities
// and the walk goes on while each attempt places at least ORDERED_FRONTIER_MIN tasks, then one
// list window (which handles tasks that fit far away or nowhere) and the frontier again.
static int ordered_frontier(pvt_ctx* ctx) {
  RoundState& R = ctx->rs;
  if (!R.ofront) return PVT_OK;
  const pvt_round* r = &R.r;
  hipStream_t st = ctx->stream;
  const bool strict = r->mode == PVT_CA_FF;
  int rc;
  while (R.T - R.t0 >= ORDERED_FRONTIER_MIN) {
    // a bounded task prefix: its smallest demand is close to each task's own (decreasing
    // orders), so hosts filled too far for it leave the window
    const int n = std::min(R.T - R.t0, R.of_tasks);
    const double* dem = P<double>(ctx->dem_ord) + (size_t)R.t0 * 4;
    // the window comes from the first R.ofh hosts (a window of fewer than ZW_M hosts stops the
    // walk at the first task fitting none of them, which is still the answer for the tasks
    // before it); the span doubles when an attempt stops on a short window
    const int hs = std::min(R.ofh, R.H);
    {
      Scope sc(ctx, PVT_K_OTHER, 0, 0);
      launch_alive_flags(r->avail, R.H, 0, hs, dem, n, strict ? 1 : 0, P<double>(ctx->hmin),
                         P<uint8_t>(ctx->kflag), st);
      if ((rc = compact_flags(ctx, hs, st))) return rc;
    }
    ENSURE(ctx->wres, sizeof(WinRec) * (size_t)n);
    ZwalkArgs za = zwalk_keyed_args(ctx, R.t0, n);
    za.kperm = P<int32_t>(ctx->kperm);
    za.kn_dev = P<int32_t>(ctx->next) + 2;
    {
      Scope sc(ctx, PVT_K_COMMIT, 0, 0, nullptr, "zwalk_kernel");
      launch_zwalk_keyed(za, strict, st);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(ctx->next_host, P<int32_t>(ctx->next), sizeof(int32_t) * 3,
                          hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const int done = ctx->next_host[0];
    bool again = false;
    if ((rc = ordered_verdict(ctx, "ordered", done, n, hs, &again))) return rc;
    R.t0 += done;
    if (!again) break;
  }
  return PVT_OK;
}

// pvt_place for the list policies. While window k is walked on the caller's stream, the side
// stream scores window k+1 on the capacities as they stand (the walk of k-1 is complete; the
// walk of k is in flight): an event recorded just before walk k releases it. The side stream
// runs on all but a few CUs (create_side_stream), so the score grid never holds back the walk,
// which needs a whole CU's LDS. Hosts window k commits to are the only ones whose list entries
// can be stale, so walk k+1 inherits them as touched (pvt_walk.hip) and stays exact. A walk that
// stops early (refill) discards the speculative lists; keyed first-fit recomputes its frozen
// key at a group start, so the pipeline drains at group boundaries.
static int place_pipelined(pvt_ctx* ctx) {
  RoundState& R = ctx->rs;
  int rc, nt = 0;
  if ((rc = ordered_frontier(ctx))) return rc;
  if ((rc = round_next_window(ctx, &nt))) return rc;
  if (nt == 0) return PVT_OK;
  int lb = 0, t0 = R.t0;
  if ((rc = window_lists(ctx, t0, nt, lb, ctx->stream))) return rc;
  int n_prev = 0;
  bool inherited = false;
  for (;;) {
    // Walk k, and beside it window k+1 (same group) scored on the state walk k-1 left.
    const int nt0 = t0 + nt, ge = group_end(R, t0);
    // (ordered frontier rounds: no speculative window; the frontier walk is tried after each)
    const int nnt = (ctx->pipeline && nt0 < ge && !R.ofront) ? std::min(R.W, ge - nt0) : 0;
    flush_touched(ctx);   // the previous walk's hosts, seen by the score pass launched next
    if (nnt > 0) HIPCHK(hipEventRecord(ctx->ev_walk, ctx->stream));
    if ((rc = walk_launch(ctx, t0, nt, lb, n_prev))) return rc;
    if (nnt > 0) {
      HIPCHK(hipStreamWaitEvent(ctx->side, ctx->ev_walk, 0));
      if ((rc = window_lists(ctx, nt0, nnt, 1 - lb, ctx->side))) return rc;
      HIPCHK(hipEventRecord(ctx->ev_lists, ctx->side));
    }
    int adv = 0;
    if ((rc = walk_status(ctx, t0, nt, inherited, &adv))) return rc;
    const int n_own = ctx->next_host[1];
    adapt_window(ctx, adv, nt);
    if (adv == nt && nnt > 0) {                 // take the speculative window
      HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->ev_lists, 0));
      t0 = nt0; nt = nnt; lb = 1 - lb; n_prev = n_own; inherited = true;
      continue;
    }
    if (nnt > 0) HIPCHK(hipStreamSynchronize(ctx->side));   // discard the speculation
    flush_touched(ctx);
    R.t0 = t0 + adv;
    if ((rc = ordered_frontier(ctx))) return rc;
    if ((rc = round_next_window(ctx, &nt))) return rc;
    if (nt == 0) break;
    t0 = R.t0; lb = 0; n_prev = 0; inherited = false;
    if ((rc = window_lists(ctx, t0, nt, lb, ctx->stream))) return rc;
  }
  return PVT_OK;
}

// The windowed / epoch / opportunistic engines on a checked round of device arrays (pvt_place
// without the resident case); synchronises before returning.
int pvt::place_windowed(pvt_ctx* ctx, const pvt_round* r) {
  int rc;
  if (r->mode == PVT_OPP) {
    ctx->rs.active = false;
    ctx->windows = ctx->refills = 0;
    HIPCHK(hipSetDevice(ctx->device));
    if (r->n_tasks == 0) return PVT_OK;
    HIPCHK(hipMemsetAsync(r->placement, 0xff, sizeof(int32_t) * r->n_tasks, ctx->stream));
    launch_iota(r->order, r->n_tasks, ctx->stream);
    return opp_round(ctx, r);
  }
  ctx->rs.sharded = false;
  if ((rc = round_begin(ctx, r, 0, r->n_hosts, 1))) return rc;
  ctx->n_epochs = ctx->n_segs = ctx->n_rejected = 0;
  ctx->n_zchains = ctx->n_gchains = ctx->n_longest = ctx->n_fastpro = 0;
  if ((rc = epoch_groups(ctx))) return rc;
  rc = (ctx->rs.egs.empty() || ctx->rs.ffe) ? place_pipelined(ctx) : place_epochs(ctx);
  if (!rc && ctx->rs.ep_to_lists) rc = place_pipelined(ctx);   // (a wide round handed over, from R.t0)
  ctx->rs.active = false;
  if (rc) {
    (void)hipStreamSynchronize(ctx->side);
    return rc;
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return PVT_OK;
}
