// pvt_capi.hip — the C ABI (include/pivot_place.h): context, scratch, profiling, round checks and
// the entry points pvt_place / pvt_place_batch / pvt_anchor / pvt_meter / pvt_meter_usage /
// pvt_host_ops_apply / pvt_host_meter_apply / pvt_host_meter_finish / pvt_rt_rows (pvt_driver.h lists the
// driver's other files).
//
// pvt_place() replaces the body of a reference policy's schedule() (scheduler/__init__.py:79-80,
// called at :103). A round runs as:
//   1. a2 order: tasks grouped (cost_aware groups, cost_aware.py:37) and stably sorted by
//      descending ||d||2 (cost_aware.py:60-61, vbp.py:17,41) with two stable radix sorts.
//   2. windows of up to W tasks: candidate lists for the window on the current state (score +
//      merge kernels, or the ordered scan for index-order first-fit), then the commit walk. A
//      walk that meets an exhausted list stops early; the next window starts at that task.
//   3. cost_aware first-fit with sort_hosts recomputes the frozen host key at every group start
//      (cost_aware.py:118-119), so its windows never cross a group boundary.
// Opportunistic (PVT_OPP) runs its own count/select kernels (pvt_opp.hip).
#include <cstdarg>

#include "pvt_driver.h"
#include "pvt_opp.h"
#include "pvt_anchor.h"
#include "pvt_groups.h"
#include "pvt_meter.h"
#include "pvt_usage.h"
#include "pvt_hostops.h"
#include "pvt_hostmeter.h"
#include "pvt_rtrows.h"
#include "pvt_stamps.h"

int pvt::fail(pvt_ctx* c, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (c) c->err = buf;
  return code;
}

int pvt::ensure(pvt_ctx* ctx, Buf& b, size_t bytes) {
  if (bytes == 0) bytes = 16;
  if (b.n >= bytes) return PVT_OK;
  const size_t want = std::max(bytes, b.n * 3 / 2);
  if (b.p) (void)hipFree(b.p);
  b.p = nullptr;
  b.n = 0;
  if (hipMalloc(&b.p, want) != hipSuccess) {
    b.p = nullptr;
    return fail(ctx, PVT_ENOMEM, "hipMalloc(%zu) failed", want);
  }
  b.n = want;
  return PVT_OK;
}

// ---------------------------------------------------------------- profiling
// Timing-only events: no system-scope fence when they complete (no cache writeback and
// invalidate between the timed kernel and its neighbours; the marker of a default event cost
// ~5 us of idle GPU per record on the default line).
static constexpr unsigned PROFILE_EVENT_FLAGS = hipEventDisableSystemFence;
hipEvent_t pvt::take_event(pvt_ctx* ctx) {
  if (!ctx->evpool.empty()) {
    hipEvent_t e = ctx->evpool.back();
    ctx->evpool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  (void)hipEventCreateWithFlags(&e, PROFILE_EVENT_FLAGS);
  return e;
}
namespace pvt { thread_local TimedEvents g_timed; }
static void harvest(pvt_ctx* ctx) {
  for (auto& t : ctx->pending) {
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, t.a, t.b);
    pvt_kstats& k = ctx->ks[t.kclass];
    k.launches += 1; k.ms += ms; k.candidates += t.candidates; k.bytes += t.bytes;
    if (t.kname) {
      pvt_kstats& n = ctx->kks[t.kname];
      n.launches += 1; n.ms += ms; n.candidates += t.candidates; n.bytes += t.bytes;
    }
    ctx->evpool.push_back(t.a);
    ctx->evpool.push_back(t.b);
  }
  ctx->pending.clear();
}

// ---------------------------------------------------------------- ABI
extern "C" int pvt_abi_version(void) { return PVT_ABI_VERSION; }

// The side stream (the next window's score / count pass while a walk runs) is ordered against
// the walks by events only -- no in-kernel flag polled by the command processor, which never
// completes under serialising tools (rocprofv3 counter collection) -- and runs at the lowest
// queue priority (the context's own stream at the highest), so when walk k and the side pass k+1 become ready together (walk k-1 done)
// the walk, one workgroup that needs a whole CU's LDS, is dispatched first. PVT_WALK_CUS=n keeps
// the side stream off n CUs instead (measured: it serialises the two streams).
static hipError_t create_streams(pvt_ctx* ctx, int ncu) {
  int prio = 1;
  if (const char* e = getenv("PVT_SIDE_PRIO")) prio = atoi(e);
  int least = 0, greatest = 0;
  if (prio && (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess || least == greatest))
    prio = 0;
  hipError_t e = prio ? hipStreamCreateWithPriority(&ctx->own, hipStreamNonBlocking, greatest)
                      : hipStreamCreateWithFlags(&ctx->own, hipStreamNonBlocking);
  if (e != hipSuccess) return e;
  int cus = 0;
  if (const char* e = getenv("PVT_WALK_CUS")) cus = atoi(e);   // tuning experiments
  if (cus > 0 && ncu > 2 * cus) {
    std::vector<uint32_t> mask((ncu + 31) / 32, 0u);
    const int stride = ncu / cus;
    int kept = 0;
    for (int i = 0; i < ncu; i++)
      if (i % stride != stride - 1 || i / stride >= cus) { mask[i / 32] |= 1u << (i % 32); kept++; }
    if (hipExtStreamCreateWithCUMask(&ctx->side, (uint32_t)mask.size(), mask.data()) == hipSuccess) {
      ctx->walk_cus = ncu - kept;
      return hipSuccess;
    }
    (void)hipGetLastError();
  }
  ctx->walk_cus = 0;
  if (prio) return hipStreamCreateWithPriority(&ctx->side, hipStreamNonBlocking, least);
  return hipStreamCreateWithFlags(&ctx->side, hipStreamNonBlocking);
}

extern "C" int pvt_ctx_create(int device, pvt_ctx** out) {
  if (!out) return PVT_EINVAL;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= device || device < 0) return PVT_ENODEV;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return PVT_ENODEV;
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return PVT_ENODEV;
  pvt_ctx* ctx = new pvt_ctx();
  ctx->device = device;
  ctx->n_cus = prop.multiProcessorCount;
  std::memset(ctx->ks, 0, sizeof(ctx->ks));
  if (hipSetDevice(device) != hipSuccess ||
      create_streams(ctx, prop.multiProcessorCount) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->ev_lists, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->ev_walk, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->ev_stage, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->ev_rstage, hipEventDisableTiming) != hipSuccess ||
      init_kernel_attrs() != hipSuccess || pvt::opp_init_attrs() != hipSuccess ||
      score_init_attrs() != hipSuccess ||
      resident_init_attrs() != hipSuccess || lwalk_init_attrs() != hipSuccess ||
      hipHostMalloc((void**)&ctx->next_host, sizeof(int32_t) * 4) != hipSuccess ||
      hipHostMalloc((void**)&ctx->flag_host, sizeof(int32_t) * 16, hipHostMallocCoherent) != hipSuccess ||
      hipHostGetDevicePointer((void**)&ctx->flag_hdev, ctx->flag_host, 0) != hipSuccess ||
      hipHostMalloc((void**)&ctx->ep_host, sizeof(int32_t) * EP_WORDS) != hipSuccess ||
      hipHostGetDevicePointer((void**)&ctx->ep_hdev, ctx->ep_host, 0) != hipSuccess) {
    delete ctx;
    return PVT_EHIP;
  }
  std::memset(ctx->flag_host, 0, sizeof(int32_t) * 16);   // (flag_seq starts at 0: no stale 1)
  ctx->stream = ctx->own;
  if (const char* e = getenv("PVT_OF_TASKS")) ctx->of_tasks = std::max(32, atoi(e));   // tuning
  if (const char* e = getenv("PVT_BAND")) ctx->band_min = std::max(0, atoi(e));       // A/B
  if (const char* e = getenv("PVT_LWALK")) ctx->lwalk = atoi(e) != 0;                  // A/B
  if (const char* e = getenv("PVT_RWALK")) ctx->rwalk = atoi(e);                       // A/B
  if (const char* e = getenv("PVT_FUSED")) ctx->fused = atoi(e) != 0;                  // A/B
  if (const char* e = getenv("PVT_BIND_EVENTS")) ctx->bind_events = atoi(e) != 0;      // A/B
  if (const char* e = getenv("PVT_SEGMENTS")) ctx->t_segments = std::max(1, atoi(e));  // tuning
  if (const char* e = getenv("PVT_BAND_SEGS")) ctx->t_band_segs = atoi(e);             // tuning
  if (const char* e = getenv("PVT_KEYED_SCAN")) ctx->t_keyed_scan = atoi(e) != 0;      // A/B
  if (const char* e = getenv("PVT_OF_HOSTS")) ctx->t_of_hosts = std::max(ZW_M, atoi(e));   // tuning
  if (const char* e = getenv("PVT_EPOCH_PLAN")) ctx->t_epoch_plan = atoi(e);           // A/B
  if (const char* e = getenv("PVT_ZPRE")) ctx->t_zpre = atoi(e) != 0;                  // A/B
  if (const char* e = getenv("PVT_CHAIN_TAB")) ctx->t_chain_tab = atoi(e) != 0;        // A/B
  if (const char* e = getenv("PVT_EPOCH_TAIL")) ctx->t_epoch_tail = atoi(e) != 0;      // A/B
  if (const char* e = getenv("PVT_CHAIN_CERT")) ctx->t_chain_cert = atoi(e) != 0;      // A/B
  if (const char* e = getenv("PVT_ZW_RUNREM")) ctx->t_zw_runrem = atoi(e) != 0;        // A/B
  if (const char* e = getenv("PVT_ZW_WIDE")) ctx->t_zw_wide = atoi(e) != 0;            // A/B
  if (const char* e = getenv("PVT_MERGE_SMALL")) ctx->t_merge_bitonic = atoi(e) == 0;  // A/B
  if (const char* e = getenv("PVT_RES_WAVES")) ctx->res_waves = atoi(e) == 8 ? 8 : atoi(e) == 2 ? 2 : atoi(e) == 1 ? 1 : 4;  // A/B
  *out = ctx;
  return PVT_OK;
}

extern "C" int pvt_ctx_destroy(pvt_ctx* ctx) {
  if (!ctx) return PVT_EINVAL;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  if (ctx->side) (void)hipStreamSynchronize(ctx->side);
  harvest(ctx);
  Buf* bufs[] = {&ctx->ord, &ctx->ord2, &ctx->keys64a, &ctx->keys64b, &ctx->keys32a, &ctx->keys32b,
                 &ctx->sorttmp, &ctx->dem_ord, &ctx->anc_ord, &ctx->grp_ord, &ctx->csum, &ctx->bsum, &ctx->key,
                 &ctx->seg, &ctx->seg_feas, &ctx->l_e[0], &ctx->l_ids[0], &ctx->l_t[0],
                 &ctx->l_e[1], &ctx->l_ids[1], &ctx->l_t[1], &ctx->next, &ctx->opp, &ctx->pkg,
                 &ctx->owned[0], &ctx->owned[1], &ctx->rdesc, &ctx->rmt, &ctx->anc_scr, &ctx->oppfault, &ctx->hdev, &ctx->kskey, &ctx->kperm, &ctx->kiota,
                 &ctx->ksorttmp, &ctx->kflag, &ctx->ep_dev, &ctx->wres, &ctx->hmin, &ctx->cmax, &ctx->fwin,
                 &ctx->bkey, &ctx->bidx, &ctx->bsa, &ctx->bstb, &ctx->btouch, &ctx->btlist,
                 &ctx->btcnt, &ctx->bsorttmp, &ctx->brun, &ctx->brdem, &ctx->bpos, &ctx->bptouch, &ctx->zt_dev,
                 &ctx->zwin, &ctx->zundo, &ctx->gcert, &ctx->run_rem, &ctx->zpairs, &ctx->zcomp, &ctx->brec, &ctx->chk_desc, &ctx->chk_slots, &ctx->chk_rep,
                 &ctx->chk_owner, &ctx->ho_key, &ctx->ho_idx, &ctx->ho_tmp, &ctx->ho_flag,
                 &ctx->hm_key, &ctx->hm_idx, &ctx->rt_val, &ctx->rt_flag};
  for (Buf* b : bufs)
    if (b->p) (void)hipFree(b->p);
  for (hipEvent_t e : ctx->evpool) (void)hipEventDestroy(e);
  if (ctx->next_host) (void)hipHostFree(ctx->next_host);
  if (ctx->flag_host) (void)hipHostFree(ctx->flag_host);
  if (ctx->ep_host) (void)hipHostFree(ctx->ep_host);
  if (ctx->gstage) (void)hipHostFree(ctx->gstage);
  if (ctx->hst) (void)hipHostFree(ctx->hst);
  if (ctx->rstage) (void)hipHostFree(ctx->rstage);
  if (ctx->rmt_host) (void)hipHostFree(ctx->rmt_host);
  if (ctx->ev_lists) (void)hipEventDestroy(ctx->ev_lists);
  if (ctx->ev_walk) (void)hipEventDestroy(ctx->ev_walk);
  if (ctx->ev_stage) (void)hipEventDestroy(ctx->ev_stage);
  if (ctx->ev_rstage) (void)hipEventDestroy(ctx->ev_rstage);
  if (ctx->side) (void)hipStreamDestroy(ctx->side);
  if (ctx->own) (void)hipStreamDestroy(ctx->own);
  delete ctx;
  return PVT_OK;
}

extern "C" int pvt_ctx_set_stream(pvt_ctx* ctx, void* stream) {
  if (!ctx) return PVT_EINVAL;
  ctx->stream = (hipStream_t)stream;   // NULL is the device's default (null) stream
  return PVT_OK;
}

// Events of the timed scopes come from a pool that harvest() refills; the pool is filled and
// every event recorded once when profiling is switched on, so a timed round neither creates an
// event nor pays a first record (measured ~11 us on the default line's critical path).
static constexpr size_t EVPOOL_WARM = 1024;
extern "C" int pvt_set_profiling_kernel(pvt_ctx* ctx, const char* kernel) {
  if (!ctx) return PVT_EINVAL;
  ctx->prof_only = kernel ? kernel : "";
  return PVT_OK;
}

extern "C" int pvt_set_profiling(pvt_ctx* ctx, int on) {
  if (!ctx) return PVT_EINVAL;
  ctx->profiling = on == 2 ? 2 : (on != 0 ? 1 : 0);
  if (ctx->profiling && ctx->evpool.size() + 2 * ctx->pending.size() < EVPOOL_WARM) {
    (void)hipSetDevice(ctx->device);
    while (ctx->evpool.size() + 2 * ctx->pending.size() < EVPOOL_WARM) {
      hipEvent_t e = nullptr;
      if (hipEventCreateWithFlags(&e, PROFILE_EVENT_FLAGS) != hipSuccess) break;
      (void)hipEventRecord(e, ctx->stream);
      ctx->evpool.push_back(e);
    }
    (void)hipStreamSynchronize(ctx->stream);
  }
  return PVT_OK;
}
extern "C" int pvt_reset_kstats(pvt_ctx* ctx) {
  if (!ctx) return PVT_EINVAL;
  (void)hipStreamSynchronize(ctx->stream);
  harvest(ctx);
  std::memset(ctx->ks, 0, sizeof(ctx->ks));
  ctx->kks.clear();
  return PVT_OK;
}
extern "C" int pvt_get_kstats(pvt_ctx* ctx, int kclass, pvt_kstats* out) {
  if (!ctx || !out || kclass < 0 || kclass >= PVT_K_COUNT) return PVT_EINVAL;
  (void)hipStreamSynchronize(ctx->stream);
  harvest(ctx);
  *out = ctx->ks[kclass];
  return PVT_OK;
}
extern "C" int pvt_get_kernel_kstats(pvt_ctx* ctx, const char* kernel, pvt_kstats* out) {
  if (!ctx || !kernel || !out) return PVT_EINVAL;
  (void)hipStreamSynchronize(ctx->stream);
  harvest(ctx);
  auto it = ctx->kks.find(kernel);
  if (it == ctx->kks.end()) std::memset(out, 0, sizeof(*out));
  else *out = it->second;
  return PVT_OK;
}
extern "C" int pvt_set_window(pvt_ctx* ctx, int tasks) {
  if (!ctx || tasks < 0) return PVT_EINVAL;
  ctx->window = std::min(tasks, MAX_WINDOW);
  return PVT_OK;
}
extern "C" int pvt_set_score_tw(pvt_ctx* ctx, int tw) {
  if (!ctx || (tw != 0 && tw != 2 && tw != 4)) return PVT_EINVAL;
  ctx->score_tw = tw;
  return PVT_OK;
}
extern "C" int pvt_set_pipeline(pvt_ctx* ctx, int on) {
  if (!ctx) return PVT_EINVAL;
  ctx->pipeline = on != 0;
  return PVT_OK;
}
extern "C" int pvt_set_epochs(pvt_ctx* ctx, int on) {
  if (!ctx) return PVT_EINVAL;
  ctx->epochs = on != 0;
  return PVT_OK;
}
extern "C" int pvt_epoch_stats(pvt_ctx* ctx, int64_t* epochs, int64_t* segments, int64_t* rejected) {
  if (!ctx) return PVT_EINVAL;
  if (epochs) *epochs = ctx->n_epochs;
  if (segments) *segments = ctx->n_segs;
  if (rejected) *rejected = ctx->n_rejected;
  return PVT_OK;
}
extern "C" int pvt_set_band(pvt_ctx* ctx, int32_t min_hosts) {
  if (!ctx || min_hosts < 0) return PVT_EINVAL;
  ctx->band_min = min_hosts;
  return PVT_OK;
}
extern "C" int pvt_set_zero_walk(pvt_ctx* ctx, int on) {
  if (!ctx) return PVT_EINVAL;
  ctx->zwalk = on != 0;
  return PVT_OK;
}
extern "C" int pvt_zero_walk_stats(pvt_ctx* ctx, int64_t* frontier_chains, int64_t* list_chains,
                                   int64_t* longest_chain) {
  if (!ctx) return PVT_EINVAL;
  if (frontier_chains) *frontier_chains = ctx->n_zchains;
  if (list_chains) *list_chains = ctx->n_gchains;
  if (longest_chain) *longest_chain = ctx->n_longest;
  return PVT_OK;
}
extern "C" int pvt_prologue_stats(pvt_ctx* ctx, int64_t* fast_chains) {
  if (!ctx) return PVT_EINVAL;
  if (fast_chains) *fast_chains = ctx->n_fastpro;
  return PVT_OK;
}
extern "C" int pvt_last_stats(pvt_ctx* ctx, int64_t* windows, int64_t* refills) {
  if (!ctx) return PVT_EINVAL;
  if (windows) *windows = ctx->windows;
  if (refills) *refills = ctx->refills;
  return PVT_OK;
}
extern "C" int pvt_last_resident_shape(pvt_ctx* ctx, int32_t* waves, int32_t* hosts_per_lane,
                                       int32_t* wide, uint32_t* switches) {
  if (!ctx) return PVT_EINVAL;
  if (waves) *waves = ctx->rs_waves;
  if (hosts_per_lane) *hosts_per_lane = ctx->rs_hpl;
  if (wide) *wide = ctx->rs_wide;
  if (switches) *switches = ctx->rs_switches;
  return PVT_OK;
}
// Diagnostic (not part of the public ABI): commit-walk phase cycle sums of a PVT_STAMPS build.
extern "C" int pvt_debug_commit_stamps(pvt_ctx* ctx, uint64_t* out, int n) {
  if (!ctx || !out || n < 8) return PVT_EINVAL;
#ifdef PVT_STAMPS
  constexpr int NW = STAMP_WORDS;            // (the slot map: pvt_stamps.h)
  if (!ctx->stamps) {
    if (hipMalloc((void**)&ctx->stamps, sizeof(uint64_t) * NW) != hipSuccess) return PVT_ENOMEM;
    (void)hipMemset(ctx->stamps, 0, sizeof(uint64_t) * NW);
    std::memset(out, 0, sizeof(uint64_t) * std::min(n, NW));
    return PVT_OK;
  }
  if (hipMemcpy(out, ctx->stamps, sizeof(uint64_t) * std::min(n, NW), hipMemcpyDeviceToHost) != hipSuccess)
    return PVT_EHIP;
  return PVT_OK;
#else
  return PVT_EUNSUPPORTED;
#endif
}

// Diagnostic (not part of the public ABI): score-pass candidate counters of a PVT_DIAG build.
extern "C" int pvt_debug_score_counts(pvt_ctx* ctx, uint64_t* out, int n, int reset) {
  if (!ctx || !out || n < 5) return PVT_EINVAL;
  (void)hipSetDevice(ctx->device);
  return pvt::score_diag(out, n, reset);
}

static_assert(PVT_MAX_ZONES == pvt::ZWIDE, "the public zone bound is the wide kernels' bound");
extern "C" int pvt_max_zones(void) { return PVT_MAX_ZONES; }

extern "C" const char* pvt_last_error(pvt_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int pvt::check_round(pvt_ctx* ctx, const pvt_round* r) {
  if (!r) return fail(ctx, PVT_EINVAL, "null round");
  if (r->reserved != 0) return fail(ctx, PVT_EINVAL, "reserved must be 0");
  if (r->n_hosts < 1 || r->n_tasks < 0 || r->n_zones < 1 || r->n_zones > PVT_MAX_ZONES)
    return fail(ctx, PVT_EINVAL, "bad sizes H=%d T=%d Z=%d (1 <= Z <= PVT_MAX_ZONES = %d)", r->n_hosts,
                r->n_tasks, r->n_zones, PVT_MAX_ZONES);
  if (r->mode < PVT_CA_FF || r->mode > PVT_VBP_BF) return fail(ctx, PVT_EINVAL, "bad mode %d", r->mode);
  if (!r->avail || !r->zone) return fail(ctx, PVT_EINVAL, "null host array");
  if (r->n_tasks > 0 && (!r->dem || !r->order || !r->placement))
    return fail(ctx, PVT_EINVAL, "null task array");
  if ((r->mode == PVT_CA_FF || r->mode == PVT_CA_BF) && (!r->cost || !r->bw))
    return fail(ctx, PVT_EINVAL, "cost_aware needs cost and bw");
  if (r->n_tasks > 0 && r->task_group && (r->n_groups < 1 || !r->group_anchor))
    return fail(ctx, PVT_EINVAL, "task_group needs n_groups >= 1 and group_anchor");
  if (r->mode == PVT_VBP_BF && !r->tiebreak) return fail(ctx, PVT_EINVAL, "vbp best-fit needs tiebreak");
  if (r->mode == PVT_OPP && !r->mt_state) return fail(ctx, PVT_EINVAL, "opportunistic needs mt_state");
  if (r->mode == PVT_CA_BF && r->decay && r->n_tasks > 0)
    return fail(ctx, PVT_EUNSUPPORTED, "cost_aware best-fit with host_decay (reference crashes, cost_aware.py:26,81)");
  return PVT_OK;
}

// ---------------------------------------------------------------- content checks (opt-in)
static const char* const CHK_NAMES[CHK_RULES + 1] = {
    "ok", "zone", "avail", "dem", "task_group", "group_anchor", "cost", "bw", "rt_bw", "decay",
    "tiebreak", "mt_state"};

// i: the round's number in its batch, or -1
int pvt::fail_check(pvt_ctx* ctx, int i, const pvt_check_report& p) {
  char where[32] = "";
  if (i >= 0) std::snprintf(where, sizeof(where), "round %d: ", i);
  return fail(ctx, PVT_EINVAL, "%scheck failed: rule %d (%s) at index %lld, value %.17g (%lld "
              "violating, mask 0x%x)", where, p.code, CHK_NAMES[p.code], (long long)p.index, p.value,
              (long long)p.count, (unsigned)p.mask);
}

// Rule 11: the MT19937 position, in host memory.
static void check_mtpos(const pvt_round* r, pvt_check_report* p) {
  if (r->mode != PVT_OPP || !r->mt_state || !chk_bad_mtpos(r->mt_state[624])) return;
  p->mask |= 1 << PVT_CHK_MTPOS;
  if (p->code) return;
  p->code = PVT_CHK_MTPOS;
  p->index = 624;
  p->count = 1;
  p->value = (double)r->mt_state[624];
}

// A round of HOST arrays (pvt_place_host*), already through check_round.
void pvt::check_host_arrays(const pvt_round* r, pvt_check_report* p) {
  check_on_host(check_describe(*r), p);
  check_mtpos(r, p);
}

// n rounds of device arrays: their structure (check_round), then one check launch over all of
// them on the context's stream, one report per round; synchronises. host_mt: the rounds'
// mt_state point at host memory (rule 11 is read there).
static int run_checks(pvt_ctx* ctx, const pvt_round* rounds, int n, pvt_check_report* out,
                      bool host_mt) {
  for (int i = 0; i < n; i++) {
    int rc = check_round(ctx, &rounds[i]);
    if (rc) return rc;
  }
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  std::vector<CheckRound>& cr = ctx->chk_host;
  cr.resize(n);
  size_t owners = 0;
  double bytes = 0.0;
  for (int i = 0; i < n; i++) {
    cr[i] = check_describe(rounds[i]);
    if (cr[i].tiebreak) owners += (size_t)cr[i].H;
    bytes += check_bytes(cr[i]);
  }
  const int grid = check_deal(cr.data(), n, ctx->n_cus);
  ENSURE(ctx->chk_owner, sizeof(uint32_t) * owners);
  ENSURE(ctx->chk_desc, sizeof(CheckRound) * (size_t)n);
  ENSURE(ctx->chk_slots, sizeof(CheckSlots) * (size_t)n);
  ENSURE(ctx->chk_rep, sizeof(pvt_check_report) * (size_t)n);
  owners = 0;
  for (int i = 0; i < n; i++)
    if (cr[i].tiebreak) {
      cr[i].owner = P<uint32_t>(ctx->chk_owner) + owners;
      owners += (size_t)cr[i].H;
    }
  const CheckRound* desc = P<CheckRound>(ctx->chk_desc);
  // (cr stays in the context until the synchronisation below: the upload may read it late)
  HIPCHK(hipMemcpyAsync(ctx->chk_desc.p, cr.data(), sizeof(CheckRound) * (size_t)n, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(ctx->chk_slots.p, 0, sizeof(CheckSlots) * (size_t)n, st));
  if (owners) {
    HIPCHK(hipMemsetAsync(ctx->chk_owner.p, 0xff, sizeof(uint32_t) * owners, st));
    launch_check_owner(desc, n, grid, st);
  }
  {
    Scope sc(ctx, PVT_K_OTHER, 0, bytes, nullptr, "check_kernel");
    launch_check(desc, n, grid, P<CheckSlots>(ctx->chk_slots), st);
  }
  launch_check_finish(desc, n, P<CheckSlots>(ctx->chk_slots), P<pvt_check_report>(ctx->chk_rep), st);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, ctx->chk_rep.p, sizeof(pvt_check_report) * (size_t)n, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (host_mt)
    for (int i = 0; i < n; i++) check_mtpos(&rounds[i], &out[i]);
  return PVT_OK;
}

// pvt_set_checks on: the entry point's rounds, before anything of the placement is launched.
int pvt::gate_checks(pvt_ctx* ctx, const pvt_round* rounds, int n, bool host_mt, bool batch) {
  std::vector<pvt_check_report> rep((size_t)n);
  int rc = run_checks(ctx, rounds, n, rep.data(), host_mt);
  if (rc) return rc;
  for (int i = 0; i < n; i++)
    if (rep[i].code) return fail_check(ctx, batch ? i : -1, rep[i]);
  return PVT_OK;
}

extern "C" int pvt_check_round(pvt_ctx* ctx, const pvt_round* r, pvt_check_report* out) {
  if (!ctx || !out) return PVT_EINVAL;
  if (!r) return fail(ctx, PVT_EINVAL, "null round");
  return run_checks(ctx, r, 1, out, true);
}

extern "C" int pvt_check_batch(pvt_ctx* ctx, const pvt_round* rounds, int32_t n, pvt_check_report* out) {
  if (!ctx) return PVT_EINVAL;
  if (n < 0 || (n > 0 && (!rounds || !out))) return fail(ctx, PVT_EINVAL, "bad batch (%d rounds)", n);
  if (n == 0) return PVT_OK;
  return run_checks(ctx, rounds, n, out, true);
}

extern "C" int pvt_set_checks(pvt_ctx* ctx, int on) {
  if (!ctx) return PVT_EINVAL;
  ctx->checks = on != 0;
  return PVT_OK;
}

extern "C" int pvt_place_batch(pvt_ctx* ctx, const pvt_round* rounds, int32_t n_rounds) {
  if (!ctx) return PVT_EINVAL;
  if (n_rounds < 0 || (n_rounds > 0 && !rounds)) return fail(ctx, PVT_EINVAL, "bad batch (%d rounds)", n_rounds);
  ctx->rs.active = false;
  if (n_rounds == 0) return PVT_OK;
  if (ctx->checks) {
    int rc = gate_checks(ctx, rounds, n_rounds, true, true);
    if (rc) return rc;
  }
  return place_resident(ctx, rounds, n_rounds);
}

extern "C" int pvt_place_batch_mt(pvt_ctx* ctx, const pvt_round* rounds, int32_t n_rounds,
                                  uint32_t* mt_dev) {
  if (!ctx) return PVT_EINVAL;
  if (n_rounds < 0 || (n_rounds > 0 && (!rounds || !mt_dev)))
    return fail(ctx, PVT_EINVAL, "bad batch (%d rounds)", n_rounds);
  ctx->rs.active = false;
  if (n_rounds == 0) return PVT_OK;
  std::vector<pvt_round> rr(rounds, rounds + n_rounds);   // (mt_state: the device rows, so
  for (int i = 0; i < n_rounds; i++) rr[i].mt_state = mt_dev + (size_t)i * 625;   // checks pass)
  if (ctx->checks) {                  // (the states are on the device: rules 1-10)
    int rc = gate_checks(ctx, rr.data(), n_rounds, false, true);
    if (rc) return rc;
  }
  return place_resident(ctx, rr.data(), n_rounds, nullptr, mt_dev);
}

// ---------------------------------------------------------------- anchor resolution (a3)
extern "C" int pvt_anchor(pvt_ctx* ctx, const pvt_anchor_args* a) {
  if (!ctx || !a) return PVT_EINVAL;
  if (a->n_items < 0 || a->n_hosts < 0 || a->n_pred < 0 || a->n_inst < 0)
    return fail(ctx, PVT_EINVAL, "negative size in pvt_anchor_args");
  if (a->n_items == 0) return PVT_OK;
  if (!a->off || !a->mode_host || !a->anchor_zone || (a->n_pred > 0 && (!a->list || !a->zone)) ||
      (a->inst_host == nullptr) != (a->n_inst == 0) || (a->item == nullptr) != (a->n_rows == 0))
    return fail(ctx, PVT_EINVAL, "null pointer in pvt_anchor_args");
  (void)hipSetDevice(ctx->device);
  ENSURE(ctx->anc_scr, 16 + sizeof(int32_t) * (size_t)a->n_items);
  int32_t* bad = P<int32_t>(ctx->anc_scr);   // [0] bad items, [1] deferred count, [4..] list
  HIPCHK(hipMemsetAsync(bad, 0, 16, ctx->stream));
  AnchorArgs k{a->n_items, a->n_hosts, a->n_pred, a->n_inst, a->n_rows, a->off, a->item,
               a->list, a->inst_host, a->zone, a->mode_host, a->anchor_zone, bad, bad + 4, bad + 1};
  {
    Scope sc(ctx, PVT_K_OTHER, 0, 4.0 * (double)a->n_pred);
    launch_anchor(k, ctx->stream);
  }
  HIPCHK(hipGetLastError());
  int32_t nbad = 0;
  HIPCHK(hipMemcpyAsync(&nbad, bad, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (nbad) return fail(ctx, PVT_EINVAL, "%d anchor item(s) with invalid offsets or indices", nbad);
  return PVT_OK;
}

// ---------------------------------------------------------------- meter aggregates (f4)
extern "C" int pvt_meter(pvt_ctx* ctx, const pvt_meter_log* m) {
  if (!ctx || !m) return PVT_EINVAL;
  if (m->n_scen < 0 || m->reserved != 0 || m->n_host_rows < 0 || m->n_iv < 0 ||
      m->n_routes < 0 || m->n_pkts < 0 || m->n_tr < 0)
    return fail(ctx, PVT_EINVAL, "bad size in pvt_meter_log");
  if (m->n_scen == 0) return PVT_OK;
  if (!m->host_off || !m->iv_off || !m->route_off || !m->pkt_off || !m->tr_off ||
      !m->instance_hours || !m->egress_cost || !m->congestion_delay ||
      (m->n_iv && (!m->iv_start || !m->iv_end)) || (m->n_routes && !m->route_cost) ||
      (m->n_tr && (!m->tr_start || !m->tr_end || !m->tr_size)))
    return fail(ctx, PVT_EINVAL, "null pointer in pvt_meter_log");
  (void)hipSetDevice(ctx->device);
  ENSURE(ctx->anc_scr, 16);
  int32_t* bad = P<int32_t>(ctx->anc_scr);
  HIPCHK(hipMemsetAsync(bad, 0, sizeof(int32_t), ctx->stream));
  MeterArgs k{m->n_scen, m->n_host_rows, m->n_iv, m->n_routes, m->n_pkts, m->n_tr,
              m->host_off, m->iv_off, m->route_off, m->pkt_off, m->tr_off,
              m->iv_start, m->iv_end, m->route_cost, m->tr_start, m->tr_end, m->tr_size,
              m->instance_hours, m->egress_cost, m->congestion_delay, bad};
  {
    Scope sc(ctx, PVT_K_OTHER, 0, 16.0 * (double)m->n_iv + 24.0 * (double)m->n_tr);
    launch_meter(k, ctx->stream);
  }
  HIPCHK(hipGetLastError());
  int32_t nbad = 0;
  HIPCHK(hipMemcpyAsync(&nbad, bad, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (nbad) return fail(ctx, PVT_EINVAL, "%d scenario(s) with out-of-range meter offsets", nbad);
  return PVT_OK;
}

// ---------------------------------------------------------------- meter usage series
extern "C" int pvt_meter_usage(pvt_ctx* ctx, const pvt_usage_log* u) {
  if (!ctx || !u) return PVT_EINVAL;
  if (u->n_scen < 0 || u->reserved != 0 || u->n_host_rows < 0 || u->n_iv < 0 || u->n_us < 0 ||
      u->n_buckets < 0 || u->sample_size < 1 || u->sample_size > INT32_MAX)
    return fail(ctx, PVT_EINVAL, "bad size in pvt_usage_log");
  if (u->n_scen == 0) return PVT_OK;
  const bool has_us = u->us_off || u->us_time || u->us_frac;
  if (!u->host_off || !u->iv_off || !u->bucket_off || !u->avg ||
      (u->n_iv && (!u->iv_start || !u->iv_end)) || (u->n_buckets && !u->n_hosts) ||
      (!u->us_off && (has_us || u->n_us)) || (u->n_us && (!u->us_time || !u->us_frac)) ||
      (has_us && u->n_buckets && (!u->res_hosts || !u->res_mean)))
    return fail(ctx, PVT_EINVAL, "null pointer in pvt_usage_log");
  (void)hipSetDevice(ctx->device);
  ENSURE(ctx->anc_scr, 16);
  int32_t* bad = P<int32_t>(ctx->anc_scr);
  HIPCHK(hipMemsetAsync(bad, 0, sizeof(int32_t), ctx->stream));
  UsageArgs k{u->n_scen, u->sample_size, u->n_host_rows, u->n_iv, u->n_us, u->n_buckets,
              u->host_off, u->iv_off, u->us_off, u->bucket_off,
              u->iv_start, u->iv_end, u->us_time, u->us_frac,
              u->n_hosts, u->res_hosts, u->res_mean, u->avg, bad};
  {
    Scope sc(ctx, PVT_K_OTHER, 0,
             16.0 * (double)u->n_iv + 40.0 * (double)u->n_us + 44.0 * (double)u->n_buckets);
    launch_usage(k, ctx->stream);
  }
  HIPCHK(hipGetLastError());
  int32_t nbad = 0;
  HIPCHK(hipMemcpyAsync(&nbad, bad, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (nbad) return fail(ctx, PVT_EINVAL, "%d scenario(s) violating the usage log contract", nbad);
  return PVT_OK;
}

// ---------------------------------------------------------------- resident host levels
extern "C" int pvt_host_ops_apply(pvt_ctx* ctx, const pvt_host_ops* o) {
  if (!ctx || !o) return PVT_EINVAL;
  if (o->n_hosts < 1 || o->n_ops < 0) return fail(ctx, PVT_EINVAL, "bad size in pvt_host_ops");
  if (o->n_ops == 0) return PVT_OK;
  if (!o->capacity || !o->level || !o->op_host || !o->op_kind || !o->op_amt || !o->op_ok)
    return fail(ctx, PVT_EINVAL, "null pointer in pvt_host_ops");
  (void)hipSetDevice(ctx->device);
  const size_t K = (size_t)o->n_ops;
  size_t tmp_bytes = 0;
  HIPCHK(hostops_sort_temp(o->n_hosts, o->n_ops, &tmp_bytes));
  ENSURE(ctx->ho_key, 2 * K * sizeof(uint32_t));
  ENSURE(ctx->ho_idx, 2 * K * sizeof(int32_t));
  ENSURE(ctx->ho_tmp, tmp_bytes);
  ENSURE(ctx->ho_flag, 16);
  uint32_t* bad = P<uint32_t>(ctx->ho_flag);
  HIPCHK(hipMemsetAsync(bad, 0xff, sizeof(uint32_t), ctx->stream));   // HO_NO_BAD
  HostOpsArgs k{o->n_hosts, o->n_ops, o->capacity, o->level, o->op_host, o->op_kind, o->op_amt,
                o->op_ok, P<uint32_t>(ctx->ho_key), P<uint32_t>(ctx->ho_key) + K,
                P<int32_t>(ctx->ho_idx), P<int32_t>(ctx->ho_idx) + K, bad};
  launch_hostops_keys(k, ctx->stream);
  HIPCHK(hostops_sort(k, ctx->ho_tmp.p, tmp_bytes, ctx->stream));
  {
    Scope sc(ctx, PVT_K_OTHER, 0, 60.0 * (double)K, nullptr, "host_ops_kernel");
    launch_hostops_apply(k, ctx->stream);
  }
  HIPCHK(hipGetLastError());
  uint32_t first = HO_NO_BAD;
  HIPCHK(hipMemcpyAsync(&first, bad, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (first != HO_NO_BAD) {
    int32_t hk[2] = {0, 0};
    HIPCHK(hipMemcpy(&hk[0], o->op_host + first, sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&hk[1], o->op_kind + first, sizeof(int32_t), hipMemcpyDeviceToHost));
    return fail(ctx, PVT_EINVAL, "op %u of the host op log: host %d (of %d), kind %d", first,
                hk[0], o->n_hosts, hk[1]);
  }
  return PVT_OK;
}

// ---------------------------------------------------------------- realtime-bandwidth rows
extern "C" int pvt_rt_rows(pvt_ctx* ctx, const pvt_route_queues* q) {
  if (!ctx || !q) return PVT_EINVAL;
  if (q->n_hosts < 1 || q->n_zones < 1 || q->n_zones > PVT_MAX_ZONES || q->n_groups < 0 ||
      q->n_routes < 0 || q->n_packets < 0)
    return fail(ctx, PVT_EINVAL, "bad size in pvt_route_queues: H=%d Z=%d (1 <= Z <= %d) G=%d R=%d P=%lld",
                q->n_hosts, q->n_zones, PVT_MAX_ZONES, q->n_groups, q->n_routes, (long long)q->n_packets);
  const int rows = q->n_groups > 0 ? q->n_groups : 1;
  if ((rows + RT_GROUPS - 1) / RT_GROUPS > 65535)
    return fail(ctx, PVT_EINVAL, "pvt_route_queues: %d groups (at most %d)", q->n_groups, 65535 * RT_GROUPS);
  if (!q->zone || !q->bw || !q->rt_bw || (q->n_groups > 0 && !q->group_anchor))
    return fail(ctx, PVT_EINVAL, "null pointer in pvt_route_queues");
  if (q->n_routes > 0 && (!q->rq_anchor || !q->rq_host || !q->rq_dir || !q->rq_bw || !q->rq_off))
    return fail(ctx, PVT_EINVAL, "null route array in pvt_route_queues");
  if (q->n_packets > 0 && (!q->rq_mbs || q->n_routes == 0))
    return fail(ctx, PVT_EINVAL, "pvt_route_queues: %lld packets of %d routes, rq_mbs %s",
                (long long)q->n_packets, q->n_routes, q->rq_mbs ? "set" : "NULL");
  if ((uintptr_t)q->rt_bw % sizeof(double))
    return fail(ctx, PVT_EINVAL, "pvt_route_queues: rt_bw is not aligned to 8 bytes");
  (void)hipSetDevice(ctx->device);
  const size_t R = (size_t)q->n_routes;
  ENSURE(ctx->rt_val, R * sizeof(double));
  ENSURE(ctx->rt_flag, 16);
  uint32_t* bad = P<uint32_t>(ctx->rt_flag);
  HIPCHK(hipMemsetAsync(bad, 0xff, 4 * sizeof(uint32_t), ctx->stream));   // RT_NO_BAD
  RtRowsArgs a{q->n_hosts, q->n_zones, q->n_groups, q->n_routes, q->n_packets, q->zone, q->bw,
               q->group_anchor, q->rq_anchor, q->rq_host, q->rq_dir, q->rq_bw, q->rq_off, q->rq_mbs,
               P<double>(ctx->rt_val), q->rt_bw, bad};
  launch_rt_check(a, ctx->stream);
  launch_rt_value(a, ctx->stream);
  {
    Scope sc(ctx, PVT_K_OTHER, 0, rtrows_fill_bytes(a), nullptr, "rt_fill_kernel");
    launch_rt_fill(a, ctx->stream);
  }
  launch_rt_patch(a, ctx->stream);
  HIPCHK(hipGetLastError());
  uint32_t first[3] = {RT_NO_BAD, RT_NO_BAD, RT_NO_BAD};
  HIPCHK(hipMemcpyAsync(first, bad, sizeof(first), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (first[0] != RT_NO_BAD) {
    const uint32_t i = first[0];
    int32_t k[3] = {0, 0, 0};
    int64_t off[2] = {0, 0};
    double b = 0.0;
    HIPCHK(hipMemcpy(&k[0], q->rq_anchor + i, sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&k[1], q->rq_host + i, sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&k[2], q->rq_dir + i, sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&b, q->rq_bw + i, sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(off, q->rq_off + i, 2 * sizeof(int64_t), hipMemcpyDeviceToHost));
    return fail(ctx, PVT_EINVAL,
                "entry %u of the route queues: anchor %d (of %d), host %d (of %d), dir %d, bw %.17g, "
                "packets [%lld, %lld) of %lld (keys ascend strictly, bw and packets are > 0)",
                i, k[0], q->n_zones, k[1], q->n_hosts, k[2], b, (long long)off[0], (long long)off[1],
                (long long)q->n_packets);
  }
  if (first[1] != RT_NO_BAD) {
    int32_t an = 0;
    HIPCHK(hipMemcpy(&an, q->group_anchor + first[1], sizeof(int32_t), hipMemcpyDeviceToHost));
    return fail(ctx, PVT_EINVAL, "group_anchor[%u] = %d of the route queues' round (of %d zones)",
                first[1], an, q->n_zones);
  }
  if (first[2] != RT_NO_BAD) {
    int32_t z = 0;
    HIPCHK(hipMemcpy(&z, q->zone + first[2], sizeof(int32_t), hipMemcpyDeviceToHost));
    return fail(ctx, PVT_EINVAL, "zone[%u] = %d of the route queues' cluster (of %d zones)", first[2],
                z, q->n_zones);
  }
  return PVT_OK;
}

// ---------------------------------------------------------------- metered resident cluster
// (levels: the call reads capacity and level; the finish does not)
static bool meter_ok(const pvt_host_meter* m, bool levels) {
  return m->n_hosts >= 1 && m->reserved == 0 && m->iv_cap >= 0 && m->us_cap >= 0 && m->n_iv >= 0 &&
         m->n_us >= 0 && m->n_iv <= m->iv_cap && m->n_us <= m->us_cap &&
         (!levels || (m->capacity && m->level)) && m->st_word && m->st_start && m->st_end &&
         (!m->iv_cap || (m->iv_host && m->iv_start && m->iv_end)) &&
         (!m->us_cap || (m->us_host && m->us_time && m->us_frac));
}

extern "C" int pvt_host_meter_apply(pvt_ctx* ctx, pvt_host_meter* m, const pvt_host_meter_ops* o) {
  if (!ctx || !m || !o) return PVT_EINVAL;
  if (!meter_ok(m, true)) return fail(ctx, PVT_EINVAL, "bad size or null pointer in pvt_host_meter");
  if (o->n_ops < 0 || o->reserved != 0) return fail(ctx, PVT_EINVAL, "bad size in pvt_host_meter_ops");
  if (o->n_ops == 0) return PVT_OK;
  if (!o->op_host || !o->op_kind || !o->op_amt || !o->op_time || !o->op_ok)
    return fail(ctx, PVT_EINVAL, "null pointer in pvt_host_meter_ops");
  const size_t K = (size_t)o->n_ops;
  if (m->n_iv + (int64_t)K > m->iv_cap || m->n_us + (int64_t)K > m->us_cap)
    return fail(ctx, PVT_EINVAL,
                "the meter's logs are full: %lld + %zu intervals of %lld, %lld + %zu usage records "
                "of %lld", (long long)m->n_iv, K, (long long)m->iv_cap, (long long)m->n_us, K,
                (long long)m->us_cap);
  (void)hipSetDevice(ctx->device);
  size_t tmp_bytes = 0;
  HIPCHK(hostops_sort_temp(m->n_hosts, o->n_ops, &tmp_bytes));
  ENSURE(ctx->ho_key, 2 * K * sizeof(uint32_t));
  ENSURE(ctx->ho_idx, 2 * K * sizeof(int32_t));
  ENSURE(ctx->ho_tmp, tmp_bytes);
  ENSURE(ctx->ho_flag, 32);
  uint32_t* bad = P<uint32_t>(ctx->ho_flag);
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(bad + 2);
  unsigned long long cnt_host[2] = {(unsigned long long)m->n_iv, (unsigned long long)m->n_us};
  HIPCHK(hipMemsetAsync(bad, 0xff, sizeof(uint32_t), ctx->stream));   // HO_NO_BAD
  HIPCHK(hipMemcpyAsync(cnt, cnt_host, sizeof(cnt_host), hipMemcpyHostToDevice, ctx->stream));
  HostMeterArgs k{m->n_hosts, o->n_ops, m->capacity, m->level, m->st_word, m->st_start, m->st_end,
                  m->iv_host, m->iv_start, m->iv_end, m->us_host, m->us_time, m->us_frac,
                  o->op_host, o->op_kind, o->op_amt, o->op_time, o->op_ok, m->last_time,
                  P<uint32_t>(ctx->ho_key), P<uint32_t>(ctx->ho_key) + K,
                  P<int32_t>(ctx->ho_idx), P<int32_t>(ctx->ho_idx) + K, bad, cnt};
  launch_hostmeter_keys(k, ctx->stream);
  HIPCHK(hostmeter_sort(k.H, k.K, k.key_in, k.key_out, k.idx_in, k.idx_out, ctx->ho_tmp.p,
                        tmp_bytes, ctx->stream));
  {
    Scope sc(ctx, PVT_K_OTHER, 0, 100.0 * (double)K, nullptr, "host_meter_kernel");
    launch_hostmeter_apply(k, ctx->stream);
  }
  HIPCHK(hipGetLastError());
  struct { uint32_t bad, pad; unsigned long long cnt[2]; } back;
  HIPCHK(hipMemcpyAsync(&back, bad, sizeof(back), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (back.bad != HO_NO_BAD) {
    const uint32_t first = back.bad;
    int32_t hk[2] = {0, 0};
    double t[2] = {m->last_time, 0.0};
    HIPCHK(hipMemcpy(&hk[0], o->op_host + first, sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&hk[1], o->op_kind + first, sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&t[1], o->op_time + first, sizeof(double), hipMemcpyDeviceToHost));
    if (first > 0)
      HIPCHK(hipMemcpy(&t[0], o->op_time + first - 1, sizeof(double), hipMemcpyDeviceToHost));
    return fail(ctx, PVT_EINVAL,
                "entry %u of the metered op log: host %d (of %d), kind %d, time %.17g (after "
                "%.17g), or a capacity of its host that is not positive", first, hk[0], m->n_hosts,
                hk[1], t[1], t[0]);
  }
  m->n_iv = (int64_t)back.cnt[0];
  m->n_us = (int64_t)back.cnt[1];
  HIPCHK(hipMemcpy(&m->last_time, o->op_time + (K - 1), sizeof(double), hipMemcpyDeviceToHost));
  return PVT_OK;
}

extern "C" int pvt_host_meter_finish(pvt_ctx* ctx, const pvt_host_meter* m, pvt_host_meter_out* out) {
  if (!ctx || !m || !out) return PVT_EINVAL;
  if (!meter_ok(m, false)) return fail(ctx, PVT_EINVAL, "bad size or null pointer in pvt_host_meter");
  if (!out->iv_off || !out->us_off) return fail(ctx, PVT_EINVAL, "null pointer in pvt_host_meter_out");
  const int64_t H = m->n_hosts, n_iv = m->n_iv, n_us = m->n_us;
  const int64_t row_max = H < n_us ? H : n_us;
  if (n_iv + H > INT32_MAX || n_us > INT32_MAX)
    return fail(ctx, PVT_EUNSUPPORTED, "pvt_host_meter_finish: more than 2^31 - 1 records");
  (void)hipSetDevice(ctx->device);
  hipStream_t st = ctx->stream;
  out->n_rows = out->n_iv = 0;
  out->n_us = n_us;
  if (n_us == 0) {                    // no mark yet: no state, no rows
    HIPCHK(hipMemsetAsync(out->iv_off, 0, sizeof(int64_t), st));
    HIPCHK(hipMemsetAsync(out->us_off, 0, sizeof(int64_t), st));
    HIPCHK(hipStreamSynchronize(st));
    return PVT_OK;
  }
  if (!out->row_host || !out->iv_start || !out->iv_end || !out->us_time || !out->us_frac)
    return fail(ctx, PVT_EINVAL, "null pointer in pvt_host_meter_out");
  const size_t n_ivk = (size_t)(n_iv + H), n_usk = (size_t)n_us;
  size_t tmp_iv = 0, tmp_us = 0, tmp_scan = 0;
  HIPCHK(hostops_sort_temp(m->n_hosts, (int32_t)n_ivk, &tmp_iv));
  HIPCHK(hostops_sort_temp(m->n_hosts, (int32_t)n_usk, &tmp_us));
  HIPCHK(hostmeter_scan_temp((int32_t)n_usk, &tmp_scan));
  ENSURE(ctx->hm_key, (2 * n_ivk + 2 * n_usk) * sizeof(uint32_t));
  ENSURE(ctx->hm_idx, (2 * n_ivk + 4 * n_usk) * sizeof(int32_t));
  ENSURE(ctx->ho_tmp, std::max(tmp_iv, std::max(tmp_us, tmp_scan)));
  ENSURE(ctx->ho_flag, 32);
  uint32_t* words = P<uint32_t>(ctx->ho_flag);
  const uint32_t words0[HM_WORDS] = {0u, 0xffffffffu, 0u, 0u};
  HIPCHK(hipMemcpyAsync(words, words0, sizeof(words0), hipMemcpyHostToDevice, st));
  uint32_t* key = P<uint32_t>(ctx->hm_key);
  int32_t* idx = P<int32_t>(ctx->hm_idx);
  HostMeterFinish f{};
  f.H = m->n_hosts; f.n_iv = (int32_t)n_iv; f.n_us = (int32_t)n_us; f.n_ivf = 0;
  f.st_word = m->st_word; f.st_start = m->st_start; f.st_end = m->st_end;
  f.iv_host = m->iv_host; f.iv_start = m->iv_start; f.iv_end = m->iv_end;
  f.us_host = m->us_host; f.us_time = m->us_time; f.us_frac = m->us_frac;
  f.ivk_in = key; f.ivk_out = key + n_ivk;
  f.usk_in = key + 2 * n_ivk; f.usk_out = f.usk_in + n_usk;
  f.ivi_in = idx; f.ivi_out = idx + n_ivk;
  f.usi_in = idx + 2 * n_ivk; f.usi_out = f.usi_in + n_usk;
  f.head = f.usi_out + n_usk; f.row = f.head + n_usk;
  f.words = words;
  f.o_row_host = out->row_host; f.o_iv_off = out->iv_off; f.o_us_off = out->us_off;
  f.o_iv_start = out->iv_start; f.o_iv_end = out->iv_end;
  f.o_us_time = out->us_time; f.o_us_frac = out->us_frac;
  launch_hostmeter_tail(f, st);
  HIPCHK(hipGetLastError());
  uint32_t w[HM_WORDS];
  HIPCHK(hipMemcpyAsync(w, words, sizeof(w), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (w[0])
    return fail(ctx, PVT_EINVAL, "%u host(s) with an open interval at finish, the first is host %u",
                w[0], w[1]);
  if ((int64_t)w[2] > row_max)        // (the caller sized its arrays for min(H, n_us) of them)
    return fail(ctx, PVT_EINVAL, "pvt_host_meter: %u closed hosts but %lld usage records", w[2],
                (long long)n_us);
  f.n_ivf = f.n_iv + (int32_t)w[2];
  if (f.n_ivf > 0) {
    HIPCHK(hostmeter_sort(f.H, f.n_ivf, f.ivk_in, f.ivk_out, f.ivi_in, f.ivi_out, ctx->ho_tmp.p,
                          tmp_iv, st));
    launch_hostmeter_iv_gather(f, st);
  }
  launch_hostmeter_us_keys(f, st);
  HIPCHK(hostmeter_sort(f.H, f.n_us, f.usk_in, f.usk_out, f.usi_in, f.usi_out, ctx->ho_tmp.p,
                        tmp_us, st));
  launch_hostmeter_heads(f, st);
  HIPCHK(hostmeter_scan(f, ctx->ho_tmp.p, tmp_scan, st));
  launch_hostmeter_rows(f, st);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(w, words, sizeof(w), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  out->n_rows = (int64_t)w[3];
  out->n_iv = (int64_t)f.n_ivf;
  return PVT_OK;
}

extern "C" int pvt_set_resident(pvt_ctx* ctx, int32_t max_hosts) {
  if (!ctx || max_hosts < 0) return PVT_EINVAL;
  ctx->resident_max = max_hosts;
  return PVT_OK;
}

extern "C" int pvt_place(pvt_ctx* ctx, const pvt_round* r) {
  if (!ctx) return PVT_EINVAL;
  int rc = check_round(ctx, r);
  if (rc) return rc;
  if (ctx->checks && (rc = gate_checks(ctx, r, 1, true, false))) return rc;
  if (r->n_tasks > 0 && resident_fits(r, ctx->resident_max)) {
    ctx->rs.active = false;
    return place_resident(ctx, r, 1);
  }
  return place_windowed(ctx, r);
}
