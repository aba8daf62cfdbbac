// pvt_driver.h -- the host-side driver's shared state (internal; the C ABI is
// include/pivot_place.h): the context and the round state every path reads and writes, the
// error / scratch / profiling helpers, and the functions one driver file calls in another.
//   pvt_capi.hip          context, streams, setters, profiling, round checks, pvt_place, batches
//   pvt_round.hip         processing order, the windowed round: lists, walks, ordered frontier
//   pvt_round_epochs.hip  group-parallel epochs (cost_aware best-fit) and first-fit zero-key epochs
//   pvt_resident.hip      resident rounds and the host-array rounds staged for them
//   pvt_shard.hip         host-sharded rounds (pvt_shard_*)
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "pivot_place.h"
#include "pvt_kernels.h"
#include "pvt_check.h"

using namespace pvt;

// Group-parallel epochs (cost_aware best-fit): at most EPOCH_SEGS group segments, walked in at
// most EPOCH_SEGS chains of <= CHAIN_MAX tasks, and EPOCH_MAX tasks per epoch (its lists: 64 B
// x LMAX per task).
static constexpr int EPOCH_SEGS = 64;
static constexpr int EPOCH_MAX = 16384;
// ep_dev / ep_host words: uploaded [seg_off | seg_chain | seg_cstart | coff | csoff | cseg |
// cmap], then read back [status (2 per chain) | bad (per segment) | res | safe (per segment) |
// cert (per chain: the frontier walk's certificate word, written to ep_host only)]
static constexpr int EP_SEG_OFF = 0, EP_SEG_CHAIN = EP_SEG_OFF + EPOCH_SEGS + 1,
                     EP_SEG_CSTART = EP_SEG_CHAIN + EPOCH_SEGS, EP_COFF = EP_SEG_CSTART + EPOCH_SEGS,
                     EP_CSOFF = EP_COFF + EPOCH_SEGS + 1, EP_CSEG = EP_CSOFF + EPOCH_SEGS + 1,
                     EP_CMAP = EP_CSEG + EPOCH_SEGS, EP_STATUS = EP_CMAP + EPOCH_MAX,
                     EP_BAD = EP_STATUS + 2 * EPOCH_SEGS, EP_RES = EP_BAD + EPOCH_SEGS,
                     EP_SAFE = EP_RES + 8, EP_CERT = EP_SAFE + EPOCH_SEGS;
static constexpr int EP_WORDS = EP_CERT + EPOCH_SEGS;
static constexpr int KEYED_FRONTIER_MIN = 32;   // group tasks worth a frontier-walk launch
static constexpr int ORDERED_FRONTIER_MIN = 32;  // tasks a frontier attempt must place to go on
static constexpr int ORDERED_FRONTIER_TASKS = 4096;   // tasks per frontier attempt (default;
                                                       // config-5 vbp_ff sweep: 512 1.75, 1024
                                                       // 1.09, 2048 0.94, 4096 0.90, 8192 0.98 ms)
static constexpr int ORDERED_FRONTIER_HOSTS = 65536;   // first span of hosts the window is taken from
// vbp best-fit: candidate lists by a memory band over hosts sorted once per round (pvt_band.hip)
// from this many hosts (per shard) on, with this many list segments per task
static constexpr int BAND_MIN_HOSTS = 65536;
static constexpr int BAND_SEGS = 16;

struct Buf {
  void* p = nullptr;
  size_t n = 0;
};

struct TimedLaunch {
  int kclass;
  const char* kname;   // the one kernel the scope brackets (pvt_get_kernel_kstats), or NULL
  double candidates, bytes;
  hipEvent_t a, b;
};

// The next epoch from task t0: consecutive group segments (processing order), each assigned to
// the chain of its anchor's zero-cost component (two groups of one component compete for the
// same hosts: one walk takes them in order). A chain holds at most CHAIN_MAX tasks; a segment
// that ends inside its group ends the epoch (the rest of the group depends on it).
struct EpochPlan {
  std::vector<int> off, chain, cstart;     // segments: window offsets (+ end), chain, start in it
  std::vector<std::vector<int>> segs;      // chains: their segments
  std::vector<int> len;                    // chains: tasks
};

// Package kinds of a host-sharded round (pvt_shard_*): candidate lists of a window, or the
// window candidates of a frontier walk (FrontierHdr + FrontierSlot per chain / walk).
enum { PK_LIST = 0, PK_EPOCH = 1, PK_KEYED = 2, PK_ORDERED = 3 };

struct RoundState {
  pvt_round r;                    // the caller's round (arrays stay caller-owned)
  bool active = false;
  int T = 0, H = 0, Z = 0, lo = 0, hi = 0, world = 0;
  bool keyed = false, ordered = false;
  bool kscan = false;             // keyed first-fit lists from the per-group sorted order
  int kmode = 0;                  // 1: zero-key prefix in host order, 2: full sort
  int kn = 0;                     // hosts in the current order (prefix length in mode 1)
  bool kstall = false;            // a walk found a prefix list exhausted: sort the rest
  int kstall_t0 = -1;             // the task of the last such stall (host-sharded: see walk_status)
  int32_t* ord = nullptr;         // processing order (ctx scratch)
  std::vector<int> gstart, ganchor, gid;   // keyed groups: starts, anchors, caller's group ids
  size_t g = 0, ngroups = 0;
  int key_group = -1;             // group whose frozen first-fit key is computed
  int t0 = 0, W = 0, Wmax = 0, nt = 0;
  int lb = 0;                     // list buffer of the current window
  // host-sharded opportunistic rounds: windows of opp_W tasks; this rank counts super-chunks
  // [opp_sq_lo, opp_sq_hi); packages hold opp_Psq super-chunks per task (the largest share)
  bool opp = false;
  int opp_W = 0, opp_nq = 0, opp_nsq = 0, opp_Psq = 0, opp_sq_lo = 0, opp_sq_hi = 0;
  // host-sharded list rounds, pipelined: the walk in flight (window if_t0 + [0, if_nt) on list
  // buffer if_lb) and the scored window awaiting its exchange (pt0, nt, plb; spec = scored
  // while a walk was in flight, so it inherits that walk's hosts)
  bool inflight = false, spec = false, if_inh = false;   // if_inh: the walk in flight
  int if_t0 = 0, if_nt = 0, if_lb = 0, pt0 = 0, plb = 0;   //   inherited touched hosts
  std::vector<int> egs, ega;      // cost_aware best-fit epochs: group starts (+ T) and anchors
  std::vector<int> ecomp;         // zone -> its component of zones joined by zero egress cost
  std::vector<int> ezcomp;        //   the same whatever PVT_EPOCH_PLAN says (the epoch tail's condition 2)
  bool in_epoch = false;          // lists scored for an epoch (place_epochs)
  bool ofront = false;            // ordered first-fit rounds walked by the frontier walk
  int ofh = 0;                    // hosts the frontier window is taken from
  // grouped rounds: per-group task counts, group anchors and (cost_aware) the cost table,
  // copied to the host once by build_order (one synchronisation) for the group plans
  bool ginfo = false;
  std::vector<int32_t> gcnt, ga_host;
  std::vector<double> cost_host;
  int of_tasks = ORDERED_FRONTIER_TASKS;   // tasks per ordered frontier attempt
  // host-sharded rounds (pvt_shard_*) on the frontier walks: the scored package's kind and size,
  // and what comes next
  bool sharded = false;
  int pkind = PK_LIST;
  int64_t pbytes = 0;
  bool sh_epochs = false;         // cost_aware best-fit: frontier epochs between list windows
  int list_until = 0;             //   list windows up to this task (a chain left unproven), then
                                  //   epochs again
  EpochPlan E;                    //   the epoch of the scored package
  bool of_try = false;            // ordered rounds: a frontier attempt comes next
  int of_n = 0, of_hs = 0;        //   the scored attempt's tasks and host span
  bool kf_pending = false;        // keyed rounds: the group start's frontier walk comes next
  bool ffe = false;               // keyed rounds: first-fit zero-key epochs (ff_epoch)
  bool hmin_pre = false;          // the first epoch's host minima were queued by round_begin
  bool zpre = false;              // ... and its zero-cost windows were prebuilt (ctx->zwin)
  bool gcert = false;             // ... and the groups' certificates were written (ctx->gcert)
  bool runrem = false;            // ... and the gathered tasks' run lengths (ctx->run_rem)
  bool stage_flag = false;        // the grouped order's counts are signalled by ctx->flag_host
  bool gathered = false;          // ... and group_sort_gather_kernel wrote the gathered order
  bool prep_fused = false;        // build_order's order_scatter_kernel filled placement / zone tables
  int ffe_skip = -1;              //   the group they could not start (the keyed path takes it)
  // rounds of more than ZMAX zones: frontier-walked epochs that missed (WIDE_MISS_MAX of them
  // hand the rest of the round to the list windows), and that hand-over from place_epochs at t0
  int wide_misses = 0;
  bool ep_to_lists = false;
  // vbp best-fit band lists (pvt_band.hip): the sorted snapshot of hosts [lo, hi) is built; a
  // walk whose committed hosts are not yet flagged as touched (its own-ids buffer)
  bool band = false;
  int band_S = BAND_SEGS;
  int touch_lb = -1;
  const int32_t* touch_status = nullptr;   //   (its status: [1] = hosts in the own-ids buffer)
  bool reps[2] = {false, false};  //   list buffer b holds representative rows (the round's runs)
  int rbase[2] = {0, 0};          //     the run of its window's first task
  std::vector<int32_t> runs;      //   the round's run ids (band_runs_kernel), on the host
  bool full_lists = false;        //   (one list per task: the list walk's fallback)
  bool lw_last = false;           // the walk in flight is the one-wave list walk (pvt_lwalk.hip)
  bool lw_flag = false;           //   reporting through ctx->flag_host[4..6] (no copy, no sync)
  int lw_lb = 0, lw_prev = 0;     //   its list buffer and inherited hosts (for the fallback)
};

struct pvt_ctx {
  int device = 0;
  hipStream_t own = nullptr, stream = nullptr;
  hipStream_t side = nullptr;     // scores the next window while the current one is walked
  hipEvent_t ev_lists = nullptr;   // side stream: the next window's lists are ready
  hipEvent_t ev_walk = nullptr;    // caller stream: everything before the current walk is done
  hipEvent_t ev_stage = nullptr;   // the grouped order's counts are in the pinned stage
  int walk_cus = 0;                // CUs the side stream leaves to the walks
  std::string err;
  int window = 0;                 // 0: per-policy default
  int64_t windows = 0, refills = 0;
  int profiling = 0;               // 0 off, 1 every launch, 2 the named kernels only
  std::string prof_only;           //   (2: this one named kernel, when set)
  int bind_events = 1;             //   (2: events bound to the kernel's dispatch; PVT_BIND_EVENTS)
  int64_t n_unbound = 0;           //   (2: named scopes whose bound events were dropped)
  pvt_kstats ks[PVT_K_COUNT];
  std::vector<hipEvent_t> evpool;
  std::vector<TimedLaunch> pending;
  std::map<std::string, pvt_kstats> kks;   // per kernel (scopes tagged with its name)
  // scratch
  Buf gcnt, goff, gskey, gsidx;   // grouped order: counts, offsets + cursors, scattered pairs
  Buf ord, ord2, keys64a, keys64b, keys32a, keys32b, sorttmp, dem_ord, anc_ord, grp_ord, csum, bsum, key,
      seg, seg_feas, l_e[2], l_ids[2], l_t[2], next, opp, pkg, owned[2], rdesc, rmt, anc_scr, oppfault, kskey, kperm, kiota, ksorttmp, kflag;
  int pipeline = 1;               // overlap scoring of window k+1 with the walk of window k
  int keyed_scan = 1;             // keyed first-fit: sorted host order + early-exit scan
  int score_tw = 0;               // score kernel tasks per wave (0: policy default; 2 or 4)
  int resident_max = PVT_RESIDENT_MAX_HOSTS;   // pvt_place: resident kernel up to this many hosts
  int epochs = 1;                 // cost_aware best-fit: group-parallel speculative epochs
  int64_t n_epochs = 0, n_segs = 0, n_rejected = 0;
  int64_t n_zchains = 0, n_gchains = 0;   // epoch chains walked by the frontier / list walk
  int64_t n_longest = 0;                  // tasks of the longest epoch chain (sum over epochs)
  int64_t n_fastpro = 0;                  // frontier chains that took the fast prologue (bit 8 of their word)
  int zwalk = 1;                          // zero-cost frontier walk of epoch chains
  int of_tasks = ORDERED_FRONTIER_TASKS;  // ordered frontier tasks per attempt (PVT_OF_TASKS)
  Buf fwin;                               // host-sharded frontier walks: merged windows
  int band_min = BAND_MIN_HOSTS;          // vbp best-fit band lists from this many hosts (0: off)
  int lwalk = 1;                          // vbp best-fit windows: the one-wave list walk
  // tuning / A-B knobs, read from the environment once, at pvt_ctx_create (never per round):
  int t_segments = 0;             // PVT_SEGMENTS: score-pass host segments (0: by policy)
  int t_band_segs = 0;            // PVT_BAND_SEGS: vbp best-fit band list segments (0: default)
  int t_keyed_scan = -1;          // PVT_KEYED_SCAN: keyed first-fit scan on / off (-1: keyed_scan)
  int t_of_hosts = 0;             // PVT_OF_HOSTS: ordered frontier host span (0: default)
  int t_epoch_plan = 1;           // PVT_EPOCH_PLAN: 0 = epoch chains by distinct zone only
  int t_zpre = 1;                 // PVT_ZPRE: 0 = every frontier walk builds its own window
  int t_chain_tab = 1;            // PVT_CHAIN_TAB: 0 = chain tables uploaded before the walk
  int t_epoch_tail = 1;           // PVT_EPOCH_TAIL: 0 = every frontier-walked epoch runs the tail kernels
  int t_chain_cert = 1;           // PVT_CHAIN_CERT: 0 = every frontier walk scans its chain's demand rows
  int t_zw_runrem = 1;            // PVT_ZW_RUNREM: 0 = the walk finds its runs itself, 64 tasks at the most
  int t_zw_wide = 1;              // PVT_ZW_WIDE: 0 = rounds of more than ZMAX zones plan no epoch and no frontier walk
  int t_merge_bitonic = 0;        // PVT_MERGE_SMALL=0: the bitonic merge always
  int res_waves = 4;              // PVT_RES_WAVES: waves per resident round (1, 2, 4 or 8)
  // the last resident launch (pvt_last_resident_shape): its plan's waves, hosts per lane, wide
  // kernel, and its switches as resident_switches_word writes them; zeros before the first one
  int rs_waves = 0, rs_hpl = 0, rs_wide = 0;
  uint32_t rs_switches = 0;
  int rwalk = 9;                  // PVT_RWALK: the raw word (resident_switches, pvt_kernels.h, decodes it)
  int fused = 1;                  // PVT_FUSED=0: host batches staged in six launches (A/B)
  Buf bkey, bidx, bsa, bstb, btouch, btlist, btcnt, bsorttmp;   // band lists: sorted snapshot
  Buf brec;                       // band lists: the snapshot's host records (BandRec)
  Buf bpos, bptouch;              // band lists: host -> sorted position, touched by position
  Buf brun, brdem;                // band lists: the round's runs of equal demands (ids, demands)
  Buf ep_dev, wres;               // epoch tables / status / flags, per-task commit logs
  Buf hmin;                       // frontier walk: per-dimension host minima (partials)
  Buf cmax;                       // frontier-walked epochs: chains' largest demands
  Buf zwin;                       // the first epoch's zero-cost windows (ZoneWindows)
  Buf zundo;                      // frontier walks' optimistic apply: per chain, what undoes it (ZwUndo)
  Buf gcert;                      // the grouped order's group certificates (GroupCert per group)
  Buf run_rem;                    //   and its run lengths (GatherOut.run_rem, int32 per gathered task)
  Buf zpairs, zcomp;              // rounds of more than ZMAX zones: the sum table's zero pairs
                                  //   (launch_zero_pairs), zone -> component root (ZwalkArgs.zcomp)
  std::vector<int32_t> zpairs_host;
  int32_t* ep_host = nullptr;     // pinned staging of ep_dev
  int32_t* ep_hdev = nullptr;     // ep_host's device address (the accept kernel's readback)
  pvt_round* rstage = nullptr;    // pvt_place_batch: descriptors staged for the device (pinned)
  size_t rstage_cap = 0;
  hipEvent_t ev_rstage = nullptr;  //   recorded after their upload (and the MT states')
  bool rstage_busy = false;
  uint32_t* rmt_host = nullptr;   //   and the rounds' MT19937 states (pinned)
  size_t rmt_cap = 0;
  RoundState rs;
  int32_t* next_host = nullptr;   // pinned
  int32_t* flag_host = nullptr;   // pinned word the grouped order's count kernel stores to
  int32_t* flag_hdev = nullptr;   //   (its device address)
  int32_t flag_seq = 0;
  int32_t walk_seq = 0;           // the one-wave list walk's report in flag_host[4..6]
  void* gstage = nullptr;         // grouped order: counts, anchors, cost table (pinned)
  size_t gstage_cap = 0;
  uint64_t* stamps = nullptr;     // PVT_STAMPS builds: device per-phase cycle sums
  void* hst = nullptr;            // pvt_place_host: pinned staging of a host-memory round
  void* hst_map = nullptr;        //   (its device address: the copy kernels' side)
  size_t hst_cap = 0;
  Buf hdev;                       //   and its device copy
  // the zone tables of the last host-array round (cost then bw, Z x Z each) kept on the device:
  // drop-in rounds of one cluster pass the same tables every time, so they are not staged again
  std::vector<double> zt_host;
  Buf zt_dev;
  int zt_Z = 0;
  // content checks (pvt_check_round, pvt_set_checks): off by default
  int checks = 0;
  int n_cus = 0;                  // the grid of the check kernel is sized from the CU count
  std::vector<CheckRound> chk_host;          // the rounds as the check reads them (uploaded)
  Buf chk_desc, chk_slots, chk_rep, chk_owner;
  // pvt_host_ops_apply: (host, k) keys and op indices, in and sorted out, the sort's temp, flag
  Buf ho_key, ho_idx, ho_tmp, ho_flag;
  // pvt_host_meter_finish: the two logs' keys and indices (in, sorted out), heads and rows
  Buf hm_key, hm_idx;
  // pvt_rt_rows: the listed routes' realtime bandwidths, the three verdict words
  Buf rt_val, rt_flag;
};

// A round of more than ZMAX zones takes the group epochs and the frontier walks (the wide
// instances, pvt_zwalk_wide.hip) when it is unsharded and has no realtime bandwidth; PVT_ZW_WIDE=0
// keeps every such round on the list path.
// A wide round whose zero-cost hosts run out gains nothing from epochs: every chain stops, and
// each missed epoch scores a short list window with the wide score pass, whose cost hardly
// depends on the window's length (measured, DESIGN.md §2.6: 5.7x slower than the pipelined
// windows at 512 zones). So after WIDE_MISS_MAX frontier-walked epochs that left a chain unproven
// (first-fit: that accepted no group) the rest of the round takes the pipelined list windows.
static constexpr int WIDE_MISS_MAX = 2;
static inline bool wide_fast(const pvt_ctx* ctx) {
  const RoundState& R = ctx->rs;
  return ctx->t_zw_wide && !R.sharded && R.world <= 1 && !R.r.rt_bw;
}

// Functions shared between the driver files: hidden, so the library exports the C ABI only.
#pragma GCC visibility push(hidden)
namespace pvt {
// pvt_capi.hip (ahead of the macros and the scope that call them)
int fail(pvt_ctx* c, int code, const char* fmt, ...);
int ensure(pvt_ctx* ctx, Buf& b, size_t bytes);
hipEvent_t take_event(pvt_ctx* ctx);
}
#pragma GCC visibility pop

#define HIPCHK(expr)                                                                     \
  do {                                                                                   \
    hipError_t e_ = (expr);                                                              \
    if (e_ != hipSuccess)                                                                \
      return fail(ctx, PVT_EHIP, "%s failed: %s", #expr, hipGetErrorString(e_));         \
  } while (0)

#define ENSURE(b, bytes)                              \
  do {                                                \
    int rc_ = ensure(ctx, (b), (bytes));              \
    if (rc_) return rc_;                              \
  } while (0)

template <class T>
static T* P(Buf& b) { return reinterpret_cast<T*>(b.p); }

// A profiling scope. profiling 1: events recorded around the scope's launches. profiling 2 (one
// named kernel): the events are bound to that kernel's dispatch by PVT_LAUNCH (pvt_kernels.h),
// with no marker packets in the stream; PVT_BIND_EVENTS=0 records them around it instead.
struct Scope {
  pvt_ctx* ctx;
  hipStream_t st;
  TimedLaunch t;
  bool bound = false;
  Scope(pvt_ctx* c, int kclass, double cand, double bytes, hipStream_t s = nullptr,
        const char* kname = nullptr)
      : ctx(c), st(s ? s : c->stream) {
    t.kclass = kclass; t.kname = kname; t.candidates = cand; t.bytes = bytes; t.a = t.b = nullptr;
    if (!on()) return;
    t.a = take_event(ctx);
    if (ctx->profiling == 2 && ctx->bind_events && !g_timed.armed) {
      t.b = take_event(ctx);
      g_timed.a = t.a; g_timed.b = t.b; g_timed.armed = true; g_timed.used = g_timed.extra = 0;
      bound = true;
    } else {
      (void)hipEventRecord(t.a, st);
    }
  }
  bool on() const {
    return ctx->profiling == 1 ||
           (ctx->profiling == 2 && t.kname && (ctx->prof_only.empty() || ctx->prof_only == t.kname));
  }
  ~Scope() {
    if (!on()) return;
    if (bound) {
      const bool ok = g_timed.used == 1 && g_timed.extra == 0;
      g_timed = TimedEvents{};
      if (ok) {
        ctx->pending.push_back(t);
      } else {                        // no launch, or more than the one the events bound to
        ctx->evpool.push_back(t.a);
        ctx->evpool.push_back(t.b);
        ctx->n_unbound++;
      }
      return;
    }
    t.b = take_event(ctx);
    (void)hipEventRecord(t.b, st);
    ctx->pending.push_back(t);
  }
};

#pragma GCC visibility push(hidden)
namespace pvt {
// pvt_capi.hip
int check_round(pvt_ctx* ctx, const pvt_round* r);
int gate_checks(pvt_ctx* ctx, const pvt_round* rounds, int n, bool host_mt, bool batch);
int fail_check(pvt_ctx* ctx, int i, const pvt_check_report& p);
void check_host_arrays(const pvt_round* r, pvt_check_report* p);
// pvt_round.hip
double bytes_per_candidate(int mode);
void lists_from(pvt_ctx* ctx, Lists& L, int b = 0);
void flush_touched(pvt_ctx* ctx);
int round_begin(pvt_ctx* ctx, const pvt_round* rin, int lo, int hi, int world);
int group_end(const RoundState& R, int t0);
CommitArgs commit_args(pvt_ctx* ctx, int t0, int nt, int lb, int n_prev, int32_t* status);
ZwalkArgs zwalk_chain_args(pvt_ctx* ctx, int t0);
ZwalkArgs zwalk_keyed_args(pvt_ctx* ctx, int t0, int n);
EpochArgs epoch_args(pvt_ctx* ctx, int t0, int nt, int nseg);
int compact_flags(pvt_ctx* ctx, int n, hipStream_t st);
int frontier_walked(pvt_ctx* ctx, const char* what, int done, int n);
int ordered_verdict(pvt_ctx* ctx, const char* what, int done, int n, int hs, bool* again);
int round_next_window(pvt_ctx* ctx, int* nt_out);
int window_lists(pvt_ctx* ctx, int t0, int nt, int lb, hipStream_t st);
int walk_launch(pvt_ctx* ctx, int t0, int nt, int lb, int n_prev);
void adapt_window(pvt_ctx* ctx, int adv, int nt);
int walk_status(pvt_ctx* ctx, int t0, int nt, bool inherited, int* adv);
int place_windowed(pvt_ctx* ctx, const pvt_round* r);
// pvt_round_epochs.hip
int zero_cost_components(pvt_ctx* ctx);
int epoch_groups(pvt_ctx* ctx);
void epoch_plan(const RoundState& R, int t0, EpochPlan& P, bool whole = false);
int upload_chain_tables(pvt_ctx* ctx, const EpochPlan& E);
void epoch_tail(pvt_ctx* ctx, const EpochArgs& ea, bool validate, int accept_nch);
int ff_epoch(pvt_ctx* ctx, int* adv_out);
int epoch_frontier_verdict(pvt_ctx* ctx, const EpochPlan& E, int t0, int* need_out, int* adv_out);
int place_epochs(pvt_ctx* ctx);
// pvt_resident.hip
bool resident_fits(const pvt_round* r, int max_hosts);
int place_resident(pvt_ctx* ctx, const pvt_round* rounds, int n,
                   const void* desc_dev = nullptr, uint32_t* mt_dev = nullptr);
}
#pragma GCC visibility pop
