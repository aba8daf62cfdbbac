// pvt_kernels.h — device data layout and kernel launch interface of the placement engine.
//
// Layout in HBM (all fp64 math is IEEE, no contraction):
//   hosts   avail[4][H] SoA fp64 (cpus, mem, disk, gpus), zone[H] i32, tiebreak[H] u32
//   tasks   processing order ord[T] i32; dem_ord[T][4] fp64 task-major (one 32-B row per
//           task, so a wave reads a task's demand with one scalar load); anc_ord[T] i32
//   zones   csum[Z][Z] = cost[a][z] + cost[z][a], bsum[Z][Z] = bw[a][z] + bw[z][a]
//   lists   per window task: KL candidates, sorted by (score, tiebreak, host) ascending
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

#include "pvt_cert.h"

namespace pvt {

// Timed launches (pvt_set_profiling 2: HIP events around one named kernel). Every launch helper
// starts its kernel through PVT_LAUNCH. When the profiling scope (pvt_driver.h Scope) has armed a
// pair of events, the first launch binds them to the kernel's own dispatch
// (hipExtLaunchKernelGGL: the events take the dispatch's start and end timestamps), so the timed
// kernel costs the stream no marker packets. A recorded event pair around a launch left ~5 us of
// idle GPU on each side of it (config-5 kernel trace: 7.7 us before the frontier walk, 5.0 after).
// `extra` counts launches past the first while armed (a scope that would time only part of its
// work; the scope then drops the sample).
struct TimedEvents {
  hipEvent_t a = nullptr, b = nullptr;
  bool armed = false;
  int used = 0, extra = 0;
};
extern thread_local TimedEvents g_timed;
#define PVT_LAUNCH(kernel, grid, block, shmem, stream, ...)                                         \
  do {                                                                                             \
    ::pvt::TimedEvents& te_ = ::pvt::g_timed;                                                      \
    if (te_.armed && te_.a) {                                                                      \
      hipExtLaunchKernelGGL(kernel, grid, block, shmem, stream, te_.a, te_.b, 0u, __VA_ARGS__);    \
      te_.a = nullptr;                                                                             \
      te_.used++;                                                                                  \
    } else {                                                                                       \
      if (te_.armed) te_.extra++;                                                                  \
      hipLaunchKernelGGL(kernel, grid, block, shmem, stream, __VA_ARGS__);                         \
    }                                                                                              \
  } while (0)

constexpr int WAVE = 64;
constexpr int KL = 64;           // candidate list length per task (one entry per lane)
constexpr int ZMAX = 32;         // zones of the fast paths: zone tables in LDS, 32-bit zone masks
                                 //   (frontier walks, epochs, resident walks; locality.yml has 31)
constexpr int ZWIDE = 512;       // zones of a round (PVT_MAX_ZONES): above ZMAX the wide kernels
                                 //   read the sum tables from global memory
constexpr int TW = 4;            // tasks per wave in the score kernel
constexpr int WPB = 4;           // waves per score-kernel block
constexpr int MAX_WINDOW = 1024; // tasks per window (bounded by the commit kernel's LDS)
constexpr int HASH_BITS = 12;    // commit kernel touched-host hash: 4096 slots
constexpr int MAX_SEG = 16;      // host segments per task at a full window
constexpr int CHAIN_MAX = 2048;  // tasks per epoch chain walk (touched-host hash: 4096 slots)

enum Mode { CA_FF = 0, CA_BF = 1, OPP = 2, VBP_FF = 3, VBP_BF = 4 };

struct SegEntry {    // 16 B: one candidate in a per-segment list
  double s;
  uint32_t tb;
  int32_t id;
};

// One candidate of a merged list: 64 B, so lane j of the commit walk reads entry j with
// four 16-B loads.
struct ListEntry {
  double s;           // score (sort key)
  uint32_t tb;        // tiebreak (host-id rank for vbp best-fit, else 0)
  int32_t id;         // host index
  int32_t zone;
  int32_t pad;
  double a[4];        // snapshot availability of the host
  double pad2;
};
// Per window task (64 B, read by lanes 0-15 of the commit walk with one vector load).
struct TaskRec {
  double d[4];
  int32_t cnt;        // valid entries (<= LMAX)
  int32_t complete;   // 1 if every snapshot-feasible host is in the list
  int32_t anc;
  int32_t ord;        // caller index of the task (where its placement is written)
  double bs;          // bound: every snapshot-feasible host NOT in the list has
  uint32_t btb;       //   (score, tiebreak, host) >= (bs, btb, bid)
  int32_t bid;
};
// Merged (final) candidate lists of one window: the exact top-cnt hosts of each task, up to
// LMAX of them (the union of the segment lists is exact below the smallest last entry of an
// incomplete segment list).
constexpr int LMAX = 1024;
struct Lists {
  ListEntry* e;       // [W][LMAX]
  int32_t* ids;       // [W][LMAX] host index of each entry (compact copy for deep searches)
  TaskRec* t;         // [W]
};

struct ScoreArgs {
  const double* avail;
  const int32_t* zone;
  const uint32_t* tb;
  const double* key;      // CA_FF: frozen per-group host key
  const double* dem;      // window tasks [nt][4]
  const int32_t* anc;     // window tasks [nt]
  const double* csum;
  const double* bsum;
  int H, Z, nt, S;        // S host segments: segment s = 64-host blocks s, s + S, ...
  int h_lo, h_hi;         // host range scored (a rank's shard; [0, H) unsharded)
  SegEntry* seg;          // [nt][S][KL]
  int32_t* seg_feas;      // [nt][S]
  int tw;                 // tasks per wave: 0 = the policy's default, else 2 or 4 (tuning/tests)
  const double* rtb;      // CA_BF realtime_bw: bandwidth per (group, host) [G][H], or NULL
  const int32_t* grp;     // window tasks' groups [nt] (rows of rtb)
};

// Merge of S sorted candidate lists per task into the task's exact top list. Two sources:
//   score segments   seg[(task*S + g)*KL + e], SL = KL, seg_feas[task*S + g] = feasible hosts
//                    of the segment (a list with more than KL of them is bounded by entry KL-1)
//   rank packages    (host-dimension sharding) seg[(g*nt + task)*(SL+1) + e]: SL entries then
//                    an explicit bound entry (id 0x7fffffff: the rank's list is complete);
//                    seg_feas = NULL
struct MergeArgs {
  const SegEntry* seg;
  const int32_t* seg_feas;
  const double* avail;
  const int32_t* zone;
  const double* dem;      // window tasks [nt][4]
  const int32_t* anc;     // window tasks [nt]
  const int32_t* ord;     // window tasks' caller indices
  int H, nt, S;
  int SL;                 // entries per source list (KL, or the package depth)
  Lists L;
  const int32_t* nt_dev;  // or NULL: only tasks [0, *nt_dev) (vbp best-fit representative lists)
  int bitonic;            // 1: the bitonic merge_kernel always (A/B; PVT_MERGE_SMALL=0 at ctx create)
};

// Host-dimension sharding: a rank's exact local lists -> its exchange package (see MergeArgs).
struct PackArgs {
  Lists L;                // local merged lists of the window
  int nt, PK;
  int ordered;            // index-order first-fit lists (score 0, bound = last id + 1)
  SegEntry* out;          // [nt][PK + 1]
};

struct OrderedArgs {      // first-fit by host index: first KL snapshot-feasible hosts
  const double* avail;
  const int32_t* zone;
  const double* dem;
  const int32_t* anc;
  const int32_t* ord;
  int H, nt, strict;
  int h_lo, h_hi;         // host range scanned
  Lists L;
};

// One walked task of an epoch walk (chain mode): its winner's key (score, host; id -1 = no
// host) and the host's capacities after the commit; sup = 1 once a later task of the same
// group segment committed to the same host (the entry is then not the segment's final state).
struct WinRec {
  double s;
  int32_t id;
  int32_t sup;
  double a[4];
};

struct CommitArgs {
  double* avail;          // global state, updated in place
  const double* dem;      // window tasks [nt][4] (for the window's minimum demand)
  const double* csum;
  const double* bsum;
  const int32_t* zone;    // host zones / tiebreak ranks (for inherited touched hosts)
  const uint32_t* tb;     //   tb may be NULL (rank 0 for every host)
  Lists L;
  int H, Z, nt, mode;
  int32_t* placement;     // [T] in caller order
  // Hosts committed to by the previous window whose list entries in THIS window are stale
  // (the lists were scored before that window's commits landed): treated as touched.
  const int32_t* prev_ids;
  int n_prev;
  int32_t* own_ids;       // out: hosts this walk committed to (distinct), for the next window
  int32_t* status;        // out: [0] window-local index where the walk stopped (nt = done,
                          //      -1 = spin timeout), [1] number of own_ids
  const double* rtb;      // CA_BF realtime_bw: bandwidth per (group, host) [G][H], or NULL
  const int32_t* grp;     // window tasks' groups [nt] (rows of rtb)
  uint64_t* stamps;       // diagnostic builds only (PVT_STAMPS): per-phase cycle sums
  // Speculative epochs (pvt_round_epochs.hip place_epochs), chain mode when cmap is set: workgroup b
  // walks the window tasks cmap[coff[b] .. coff[b+1]) (processing order), a chain of group
  // segments whose chain-local starts are cseg[csoff[b] .. csoff[b+1]); it writes wlog[w] for
  // every walked window task w instead of avail, and status[2b] = tasks walked.
  const int32_t* coff;
  const int32_t* cmap;
  const int32_t* csoff;
  const int32_t* cseg;
  WinRec* wlog;
  int skip_done;          // chain mode: a chain whose status already says "all walked" is skipped
  // vbp best-fit representative lists (pvt_band.hip band_runs_kernel): window task w's list is row
  // rowmap[w], its caller index ordw[w] (the list rows' TaskRec.ord belong to other tasks);
  // NULL: row w, TaskRec.ord
  const int32_t* rowmap;  //   (row = rowmap[w] - rowbase: the round's run ids, band_runs_kernel)
  const int32_t* ordw;
  int rowbase;
  // or NULL: mapped pinned words the walk also reports to -- [1] = status[0], [2] = status[1],
  // then [0] = hseq (system-scope release): the host polls them instead of a copy + sync
  int32_t* hflag;
  int32_t hseq;
};

// Speculative epochs, cost_aware best-fit. The epoch's group segments (processing order,
// contiguous window ranges seg_off) are walked in chains -- the segments whose anchors share a
// zero-cost zone component, in order, by one workgroup -- all chains side by side on the epoch's
// start state. Segment j is exact iff every earlier segment is exact and complete, and for
// every task t it walked and every final log entry (host h, capacities after that segment) of
// an earlier segment of ANOTHER chain: h is not t's winner and h does not fit t with a key
// (score, index) below the winner's.
struct EpochArgs {
  const double* dem;      // window tasks [nt][4]
  const int32_t* anc;     // window tasks [nt]
  const double* csum;
  const double* bsum;
  const int32_t* zone;
  const int32_t* seg_off; // [nseg + 1] window offsets of the segments (processing order)
  const int32_t* seg_chain;   // [nseg] chain of each segment
  const int32_t* seg_cstart;  // [nseg] index of the segment's first task in its chain's walk
  const int32_t* status;  // [nchains][2]: tasks the chain's walk got through (-1: timeout)
  WinRec* wlog;           // [nt] (sup set by the finality pass)
  double* avail;          // apply: accepted segments' final entries written here
  int H, Z, nt, nseg;
  int32_t* bad;           // [nseg] out: 1 = segment j is not exact (zeroed by the caller)
  const double* rtb;      // realtime_bw: bandwidth per (group, host) [G][H], or NULL
  const int32_t* grp;     // window tasks' groups [nt]
  int whole;              // accept: whole segments only (first-fit zero-key epochs)
  // frontier-walked epochs (cost_aware best-fit): when every chain was walked to its end by the
  // zero-cost frontier walk and every final log entry exceeds the epoch's largest demand by
  // 2^-287 in some dimension (safe[j], set by the finality pass from the chains' cmax), no pair
  // can beat a winner (hosts of different components, scores > 0) and validation is skipped
  const double* cmax;     // [nch][4] or NULL
  const int32_t* coff;    // [nch + 1] chains' task ranges (their lengths)
  int nch;
  int32_t* safe;          // [nseg]
};
// pair validation (after launch_epoch_final, which zeroes the verdicts it sets)
void launch_epoch_validate(const EpochArgs& a, hipStream_t st);
// finality (alone: first-fit zero-key epochs need no pair validation)
void launch_epoch_final(const EpochArgs& a, hipStream_t st);
// apply: the accepted segments [0, n_accept) of each chain, chain by chain in segment order
void launch_epoch_apply(const EpochArgs& a, int n_accept, int nchains, hipStream_t st);
// validate's verdict to the accepted prefix and its apply, on the device; res[5] reported, and
// (hout: mapped pinned memory) the nwords readback words from a.status copied there
void launch_epoch_accept_apply(const EpochArgs& a, int32_t* res, int nchains, hipStream_t st,
                               int32_t* hout = nullptr, int nwords = 0);
// a missed optimistic apply of the frontier walk (ZwalkArgs.undo): the chains of `chains` (bit c:
// chain c wrote its window back) get their windows' epoch-start rows again
// (chains of `fast` took the fast prologue: their start rows are those of the prebuilt window
// zpre->w[win.w[c]], which nothing modifies before the verdict)
struct UndoWin { uint8_t w[64]; };
void launch_epoch_undo(const struct ZwUndo* undo, uint64_t chains, int nchains, double* avail, int H,
                       hipStream_t st, uint64_t fast = 0, const struct ZoneWindows* zpre = nullptr,
                       const UndoWin* win = nullptr);
void launch_commit_chains(const CommitArgs& a, int nchains, hipStream_t st);
// vbp best-fit windows: the one-wave list walk with list cursors (pvt_lwalk.hip); CommitArgs as
// for launch_commit (no epochs, no stamps). status[0] < nt: refill there (0: the list walk decides)
void launch_lwalk(const CommitArgs& a, hipStream_t st);
hipError_t lwalk_init_attrs();

// Zero-cost frontier walk of epoch chains (pvt_zwalk.hip): workgroup b walks chain b like the
// list walk's chain mode (same tables, WinRec log, status[2b] = tasks walked) while it can prove
// every winner is the lowest-index fitting zero-cost host of its window; otherwise it writes
// status[2b] = -2 and leaves the chain to the list walk (CommitArgs.skip_done).
// An epoch's chain tables passed BY VALUE in the frontier walk's kernel arguments (instead of an
// upload launch before the walk: ~4 us of kernel plus its dispatch gap on the default line).
// Segment k (one group's tasks in the epoch, processing order): epoch tasks [seg_off[k],
// seg_off[k + 1]), walked by chain seg_chain[k] from chain-local position seg_cstart[k]. Chain c:
// chain-local positions [0, coff[c + 1] - coff[c]), its segments csegid[csoff[c] .. csoff[c+1]) in
// order. The walk's block 0 writes seg_off / seg_chain / seg_cstart / coff to the out pointers for
// the epoch kernels after it. nch = 0: the tables come from the device arrays (ZwalkArgs.coff ...).
constexpr int CT_SEGS = 64;
struct ChainTab {
  int32_t nseg, nch;
  int32_t seg_off[CT_SEGS + 1];
  int32_t seg_chain[CT_SEGS];
  int32_t seg_cstart[CT_SEGS];
  int32_t coff[CT_SEGS + 1];
  int32_t csoff[CT_SEGS + 1];
  int32_t csegid[CT_SEGS];
  int32_t* o_seg_off;
  int32_t* o_seg_chain;
  int32_t* o_seg_cstart;
  int32_t* o_coff;
};
// Group certificates (written by group_sort_gather_kernel's group blocks, one record per group)
// and what the host knows of an epoch's chains, by value: together they replace the frontier
// walk's pass over the chain's demand rows and anchors (the fast prologue, pvt_zwalk.hip). A
// record's sub-batch j covers the group's sorted tasks [64 j, 64 j + 64).
constexpr int GC_SUB = 4096 / 64;          // (GSORT_MAX / 64, asserted below)
struct GroupCert {
  double mx[4], mn[4];    // per-dimension extremes of the group's demands
  int32_t bad;            // 1: some |d| is not <= 2^500 (NaN included); 2: no record (n > GSORT_MAX)
  int32_t n;              // tasks
  int32_t pad[2];
  double smin[GC_SUB][4]; // per-dimension minima of each sub-batch
};
// fast = 1: every segment of the epoch is a whole group with a record and an anchor in [0, Z),
// the epoch is the round's first (ZwalkArgs.zpre) and every chain has at most ZW_ENT (segment,
// sub-batch) entries. Segment k: its group's record rec[seg_grp[k]], its first entry's index
// seg_ent[k] among its chain's entries (chain order). Chain c: its zone set cu[c] (the union of
// its anchors' zero-cost zones, from the cost table as the device computes it), the prebuilt
// window cwin[c] of its component (ZoneWindows: the component's lowest zone) and its entry
// count cent[c].
constexpr int ZW_ENT = 64;
struct ChainCert {
  int32_t fast;
  const GroupCert* rec;
  uint32_t cu[CT_SEGS];
  uint8_t seg_grp[CT_SEGS];
  uint8_t seg_ent[CT_SEGS];
  uint8_t cwin[CT_SEGS];
  uint8_t cent[CT_SEGS];
};
struct ZwalkArgs {
  const double* avail;    // epoch-start capacities [4][H]
  const int32_t* zone;
  int H, Z;
  const double* dem;      // window tasks [nt][4]
  const int32_t* anc;     // window tasks' anchors
  const int32_t* ord;     // window task -> caller index (placement)
  // window tasks' run lengths (GatherOut.run_rem), or NULL: the fast prologue's instance takes a
  // run's length from it, min(run_rem, ZW_RMAX), instead of comparing the batch's demand rows;
  // set only where the order came from this round's grouped-order launch (chain_cert)
  const int32_t* run_rem;
  const double* csum;
  const double* bsum;
  const int32_t* coff;
  const int32_t* cmap;
  int32_t* status;
  WinRec* wlog;
  int32_t* placement;
  const double* hmin;     // per-dimension host minima, launch_host_min partials
  uint64_t* stamps;       // diagnostic builds only (PVT_STAMPS)
  // keyed first-fit mode (launch_zwalk_keyed): one group of knt tasks, window = the first hosts
  // of the zero-key prefix kperm[0, kn) (+ lo), capacities written back to wb at the end
  const int32_t* kperm;
  int kn, lo, knt;
  double* wb;
  const int32_t* kn_dev;  // keyed: prefix length read on the device (NULL: kn)
  // host-sharded rounds: the merged window of chain b (keyed / ordered: of the walk) -- hosts
  // in index order with their capacities, as the unsharded walk builds it -- or NULL (build it)
  const struct FrontierSlot* pwin;
  // chain mode: chain b's group segments start at chain-local positions cseg[csoff[b] ..
  // csoff[b+1]) (a run of equal demands never crosses one: finality and apply work per
  // segment, so every segment's last copy on a host must be logged); NULL in keyed mode
  const int32_t* csoff;
  const int32_t* cseg;
  double* cmax;           // chain mode: [chains][4] out, each chain's largest demand per dimension
  // chain mode, the round's first epoch: windows the grouped order's launch built from the
  // snapshot (a chain uses the one whose zone set covers its anchors' zero-cost zones), or NULL
  const struct ZoneWindows* zpre;
  // chain mode, optimistic apply (the driver's epoch tail), or NULL: a chain that
  // walked all its tasks writes its window's capacities to wb (the round's avail) itself; every
  // chain first saves its window's hosts and start capacities in undo[b], and reports status[0],
  // status[1] also to hstat[2b], hstat[2b + 1] and its certificate word to hcert[b] (both mapped
  // pinned; bit fields: pvt_cert.h): the dimensions no task of the chain demands, the dimensions
  // whose host minimum is at least CERT_MARGIN (best-fit; first-fit reports 0), and ZW_CERT_FAST:
  // the chain took the fast prologue, it saved nothing in undo[b], its start rows are the
  // prebuilt window's (cert.cwin[b]). hcert alone may be set (cert.fast without undo).
  struct ZwUndo* undo;
  int32_t* hstat;
  int32_t* hcert;
  ChainTab tab;           // chain mode: the epoch's chain tables by value (tab.nch > 0), or none
  ChainCert cert;         // chain mode: cert.fast = the fast prologue (launch_zwalk), or none
  // chain mode, rounds of more than ZMAX zones (launch_zwalk_wide): zone -> the root of its
  // zero-cost component [Z] (the driver's zero_cost_components), else NULL
  const int32_t* zcomp;
};
constexpr int ZW_MIN_PARTS = 256;
// per-dimension minima of avail over hosts [lo, hi) into part[ZW_MIN_PARTS][4]
void launch_host_min(const double* avail, int H, int lo, int hi, double* part, hipStream_t st);
void launch_zwalk(const ZwalkArgs& a, int nchains, hipStream_t st);
// the same walk over a window of ZW_MBIG hosts (status[1] == 2: a chain's window of ZW_M was
// exhausted while more of its zones' hosts exist -- config 5 with loaded hosts)
void launch_zwalk_big(const ZwalkArgs& a, int nchains, hipStream_t st);
// cost_aware first-fit with sort_hosts: the zero-key chain walk (FF mode; hmin = the
// launch_host_absmax partials)
void launch_zwalk_ff(const ZwalkArgs& a, int nchains, hipStream_t st);
// Rounds of more than ZMAX zones (pvt_zwalk_wide.hip; a.zcomp set): the same chain walks on the
// zones of the chain's zero-cost component, renumbered 0..k-1 in ascending zone id (k <= ZMAX;
// a chain of a larger component reports (0, 1): the list walk takes it). big: the ZW_MBIG window.
void launch_zwalk_wide(const ZwalkArgs& a, int nchains, bool big, hipStream_t st);
void launch_zwalk_ff_wide(const ZwalkArgs& a, int nchains, hipStream_t st);
// The zone pairs a < z with csum[a][z] == 0.0 of a Z x Z sum table, as words a << 16 | z in
// pairs[1 ..] in any order, their count in pairs[0] (zeroed here; pairs past cap are counted and
// not stored).
constexpr int ZP_MAX = 8191;
void launch_zero_pairs(const double* csum, int Z, int32_t* pairs, int cap, hipStream_t st);
void launch_host_absmax(const double* avail, int H, int lo, int hi, double* part, hipStream_t st);
constexpr int ZW_M = 1024;                 // frontier-walk window hosts
constexpr int ZW_MBIG = 3072;              // the large window (a retry for chains that outgrow ZW_M)
// What undoes a chain's optimistic apply: its window's hosts and their epoch-start capacities.
struct ZwUndo {
  int32_t count, pad[3];
  int32_t id[ZW_MBIG];
  double a[4][ZW_MBIG];
};
void launch_zwalk_keyed(const ZwalkArgs& a, bool strict, hipStream_t st);
// ordered first-fit frontier: flags[h - lo] = host h in [lo, hs) fits the smallest demand of
// tasks dem[0, n)
void launch_alive_flags(const double* avail, int H, int lo, int hs, const double* dem, int n,
                        int strict, double* dmin, uint8_t* flags, hipStream_t st);

// Host-sharded frontier walks (pvt_shard.hip pvt_shard_*). A rank's package carries, per chain
// (cost_aware best-fit epochs) or for the one keyed / ordered walk, the first ZW_M window hosts
// of ITS host range in index order with their capacities, plus its host minima (certificate 2).
// After the all-gather every rank merges the packages -- ranks own ascending contiguous ranges,
// so the concatenation in rank order truncated to ZW_M is the window the unsharded walk builds
// -- and runs the same walk on identical inputs.
struct FrontierSlot {
  int32_t n;              // window hosts listed (<= ZW_M)
  int32_t total;          // candidates counted in the range (ordered walk: alive hosts)
  int32_t pad[2];
  int32_t id[ZW_M];       // global host index, ascending
  double a[4][ZW_M];      // capacities
};
// Zero-cost windows prebuilt by the grouped order's launch (group_sort_gather_kernel) for the
// round's first epoch of cost_aware best-fit: for each zone j that is the lowest zone of its
// zero-cost component (zones joined by csum = 0), U[j] = the union of the zero-cost zones of the
// round's group anchors in that component, and w[j] the first ZW_M hosts of U[j] in index order
// with their zones and snapshot capacities (bad: some capacity is not finite with |x| <= 2^500,
// certificate 3). U[j] = 0: no window for j. A chain's U (its anchors' zero-cost zones) lies in
// one component, so it is covered by that component's U[j]; a window over a superset of the
// zones is exact for the walk (pvt_zwalk.hip certificates).
struct ZoneWindow {
  int32_t n, bad, pad[2];
  int32_t id[ZW_M];
  int32_t z[ZW_M];
  double a[4][ZW_M];
};
struct ZoneWindows {
  uint32_t U[ZMAX];
  ZoneWindow w[ZMAX];
};
struct FrontierHdr {
  int32_t kind, nslots, pad[14];
  double hmin[ZW_MIN_PARTS][4];   // host-minimum partials over the rank's range
};
struct ZwinArgs {         // window candidates of one rank, per epoch chain
  const double* avail;
  const int32_t* zone;
  int H, Z, lo, hi;
  const double* csum;
  const int32_t* anc;     // epoch tasks' anchors
  const int32_t* coff;    // chain c: epoch tasks cmap[coff[c] .. coff[c+1])
  const int32_t* cmap;
  FrontierSlot* out;      // [nchains]
};
void launch_zwin_build(const ZwinArgs& a, int nchains, hipStream_t st);
// keyed / ordered walks: slot from a compacted local host list (host lo + perm[p], p < *count)
void launch_zwin_gather(const double* avail, int H, int lo, const int32_t* perm,
                        const int32_t* count, FrontierSlot* out, hipStream_t st);
// after the all-gather: merged slots [nslots] and host-minimum partials (ZW_MIN_PARTS x 4)
void launch_zwin_merge(const uint8_t* pkgs, int64_t pkg_bytes, int world, int nslots,
                       FrontierSlot* out, double* hmin, hipStream_t st);

// cost_aware first-fit with sort_hosts, as the reference runs it (cost_aware.py:118-124): the
// hosts sorted once per group by the frozen key (perm, skey = sorted key bits; the radix sort
// is stable, so equal keys keep host order), then per task the first `depth` snapshot-feasible
// hosts in that order. Lists come out exactly as merge_kernel would build them: sorted by
// (key, 0, host), cnt, complete, and a bound every unlisted host ranks at or after.
struct PermArgs {
  const double* avail;
  const int32_t* zone;
  const uint64_t* skey;   // [n] sorted key bits
  const int32_t* perm;    // [n] host at each sorted position, minus h_lo
  const double* dem;      // window tasks [nt][4]
  const int32_t* anc;
  const int32_t* ord;
  int H, nt, n, depth;    // depth <= LMAX
  int h_lo;               // first host of the sorted range (a rank's shard; 0 unsharded)
  int partial;            // perm is a prefix of the order: every other host's key >= rest_s
  double rest_s;
  Lists L;
};

struct KeyArgs {          // CA_FF sort_hosts: key[h] = c*df / (||avail_h|| * bw)
  const double* avail;
  const int32_t* zone;
  const int32_t* decay;
  const double* csum;
  const double* bsum;
  int H, Z, anchor;
  int h_lo, h_hi;         // hosts whose key is computed
  double* key;
  const double* rtb;      // realtime_bw: the group's bandwidth row [H], or NULL
};

// vbp best-fit lists by a memory band (pvt_band.hip): hosts [lo, hi) sorted once per round by
// snapshot memory (sorted copy of their snapshot state), plus the hosts committed to since
// (touched: flags[H], list, count), scanned with their live state.
struct BandArgs {
  const uint64_t* key;    // [n] orderable bits of the snapshot avail[1], ascending
  const double* sa;       // [4][n] snapshot capacities in sorted order
  const uint32_t* stb;    // [n] host-id ranks in sorted order
  const int32_t* sid;     // [n] host index at each sorted position
  int n, lo, hi;          // sorted hosts = [lo, hi)
  const uint8_t* touched; // [H] 1: committed to since the snapshot
  const int32_t* tlist;   // touched hosts
  const int32_t* tcount;  // [1]
  const double* avail;    // live state [4][H]
  const uint32_t* tb;     // [H]
  int H;
  const double* dem;      // window tasks [nt][4]
  int nt, S;              // S list segments per task
  SegEntry* seg;          // [nt][S][KL]
  int32_t* seg_feas;      // [nt][S]
  const int32_t* nt_dev;  // or NULL: only tasks [0, *nt_dev) (representative lists)
  const uint8_t* ptouched;  // [n] touched by sorted position (= touched[sid[p]], read with the chunk)
};

// A host's snapshot row for the band sort's gather (one 64-byte line per host).
struct alignas(64) BandRec {
  double a[4];
  uint32_t tb;
  uint32_t pad[7];
};
// sort keys and host records (rec[p] for host lo + p)
void launch_band_keys(const double* avail, const uint32_t* tb, int H, int lo, int n, uint64_t* key,
                      int32_t* idx, BandRec* rec, hipStream_t st);
void launch_band_gather(const BandRec* rec, int lo, int n, const int32_t* sid, double* sa,
                        uint32_t* stb, int32_t* pos, hipStream_t st);
void launch_touch_update(const int32_t* own, const int32_t* status, uint8_t* flags, int32_t* tlist,
                         int32_t* tcount, const int32_t* pos, int lo, int hi, uint8_t* ptouch,
                         hipStream_t st);
void launch_band_score(const BandArgs& a, hipStream_t st);
// Window tasks -> list rows: each run of equal demand vectors (bit for bit) shares one list row;
// rdem = the rows' demands, *nrep = rows (nt <= MAX_WINDOW)
void launch_band_runs(const double* dem, int T, int32_t* run, double* rdem, hipStream_t st);

int score_tasks_per_wave(int mode, int hosts, int force = 0, int zones = 0);
hipError_t score_init_attrs();
int score_diag(uint64_t* out, int n, int reset);   // PVT_DIAG builds; else PVT_EUNSUPPORTED
void launch_score(int mode, const ScoreArgs& a, hipStream_t st);
void launch_merge(const MergeArgs& a, hipStream_t st);
const char* merge_kernel_name(const MergeArgs& a);   // the kernel launch_merge picks
void launch_pack(const PackArgs& a, hipStream_t st);
void launch_ordered(const OrderedArgs& a, hipStream_t st);
void launch_perm_scan(const PermArgs& a, hipStream_t st);
void launch_zero_key_flags(const double* key, int n, uint8_t* flags, hipStream_t st);
void launch_commit(const CommitArgs& a, hipStream_t st);
void launch_key(const KeyArgs& a, hipStream_t st);
void launch_zone_tables(const double* cost, const double* bw, int Z, double* csum, double* bsum,
                        hipStream_t st);
// a2: u64 sort key ~bits(||d||2) per task (descending norm == ascending key)
void launch_norm_keys(const double* dem, int T, const int32_t* idx, uint64_t* keys,
                      hipStream_t st);
void launch_group_keys(const int32_t* task_group, const int32_t* idx, int T, uint32_t* keys,
                       hipStream_t st);
// Resident rounds (pvt_batch.hip): one block per round (1 wave up to 1024 hosts, else 4), hosts
// in registers (HPL hosts per lane, HPL in {1, 2, 4, 8, 16}).
constexpr int RES_THREADS = 256;
constexpr int RES_MAX_HPL = 16;
constexpr int RES_MAX_HOSTS = RES_THREADS * RES_MAX_HPL;   // 4096
constexpr int RES_MAX_TASKS = 4096;
constexpr int RES_MIXED = -1;   // launch_resident: rounds of different policies (4 waves)
constexpr int RW_MAXH = 1024;   // resident walk: hosts held in LDS
// The resident kernel's A/B switches, decoded from the PVT_RWALK word (default 9) by
// resident_switches. One-wave walks (batches whose largest round has at most RW_MAXH hosts):
//   1  cost_aware best-fit rounds start with the one-wave walk (resident_walk)
//   8  first fit by index is walked by one wave (resident_walk_ff)
//   2  the walking wave moves with the workgroup index (2 without 1 also turns the cost_aware
//      walk on; 3 is 1)
//   4  no bulk runs in the walks
// The 4-wave path (every resident size):
//   16 no bulk sticky runs (and so no run lists)
//   32 no run lists
//   64 run lists for every policy but the opportunistic one (default: vbp best-fit only)
//   bits 8-15 the shortest remaining run given a list (0: RES_LIST_MIN)
struct ResidentSwitches {     // (one 32-bit kernel argument; all zero: no walk, no bulk runs, no lists)
  uint32_t walk_ca_bf : 1;    // one-wave walks: cost_aware best-fit,
  uint32_t walk_ff : 1;       //   first fit by index,
  uint32_t walk_rotate : 1;   //   the walking wave rotates with the workgroup,
  uint32_t walk_bulk : 1;     //   bulk runs in the walk
  uint32_t bulk_sticky : 1;   // 4-wave path: bulk sticky runs,
  uint32_t run_lists : 1;     //   run lists,
  uint32_t lists_all : 1;     //   for every policy,
  uint32_t list_min : 8;      //   from this many remaining tasks (0: RES_LIST_MIN)
  constexpr bool walks() const { return walk_ca_bf || walk_ff; }   // the walk's LDS region is laid out
};
constexpr ResidentSwitches resident_switches(int word, int maxH) {
  const unsigned w = (unsigned)word;
  const bool small = maxH <= RW_MAXH;
  ResidentSwitches s{};
  s.walk_ca_bf = small && (w & 3) != 0;
  s.walk_ff = small && (w & 8) != 0;
  s.walk_rotate = s.walks() && (w & 3) == 2;
  s.walk_bulk = s.walks() && (w & 4) == 0;
  s.bulk_sticky = (w & 16) == 0;
  s.run_lists = (w & 32) == 0;
  s.lists_all = (w & 64) != 0;
  s.list_min = w / 256 % 256;   // bits 8-15
  return s;
}
constexpr bool operator==(const ResidentSwitches& a, const ResidentSwitches& b) {
  return a.walk_ca_bf == b.walk_ca_bf && a.walk_ff == b.walk_ff && a.walk_rotate == b.walk_rotate &&
         a.walk_bulk == b.walk_bulk && a.bulk_sticky == b.bulk_sticky && a.run_lists == b.run_lists &&
         a.lists_all == b.lists_all && a.list_min == b.list_min;
}
static_assert(sizeof(ResidentSwitches) == 4, "a plain kernel argument of a few bytes");
static_assert(resident_switches(9, 1024) == ResidentSwitches{1, 1, 0, 1, 1, 1, 0, 0}, "the default");
static_assert(resident_switches(0, 1024) == ResidentSwitches{0, 0, 0, 0, 1, 1, 0, 0} &&
              resident_switches(0, 1025) == resident_switches(0, 1024), "0: no walk, the 4-wave defaults");
static_assert(resident_switches(9, 1025) == resident_switches(0, 1025), "no walk above RW_MAXH hosts");
static_assert(resident_switches(5, 1024) == ResidentSwitches{1, 0, 0, 0, 1, 1, 0, 0} &&
              resident_switches(5, 1025) == resident_switches(0, 1025), "5: the cost_aware walk without bulk runs");
static_assert(resident_switches(16, 1024) == ResidentSwitches{0, 0, 0, 0, 0, 1, 0, 0} &&
              resident_switches(16, 1025) == resident_switches(16, 1024), "16 holds at every size");
static_assert(resident_switches(32, 1024) == ResidentSwitches{0, 0, 0, 0, 1, 0, 0, 0} &&
              resident_switches(32, 1025) == resident_switches(32, 1024), "32 holds at every size");
static_assert(resident_switches(64 + (12 << 8), 1024) == ResidentSwitches{0, 0, 0, 0, 1, 1, 1, 12} &&
              resident_switches(64 + (12 << 8), 1025) == resident_switches(64 + (12 << 8), 1024),
              "64 and the list minimum hold at every size");
static_assert(resident_switches(2, 1024) == ResidentSwitches{1, 0, 1, 1, 1, 1, 0, 0}, "2: rotated walker");
// The switches as they took effect, in the PVT_RWALK bit values above (pvt_last_resident_shape):
// the word that decodes to `s`, with 3 written as 1 and no walk bit where nothing is walked.
constexpr uint32_t resident_switches_word(const ResidentSwitches& s) {
  return (s.walk_rotate ? 2u : s.walk_ca_bf ? 1u : 0u) | (s.walk_ff ? 8u : 0u) |
         (s.walks() && !s.walk_bulk ? 4u : 0u) | (s.bulk_sticky ? 0u : 16u) | (s.run_lists ? 0u : 32u) |
         (s.lists_all ? 64u : 0u) | ((uint32_t)s.list_min << 8);
}
static_assert(resident_switches_word(resident_switches(9, 1024)) == 9 &&
              resident_switches_word(resident_switches(9, 1025)) == 0, "the default; no walk above RW_MAXH");
static_assert(resident_switches_word(resident_switches(3, 1024)) == 1 &&
              resident_switches_word(resident_switches(10, 1024)) == 10 &&
              resident_switches_word(resident_switches(13, 1024)) == 13 &&
              resident_switches_word(resident_switches(13, 1025)) == 0, "the walk bits");
static_assert(resident_switches_word(resident_switches(73, 1024)) == 73 &&
              resident_switches_word(resident_switches(585, 1024)) == 585 &&
              resident_switches_word(resident_switches(585, 1025)) == 576 &&
              resident_switches_word(resident_switches(48, 4096)) == 48, "the 4-wave bits at every size");
static_assert(resident_switches(resident_switches_word(resident_switches(0x1f7f, 1024)), 1024) ==
              resident_switches(0x1f7f, 1024), "the word decodes to the same switches");
struct ResidentArgs {
  const void* rounds;     // device copy of pvt_round[n] (device array pointers)
  uint32_t* mt;           // [n][625] MT19937 states (PVT_OPP; the kernel uses R.mt_state)
  int Zb;                 // zone-table stride in LDS: max n_zones of the batch
  int Tpad;               // power of two >= max n_tasks of the batch (sort network size)
  uint64_t* stamps;       // diagnostic builds only (PVT_STAMPS): block 0 wave 0 phase cycles
  ResidentSwitches sw;
};
size_t resident_lds_bytes(int Zb, int Tpad, const ResidentSwitches& sw);
// Waves and hosts per lane of a batch whose largest round has maxH hosts. `pref` is the preferred
// number of waves: 4 (the default) or, as A/B preferences (PVT_RES_WAVES), 8 -- every resident
// size, at most 8 hosts per lane -- , 2 -- rounds of 513 to 2048 hosts, 8 or 16 hosts per lane --
// and 1 -- rounds of 513 to 1024 hosts, 16 hosts per lane; outside those sizes four waves.
struct ResidentShape {
  int waves, hpl;
};
constexpr ResidentShape resident_shape(int pref, int maxH) {
  const int w = (pref == 8 && maxH <= 8 * 8 * WAVE) ? 8
                : (pref == 2 && maxH > 2 * 4 * WAVE && maxH <= 2 * 16 * WAVE) ? 2
                : (pref == 1 && maxH > 8 * WAVE && maxH <= 16 * WAVE) ? 1 : 4;
  int h = 1;
  while (h * w * WAVE < maxH) h <<= 1;
  return ResidentShape{w, h};
}
constexpr bool operator==(const ResidentShape& a, const ResidentShape& b) {
  return a.waves == b.waves && a.hpl == b.hpl;
}
static_assert(resident_shape(4, 1) == ResidentShape{4, 1} && resident_shape(4, 256) == ResidentShape{4, 1} &&
              resident_shape(4, 257) == ResidentShape{4, 2} && resident_shape(4, 1024) == ResidentShape{4, 4} &&
              resident_shape(4, 1025) == ResidentShape{4, 8} && resident_shape(4, 2049) == ResidentShape{4, 16} &&
              resident_shape(4, RES_MAX_HOSTS) == ResidentShape{4, 16}, "the default: four waves");
static_assert(resident_shape(8, 1) == ResidentShape{8, 1} && resident_shape(8, 65) == ResidentShape{8, 1} &&
              resident_shape(8, 512) == ResidentShape{8, 1} && resident_shape(8, 513) == ResidentShape{8, 2} &&
              resident_shape(8, 1024) == ResidentShape{8, 2} && resident_shape(8, 1025) == ResidentShape{8, 4} &&
              resident_shape(8, 2048) == ResidentShape{8, 4} && resident_shape(8, 2049) == ResidentShape{8, 8} &&
              resident_shape(8, RES_MAX_HOSTS) == ResidentShape{8, 8}, "8: eight waves at every resident size");
static_assert(resident_shape(2, 512) == ResidentShape{4, 2} && resident_shape(2, 513) == ResidentShape{2, 8} &&
              resident_shape(2, 1024) == ResidentShape{2, 8} && resident_shape(2, 1025) == ResidentShape{2, 16} &&
              resident_shape(2, 2048) == ResidentShape{2, 16} && resident_shape(2, 2049) == ResidentShape{4, 16},
              "2: two waves for 513 to 2048 hosts, four outside");
static_assert(resident_shape(1, 512) == ResidentShape{4, 2} && resident_shape(1, 513) == ResidentShape{1, 16} &&
              resident_shape(1, 1024) == ResidentShape{1, 16} && resident_shape(1, 1025) == ResidentShape{4, 8},
              "1: one wave for 513 to 1024 hosts, four outside");
// lds: resident_lds_bytes of (a.Zb, a.Tpad, a.sw) at least
void launch_resident(int mode, int waves, int hpl, int n, size_t lds, const ResidentArgs& a,
                     hipStream_t st);
hipError_t resident_init_attrs();
// Batches with a round of more than ZMAX zones (pvt_batch_wide.hip): mode CA_FF, CA_BF or
// RES_MIXED -- batches of one other policy run launch_resident with a.Zb = 0. Four waves, hpl <=
// RES_WIDE_MAX_HPL (16 hosts per lane would spill registers), a.Zb = 0 and no walk switches.
constexpr int RES_WIDE_MAX_HPL = 8;
constexpr int RES_WIDE_MAX_HOSTS = 4 * WAVE * RES_WIDE_MAX_HPL;   // 2048
void launch_resident_wide(int mode, int hpl, int n, size_t lds, const ResidentArgs& a, hipStream_t st);
hipError_t resident_wide_init_attrs();

// The fused host batch (pvt_place_host_batch): per round (one workgroup of four waves), its byte
// ranges of the pinned stage -- the same offsets in the mapped host copy and the device copy --
// and its index in the stage's AnchorArgs / CaGroupArgs arrays (-1: no fused grouping).
struct FusedRound {
  int64_t out_lo, out_hi, in_lo, in_hi;
  int64_t desc;           // byte offset of its pvt_round (device array pointers)
  int32_t items, pad;
};
struct FusedArgs {
  const char* hmap;       // the mapped pinned stage (the device reads its inputs, writes results)
  char* dev;              // the device copy of the stage
  int64_t o_rounds;       // FusedRound[n] (read from hmap)
  int64_t o_ka, o_kg;     // AnchorArgs[ni], CaGroupArgs[ni] (read from hmap)
  ResidentArgs ra;        // Zb, Tpad, sw, stamps (rounds unused: each workgroup has its own)
};
size_t fused_pre_lds_bytes();   // LDS of the anchor and grouping phases
void launch_fused(int mode, int hpl, int n, size_t lds, const FusedArgs& F, hipStream_t st);
void launch_fused_wide(int mode, int hpl, int n, size_t lds, const FusedArgs& F, hipStream_t st);
size_t commit_lds_bytes();
hipError_t init_kernel_attrs();
// grouped processing order: group counts (cnt[G] = out-of-range ids), scatter by group, one
// LDS bitonic sort of (key, task index) per group of at most GSORT_MAX tasks
constexpr int GSORT_MAX = 4096;
void launch_group_hist(const int32_t* tg, int T, int G, int32_t* cnt, hipStream_t st);
// the grouped order's preparation in one block (T <= PREP_T_MAX, G <= GAGG_MAX): placement fill,
// group counts, pinned staging, offsets, zone tables, sort keys and the (key, task) scatter
constexpr int PREP_T_MAX = 65536;
constexpr int GAGG_MAX = 4096;
struct PrepArgs {
  const int32_t* tg;
  int T, G;
  const int32_t* ganc;
  const double* cost;
  const double* bw;
  int Z, nz2;                 // nz2: entries of the cost table staged (0: none)
  const double* dem;
  int sort_tasks;
  int32_t* placement;         // filled with -1, or NULL
  int32_t* off;               // [G + 1] group offsets in processing order
  int32_t* hcnt;              // pinned (device-mapped): counts [G + 1], anchors [G], cost [nz2]
  int32_t* hgan;
  double* hcst;
  double* csum;               // zone tables [Z * Z], or NULL
  double* bsum;
  uint64_t* skey;
  int32_t* sidx;
  int32_t* hflag;             // mapped pinned word, or NULL: order_count_kernel stores seq there
  int32_t seq;                //   once the staged counts are visible to the host
};
// counted (optional): recorded once the counts are staged, before the scatter launch (scatter
// = false: counts only, for launch_group_sort_gather)
void launch_order_prep(const PrepArgs& a, hipStream_t st, hipEvent_t counted = nullptr,
                       bool scatter = true);
// Few groups (G <= GCOMPACT_MAX): after the counts, one launch collects, sorts and gathers every
// group (order, caller order, demand rows, anchors, groups), fills placement and zone tables.
constexpr int GCOMPACT_MAX = 64;
struct GatherOut {
  int32_t* ord;
  double* dem_ord;
  int32_t* anc_ord;
  int32_t* grp_ord;
  int32_t* order_out;         // the caller's order, or NULL
  const double* avail;        // hmin != NULL: the same launch also writes the host minima over
  int H;                      //   [0, H) (ZW_MIN_PARTS partials as host_min_kernel's, one per
  double* hmin;               //   extra block)
  uint64_t* stamps;           // diagnostic builds only (PVT_STAMPS): block 0's phases, [16, 20)
  const int32_t* zone;        // zwin != NULL: Z more blocks prebuild the first epoch's zero-cost
  struct ZoneWindows* zwin;   //   windows from the snapshot (ZoneWindows), or NULL
  struct GroupCert* gcert;    // [G] group certificates written by the groups' blocks, or NULL
  // [T] gathered order, with gcert only, or NULL: the tasks from p to the end of p's stretch of
  // bit-identical demand rows inside its group, p counted (the frontier walk's run lengths)
  int32_t* run_rem;
};
static_assert(GC_SUB * 64 == GSORT_MAX, "a group record holds every sub-batch of a sorted group");
void launch_group_sort_gather(const PrepArgs& a, const GatherOut& o, hipStream_t st);
// bytes (rounded up to 16; both buffers 16-B aligned and that long) from mapped pinned memory
void launch_upload(const void* src_mapped, void* dst, size_t bytes, hipStream_t st);
void launch_restore_hosts(double* avail, const double* avail0, int H, const int32_t* hosts, int n,
                          hipStream_t st);
void launch_group_stage(const int32_t* cnt, int G, const int32_t* ganc, const double* cost, int nz2,
                        int32_t* off, int32_t* hcnt, int32_t* hgan, double* hcst, hipStream_t st);
void launch_group_scatter(const int32_t* tg, const uint64_t* keys, int T, int G, int32_t* cursor,
                          uint64_t* skey, int32_t* sidx, hipStream_t st);
void launch_group_sort(const int32_t* off, int G, const uint64_t* skey, const int32_t* sidx,
                       int32_t* ord, hipStream_t st);
void launch_iota(int32_t* out, int n, hipStream_t st);
// gather tasks into processing order: dem_ord[p][r] = dem[r*T + ord[p]], anc_ord[p]
void launch_gather_tasks(const double* dem, const int32_t* ord, const int32_t* task_group,
                         const int32_t* group_anchor, int T, double* dem_ord, int32_t* anc_ord,
                         int32_t* grp_ord, hipStream_t st, int G = 0x7fffffff,
                         int32_t* order_out = nullptr);

}  // namespace pvt
