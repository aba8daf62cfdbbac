// pvt_stamps.h — the device stamps of the diagnostic build (`make stamps`, -DPVT_STAMPS): the one
// clock reader, a phase clock, each instrumented kernel's stamps type, and the slot map of the
// shared buffer (ctx->stamps, read back by pvt_debug_commit_stamps for tools/*_stamps.py). The
// frontier walk's type, ZwStamps, is in pvt_zwalk_stamps.h.
//
// A kernel owns one stamps object and calls its named methods where a phase ends or a path is
// taken. Without PVT_STAMPS every type is empty, every method a static no-op and a call compiles
// to nothing: no argument of a stamps call may have a side effect. The default build's device
// assembly is the gate for a new call (`make isa-diff`, EXPERIMENTS.md round 13): an empty call
// at the end of a short `if` or right after one has changed the register allocation; a few lines
// earlier or later it did not.
// PVT_STAMPS is tested here, in pvt_zwalk_stamps.h and in pvt_debug_commit_stamps, nowhere else.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pvt {

// ---- The slot map (uint64 words). Every kernel adds into the same buffer; a tool zeroes it, runs
// one kind of round and reads the ranges of the kernels that round launches. Ranges of different
// kernels overlap where no tool's run launches both:
//   resident batch (resident_stamps.py)   [0, 15) + [24, 26) + per-round [32, 32 + 4096)
//   fused host batch (fused_stamps.py)    the resident ranges + [16, 21)
//   windowed round (commit_stamps.py)     commit walk [0, 7)  or  opportunistic walk [0, 14)
//   list walk (lwalk_stamps.py)           [0, 9)
//   grouped order launch (order_stamps.py) [16, 20) (beside the frontier walk's [0, 16), [20, 32))
//   frontier walk (zwalk_stamps.py)       [0, 32) + per-chain [ZW_STAMP_CHAIN, + 8 * 64)
// so the resident phases, the three walks and the frontier walk all start at 0, and 16-19 is the
// fused phases' or the order launch's, never in one run.
//
// resident_round, block 0, wave 0 (ResRoundStamps): cycles of 0 anchor rows, 1 slot scan, 2 wave
// reduction, 3 exchange (post, barrier, merge), 4 full path, 5 commit; counts: 6 tasks, 7 full paths
constexpr int RES_ST_ROUND = 0;
// the one-wave walks, block 0: tasks walked and the walk's cycles as the round sees it (thread 0);
// the walking wave's (ResWalkStamps) LDS chunk probes, register-chunk advances, (12: unused,)
// cycles in the task bodies, cycles of its whole walk, bulk runs and the tasks they placed
constexpr int RES_ST_WALKED = 8, RES_ST_WALK_CYC = 9, RES_ST_PROBES = 10, RES_ST_ADVANCES = 11,
              RES_ST_TASK_CYC = 13, RES_ST_WALKER_CYC = 14, RES_ST_BULK = 24, RES_ST_BULK_TASKS = 25;
// resident_fused_kernel, block 0, thread 0 (FusedStamps): cycles of stage in, anchors, grouping,
// placement, results out
constexpr int FUSED_ST = 16;
// resident_kernel, every block b < RES_STAMP_ROUNDS (RoundCycles): the workgroup's cycles, set
constexpr int RES_STAMP_BASE = 32, RES_STAMP_ROUNDS = 4096;
// commit_kernel's walker (CommitStamps): cycles of 0 wait-prefetch, 1 hash lookup, 2 untouched
// pick, 3 touched rescore, 4 commit; 5 tasks walked (the status), 6 live touched hosts, summed
constexpr int COMMIT_ST = 0;
// lwalk_kernel (LwalkStamps): cycles of 0 task record, 1 untouched pick, 2 touched rescore,
// 3 commit; counts: 4 tasks, 5 chunk loads, 6 live iterations, 7 touched winners, 8 live hosts, summed
constexpr int LWALK_ST = 0;
// opp_commit_kernel (OppStamps): cycles of 0 pass 1, 1 pass 2, 5 / 6 / 2 pass 3's select and load,
// candidates, capacities, 9 / 8 / 3 pass 4's setup, loop, commits; counts: 4 ranges, 7 tasks,
// 13 pass-4 commits, 11 those lost to a later task, 12 those in a later task's id range (10: unused)
constexpr int OPP_ST = 0;
// group_sort_gather_kernel, group 0, thread 0 (OrderStamps): cycles of setup, key build, sort, gather
constexpr int ORDER_ST = 16;
// zwalk_kernel: [0, 32) as ZwStamps::add_to lists them, and chain b's own 8 words from
// ZW_STAMP_CHAIN + 8 b, b < ZW_STAMP_CHAINS (past the per-round words): run_bulk calls,
// continued-run calls, cycles between calls, cycles of the continued calls with the gap before
// each, walk cycles, tasks walked, chain tasks, 0
constexpr int ZW_STAMP_CHAIN = RES_STAMP_BASE + RES_STAMP_ROUNDS, ZW_STAMP_CHAINS = 64;
constexpr int STAMP_WORDS = ZW_STAMP_CHAIN + 8 * ZW_STAMP_CHAINS;   // the buffer

#ifdef PVT_STAMPS
#define PVT_ST __device__ __forceinline__ void          // (a method of a kernel's type, below)
__device__ __forceinline__ uint64_t cycle_stamp() {
  uint64_t t;
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  __builtin_amdgcn_sched_barrier(0);
  return t;
}

// N words of cycle sums and counts, and the clock that laps into them.
template <int N>
struct PhaseClock {
  uint64_t ph[N] = {}, last = 0;
  bool on = false;
  __device__ __forceinline__ void begin(bool enabled) { on = enabled; last = on ? cycle_stamp() : 0; }
  __device__ __forceinline__ void lap(int k) {   // ph[k] += now - last; last = now
    if (!on) return;
    const uint64_t t = cycle_stamp();
    ph[k] += t - last;
    last = t;
  }
  __device__ __forceinline__ void count(int k, uint64_t n = 1) { if (on) ph[k] += n; }
  static __device__ __forceinline__ void stamps_barrier() { __syncthreads(); }   // (this build's only)
  // ph[0..N) into slots[0..N): plainly (a single writer) or with atomicAdd (many workgroups)
  __device__ __forceinline__ void store_to(uint64_t* slots, bool writer) const {
    if (on && writer)
      for (int k = 0; k < N; k++) slots[k] += ph[k];
  }
  __device__ __forceinline__ void add_to(uint64_t* slots, bool writer) const {
    if (on && writer)
      for (int k = 0; k < N; k++) atomicAdd((unsigned long long*)&slots[k], (unsigned long long)ph[k]);
  }
};

// resident_walk / resident_walk_ff: the walking wave's counters (RES_ST_PROBES .. RES_ST_BULK_TASKS)
struct ResWalkStamps {
  uint64_t n_probe = 0, n_adv = 0, st_task = 0, n_bulk = 0, n_bulk_tasks = 0, t_start = 0, t_task = 0;
  __device__ __forceinline__ void walk_begins() { t_start = cycle_stamp(); }
  __device__ __forceinline__ void task_begins() { t_task = cycle_stamp(); }
  __device__ __forceinline__ void task_ends() { st_task += cycle_stamp() - t_task; }
  __device__ __forceinline__ void chunk_probed() { n_probe++; }
  __device__ __forceinline__ void chunk_advanced() { n_adv++; }
  __device__ __forceinline__ void run_placed(int tasks) { n_bulk++; n_bulk_tasks += tasks; }
  __device__ __forceinline__ void walk_ends(uint64_t* stamps, int lane) {
    if (blockIdx.x != 0 || lane != 0 || !stamps) return;
    stamps[RES_ST_PROBES] += n_probe;
    stamps[RES_ST_ADVANCES] += n_adv;
    stamps[RES_ST_TASK_CYC] += st_task;
    stamps[RES_ST_BULK] += n_bulk;
    stamps[RES_ST_BULK_TASKS] += n_bulk_tasks;
    stamps[RES_ST_WALKER_CYC] += cycle_stamp() - t_start;   // (its records included)
  }
};

// resident_kernel: one workgroup's cycles from its start to its end
struct RoundCycles {
  uint64_t t0 = 0;
  __device__ __forceinline__ void begin() { t0 = cycle_stamp(); }
  __device__ __forceinline__ void end(uint64_t* stamps) {
    if (threadIdx.x == 0 && stamps && blockIdx.x < RES_STAMP_ROUNDS)
      stamps[RES_STAMP_BASE + blockIdx.x] = cycle_stamp() - t0;
  }
};
#else
#define PVT_ST static __device__ __forceinline__ void   // (static: a call must not touch the object)
template <int N>
struct PhaseClock {
  static __device__ __forceinline__ void begin(bool) {}
  static __device__ __forceinline__ void lap(int) {}
  static __device__ __forceinline__ void count(int, uint64_t = 1) {}
  static __device__ __forceinline__ void stamps_barrier() {}
  static __device__ __forceinline__ void store_to(uint64_t*, bool) {}
  static __device__ __forceinline__ void add_to(uint64_t*, bool) {}
};
struct ResWalkStamps {
  static __device__ __forceinline__ void walk_begins() {}
  static __device__ __forceinline__ void task_begins() {}
  static __device__ __forceinline__ void task_ends() {}
  static __device__ __forceinline__ void chunk_probed() {}
  static __device__ __forceinline__ void chunk_advanced() {}
  static __device__ __forceinline__ void run_placed(int) {}
  static __device__ __forceinline__ void walk_ends(uint64_t*, int) {}
};
struct RoundCycles {
  static __device__ __forceinline__ void begin() {}
  static __device__ __forceinline__ void end(uint64_t*) {}
};
#endif

// ---- The kernels' types: names for a PhaseClock's laps and counts. Without PVT_STAMPS their
// methods are static too (PVT_ST): a call that took the object's address changed the default
// build's register allocation, one that does not compiles to the parent's code.
struct ResRoundStamps : PhaseClock<8>, PhaseClock<2> {
  using Round = PhaseClock<8>;              // the 4-wave path's phases and counts
  using Walk = PhaseClock<2>;               // a one-wave walk as the round sees it: tasks, cycles
  PVT_ST walk_called(const uint64_t* stamps, int tid) { Walk::begin(blockIdx.x == 0 && tid == 0 && stamps); }
  PVT_ST walk_returned(uint64_t* stamps, int walked) {
    Walk::count(0, walked);
    Walk::lap(1);
    Walk::store_to(stamps + RES_ST_WALKED, true);
  }
  PVT_ST round_begins(const uint64_t* stamps, int wave) { Round::begin(blockIdx.x == 0 && wave == 0 && stamps); }
  PVT_ST rows_loaded() { Round::lap(0); Round::count(6); }   // (once per task)
  PVT_ST scanned() { Round::lap(1); }
  PVT_ST reduced() { Round::lap(2); }
  PVT_ST exchanged() { Round::lap(3); }
  PVT_ST full_path_done() { Round::count(7); Round::lap(4); }
  PVT_ST committed() { Round::lap(5); }
  PVT_ST round_ends(uint64_t* stamps, int lane) { Round::store_to(stamps + RES_ST_ROUND, lane == 0); }
};

struct FusedStamps : PhaseClock<5> {
  PVT_ST begins(const uint64_t* stamps) { begin(blockIdx.x == 0 && threadIdx.x == 0 && stamps); }
  PVT_ST staged_in() { lap(0); }
  PVT_ST anchors_done() { lap(1); }
  PVT_ST grouped() { lap(2); }
  PVT_ST placed() { lap(3); }
  PVT_ST results_out(uint64_t* stamps) { lap(4); store_to(stamps + FUSED_ST, true); }
};

struct CommitStamps : PhaseClock<7> {
  PVT_ST begins() { begin(true); }
  PVT_ST slot_read() { lap(0); }
  PVT_ST looked_up() { lap(1); }
  PVT_ST picked() { lap(2); }
  PVT_ST rescored() { lap(3); }
  PVT_ST waits() { lap(3); lap(4); }                  // (a task no host fits)
  PVT_ST committed(int live) { count(6, live); lap(4); }
  PVT_ST walk_ends(uint64_t* stamps, int lane, int status) {
    count(5, status < 0 ? 0 : status);
    add_to(stamps + COMMIT_ST, lane == 0 && stamps);
  }
};

struct LwalkStamps : PhaseClock<9> {
  PVT_ST begins() { begin(true); }
  PVT_ST chunk_loaded() { count(5); }
  PVT_ST task_read(int live) { count(4); count(8, live); lap(0); }
  PVT_ST run_placed(int tasks) { count(4, tasks - 1); lap(3); }   // (task_read counted its first)
  PVT_ST picked() { lap(1); }
  PVT_ST live_iteration() { count(6); }
  PVT_ST rescored(bool touched_wins) { lap(2); count(7, touched_wins); }
  PVT_ST committed() { lap(3); }
  PVT_ST walk_ends(uint64_t* stamps, int lane) { add_to(stamps + LWALK_ST, lane == 0 && stamps); }
};

struct OppStamps : PhaseClock<14> {
  PVT_ST begins() { begin(true); }
  PVT_ST counted() { lap(0); }
  PVT_ST drawn() { lap(1); }
  PVT_ST selected() { lap(5); }
  PVT_ST candidates_built() { lap(6); }
  PVT_ST capacities_loaded() { lap(2); }
  PVT_ST walk_set_up() { lap(9); }
  PVT_ST commit_checked(uint64_t lost, uint64_t in_range) { count(13); count(11, lost != 0); count(12, in_range != 0); }
  PVT_ST walked() { lap(8); }
  PVT_ST range_done() { lap(3); count(4); }
  PVT_ST walk_ends(uint64_t* stamps, int tx, int tasks) { count(7, tasks); add_to(stamps + OPP_ST, tx == 0 && stamps); }
};

struct OrderStamps : PhaseClock<4> {
  PVT_ST begins(const uint64_t* stamps, int g, int tid) { begin(g == 0 && tid == 0 && stamps); }
  PVT_ST set_up() { lap(0); }
  PVT_ST keys_built() { lap(1); }
  PVT_ST sorted() { lap(2); }
  PVT_ST gathered(uint64_t* stamps) { stamps_barrier(); lap(3); add_to(stamps + ORDER_ST, true); }
};

#undef PVT_ST

}  // namespace pvt
