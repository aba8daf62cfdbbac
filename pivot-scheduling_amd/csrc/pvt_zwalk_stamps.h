// pvt_zwalk_stamps.h — the frontier walk's instrumentation (PVT_STAMPS builds, `make stamps`;
// read by tools/zwalk_stamps.py). ZwStamps owns every counter and timestamp of zwalk_kernel; the
// walk calls its named methods where a phase ends or a path is taken. Without PVT_STAMPS the type
// is empty and every call compiles to nothing: no argument of a call may have a side effect.
#pragma once
#include <stdint.h>

#include "pvt_device.h"
#include "pvt_kernels.h"
#include "pvt_stamps.h"

namespace pvt {

#ifdef PVT_STAMPS
struct ZwStamps {
  uint64_t t_start = 0, t_load = 0, t_cert = 0, t_win = 0, t_cap = 0, t_walk = 0;
  uint64_t n_chunks = 0, n_switch = 0, n_bulk = 0, n_runs = 0;
  uint64_t st_search = 0, st_p1 = 0, st_p2 = 0, n_probe = 0, n_iter = 0, st_batch = 0, n_single = 0;
  uint64_t st_setup = 0, st_loop = 0, st_who = 0, st_rep = 0;   // run_bulk's parts
  uint64_t n_part = 0, s_pasg = 0, n_fromc = 0, n_rep = 0;       // pass 2: calls with a partial lane, its asg; replays from c; copies
  // per chain (ZW_STAMP_CHAIN): run_bulk calls; those that continue a run a cap cut (the task
  // before the call's first has its demand row, anchor and segment: Ec, per batch); the cycles
  // between one call's return and the next one's entry; a continued call's cost from the return
  // before it to its own
  uint64_t n_calls = 0, n_cont = 0, st_between = 0, st_cont = 0, t_ret = 0, Ec = 0;
  uint64_t tA = 0, tA1 = 0, tB = 0, tC = 0, gap = 0, t0 = 0, tb0 = 0;   // the open call / search / batch part
  bool contd = false;
  double pl[4] = {0.0, 0.0, 0.0, 0.0};       // the last batch's last demand row and anchor (Ec)
  int panc = -1, prr = 0;

  // phases of the prologue (the fast prologue's window is part of its entry loads)
  __device__ __forceinline__ void start() { t_start = cycle_stamp(); }
  __device__ __forceinline__ void loaded() { t_load = cycle_stamp(); }
  __device__ __forceinline__ void certified() { t_cert = cycle_stamp(); }
  __device__ __forceinline__ void certified_fast() { t_cert = t_win = t_cap = cycle_stamp(); }
  __device__ __forceinline__ void window_built() { t_win = cycle_stamp(); }
  __device__ __forceinline__ void capacities_loaded() { t_cap = cycle_stamp(); }
  __device__ __forceinline__ void walk_begins() { t_walk = cycle_stamp(); }

  // run_bulk: entry (k: the call's first ring position), the ends of its parts, exit
  __device__ __forceinline__ void bulk_enter(int k) {
    tA = cycle_stamp();
    gap = t_ret ? tA - t_ret : 0;
    contd = (Ec >> (k & 63)) & 1ull;
    n_calls++;
    st_between += gap;
  }
  __device__ __forceinline__ void bulk_setup_done() { tA1 = cycle_stamp(); st_setup += tA1 - tA; }
  __device__ __forceinline__ void bulk_pass1_done(int t) { n_iter += t; st_loop += cycle_stamp() - tA1; }
  __device__ __forceinline__ void bulk_counted() { tB = cycle_stamp(); st_p1 += tB - tA; }
  __device__ __forceinline__ void bulk_assigned(int asg, int cnt, uint64_t over) {
    const uint64_t part = __ballot(asg > 0 && asg < cnt);
    n_part += part != 0;
    if (part) s_pasg += (uint64_t)__builtin_amdgcn_readlane(asg, __builtin_ctzll(part));
    n_fromc += over != 0;
    tC = cycle_stamp();
    st_who += tC - tB;
  }
  __device__ __forceinline__ void bulk_replay_block() { n_rep += 4; }
  __device__ __forceinline__ void bulk_replayed() { st_rep += cycle_stamp() - tC; }
  __device__ __forceinline__ void bulk_exit() {
    t_ret = cycle_stamp();
    st_p2 += t_ret - tB;
    if (contd) { n_cont++; st_cont += gap + (t_ret - tA); }
  }

  // a batch's head and tail (records, run masks, log flush)
  __device__ __forceinline__ void batch_part_begins() { tb0 = cycle_stamp(); }
  __device__ __forceinline__ void batch_part_ends() { st_batch += cycle_stamp() - tb0; }
  // Ec: E, and the batch's first task against the last batch's last
  __device__ __forceinline__ void batch_runs(uint64_t E, int i0, int kn, int lane, double d0, double d1,
                                             double d2, double d3, int tanc, int trr, bool rrm,
                                             bool segm, const uint64_t* sbits) {
    const double td[4] = {d0, d1, d2, d3};
    bool c0 = i0 > 0 && lane == 0 && tanc == panc;
#pragma unroll
    for (int r = 0; r < 4; r++) c0 = c0 && __double_as_longlong(td[r]) == __double_as_longlong(pl[r]);
    if (segm) c0 = c0 && !(rfl_u64(sbits[i0 >> 6]) & 1ull);
    Ec = E | (__ballot(c0) & 1ull);
    if (rrm) {                               // (the task before belongs to a stretch that goes on)
      const int up = __shfl_up(trr, 1);
      Ec = __ballot(lane < kn && (lane == 0 ? (i0 > 0 && prr >= 2) : up >= 2));
      prr = readlane_i(trr, 63);
    }
#pragma unroll
    for (int r = 0; r < 4; r++) pl[r] = readlane_d(td[r], 63);
    panc = readlane_i(tanc, 63);
  }

  // the walk's paths (run_placed: a run of that many tasks, 0: none)
  __device__ __forceinline__ void search_begins() { t0 = cycle_stamp(); }
  __device__ __forceinline__ void search_ends() { st_search += cycle_stamp() - t0; }
  __device__ __forceinline__ void probe() { n_probe++; }
  __device__ __forceinline__ void run_placed(int tasks) { n_chunks += tasks; n_bulk += tasks; n_runs += tasks > 0; }
  __device__ __forceinline__ void single_placed() { n_chunks++; n_single++; }
  __device__ __forceinline__ void chunk_scanned() { n_chunks++; }
  __device__ __forceinline__ void anchor_switched() { n_switch++; }

  // the sums, by one lane of the chain's walker (slot 28 is unused)
  __device__ __forceinline__ void add_to(uint64_t* stamps, int b, int done, int nt) {
    if (!stamps) return;
    const uint64_t t_end = cycle_stamp();
    auto add = [&](int slot, uint64_t v) {
      atomicAdd((unsigned long long*)&stamps[slot], (unsigned long long)v);
    };
    add(0, t_walk - t_start); add(1, t_end - t_walk); add(2, n_chunks); add(3, (uint64_t)done);
    add(4, n_switch); add(5, n_bulk); add(6, n_runs); add(7, st_search);
    add(8, st_p1); add(9, st_p2); add(10, n_probe); add(11, n_iter);
    add(12, st_batch); add(13, n_single); add(14, n_part); add(15, s_pasg);
    add(30, n_fromc); add(31, n_rep);
    add(20, t_cert - t_start); add(21, t_win - t_cert); add(22, t_cap - t_win); add(23, t_walk - t_cap);
    add(24, st_setup); add(25, st_loop); add(26, st_who); add(27, st_rep);
    add(29, t_load - t_start);
    if (b < ZW_STAMP_CHAINS) {
      const uint64_t v[8] = {n_calls, n_cont, st_between, st_cont, t_end - t_walk, (uint64_t)done,
                             (uint64_t)nt, 0};
      for (int q = 0; q < 8; q++) add(ZW_STAMP_CHAIN + 8 * b + q, v[q]);
    }
  }
};
#else
struct ZwStamps {
  static __device__ __forceinline__ void start() {}
  static __device__ __forceinline__ void loaded() {}
  static __device__ __forceinline__ void certified() {}
  static __device__ __forceinline__ void certified_fast() {}
  static __device__ __forceinline__ void window_built() {}
  static __device__ __forceinline__ void capacities_loaded() {}
  static __device__ __forceinline__ void walk_begins() {}
  static __device__ __forceinline__ void bulk_enter(int) {}
  static __device__ __forceinline__ void bulk_setup_done() {}
  static __device__ __forceinline__ void bulk_pass1_done(int) {}
  static __device__ __forceinline__ void bulk_counted() {}
  static __device__ __forceinline__ void bulk_assigned(int, int, uint64_t) {}
  static __device__ __forceinline__ void bulk_replay_block() {}
  static __device__ __forceinline__ void bulk_replayed() {}
  static __device__ __forceinline__ void bulk_exit() {}
  static __device__ __forceinline__ void batch_part_begins() {}
  static __device__ __forceinline__ void batch_part_ends() {}
  static __device__ __forceinline__ void batch_runs(uint64_t, int, int, int, double, double, double, double, int,
                                             int, bool, bool, const uint64_t*) {}
  static __device__ __forceinline__ void search_begins() {}
  static __device__ __forceinline__ void search_ends() {}
  static __device__ __forceinline__ void probe() {}
  static __device__ __forceinline__ void run_placed(int) {}
  static __device__ __forceinline__ void single_placed() {}
  static __device__ __forceinline__ void chunk_scanned() {}
  static __device__ __forceinline__ void anchor_switched() {}
  static __device__ __forceinline__ void add_to(uint64_t*, int, int, int) {}
};
#endif

}  // namespace pvt
