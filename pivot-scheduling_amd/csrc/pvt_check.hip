// pvt_check.hip — opt-in validation of a round's contents (pvt_check_round / pvt_check_batch and
// the pvt_set_checks switch; rules: include/pivot_place.h, predicates: pvt_check_rules.h).
//
// One launch checks n rounds. The launch's blocks (256 threads, four wave64) are dealt to the
// rounds in proportion to their bytes, at least one block each, and the grid is sized from the
// CU count, never from H. A round's blocks grid-stride each of its arrays in turn: fp64 arrays
// 16 bytes per lane (one 1-KiB load per wave) with a scalar head and tail where the pointer or
// the length is odd, index arrays 4 bytes per lane. Every index is tested before it is used
// (rule 10 reads owner[rank] only for rank < H), and only the round's inputs are read. A
// thread keeps (~lowest violating index, count) per array; a wave that saw a violation reduces
// the pair across its lanes and adds it to the block's LDS slots, and a block adds a violated
// rule's slot to the round's with one integer atomicMax and one integer atomicAdd, so the report
// is the same whatever the block schedule. A clean round costs no atomic at all.
//
// Rule 10 (distinct tiebreak ranks) takes two passes without a sort: check_owner_kernel records
// owner[rank] = the lowest host holding the rank (integer atomicMin), then host h violates when
// its rank is out of range or owner[rank] != h -- every holder of a duplicated rank but the first.
// HBM-bound streaming reduction, no MFMA.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "pvt_check.h"
#include "pvt_kernels.h"

namespace pvt {

namespace {

using u64 = unsigned long long;

struct Acc {
  u64 key = 0;   // ~(lowest violating index), 0: none
  u64 cnt = 0;
};

__device__ __forceinline__ void hit(Acc& a, int64_t i) {
  const u64 k = ~(u64)i;
  a.key = k > a.key ? k : a.key;
  a.cnt++;
}

// Every lane of the wave calls this (block-uniform control flow around it).
__device__ __forceinline__ void flush(const Acc& a, int rule, u64* s_key, u64* s_cnt) {
  if (__ballot(a.cnt != 0) == 0) return;
  u64 key = a.key, cnt = a.cnt;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u64 k = __shfl_xor(key, o, 64);
    key = k > key ? k : key;
    cnt += __shfl_xor(cnt, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    atomicMax(&s_key[rule], key);
    atomicAdd(&s_cnt[rule], cnt);
  }
}

template <bool RT>
__device__ __forceinline__ bool bad_amount(double v) {
  return RT ? chk_bad_rt_bw(v) : chk_bad_amount(v);
}

// fp64 array p[0 .. n): rules 2, 3 (RT = false) and 8 (RT = true)
template <bool RT>
__device__ __forceinline__ Acc scan_amounts(const double* p, int64_t n, int64_t tid, int64_t stride) {
  Acc a;
  if (!p || n <= 0) return a;
  const uintptr_t ad = reinterpret_cast<uintptr_t>(p);
  // elements in front of the first 16-byte boundary (all of them for a pointer that is not even
  // 8-byte aligned: those take the scalar path)
  int64_t head = (ad & 7) ? n : ((ad & 15) ? 1 : 0);
  if (head > n) head = n;
  const int64_t pairs = (n - head) / 2;
  const double2* q = reinterpret_cast<const double2*>(p + head);
#pragma unroll 4
  for (int64_t i = tid; i < pairs; i += stride) {
    const double2 v = q[i];
    if (bad_amount<RT>(v.x)) hit(a, head + 2 * i);
    if (bad_amount<RT>(v.y)) hit(a, head + 2 * i + 1);
  }
  const int64_t ns = n - 2 * pairs;   // the head and the tail
  for (int64_t s = tid; s < ns; s += stride) {
    const int64_t i = s < head ? s : 2 * pairs + s;
    if (bad_amount<RT>(p[i])) hit(a, i);
  }
  return a;
}

__device__ __forceinline__ Acc scan_index(const int32_t* p, int64_t n, int32_t bound, int64_t tid,
                                          int64_t stride) {
  Acc a;
  if (!p) return a;
  for (int64_t i = tid; i < n; i += stride)
    if (chk_bad_index(p[i], bound)) hit(a, i);
  return a;
}

// The round of this block: the last one whose first block is not past it.
__device__ __forceinline__ int round_of_block(const CheckRound* rounds, int n) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (rounds[mid].blk_lo <= (int)blockIdx.x) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__global__ void __launch_bounds__(CHK_THREADS) check_owner_kernel(const CheckRound* rounds, int n) {
  const CheckRound& r = rounds[round_of_block(rounds, n)];
  const uint32_t* tb = r.tiebreak;
  uint32_t* owner = r.owner;
  const int b = (int)blockIdx.x - r.blk_lo;
  if (!tb || !owner || b < 0 || b >= r.blk_n) return;
  const int32_t H = r.H;
  const int64_t stride = (int64_t)r.blk_n * CHK_THREADS;
  for (int64_t h = (int64_t)b * CHK_THREADS + threadIdx.x; h < H; h += stride) {
    const uint32_t rank = tb[h];
    if (!chk_bad_rank(rank, H)) atomicMin(&owner[rank], (uint32_t)h);
  }
}

__global__ void __launch_bounds__(CHK_THREADS) check_kernel(const CheckRound* rounds, int n,
                                                            CheckSlots* slots) {
  __shared__ u64 s_key[CHK_RULES + 1], s_cnt[CHK_RULES + 1];
  const int ri = round_of_block(rounds, n);
  const CheckRound r = rounds[ri];
  const int b = (int)blockIdx.x - r.blk_lo;
  if (b < 0 || b >= r.blk_n) return;   // (block-uniform)
  if (threadIdx.x <= CHK_RULES) s_key[threadIdx.x] = s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const int64_t tid = (int64_t)b * CHK_THREADS + threadIdx.x;
  const int64_t stride = (int64_t)r.blk_n * CHK_THREADS;
  const int32_t H = r.H, T = r.T, Z = r.Z;

  flush(scan_index(r.zone, H, Z, tid, stride), PVT_CHK_ZONE, s_key, s_cnt);
  flush(scan_amounts<false>(r.avail, 4 * (int64_t)H, tid, stride), PVT_CHK_AVAIL, s_key, s_cnt);
  flush(scan_amounts<false>(r.dem, 4 * (int64_t)T, tid, stride), PVT_CHK_DEM, s_key, s_cnt);
  flush(scan_index(r.task_group, T, r.G, tid, stride), PVT_CHK_GROUP, s_key, s_cnt);
  flush(scan_index(r.group_anchor, r.G, Z, tid, stride), PVT_CHK_ANCHOR, s_key, s_cnt);
  {
    Acc ac, ab;
    const int64_t zz = (int64_t)Z * Z;
    if (r.cost && r.bw)
      for (int64_t i = tid; i < zz; i += stride) {
        const int64_t j = (i % Z) * Z + i / Z;   // the transposed entry
        if (chk_bad_cost_sum(r.cost[i] + r.cost[j])) hit(ac, i);
        if (chk_bad_bw_sum(r.bw[i] + r.bw[j])) hit(ab, i);
      }
    flush(ac, PVT_CHK_COST, s_key, s_cnt);
    flush(ab, PVT_CHK_BW, s_key, s_cnt);
  }
  flush(scan_amounts<true>(r.rt_bw, r.n_rt, tid, stride), PVT_CHK_RTBW, s_key, s_cnt);
  {
    Acc a;
    if (r.decay)
      for (int64_t h = tid; h < H; h += stride)
        if (chk_bad_decay(r.decay[h])) hit(a, h);
    flush(a, PVT_CHK_DECAY, s_key, s_cnt);
  }
  {
    Acc a;
    if (r.tiebreak && r.owner)
      for (int64_t h = tid; h < H; h += stride) {
        const uint32_t rank = r.tiebreak[h];
        if (chk_bad_rank(rank, H) || r.owner[rank] != (uint32_t)h) hit(a, h);
      }
    flush(a, PVT_CHK_TIEBREAK, s_key, s_cnt);
  }
  __syncthreads();
  if (threadIdx.x >= 1 && threadIdx.x < CHK_RULES && s_cnt[threadIdx.x]) {
    atomicMax(&slots[ri].key[threadIdx.x], s_key[threadIdx.x]);
    atomicAdd(&slots[ri].cnt[threadIdx.x], s_cnt[threadIdx.x]);
  }
}

// The element a report names (ints converted; rules 6 / 7: the sum).
__host__ __device__ inline double chk_value(const CheckRound& r, int code, int64_t i) {
  const int64_t Z = r.Z;
  switch (code) {
    case PVT_CHK_ZONE: return (double)r.zone[i];
    case PVT_CHK_AVAIL: return r.avail[i];
    case PVT_CHK_DEM: return r.dem[i];
    case PVT_CHK_GROUP: return (double)r.task_group[i];
    case PVT_CHK_ANCHOR: return (double)r.group_anchor[i];
    case PVT_CHK_COST: return r.cost[i] + r.cost[(i % Z) * Z + i / Z];
    case PVT_CHK_BW: return r.bw[i] + r.bw[(i % Z) * Z + i / Z];
    case PVT_CHK_RTBW: return r.rt_bw[i];
    case PVT_CHK_DECAY: return (double)r.decay[i];
    case PVT_CHK_TIEBREAK: return (double)r.tiebreak[i];
    default: return 0.0;
  }
}

__host__ __device__ inline void chk_report(const CheckRound& r, const CheckSlots& s,
                                           pvt_check_report* out) {
  int code = 0, mask = 0;
  for (int k = 1; k < CHK_RULES; k++)   // (rule 11 is the host's)
    if (s.cnt[k]) {
      mask |= 1 << k;
      if (!code) code = k;
    }
  out->code = code;
  out->mask = mask;
  out->index = code ? (int64_t)~s.key[code] : -1;
  out->count = code ? (int64_t)s.cnt[code] : 0;
  out->value = code ? chk_value(r, code, out->index) : 0.0;
}

__global__ void __launch_bounds__(CHK_THREADS) check_finish_kernel(const CheckRound* rounds, int n,
                                                                   const CheckSlots* slots,
                                                                   pvt_check_report* out) {
  const int i = blockIdx.x * CHK_THREADS + threadIdx.x;
  if (i < n) chk_report(rounds[i], slots[i], &out[i]);
}

}  // namespace

CheckRound check_describe(const pvt_round& r) {
  CheckRound c{};
  const bool ca = r.mode == PVT_CA_FF || r.mode == PVT_CA_BF;
  const int T = r.n_tasks;
  const bool grouped = r.task_group && T > 0;
  c.mode = r.mode; c.H = r.n_hosts; c.T = T; c.Z = r.n_zones;
  c.G = r.task_group ? r.n_groups : 0;
  c.n_rt = (int64_t)std::max(c.G, 1) * r.n_hosts;
  c.avail = r.avail;
  c.zone = r.zone;
  c.dem = T > 0 ? r.dem : nullptr;
  c.task_group = grouped ? r.task_group : nullptr;
  c.group_anchor = grouped ? r.group_anchor : nullptr;
  c.cost = ca && T > 0 ? r.cost : nullptr;
  c.bw = ca && T > 0 ? r.bw : nullptr;
  c.rt_bw = ca ? r.rt_bw : nullptr;
  c.decay = r.decay;
  c.tiebreak = r.mode == PVT_VBP_BF ? r.tiebreak : nullptr;
  return c;
}

double check_bytes(const CheckRound& c) {
  double b = 36.0 * c.H;                                  // avail + zone
  if (c.dem) b += 32.0 * c.T;
  if (c.task_group) b += 4.0 * c.T + 4.0 * std::max(c.G, 0);
  if (c.cost) b += 32.0 * c.Z * c.Z;                      // cost and bw, each entry and its transpose
  if (c.rt_bw) b += 8.0 * (double)c.n_rt;
  if (c.decay) b += 4.0 * c.H;
  if (c.tiebreak) b += 12.0 * c.H;                        // ranks twice, owners once
  return b;
}

int check_deal(CheckRound* rounds, int n, int cus) {
  double total = 0.0;
  for (int i = 0; i < n; i++) total += check_bytes(rounds[i]);
  const double budget = std::max(n, std::max(cus, 1) * CHK_BLOCKS_PER_CU);
  int grid = 0;
  for (int i = 0; i < n; i++) {
    const double bytes = check_bytes(rounds[i]);
    const double worth = (bytes + CHK_BLOCK_BYTES - 1) / CHK_BLOCK_BYTES;
    const double share = total > 0.0 ? budget * bytes / total : 1.0;
    rounds[i].blk_lo = grid;
    rounds[i].blk_n = (int)std::max(1.0, std::min(share, worth));
    grid += rounds[i].blk_n;
  }
  return grid;
}

void launch_check_owner(const CheckRound* rounds_dev, int n, int grid, hipStream_t st) {
  if (n > 0 && grid > 0)
    PVT_LAUNCH(check_owner_kernel, dim3(grid), dim3(CHK_THREADS), 0, st, rounds_dev, n);
}

void launch_check(const CheckRound* rounds_dev, int n, int grid, CheckSlots* slots, hipStream_t st) {
  if (n > 0 && grid > 0)
    PVT_LAUNCH(check_kernel, dim3(grid), dim3(CHK_THREADS), 0, st, rounds_dev, n, slots);
}

void launch_check_finish(const CheckRound* rounds_dev, int n, const CheckSlots* slots,
                         pvt_check_report* out_dev, hipStream_t st) {
  if (n > 0)
    PVT_LAUNCH(check_finish_kernel, dim3((n + CHK_THREADS - 1) / CHK_THREADS), dim3(CHK_THREADS), 0,
               st, rounds_dev, n, slots, out_dev);
}

void check_on_host(const CheckRound& c, pvt_check_report* out) {
  CheckSlots s{};
  auto hit = [&s](int rule, int64_t i) {
    const u64 k = ~(u64)i;
    if (k > s.key[rule]) s.key[rule] = k;
    s.cnt[rule]++;
  };
  const int64_t H = c.H, T = c.T, Z = c.Z;
  for (int64_t h = 0; h < H; h++)
    if (chk_bad_index(c.zone[h], c.Z)) hit(PVT_CHK_ZONE, h);
  for (int64_t i = 0; i < 4 * H; i++)
    if (chk_bad_amount(c.avail[i])) hit(PVT_CHK_AVAIL, i);
  if (c.dem)
    for (int64_t i = 0; i < 4 * T; i++)
      if (chk_bad_amount(c.dem[i])) hit(PVT_CHK_DEM, i);
  if (c.task_group)
    for (int64_t t = 0; t < T; t++)
      if (chk_bad_index(c.task_group[t], c.G)) hit(PVT_CHK_GROUP, t);
  if (c.group_anchor)
    for (int64_t g = 0; g < c.G; g++)
      if (chk_bad_index(c.group_anchor[g], c.Z)) hit(PVT_CHK_ANCHOR, g);
  if (c.cost && c.bw)
    for (int64_t i = 0; i < Z * Z; i++) {
      const int64_t j = (i % Z) * Z + i / Z;
      if (chk_bad_cost_sum(c.cost[i] + c.cost[j])) hit(PVT_CHK_COST, i);
      if (chk_bad_bw_sum(c.bw[i] + c.bw[j])) hit(PVT_CHK_BW, i);
    }
  if (c.rt_bw)
    for (int64_t i = 0; i < c.n_rt; i++)
      if (chk_bad_rt_bw(c.rt_bw[i])) hit(PVT_CHK_RTBW, i);
  if (c.decay)
    for (int64_t h = 0; h < H; h++)
      if (chk_bad_decay(c.decay[h])) hit(PVT_CHK_DECAY, h);
  if (c.tiebreak) {
    std::vector<uint32_t> owner((size_t)H, 0xffffffffu);
    for (int64_t h = 0; h < H; h++) {
      const uint32_t rank = c.tiebreak[h];
      if (!chk_bad_rank(rank, c.H)) owner[rank] = std::min(owner[rank], (uint32_t)h);
    }
    for (int64_t h = 0; h < H; h++) {
      const uint32_t rank = c.tiebreak[h];
      if (chk_bad_rank(rank, c.H) || owner[rank] != (uint32_t)h) hit(PVT_CHK_TIEBREAK, h);
    }
  }
  chk_report(c, s, out);
}

}  // namespace pvt
