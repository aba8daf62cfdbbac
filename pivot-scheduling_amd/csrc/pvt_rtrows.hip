// pvt_rtrows.hip — the realtime-bandwidth rows of a cost_aware round (pvt_round.rt_bw), built in
// HBM from the zone table and a sparse list of route queues (the contract is in
// include/pivot_place.h at pvt_route_queues; pivot_place/routes.py states the rule in Python).
//
// A route's realtime bandwidth (reference resources/network.py:70-73) is
//   est = (Q + 1) / bw;  est ? 1 / est : bw
// with Q the sum of the queued packets' MB, left to right in queue order, from 0. Row g of rt_bw
// holds, per host h, in + out of the two routes between g's anchor storage and h
// (scheduler/cost_aware.py:73-79,106-112). A route that is not listed is idle on the zone table's
// bandwidth, so its value depends on the zone pair alone -- but it is not the table's entry: both
// divisions are performed (1 / (1 / b) != b for about one b in nine).
//   check   a thread per entry (and its packets), per group anchor and per host zone tests the
//           contract; the first offender of each kind goes to bad[] by an integer atomic minimum.
//           Every later pass leaves before any store when a word of bad[] is set, so an invalid
//           call writes nothing and the verdict needs no synchronisation between the passes.
//   value   a thread per entry: the sequential sum of its packets, then the two divisions, to a
//           scratch array. Queues are a few packets long; a long one costs latency only.
//   fill    the hot pass. A workgroup takes a tile of RT_TILE hosts and up to RT_GROUPS rows. It
//           builds in LDS one idle table per distinct anchor among its rows,
//           idle[z] = f(bw[a][z]) + f(bw[z][a]) with f the value of an empty queue (the same
//           device function as in the value pass), then per lane reads four zones with one 16-B
//           load, gathers the four sums from LDS and stores them with two 16-B stores per row. A
//           row starts at byte g*H*8, 16-byte aligned only when g*H is even: a lane whose four
//           elements start on an odd double stores 8 + 16 + 8 bytes instead, and the last hosts of
//           an H that is no multiple of four are stored one by one.
//           Bytes moved: rows*H*8 written and H*4 read per chunk of rows, that is
//           G*H*8 + ceil(G / RT_GROUPS)*H*4 (the re-reads of zone after the first are served by
//           L2 / Infinity Cache; the Z*Z table is read from L2 by every workgroup and not counted).
//   patch   a thread per entry, after the fill: the first listed direction of a (anchor, host)
//           pair takes in and out from the scratch values where listed and from the table where
//           not, and stores in + out to every row anchored at that zone.
// Plain loads and stores, IEEE divisions, no contraction, no floating-point atomics, no MFMA: the
// rows are bit-identical on every call.
#include <hip/hip_runtime.h>

#include "pvt_kernels.h"
#include "pvt_rtrows.h"

namespace pvt {

namespace {

// network.py:72-73 with Q = s. A NaN est is true in Python and takes the division.
__device__ __forceinline__ double rt_value(double s, double bw) {
  const double est = (s + 1.0) / bw;
  return est != 0.0 ? 1.0 / est : bw;
}

__device__ __forceinline__ bool rt_is_bad(const uint32_t* bad) {
  return (bad[0] & bad[1] & bad[2]) != RT_NO_BAD;
}

__global__ void __launch_bounds__(RT_THREADS) rt_check_kernel(RtRowsArgs a) {
  const int64_t i = (int64_t)blockIdx.x * RT_THREADS + threadIdx.x;
  if (i < a.R) {
    const int32_t an = a.rq_anchor[i], h = a.rq_host[i], d = a.rq_dir[i];
    bool ok = an >= 0 && an < a.Z && h >= 0 && h < a.H && (d == 0 || d == 1);
    if (i > 0) {   // keys strictly ascending
      const int32_t pa = a.rq_anchor[i - 1], ph = a.rq_host[i - 1], pd = a.rq_dir[i - 1];
      ok &= pa < an || (pa == an && (ph < h || (ph == h && pd < d)));
    }
    ok &= a.rq_bw[i] > 0.0;   // (false for NaN)
    const int64_t lo = a.rq_off[i], hi = a.rq_off[i + 1];
    bool range = lo >= 0 && lo <= hi && hi <= a.P;
    if (i == 0) range &= lo == 0;
    if (i == a.R - 1) range &= hi == a.P;
    ok &= range;
    if (range)
      for (int64_t p = lo; p < hi; ++p) ok &= a.rq_mbs[p] > 0.0;
    if (!ok) atomicMin(a.bad + 0, (uint32_t)i);
  }
  if (i < a.G) {
    const int32_t an = a.group_anchor[i];
    if (an < 0 || an >= a.Z) atomicMin(a.bad + 1, (uint32_t)i);
  }
  if (i < a.H) {
    const int32_t z = a.zone[i];
    if (z < 0 || z >= a.Z) atomicMin(a.bad + 2, (uint32_t)i);
  }
}

__global__ void __launch_bounds__(RT_THREADS) rt_value_kernel(RtRowsArgs a) {
  if (rt_is_bad(a.bad)) return;
  const int64_t i = (int64_t)blockIdx.x * RT_THREADS + threadIdx.x;
  if (i >= a.R) return;
  double s = 0.0;
  for (int64_t p = a.rq_off[i], hi = a.rq_off[i + 1]; p < hi; ++p) s = s + a.rq_mbs[p];
  a.val[i] = rt_value(s, a.rq_bw[i]);
}

__device__ __forceinline__ bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

__global__ void __launch_bounds__(RT_THREADS) rt_fill_kernel(RtRowsArgs a, int gc) {
  extern __shared__ double idle[];            // [ng][Z], the tables of the chunk's distinct anchors
  __shared__ int32_t anc[RT_GROUPS], tab[RT_GROUPS];
  if (rt_is_bad(a.bad)) return;
  const int tid = threadIdx.x;
  const int Z = a.Z;
  const int64_t H = a.H;
  const int rows = a.G > 0 ? a.G : 1;
  const int g0 = blockIdx.y * gc;
  const int ng = min(gc, rows - g0);
  if (tid < ng) anc[tid] = a.G > 0 ? a.group_anchor[g0 + tid] : 0;
  __syncthreads();
  if (tid < ng) {                             // the first row of the chunk with this anchor
    int s = tid;
    for (int j = tid - 1; j >= 0; --j)
      if (anc[j] == anc[tid]) s = j;
    tab[tid] = s;
  }
  __syncthreads();
  for (int i = tid; i < ng * Z; i += RT_THREADS) {
    const int s = i / Z, z = i - s * Z;
    if (tab[s] != s) continue;
    const int64_t an = anc[s];
    idle[i] = rt_value(0.0, a.bw[an * Z + z]) + rt_value(0.0, a.bw[(int64_t)z * Z + an]);
  }
  __syncthreads();
  const bool zal = aligned16(a.zone);
  const int64_t hbase = (int64_t)blockIdx.x * RT_TILE;
#pragma unroll
  for (int it = 0; it < RT_TILE / (4 * RT_THREADS); ++it) {
    const int64_t h = hbase + ((int64_t)it * RT_THREADS + tid) * 4;
    if (h >= H) return;
    if (h + 4 <= H) {
      int4 z;
      if (zal) {
        z = *reinterpret_cast<const int4*>(a.zone + h);
      } else {
        z.x = a.zone[h]; z.y = a.zone[h + 1]; z.z = a.zone[h + 2]; z.w = a.zone[h + 3];
      }
      for (int g = 0; g < ng; ++g) {
        const double* t = idle + tab[g] * Z;
        const double v0 = t[z.x], v1 = t[z.y], v2 = t[z.z], v3 = t[z.w];
        double* p = a.rt_bw + (int64_t)(g0 + g) * H + h;
        if (aligned16(p)) {
          *reinterpret_cast<double2*>(p) = make_double2(v0, v1);
          *reinterpret_cast<double2*>(p + 2) = make_double2(v2, v3);
        } else {                              // the row starts on an odd double
          p[0] = v0;
          *reinterpret_cast<double2*>(p + 1) = make_double2(v1, v2);
          p[3] = v3;
        }
      }
    } else {                                  // the last one to three hosts
      for (int64_t k = h; k < H; ++k) {
        const int32_t z = a.zone[k];
        for (int g = 0; g < ng; ++g) a.rt_bw[(int64_t)(g0 + g) * H + k] = idle[tab[g] * Z + z];
      }
    }
  }
}

__global__ void __launch_bounds__(RT_THREADS) rt_patch_kernel(RtRowsArgs a) {
  if (rt_is_bad(a.bad)) return;
  const int64_t i = (int64_t)blockIdx.x * RT_THREADS + threadIdx.x;
  if (i >= a.R) return;
  const int32_t an = a.rq_anchor[i], h = a.rq_host[i], d = a.rq_dir[i];
  // keys ascend strictly, so a predecessor on the same pair is its dir 0 and handles both
  if (i > 0 && a.rq_anchor[i - 1] == an && a.rq_host[i - 1] == h) return;
  const int64_t Z = a.Z, H = a.H;
  const int64_t z = a.zone[h];
  double in, out;
  if (d == 0) {
    in = a.val[i];
    const bool partner = i + 1 < a.R && a.rq_anchor[i + 1] == an && a.rq_host[i + 1] == h;
    out = partner ? a.val[i + 1] : rt_value(0.0, a.bw[z * Z + an]);
  } else {
    in = rt_value(0.0, a.bw[an * Z + z]);
    out = a.val[i];
  }
  const double v = in + out;
  if (a.G <= 0) {
    if (an == 0) a.rt_bw[h] = v;
    return;
  }
  for (int g = 0; g < a.G; ++g)
    if (a.group_anchor[g] == an) a.rt_bw[(int64_t)g * H + h] = v;
}

uint32_t rt_blocks(int64_t n) { return (uint32_t)((n + RT_THREADS - 1) / RT_THREADS); }

}  // namespace

int rtrows_chunk(int32_t rows) {
  const int chunks = (rows + RT_GROUPS - 1) / RT_GROUPS;
  return (rows + chunks - 1) / chunks;
}

double rtrows_fill_bytes(const RtRowsArgs& a) {
  const int rows = a.G > 0 ? a.G : 1;
  const int chunks = (rows + RT_GROUPS - 1) / RT_GROUPS;
  return 8.0 * (double)rows * (double)a.H + 4.0 * (double)chunks * (double)a.H;
}

// Only the fill has a profiling scope (pvt_capi.hip), so only it starts through PVT_LAUNCH, which
// binds the scope's events to the dispatch; the three small passes are plain launches.
void launch_rt_check(const RtRowsArgs& a, hipStream_t st) {
  int64_t n = a.H;
  if (a.R > n) n = a.R;
  if (a.G > n) n = a.G;
  hipLaunchKernelGGL(rt_check_kernel, dim3(rt_blocks(n)), dim3(RT_THREADS), 0, st, a);
}

void launch_rt_value(const RtRowsArgs& a, hipStream_t st) {
  if (a.R <= 0) return;
  hipLaunchKernelGGL(rt_value_kernel, dim3(rt_blocks(a.R)), dim3(RT_THREADS), 0, st, a);
}

void launch_rt_fill(const RtRowsArgs& a, hipStream_t st) {
  const int rows = a.G > 0 ? a.G : 1;
  const int gc = rtrows_chunk(rows);
  const uint32_t tiles = (uint32_t)(((int64_t)a.H + RT_TILE - 1) / RT_TILE);
  const uint32_t chunks = (uint32_t)((rows + gc - 1) / gc);
  const size_t lds = (size_t)gc * (size_t)a.Z * sizeof(double);
  PVT_LAUNCH(rt_fill_kernel, dim3(tiles, chunks), dim3(RT_THREADS), lds, st, a, gc);
}

void launch_rt_patch(const RtRowsArgs& a, hipStream_t st) {
  if (a.R <= 0) return;
  hipLaunchKernelGGL(rt_patch_kernel, dim3(rt_blocks(a.R)), dim3(RT_THREADS), 0, st, a);
}

}  // namespace pvt
