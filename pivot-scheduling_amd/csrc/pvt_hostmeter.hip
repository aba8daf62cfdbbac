// pvt_hostmeter.hip — the reference meter's host half (Meter.host_check_in / host_check_out,
// resources/meter.py:59-81, and _track_resource_usage, :181-187) run from the resident op log;
// the contract is in include/pivot_place.h at pvt_host_meter.
//
// A check-in or check-out is one more kind of entry in the log of pvt_hostops.hip, and the
// per-host segment walk has the host's levels and capacities in registers at that point of the
// log. So the apply is that file's three passes with a wider walk:
//   keys    as there, and the entry's time (finite, in range, not below its predecessor's or the
//           previous call's last) and its host's capacities (> 0: a mark divides by them).
//   sort    the same stable radix sort by host.
//   walk    the head of a host's segment walks it alone, with the host's meter state (word,
//           start, end) in registers beside the levels. A mark appends one usage record -- four
//           times one fp64 subtraction and one division -- and runs the state machine; a check-in
//           that opens an interval after a closed one appends the closed one to the interval log.
//           Slots in the two append logs come from integer atomics on two device counters: one
//           thread owns a host, so a host's records take increasing slots in its log order, within
//           a call and across calls. Records of different hosts interleave as the hardware
//           schedules them; the finish orders them, so nothing the caller sees depends on that.
// finish    sorts each log's records by host (stable, over the bits that vary), the closed last
//           interval of every host appended behind the interval log's own, and gathers: a host's
//           records keep their log order, so the arrays are the same from run to run and however
//           the log was cut into calls. Rows are the distinct hosts of the sorted usage keys.
// No floating-point atomics, no LDS, no MFMA; host_ops_kernel is untouched (two kernels, not a
// template over it).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "pvt_kernels.h"
#include "pvt_hostmeter.h"

namespace pvt {

namespace {

constexpr double HM_TIME_LIMIT = 4503599627370496.0;   // 2^52

__global__ void __launch_bounds__(HO_THREADS) host_meter_keys_kernel(HostMeterArgs a) {
  const int64_t k = (int64_t)blockIdx.x * HO_THREADS + threadIdx.x;
  if (k >= a.K) return;
  const int32_t h = a.op_host[k];
  const int32_t kind = a.op_kind[k];
  const double t = a.op_time[k];
  const double prev = k > 0 ? a.op_time[k - 1] : a.last_time;
  bool ok = h >= 0 && h < a.H && kind >= 0 && kind <= HM_CHECK_OUT;
  ok = ok && t >= 0.0 && t < HM_TIME_LIMIT && t >= prev;   // (a NaN fails every compare)
  if (ok) {
#pragma unroll
    for (int r = 0; r < 4; ++r) ok = ok && a.capacity[(int64_t)r * a.H + h] > 0.0;
  }
  if (!ok) atomicMin(a.bad, (uint32_t)k);
  a.key_in[k] = ok ? (uint32_t)h : 0u;
  a.idx_in[k] = (int32_t)k;
}

// (the two ops: pvt_hostops.hip's, word for word)
__device__ __forceinline__ int32_t subscribe(double (&l)[4], const double (&d)[4]) {
  bool refuse = false;
#pragma unroll
  for (int r = 0; r < 4; ++r) refuse |= (d[r] > l[r]) | (d[r] < 0.0);
  if (refuse) return 0;
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if (d[r] > 0.0) l[r] = l[r] - d[r];
  return 1;
}

__device__ __forceinline__ int32_t unsubscribe(double (&l)[4], const double (&c)[4],
                                               const double (&d)[4]) {
  int32_t mask = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const double used = c[r] - l[r];
    if (0.0 < d[r] && d[r] <= used) {
      l[r] = l[r] + d[r];
      mask |= 1 << r;
    }
  }
  return mask;
}

__global__ void __launch_bounds__(HO_THREADS) host_meter_kernel(HostMeterArgs a) {
  if (*a.bad != HO_NO_BAD) return;
  const int64_t i = (int64_t)blockIdx.x * HO_THREADS + threadIdx.x;
  if (i >= a.K) return;
  const uint32_t h = a.key_out[i];
  if (i > 0 && a.key_out[i - 1] == h) return;   // not the head of a segment
  const int64_t H = a.H, K = a.K;
  double l[4], c[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    l[r] = a.level[r * H + h];
    c[r] = a.capacity[r * H + h];
  }
  int32_t w = a.st_word[h];
  double s = a.st_start[h], e = a.st_end[h];
  for (int64_t j = i; j < K && a.key_out[j] == h; ++j) {
    const int64_t k = a.idx_out[j];
    const int32_t kind = a.op_kind[k];
    if (kind < HM_CHECK_IN) {
      double d[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) d[r] = a.op_amt[r * K + k];
      a.op_ok[k] = kind == 0 ? subscribe(l, d) : unsubscribe(l, c, d);
      continue;
    }
    const double t = a.op_time[k];
    const unsigned long long u = atomicAdd(a.cnt + 1, 1ull);   // (below us_cap: the caller's check)
    a.us_host[u] = (int32_t)h;
    a.us_time[u] = t;
#pragma unroll
    for (int r = 0; r < 4; ++r) a.us_frac[4 * u + r] = (c[r] - l[r]) / c[r];
    int32_t code;
    if (kind == HM_CHECK_IN) {
      if (w == HM_NONE) {
        w = HM_OPEN; s = t; e = 0.0; code = 1;
      } else if (w == HM_CLOSED) {
        if (t > e) {                  // the closed interval is final
          const unsigned long long v = atomicAdd(a.cnt, 1ull);
          a.iv_host[v] = (int32_t)h;
          a.iv_start[v] = s;
          a.iv_end[v] = e;
          s = t; code = 2;
        } else {
          code = 3;                   // the reference pops the end: open(start) again
        }
        w = HM_OPEN; e = 0.0;
      } else {
        code = 4;
      }
    } else {
      if (w == HM_OPEN) {
        w = HM_CLOSED; e = t; code = 1;
      } else if (w == HM_CLOSED) {
        if (t > e) { e = t; code = 2; } else { code = 3; }
      } else {
        code = 0;                     // (the reference raises here, after the record)
      }
    }
    a.op_ok[k] = code;
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) a.level[r * H + h] = l[r];
  a.st_word[h] = w;
  a.st_start[h] = s;
  a.st_end[h] = e;
}

// ------------------------------------------------------------------------------- finish
__device__ __forceinline__ uint32_t host_key(int32_t h, int32_t H) {
  return (uint32_t)h < (uint32_t)H ? (uint32_t)h : (uint32_t)(H - 1);   // (a caller's log: clamped)
}

// a thread per logged interval and per host
__global__ void __launch_bounds__(HO_THREADS) host_meter_tail_kernel(HostMeterFinish f) {
  const int64_t i = (int64_t)blockIdx.x * HO_THREADS + threadIdx.x;
  if (i < f.n_iv) {
    f.ivk_in[i] = host_key(f.iv_host[i], f.H);
    f.ivi_in[i] = (int32_t)i;
  }
  if (i >= f.H) return;
  const int32_t w = f.st_word[i];
  if (w == HM_OPEN) {
    atomicAdd(f.words + 0, 1u);
    atomicMin(f.words + 1, (uint32_t)i);
  } else if (w == HM_CLOSED) {        // (at most H of them: the scratch holds n_iv + H)
    const uint32_t v = atomicAdd(f.words + 2, 1u);
    f.ivk_in[(int64_t)f.n_iv + v] = (uint32_t)i;
    f.ivi_in[(int64_t)f.n_iv + v] = f.n_iv;    // any index >= n_iv: read from the host's state
  }
}

__global__ void __launch_bounds__(HO_THREADS) host_meter_iv_gather_kernel(HostMeterFinish f) {
  const int64_t j = (int64_t)blockIdx.x * HO_THREADS + threadIdx.x;
  if (j >= f.n_ivf) return;
  const int32_t src = f.ivi_out[j];
  const uint32_t h = f.ivk_out[j];
  f.o_iv_start[j] = src < f.n_iv ? f.iv_start[src] : f.st_start[h];
  f.o_iv_end[j] = src < f.n_iv ? f.iv_end[src] : f.st_end[h];
}

__global__ void __launch_bounds__(HO_THREADS) host_meter_us_keys_kernel(HostMeterFinish f) {
  const int64_t u = (int64_t)blockIdx.x * HO_THREADS + threadIdx.x;
  if (u >= f.n_us) return;
  f.usk_in[u] = host_key(f.us_host[u], f.H);
  f.usi_in[u] = (int32_t)u;
}

__global__ void __launch_bounds__(HO_THREADS) host_meter_heads_kernel(HostMeterFinish f) {
  const int64_t u = (int64_t)blockIdx.x * HO_THREADS + threadIdx.x;
  if (u >= f.n_us) return;
  f.head[u] = (u == 0 || f.usk_out[u] != f.usk_out[u - 1]) ? 1 : 0;
}

// a thread per sorted usage record: the gather (transposed to resource-major), and at the first
// record of a host its row (at most min(H, n_us) rows: the keys are hosts below H)
__global__ void __launch_bounds__(HO_THREADS) host_meter_rows_kernel(HostMeterFinish f) {
  const int64_t u = (int64_t)blockIdx.x * HO_THREADS + threadIdx.x;
  const int64_t n = f.n_us;
  if (u >= n) return;
  const int64_t src = f.usi_out[u];
  f.o_us_time[u] = f.us_time[src];
#pragma unroll
  for (int r = 0; r < 4; ++r) f.o_us_frac[r * n + u] = f.us_frac[4 * src + r];
  const uint32_t h = f.usk_out[u];
  const int32_t row = f.row[u], head = f.head[u];
  if (head) {
    int64_t lo = 0, hi = f.n_ivf;     // the first interval whose host is not below h
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (f.ivk_out[mid] < h) lo = mid + 1; else hi = mid;
    }
    f.o_row_host[row] = (int32_t)h;
    f.o_us_off[row] = u;
    f.o_iv_off[row] = lo;
  }
  if (u == n - 1) {
    const int32_t R = row + head;
    f.words[3] = (uint32_t)R;
    f.o_us_off[R] = n;
    f.o_iv_off[R] = f.n_ivf;
  }
}

uint32_t blocks(int64_t n) { return (uint32_t)((n + HO_THREADS - 1) / HO_THREADS); }

}  // namespace

void launch_hostmeter_keys(const HostMeterArgs& a, hipStream_t st) {
  if (a.K <= 0) return;
  hipLaunchKernelGGL(host_meter_keys_kernel, dim3(blocks(a.K)), dim3(HO_THREADS), 0, st, a);
}

hipError_t hostmeter_sort(int32_t H, int32_t n, const uint32_t* key_in, uint32_t* key_out,
                          const int32_t* idx_in, int32_t* idx_out, void* tmp, size_t tmp_bytes,
                          hipStream_t st) {
  return hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, key_in, key_out, idx_in, idx_out, n, 0,
                                            hostops_key_bits(H), st);
}

void launch_hostmeter_apply(const HostMeterArgs& a, hipStream_t st) {
  if (a.K <= 0) return;
  PVT_LAUNCH(host_meter_kernel, dim3(blocks(a.K)), dim3(HO_THREADS), 0, st, a);
}

void launch_hostmeter_tail(const HostMeterFinish& f, hipStream_t st) {
  const int64_t n = f.n_iv > f.H ? f.n_iv : f.H;
  hipLaunchKernelGGL(host_meter_tail_kernel, dim3(blocks(n)), dim3(HO_THREADS), 0, st, f);
}

void launch_hostmeter_iv_gather(const HostMeterFinish& f, hipStream_t st) {
  if (f.n_ivf <= 0) return;
  hipLaunchKernelGGL(host_meter_iv_gather_kernel, dim3(blocks(f.n_ivf)), dim3(HO_THREADS), 0, st, f);
}

void launch_hostmeter_us_keys(const HostMeterFinish& f, hipStream_t st) {
  if (f.n_us <= 0) return;
  hipLaunchKernelGGL(host_meter_us_keys_kernel, dim3(blocks(f.n_us)), dim3(HO_THREADS), 0, st, f);
}

void launch_hostmeter_heads(const HostMeterFinish& f, hipStream_t st) {
  if (f.n_us <= 0) return;
  hipLaunchKernelGGL(host_meter_heads_kernel, dim3(blocks(f.n_us)), dim3(HO_THREADS), 0, st, f);
}

hipError_t hostmeter_scan_temp(int32_t n, size_t* bytes) {
  *bytes = 0;
  return hipcub::DeviceScan::ExclusiveSum(nullptr, *bytes, (const int32_t*)nullptr,
                                          (int32_t*)nullptr, n);
}

hipError_t hostmeter_scan(const HostMeterFinish& f, void* tmp, size_t tmp_bytes, hipStream_t st) {
  return hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, (const int32_t*)f.head, f.row, f.n_us, st);
}

void launch_hostmeter_rows(const HostMeterFinish& f, hipStream_t st) {
  if (f.n_us <= 0) return;
  hipLaunchKernelGGL(host_meter_rows_kernel, dim3(blocks(f.n_us)), dim3(HO_THREADS), 0, st, f);
}

}  // namespace pvt
