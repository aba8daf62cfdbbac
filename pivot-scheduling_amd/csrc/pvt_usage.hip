// pvt_usage.hip — Meter usage series of a batch of scenarios: hosts in use and mean utilisation
// per time bucket (reference resources/meter.py:135-179, the half of the meter that
// pvt_meter.hip leaves; Meter.save writes the host series on every run, :128-133).
//
// With s = sample_size, bucket b is [b*s, (b+1)*s). One 256-thread workgroup per scenario:
//   checks          a thread per host row checks its offsets; non-decreasing offsets make the
//                   scenario's rows tile one range of the interval and of the record arrays, so
//                   both are then walked flat and coalesced, a thread per element: the times are
//                   checked alone, the order against the element in front -- an element that
//                   comes before its predecessor must be the first of a row (a binary search of
//                   the offsets, taken only there).
//   host series     the thread of an interval adds +1 at floor(start)/s and -1 at floor(end)/s
//                   into the scenario's int32 output row (the reference counts buckets
//                   start//s .. end//s - 1: the bucket that holds `end` is not counted, an
//                   interval inside one bucket counts nowhere); the block then turns the row into
//                   counts with an inclusive scan, 256 buckets at a time with a carry. A host's
//                   intervals are ordered and disjoint (checked), so its bucket ranges are too and
//                   every host counts once per bucket, as in the reference's sets. Integer
//                   atomics: the order of the adds cannot show.
//   resource series a wave per bucket, lanes over the host rows 64 at a time; a lane finds its
//                   host's first record of the bucket by binary search on the time-ordered
//                   records, folds the four fractions of the run in record order and divides by
//                   the run length; the wave adds the lanes in a fixed shuffle tree, host chunks
//                   in order. No floating-point atomics anywhere.
//   averages        mean over the non-empty buckets: the host one as an integer sum and one
//                   division (exact), the resource ones per wave in bucket order, waves in order.
// All divisions of times are int64: for an integral s and 0 <= t < 2^52, floor(floor(t)/s) is
// Python's float t // s. A latency-bound streaming reduction (the work of one scenario is small;
// a batch fills the device with independent workgroups), no MFMA.
#include <hip/hip_runtime.h>

#include "pvt_device.h"
#include "pvt_usage.h"

namespace pvt {

namespace {

constexpr int USE_WAVES = USE_THREADS / 64;

__device__ __forceinline__ bool span_ok(gptr<const int64_t> off, int64_t i, int64_t n,
                                        int64_t* lo, int64_t* hi) {
  *lo = off[i];
  *hi = off[i + 1];
  return *lo >= 0 && *hi >= *lo && *hi <= n;
}

__device__ __forceinline__ bool time_ok(double t) {   // false for NaN
  return t >= 0.0 && t < (double)USE_TIME_END;
}

__device__ __forceinline__ int64_t block_sum_i64(int64_t v, int64_t* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  int64_t s = red[0];
#pragma unroll
  for (int w = 1; w < USE_WAVES; ++w) s += red[w];
  return s;
}

// first record of [lo, hi) with time >= thr (the records are time-ordered)
__device__ __forceinline__ int64_t first_at(gptr<const double> t, int64_t lo, int64_t hi,
                                            double thr) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (t[mid] < thr) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// does a row of off[h0 .. h1] (non-decreasing) begin at element i?
__device__ __forceinline__ bool row_start(gptr<const int64_t> off, int64_t h0, int64_t h1,
                                          int64_t i) {
  while (h0 < h1) {
    const int64_t mid = h0 + ((h1 - h0) >> 1);
    if (off[mid] < i) h0 = mid + 1; else h1 = mid;
  }
  return off[h0] == i;
}

}  // namespace

__global__ void __launch_bounds__(USE_THREADS) usage_kernel(UsageArgs a) {
  __shared__ int32_t wtot[USE_WAVES];
  __shared__ int64_t red[USE_WAVES];
  __shared__ double wsum[USE_WAVES][4];
  __shared__ int64_t wcnt[USE_WAVES];
  const int s = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t ss = a.sample_size;
  const auto host_off = G(a.host_off), iv_off = G(a.iv_off), us_off = G(a.us_off);
  const auto bucket_off = G(a.bucket_off);
  const auto iv_start = G(a.iv_start), iv_end = G(a.iv_end), us_time = G(a.us_time);
  const auto us_frac = G(a.us_frac);
  const auto n_hosts = G(a.n_hosts), res_hosts = G(a.res_hosts);
  const auto res_mean = G(a.res_mean), avg = G(a.avg);
  const bool has_us = a.us_off != nullptr;

  // the scenario's host rows and output row; the same in every thread
  int64_t h0, h1, b0, b1;
  bool ok = span_ok(host_off, s, a.n_host_rows, &h0, &h1);
  ok = span_ok(bucket_off, s, a.n_buckets, &b0, &b1) && ok;
  ok = ok && bucket_off[a.n_scen] == a.n_buckets;
  const int64_t nb = b1 - b0;
  // every bucket start is a time below 2^52 (so b * s is exact in a double)
  ok = ok && (nb == 0 || nb - 1 <= (USE_TIME_END - 1) / ss);
  if (!ok) {
    if (tid == 0) __hip_atomic_fetch_add(G(a.bad), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  // only this workgroup touches the row: workgroup scope for its fences, adds and loads
  const auto row = n_hosts + b0;
  for (int64_t b = tid; b < nb; b += USE_THREADS) row[b] = 0;
  __threadfence_block();
  __syncthreads();

  // every host row's offsets; non-decreasing offsets make the rows of the scenario tile
  // [off[h0], off[h1]), so the intervals and the records can be walked flat
  for (int64_t h = h0 + tid; h < h1; h += USE_THREADS) {
    int64_t lo, hi;
    ok = span_ok(iv_off, h, a.n_iv, &lo, &hi) && ok;
    if (has_us) ok = span_ok(us_off, h, a.n_us, &lo, &hi) && ok;
  }
  if (__syncthreads_or(!ok)) {
    if (tid == 0) __hip_atomic_fetch_add(G(a.bad), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }

  // difference row of the host series: a thread per interval. An interval that starts before
  // the one in front of it ends must be the first of its host.
  const int64_t v0 = iv_off[h0], v1 = iv_off[h1];
  for (int64_t v = v0 + tid; v < v1; v += USE_THREADS) {
    const double st = iv_start[v], en = iv_end[v];
    if (!time_ok(st) || !time_ok(en) || en < st) { ok = false; continue; }
    if (v > v0 && st < iv_end[v - 1] && !row_start(iv_off, h0, h1, v)) ok = false;
    const int64_t lo = (int64_t)st / ss, e = (int64_t)en / ss;
    if (e >= nb) { ok = false; continue; }
    if (e > lo) {
      __hip_atomic_fetch_add(row + lo, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      __hip_atomic_fetch_add(row + e, -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
  }
  // the records: a thread per record; bucket < nb is t < nb * s
  const int64_t r0 = has_us ? us_off[h0] : 0, r1 = has_us ? us_off[h1] : 0;
  const double t_end = (double)(nb * ss);
  for (int64_t u = r0 + tid; u < r1; u += USE_THREADS) {
    const double t = us_time[u];
    if (!time_ok(t) || !(t < t_end)) { ok = false; continue; }
    if (u > r0 && t < us_time[u - 1] && !row_start(us_off, h0, h1, u)) ok = false;
  }
  __threadfence_block();
  if (__syncthreads_or(!ok)) {
    if (tid == 0) __hip_atomic_fetch_add(G(a.bad), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }

  // inclusive scan of the difference row, 256 buckets at a time
  int32_t carry = 0;
  int64_t hsum = 0, hcnt = 0;
  for (int64_t c = 0; c < nb; c += USE_THREADS) {
    const int64_t b = c + tid;
    int32_t v = b < nb ? __hip_atomic_load(row + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
                       : 0;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int32_t t = __shfl_up(v, o, 64);
      if (lane >= o) v += t;
    }
    if (lane == 63) wtot[wave] = v;
    __syncthreads();
    int32_t pre = carry, tot = 0;
#pragma unroll
    for (int w = 0; w < USE_WAVES; ++w) {
      if (w < wave) pre += wtot[w];
      tot += wtot[w];
    }
    v += pre;
    carry += tot;
    if (b < nb) {
      row[b] = v;
      hsum += v;
      hcnt += v != 0;
    }
    __syncthreads();
  }
  hsum = block_sum_i64(hsum, red);
  hcnt = block_sum_i64(hcnt, red);
  if (tid == 0) avg[(int64_t)s * 5] = hcnt ? (double)hsum / (double)hcnt : __builtin_nan("");
  if (!has_us) return;

  // resource series: a wave per bucket
  double asum[4] = {0.0, 0.0, 0.0, 0.0};
  int64_t acnt = 0;
  for (int64_t b = wave; b < nb; b += USE_WAVES) {
    const double t_lo = (double)(b * ss), t_hi = (double)((b + 1) * ss);
    double m[4] = {0.0, 0.0, 0.0, 0.0};
    int32_t nh = 0;
    for (int64_t hc = h0; hc < h1; hc += 64) {
      const int64_t h = hc + lane;
      double p[4] = {0.0, 0.0, 0.0, 0.0};
      int32_t in = 0;
      if (h < h1) {
        const int64_t u1 = us_off[h + 1];
        const int64_t lo = first_at(us_time, us_off[h], u1, t_lo);
        int64_t u = lo;
        for (; u < u1 && us_time[u] < t_hi; ++u) {
#pragma unroll
          for (int r = 0; r < 4; ++r) p[r] += us_frac[r * a.n_us + u];
        }
        if (u > lo) {
          in = 1;
          const double n = (double)(u - lo);
#pragma unroll
          for (int r = 0; r < 4; ++r) p[r] /= n;
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int r = 0; r < 4; ++r) p[r] += __shfl_xor(p[r], o, 64);
        in += __shfl_xor(in, o, 64);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) m[r] += p[r];
      nh += in;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      m[r] = nh ? m[r] / (double)nh : 0.0;
      asum[r] += m[r];
    }
    acnt += nh != 0;
    if (lane == 0) {
      res_hosts[b0 + b] = nh;
#pragma unroll
      for (int r = 0; r < 4; ++r) res_mean[r * a.n_buckets + b0 + b] = m[r];
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) wsum[wave][r] = asum[r];
    wcnt[wave] = acnt;
  }
  __syncthreads();
  if (tid < 4) {
    double t = 0.0;
    int64_t n = 0;
#pragma unroll
    for (int w = 0; w < USE_WAVES; ++w) {
      t += wsum[w][tid];
      n += wcnt[w];
    }
    avg[(int64_t)s * 5 + 1 + tid] = n ? t / (double)n : __builtin_nan("");
  }
}

void launch_usage(const UsageArgs& a, hipStream_t st) {
  if (a.n_scen <= 0) return;
  usage_kernel<<<a.n_scen, USE_THREADS, 0, st>>>(a);
}

}  // namespace pvt
