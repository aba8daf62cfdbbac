// pvt_hostops.hip — a log of subscribe / unsubscribe ops applied to host levels that stay on
// the device between rounds (reference HostResource.subscribe / unsubscribe,
// resources/__init__.py:433-461, over SimPy containers; the contract is in include/pivot_place.h
// at pvt_host_ops).
//
// The ops of one host must be applied in log order, each with the reference's own compares and
// one rounding per add or subtract: a put-back that misses `d <= capacity - level` by an ulp is
// skipped and shapes every later op of that host. Ops of different hosts are independent. So:
//   keys    a thread per op writes the pair (host, k) and checks the host's range and the kind;
//           the first invalid op goes to *bad by an integer atomic minimum.
//   sort    hipCUB's radix sort of the pairs by host over the ceil(log2 H) bits that vary. It is
//           stable, so a host's ops keep their log order.
//   walk    a thread per sorted position; the thread at the head of a host's segment (its
//           predecessor's key differs) walks the segment alone: the host's four levels and
//           capacities in registers, the op's kind and amounts gathered through the permutation,
//           op_ok stored per op, the levels stored once at the end. It leaves before any store
//           when *bad is set, so an invalid log writes nothing and the verdict needs no
//           synchronisation between the passes.
// No floating-point atomics, no reduction: a level is a chain of fp64 adds in log order, equal on
// every call and however the log is cut into calls. Segments are short (a host holds a few dozen
// tasks at the most); a long one costs latency only. Plain loads and stores, no LDS, no MFMA.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "pvt_kernels.h"
#include "pvt_hostops.h"

namespace pvt {

namespace {

__global__ void __launch_bounds__(HO_THREADS) host_ops_keys_kernel(HostOpsArgs a) {
  const int64_t k = (int64_t)blockIdx.x * HO_THREADS + threadIdx.x;
  if (k >= a.K) return;
  const int32_t h = a.op_host[k];
  const int32_t kind = a.op_kind[k];
  const bool ok = h >= 0 && h < a.H && (kind == 0 || kind == 1);
  if (!ok) atomicMin(a.bad, (uint32_t)k);
  a.key_in[k] = ok ? (uint32_t)h : 0u;   // (an invalid log is sorted too, and then not walked)
  a.idx_in[k] = (int32_t)k;
}

// subscribe: refused as a whole, else every positive amount leaves its level.
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

// unsubscribe: each resource on its own, against what is in use (rounded once).
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

__global__ void __launch_bounds__(HO_THREADS) host_ops_kernel(HostOpsArgs a) {
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
  for (int64_t j = i; j < K && a.key_out[j] == h; ++j) {
    const int64_t k = a.idx_out[j];
    double d[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) d[r] = a.op_amt[r * K + k];
    a.op_ok[k] = a.op_kind[k] == 0 ? subscribe(l, d) : unsubscribe(l, c, d);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) a.level[r * H + h] = l[r];
}

// (K + 255 would overflow int32 for the largest logs)
uint32_t hostops_blocks(int32_t K) { return (uint32_t)(((int64_t)K + HO_THREADS - 1) / HO_THREADS); }

}  // namespace

int hostops_key_bits(int32_t H) {
  int bits = 1;
  while (bits < 32 && ((int64_t)1 << bits) < (int64_t)H) ++bits;
  return bits;
}

hipError_t hostops_sort_temp(int32_t H, int32_t K, size_t* bytes) {
  *bytes = 0;
  return hipcub::DeviceRadixSort::SortPairs(nullptr, *bytes, (const uint32_t*)nullptr,
                                            (uint32_t*)nullptr, (const int32_t*)nullptr,
                                            (int32_t*)nullptr, K, 0, hostops_key_bits(H));
}

void launch_hostops_keys(const HostOpsArgs& a, hipStream_t st) {
  if (a.K <= 0) return;
  hipLaunchKernelGGL(host_ops_keys_kernel, dim3(hostops_blocks(a.K)), dim3(HO_THREADS), 0, st, a);
}

hipError_t hostops_sort(const HostOpsArgs& a, void* tmp, size_t tmp_bytes, hipStream_t st) {
  return hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, (const uint32_t*)a.key_in, a.key_out,
                                            (const int32_t*)a.idx_in, a.idx_out, a.K, 0,
                                            hostops_key_bits(a.H), st);
}

void launch_hostops_apply(const HostOpsArgs& a, hipStream_t st) {
  if (a.K <= 0) return;
  PVT_LAUNCH(host_ops_kernel, dim3(hostops_blocks(a.K)), dim3(HO_THREADS), 0, st, a);
}

}  // namespace pvt
