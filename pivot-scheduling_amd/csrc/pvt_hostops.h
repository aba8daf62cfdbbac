// pvt_hostops.h — a subscribe / unsubscribe log applied to resident host levels (see
// pvt_hostops.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pvt {

constexpr int HO_THREADS = 256;
constexpr uint32_t HO_NO_BAD = 0xffffffffu;   // *bad while every op seen so far is valid

struct HostOpsArgs {
  int32_t H, K;
  const double* capacity;
  double* level;
  const int32_t *op_host, *op_kind;
  const double* op_amt;
  int32_t* op_ok;
  uint32_t *key_in, *key_out;   // [K] the op's host, before and after the sort
  int32_t *idx_in, *idx_out;    // [K] the op's index k: idx_out is the permutation
  uint32_t* bad;                // the first invalid op, or HO_NO_BAD
};

// Key bits that vary over hosts 0 .. H-1: ceil(log2 H), at least 1.
int hostops_key_bits(int32_t H);
// Bytes of temporary storage the sort of K pairs needs.
hipError_t hostops_sort_temp(int32_t H, int32_t K, size_t* bytes);
// The three passes, on st: keys (+ range check into *bad, which the caller has set to HO_NO_BAD),
// the stable sort by host, the segment walk (which leaves at once when *bad is set).
void launch_hostops_keys(const HostOpsArgs& a, hipStream_t st);
hipError_t hostops_sort(const HostOpsArgs& a, void* tmp, size_t tmp_bytes, hipStream_t st);
void launch_hostops_apply(const HostOpsArgs& a, hipStream_t st);

}  // namespace pvt
