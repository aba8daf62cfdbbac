// pvt_hostmeter.h — the reference meter's host half run from the resident op log (see
// pvt_hostmeter.hip; the contract is in include/pivot_place.h at pvt_host_meter).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pvt_hostops.h"

namespace pvt {

// st_word values, and the kinds of a mark
constexpr int32_t HM_NONE = 0, HM_OPEN = 1, HM_CLOSED = 2;
constexpr int32_t HM_CHECK_IN = 2, HM_CHECK_OUT = 3;

struct HostMeterArgs {
  int32_t H, K;
  const double* capacity;
  double* level;
  int32_t* st_word;
  double *st_start, *st_end;
  int32_t* iv_host;
  double *iv_start, *iv_end;
  int32_t* us_host;
  double *us_time, *us_frac;
  const int32_t *op_host, *op_kind;
  const double *op_amt, *op_time;
  int32_t* op_ok;
  double last_time;
  uint32_t *key_in, *key_out;   // [K] as in HostOpsArgs
  int32_t *idx_in, *idx_out;
  uint32_t* bad;                // the first invalid entry, or HO_NO_BAD
  unsigned long long* cnt;      // [0] intervals, [1] usage records in the logs (slots by atomicAdd)
};

// finish: device words the passes share
//   [0] hosts with an open interval   [1] the first of them   [2] closed last intervals (the tail)
//   [3] rows
constexpr int HM_WORDS = 4;

struct HostMeterFinish {
  int32_t H;
  int32_t n_iv, n_us;           // records in the raw logs
  int32_t n_ivf;                // intervals after the tail is appended (set for the second half)
  const int32_t* st_word;
  const double *st_start, *st_end;
  const int32_t* iv_host;
  const double *iv_start, *iv_end;
  const int32_t* us_host;
  const double *us_time, *us_frac;
  uint32_t *ivk_in, *ivk_out;   // [n_iv + tail bound] interval keys (hosts), in and sorted
  int32_t *ivi_in, *ivi_out;    //   and where each comes from: a log index, or >= n_iv: the state
  uint32_t *usk_in, *usk_out;   // [n_us] usage keys
  int32_t *usi_in, *usi_out;
  int32_t *head, *row;          // [n_us] 1 at the first record of a host; its exclusive sum
  uint32_t* words;              // [HM_WORDS]
  int32_t* o_row_host;
  int64_t *o_iv_off, *o_us_off;
  double *o_iv_start, *o_iv_end, *o_us_time, *o_us_frac;
};

// apply: keys (+ the per-entry contract into *bad), then hostops' stable sort, then the walk
void launch_hostmeter_keys(const HostMeterArgs& a, hipStream_t st);
hipError_t hostmeter_sort(int32_t H, int32_t n, const uint32_t* key_in, uint32_t* key_out,
                          const int32_t* idx_in, int32_t* idx_out, void* tmp, size_t tmp_bytes,
                          hipStream_t st);
void launch_hostmeter_apply(const HostMeterArgs& a, hipStream_t st);
// finish, first half: open hosts counted, interval keys written with the tail appended
void launch_hostmeter_tail(const HostMeterFinish& f, hipStream_t st);
// finish, second half (the interval keys sorted, n_ivf known): interval gather; usage keys; after
// the usage sort the heads, their exclusive sum (hostmeter_scan) and the rows + usage gather
void launch_hostmeter_iv_gather(const HostMeterFinish& f, hipStream_t st);
void launch_hostmeter_us_keys(const HostMeterFinish& f, hipStream_t st);
void launch_hostmeter_heads(const HostMeterFinish& f, hipStream_t st);
hipError_t hostmeter_scan_temp(int32_t n, size_t* bytes);
hipError_t hostmeter_scan(const HostMeterFinish& f, void* tmp, size_t tmp_bytes, hipStream_t st);
void launch_hostmeter_rows(const HostMeterFinish& f, hipStream_t st);

}  // namespace pvt
