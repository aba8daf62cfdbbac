// pvt_usage.h — Meter usage series over a batch of scenarios (see pvt_usage.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pvt {

constexpr int USE_THREADS = 256;
constexpr int64_t USE_TIME_END = (int64_t)1 << 52;   // times lie in [0, 2^52)

struct UsageArgs {
  int32_t n_scen;
  int64_t sample_size;
  int64_t n_host_rows, n_iv, n_us, n_buckets;
  const int64_t *host_off, *iv_off, *us_off, *bucket_off;   // us_off NULL: no resource series
  const double *iv_start, *iv_end, *us_time, *us_frac;
  int32_t *n_hosts, *res_hosts;
  double *res_mean, *avg;
  int32_t* bad;
};

void launch_usage(const UsageArgs& a, hipStream_t st);

}  // namespace pvt
