// pvt_rtrows.h — realtime-bandwidth rows built on the device from a sparse list of route queues
// (see pvt_rtrows.hip; the contract is in include/pivot_place.h at pvt_route_queues).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pvt {

constexpr int RT_THREADS = 256;
constexpr int RT_TILE = 2048;          // hosts per workgroup of the fill: 2 quads of hosts per lane
constexpr int RT_GROUPS = 8;           // rows per workgroup of the fill at the most (one LDS table each)
constexpr uint32_t RT_NO_BAD = 0xffffffffu;   // a word of bad[] while nothing invalid was seen

struct RtRowsArgs {
  int32_t H, Z, G, R;            // G as the caller gave it (0: one row, anchored at zone 0)
  int64_t P;
  const int32_t* zone;           // [H]
  const double* bw;              // [Z*Z]
  const int32_t* group_anchor;   // [G] or NULL
  const int32_t *rq_anchor, *rq_host, *rq_dir;   // [R]
  const double* rq_bw;           // [R]
  const int64_t* rq_off;         // [R+1]
  const double* rq_mbs;          // [P]
  double* val;                   // [R] scratch: the listed routes' realtime bandwidths
  double* rt_bw;                 // [max(G,1)*H] out
  uint32_t* bad;                 // [3] the first invalid entry, group anchor, host zone (RT_NO_BAD: none)
};

// Rows per workgroup of the fill, balanced over ceil(rows / RT_GROUPS) chunks.
int rtrows_chunk(int32_t rows);
// The bytes the fill moves by the model in pvt_rtrows.hip's header.
double rtrows_fill_bytes(const RtRowsArgs& a);
// The four passes, on st, in this order; the caller has set bad[0..2] to RT_NO_BAD. Each pass
// after the check leaves at once when a word of bad[] is set.
void launch_rt_check(const RtRowsArgs& a, hipStream_t st);
void launch_rt_value(const RtRowsArgs& a, hipStream_t st);
void launch_rt_fill(const RtRowsArgs& a, hipStream_t st);
void launch_rt_patch(const RtRowsArgs& a, hipStream_t st);

}  // namespace pvt
