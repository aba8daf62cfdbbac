// pvt_batch_wide.hip -- the resident kernels for batches with a round of more than ZMAX zones
// (the __global__ resident_wide_kernel and the wide instances of resident_fused_kernel): the wide section of pvt_batch.hip, compiled
// as a translation unit of its own so the two halves build side by side.
#define PVT_RESIDENT_WIDE_TU 1
#include "pvt_batch.hip"
