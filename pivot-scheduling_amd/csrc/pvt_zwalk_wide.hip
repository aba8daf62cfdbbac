// pvt_zwalk_wide.hip -- the frontier walk for rounds of more than ZMAX zones: the wide instances
// of the __global__ zwalk_kernel (window of ZW_M and ZW_MBIG hosts, best-fit and first-fit chains)
// and the zero-pair kernel of the driver's component plan. The wide section of pvt_zwalk.hip,
// compiled as a translation unit of its own, so that pvt_zwalk.hip holds exactly the instances it
// held before (make isa-diff compares like with like).
#define PVT_ZWALK_WIDE_TU 1
#include "pvt_zwalk.hip"
