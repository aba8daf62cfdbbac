// Latency probe (stand-alone, `make f64-chain`; never linked into the library): what one wave
// pays per dependent link of a chain of v_add_f64 or v_fma_f64 on this part -- the floor of
// run_bulk's copy loops (pvt_zwalk.hip).
//
// One wave of one workgroup runs LINKS dependent links of each of C independent chains (C = 1, 2,
// 4), the chains interleaved link by link, in three forms:
//   bare  the chain instructions only;
//   test  plus, per link step, the fit test of a copy: one v_min_f64 per chain pair, one v_cmp and
//         one carry add, all on registers no chain writes;
//   keep  plus two 32-bit selects per chain (the 64-bit "capacities after the last fitting copy").
// The extra instructions are independent of the chains, and the compare reads the minimum of the
// step before; only the selects and the carry add hang on their step's compare, through vcc. So
// nearly all they cost beyond the bare form is issue, not latency. Every instruction is one asm volatile statement (or a group of them): the
// order written is the order run. s_memtime stamps around the loop only; random finite inputs.
//
// Prints cycles per link step (all C chains advance one link) and per chain link for each form.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#define CK(e)                                                                  \
  do {                                                                         \
    hipError_t r_ = (e);                                                       \
    if (r_ != hipSuccess) {                                                    \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, hipGetErrorString(r_)); \
      exit(1);                                                                 \
    }                                                                          \
  } while (0)

constexpr int UNROLL = 16;
constexpr int ITERS = 64;
constexpr int LINKS = UNROLL * ITERS;

__device__ __forceinline__ uint64_t stamp() {
  uint64_t t;
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  return t;
}

// OP 0: x = x + d (v_add_f64); OP 1: x = fma(o, d, x) (v_fma_f64). FORM 0 bare, 1 test, 2 keep.
template <int OP, int C, int FORM>
__global__ __launch_bounds__(64) void chain_kernel(const double* in, double* out, uint64_t* cyc) {
  const int l = threadIdx.x;
  double x[4], d[4];
  for (int c = 0; c < 4; c++) {
    x[c] = in[l * 16 + c];
    d[c] = in[l * 16 + 4 + c];
  }
  double o = in[l * 16 + 8] < 2.0 ? -1.0 : 1.0;   // (-1 in every lane, unknown to the compiler)
  double p = in[l * 16 + 9], q = in[l * 16 + 10], r = in[l * 16 + 11], s = in[l * 16 + 12];
  double m0 = in[l * 16 + 13], m1 = in[l * 16 + 14], m2 = 0.0, m3 = 0.0;
  uint32_t y[8] = {0, 0, 0, 0, 0, 0, 0, 0}, w = (uint32_t)l, cnt = 0;
  __builtin_amdgcn_sched_barrier(0);
  const uint64_t t0 = stamp();
  for (int it = 0; it < ITERS; it++) {
#pragma unroll
    for (int u = 0; u < UNROLL; u++) {
#pragma unroll
      for (int c = 0; c < C; c++) {
        if (OP == 0) asm volatile("v_add_f64 %0, %0, %1" : "+v"(x[c]) : "v"(d[c]));
        else asm volatile("v_fma_f64 %0, %1, %2, %0" : "+v"(x[c]) : "v"(o), "v"(d[c]));
      }
      if (FORM >= 1) {
        // the minimum of this step; the compare (and what hangs on it) on the minimum of the step
        // before
        double& mw = (u & 1) ? m1 : m0;
        const double mr = (u & 1) ? m0 : m1;
        if (C == 4) {
          asm volatile("v_min_f64 %0, %1, %2" : "=v"(m2) : "v"(r), "v"(s));
          asm volatile("v_min_f64 %0, %1, %2" : "=v"(m3) : "v"(r), "v"(q));
        }
        asm volatile("v_min_f64 %0, %1, %2" : "=v"(mw) : "v"(p), "v"(q));
        if (FORM == 1)
          asm volatile("v_cmp_le_f64 vcc, 0, %1\n\tv_addc_co_u32 %0, vcc, 0, %0, vcc" : "+v"(cnt) : "v"(mr) : "vcc");
        else if (C == 1)
          asm volatile("v_cmp_le_f64 vcc, 0, %3\n\tv_cndmask_b32 %1, %1, %4, vcc\n\tv_cndmask_b32 %2, %2, %4, vcc\n\t"
                       "v_addc_co_u32 %0, vcc, 0, %0, vcc"
                       : "+v"(cnt), "+v"(y[0]), "+v"(y[1]) : "v"(mr), "v"(w) : "vcc");
        else if (C == 2)
          asm volatile("v_cmp_le_f64 vcc, 0, %5\n\tv_cndmask_b32 %1, %1, %6, vcc\n\tv_cndmask_b32 %2, %2, %6, vcc\n\t"
                       "v_cndmask_b32 %3, %3, %6, vcc\n\tv_cndmask_b32 %4, %4, %6, vcc\n\t"
                       "v_addc_co_u32 %0, vcc, 0, %0, vcc"
                       : "+v"(cnt), "+v"(y[0]), "+v"(y[1]), "+v"(y[2]), "+v"(y[3]) : "v"(mr), "v"(w) : "vcc");
        else
          asm volatile("v_cmp_le_f64 vcc, 0, %9\n\tv_cndmask_b32 %1, %1, %10, vcc\n\tv_cndmask_b32 %2, %2, %10, vcc\n\t"
                       "v_cndmask_b32 %3, %3, %10, vcc\n\tv_cndmask_b32 %4, %4, %10, vcc\n\t"
                       "v_cndmask_b32 %5, %5, %10, vcc\n\tv_cndmask_b32 %6, %6, %10, vcc\n\t"
                       "v_cndmask_b32 %7, %7, %10, vcc\n\tv_cndmask_b32 %8, %8, %10, vcc\n\t"
                       "v_addc_co_u32 %0, vcc, 0, %0, vcc"
                       : "+v"(cnt), "+v"(y[0]), "+v"(y[1]), "+v"(y[2]), "+v"(y[3]), "+v"(y[4]), "+v"(y[5]),
                         "+v"(y[6]), "+v"(y[7]) : "v"(mr), "v"(w) : "vcc");
      }
    }
  }
  const uint64_t t1 = stamp();
  __builtin_amdgcn_sched_barrier(0);
  double acc = m0 + m1 + m2 + m3;
  for (int c = 0; c < 4; c++) acc += x[c];
  uint32_t yy = cnt;
  for (int c = 0; c < 8; c++) yy ^= y[c];
  out[l] = acc + (double)yy;
  if (l == 0) cyc[0] = t1 - t0;
}

template <int OP, int C, int FORM>
static void run(const double* in, double* out, uint64_t* cyc, uint64_t* hcyc) {
  uint64_t best = ~0ull;
  for (int rep = 0; rep < 5; rep++) {            // (the first launch loads the code; keep the minimum)
    chain_kernel<OP, C, FORM><<<1, 64>>>(in, out, cyc);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(hcyc, cyc, sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (*hcyc < best) best = *hcyc;
  }
  static const char* form[3] = {"bare", "test", "keep"};
  const int extra = FORM == 0 ? 0 : (C == 4 ? 3 : 1) + 2 + (FORM == 2 ? 2 * C : 0);
  printf("%-9s chains %d  %-4s  %2d instr/step  %7.2f cycles per link step  %6.2f per chain link\n",
         OP ? "v_fma_f64" : "v_add_f64", C, form[FORM], C + extra, (double)best / LINKS,
         (double)best / LINKS / C);
}

template <int OP>
static void run_op(const double* in, double* out, uint64_t* cyc, uint64_t* hcyc) {
  run<OP, 1, 0>(in, out, cyc, hcyc); run<OP, 1, 1>(in, out, cyc, hcyc); run<OP, 1, 2>(in, out, cyc, hcyc);
  run<OP, 2, 0>(in, out, cyc, hcyc); run<OP, 2, 1>(in, out, cyc, hcyc); run<OP, 2, 2>(in, out, cyc, hcyc);
  run<OP, 4, 0>(in, out, cyc, hcyc); run<OP, 4, 1>(in, out, cyc, hcyc); run<OP, 4, 2>(in, out, cyc, hcyc);
}

int main() {
  std::mt19937_64 rng(12345);
  std::uniform_real_distribution<double> cap(1.0, 1.0e6), dem(-4.0, -0.01);
  std::vector<double> h(64 * 16);
  for (int l = 0; l < 64; l++)
    for (int k = 0; k < 16; k++) h[l * 16 + k] = (k >= 4 && k < 8) ? dem(rng) : cap(rng);
  for (int l = 0; l < 64; l++) h[l * 16 + 8] = 1.0;
  double *in, *out;
  uint64_t *cyc, hcyc = 0;
  CK(hipMalloc(&in, h.size() * sizeof(double)));
  CK(hipMalloc(&out, 64 * sizeof(double)));
  CK(hipMalloc(&cyc, sizeof(uint64_t)));
  CK(hipMemcpy(in, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
  printf("# one wave, %d links per chain, s_memtime around the loop, minimum of 5 launches\n", LINKS);
  run_op<0>(in, out, cyc, &hcyc);
  run_op<1>(in, out, cyc, &hcyc);
  CK(hipFree(in)); CK(hipFree(out)); CK(hipFree(cyc));
  return 0;
}
