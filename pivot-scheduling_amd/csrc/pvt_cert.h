// pvt_cert.h — the zero-score certificates: thresholds, predicates and the certificate word
// ("Certificate thresholds"). Host and device code; no dependency but <cstdint>.
//
// A cost_aware host scores (c * ||avail - d||) / bw, exactly +0 only in a zero-cost zone of the
// anchor (c == 0) or as an exact fit (s2 = ||avail - d||^2 == 0). Every fast path -- the frontier
// walk, the list walks, epoch validation and finality, the host's verdict after the walk, the
// resident kernel's fast winner and its dense window -- skips scoring where the thresholds below
// prove a score positive (or exactly 0) and hands over to the exact path where one fails. This
// file is the only place that knows the numbers; tests/cert_cases.py plants its rounds at them
// (tests/test_cert_cases.py reads them from the `constexpr double NAME = 0x1p...;` lines).
//
// The slack. Together the thresholds bound a positive score from below by about
// CERT_C_MIN * CERT_SEP / CERT_BW_MAX = 2^-300 * 2^-288 / 2^300 = 2^-888 (2^-889 after the
// roundings of the norm), while a score rounds to 0 only below 2^-1075. A single threshold
// loosened by less than about 2^186, the others unchanged, is therefore still exact, and no test
// can or should catch that: a typo here is a wrong placement most tests cannot see.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PVT_CERT_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define PVT_CERT_FN inline
#endif

namespace pvt {

constexpr double CERT_C_MIN = 0x1p-300;    // c >= : a cost this large times a proven norm cannot underflow
constexpr double CERT_BW_MAX = 0x1p300;    // 0 < bw <= : dividing by it cannot take a proven score to 0
constexpr double CERT_S2_MIN = 0x1p-600;   // s2 >= : sqrt(s2) >= 2^-300, so c * sqrt(s2) / bw >= 2^-900 > 0
constexpr double CERT_RES_MIN = 0x1p-300;  // largest residual >= : s2 >= CERT_S2_MIN (the norm only adds terms >= 0)
constexpr double CERT_SEP = 0x1p-288;      // capacity - demand >= in some dimension: s2 >= 2^-578 for every such pair
constexpr double CERT_MARGIN = 0x1p-287;   // a log entry above the largest demand, and the verdict's host minimum: s2 >= 2^-576
constexpr double CERT_BOUND = 0x1p500;     // |x| <= : s2 stays finite, so c == 0 scores exactly +0 (bw > 0)
constexpr double CERT_FF_CAP = 0x1p298;    // first-fit, capacity <= : the host norm is <= 2^299, a positive key >= 2^-899

// What the code relies on between them.
static_assert(CERT_S2_MIN == CERT_RES_MIN * CERT_RES_MIN, "a residual at its bound gives s2 at its bound");
static_assert(CERT_SEP * CERT_SEP * 0x1p-2 >= CERT_S2_MIN && CERT_SEP >= CERT_RES_MIN,
              "a separated pair passes the per-entry tests (s2, residual) of the exact paths");
static_assert(CERT_MARGIN == 2 * CERT_SEP,
              "the verdict's minimum is the binade above the separation: a host minimum that vouches for an "
              "undemanded dimension also separates it in the walk, and 2^-288 (verdict_min_below) does not vouch");
static_assert(CERT_C_MIN * CERT_SEP / CERT_BW_MAX >= 0x1p-1022 && CERT_C_MIN * CERT_RES_MIN / CERT_BW_MAX >= 0x1p-1022,
              "the proven lower bounds of a score (2^-888, 2^-900) are normal numbers, far from rounding to 0");
static_assert(4 * ((2 * CERT_BOUND) * (2 * CERT_BOUND)) < __builtin_inf(),
              "s2 of four residuals of bounded operands is finite");
// First-fit key c * df / (||avail|| * bw): four capacities <= CERT_FF_CAP have a norm <= 2 * CERT_FF_CAP
// = 2^299, so with c >= CERT_C_MIN and bw <= CERT_BW_MAX a positive key is >= 2^-899 (df = 1), never 0.
static_assert(CERT_C_MIN / (2 * CERT_FF_CAP * CERT_BW_MAX) >= 0x1p-1022, "a positive first-fit key is a normal number");

// ---- predicates -------------------------------------------------------------------------------
// A site uses a predicate below where the call leaves the unit's gfx950 assembly as it was, and
// writes the same expression out with the constants above where it does not (EXPERIMENTS.md,
// round 14, lists those sites; a search for the constant finds them).
//
// The zone clause of the frontier walk, for a zone outside the chain's zone set U (first-fit:
// every zone with c != 0), is one of the written-out ones (zwalk_kernel, twice):
//   c >= CERT_C_MIN && bw > 0 && bw <= CERT_BW_MAX
// no host of such a zone scores 0 once a dimension separates. bw > 0: a negative bandwidth would
// give a negative key, ahead of every zero key. NaN fails every compare.
//
// The resident kernels' "safe" zone of an anchor: bw in (0, 2^300] and c == 0 or c in [2^-300, inf).
// Unlike the zone clause it classifies every zone, the anchor's zero-cost zones included (c == 0
// is safe: the score is exactly +0 while s2 is finite), and it excludes c == inf: the zero class
// below takes an exact fit (mx == 0) of a safe slot as score 0 whatever c is, and inf * 0 is NaN.
// The frontier walk's separation rules exact fits outside U out before its zone clause matters.
PVT_CERT_FN bool cert_safe_slot(double c, double bw) {
  return bw > 0.0 && bw <= CERT_BW_MAX && (c == 0.0 || (c >= CERT_C_MIN && c < __builtin_inf()));
}

// The score (c * sqrt(s2)) / bw is provably positive (>= 2^-900): it cannot tie a winner scoring +0.
PVT_CERT_FN bool cert_score_positive(double c, double s2, double bw) {
  return s2 >= CERT_S2_MIN && c >= CERT_C_MIN && bw <= CERT_BW_MAX;
}

// Some dimension holds the capacities a above the demands m by the margin (CERT_SEP: host minima
// against a chain's largest demands; CERT_MARGIN: a log entry against a block's largest demands).
// (a, m: four values each, read in order until one separates.)
PVT_CERT_FN bool cert_separates(const double* a, const double* m, double margin) {
  return (a[0] - m[0] >= margin) || (a[1] - m[1] >= margin) || (a[2] - m[2] >= margin) || (a[3] - m[3] >= margin);
}

// First-fit certificates (2') and (3') in one dimension: the largest capacity bounded (NaN fails:
// the caller's maximum propagates it), no demand negative.
PVT_CERT_FN bool cert_ff_bounded(double hmax, double dmin) { return (hmax <= CERT_FF_CAP) && (dmin >= 0.0); }

// Certificate 3: a window capacity or chain demand is finite and bounded. NaN fails.
PVT_CERT_FN bool cert_bounded(double x) { return __builtin_fabs(x) <= CERT_BOUND; }

// (The resident walks also test capacities and residuals of fitting hosts, which are >= +0, one
// sided: `!(x <= CERT_BOUND)`, true for NaN, and `x > CERT_BOUND`, false for NaN. Each site's NaN
// behaviour is what it needs; they are written out there and are not this predicate.)

// The resident kernels' classification of a host by its largest residual mx = max(a - d) (all
// residuals >= +0 when it fits): mx == 0 is an exact fit (s2 == 0, score 0); mx >= 2^-300 gives
// s2 >= 2^-600 (the FMA chain only adds non-negative terms), so with a safe slot and c > 0 the
// score is >= 2^-900; with c == 0 (zc) the score is 0 while s2 is finite (mx <= 2^500). A fitting
// host of the zero class can win at score 0; a fitting host that is neither of the zero class nor
// proven positive is risky and goes to the full path. (zero does not ask whether the host fits:
// the callers do.)
struct CertClass { bool zero, risky; };
PVT_CERT_FN CertClass cert_classify(bool fits, bool safe, bool zc, double mx) {
  const bool zero = safe && ((zc && mx <= CERT_BOUND) || mx == 0.0);
  return {zero, fits && !zero && (!safe || !(mx >= CERT_RES_MIN) || zc)};
}

// ---- the certificate word of a chain (frontier walk -> the host's verdict) ----------------------
// bit r (ZW_CERT_UNDEMANDED << r): every task of the chain demands +-0 in dimension r;
// bit 4 + r (ZW_CERT_HOSTMIN << r): the host minimum of dimension r is >= CERT_MARGIN (best-fit;
// first-fit reports 0); ZW_CERT_FAST: the chain took the fast prologue (it saved no undo rows).
constexpr int ZW_CERT_DIMS = 0xf;
constexpr int ZW_CERT_HOSTMIN_SHIFT = 4;
constexpr int ZW_CERT_UNDEMANDED = 1;
constexpr int ZW_CERT_HOSTMIN = 1 << ZW_CERT_HOSTMIN_SHIFT;
constexpr int ZW_CERT_FAST = 1 << 8;
constexpr int ZW_CERT_EVERY_DIM = ZW_CERT_DIMS | (ZW_CERT_DIMS << ZW_CERT_HOSTMIN_SHIFT);   // the AND's identity

// Dimension r's bits of the word. mx, mn: the chain's largest and smallest demand in r; ha: the
// host minimum of r. A chain's word is the OR over r = 0..3, plus ZW_CERT_FAST.
PVT_CERT_FN int zw_cert_dim(double mx, double mn, double ha, int r) {
  return ((mx <= 0.0 && mn >= 0.0) ? (ZW_CERT_UNDEMANDED << r) : 0) | ((ha >= CERT_MARGIN) ? (ZW_CERT_HOSTMIN << r) : 0);
}

// The host's verdict from the AND of every chain's word: some dimension is undemanded by every
// chain and has a host minimum >= CERT_MARGIN. Then each log entry keeps its start value there,
// above the epoch's largest demand (+-0) by the margin epoch_final_kernel asks for.
PVT_CERT_FN bool zw_cert_verdict(int all_chains) {
  return ((all_chains & ZW_CERT_DIMS) & (all_chains >> ZW_CERT_HOSTMIN_SHIFT)) != 0;
}

}  // namespace pvt
