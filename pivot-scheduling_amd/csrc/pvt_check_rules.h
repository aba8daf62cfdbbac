// pvt_check_rules.h — the content rules of a round (include/pivot_place.h, pvt_check_round),
// written once: the device check kernel (pvt_check.hip) and the host-array check of
// pvt_place_host* (pvt_resident.hip) both call these predicates, so they cannot drift apart. Each
// returns true when the element VIOLATES its rule. pivot_place/checks.py restates them in numpy.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PVT_CHK_HD __host__ __device__
#else
#define PVT_CHK_HD
#endif

namespace pvt {

constexpr int CHK_RULES = 11;   // rule codes 1 .. CHK_RULES (enum pvt_check)

PVT_CHK_HD inline uint64_t chk_bits(double v) {
  uint64_t b;
  __builtin_memcpy(&b, &v, sizeof(b));
  return b;
}

// rules 1, 4, 5: an index outside [0, n)
PVT_CHK_HD inline bool chk_bad_index(int32_t v, int32_t n) { return v < 0 || v >= n; }

// rules 2, 3: an amount that is not finite or has its sign bit set (-0.0 included). The engine
// orders such keys by their bits: as an unsigned word everything from +inf up (inf, NaN, and
// every value with the sign bit) is out.
PVT_CHK_HD inline bool chk_bad_amount(double v) { return chk_bits(v) >= 0x7ff0000000000000ull; }

// rule 6: the cost sum cost[a][z] + cost[z][a] (NaN violates)
PVT_CHK_HD inline bool chk_bad_cost_sum(double c) { return !(c >= 0.0); }

// rule 7: the bandwidth sum bw[a][z] + bw[z][a] (NaN violates)
PVT_CHK_HD inline bool chk_bad_bw_sum(double b) { return !(b > 0.0); }

// rule 8: a realtime bandwidth that is not finite or not > 0
PVT_CHK_HD inline bool chk_bad_rt_bw(double v) {
  return !(v > 0.0) || chk_bits(v) >= 0x7ff0000000000000ull;
}

// rule 9: host_decay is max(len(h.tasks), 1)
PVT_CHK_HD inline bool chk_bad_decay(int32_t v) { return v < 1; }

// rule 10, first half: a rank outside [0, H) (the second half, a rank an earlier host holds,
// needs the owner table: owner[rank] = the lowest host with that rank)
PVT_CHK_HD inline bool chk_bad_rank(uint32_t rank, int32_t H) { return rank >= (uint32_t)H; }

// rule 11: the MT19937 position (mt_state[624])
PVT_CHK_HD inline bool chk_bad_mtpos(uint32_t pos) { return pos > 624u; }

}  // namespace pvt
