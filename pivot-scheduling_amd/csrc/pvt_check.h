// pvt_check.h — opt-in validation of a round's contents (see pvt_check.hip, pvt_check_rules.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pivot_place.h"
#include "pvt_check_rules.h"

namespace pvt {

constexpr int CHK_THREADS = 256;         // four wave64 per block
constexpr int CHK_BLOCKS_PER_CU = 8;     // grid of a large round: every CU's wave slots filled
constexpr int64_t CHK_BLOCK_BYTES = 16384;   // a block is worth launching per this many bytes

// One round as the check reads it. A NULL array is a rule that does not apply (the table of
// include/pivot_place.h): check_describe() decides that once, for the device and the host path.
struct CheckRound {
  int32_t mode, H, T, Z, G;        // G: n_groups with task_group, else 0
  int32_t blk_lo, blk_n;           // its blocks of the launch: [blk_lo, blk_lo + blk_n)
  int32_t pad;
  int64_t n_rt;                    // elements of rt_bw: max(G, 1) * H
  const double *avail, *dem, *cost, *bw, *rt_bw;
  const int32_t *zone, *task_group, *group_anchor, *decay;
  const uint32_t* tiebreak;
  uint32_t* owner;                 // [H] rule 10: lowest host of each rank (context scratch)
};

// Per round and rule k: key[k] = ~(lowest violating index) (0: none), cnt[k] = violations.
// Zeroed before the launch; integer atomicMax / atomicAdd only, so the report does not depend
// on the block schedule.
struct CheckSlots {
  unsigned long long key[CHK_RULES + 1];
  unsigned long long cnt[CHK_RULES + 1];
};

CheckRound check_describe(const pvt_round& r);
double check_bytes(const CheckRound& c);
// Deals the launch's blocks to the rounds in proportion to their bytes, at least one each;
// returns the grid.
int check_deal(CheckRound* rounds, int n, int cus);
void launch_check_owner(const CheckRound* rounds_dev, int n, int grid, hipStream_t st);
void launch_check(const CheckRound* rounds_dev, int n, int grid, CheckSlots* slots, hipStream_t st);
void launch_check_finish(const CheckRound* rounds_dev, int n, const CheckSlots* slots,
                         pvt_check_report* out_dev, hipStream_t st);
// The same rules over HOST arrays (pvt_place_host*), rules 1-10; the verdict equals the device's.
void check_on_host(const CheckRound& c, pvt_check_report* out);

}  // namespace pvt
