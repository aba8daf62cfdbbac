/*
 * pivot_place.h — C ABI of the MI355X placement engine for the PIVOT simulator.
 *
 * One call, pvt_place(), runs one scheduling round of one policy: every ready task x host
 * candidate is scored on the GPU and a host is picked per task, with capacity commits applied
 * in the reference's sequential order. It replaces the body of the reference policies'
 * schedule() hook:
 *
 *   - scheduler/__init__.py:79-80   GlobalSchedulerBase.schedule(self, tasks)   (plugin hook)
 *   - scheduler/__init__.py:103     the per-round call site in _dispatch
 *   - scheduler/cost_aware.py:28-43, 60-127   PVT_CA_FF / PVT_CA_BF
 *   - scheduler/opportunistic.py:11-20        PVT_OPP
 *   - scheduler/vbp.py:13-29                  PVT_VBP_FF
 *   - scheduler/vbp.py:39-50                  PVT_VBP_BF
 *
 * The reference binds nothing natively (it is pure Python); the binding a maintainer adds is
 * a ctypes stub, shown in INTEGRATION.md and implemented in pivot_place/engine.py + _abi.py.
 *
 * Conventions
 *   - Plain C types only. Returns PVT_OK (0) or a negative PVT_E* code; never throws.
 *   - Array pointers in pvt_round are DEVICE pointers (HBM, e.g. from torch-ROCm tensors),
 *     except mt_state, which is host memory. The library never frees caller memory; scratch
 *     lives in the context and grows on demand.
 *   - Work is ordered on the context's stream; pvt_place() synchronises before it returns.
 *   - A context is not thread-safe. Use one per thread and per GPU.
 *   - Arithmetic is IEEE fp64 with no contraction, so results are bit-exact against the
 *     reference (squared norms are the sequential FMA chain numpy/OpenBLAS ddot performs).
 */
#ifndef PIVOT_PLACE_H
#define PIVOT_PLACE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PVT_ABI_VERSION 3

/* Zones of a round: 1 <= pvt_round.n_zones <= PVT_MAX_ZONES at every entry point that takes a
 * round; more is PVT_EINVAL and nothing is written. Up to 32 zones a round runs the fast paths
 * (zone tables in LDS, zero-cost frontier walks, group epochs, one-wave resident walks). From 33
 * on, the windowed engine runs the group epochs and the frontier walks for unsharded cost_aware
 * rounds without rt_bw whose zero-cost components have at most 32 zones each (a chain of a larger
 * component, and any chain a certificate fails for, goes to the lists); every other wide round
 * -- host-sharded, rt_bw, the resident kernels -- runs bit-exactly on the list-based windows and
 * the wide resident kernels, which read the Z x Z tables from global memory and run no one-wave
 * walk. PVT_ZW_WIDE=0 at pvt_ctx_create keeps all wide rounds on the lists. pvt_max_zones() is
 * the loaded library's bound. */
#define PVT_MAX_ZONES 512

/* Return codes. */
#define PVT_OK            0
#define PVT_EINVAL       -1   /* bad argument (null pointer, size, mode)          */
#define PVT_ENODEV       -2   /* no usable gfx950 device                          */
#define PVT_EHIP         -3   /* a HIP runtime call failed (see pvt_last_error)   */
#define PVT_ENOMEM       -4   /* scratch allocation failed                        */
#define PVT_EUNSUPPORTED -5   /* configuration the engine does not implement      */
#define PVT_ESTALE       -6   /* pvt_shard_commit: the exchanged window was scored while the
                                 previous walk ran, and that walk stopped early -- call
                                 pvt_shard_score again (every rank gets it together)     */

/* Policies (kernel modes). */
enum pvt_mode {
  PVT_CA_FF  = 0, /* cost_aware first-fit: strict fit, hosts ordered by frozen per-group key
                     (sort_hosts) or by index; scheduler/cost_aware.py:99-127              */
  PVT_CA_BF  = 1, /* cost_aware best-fit: fit >=, min egress-cost x residual / bw;
                     scheduler/cost_aware.py:63-97                                         */
  PVT_OPP    = 2, /* opportunistic: fit >=, uniform pick by MT19937 randint;
                     scheduler/opportunistic.py:11-20                                      */
  PVT_VBP_FF = 3, /* vbp first-fit: fit >=, lowest index; scheduler/vbp.py:13-29          */
  PVT_VBP_BF = 4  /* vbp best-fit: strict fit, min residual norm, tie by host-id string;
                     scheduler/vbp.py:39-50                                                */
};

/*
 * One scheduling round. Sizes: H hosts, T ready tasks, Z zones, G groups.
 *
 * Host state is SoA: avail[r*H + h] for resource r in {0 cpus, 1 mem, 2 disk, 3 gpus}
 * (the snapshot of scheduler/__init__.py:82-85, in cluster.hosts order). Task demands are
 * SoA too: dem[r*T + t], in the order of the `tasks` list passed to schedule().
 *
 * Groups (cost_aware only, scheduler/cost_aware.py:45-58): task_group[t] in [0, G) and
 * group_anchor[g] is the anchor storage zone. Groups run in id order; tasks of a group in
 * caller order, stably sorted by descending ||d||2 when sort_tasks is set. For the other
 * policies pass task_group = NULL (one group holding every task).
 *
 * realtime_bw (cost_aware, scheduler/cost_aware.py:17,79,112): rt_bw[g*H + h] is the bandwidth
 * the reference uses instead of the static one for group g (0 without task_group) and host h,
 * in_route.realtime_bw + out_route.realtime_bw of the routes between g's anchor storage and h
 * (resources/network.py:70-73: 1 / ((queued MB + 1) / bw) per route, summed in that order). NULL:
 * the static bw[a][z] + bw[z][a].
 */
typedef struct pvt_round {
  int32_t mode;          /* enum pvt_mode                                                 */
  int32_t n_hosts;       /* H >= 1                                                        */
  int32_t n_tasks;       /* T >= 0                                                        */
  int32_t n_zones;       /* 1 <= Z <= PVT_MAX_ZONES (cost/bw are Z x Z)                   */
  int32_t n_groups;      /* G (cost_aware); ignored when task_group is NULL               */
  int32_t sort_tasks;    /* stable sort by descending ||d||2 within each group            */
  int32_t sort_hosts;    /* PVT_CA_FF: order hosts by the frozen key (cost_aware.py:118)  */
  int32_t reserved;      /* must be 0                                                     */
  double* avail;         /* [4*H] in/out: commits are applied. Rule 2 (PVT_CHK_AVAIL): every
                            element finite with a clear sign bit (no -0.0): the engine orders
                            residuals by their bits                                        */
  const int32_t* zone;   /* [H] zone index of each host (Host.locality). Rule 1
                            (PVT_CHK_ZONE): every zone[h] in [0, Z) -- it indexes the zone
                            tables                                                         */
  const uint32_t* tiebreak; /* [H] rank of the host-id string (PVT_VBP_BF), else NULL. Rule 10
                            (PVT_CHK_TIEBREAK, PVT_VBP_BF): ranks < H and distinct (the
                            violators: an out-of-range rank, and every host but the first
                            that holds a rank)                                             */
  const int32_t* decay;  /* [H] max(len(h.tasks),1) (PVT_CA_FF host_decay), else NULL. Rule 9
                            (PVT_CHK_DECAY, when set): every decay[h] >= 1                 */
  const double* cost;    /* [Z*Z] egress cost, cost[src*Z + dst] (ResourceMetadata.cost).
                            Rule 6 (PVT_CHK_COST, cost_aware with T > 0):
                            every cost[a][z] + cost[z][a] >= +0 (egress prices: a score
                            c*r/bw then never grows as a residual r shrinks, and 0 is the
                            least score). Host-array calls (pvt_place_host*) check both
                            contracts (PVT_EINVAL), device rounds must meet them
                            (pvt_check_round / pvt_set_checks test them on the device)     */
  const double* bw;      /* [Z*Z] jittered bandwidth, bw[src*Z + dst]. Rule 7 (PVT_CHK_BW,
                            cost_aware with T > 0): every bw[a][z] +
                            bw[z][a] > 0 (resources/network.py bandwidths are positive: the
                            engine orders cost_aware scores >= +0 by their bits)           */
  const double* dem;     /* [4*T] task demand (cpus, mem, disk, gpus). Rule 3 (PVT_CHK_DEM,
                            T > 0): as rule 2 (suffix maxima of demands prune by bits)     */
  const int32_t* task_group;   /* [T] or NULL. Rule 4 (PVT_CHK_GROUP, when set and T > 0):
                            every task_group[t] in [0, G)                                  */
  const int32_t* group_anchor; /* [G] anchor zone per group, or NULL. Rule 5 (PVT_CHK_ANCHOR,
                            with task_group and T > 0): every group_anchor[g] in [0, Z)    */
  int32_t* order;        /* [T] out: processing order (task indices)                      */
  int32_t* placement;    /* [T] out: host index, -1 = not placed (task stays waiting)     */
  uint32_t* mt_state;    /* HOST [625] in/out: MT19937 key[624] then pos (PVT_OPP). Rule 11
                            (PVT_CHK_MTPOS, PVT_OPP): pos <= 624                           */
  const double* rt_bw;   /* [G*H] realtime bandwidth per (group, host), or NULL (cost_aware).
                            Rule 8 (PVT_CHK_RTBW, cost_aware when set): each of the
                            max(G,1)*H elements finite and > 0                             */
} pvt_round;

typedef struct pvt_ctx pvt_ctx;

/* Per-kernel-class timing gathered while profiling is on (HIP events on the ctx stream). */
typedef struct pvt_kstats {
  int64_t launches;      /* kernel launches timed                                         */
  double  ms;            /* summed device time, milliseconds                              */
  double  candidates;    /* task x host candidates those launches evaluated               */
  double  bytes;         /* algorithmic bytes: candidates x bytes/candidate (§8(d))       */
} pvt_kstats;

/* Kernel classes reported by pvt_get_kstats. */
enum pvt_kclass {
  PVT_K_SCORE = 0,   /* fused fit-mask + score + per-task top-K (the hot kernel)          */
  PVT_K_MERGE = 1,   /* per-task merge of segment top-K lists                              */
  PVT_K_COMMIT = 2,  /* sequential in-order commit walk                                    */
  PVT_K_OTHER = 3,   /* keys, norms, sorts, counts                                         */
  PVT_K_COUNT = 4
};

int  pvt_abi_version(void);
int  pvt_max_zones(void);   /* PVT_MAX_ZONES of the loaded library */
int  pvt_ctx_create(int device, pvt_ctx** out);
int  pvt_ctx_destroy(pvt_ctx* ctx);
/* Order the context's work on a caller stream (hipStream_t as void*), e.g.
 * torch.cuda.current_stream().cuda_stream. NULL is the device's default (null) stream, which is
 * what torch's default stream is. Until the first call the context uses a stream of its own. */
int  pvt_ctx_set_stream(pvt_ctx* ctx, void* stream);
int  pvt_place(pvt_ctx* ctx, const pvt_round* r);
/* Profiling: on = 1 records HIP events around every kernel launch (adds a little host overhead:
 * ~30 us per config-5 round of ~15 launches); on = 2 only around the named kernels of
 * pvt_get_kernel_kstats (the kernel-class times of the other launches stay zero). The events are
 * timing-only (hipEventDisableSystemFence) and come from a pool this call fills and records once
 * (synchronising the context's stream), so a timed round creates none. */
int  pvt_set_profiling(pvt_ctx* ctx, int on);
int  pvt_reset_kstats(pvt_ctx* ctx);
int  pvt_get_kstats(pvt_ctx* ctx, int kclass, pvt_kstats* out);
/* Per-kernel timing while profiling is on: the launches of the named __global__ kernel of the
 * placement path ("zwalk_kernel", "commit_kernel", "lwalk_kernel", "opp_commit_kernel",
 * "opp_count_kernel", "score_kernel", "band_score_kernel", "perm_scan_kernel", "ordered_kernel",
 * "resident_kernel", "merge_kernel", "merge_small_kernel", "merge_pkg_kernel",
 * "merge_path_kernel"; "check_kernel" of pvt_check_round / pvt_set_checks; and
 * "host_ops_kernel", the segment walk of pvt_host_ops_apply, and "rt_fill_kernel", the
 * streaming pass of pvt_rt_rows), each bracketed
 * by its own HIP events on the stream it runs on. An unknown or unlaunched name gives zeros. */
int  pvt_get_kernel_kstats(pvt_ctx* ctx, const char* kernel, pvt_kstats* out);
/* With profiling on = 2, record events around the launches of this one named kernel only
 * (NULL or "": every named kernel). Each event pair costs the stream a few microseconds of idle
 * GPU (config 5: 0.33 ms of a 2.74 ms vbp best-fit round with every named kernel timed), so a
 * benchmark times only the kernel its roofline is about. */
int  pvt_set_profiling_kernel(pvt_ctx* ctx, const char* kernel);
/* Tuning knob: tasks per window (0 = the policy's default; capped at 1024). */
int  pvt_set_window(pvt_ctx* ctx, int tasks);
/* Tuning knob: tasks per wave of the best-fit score kernel, 0 (the policy's default: 2 for vbp
 * best-fit and for cost_aware below 262144 hosts, else 4), 2 or 4. Results are identical. */
int  pvt_set_score_tw(pvt_ctx* ctx, int tw);
/* Tuning knob: vbp best-fit rounds of at least min_hosts hosts (per shard) build their candidate
 * lists from a memory band over the hosts sorted once per round by snapshot memory (hosts
 * committed to since the snapshot are scanned with their live state) instead of streaming every
 * host per task; 0 disables it. Default 65536. Results are identical either way. Replaces the
 * per-task host scan of scheduler/vbp.py:43-47. */
int  pvt_set_band(pvt_ctx* ctx, int32_t min_hosts);
/* Window pipelining (default on): score window k+1 on a side stream while window k is walked.
 * Results are identical either way; off runs windows strictly one after the other. */
int  pvt_set_pipeline(pvt_ctx* ctx, int on);
/*
 * Group-parallel epochs (default on): a cost_aware best-fit round of several groups walks
 * consecutive groups of distinct anchor zones side by side, each on the epoch's start state,
 * and keeps exactly the prefix the sequential order would have produced (a group is rejected,
 * and walked again in the next epoch, if a host an earlier group committed to is its winner or
 * beats it); results are identical either way. Replaces the group loop of
 * scheduler/cost_aware.py:37-42 around _best_fit (:63-97).
 * Rounds of 33 to PVT_MAX_ZONES zones plan epochs when they are unsharded and have no rt_bw
 * (host-sharded and rt_bw wide rounds, and every wide round under PVT_ZW_WIDE=0, take the
 * pipelined list windows).
 * pvt_epoch_stats: epochs run, segments walked and segments rejected in the last pvt_place.
 */
int  pvt_set_epochs(pvt_ctx* ctx, int on);
int  pvt_epoch_stats(pvt_ctx* ctx, int64_t* epochs, int64_t* segments, int64_t* rejected);
/*
 * Zero-cost frontier walk (default on; results identical either way): an epoch chain whose
 * tasks all find a zero-egress-cost host (score exactly 0) among the first 1024 hosts of its
 * zones is walked as a first fit over those hosts in LDS, with no candidate lists; the walk
 * proves each winner exact (pvt_zwalk.hip) and leaves any chain it cannot prove to the
 * list-based walk. In a round of 33 to PVT_MAX_ZONES zones (unsharded, no rt_bw) a chain is
 * walked when its anchors' zero-cost component has at most 32 zones; chains of larger
 * components, host-sharded and rt_bw wide rounds and the resident kernels' one-wave walks are
 * not (PVT_ZW_WIDE=0 at pvt_ctx_create: no wide round is). pvt_zero_walk_stats: chains of the last pvt_place walked each way, and the
 * tasks of each epoch's longest chain (summed over its epochs: the walks' critical path).
 */
int  pvt_set_zero_walk(pvt_ctx* ctx, int on);
int  pvt_zero_walk_stats(pvt_ctx* ctx, int64_t* frontier_chains, int64_t* list_chains,
                         int64_t* longest_chain);
/*
 * Frontier chains of the last pvt_place that took the walk's fast prologue (group certificates
 * from the order launch instead of a pass over the chain's demand rows; PVT_CHAIN_CERT=0 at
 * context creation turns it off; results identical either way).
 */
int  pvt_prologue_stats(pvt_ctx* ctx, int64_t* fast_chains);
/* Counters of the last pvt_place call: windows run and refills forced by exhausted lists. */
int  pvt_last_stats(pvt_ctx* ctx, int64_t* windows, int64_t* refills);
/*
 * The resident kernel instance of the context's last resident launch (pvt_place_batch, pvt_place
 * and the host-array calls on rounds within the resident limits): the waves of a round's
 * workgroup, the hosts per lane, whether a wide kernel ran (a round of more than 32 zones whose
 * policy reads the zone tables), and the A/B switches as they took effect, in the bit values of
 * PVT_RWALK (1, 2, 4, 8: the one-wave walks, cleared for batches with a round of more than 1024
 * hosts and for wide kernels; 16, 32, 64 and the list minimum in bits 8-15: the multi-wave path).
 * PVT_RES_WAVES (1, 2, 4 or 8; default 4) and PVT_RWALK are read at pvt_ctx_create and are for
 * A/B runs; results are identical under every value. All zeros before the first resident
 * launch. A NULL output is skipped.
 */
int  pvt_last_resident_shape(pvt_ctx* ctx, int32_t* waves, int32_t* hosts_per_lane, int32_t* wide,
                             uint32_t* switches);
/*
 * Host-dimension sharding (BASELINE config 5): `world` ranks (one per GPU)
 * each score a contiguous host range [host_lo, host_hi) and exchange per-task candidate
 * packages once per window; every rank then runs the same commit walk, so placements are
 * identical on all ranks and equal to pvt_place(). Each rank keeps the FULL availability array
 * (32 B per host, replicated and updated identically by the walk); only scoring is split.
 * The exchange is the caller's (an all-gather, e.g. RCCL through torch.distributed):
 *
 *   pvt_shard_begin(ctx, r, lo, hi, world, &max_bytes)     allocate send [max_bytes] and
 *                                                          recv [world * max_bytes] (device)
 *   loop:
 *     pvt_shard_score(ctx, send, &nt, &bytes)              nt == 0: the round is done
 *     all-gather `bytes` from every rank into recv, rank order, contiguous (recv[k*bytes..])
 *     pvt_shard_commit(ctx, recv)                          PVT_ESTALE: score again
 *
 * pvt_shard_commit launches the window's commit walk and returns without waiting for it
 * (pvt_set_pipeline on, the default): the next pvt_shard_score scores the following window on
 * a side stream while the walk runs and returns its package (complete on return), so the
 * caller's exchange -- issued on a stream that does not wait for the context's stream -- also
 * overlaps the walk. If that walk stops early the speculative package is stale: the next
 * pvt_shard_commit returns PVT_ESTALE on every rank and the caller scores again. With the
 * pipeline off every call completes its window before returning.
 * Opportunistic rounds shard by whole super-chunks of 16384 hosts: rank r of world W must take
 * hosts [r * P * 16384, (r + 1) * P * 16384) clamped to H, P = ceil(ceil(H / 16384) / W); the
 * packages carry its per-task feasibility bitmaps and super-chunk counts and every rank runs the
 * same draw / selection walk (windows of 256 tasks, not pipelined).
 *
 * `r` and its arrays must stay valid until the round is done. nt and bytes are the same on
 * every rank (window sizes depend only on walk results, which every rank shares).
 * Replaces the per-task scan of scheduler/cost_aware.py:88-92,
 * :118-122 and scheduler/vbp.py:19-22, :43-47 over a cluster too large for one GPU's pass.
 */
#define PVT_SHARD_MAX_WORLD 64
int  pvt_shard_begin(pvt_ctx* ctx, const pvt_round* r, int32_t host_lo, int32_t host_hi,
                     int32_t world, int64_t* max_package_bytes);
int  pvt_shard_score(pvt_ctx* ctx, void* package, int32_t* n_tasks, int64_t* package_bytes);
int  pvt_shard_commit(pvt_ctx* ctx, const void* packages);
/*
 * Resident rounds and scenario batches (BASELINE configs 1, 2 and 4; SURVEY.md §8(e), §8(f)
 * rank 2). A round with n_hosts <= PVT_RESIDENT_MAX_HOSTS and n_tasks <= PVT_RESIDENT_MAX_TASKS
 * fits one workgroup: its hosts stay in registers for the whole round and every task rescans
 * them (the reference's loop, restated). pvt_place_batch() runs n such rounds of ONE policy
 * (rounds[i].mode all equal) in a single launch, one workgroup per round, so independent
 * scenarios' rounds run side by side on all CUs. `rounds` is a HOST array of descriptors whose
 * array pointers are device pointers, exactly as for pvt_place() (mt_state in host memory);
 * each round is placed exactly as pvt_place() would place it. Synchronises before returning.
 * Returns PVT_EUNSUPPORTED if a round exceeds the limits (use pvt_place for it).
 * A cost_aware round of more than 32 zones, and every round of a mixed-policy batch that holds
 * a round of more than 32 zones, is resident up to PVT_RESIDENT_WIDE_MAX_HOSTS hosts (the wide
 * kernels hold at most 8 hosts per lane); pvt_place and pvt_place_host run larger ones on the
 * windowed engine.
 *
 * pvt_set_resident(ctx, max_hosts): pvt_place() runs rounds with n_hosts <= max_hosts (and
 * n_tasks within the limit) as a batch of one; 0 disables it (the windowed score/commit path
 * runs every round). Default PVT_RESIDENT_MAX_HOSTS. Results are identical either way.
 */
#define PVT_RESIDENT_MAX_HOSTS 4096
#define PVT_RESIDENT_WIDE_MAX_HOSTS 2048
#define PVT_RESIDENT_MAX_TASKS 4096
int  pvt_place_batch(pvt_ctx* ctx, const pvt_round* rounds, int32_t n_rounds);
/* pvt_place_batch with the rounds' MT19937 states resident on the device: mt_dev[n_rounds][625]
 * (in/out, key then pos, as mt_state), so no state crosses PCIe; the rounds' mt_state fields are
 * ignored. The scenario-batch driver (config 4) keeps its states on the device across rounds. */
int  pvt_place_batch_mt(pvt_ctx* ctx, const pvt_round* rounds, int32_t n_rounds, uint32_t* mt_dev);
int  pvt_set_resident(pvt_ctx* ctx, int32_t max_hosts);
/*
 * Anchor resolution for cost_aware groups (replaces the Counter/max of
 * CostAwareGlobalScheduler._group_tasks, scheduler/cost_aware.py:45-58).
 *
 * Item c (a container of ready tasks) has the predecessor list list[off[c] .. off[c+1]): the
 * placement of every task of every predecessor container, in the reference's iteration order
 * (app.get_predecessors(c.id) order = the container's `dependencies` order, application/
 * __init__.py:87-92,137-139; then p.tasks order). An entry is a host index (-1 = a predecessor
 * task without placement), or, when inst_host is set, an index into inst_host (a per-instance
 * host table kept resident in HBM, e.g. pivot_place.trace.DeviceTrace).
 * Outputs per item: mode_host = the host with the highest count, the first seen among equal
 * counts (Counter insertion order + max's first maximum); anchor_zone = zone[mode_host], or
 *   -1  empty list (the task groups by its application, cost_aware.py:56-57),
 *   -2  the mode entry is -1 (the reference raises AttributeError on get_host(None).locality),
 *   -3  invalid row, offsets or index out of range (the call then returns PVT_EINVAL).
 * With `item` set, item c uses row item[c] of a resident list table instead: its list is
 * list[off[item[c]] .. off[item[c]+1]) (off then has n_rows + 1 entries), so a trace kept in
 * HBM uploads only the ready containers' row numbers per round.
 * All pointers are device pointers. Lists may hold up to 2^30 entries. Synchronises before
 * returning.
 */
typedef struct pvt_anchor_args {
  int32_t n_items;            /* C                                                        */
  int32_t n_hosts;            /* H                                                        */
  int64_t n_pred;             /* length of list                                           */
  int64_t n_inst;             /* length of inst_host (0 when inst_host is NULL)           */
  const int64_t* off;         /* [C+1], or [n_rows+1] when item is set                    */
  const int32_t* list;        /* [n_pred]                                                 */
  const int32_t* inst_host;   /* [n_inst] or NULL                                         */
  const int32_t* zone;        /* [H]                                                      */
  int32_t* mode_host;         /* [C] out                                                  */
  int32_t* anchor_zone;       /* [C] out                                                  */
  const int32_t* item;        /* [C] row of off per item, or NULL (item c = row c)        */
  int64_t n_rows;             /* rows of off when item is set (0 when item is NULL)       */
} pvt_anchor_args;
int  pvt_anchor(pvt_ctx* ctx, const pvt_anchor_args* a);

/*
 * Drop-in round from HOST memory in one round trip (the reference's synchronous schedule()
 * call, scheduler/__init__.py:100-103). Every array pointer of r is a HOST pointer: avail
 * in/out, placement and order out, mt_state in/out. The context packs the inputs into its
 * pinned staging buffer, copies them to the device with ONE copy, places the round, and copies
 * avail, placement, order and the MT19937 states back with ONE copy and one synchronisation.
 * On error the outputs are left untouched.
 *
 * cost_aware rounds may pass `items` and leave task_group / group_anchor NULL: the grouping of
 * scheduler/cost_aware.py:30-58 then runs on the device in the same round trip -- per item the
 * mode host of its predecessor placements (as pvt_anchor), groups keyed by the storage of that
 * host's zone or, for items without predecessors, by their application, numbered in first-seen
 * task order, and one randomizer.choice(storage) per application group, in group order, from
 * items->mt_state (the policy's RandomState; in/out). items->status[0] returns the number of
 * groups, status[1] an error kind with PVT_EINVAL: 1 a mode placement that is not a host of the
 * cluster, 2 a zone without storage (the reference raises AttributeError for both), 3 malformed
 * item lists. Rounds beyond the fused grouping's limits (T > 16384, n_storage + n_apps > 8192)
 * return PVT_EUNSUPPORTED before any work (the caller then uses pvt_anchor + pvt_place).
 */
typedef struct pvt_ca_items {
  int32_t n_items;             /* C: distinct containers of the ready tasks                 */
  int32_t n_apps;              /* applications of the items (item_app in [0, n_apps))        */
  int64_t n_pred;              /* length of pred_host                                       */
  const int32_t* task_item;    /* [T] item of each task                                     */
  const int64_t* pred_off;     /* [C+1] item c's predecessor placements pred_off[c..c+1)     */
  const int32_t* pred_host;    /* [n_pred] host index of each placement, -1 = not a host     */
  const int32_t* item_app;     /* [C] application of each item                               */
  int32_t n_storage;           /* S = len(cluster.storage)                                   */
  int32_t reserved;            /* must be 0                                                  */
  const int32_t* storage_zone; /* [S] zone of each storage, cluster.storage order            */
  const int32_t* zone_storage; /* [Z] storage index of get_storage_by_locality(zone), -1 None */
  uint32_t* mt_state;          /* [625] in/out: the policy randomizer (MT19937 key + pos)    */
  int32_t* status;             /* [2] out: groups formed, error kind                         */
} pvt_ca_items;
int  pvt_place_host(pvt_ctx* ctx, pvt_round* r, pvt_ca_items* items);
/*
 * Several independent drop-in rounds from HOST memory in one round trip: the lock-step driver's
 * tick, where simulations running different policies each wait on one schedule() round
 * (scheduler/__init__.py:100-103 once per simulation). rounds[i] is as for pvt_place_host, with
 * items[i] its optional fused cost_aware grouping (items itself may be NULL); the policies may
 * differ between rounds. Every round with tasks must fit the resident limits (n_hosts <=
 * min(pvt_set_resident limit, PVT_RESIDENT_MAX_HOSTS), n_tasks <= PVT_RESIDENT_MAX_TASKS) --
 * else PVT_EUNSUPPORTED before any work. One staging copy up, one launch for all rounds (one
 * workgroup each), one copy back, one synchronisation. rcs[i] receives each round's own result
 * (PVT_OK, or PVT_EINVAL with items[i]->status[1] set for a grouping error, its outputs then
 * untouched); the call returns PVT_OK when the batch ran.
 */
int  pvt_place_host_batch(pvt_ctx* ctx, pvt_round* rounds, pvt_ca_items* const* items,
                          int32_t n_rounds, int32_t* rcs);

/*
 * Replay support (no reference counterpart): avail[r][h] = avail0[r][h], r = 0..3, for every
 * h = hosts[i], i < n, with 0 <= h < n_hosts (other entries are ignored), on the context's
 * stream; device pointers. A round placed again from the same snapshot needs only the hosts
 * its placement names restored -- a round changes no other capacity -- so passing the round's
 * placement array as `hosts` resets it in one small launch instead of a copy of all 4 x H.
 */
int  pvt_restore_hosts(pvt_ctx* ctx, double* avail, const double* avail0, int32_t n_hosts,
                       const int32_t* hosts, int32_t n);

/*
 * Meter aggregates of a batch of S scenarios (replaces the properties
 * Meter.cumulative_instance_hours, .total_network_traffic_cost and .average_congestion_delay,
 * resources/meter.py:31-53, read by alibaba/runner.py:45-51 via Meter.save).
 *
 * The logs are nested CSR arrays in the meter's own dict orders:
 *   scenario s -> hosts  host_off[s] .. host_off[s+1]          (Meter.__hosts)
 *   host h     -> intervals iv_off[h] .. iv_off[h+1]: [iv_start, iv_end] (check-in/out)
 *   scenario s -> routes route_off[s] .. route_off[s+1]        (Meter.__routes)
 *   route r    -> packets pkt_off[r] .. pkt_off[r+1]; route_cost[r] = cost[src.loc, dst.loc]
 *   packet p   -> transfers tr_off[p] .. tr_off[p+1]: [tr_start, tr_end, tr_size]
 * Per scenario: instance_hours = sum_h sum_v (end - start) / 3600; egress_cost = sum_r
 * route_cost * (sum_p sum_t size) / 8000 (ResourceMetadata.calc_network_traffic_cost,
 * resources/__init__.py:565-569); congestion_delay = sum over consecutive transfers of a packet
 * of (start_i - end_{i-1}) / #packets, 0 without packets. Per host and per route the sums run
 * in the reference's order; across hosts / routes a fixed tree (fp64, within 1e-9 relative of
 * the reference's left-to-right sum). All pointers are device pointers. Returns PVT_EINVAL if an
 * offset is out of range. Synchronises before returning.
 */
typedef struct pvt_meter_log {
  int32_t n_scen;             /* S                                                        */
  int32_t reserved;           /* must be 0                                                */
  int64_t n_host_rows, n_iv, n_routes, n_pkts, n_tr;   /* lengths of the level arrays    */
  const int64_t* host_off;    /* [S+1]                                                    */
  const int64_t* iv_off;      /* [n_host_rows+1]                                          */
  const double* iv_start;     /* [n_iv]                                                   */
  const double* iv_end;       /* [n_iv]                                                   */
  const int64_t* route_off;   /* [S+1]                                                    */
  const double* route_cost;   /* [n_routes]                                               */
  const int64_t* pkt_off;     /* [n_routes+1]                                             */
  const int64_t* tr_off;      /* [n_pkts+1]                                               */
  const double* tr_start;     /* [n_tr]                                                   */
  const double* tr_end;       /* [n_tr]                                                   */
  const double* tr_size;      /* [n_tr]                                                   */
  double* instance_hours;     /* [S] out                                                  */
  double* egress_cost;        /* [S] out                                                  */
  double* congestion_delay;   /* [S] out                                                  */
} pvt_meter_log;
int  pvt_meter(pvt_ctx* ctx, const pvt_meter_log* m);

/*
 * Meter usage series of a batch of S scenarios: the reference's series, Meter.plot_host_usage
 * (resources/meter.py:135-148; Meter.save writes it to host_usage.json on every run, :128-133,
 * alibaba/runner.py:46), Meter.plot_resource_usage (:150-159) and the five get_avg_*_usage
 * (:161-179). With s = sample_size, bucket b is the time range [b*s, (b+1)*s).
 *
 * Inputs: hosts and intervals exactly as in pvt_meter_log; host h's usage records
 * us_off[h] .. us_off[h+1] in time order (Meter.__usage, one record per resource at every host
 * check-in / check-out, :181-187): us_time[u] and the four fractions us_frac[r * n_us + u],
 * r = 0 cpus, 1 mem, 2 disk, 3 gpus. us_off, us_time and us_frac all NULL with n_us = 0: no
 * resource series (res_hosts, res_mean and avg[1..4] are then not written). The caller sizes the
 * output rows: scenario s owns buckets bucket_off[s] .. bucket_off[s+1] (nb_s of them) of the
 * dense outputs, bucket_off[0] = 0, bucket_off[S] = n_buckets.
 *
 * Outputs, per scenario and bucket b < nb_s (every entry of a row is written):
 *   n_hosts[bucket_off[s] + b]   hosts with an interval [start, end] that has
 *                                start // s <= b <= end // s - 1: the bucket that holds `end` is
 *                                not counted and an interval inside one bucket counts nowhere
 *                                (:139-145). 0 = a bucket the reference's series leaves out.
 *   res_hosts[bucket_off[s] + b] hosts with a record in b (time // s == b); 0 = left out.
 *   res_mean[r * n_buckets + bucket_off[s] + b]   mean over those hosts of the mean of the
 *                                host's values of resource r in b (:155-156); 0 when left out.
 *   avg[s * 5 + k]               mean over the buckets not left out of n_hosts (k = 0) and of
 *                                res_mean of resource k - 1 (k = 1..4); NaN without such a bucket.
 * The integer outputs and avg[.. + 0] are exact; the means sum in another order than numpy
 * (fp64, within 1e-9 relative; every term is non-negative). No floating-point atomics: a call's
 * result does not depend on scheduling or on the other scenarios of the batch.
 *
 * Contract (PVT_EINVAL on a violation, with the number of violating scenarios in
 * pvt_last_error; output contents are then unspecified): offsets in range and non-decreasing;
 * every time finite with 0 <= t < 2^52; per host end >= start and start[i+1] >= end[i] (the
 * meter's own order, :59-81) and us_time non-decreasing; the bucket of every interval start,
 * interval end and record time lies below nb_s. 1 <= sample_size <= 2^31 - 1 (integral: then
 * floor(floor(t) / s) in int64 is Python's float t // s). All pointers are device pointers.
 * Synchronises before returning.
 */
typedef struct pvt_usage_log {
  int32_t n_scen;             /* S                                                        */
  int32_t reserved;           /* must be 0                                                */
  int64_t sample_size;        /* s                                                        */
  int64_t n_host_rows;        /* hosts of all scenarios                                   */
  int64_t n_iv;               /* intervals of all hosts                                   */
  int64_t n_us;               /* usage records of all hosts                               */
  int64_t n_buckets;          /* buckets of all scenarios                                 */
  const int64_t* host_off;    /* [S+1]                                                    */
  const int64_t* iv_off;      /* [n_host_rows+1]                                          */
  const double* iv_start;     /* [n_iv]                                                   */
  const double* iv_end;       /* [n_iv]                                                   */
  const int64_t* us_off;      /* [n_host_rows+1] or NULL                                  */
  const double* us_time;      /* [n_us]                                                   */
  const double* us_frac;      /* [4 * n_us]                                               */
  const int64_t* bucket_off;  /* [S+1]                                                    */
  int32_t* n_hosts;           /* [n_buckets] out                                          */
  int32_t* res_hosts;         /* [n_buckets] out                                          */
  double* res_mean;           /* [4 * n_buckets] out                                      */
  double* avg;                /* [5 * S] out                                              */
} pvt_usage_log;
int  pvt_meter_usage(pvt_ctx* ctx, const pvt_usage_log* u);

/*
 * Resident cluster state: a log of subscribe / unsubscribe ops applied to the hosts' levels on
 * the device, by the rules of the reference's host accounting (HostResource.subscribe,
 * resources/__init__.py:433-449, and HostResource.unsubscribe, :451-461, over SimPy containers;
 * cpus_used etc. are `capacity - level`, :401-415). A caller that simulates many rounds keeps
 * `level` on the device and sends the few thousand ops between two rounds instead of a new
 * 4 x H snapshot.
 *
 * State: capacity[r * H + h] (constant) and level[r * H + h] (in/out), fp64, in the layout of
 * pvt_round.avail, r = 0 cpus, 1 mem, 2 disk, 3 gpus. The log holds K ops in event order:
 * op_host[k], op_kind[k] (0 subscribe, 1 unsubscribe) and the amounts d_r = op_amt[r * K + k].
 * The ops of one host are applied in log order; ops of different hosts are independent.
 *
 *   subscribe(d)    refused if, for any r, d_r > level_r or d_r < 0 (:436-440): op_ok[k] = 0 and
 *                   nothing changes. Otherwise level_r -= d_r for every r with d_r > 0
 *                   (:441-448) and op_ok[k] = 1.
 *   unsubscribe(d)  independently for each r: if 0 < d_r and d_r <= capacity_r - level_r (the
 *                   subtraction rounded once, in fp64), then level_r += d_r (:454-461).
 *                   op_ok[k] = the mask of the resources put back (bit r). A put-back that
 *                   misses the test by an ulp is skipped, as in the reference.
 *
 * The compares are IEEE compares, so NaN, infinite and negative amounts behave as in Python (a
 * NaN amount passes the subscribe test and changes nothing). One rounding per add or subtract,
 * no contraction, no floating-point atomics: the result is bit-identical across calls and does
 * not depend on how a log is cut into calls.
 *
 * PVT_EINVAL when an op names a host outside [0, H) or a kind other than 0 or 1; pvt_last_error
 * names the first such op, and neither level nor op_ok is written. Runs on the context's stream
 * and synchronises before returning; n_ops = 0 returns PVT_OK without a launch. All pointers
 * are device pointers. Timed under the name "host_ops_kernel" (pvt_get_kernel_kstats).
 */
typedef struct pvt_host_ops {
  int32_t n_hosts, n_ops;     /* H >= 1, K >= 0                                           */
  const double* capacity;     /* [4 * H]                                                  */
  double* level;              /* [4 * H] in/out                                           */
  const int32_t* op_host;     /* [K]                                                      */
  const int32_t* op_kind;     /* [K] 0 subscribe, 1 unsubscribe                           */
  const double* op_amt;       /* [4 * K]                                                  */
  int32_t* op_ok;             /* [K] out                                                  */
} pvt_host_ops;
int  pvt_host_ops_apply(pvt_ctx* ctx, const pvt_host_ops* ops);

/*
 * Realtime-bandwidth rows built on the device: pvt_round.rt_bw of a cost_aware round with
 * realtime_bw (scheduler/cost_aware.py:73-79,106-112) from the zone table and a sparse list of
 * route queues, so that a resident cluster uploads O(listed routes + packets) bytes per round
 * and no dense [G*H] array.
 *
 * The rule (resources/network.py:70-73): a route's realtime bandwidth is
 *     est = (Q + 1) / bw;   est ? 1 / est : bw
 * with Q the sum of its queued packets' MB, added left to right in queue order, from 0, in fp64
 * (the sum depends on the order, and _transfer rotates the queue, :99-100), and bw the route's
 * own bandwidth. Both divisions are performed: an idle route's value is 1 / (1 / bw), which is
 * not bw for about one bw in nine. A NaN est takes the division, as in Python.
 *
 *     rt_bw[g*H + h] = in + out      (in that order), a = group_anchor[g]
 *     in   the value of the listed route (a, h, dir 0: storage -> host, the reference's in_route),
 *          or of an empty queue on bw[a*Z + zone[h]] when it is not listed
 *     out  likewise for (a, h, dir 1: host -> storage, out_route) and bw[zone[h]*Z + a]
 * G = 0 (group_anchor ignored) gives the one row of zone 0, pvt_round.rt_bw's convention for a
 * round without task_group. Groups that share an anchor get equal rows; an entry whose anchor
 * is no group's is checked and stores nothing.
 *
 * The list: R entries sorted by (rq_anchor, rq_host, rq_dir), strictly ascending (no
 * duplicates), with 0 <= rq_anchor < Z, 0 <= rq_host < H, rq_dir 0 or 1, rq_bw > 0 (NaN fails;
 * the reference raises on 0); entry i's packets are rq_mbs[rq_off[i] .. rq_off[i+1]), each > 0
 * (NaN fails; Packet.__init__ asserts it), with rq_off[0] = 0, rq_off non-decreasing and
 * rq_off[R] = n_packets. An entry without packets is legal (a route replaced by one of another
 * bandwidth). Infinite values are allowed and follow IEEE. group_anchor[g] and zone[h] lie in
 * [0, Z).
 *
 * PVT_EINVAL, with rt_bw untouched, when the list breaks the contract (pvt_last_error names the
 * first such entry), or a group_anchor[g] or a zone[h] is out of range. R = 0 fills idle rows
 * only. IEEE divisions, no contraction, no floating-point atomics: equal bits on every call.
 * Runs on the context's stream and synchronises before returning. All pointers are device
 * pointers. The pass that streams the rows is timed under the name "rt_fill_kernel"
 * (pvt_get_kernel_kstats; its bytes: G*H*8 written + ceil(G/8)*H*4 read).
 */
typedef struct pvt_route_queues {
  int32_t n_hosts, n_zones, n_groups, n_routes;  /* H >= 1, 1 <= Z <= PVT_MAX_ZONES, G >= 0 (0: one row, zone 0), R >= 0 */
  const int32_t* zone;          /* [H]            */
  const double*  bw;            /* [Z*Z]          */
  const int32_t* group_anchor;  /* [G] or NULL    */
  const int32_t* rq_anchor;     /* [R]            */
  const int32_t* rq_host;       /* [R]            */
  const int32_t* rq_dir;        /* [R]            */
  const double*  rq_bw;         /* [R]            */
  const int64_t* rq_off;        /* [R+1]          */
  const double*  rq_mbs;        /* [rq_off[R]]    */
  int64_t n_packets;            /* P, the caller's count: rq_off[R] must equal it */
  double* rt_bw;                /* [max(G,1)*H] out */
} pvt_route_queues;
int  pvt_rt_rows(pvt_ctx* ctx, const pvt_route_queues* q);

/*
 * Metering the resident cluster: the reference Meter's host half (Meter.host_check_in,
 * resources/meter.py:59-69, Meter.host_check_out, :71-81, and _track_resource_usage, :181-187)
 * run from the op log, on the levels the device already holds. The log of pvt_host_ops gains a
 * time per entry, op_time[k], and two kinds: 2 = check-in and 3 = check-out of op_host[k] at
 * op_time[k] (the amounts of a mark are ignored). Kinds 0 and 1 are as in pvt_host_ops_apply.
 * Entries of one host apply in log order; hosts are independent.
 *
 * Per host the meter state is the last element of Meter.__hosts[h]: st_word[h] = 0 none,
 * 1 open(start), 2 closed(start, end), with st_start[h] and st_end[h] (0 where not defined). A
 * mark first records usage -- frac_r = (capacity_r - level_r) / capacity_r, one fp64 subtraction
 * and one division, at the levels as they stand at that point of the host's log -- into the
 * usage log, then runs the state machine; op_ok[k] receives the row's code:
 *
 *   check-in   none               open(t)                                              1
 *              closed, t >  end   the closed interval goes to the interval log; open(t) 2
 *              closed, t <= end   open(start) (the reference pops the end)             3
 *              open               nothing                                              4
 *   check-out  open               closed(start, t)                                     1
 *              closed, t >  end   closed(start, t)                                     2
 *              closed, t <= end   nothing                                              3
 *              none               nothing (the reference raises, after the record)     0
 *
 * The two append logs are caller-owned device arrays of iv_cap and us_cap records: final
 * intervals (iv_host, iv_start, iv_end) and usage records (us_host, us_time, and the four
 * fractions record-major, us_frac[4 * i + r], so growing a log is a plain copy of its front).
 * n_iv, n_us (the logs' counts) and last_time (the time of the last entry applied) are host-side
 * in/out fields; a fresh meter has all three 0 and the per-host arrays zeroed. One host's records
 * keep their log order in the raw logs, within a call and across calls; records of different
 * hosts are in no particular order there (pvt_host_meter_finish orders them). Slots are taken
 * with integer atomics; there are no floating-point atomics.
 *
 * pvt_host_meter_apply: PVT_EINVAL before any launch when n_iv + K > iv_cap or n_us + K > us_cap
 * (a call appends at most K records to each; the caller grows the logs). PVT_EINVAL, naming the
 * first offending entry in pvt_last_error and writing nothing (level, state, logs, counts, op_ok),
 * when an entry has a host outside [0, H), a kind outside 0..3, a time that is not finite with
 * 0 <= t < 2^52, a time below its predecessor's or (entry 0) below last_time, or a host with a
 * capacity that is not > 0 in all four resources. Runs on the context's stream and synchronises
 * before returning; the segment walk is timed under the name "host_meter_kernel". All array
 * pointers are device pointers.
 */
typedef struct pvt_host_meter {
  int32_t n_hosts, reserved;  /* H >= 1; must be 0                                        */
  const double* capacity;     /* [4 * H]                                                  */
  double* level;              /* [4 * H] in/out                                           */
  int32_t* st_word;           /* [H] in/out                                               */
  double* st_start;           /* [H] in/out                                               */
  double* st_end;             /* [H] in/out                                               */
  int64_t iv_cap, us_cap;     /* records the logs can hold                                */
  int32_t* iv_host;           /* [iv_cap]                                                 */
  double* iv_start;           /* [iv_cap]                                                 */
  double* iv_end;             /* [iv_cap]                                                 */
  int32_t* us_host;           /* [us_cap]                                                 */
  double* us_time;            /* [us_cap]                                                 */
  double* us_frac;            /* [4 * us_cap] record-major                                */
  int64_t n_iv, n_us;         /* host-side in/out: records in the logs                    */
  double last_time;           /* host-side in/out                                         */
} pvt_host_meter;
typedef struct pvt_host_meter_ops {
  int32_t n_ops, reserved;    /* K >= 0; must be 0                                        */
  const int32_t* op_host;     /* [K]                                                      */
  const int32_t* op_kind;     /* [K] 0 subscribe, 1 unsubscribe, 2 check-in, 3 check-out  */
  const double* op_amt;       /* [4 * K] as in pvt_host_ops                               */
  const double* op_time;      /* [K] non-decreasing                                       */
  int32_t* op_ok;             /* [K] out                                                  */
} pvt_host_meter_ops;
int  pvt_host_meter_apply(pvt_ctx* ctx, pvt_host_meter* m, const pvt_host_meter_ops* ops);

/*
 * The metered run so far in the layout pvt_meter_log and pvt_usage_log take (one scenario:
 * host_off = {0, n_rows}). Non-destructive: it reads the meter and writes `out` only, so the
 * caller may go on applying and finish again. Every host's last interval is taken as final; a
 * host whose last interval is open gives PVT_EINVAL with the number of such hosts and the first
 * in pvt_last_error (the reference's own properties raise on it), `out` then unspecified.
 *
 * capacity and level are not read and may be NULL here.
 *
 * Rows are the hosts with at least one usage record in HOST-INDEX order -- not the meter's dict
 * order (first check-in). The series' integer outputs do not depend on the order of the rows;
 * the means stay within the 1e-9 relative pvt_meter_usage states. Row i: host row_host[i], its
 * intervals iv_off[i] .. iv_off[i+1] and records us_off[i] .. us_off[i+1], both in log order,
 * with the fractions resource-major, us_frac[r * n_us + u]. The result is bit-identical from run
 * to run and however the log was cut into calls.
 *
 * The caller sizes the arrays before the call from the meter's counts: n_us is exact
 * (m->n_us), n_rows <= min(H, m->n_us), n_iv <= m->n_iv + min(H, m->n_us); the offset arrays
 * hold one more than the row bound. The counts are returned in the struct. Runs on the context's
 * stream and synchronises before returning. All array pointers are device pointers.
 */
typedef struct pvt_host_meter_out {
  int32_t* row_host;          /* [R] out                                                  */
  int64_t* iv_off;            /* [R+1] out                                                */
  double* iv_start;           /* [n_iv] out                                               */
  double* iv_end;             /* [n_iv] out                                               */
  int64_t* us_off;            /* [R+1] out                                                */
  double* us_time;            /* [n_us] out                                               */
  double* us_frac;            /* [4 * n_us] out, resource-major                           */
  int64_t n_rows, n_iv, n_us; /* host-side out                                            */
} pvt_host_meter_out;
int  pvt_host_meter_finish(pvt_ctx* ctx, const pvt_host_meter* m, pvt_host_meter_out* out);

/*
 * Opt-in validation of a round's CONTENTS (no reference counterpart). The placement entry points
 * validate sizes, the mode and NULL pointers only and trust what the arrays hold -- zone, group
 * and anchor values index tables directly, and the kernels order keys by their bits -- so a caller
 * that is being brought up can ask first. The rules are numbered as enum pvt_check and stated at
 * the pvt_round fields they bind. A rule applies only where the engine reads the array.
 *
 * pvt_check_round / pvt_check_batch validate the round's structure as pvt_place does (PVT_EINVAL
 * and friends as there), then run one check kernel over the arrays of all n rounds on the
 * context's stream, synchronise, and return PVT_OK with one verdict per round in `out`. They read
 * the rounds' input arrays only and test every index before using it; they never touch order or
 * placement and never write avail. mt_state (rule 11) is read on the host.
 *
 * pvt_set_checks(ctx, 1): pvt_place, pvt_place_batch, pvt_place_batch_mt (its device-resident
 * MT19937 states are not read: rules 1-10), pvt_shard_begin, pvt_place_host and
 * pvt_place_host_batch check first. On a violation they launch no placement kernel, write no
 * output and return PVT_EINVAL. pvt_last_error names the rule, the index and the value (for the
 * host batch rcs[i] carries each round's own result). Host-array calls check on the host, with
 * the same predicates, before staging. Off (the default): no entry point issues an extra launch,
 * copy or synchronisation.
 */
enum pvt_check {
  PVT_CHK_OK = 0,
  PVT_CHK_ZONE = 1,
  PVT_CHK_AVAIL = 2,
  PVT_CHK_DEM = 3,
  PVT_CHK_GROUP = 4,
  PVT_CHK_ANCHOR = 5,
  PVT_CHK_COST = 6,      /* flat index a*Z + z of the zone pair (a, z)                     */
  PVT_CHK_BW = 7,        /* as PVT_CHK_COST                                                */
  PVT_CHK_RTBW = 8,
  PVT_CHK_DECAY = 9,
  PVT_CHK_TIEBREAK = 10,
  PVT_CHK_MTPOS = 11     /* index 624                                                      */
};
typedef struct pvt_check_report {
  int32_t code;     /* lowest-numbered violated rule, 0 = none                    */
  int32_t mask;     /* bit k set: rule k is violated                              */
  int64_t index;    /* lowest violating flat index of rule `code` (-1 when ok)    */
  int64_t count;    /* violating elements of rule `code`                          */
  double  value;    /* the element at `index` (ints converted; rules 6/7: the sum) */
} pvt_check_report;
int  pvt_check_round(pvt_ctx* ctx, const pvt_round* r, pvt_check_report* out);
int  pvt_check_batch(pvt_ctx* ctx, const pvt_round* rounds, int32_t n, pvt_check_report* out);
int  pvt_set_checks(pvt_ctx* ctx, int on);   /* default 0 */

/* Human-readable text of the last error on this context (static storage of the ctx). */
const char* pvt_last_error(pvt_ctx* ctx);

#ifdef __cplusplus
}
#endif

#endif /* PIVOT_PLACE_H */
