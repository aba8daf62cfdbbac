// pvt_shard.hip — host-sharded rounds (pvt_shard_begin / score / commit): each rank scores its
// host range, the caller exchanges the packages, every rank runs the same walk.
#include "pvt_driver.h"
#include "pvt_opp.h"

// ---------------------------------------------------------------- host-dimension sharding
static int shard_depth(int world) { return std::max(KL, LMAX / std::max(world, 1)); }
static int64_t frontier_pkg_bytes(int nslots) {
  return (int64_t)sizeof(FrontierHdr) + (int64_t)sizeof(FrontierSlot) * nslots;
}

// ---- host-sharded opportunistic rounds (per-rank feasible counts, exchanged;
// the draw and the k-th selection replicated). Each rank counts its super-chunks of a window
// (bitmaps + counts, task-major) into its package; after the all-gather every rank unpacks the
// full tables and runs the same commit walk, so placements, availability and the MT19937 state
// are identical on all ranks and equal to pvt_place()'s.
static constexpr int OPP_SHARD_WINDOW = OPP_WINDOW_DEFAULT;
static constexpr int OPP_SUP_HOSTS = OPP_SUP * OPP_CH;

static size_t opp_pkg_bytes(const RoundState& R, int nt) {
  return (size_t)nt * R.opp_Psq * OPP_SUP * 4 * sizeof(uint64_t) + (size_t)nt * R.opp_Psq * sizeof(int32_t);
}
static size_t opp_table_bytes(const RoundState& R) {   // full bitmaps + counts of one window
  return (((size_t)R.opp_W * R.opp_nq * 4 * sizeof(uint64_t) + (size_t)R.opp_W * R.opp_nsq * sizeof(int32_t)) + 255) / 256 * 256;
}

static int opp_shard_begin(pvt_ctx* ctx, const pvt_round* r, int lo, int hi, int world,
                           int64_t* max_package_bytes) {
  RoundState& R = ctx->rs;
  const int H = r->n_hosts, T = r->n_tasks;
  if (!r->mt_state) return fail(ctx, PVT_EINVAL, "opportunistic needs mt_state");
  R.r = *r;
  R.T = T; R.H = H; R.Z = r->n_zones; R.lo = lo; R.hi = hi; R.world = world;
  R.t0 = 0; R.nt = 0; R.opp = true;
  R.opp_W = OPP_SHARD_WINDOW;
  R.opp_nq = (H + OPP_CH - 1) / OPP_CH;
  R.opp_nsq = (R.opp_nq + OPP_SUP - 1) / OPP_SUP;
  R.opp_Psq = (R.opp_nsq + world - 1) / world;
  if ((lo % OPP_SUP_HOSTS != 0 && lo != H) || (hi != H && hi % OPP_SUP_HOSTS != 0) ||
      hi - lo > R.opp_Psq * OPP_SUP_HOSTS)
    return fail(ctx, PVT_EINVAL, "opportunistic shard [%d, %d) must span whole super-chunks of %d hosts, "
                "at most %d of them (rank r: [r*%d, (r+1)*%d) clamped to H)", lo, hi, OPP_SUP_HOSTS,
                R.opp_Psq, R.opp_Psq * OPP_SUP_HOSTS, R.opp_Psq * OPP_SUP_HOSTS);
  R.opp_sq_lo = lo < hi ? lo / OPP_SUP_HOSTS : 0;    // an empty shard counts nothing
  R.opp_sq_hi = lo < hi ? (hi + OPP_SUP_HOSTS - 1) / OPP_SUP_HOSTS : 0;
  if (max_package_bytes) *max_package_bytes = (int64_t)opp_pkg_bytes(R, R.opp_W);
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  if (T > 0) {
    HIPCHK(hipMemsetAsync(r->placement, 0xff, sizeof(int32_t) * T, st));
    launch_iota(r->order, T, st);
    ENSURE(ctx->dem_ord, sizeof(double) * 4 * T);
    launch_gather_tasks(r->dem, r->order, nullptr, nullptr, T, P<double>(ctx->dem_ord), nullptr,
                        nullptr, st);
    ENSURE(ctx->opp, opp_table_bytes(R) + sizeof(uint32_t) * 640);
    uint32_t* mt = reinterpret_cast<uint32_t*>(P<char>(ctx->opp) + opp_table_bytes(R));
    HIPCHK(hipMemcpyAsync(mt, r->mt_state, sizeof(uint32_t) * 625, hipMemcpyHostToDevice, st));
  }
  ENSURE(ctx->oppfault, 16);
  HIPCHK(hipMemsetAsync(ctx->oppfault.p, 0, sizeof(int32_t), st));   // the walks' fault word
  R.active = true;
  return PVT_OK;
}

static int opp_shard_score(pvt_ctx* ctx, void* package, int32_t* n_tasks_out, int64_t* package_bytes) {
  RoundState& R = ctx->rs;
  hipStream_t st = ctx->stream;
  if (R.t0 >= R.T) {                          // done: the MT19937 state back to the caller
    if (R.T > 0) {
      uint32_t* mt = reinterpret_cast<uint32_t*>(P<char>(ctx->opp) + opp_table_bytes(R));
      HIPCHK(hipMemcpyAsync(R.r.mt_state, mt, sizeof(uint32_t) * 625, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipMemcpyAsync(ctx->next_host + 3, ctx->oppfault.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    R.active = false;
    if (ctx->next_host[3])
      return fail(ctx, PVT_EHIP, "opportunistic walk: inconsistent feasible counts");
    return PVT_OK;
  }
  const int nt = std::min(R.opp_W, R.T - R.t0);
  const int nsr = std::max(0, R.opp_sq_hi - R.opp_sq_lo);
  uint64_t* bm = reinterpret_cast<uint64_t*>(package);
  int32_t* sc = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(package) +
                                           (size_t)nt * R.opp_Psq * OPP_SUP * 4 * sizeof(uint64_t));
  if (nsr > 0) {
    OppCountArgs ca{R.r.avail, P<double>(ctx->dem_ord) + (size_t)R.t0 * 4, R.H, nt, 0, 0,
                    R.opp_nq, R.opp_nsq, nt, bm, sc, R.opp_sq_lo, R.opp_sq_hi,
                    R.opp_Psq * OPP_SUP, R.opp_Psq};
    Scope s(ctx, PVT_K_SCORE, (double)nt * (R.hi - R.lo), (double)nt * (R.hi - R.lo) * 32.0);
    launch_opp_count(ca, st);
  }
  HIPCHK(hipGetLastError());
  R.nt = nt;
  ctx->windows++;
  *n_tasks_out = nt;
  *package_bytes = (int64_t)opp_pkg_bytes(R, nt);
  HIPCHK(hipStreamSynchronize(st));           // the package is complete when this returns
  return PVT_OK;
}

static int opp_shard_commit(pvt_ctx* ctx, const void* packages) {
  RoundState& R = ctx->rs;
  const pvt_round* r = &R.r;
  hipStream_t st = ctx->stream;
  const int nt = R.nt, t0 = R.t0;
  char* base = P<char>(ctx->opp);
  uint64_t* bm = reinterpret_cast<uint64_t*>(base);
  int32_t* sc = reinterpret_cast<int32_t*>(base + (size_t)R.opp_W * R.opp_nq * 4 * sizeof(uint64_t));
  uint32_t* mt = reinterpret_cast<uint32_t*>(base + opp_table_bytes(R));
  OppUnpackArgs ua{reinterpret_cast<const uint8_t*>(packages), (int64_t)opp_pkg_bytes(R, nt),
                   R.world, nt, R.opp_nq, R.opp_nsq, R.opp_Psq, R.opp_W, bm, sc};
  {
    Scope s(ctx, PVT_K_MERGE, 0, 0);
    launch_opp_unpack(ua, st);
  }
  OppCommitArgs oa{r->avail, P<double>(ctx->dem_ord) + (size_t)t0 * 4, bm, sc, R.H, nt, R.opp_nq,
                   R.opp_nsq, R.opp_W, r->placement + t0, mt, ctx->stamps, nullptr, nullptr, 1,
                   P<int32_t>(ctx->oppfault)};
  {
    Scope s(ctx, PVT_K_COMMIT, 0, 0, nullptr, "opp_commit_kernel");
    launch_opp_commit(oa, st);
  }
  HIPCHK(hipGetLastError());
  R.t0 += nt;
  R.nt = 0;
  return PVT_OK;
}

extern "C" int pvt_shard_begin(pvt_ctx* ctx, const pvt_round* r, int32_t host_lo,
                               int32_t host_hi, int32_t world, int64_t* max_package_bytes) {
  if (!ctx || !r) return PVT_EINVAL;
  ctx->rs.active = false;
  if (world < 1 || world > PVT_SHARD_MAX_WORLD)
    return fail(ctx, PVT_EINVAL, "world %d outside [1, %d]", world, PVT_SHARD_MAX_WORLD);
  if (host_lo < 0 || host_hi < host_lo || host_hi > r->n_hosts)
    return fail(ctx, PVT_EINVAL, "bad host range [%d, %d) of %d", host_lo, host_hi, r->n_hosts);
  ctx->rs.opp = false;
  ctx->rs.inflight = ctx->rs.spec = false;
  ctx->rs.nt = 0;
  ctx->rs.pkind = PK_LIST;
  ctx->n_epochs = ctx->n_segs = ctx->n_rejected = 0;
  ctx->n_zchains = ctx->n_gchains = ctx->n_longest = ctx->n_fastpro = 0;
  if (ctx->checks) {
    int rc = gate_checks(ctx, r, 1, true, false);
    if (rc) return rc;
  }
  if (r->mode == PVT_OPP) {
    int rc = check_round(ctx, r);
    if (rc) return rc;
    ctx->windows = ctx->refills = 0;
    return opp_shard_begin(ctx, r, host_lo, host_hi, world, max_package_bytes);
  }
  RoundState& R = ctx->rs;
  R.sharded = true;
  int rc = round_begin(ctx, r, host_lo, host_hi, world);
  if (rc) return rc;
  // cost_aware best-fit: frontier-walked epochs (the walk's exchange is its window candidates),
  // list windows for what they cannot prove
  if ((rc = epoch_groups(ctx))) return rc;
  R.sh_epochs = !R.egs.empty() && ctx->zwalk && !R.r.rt_bw && R.Z <= ZMAX;
  R.list_until = 0;
  if (R.sh_epochs) {
    ENSURE(ctx->ep_dev, sizeof(int32_t) * EP_WORDS);
    ENSURE(ctx->wres, sizeof(WinRec) * (size_t)EPOCH_MAX);
    ENSURE(ctx->hmin, sizeof(double) * 4 * ZW_MIN_PARTS);
  }
  if (R.sh_epochs || R.ofront || R.keyed) {
    ENSURE(ctx->fwin, sizeof(FrontierSlot) * (size_t)EPOCH_SEGS);
    ENSURE(ctx->hmin, sizeof(double) * 4 * ZW_MIN_PARTS);
  }
  const int PK = shard_depth(world);
  ENSURE(ctx->pkg, sizeof(SegEntry) * (size_t)(PK + 1) * R.Wmax);
  const int64_t lists = (int64_t)sizeof(SegEntry) * (PK + 1) * R.Wmax;
  if (max_package_bytes) *max_package_bytes = std::max(lists, frontier_pkg_bytes(EPOCH_SEGS));
  return PVT_OK;
}

// The walk in flight, waited for: the round continues where it stopped.
static int shard_finish_walk(pvt_ctx* ctx) {
  RoundState& R = ctx->rs;
  if (!R.inflight) return PVT_OK;
  R.inflight = false;
  int adv = 0, rc;
  if ((rc = walk_status(ctx, R.if_t0, R.if_nt, R.if_inh, &adv))) return rc;
  adapt_window(ctx, adv, R.if_nt);
  R.t0 = R.if_t0 + adv;
  R.of_try = R.ofront;            // (place_pipelined: ordered_frontier after every list walk)
  return PVT_OK;
}

// Last task (exclusive) a list window starting at t0 may reach: keyed rounds stop at the group
// end (frozen keys), sharded best-fit epochs at list_until (frontier epochs go on from there).
static int list_end(const RoundState& R, int t0) {
  int ge = group_end(R, t0);
  if (R.sh_epochs) ge = std::min(ge, std::max(R.list_until, t0));
  return ge;
}

// ---- host-sharded frontier walks. A step's package is this rank's window candidates
// (FrontierHdr, then a FrontierSlot per epoch chain or for the one keyed / ordered walk); after
// the all-gather every rank merges them (launch_zwin_merge) into exactly the window the unsharded
// walk builds over all hosts, and runs the same walk, validation and apply on identical inputs.
// Returns with *made = false when the next step is a list window.
static int shard_frontier_score(pvt_ctx* ctx, void* package, int* nt_out, int64_t* bytes_out,
                                bool* made) {
  RoundState& R = ctx->rs;
  const pvt_round* r = &R.r;
  hipStream_t st = ctx->stream;
  *made = false;
  FrontierHdr* hdr = reinterpret_cast<FrontierHdr*>(package);
  FrontierSlot* slots = reinterpret_cast<FrontierSlot*>(hdr + 1);
  if (R.sh_epochs && R.t0 < R.T && R.t0 >= R.list_until) {
    epoch_plan(R, R.t0, R.E);
    const int nch = (int)R.E.segs.size(), nt = R.E.off.back();
    if (nch <= 1) {                 // one chain: list windows (as place_epochs)
      R.list_until = R.t0 + nt;
      return PVT_OK;
    }
    int rc;
    if ((rc = upload_chain_tables(ctx, R.E))) return rc;
    int32_t* dev = P<int32_t>(ctx->ep_dev);
    {
      Scope sc(ctx, PVT_K_OTHER, 0, 0);
      launch_host_min(r->avail, R.H, R.lo, R.hi, &hdr->hmin[0][0], st);
      ZwinArgs za{r->avail, r->zone, R.H, R.Z, R.lo, R.hi, P<double>(ctx->csum),
                  P<int32_t>(ctx->anc_ord) + R.t0, dev + EP_COFF, dev + EP_CMAP, slots};
      launch_zwin_build(za, nch, st);
    }
    ctx->n_epochs++;
    ctx->n_segs += (int)R.E.chain.size();
    R.pkind = PK_EPOCH;
    *nt_out = nt;
    *bytes_out = frontier_pkg_bytes(nch);
    *made = true;
  } else if (R.ofront && R.of_try && R.T - R.t0 >= ORDERED_FRONTIER_MIN) {
    // this rank's first hosts alive for the next tasks' smallest demand, among the first R.ofh
    // hosts of the cluster (ordered_frontier)
    const int n = std::min(R.T - R.t0, R.of_tasks);
    const int hs = std::min(R.ofh, R.H);
    const int he = std::min(R.hi, hs), nloc = std::max(0, he - R.lo);
    const double* dem = P<double>(ctx->dem_ord) + (size_t)R.t0 * 4;
    {
      Scope sc(ctx, PVT_K_OTHER, 0, 0);
      launch_alive_flags(r->avail, R.H, R.lo, he, dem, n, r->mode == PVT_CA_FF ? 1 : 0,
                         P<double>(ctx->hmin), P<uint8_t>(ctx->kflag), st);
      if (nloc > 0) {
        int rc = compact_flags(ctx, nloc, st);
        if (rc) return rc;
      } else {
        HIPCHK(hipMemsetAsync(P<int32_t>(ctx->next) + 2, 0, sizeof(int32_t), st));
      }
      launch_zwin_gather(r->avail, R.H, R.lo, P<int32_t>(ctx->kperm), P<int32_t>(ctx->next) + 2,
                         slots, st);
    }
    R.pkind = PK_ORDERED;
    R.of_n = n;
    R.of_hs = hs;
    *nt_out = n;
    *bytes_out = frontier_pkg_bytes(1);
    *made = true;
  }
  if (*made) {
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));   // the package is complete when pvt_shard_score returns
  }
  return PVT_OK;
}

// Keyed first-fit at a group start (round_next_window set kf_pending): this rank's first hosts
// of the group's zero-key prefix (its own sorted range, kperm; length on the device).
static int shard_keyed_score(pvt_ctx* ctx, void* package, int* nt_out, int64_t* bytes_out) {
  RoundState& R = ctx->rs;
  hipStream_t st = ctx->stream;
  FrontierSlot* slots = reinterpret_cast<FrontierSlot*>(reinterpret_cast<FrontierHdr*>(package) + 1);
  {
    Scope sc(ctx, PVT_K_OTHER, 0, 0);
    launch_zwin_gather(R.r.avail, R.H, R.lo, P<int32_t>(ctx->kperm), P<int32_t>(ctx->next) + 2,
                       slots, st);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  R.pkind = PK_KEYED;
  *nt_out = group_end(R, R.t0) - R.t0;
  *bytes_out = frontier_pkg_bytes(1);
  return PVT_OK;
}

// The exchanged frontier packages: merge, walk, and (epochs) validate + apply; the round goes on
// from the tasks the walk proved. Synchronous.
static int shard_frontier_commit(pvt_ctx* ctx, const void* packages) {
  RoundState& R = ctx->rs;
  const pvt_round* r = &R.r;
  hipStream_t st = ctx->stream;
  const int kind = R.pkind, nt = R.nt, t0 = R.t0;
  const int nslots = kind == PK_EPOCH ? (int)R.E.segs.size() : 1;
  FrontierSlot* win = P<FrontierSlot>(ctx->fwin);
  {
    Scope sc(ctx, PVT_K_MERGE, 0, 0);
    launch_zwin_merge(reinterpret_cast<const uint8_t*>(packages), R.pbytes, R.world, nslots, win,
                      kind == PK_EPOCH ? P<double>(ctx->hmin) : nullptr, st);
  }
  R.nt = 0;
  R.pkind = PK_LIST;
  int rc;
  if (kind == PK_EPOCH) {
    const EpochPlan& E = R.E;
    const int nseg = (int)E.chain.size(), nch = nslots;
    int32_t* dev = P<int32_t>(ctx->ep_dev);
    ENSURE(ctx->cmax, sizeof(double) * 4 * EPOCH_SEGS);
    ZwalkArgs za = zwalk_chain_args(ctx, t0);
    za.pwin = win;
    za.cmax = P<double>(ctx->cmax);
    {
      Scope sc(ctx, PVT_K_COMMIT, 0, 0, nullptr, "zwalk_kernel");
      launch_zwalk(za, nch, st);
    }
    EpochArgs ea = epoch_args(ctx, t0, nt, nseg);
    ea.rtb = r->rt_bw;
    ea.cmax = P<double>(ctx->cmax);
    ea.coff = dev + EP_COFF;
    ea.nch = nch;
    ea.safe = dev + EP_SAFE;
    epoch_tail(ctx, ea, true, nch);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    int need = 0, adv = 0;
    if ((rc = epoch_frontier_verdict(ctx, E, t0, &need, &adv))) return rc;
    // chains the walk could not prove: list windows over the rest of this epoch's tasks
    if (need && adv < nt) R.list_until = t0 + nt;
    R.t0 = t0 + adv;
    return PVT_OK;
  }
  // keyed / ordered: one walk over the merged window, capacities written back
  const bool strict = r->mode == PVT_CA_FF;
  const int n = kind == PK_ORDERED ? R.of_n : nt;
  ENSURE(ctx->wres, sizeof(WinRec) * (size_t)n);
  ZwalkArgs za = zwalk_keyed_args(ctx, t0, n);
  za.lo = R.lo;
  za.pwin = win;
  {
    Scope sc(ctx, PVT_K_COMMIT, 0, 0, nullptr, "zwalk_kernel");
    launch_zwalk_keyed(za, strict, st);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(ctx->next_host, P<int32_t>(ctx->next), sizeof(int32_t) * 2,
                        hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(ctx->next_host + 2, &win->total, sizeof(int32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  const int done = ctx->next_host[0];
  if (kind == PK_KEYED) {
    if ((rc = frontier_walked(ctx, "sharded", done, n))) return rc;
    R.t0 = t0 + done;
    R.kf_pending = false;
    return PVT_OK;
  }
  // ordered: as ordered_frontier; the attempt that is not to be repeated hands over to one list
  // window
  bool again = false;
  if ((rc = ordered_verdict(ctx, "sharded", done, n, R.of_hs, &again))) return rc;
  R.t0 = t0 + done;
  if (!again) R.of_try = false;
  return PVT_OK;
}

// Pipelined (pvt_set_pipeline, default on): while walk k runs, window k+1 of the same group is
// scored on the side stream -- on the state walk k-1 left -- and its package returned for the
// exchange, which the caller overlaps with walk k; pvt_shard_commit then waits for walk k and
// returns PVT_ESTALE if it stopped early (every rank sees the same walk, so all ranks agree).
extern "C" int pvt_shard_score(pvt_ctx* ctx, void* package, int32_t* n_tasks_out,
                               int64_t* package_bytes) {
  if (!ctx || !package || !n_tasks_out || !package_bytes) return PVT_EINVAL;
  *n_tasks_out = 0;
  *package_bytes = 0;
  RoundState& R = ctx->rs;
  if (!R.active || R.world < 1) return fail(ctx, PVT_EINVAL, "no sharded round in progress");
  if (R.nt != 0) return fail(ctx, PVT_EINVAL, "pvt_shard_score called twice without pvt_shard_commit");
  if (R.opp) return opp_shard_score(ctx, package, n_tasks_out, package_bytes);
  const int PK = shard_depth(R.world);
  int nt = 0, rc, lb = 0;
  hipStream_t st = ctx->stream;
  R.spec = false;
  if (R.inflight) {
    const int t1 = R.if_t0 + R.if_nt, ge = list_end(R, R.if_t0);
    // (ordered rounds: no speculative window; the frontier walk is tried after each)
    if (ctx->pipeline && t1 < ge && !R.ofront) {   // speculative: the window after the walk in flight
      nt = std::min(R.W, ge - t1);
      lb = 1 - R.if_lb;
      st = ctx->side;
      HIPCHK(hipStreamWaitEvent(st, ctx->ev_walk, 0));
      if ((rc = window_lists(ctx, t1, nt, lb, st))) return rc;
      R.spec = true;
      R.pt0 = t1;
    } else if ((rc = shard_finish_walk(ctx))) {
      return rc;
    }
  }
  if (!R.spec) flush_touched(ctx);   // (no band score in flight)
  if (!R.spec) {
    bool made = false;
    int64_t fb = 0;
    if ((rc = shard_frontier_score(ctx, package, &nt, &fb, &made))) return rc;
    if (!made) {
      if ((rc = round_next_window(ctx, &nt))) return rc;
      if (nt > 0 && R.kf_pending) {
        if ((rc = shard_keyed_score(ctx, package, &nt, &fb))) return rc;
        made = true;
      }
    }
    if (made) {
      R.nt = nt;
      R.pt0 = R.t0;
      R.pbytes = fb;
      *n_tasks_out = nt;
      *package_bytes = fb;
      return PVT_OK;
    }
    if (nt == 0) {
      R.active = false;
      HIPCHK(hipStreamSynchronize(ctx->stream));
      return PVT_OK;
    }
    if (R.sh_epochs) nt = std::min(nt, list_end(R, R.t0) - R.t0);
    if ((rc = window_lists(ctx, R.t0, nt, lb, st))) return rc;
    R.pt0 = R.t0;
  }
  R.pkind = PK_LIST;
  Lists L;
  lists_from(ctx, L, lb);
  PackArgs pa{L, nt, PK, R.ordered ? 1 : 0, reinterpret_cast<SegEntry*>(package)};
  {
    Scope sc(ctx, PVT_K_MERGE, 0, 0, st);
    launch_pack(pa, st);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));           // the package is complete when this returns
  R.nt = nt;
  R.plb = lb;
  *n_tasks_out = nt;
  *package_bytes = (int64_t)sizeof(SegEntry) * (PK + 1) * nt;
  return PVT_OK;
}

extern "C" int pvt_shard_commit(pvt_ctx* ctx, const void* packages) {
  if (!ctx || !packages) return PVT_EINVAL;
  RoundState& R = ctx->rs;
  if (!R.active || R.nt == 0) return fail(ctx, PVT_EINVAL, "pvt_shard_commit without a scored window");
  if (R.opp) return opp_shard_commit(ctx, packages);
  if (R.pkind != PK_LIST) return shard_frontier_commit(ctx, packages);
  int rc, n_prev = 0;
  if (R.spec) {                               // wait for the walk the package speculated past
    if ((rc = shard_finish_walk(ctx))) return rc;
    if (R.t0 != R.pt0) {                      // it stopped early: the package is stale
      R.nt = 0;
      R.spec = false;
      return PVT_ESTALE;
    }
    n_prev = ctx->next_host[1];               // its hosts: stale in these lists, so touched
  }
  const int PK = shard_depth(R.world), t0 = R.pt0, nt = R.nt, lb = R.plb;
  flush_touched(ctx);   // the walk before: its package's score pass has completed
  Lists L;
  lists_from(ctx, L, lb);
  MergeArgs ma{reinterpret_cast<const SegEntry*>(packages), nullptr, R.r.avail, R.r.zone,
               P<double>(ctx->dem_ord) + (size_t)t0 * 4, P<int32_t>(ctx->anc_ord) + t0,
               R.ord + t0, R.H, nt, R.world, PK, L, nullptr, ctx->t_merge_bitonic};
  {
    Scope sc(ctx, PVT_K_MERGE, 0, 0, nullptr, merge_kernel_name(ma));
    launch_merge(ma, ctx->stream);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ctx->ev_walk, ctx->stream));   // releases the next speculative score
  if ((rc = walk_launch(ctx, t0, nt, lb, n_prev))) return rc;
  R.inflight = true;
  R.if_t0 = t0; R.if_nt = nt; R.if_lb = lb; R.if_inh = R.spec;
  R.nt = 0;
  if (!ctx->pipeline) return shard_finish_walk(ctx);
  return PVT_OK;
}
