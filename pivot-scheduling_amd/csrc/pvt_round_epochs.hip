// pvt_round_epochs.hip — group-parallel epochs of the windowed round: zero-cost components,
// the epoch plan and its chain tables, cost_aware best-fit epochs (place_epochs) and the
// first-fit zero-key epochs of keyed rounds (ff_epoch).
#include "pvt_driver.h"

// ---------------------------------------------------------------- group-parallel epochs
// Zones joined by zero egress cost (csum = 0) form one component: a group's winners are the
// lowest-index fitting hosts of its anchor's component (score 0), so two groups anchored in one
// component compete for the same hosts and an epoch never holds both (R.ecomp: zone -> root).
//
// Rounds of more than ZMAX zones (wide_components): the Z x Z table (2 MB at 512 zones) neither
// crosses the bus nor is looped over. A launch over the device sum table lists the pairs a < z
// with csum[a][z] == 0.0 -- the same doubles and the same test as below, fl(x + y) = fl(y + x) --
// and the host unions those: what it copies and loops over is proportional to the zero pairs
// (4 KB first, the rest only when there are more than ZP_FIRST - 1 of them). More than ZP_MAX
// pairs: the table path below. The components go to the device for the wide walk (ctx->zcomp).
static constexpr int ZP_FIRST = 1024;           // words of the first copy: the count and 1023 pairs
static int wide_components(pvt_ctx* ctx, bool* done) {
  RoundState& R = ctx->rs;
  const int Z = R.Z;
  hipStream_t st = ctx->stream;
  *done = false;
  ENSURE(ctx->zpairs, sizeof(int32_t) * (ZP_MAX + 1));
  std::vector<int32_t>& hp = ctx->zpairs_host;
  hp.resize(ZP_MAX + 1);
  launch_zero_pairs(P<double>(ctx->csum), Z, P<int32_t>(ctx->zpairs), ZP_MAX, st);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(hp.data(), ctx->zpairs.p, sizeof(int32_t) * ZP_FIRST, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  const int n = hp[0];
  if (n < 0 || n > ZP_MAX) return PVT_OK;       // (too many: the caller takes the table)
  if (n + 1 > ZP_FIRST) {
    HIPCHK(hipMemcpyAsync(hp.data() + ZP_FIRST, P<int32_t>(ctx->zpairs) + ZP_FIRST,
                          sizeof(int32_t) * (size_t)(n + 1 - ZP_FIRST), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  R.ecomp.resize(Z);
  R.ezcomp.resize(Z);
  for (int z = 0; z < Z; z++) R.ecomp[z] = R.ezcomp[z] = z;
  auto zroot = [&](int z) { while (R.ezcomp[z] != z) z = R.ezcomp[z] = R.ezcomp[R.ezcomp[z]]; return z; };
  for (int i = 1; i <= n; i++) {
    const int a = hp[i] >> 16, z = hp[i] & 0xffff;
    if (a < 0 || a >= Z || z >= Z) return fail(ctx, PVT_EHIP, "zero pair (%d, %d) of %d zones", a, z, Z);
    R.ezcomp[zroot(a)] = zroot(z);
  }
  for (int z = 0; z < Z; z++) R.ezcomp[z] = zroot(z);
  if (ctx->t_epoch_plan) R.ecomp = R.ezcomp;    // (PVT_EPOCH_PLAN=0: distinct zones only)
  *done = true;
  return PVT_OK;
}

// The components to the device, for the wide frontier walk (ZwalkArgs.zcomp).
static int upload_components(pvt_ctx* ctx) {
  const RoundState& R = ctx->rs;
  static_assert(sizeof(int) == sizeof(int32_t), "zone components as int32");
  ENSURE(ctx->zcomp, sizeof(int32_t) * (size_t)R.Z);
  HIPCHK(hipMemcpyAsync(ctx->zcomp.p, R.ezcomp.data(), sizeof(int32_t) * (size_t)R.Z, hipMemcpyHostToDevice,
                        ctx->stream));
  return PVT_OK;
}

int pvt::zero_cost_components(pvt_ctx* ctx) {
  RoundState& R = ctx->rs;
  const pvt_round* r = &R.r;
  const int Z = R.Z;
  if (Z > ZMAX) {
    bool done = false;
    int rc = wide_components(ctx, &done);
    if (rc) return rc;
    if (done) return upload_components(ctx);
  }
  std::vector<double> cost((size_t)Z * Z);
  if (R.ginfo && R.cost_host.size() == cost.size()) {
    cost = R.cost_host;
  } else {
    HIPCHK(hipMemcpyAsync(cost.data(), r->cost, sizeof(double) * Z * Z, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
  }
  R.ecomp.resize(Z);
  for (int z = 0; z < Z; z++) R.ecomp[z] = z;
  auto root = [&](int z) { while (R.ecomp[z] != z) z = R.ecomp[z] = R.ecomp[R.ecomp[z]]; return z; };
  const int plan = ctx->t_epoch_plan;   // (PVT_EPOCH_PLAN=0: distinct zones only)
  for (int a = 0; a < Z && plan; a++)
    for (int z = 0; z < Z; z++)
      if (cost[(size_t)a * Z + z] + cost[(size_t)z * Z + a] == 0.0) R.ecomp[root(a)] = root(z);
  for (int z = 0; z < Z; z++) R.ecomp[z] = root(z);
  // the components proper, whatever the plan (under PVT_EPOCH_PLAN=0 chains of one component share
  // window hosts: the epoch tail's condition 2)
  R.ezcomp.resize(Z);
  for (int z = 0; z < Z; z++) R.ezcomp[z] = z;
  auto zroot = [&](int z) { while (R.ezcomp[z] != z) z = R.ezcomp[z] = R.ezcomp[R.ezcomp[z]]; return z; };
  for (int a = 0; a < Z; a++)
    for (int z = 0; z < Z; z++)
      if (cost[(size_t)a * Z + z] + cost[(size_t)z * Z + a] == 0.0) R.ezcomp[zroot(a)] = zroot(z);
  for (int z = 0; z < Z; z++) R.ezcomp[z] = zroot(z);
  return Z > ZMAX ? upload_components(ctx) : PVT_OK;
}

// cost_aware best-fit rounds of several groups (pvt_epoch.hip). The groups in processing
// order, from the caller's task_group / group_anchor (a group's tasks are contiguous).
int pvt::epoch_groups(pvt_ctx* ctx) {
  RoundState& R = ctx->rs;
  const pvt_round* r = &R.r;
  if (R.ffe) return PVT_OK;                   // keyed rounds: ff_epoch plans on round_begin's groups
  R.egs.clear();
  R.ega.clear();
  const int T = R.T;
  if (!ctx->epochs || r->mode != PVT_CA_BF || !r->task_group || r->n_groups < 2 || T < 2) return PVT_OK;
  // rounds of more than ZMAX zones: epochs where the wide frontier walk can run (unsharded, no
  // realtime bandwidth; PVT_ZW_WIDE=0: never), else pipelined windows as ever
  if (R.Z > ZMAX && !wide_fast(ctx)) return PVT_OK;
  hipStream_t st = ctx->stream;
  int rc;
  std::vector<int> cnt(r->n_groups, 0);
  std::vector<int32_t> ga;
  if (R.ginfo) {                              // copied by build_order
    for (int g = 0; g < r->n_groups; g++) cnt[g] = R.gcnt[g];
    ga = R.ga_host;
  } else {
    std::vector<int32_t> tg(T);
    ga.resize(r->n_groups);
    HIPCHK(hipMemcpyAsync(tg.data(), r->task_group, sizeof(int32_t) * T, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(ga.data(), r->group_anchor, sizeof(int32_t) * r->n_groups,
                          hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int t = 0; t < T; t++) {
      if (tg[t] < 0 || tg[t] >= r->n_groups) return fail(ctx, PVT_EINVAL, "task_group out of range");
      cnt[tg[t]]++;
    }
  }
  int off = 0, ng = 0;
  for (int g = 0; g < r->n_groups; g++) {
    if (cnt[g] == 0) continue;
    R.egs.push_back(off);
    R.ega.push_back(ga[g]);
    off += cnt[g];
    ng++;
  }
  R.egs.push_back(T);
  if ((rc = zero_cost_components(ctx))) return rc;
  // worth it when groups are many and short (a group longer than a walk's window is walked in
  // sequential epochs of one segment, without the score / walk pipeline of place_pipelined)
  if (ng < 2 || T > ng * MAX_WINDOW) { R.egs.clear(); R.ega.clear(); }
  return PVT_OK;
}

void pvt::epoch_plan(const RoundState& R, int t0, EpochPlan& P, bool whole) {
  P.off.assign(1, 0);
  P.chain.clear(); P.cstart.clear(); P.segs.clear(); P.len.clear();
  size_t g = 0;
  while (g + 1 < R.egs.size() && R.egs[g + 1] <= t0) g++;
  std::vector<int> chain_of(R.ecomp.size() + 1, -1);
  int t = t0;
  while (t < R.T && (int)P.chain.size() < EPOCH_SEGS) {
    const int ge = R.egs[g + 1];
    const int z = R.ega[g];
    const int comp = (z >= 0 && z < (int)R.ecomp.size()) ? R.ecomp[z] : (int)R.ecomp.size();
    int c = chain_of[comp];
    if (c < 0) {
      c = chain_of[comp] = (int)P.segs.size();
      P.segs.emplace_back();
      P.len.push_back(0);
    }
    const int take = std::min({ge - t, CHAIN_MAX - P.len[c], t0 + EPOCH_MAX - t});
    if (take <= 0 || (whole && take < ge - t)) {
      if (P.len[c] == 0) { P.segs.pop_back(); P.len.pop_back(); }   // (a chain opened for it)
      break;
    }
    P.segs[c].push_back((int)P.chain.size());
    P.chain.push_back(c);
    P.cstart.push_back(P.len[c]);
    P.len[c] += take;
    t += take;
    P.off.push_back(t - t0);
    if (t < ge) break;
    g++;
  }
}

// The epoch's chain tables to the device (one upload): segment offsets / chains / chain-local
// starts, per chain its task range in cmap and its segments' chain-local starts.
int pvt::upload_chain_tables(pvt_ctx* ctx, const EpochPlan& E) {
  int32_t* host = ctx->ep_host;
  const int nseg = (int)E.chain.size(), nch = (int)E.segs.size();
  for (int k = 0; k <= nseg; k++) host[EP_SEG_OFF + k] = E.off[k];
  for (int k = 0; k < nseg; k++) { host[EP_SEG_CHAIN + k] = E.chain[k]; host[EP_SEG_CSTART + k] = E.cstart[k]; }
  int nm = 0, ns = 0;
  for (int c = 0; c < nch; c++) {
    host[EP_COFF + c] = nm;
    host[EP_CSOFF + c] = ns;
    for (int sg : E.segs[c]) {
      host[EP_CSEG + ns++] = E.cstart[sg];
      for (int w = E.off[sg]; w < E.off[sg + 1]; w++) host[EP_CMAP + nm++] = w;
    }
  }
  host[EP_COFF + nch] = nm;
  host[EP_CSOFF + nch] = ns;
  launch_upload(ctx->ep_hdev, ctx->ep_dev.p, sizeof(int32_t) * (EP_CMAP + nm), ctx->stream);
  HIPCHK(hipGetLastError());
  return PVT_OK;
}

// The same tables by value for the frontier walk (ChainTab: no upload launch); false when the
// epoch does not fit them (the caller uploads instead).
static_assert(EPOCH_SEGS == CT_SEGS, "chain tables by value hold every epoch segment");
static bool chain_tab(pvt_ctx* ctx, const EpochPlan& E, ChainTab& t) {
  const int nseg = (int)E.chain.size(), nch = (int)E.segs.size();
  if (nseg < 1 || nseg > CT_SEGS || nch < 1 || nch > CT_SEGS) return false;
  for (int c = 0; c < nch; c++)
    if (E.len[c] > CHAIN_MAX) return false;
  int32_t* dev = P<int32_t>(ctx->ep_dev);
  t.nseg = nseg;
  t.nch = nch;
  for (int k = 0; k <= nseg; k++) t.seg_off[k] = E.off[k];
  for (int k = 0; k < nseg; k++) { t.seg_chain[k] = E.chain[k]; t.seg_cstart[k] = E.cstart[k]; }
  int nm = 0, ns = 0;
  for (int c = 0; c < nch; c++) {
    t.coff[c] = nm;
    t.csoff[c] = ns;
    for (int sg : E.segs[c]) t.csegid[ns++] = sg;
    nm += E.len[c];
  }
  t.coff[nch] = nm;
  t.csoff[nch] = ns;
  t.o_seg_off = dev + EP_SEG_OFF;
  t.o_seg_chain = dev + EP_SEG_CHAIN;
  t.o_seg_cstart = dev + EP_SEG_CSTART;
  t.o_coff = dev + EP_COFF;
  return true;
}

// What the host knows of the first epoch's chains, by value, for the frontier walk's fast prologue
// (ChainCert, pvt_kernels.h): false unless the grouped order's launch wrote this
// round's group certificates and every segment is a whole group of at most GSORT_MAX tasks with
// an anchor in [0, Z). Segment k of an epoch planned from task 0 is the round's k-th non-empty
// group (epoch_plan). A chain's zone set is the union of its anchors' zero-cost zones, by the
// expression the device uses (cost[a][z] + cost[z][a] == 0.0); its window is the one
// zone_window_block built for the lowest zone of its anchors' zero-cost component. uw: the same
// windows for epoch_undo_kernel.
static bool chain_cert(pvt_ctx* ctx, int t0, const EpochPlan& E, ChainCert& cc, UndoWin& uw) {
  const RoundState& R = ctx->rs;
  const int Z = R.Z, G = R.r.n_groups;
  const int nseg = (int)E.chain.size(), nch = (int)E.segs.size();
  if (!ctx->t_chain_cert || !R.gcert || !R.ginfo || t0 != 0) return false;
  if (Z > ZMAX || (int)R.ezcomp.size() != Z || R.cost_host.size() != (size_t)Z * Z) return false;
  if (G > GCOMPACT_MAX || (int)R.gcnt.size() < G || nseg > CT_SEGS || nch > CT_SEGS) return false;
  std::vector<int> gids;                      // the non-empty groups, in order
  for (int g = 0; g < G; g++)
    if (R.gcnt[g] > 0) gids.push_back(g);
  if (gids.size() + 1 != R.egs.size() || (int)gids.size() < nseg) return false;
  std::vector<uint32_t> am(Z, 0u);
  for (int a = 0; a < Z; a++)
    for (int z = 0; z < Z; z++)
      if (R.cost_host[(size_t)a * Z + z] + R.cost_host[(size_t)z * Z + a] == 0.0) am[a] |= 1u << z;
  cc = ChainCert{};
  for (int c = 0; c < nch; c++) {
    int root = -1, ent = 0;
    uint32_t U = 0;
    for (int sg : E.segs[c]) {
      const int len = E.off[sg + 1] - E.off[sg], a = R.ega[sg];
      if (len != R.gcnt[gids[sg]] || len > GSORT_MAX || a < 0 || a >= Z) return false;
      if (root >= 0 && R.ezcomp[a] != root) return false;   // (a chain lies in one component)
      root = R.ezcomp[a];
      U |= am[a];
      cc.seg_grp[sg] = (uint8_t)gids[sg];
      if (ent >= ZW_ENT) return false;
      cc.seg_ent[sg] = (uint8_t)ent;
      ent += (len + 63) / 64;
    }
    if (root < 0 || ent > ZW_ENT) return false;
    int j = 0;
    while (R.ezcomp[j] != root) j++;          // the component's lowest zone
    cc.cu[c] = U;
    cc.cwin[c] = uw.w[c] = (uint8_t)j;
    cc.cent[c] = (uint8_t)ent;
  }
  cc.rec = P<GroupCert>(ctx->gcert);
  cc.fast = 1;
  return true;
}

// ---------------------------------------------------------------- the epoch tail
// A frontier-walked epoch whose chains all walk to their end needs none of the kernels after the
// walk: each chain writes its window back itself (ZwalkArgs.undo: the optimistic
// apply) and the host reads the verdict from the chains' own words. Where the walk owns its
// window: unsharded rounds without realtime bandwidth (of more than ZMAX zones: the wide walk's).
static bool tail_eligible(pvt_ctx* ctx) {
  const RoundState& R = ctx->rs;
  return ctx->t_epoch_tail && !R.sharded && R.world <= 1 && !R.r.rt_bw && (R.Z <= ZMAX || wide_fast(ctx));
}

// Condition 2: no two chains hold anchors of one zero-cost component. A chain's zones U (its
// anchors' zero-cost zones) and a prebuilt window's zones (ZoneWindows: zones of one component)
// lie inside its anchors' components, so the chains' windows are then disjoint: a chain's
// write-back touches no host another chain reads or commits to. False under PVT_EPOCH_PLAN=0
// whenever two chains' U intersect.
static bool tail_chains_apart(const RoundState& R, int t0, const EpochPlan& E) {
  if ((int)R.ezcomp.size() != R.Z) return false;
  size_t g = 0;
  while (g + 1 < R.egs.size() && R.egs[g + 1] <= t0) g++;
  const int nseg = (int)E.chain.size(), nch = (int)E.segs.size();
  if (nch > 64) return false;
  std::vector<int> owner(R.Z, -1);           // component root -> the chain that holds its anchors
  for (int k = 0; k < nseg; k++, g++) {      // (segment k is the epoch's k-th group, epoch_plan)
    if (g >= R.ega.size()) return false;
    const int z = R.ega[g];
    if (z < 0 || z >= R.Z) continue;         // (the walk bails)
    int& o = owner[R.ezcomp[z]];
    if (o >= 0 && o != E.chain[k]) return false;
    o = E.chain[k];
  }
  return true;
}

// The optimistic apply's arguments of the frontier walk.
static int tail_walk_args(pvt_ctx* ctx, ZwalkArgs& za) {
  ENSURE(ctx->zundo, sizeof(ZwUndo) * (size_t)EPOCH_SEGS);
  za.undo = P<ZwUndo>(ctx->zundo);
  za.wb = ctx->rs.r.avail;
  za.hstat = ctx->ep_hdev + EP_STATUS;
  za.hcert = ctx->ep_hdev + EP_CERT;
  return PVT_OK;
}

// After the walk's synchronisation: the epoch is accepted whole iff (1) every chain walked all its
// tasks with no certificate failed, and (3, best-fit) some dimension no chain demands has a host
// minimum of at least 2^-287 -- then every log entry keeps its start value there, which exceeds
// the epoch's largest demand (+-0) by 2^-287: every segment is safe, as epoch_final_kernel would
// find, and epoch_accept_apply_kernel would accept all of them and write each host's last entry,
// the window state the chains wrote themselves. (Condition 2 was decided before the launch.)
// *wrote: the chains that wrote their windows back.
static bool tail_accepted(pvt_ctx* ctx, const EpochPlan& E, bool best_fit, uint64_t* wrote) {
  const int32_t* host = ctx->ep_host;
  const int nch = (int)E.segs.size();
  uint64_t w = 0;
  int cert = ZW_CERT_EVERY_DIM;
  for (int c = 0; c < nch; c++) {
    if (host[EP_STATUS + 2 * c] == E.len[c] && host[EP_STATUS + 2 * c + 1] == 0) w |= 1ull << c;
    cert &= host[EP_CERT + c];
  }
  *wrote = w;
  const bool all = w == (nch >= 64 ? ~0ull : (1ull << nch) - 1ull);
  return all && (!best_fit || zw_cert_verdict(cert));
}

// A missed optimistic apply: the chains that wrote back get their start rows again, before the
// tail kernels run on the epoch's start state as ever.
// (fast: the chains that took the fast prologue saved nothing: their rows are those of the
// prebuilt windows uw they walked)
static void tail_undo(pvt_ctx* ctx, uint64_t wrote, int nch, uint64_t fast = 0, const UndoWin* uw = nullptr) {
  Scope sc(ctx, PVT_K_OTHER, 0, 0, nullptr, "epoch_undo_kernel");
  launch_epoch_undo(P<ZwUndo>(ctx->zundo), wrote, nch, ctx->rs.r.avail, ctx->rs.H, ctx->stream, fast,
                    fast ? P<ZoneWindows>(ctx->zwin) : nullptr, uw);
}

// The chains whose certificate word reports the fast prologue (counted: pvt_prologue_stats).
static uint64_t fast_chains(pvt_ctx* ctx, int nch) {
  uint64_t m = 0;
  for (int c = 0; c < nch && c < 64; c++)
    if (ctx->ep_host[EP_CERT + c] & ZW_CERT_FAST) m |= 1ull << c;
  ctx->n_fastpro += __builtin_popcountll(m);
  return m;
}

// The tail kernels, each in a scope of its own name: finality, pair validation (validate), and
// (accept_nch > 0) the accepted prefix with its apply and the mapped readback.
void pvt::epoch_tail(pvt_ctx* ctx, const EpochArgs& ea, bool validate, int accept_nch) {
  hipStream_t st = ctx->stream;
  {
    Scope sc(ctx, PVT_K_OTHER, 0, 0, nullptr, "epoch_final_kernel");
    launch_epoch_final(ea, st);
  }
  if (validate) {
    Scope sc(ctx, PVT_K_OTHER, 0, 0, nullptr, "epoch_validate_kernel");
    launch_epoch_validate(ea, st);
  }
  if (accept_nch > 0) {
    Scope sc(ctx, PVT_K_OTHER, 0, 0, nullptr, "epoch_accept_apply_kernel");
    launch_epoch_accept_apply(ea, P<int32_t>(ctx->ep_dev) + EP_RES, accept_nch, st,
                              ctx->ep_hdev + EP_STATUS, EP_WORDS - EP_STATUS);   // (readback: mapped)
  }
}

// cost_aware first-fit with sort_hosts (cost_aware.py:99-127): an epoch of WHOLE groups from
// the group start R.t0, chains of zero-cost components walked side by side by the first-fit
// zero-key chain walk (pvt_zwalk.hip, FF). Every task it proves takes the lowest-index strictly
// fitting host of its anchor's zero-cost zones -- the first host of the frozen key order -- and
// chains of different components touch disjoint hosts that are never zero-key for another
// chain's anchors, so no pair validation is needed. Groups are accepted whole, in order, up to
// the first one a chain did not complete (the keyed path then takes that group from its start,
// computing its frozen key on the capacities at the group start, as the reference does).
int pvt::ff_epoch(pvt_ctx* ctx, int* adv_out) {
  RoundState& R = ctx->rs;
  const pvt_round* r = &R.r;
  hipStream_t st = ctx->stream;
  *adv_out = 0;
  const int t0 = R.t0;
  EpochPlan E;
  epoch_plan(R, t0, E, true);
  const int nseg = (int)E.chain.size(), nch = (int)E.segs.size();
  if (nseg == 0 || nch == 0) return PVT_OK;
  const int nt = E.off.back();
  ENSURE(ctx->ep_dev, sizeof(int32_t) * EP_WORDS);
  ENSURE(ctx->wres, sizeof(WinRec) * (size_t)EPOCH_MAX);
  ENSURE(ctx->hmin, sizeof(double) * 4 * ZW_MIN_PARTS);
  int32_t* host = ctx->ep_host;
  int rc;
  {
    Scope sc(ctx, PVT_K_OTHER, 0, 0);
    launch_host_absmax(r->avail, R.H, 0, R.H, P<double>(ctx->hmin), st);
  }
  ZwalkArgs za = zwalk_chain_args(ctx, t0);
  if (!(ctx->t_chain_tab && chain_tab(ctx, E, za.tab)) && (rc = upload_chain_tables(ctx, E))) return rc;
  // the epoch tail: chains of different components write their windows back themselves, and an
  // epoch all of whose chains completed needs no launch after the walk (no pair validation here)
  // (chains that share a component, PVT_EPOCH_PLAN=0, would take the same hosts side by side and
  // nothing here checks pairs: those groups go to the keyed path)
  if (!tail_chains_apart(R, t0, E)) return PVT_OK;
  const bool opt = tail_eligible(ctx);
  if (opt && (rc = tail_walk_args(ctx, za))) return rc;
  {
    Scope sc(ctx, PVT_K_COMMIT, 0, 0, nullptr, "zwalk_kernel");
    if (R.Z > ZMAX) launch_zwalk_ff_wide(za, nch, st);
    else launch_zwalk_ff(za, nch, st);
  }
  ctx->n_epochs++;
  ctx->n_segs += nseg;
  if (opt) {
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    uint64_t wrote = 0;
    if (tail_accepted(ctx, E, false, &wrote)) {
      ctx->n_zchains += nch;
      ctx->n_longest += *std::max_element(E.len.begin(), E.len.end());
      *adv_out = nt;
      return PVT_OK;
    }
    tail_undo(ctx, wrote, nch);
  }
  EpochArgs ea = epoch_args(ctx, t0, nt, nseg);
  ea.whole = 1;
  epoch_tail(ctx, ea, false, nch);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  int proven = 0;
  for (int c = 0; c < nch; c++) proven += host[EP_STATUS + 2 * c] == E.len[c];
  ctx->n_zchains += proven;
  ctx->n_longest += *std::max_element(E.len.begin(), E.len.end());
  ctx->n_rejected += host[EP_RES + 3];
  const int adv = host[EP_RES + 1];
  if (adv < 0 || adv > nt) return fail(ctx, PVT_EHIP, "first-fit epoch returned %d of %d tasks", adv, nt);
  *adv_out = adv;
  return PVT_OK;
}

// A frontier-walked epoch's verdict (validation, accepted prefix and its apply ran on the
// device; ctx->ep_host holds the readback): chains left unproven, and the tasks accepted.
int pvt::epoch_frontier_verdict(pvt_ctx* ctx, const EpochPlan& E, int t0, int* need_out, int* adv_out) {
  const int32_t* host = ctx->ep_host;
  const int nch = (int)E.segs.size();
  int need = 0;
  for (int c = 0; c < nch; c++) need += host[EP_STATUS + 2 * c] != E.len[c];
  ctx->n_zchains += nch - need;
  ctx->n_longest += *std::max_element(E.len.begin(), E.len.end());
  if (host[EP_RES + 4])
    return fail(ctx, PVT_EHIP, "commit walk: ring hand-off timed out (epoch at task %d)", t0);
  const int adv = host[EP_RES + 1];
  // (a segment cut short here is a frontier-walk fallback, not a list refill: the chains the
  // walk could not prove are walked with lists next; the tasks it proved are accepted)
  ctx->n_rejected += host[EP_RES + 3];
  if (adv <= 0 && !need) return fail(ctx, PVT_EHIP, "epoch made no progress at task %d", t0);
  *need_out = need;
  *adv_out = adv;
  return PVT_OK;
}

int pvt::place_epochs(pvt_ctx* ctx) {
  RoundState& R = ctx->rs;
  const pvt_round* r = &R.r;
  hipStream_t st = ctx->stream;
  ENSURE(ctx->ep_dev, sizeof(int32_t) * EP_WORDS);
  ENSURE(ctx->wres, sizeof(WinRec) * (size_t)EPOCH_MAX);
  ENSURE(ctx->owned[0], sizeof(int32_t) * (size_t)CHAIN_MAX);
  ENSURE(ctx->l_e[0], sizeof(ListEntry) * (size_t)EPOCH_MAX * LMAX);
  ENSURE(ctx->l_ids[0], sizeof(int32_t) * (size_t)EPOCH_MAX * LMAX);
  ENSURE(ctx->l_t[0], sizeof(TaskRec) * (size_t)EPOCH_MAX);
  int32_t* dev = P<int32_t>(ctx->ep_dev);
  int32_t* host = ctx->ep_host;
  EpochPlan E;
  int t0 = 0, rc;
  bool force_lists = false;       // the last epoch's frontier walk left chains unproven
  bool big = false;               // ... because a chain outgrew its window: retry with ZW_MBIG
  int big_t0 = -1;                //   (at most once per epoch start)
  R.in_epoch = true;
  struct Reset { bool& f; ~Reset() { f = false; } } reset_{R.in_epoch};
  const bool zones_ok = R.Z <= ZMAX || wide_fast(ctx);   // (the wide walk, pvt_zwalk_wide.hip)
  const bool zw_possible = ctx->zwalk && !r->rt_bw && zones_ok;
  while (t0 < R.T) {
    // (a wide round whose frontier walks keep missing: the rest on the pipelined list windows,
    // from the state the accepted epochs left -- every accepted segment is applied by here)
    if (R.Z > ZMAX && R.wide_misses >= WIDE_MISS_MAX) {
      R.t0 = t0;
      R.ep_to_lists = true;
      return PVT_OK;
    }
    // the frontier walk's host minima (certificate 2) depend only on the epoch's start state:
    // reduced while the host plans the epoch
    if (zw_possible && !force_lists && !(R.hmin_pre && t0 == 0)) {
      ENSURE(ctx->hmin, sizeof(double) * 4 * ZW_MIN_PARTS);
      Scope sc(ctx, PVT_K_OTHER, 0, 0);
      launch_host_min(r->avail, R.H, 0, R.H, P<double>(ctx->hmin), st);
    }
    R.hmin_pre = false;
    epoch_plan(R, t0, E);
    const int nseg = (int)E.chain.size(), nch = (int)E.segs.size(), nt = E.off.back();
    ctx->n_epochs++;
    ctx->n_segs += nseg;
    // chains the zero-cost frontier walk can prove need no candidate lists (pvt_zwalk.hip);
    // the lists are scored only for the others
    const bool zw = ctx->zwalk && nch > 1 && !r->rt_bw && zones_ok && !force_lists;
    force_lists = false;
    if (!zw && (rc = window_lists(ctx, t0, nt, 0, st))) return rc;
    if (nch == 1) {                           // one chain: the plain walk (writes avail)
      if ((rc = walk_launch(ctx, t0, nt, 0, 0))) return rc;
      int adv = 0;
      if ((rc = walk_status(ctx, t0, nt, false, &adv))) return rc;
      if (adv < nt) ctx->refills++;
      t0 += adv;
      continue;
    }
    // (the frontier walk takes the chain tables by value: no upload)
    ChainTab tab{};
    const bool tabv = zw && ctx->t_chain_tab && chain_tab(ctx, E, tab);
    if (!tabv && (rc = upload_chain_tables(ctx, E))) return rc;
    // (the rejection flags are zeroed by epoch_final_kernel, launched before every validation)
    int need = nch;                           // chains left to the list walk
    EpochArgs ea = epoch_args(ctx, t0, nt, nseg);
    ea.rtb = r->rt_bw;
    auto validate_and_read = [&]() -> int {
      epoch_tail(ctx, ea, true, 0);
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(host + EP_STATUS, dev + EP_STATUS, sizeof(int32_t) * (EP_WORDS - EP_STATUS),
                            hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      return PVT_OK;
    };
    if (zw) {
      ENSURE(ctx->cmax, sizeof(double) * 4 * EPOCH_SEGS);
      ZwalkArgs za = zwalk_chain_args(ctx, t0);
      za.cmax = P<double>(ctx->cmax);
      // (the first epoch starts from the snapshot the grouped order's launch built its windows from)
      if (R.zpre && t0 == 0 && !big) za.zpre = P<ZoneWindows>(ctx->zwin);
      if (tabv) za.tab = tab;
      // the fast prologue: the groups' certificates instead of a pass over the chains' rows
      UndoWin uw{};
      const bool fastp = tabv && za.zpre && chain_cert(ctx, t0, E, za.cert, uw);
      // (run lengths: with the fast prologue only -- every segment a whole group of this round's
      // grouped-order launch, the epoch from task 0, so gathered position = epoch task)
      if (fastp && R.runrem && ctx->t_zw_runrem) za.run_rem = P<int32_t>(ctx->run_rem);
      R.zpre = false;
      R.gcert = false;
      R.runrem = false;
      ea.cmax = P<double>(ctx->cmax);
      ea.coff = dev + EP_COFF;
      ea.nch = nch;
      ea.safe = dev + EP_SAFE;
      // the epoch tail: chains of different components write their windows back themselves
      // (chains that share a component, PVT_EPOCH_PLAN=0, can win each other's hosts at score 0:
      // no write-back, and no fast path in the validation -- every pair is checked)
      const bool apart = tail_chains_apart(R, t0, E);
      const bool opt = apart && tail_eligible(ctx);
      if (!apart) ea.cmax = nullptr;
      if (opt && (rc = tail_walk_args(ctx, za))) return rc;
      // (without the optimistic apply the chains' words go to the device, and come back with the
      // tail's readback)
      if (fastp && !opt) za.hcert = dev + EP_CERT;
      {
        Scope sc(ctx, PVT_K_COMMIT, 0, 0, nullptr, "zwalk_kernel");
        if (R.Z > ZMAX) launch_zwalk_wide(za, nch, big, st);
        else if (big) launch_zwalk_big(za, nch, st);
        else launch_zwalk(za, nch, st);
      }
      const bool was_big = big;
      big = false;
      HIPCHK(hipGetLastError());
      if (opt) {
        // one synchronisation, the verdict from the chains' own words: accepted whole, no further
        // launch; else the write-backs are undone and the tail decides as ever
        HIPCHK(hipStreamSynchronize(st));
        uint64_t wrote = 0;
        const uint64_t fastm = fastp ? fast_chains(ctx, nch) : 0;
        if (tail_accepted(ctx, E, true, &wrote)) {
          ctx->n_zchains += nch;
          ctx->n_longest += *std::max_element(E.len.begin(), E.len.end());
          t0 += nt;
          continue;
        }
        tail_undo(ctx, wrote, nch, fastm & wrote, &uw);
      }
      // validation, the accepted prefix and its apply all on the device, then one readback. A
      // chain the frontier walk could not prove is not accepted past its first segment; the
      // next epoch then walks its chains with candidate lists (force_lists) -- or, when a chain
      // only ran out of window hosts, once more with the large window.
      epoch_tail(ctx, ea, true, nch);
      HIPCHK(hipGetLastError());
      HIPCHK(hipStreamSynchronize(st));
      if (fastp && !opt) (void)fast_chains(ctx, nch);
      int adv = 0;
      if ((rc = epoch_frontier_verdict(ctx, E, t0, &need, &adv))) return rc;
      if (need && adv < nt) {
        R.wide_misses++;
        bool exhausted = false;
        for (int c = 0; c < nch; c++) exhausted |= host[EP_STATUS + 2 * c + 1] == 2;
        if (exhausted && !was_big && big_t0 != t0 + adv) {
          big = true;
          big_t0 = t0 + adv;
        } else {
          force_lists = true;
        }
      }
      t0 += adv;
      continue;
    }
    ctx->n_gchains += need;
    ctx->n_longest += *std::max_element(E.len.begin(), E.len.end());
    CommitArgs ca_ = commit_args(ctx, t0, nt, 0, 0, dev + EP_STATUS);
    ca_.prev_ids = nullptr;
    ca_.coff = dev + EP_COFF;
    ca_.cmap = dev + EP_CMAP;
    ca_.csoff = dev + EP_CSOFF;
    ca_.cseg = dev + EP_CSEG;
    ca_.wlog = P<WinRec>(ctx->wres);
    ca_.skip_done = zw ? 1 : 0;
    if (need) {
      {
        Scope sc(ctx, PVT_K_COMMIT, 0, 0, nullptr, "commit_kernel");
        launch_commit_chains(ca_, nch, st);
      }
      if ((rc = validate_and_read())) return rc;
    }
    // the exact prefix: segments before the first rejected one, up to and including the first
    // that its chain did not finish (its walked tasks are exact; the next epoch starts there)
    for (int c = 0; c < nch; c++)
      if (host[EP_STATUS + 2 * c] == -1)
        return fail(ctx, PVT_EHIP, "commit walk: ring hand-off timed out (epoch at task %d)", t0);
    int acc = 0, next = t0;
    for (int j = 0; j < nseg; j++) {
      const int len = E.off[j + 1] - E.off[j];
      const int adv = std::max(0, std::min(len, host[EP_STATUS + 2 * E.chain[j]] - E.cstart[j]));
      if (j > 0 && host[EP_BAD + j]) { ctx->n_rejected += nseg - j; break; }
      acc = j + 1;
      next = t0 + E.off[j] + adv;
      if (adv < len) { ctx->refills++; ctx->n_rejected += nseg - j - 1; break; }
    }
    if (next == t0) return fail(ctx, PVT_EHIP, "epoch made no progress at task %d", t0);
    {
      Scope sc(ctx, PVT_K_OTHER, 0, 0);
      launch_epoch_apply(ea, acc, nch, st);
    }
    HIPCHK(hipGetLastError());
    t0 = next;
  }
  return PVT_OK;
}
