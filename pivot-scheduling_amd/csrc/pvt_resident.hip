// pvt_resident.hip — rounds small enough for the resident kernel (pvt_batch.hip): the launch
// plan, pvt_place_batch's place_resident, and the host-array rounds (pvt_place_host,
// pvt_place_host_batch, pvt_restore_hosts) staged through pinned memory for it.
#include "pvt_driver.h"
#include "pvt_anchor.h"
#include "pvt_groups.h"

// ---------------------------------------------------------------- resident rounds / batches
bool pvt::resident_fits(const pvt_round* r, int max_hosts) {
  // (a cost_aware round of more than ZMAX zones runs the wide kernels, which hold at most
  // RES_WIDE_MAX_HPL hosts per lane; so does every round of a mixed batch with one: plan_check)
  const bool ca = r->mode == PVT_CA_FF || r->mode == PVT_CA_BF;
  const int cap = ca && r->n_zones > ZMAX ? RES_WIDE_MAX_HOSTS : (int)PVT_RESIDENT_MAX_HOSTS;
  return r->n_hosts <= std::min(max_hosts, cap) && r->n_tasks <= PVT_RESIDENT_MAX_TASKS;
}

template <class T>
static int ensure_pinned_array(pvt_ctx* ctx, T*& p, size_t& cap, size_t n) {
  if (cap >= n) return PVT_OK;
  const size_t want = std::max(n, cap * 3 / 2);
  if (p) (void)hipHostFree(p);
  p = nullptr;
  cap = 0;
  if (hipHostMalloc((void**)&p, sizeof(T) * want) != hipSuccess) {
    p = nullptr;
    return fail(ctx, PVT_ENOMEM, "hipHostMalloc(%zu) failed", sizeof(T) * want);
  }
  cap = want;
  return PVT_OK;
}

// The launch of a batch of resident rounds: its shape from the largest round, the A/B switches,
// the LDS it needs and the profiling scope's sums.
struct ResidentPlan {
  int n = 0, waves = 4, hpl = 1;
  int Zb = 1, Tpad = 64;          // LDS zone-table stride, sort network size (a power of two)
  ResidentSwitches sw;
  bool wide_kernel = false;       // a round of more than ZMAX zones (no zone tables in LDS: Zb = 0)
                                  //   and a policy that reads them, or mixed policies: the wide kernels
  size_t lds = 0;
  double cand = 0.0, bytes = 0.0;
};

// rounds[idx[k]], k < n (idx NULL: rounds[k]); waves: the preference resident_shape starts from;
// min_lds: LDS the launch needs beside the placement (the fused batch's grouping phases).
static ResidentPlan plan_resident(const pvt_ctx* ctx, const pvt_round* rounds, const int* idx, int n,
                                  int waves, size_t min_lds = 0) {
  ResidentPlan plan;
  plan.n = n;
  int maxH = 1, maxT = 1;
  bool tables = false, mixed = false;   // a cost_aware round; rounds of different policies
  for (int k = 0; k < n; k++) {
    const pvt_round& r = rounds[idx ? idx[k] : k];
    tables |= r.mode == PVT_CA_FF || r.mode == PVT_CA_BF;
    mixed |= r.mode != rounds[idx ? idx[0] : 0].mode;
    maxH = std::max(maxH, r.n_hosts);
    maxT = std::max(maxT, r.n_tasks);
    plan.Zb = std::max(plan.Zb, r.n_zones);
    const double c = (double)r.n_tasks * r.n_hosts;
    plan.cand += c;
    plan.bytes += c * bytes_per_candidate(r.mode);
  }
  const ResidentShape shape = resident_shape(waves, maxH);
  plan.waves = shape.waves;
  plan.hpl = shape.hpl;
  while (plan.Tpad < maxT) plan.Tpad <<= 1;
  plan.sw = resident_switches(ctx->rwalk, maxH);
  if (plan.Zb > ZMAX) {
    plan.Zb = 0;
    plan.wide_kernel = tables || mixed;
    if (plan.wide_kernel) {       // four waves, no one-wave walks (32-bit zone masks)
      plan.waves = 4;
      plan.hpl = resident_shape(4, maxH).hpl;
      plan.sw.walk_ca_bf = plan.sw.walk_ff = plan.sw.walk_rotate = plan.sw.walk_bulk = 0;
    }
  }
  plan.lds = std::max(resident_lds_bytes(plan.Zb, plan.Tpad, plan.sw), min_lds);
  return plan;
}

// A wide batch on the wide kernels holds at most RES_WIDE_MAX_HPL hosts per lane: every round of
// it, the narrow ones too.
static int plan_check(pvt_ctx* ctx, const ResidentPlan& plan) {
  if (plan.wide_kernel && plan.hpl > RES_WIDE_MAX_HPL)
    return fail(ctx, PVT_EUNSUPPORTED, "a batch with a round of more than %d zones takes rounds of at most "
                "%d hosts: place the larger rounds in a batch of their own", ZMAX, RES_WIDE_MAX_HOSTS);
  return PVT_OK;
}

// What pvt_last_resident_shape reports: the plan of the launch just made.
static void plan_launched(pvt_ctx* ctx, const ResidentPlan& plan) {
  ctx->rs_waves = plan.waves;
  ctx->rs_hpl = plan.hpl;
  ctx->rs_wide = plan.wide_kernel ? 1 : 0;
  ctx->rs_switches = resident_switches_word(plan.sw);
}

static ResidentArgs plan_args(const pvt_ctx* ctx, const ResidentPlan& plan, const void* desc, uint32_t* mt) {
  return ResidentArgs{desc, mt, plan.Zb, plan.Tpad, ctx->stamps, plan.sw};
}

// mode: the rounds' policy, or RES_MIXED; desc: their descriptors on the device
static int run_resident(pvt_ctx* ctx, const ResidentPlan& plan, int mode, const void* desc, uint32_t* mt) {
  int rc = plan_check(ctx, plan);
  if (rc) return rc;
  {
    Scope sc(ctx, PVT_K_SCORE, plan.cand, plan.bytes, nullptr, "resident_kernel");
    if (plan.wide_kernel)
      launch_resident_wide(mode, plan.hpl, plan.n, plan.lds, plan_args(ctx, plan, desc, mt), ctx->stream);
    else
      launch_resident(mode, plan.waves, plan.hpl, plan.n, plan.lds, plan_args(ctx, plan, desc, mt),
                      ctx->stream);
  }
  HIPCHK(hipGetLastError());
  plan_launched(ctx, plan);
  ctx->windows = plan.n;
  ctx->refills = 0;
  return PVT_OK;
}

// desc_dev: the rounds' descriptors already on the device (pvt_place_host's staging, MT states
// at mt_dev): nothing is copied and nothing waited for here; the caller copies back and syncs.
// mt_dev alone (pvt_place_batch_mt): the rounds' MT19937 states live on the device, [n][625].
int pvt::place_resident(pvt_ctx* ctx, const pvt_round* rounds, int n, const void* desc_dev,
                        uint32_t* mt_dev) {
  const int mode = rounds[0].mode;
  for (int i = 0; i < n; i++) {
    const pvt_round* r = &rounds[i];
    int rc = check_round(ctx, r);
    if (rc) return rc;
    if (r->mode != mode) return fail(ctx, PVT_EINVAL, "batch round %d: mode %d != %d", i, r->mode, mode);
    if (!resident_fits(r, PVT_RESIDENT_MAX_HOSTS))
      return fail(ctx, PVT_EUNSUPPORTED, "batch round %d: H=%d T=%d exceeds the resident limits (%d, %d; "
                  "%d hosts with more than %d zones)", i, r->n_hosts, r->n_tasks, PVT_RESIDENT_MAX_HOSTS,
                  PVT_RESIDENT_MAX_TASKS, RES_WIDE_MAX_HOSTS, ZMAX);
  }
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const ResidentPlan plan = plan_resident(ctx, rounds, nullptr, n, ctx->res_waves);
  if (desc_dev) return run_resident(ctx, plan, mode, desc_dev, mt_dev);
  int rc;
  // the staged descriptors (and MT states) reach the device by an upload kernel reading their
  // mapped pages when it runs: a new batch waits until the previous batch's upload has run
  if (ctx->rstage_busy) HIPCHK(hipEventSynchronize(ctx->ev_rstage));
  ctx->rstage_busy = false;
  if ((rc = ensure_pinned_array(ctx, ctx->rstage, ctx->rstage_cap, (size_t)n))) return rc;
  std::memcpy(ctx->rstage, rounds, sizeof(pvt_round) * n);
  ENSURE(ctx->rdesc, sizeof(pvt_round) * (size_t)n + 16);   // (+16: the upload's rounding)
  uint32_t* mt = nullptr;
  const bool host_mt = mode == PVT_OPP && !mt_dev;
  if (mode == PVT_OPP && mt_dev) {
    mt = mt_dev;
    for (int i = 0; i < n; i++) ctx->rstage[i].mt_state = mt + (size_t)i * 625;
  } else if (host_mt) {
    ENSURE(ctx->rmt, sizeof(uint32_t) * 625 * (size_t)n + 16);
    mt = P<uint32_t>(ctx->rmt);
    if ((rc = ensure_pinned_array(ctx, ctx->rmt_host, ctx->rmt_cap, (size_t)n * 625))) return rc;
    for (int i = 0; i < n; i++) {
      std::memcpy(ctx->rmt_host + (size_t)i * 625, rounds[i].mt_state, sizeof(uint32_t) * 625);
      ctx->rstage[i].mt_state = mt + (size_t)i * 625;   // the device copy the kernel draws from
    }
    void* dmt = nullptr;
    HIPCHK(hipHostGetDevicePointer(&dmt, ctx->rmt_host, 0));
    launch_upload(dmt, mt, sizeof(uint32_t) * 625 * n, st);
  }
  {
    void* dst = nullptr;
    HIPCHK(hipHostGetDevicePointer(&dst, ctx->rstage, 0));
    launch_upload(dst, ctx->rdesc.p, sizeof(pvt_round) * n, st);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ctx->ev_rstage, st));
  ctx->rstage_busy = true;
  if ((rc = run_resident(ctx, plan, mode, ctx->rdesc.p, mt))) return rc;
  if (host_mt)
    HIPCHK(hipMemcpyAsync(ctx->rmt_host, mt, sizeof(uint32_t) * 625 * n, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (host_mt)
    for (int i = 0; i < n; i++)
      std::memcpy(rounds[i].mt_state, ctx->rmt_host + (size_t)i * 625, sizeof(uint32_t) * 625);
  return PVT_OK;
}

// ---------------------------------------------------------------- drop-in rounds, host memory
static int ensure_pinned(pvt_ctx* ctx, size_t bytes) {
  if (ctx->hst_cap >= bytes) return PVT_OK;
  const size_t want = std::max({bytes, ctx->hst_cap * 3 / 2, (size_t)1 << 16});
  if (ctx->hst) (void)hipHostFree(ctx->hst);
  ctx->hst = nullptr;
  ctx->hst_map = nullptr;
  ctx->hst_cap = 0;
  if (hipHostMalloc(&ctx->hst, want) != hipSuccess) {
    ctx->hst = nullptr;
    return fail(ctx, PVT_ENOMEM, "hipHostMalloc(%zu) failed", want);
  }
  if (hipHostGetDevicePointer(&ctx->hst_map, ctx->hst, 0) != hipSuccess) {
    (void)hipHostFree(ctx->hst);
    ctx->hst = ctx->hst_map = nullptr;
    return fail(ctx, PVT_EHIP, "hipHostGetDevicePointer of the staging buffer failed");
  }
  ctx->hst_cap = want;
  return PVT_OK;
}

// One host-memory round's place in the staging buffer (pvt_place_host, pvt_place_host_batch):
// the out region (copied back: avail, placement, order, MT states, grouping status) of every
// round of a call comes first, so the results return with ONE copy.
struct HostSlot {
  size_t av = 0, pl = 0, orr = 0, mt = 0, cmt = 0, st = 0;
  size_t zone = 0, tb = 0, dc = 0, cost = 0, bw = 0, dem = 0, tg = 0, ga = 0, rt = 0;
  size_t ti = 0, off = 0, ph = 0, ia = 0, sz = 0, zs = 0, mh = 0, az = 0, ab = 0, desc = 0;
  size_t out_lo = 0, out_hi = 0, in_lo = 0, in_hi = 0;   // its byte ranges (fused host batch)
  const double* zt = nullptr;         // device zone tables (cost, then bw) when cached, else NULL
  int C = 0, S = 0, G = 0, GR = 0;
  int64_t NP = 0;
  bool resident = false, dev_mt = false;
  bool violated = false;              // pvt_set_checks: a content rule failed (check_host_round)
  pvt_round hr{};                     // the round as checked (grouped fields stand in with items)
  pvt_round d{};                      // the device round (arrays in the staging buffer)
};

// Validation of a host round and its optional fused-grouping items (pvt_place_host's contract).
static int check_host_round(pvt_ctx* ctx, const pvt_round* r, pvt_ca_items* it, HostSlot& s) {
  const bool ca = r->mode == PVT_CA_FF || r->mode == PVT_CA_BF;
  const int T = r->n_tasks, Z = r->n_zones;
  if (it) {
    if (!ca) return fail(ctx, PVT_EINVAL, "pvt_ca_items need a cost_aware round");
    if (it->reserved != 0 || it->n_items < 0 || it->n_apps < 0 || it->n_pred < 0 || it->n_storage < 0)
      return fail(ctx, PVT_EINVAL, "bad sizes in pvt_ca_items");
    if (r->task_group || r->group_anchor || r->rt_bw)
      return fail(ctx, PVT_EINVAL, "pvt_ca_items replace task_group / group_anchor (realtime_bw "
                  "rows are per group: use pvt_anchor + pvt_place)");
    if (!it->status || (T > 0 && (!it->task_item || !it->pred_off || (it->n_pred && !it->pred_host) ||
                                  (it->n_items && !it->item_app) || !it->storage_zone ||
                                  !it->zone_storage || !it->mt_state)))
      return fail(ctx, PVT_EINVAL, "null pointer in pvt_ca_items");
    it->status[0] = it->status[1] = 0;
    if (T > GRP_MAX_TASKS || it->n_storage + it->n_apps > GRP_MAX_KEYS || it->n_storage < 1)
      return fail(ctx, PVT_EUNSUPPORTED, "fused grouping limits: T=%d (max %d), %d storages + %d "
                  "applications (max %d, at least one storage)", T, GRP_MAX_TASKS, it->n_storage,
                  it->n_apps, GRP_MAX_KEYS);
    if (Z < 1 || Z > PVT_MAX_ZONES)
      return fail(ctx, PVT_EINVAL, "bad sizes H=%d T=%d Z=%d (1 <= Z <= PVT_MAX_ZONES = %d)", r->n_hosts, T, Z,
                  PVT_MAX_ZONES);
    for (int k = 0; k < it->n_storage; k++)
      if (it->storage_zone[k] < 0 || it->storage_zone[k] >= Z)
        return fail(ctx, PVT_EINVAL, "storage %d: zone %d outside [0, %d)", k, it->storage_zone[k], Z);
    for (int z = 0; z < Z; z++)
      if (it->zone_storage[z] < -1 || it->zone_storage[z] >= it->n_storage)
        return fail(ctx, PVT_EINVAL, "zone %d: storage %d outside [-1, %d)", z, it->zone_storage[z], it->n_storage);
    for (int c = 0; c <= it->n_items && T > 0; c++)   // (the anchor kernels check each range too)
      if (it->pred_off[c] < 0 || it->pred_off[c] > it->n_pred || (c && it->pred_off[c] < it->pred_off[c - 1]))
        return fail(ctx, PVT_EINVAL, "pred_off[%d] = %lld out of order or range", c, (long long)it->pred_off[c]);
  }
  s.hr = *r;
  static const int32_t one = 0;
  if (it) { s.hr.task_group = &one; s.hr.group_anchor = &one; s.hr.n_groups = 1; }
  int rc = check_round(ctx, &s.hr);
  if (rc) return rc;
  if (ctx->checks) {   // the content rules, through the predicates the device check uses
    pvt_check_report p;
    check_host_arrays(r, &p);
    if (p.code) {
      s.violated = true;
      return fail_check(ctx, -1, p);
    }
  }
  if (ca && T > 0)   // host arrays: the zone-table contract of include/pivot_place.h (cost, bw)
    for (int a = 0; a < Z; a++)
      for (int z = 0; z < Z; z++) {
        const double c = r->cost[a * Z + z] + r->cost[z * Z + a], b = r->bw[a * Z + z] + r->bw[z * Z + a];
        if (!(c >= 0.0) || !(b > 0.0))
          return fail(ctx, PVT_EINVAL, "zones (%d, %d): cost sum %g, bw sum %g (the engine needs "
                      "cost sums >= 0 and bw sums > 0)", a, z, c, b);
      }
  s.resident = T > 0 && resident_fits(&s.hr, ctx->resident_max);
  s.C = it ? it->n_items : 0;
  s.S = it ? it->n_storage : 0;
  s.NP = it ? it->n_pred : 0;
  s.G = it ? T : (r->task_group ? r->n_groups : 0);
  s.GR = r->rt_bw ? std::max(r->task_group ? r->n_groups : 1, 1) : 0;
  s.dev_mt = r->mt_state && s.resident;
  return PVT_OK;
}

// The device copy of a host round's zone tables, when they equal the cached ones (s.zt); the
// cache takes the tables of the first cost_aware round of a call that misses it (one small
// copy on the stream; every host-array call ends with a synchronisation, so no kernel of an
// earlier call still reads the old tables). may_fill = false: a miss leaves s.zt NULL and the
// round stages its own tables (a batch whose earlier round already reads the cached ones).
static int zone_cache(pvt_ctx* ctx, const pvt_round* r, HostSlot& s, bool may_fill = true) {
  s.zt = nullptr;
  if (!r->cost || !r->bw || r->n_tasks == 0) return PVT_OK;
  const int Z = r->n_zones;
  const size_t zz = (size_t)Z * Z;
  const bool hit = ctx->zt_Z == Z && ctx->zt_host.size() == 2 * zz &&
                   std::memcmp(ctx->zt_host.data(), r->cost, 8 * zz) == 0 &&
                   std::memcmp(ctx->zt_host.data() + zz, r->bw, 8 * zz) == 0;
  if (!hit) {
    if (!may_fill) return PVT_OK;
    ctx->zt_host.resize(2 * zz);
    std::memcpy(ctx->zt_host.data(), r->cost, 8 * zz);
    std::memcpy(ctx->zt_host.data() + zz, r->bw, 8 * zz);
    ctx->zt_Z = Z;
    ENSURE(ctx->zt_dev, 16 * zz);
    HIPCHK(hipMemcpyAsync(ctx->zt_dev.p, ctx->zt_host.data(), 16 * zz, hipMemcpyHostToDevice, ctx->stream));
  }
  s.zt = P<double>(ctx->zt_dev);
  return PVT_OK;
}

struct StageLayout {
  size_t o = 0;
  size_t take(size_t bytes) { const size_t at = o; o = (o + bytes + 255) / 256 * 256; return at; }
};

static void plan_out(StageLayout& L, HostSlot& s, const pvt_round* r, const pvt_ca_items* it) {
  const int H = r->n_hosts, T = r->n_tasks;
  s.out_lo = L.o;
  s.av = L.take(32 * (size_t)H);
  s.pl = L.take(4 * (size_t)T);
  s.orr = L.take(4 * (size_t)T);
  s.mt = r->mt_state ? L.take(4 * 625) : 0;
  s.cmt = it ? L.take(4 * 625) : 0;
  s.st = it ? L.take(16) : 0;
  s.out_hi = L.o;
}

static void plan_in(StageLayout& L, HostSlot& s, const pvt_round* r, const pvt_ca_items* it) {
  const int H = r->n_hosts, T = r->n_tasks, Z = r->n_zones;
  s.in_lo = L.o;
  s.zone = L.take(4 * (size_t)H);
  s.tb = r->tiebreak ? L.take(4 * (size_t)H) : 0;
  s.dc = r->decay ? L.take(4 * (size_t)H) : 0;
  s.cost = s.zt ? 0 : L.take(8 * (size_t)Z * Z);
  s.bw = s.zt ? 0 : L.take(8 * (size_t)Z * Z);
  s.dem = L.take(32 * (size_t)T);
  s.tg = (it || r->task_group) ? L.take(4 * (size_t)T) : 0;
  s.ga = (it || r->task_group) ? L.take(4 * (size_t)std::max(s.G, 1)) : 0;
  s.rt = s.GR ? L.take(8 * (size_t)s.GR * H) : 0;
  if (it) {
    s.ti = L.take(4 * (size_t)T);
    s.off = L.take(8 * (size_t)(s.C + 1));
    s.ph = L.take(4 * (size_t)std::max<int64_t>(s.NP, 1));
    s.ia = L.take(4 * (size_t)std::max(s.C, 1));
    s.sz = L.take(4 * (size_t)s.S);
    s.zs = L.take(4 * (size_t)Z);
    s.mh = L.take(4 * (size_t)std::max(s.C, 1));
    s.az = L.take(4 * (size_t)std::max(s.C, 1));
    s.ab = L.take(16 + 4 * (size_t)std::max(s.C, 1));
  }
  s.in_hi = L.o;
}

// The round's inputs into the pinned buffer and its device descriptor (arrays in the device
// copy of the buffer; a windowed opportunistic round's MT state stays a host pointer: opp_round
// moves it itself).
static void stage_round(char* hb, char* db, HostSlot& s, const pvt_round* r, const pvt_ca_items* it) {
  const int H = r->n_hosts, T = r->n_tasks, Z = r->n_zones;
  auto put = [&](size_t at, const void* src, size_t bytes) { if (bytes) std::memcpy(hb + at, src, bytes); };
  put(s.av, r->avail, 32 * (size_t)H);
  if (r->mt_state) put(s.mt, r->mt_state, 4 * 625);
  if (it) { put(s.cmt, it->mt_state, 4 * 625); std::memset(hb + s.st, 0, 16); }
  put(s.zone, r->zone, 4 * (size_t)H);
  if (r->tiebreak) put(s.tb, r->tiebreak, 4 * (size_t)H);
  if (r->decay) put(s.dc, r->decay, 4 * (size_t)H);
  if (!s.zt) {
    put(s.cost, r->cost, r->cost ? 8 * (size_t)Z * Z : 0);
    put(s.bw, r->bw, r->bw ? 8 * (size_t)Z * Z : 0);
  }
  put(s.dem, r->dem, 32 * (size_t)T);
  if (r->task_group) { put(s.tg, r->task_group, 4 * (size_t)T); put(s.ga, r->group_anchor, 4 * (size_t)s.G); }
  if (s.GR) put(s.rt, r->rt_bw, 8 * (size_t)s.GR * H);
  if (it) {
    put(s.ti, it->task_item, 4 * (size_t)T);
    put(s.off, it->pred_off, 8 * (size_t)(s.C + 1));
    put(s.ph, it->pred_host, 4 * (size_t)s.NP);
    put(s.ia, it->item_app, 4 * (size_t)s.C);
    put(s.sz, it->storage_zone, 4 * (size_t)s.S);
    put(s.zs, it->zone_storage, 4 * (size_t)Z);
    std::memset(hb + s.ab, 0, 16);
  }
  pvt_round& d = s.d;
  d = s.hr;
  d.avail = reinterpret_cast<double*>(db + s.av);
  d.zone = reinterpret_cast<const int32_t*>(db + s.zone);
  d.tiebreak = r->tiebreak ? reinterpret_cast<const uint32_t*>(db + s.tb) : nullptr;
  d.decay = r->decay ? reinterpret_cast<const int32_t*>(db + s.dc) : nullptr;
  d.cost = s.zt ? s.zt : r->cost ? reinterpret_cast<const double*>(db + s.cost) : nullptr;
  d.bw = s.zt ? s.zt + (size_t)Z * Z : r->bw ? reinterpret_cast<const double*>(db + s.bw) : nullptr;
  d.dem = reinterpret_cast<const double*>(db + s.dem);
  d.task_group = s.tg ? reinterpret_cast<const int32_t*>(db + s.tg) : nullptr;
  d.group_anchor = s.ga ? reinterpret_cast<const int32_t*>(db + s.ga) : nullptr;
  d.rt_bw = s.GR ? reinterpret_cast<const double*>(db + s.rt) : nullptr;
  d.placement = reinterpret_cast<int32_t*>(db + s.pl);
  d.order = reinterpret_cast<int32_t*>(db + s.orr);
  d.mt_state = s.dev_mt ? reinterpret_cast<uint32_t*>(db + s.mt) : r->mt_state;
  std::memcpy(hb + s.desc, &d, sizeof(pvt_round));
}

// The fused cost_aware grouping of an items round on the device (anchors, groups, draws); a
// resident round's descriptor receives its group count.
static void items_args(char* db, const HostSlot& s, const pvt_ca_items* it, AnchorArgs* ka,
                       CaGroupArgs* ga) {
  const int T = s.hr.n_tasks, H = s.hr.n_hosts, Z = s.hr.n_zones;
  int32_t* ab = reinterpret_cast<int32_t*>(db + s.ab);
  *ka = AnchorArgs{s.C, H, s.NP, 0, 0, reinterpret_cast<const int64_t*>(db + s.off), nullptr,
                   reinterpret_cast<const int32_t*>(db + s.ph), nullptr, s.d.zone,
                   reinterpret_cast<int32_t*>(db + s.mh), reinterpret_cast<int32_t*>(db + s.az), ab,
                   ab + 4, ab + 1};
  *ga = CaGroupArgs{T, s.C, Z, s.S, it->n_apps, reinterpret_cast<const int32_t*>(db + s.ti),
                    reinterpret_cast<const int32_t*>(db + s.az), reinterpret_cast<const int32_t*>(db + s.ia),
                    reinterpret_cast<const int32_t*>(db + s.sz), reinterpret_cast<const int32_t*>(db + s.zs),
                    reinterpret_cast<uint32_t*>(db + s.cmt), reinterpret_cast<int32_t*>(db + s.tg),
                    reinterpret_cast<int32_t*>(db + s.ga), reinterpret_cast<int32_t*>(db + s.st),
                    s.resident ? &reinterpret_cast<pvt_round*>(db + s.desc)->n_groups : nullptr};
}

static int launch_items(pvt_ctx* ctx, char* db, const HostSlot& s, const pvt_ca_items* it, hipStream_t st) {
  AnchorArgs k;
  CaGroupArgs g;
  items_args(db, s, it, &k, &g);
  {
    Scope sc(ctx, PVT_K_OTHER, 0, 4.0 * (double)s.NP);
    if (s.C > 0) launch_anchor(k, st);
    launch_ca_groups(g, st);
  }
  HIPCHK(hipGetLastError());
  return PVT_OK;
}

static int group_error(pvt_ctx* ctx, const char* hb, const HostSlot& s, pvt_ca_items* it) {
  const int32_t* hs = reinterpret_cast<const int32_t*>(hb + s.st);
  const int e = hs[1];
  it->status[0] = hs[0];
  it->status[1] = e;
  if (!e) return PVT_OK;
  return fail(ctx, PVT_EINVAL, "%s", e == 1 ? "a mode predecessor placement is not a host of the cluster" :
              e == 2 ? "an anchor zone has no storage (get_storage_by_locality -> None)" :
              "malformed anchor item lists");
}

static void return_round(const char* hb, const HostSlot& s, pvt_round* r, pvt_ca_items* it) {
  const int H = r->n_hosts, T = r->n_tasks;
  std::memcpy(r->avail, hb + s.av, 32 * (size_t)H);
  std::memcpy(r->placement, hb + s.pl, 4 * (size_t)T);
  std::memcpy(r->order, hb + s.orr, 4 * (size_t)T);
  if (s.dev_mt) std::memcpy(r->mt_state, hb + s.mt, 4 * 625);
  if (it) std::memcpy(it->mt_state, hb + s.cmt, 4 * 625);
}

// The staging buffer to the device and the results back as copy kernels over its mapped pages:
// a hipMemcpyAsync from or to pinned memory goes through the copy engine, and the next kernel
// on the stream started ~20 us after the copy was queued (launch_upload).
static void stage_up(pvt_ctx* ctx, size_t bytes, hipStream_t st) {
  launch_upload(ctx->hst_map, ctx->hdev.p, bytes, st);
}
static void stage_down(pvt_ctx* ctx, size_t bytes, hipStream_t st) {
  launch_upload(ctx->hdev.p, ctx->hst_map, bytes, st);   // (the same copy kernel, device -> mapped)
}

extern "C" int pvt_place_host(pvt_ctx* ctx, pvt_round* r, pvt_ca_items* it) {
  if (!ctx || !r) return PVT_EINVAL;
  HostSlot s;
  int rc = check_host_round(ctx, r, it, s);
  if (rc) return rc;
  ctx->rs.active = false;
  if (r->n_tasks == 0) return PVT_OK;
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  if ((rc = zone_cache(ctx, r, s))) return rc;
  StageLayout L;
  plan_out(L, s, r, it);
  const size_t n_out = L.o;
  plan_in(L, s, r, it);
  s.desc = L.take(sizeof(pvt_round));
  if ((rc = ensure_pinned(ctx, L.o))) return rc;
  ENSURE(ctx->hdev, L.o);
  char* hb = static_cast<char*>(ctx->hst);
  char* db = static_cast<char*>(ctx->hdev.p);
  stage_round(hb, db, s, r, it);
  stage_up(ctx, L.o, st);
  HIPCHK(hipGetLastError());
  if (it && (rc = launch_items(ctx, db, s, it, st))) return rc;
  if (s.resident) {
    if ((rc = place_resident(ctx, &s.d, 1, db + s.desc, s.dev_mt ? reinterpret_cast<uint32_t*>(db + s.mt) : nullptr)))
      return rc;
  } else {
    if (it) {                         // the windowed engine plans groups on the host
      launch_upload(db + s.st, static_cast<char*>(ctx->hst_map) + s.st, 16, st);
      HIPCHK(hipStreamSynchronize(st));
      if ((rc = group_error(ctx, hb, s, it))) return rc;
      s.d.n_groups = std::max(reinterpret_cast<const int32_t*>(hb + s.st)[0], 1);
    }
    if ((rc = place_windowed(ctx, &s.d))) return rc;
  }
  stage_down(ctx, n_out, st);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  if (it && (rc = group_error(ctx, hb, s, it))) return rc;
  return_round(hb, s, r, it);
  return PVT_OK;
}

extern "C" int pvt_restore_hosts(pvt_ctx* ctx, double* avail, const double* avail0, int32_t n_hosts,
                                 const int32_t* hosts, int32_t n) {
  if (!ctx || n < 0 || n_hosts < 0 || (n > 0 && (!avail || !avail0 || !hosts))) return PVT_EINVAL;
  HIPCHK(hipSetDevice(ctx->device));
  launch_restore_hosts(avail, avail0, n_hosts, hosts, n, ctx->stream);
  HIPCHK(hipGetLastError());
  return PVT_OK;
}

// A host batch as staged (pvt_place_host_batch).
struct HostBatch {
  pvt_round* rounds;
  pvt_ca_items* const* items;        // per round, or NULL
  std::vector<HostSlot> s;           // per round
  std::vector<int> live, withit;     // the rounds with tasks; those of them with items
  int mode = -1;                     // the live rounds' policy, or RES_MIXED
  size_t o_fr = 0, o_ka = 0, o_kg = 0;   // stage offsets: FusedRound[live], AnchorArgs / CaGroupArgs[withit]
  pvt_ca_items* it(int i) const { return items ? items[i] : nullptr; }
};

// The staged host batch in ONE launch (resident_fused_kernel, pvt_batch.hip): every round's
// workgroup copies its ranges of the mapped stage to the device copy, runs its grouping (items)
// and its placement, and copies its results back; one synchronisation. PVT_FUSED=0: the staged
// upload / anchor / grouping / placement / download launches instead (A/B).
static int place_host_fused(pvt_ctx* ctx, const HostBatch& B) {
  char* hb = static_cast<char*>(ctx->hst);
  FusedRound* fr = reinterpret_cast<FusedRound*>(hb + B.o_fr);
  for (size_t k = 0; k < B.live.size(); k++) {
    const HostSlot& h = B.s[B.live[k]];
    fr[k] = FusedRound{(int64_t)h.out_lo, (int64_t)h.out_hi, (int64_t)h.in_lo, (int64_t)h.in_hi,
                       (int64_t)h.desc, -1, 0};
  }
  for (size_t k = 0; k < B.withit.size(); k++)
    for (size_t j = 0; j < B.live.size(); j++)
      if (B.live[j] == B.withit[k]) fr[j].items = (int32_t)k;
  const ResidentPlan plan = plan_resident(ctx, B.rounds, B.live.data(), (int)B.live.size(), 4,
                                          B.withit.empty() ? 0 : fused_pre_lds_bytes());
  int rc = plan_check(ctx, plan);
  if (rc) return rc;
  FusedArgs F{static_cast<const char*>(ctx->hst_map), static_cast<char*>(ctx->hdev.p),
              (int64_t)B.o_fr, (int64_t)B.o_ka, (int64_t)B.o_kg, plan_args(ctx, plan, nullptr, nullptr)};
  {
    Scope sc(ctx, PVT_K_SCORE, plan.cand, plan.bytes, nullptr, "resident_fused_kernel");
    if (plan.wide_kernel) launch_fused_wide(B.mode, plan.hpl, plan.n, plan.lds, F, ctx->stream);
    else launch_fused(B.mode, plan.hpl, plan.n, plan.lds, F, ctx->stream);
  }
  HIPCHK(hipGetLastError());
  plan_launched(ctx, plan);
  ctx->windows = plan.n;
  ctx->refills = 0;
  return PVT_OK;
}

extern "C" int pvt_place_host_batch(pvt_ctx* ctx, pvt_round* rounds, pvt_ca_items* const* items,
                                    int32_t n_rounds, int32_t* rcs) {
  if (!ctx) return PVT_EINVAL;
  if (n_rounds < 0 || (n_rounds > 0 && (!rounds || !rcs)))
    return fail(ctx, PVT_EINVAL, "bad host batch (%d rounds)", n_rounds);
  ctx->rs.active = false;
  if (n_rounds == 0) return PVT_OK;
  HostBatch B{rounds, items, std::vector<HostSlot>(n_rounds)};
  std::vector<HostSlot>& s = B.s;
  std::vector<int>& live = B.live;
  std::vector<int>& withit = B.withit;
  int rc;
  bool mixed = false;   // (an empty round launches nothing and mixes no modes)
  std::string violation;   // pvt_set_checks: the first violating round's text
  for (int i = 0; i < n_rounds; i++) {
    rcs[i] = PVT_OK;
    if ((rc = check_host_round(ctx, &rounds[i], B.it(i), s[i]))) {
      char msg[64];
      std::snprintf(msg, sizeof(msg), "host batch round %d: ", i);
      ctx->err = msg + ctx->err;
      if (!s[i].violated) return rc;
      rcs[i] = rc;                   // every round gets its own verdict; nothing is launched
      if (violation.empty()) violation = ctx->err;
      continue;
    }
    if (rounds[i].n_tasks > 0 && !s[i].resident)
      return fail(ctx, PVT_EUNSUPPORTED, "host batch round %d: H=%d T=%d exceeds the resident limits "
                  "(%d, %d): place it with pvt_place_host", i, rounds[i].n_hosts, rounds[i].n_tasks,
                  std::min(ctx->resident_max, (int)PVT_RESIDENT_MAX_HOSTS), PVT_RESIDENT_MAX_TASKS);
    if (rounds[i].n_tasks == 0) continue;
    live.push_back(i);
    if (B.it(i)) withit.push_back(i);
    mixed |= rounds[i].mode != rounds[live[0]].mode;
  }
  if (!violation.empty()) return fail(ctx, PVT_EINVAL, "%s", violation.c_str());
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  if (live.empty()) return PVT_OK;
  B.mode = mixed ? RES_MIXED : rounds[live[0]].mode;
  // out regions of every round, then the inputs, then the descriptors of the rounds with tasks
  // (contiguous: one resident launch takes them all)
  StageLayout L;
  for (int i : live) plan_out(L, s[i], &rounds[i], B.it(i));
  const size_t n_out = L.o;
  // the cached zone tables: refilled at most by the first round that takes them (a later refill
  // would replace the tables that round reads in the same launch)
  bool may_fill = true;
  for (int i : live) {
    if ((rc = zone_cache(ctx, &rounds[i], s[i], may_fill))) return rc;
    if (s[i].zt) may_fill = false;
  }
  for (int i : live) plan_in(L, s[i], &rounds[i], B.it(i));
  // the fused groupings of every cost_aware round: their kernel arguments in the stage, so the
  // anchors and the groups of all of them take three launches
  const int ni = (int)withit.size();
  B.o_ka = ni ? L.take(sizeof(AnchorArgs) * ni) : 0;
  const size_t o_kb = ni ? L.take(sizeof(int32_t) * (ni + 1)) : 0;
  B.o_kg = ni ? L.take(sizeof(CaGroupArgs) * ni) : 0;
  const size_t o_desc = L.take(sizeof(pvt_round) * live.size());
  for (size_t k = 0; k < live.size(); k++) s[live[k]].desc = o_desc + sizeof(pvt_round) * k;
  const bool fused = ctx->fused != 0;
  B.o_fr = fused ? L.take(sizeof(FusedRound) * live.size()) : 0;
  if ((rc = ensure_pinned(ctx, L.o))) return rc;
  ENSURE(ctx->hdev, L.o);
  char* hb = static_cast<char*>(ctx->hst);
  char* db = static_cast<char*>(ctx->hdev.p);
  for (int i : live) stage_round(hb, db, s[i], &rounds[i], B.it(i));
  int nab = 0;
  for (int k = 0; k < ni; k++) {
    const int i = withit[k];
    AnchorArgs ka;
    CaGroupArgs ga;
    items_args(db, s[i], items[i], &ka, &ga);
    std::memcpy(hb + B.o_ka + sizeof(AnchorArgs) * k, &ka, sizeof(AnchorArgs));
    std::memcpy(hb + B.o_kg + sizeof(CaGroupArgs) * k, &ga, sizeof(CaGroupArgs));
    reinterpret_cast<int32_t*>(hb + o_kb)[k] = nab;
    nab += anchor_batch_blocks(s[i].C);
  }
  if (ni) reinterpret_cast<int32_t*>(hb + o_kb)[ni] = nab;
  if (fused) {
    if ((rc = place_host_fused(ctx, B))) return rc;
  } else {
    stage_up(ctx, L.o, st);
    HIPCHK(hipGetLastError());
    if (ni) {
      double np = 0.0;
      for (int i : withit) np += (double)s[i].NP;
      Scope sc(ctx, PVT_K_OTHER, 0, 4.0 * np);
      launch_anchor_batch(reinterpret_cast<const AnchorArgs*>(db + B.o_ka),
                          reinterpret_cast<const int32_t*>(db + o_kb), ni, nab, st);
      launch_ca_groups_batch(reinterpret_cast<const CaGroupArgs*>(db + B.o_kg), ni, st);
    }
    HIPCHK(hipGetLastError());
    // one resident launch for every round (one workgroup each; mixed policies branch per
    // workgroup), the MT states read and written through each descriptor's mt_state
    const ResidentPlan plan = plan_resident(ctx, rounds, live.data(), (int)live.size(),
                                            mixed ? 4 : ctx->res_waves);
    if ((rc = run_resident(ctx, plan, B.mode, db + o_desc, nullptr))) return rc;
    stage_down(ctx, n_out, st);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipStreamSynchronize(st));
  for (int i : live) {
    pvt_ca_items* it = B.it(i);
    if (it && (rcs[i] = group_error(ctx, hb, s[i], it))) continue;
    return_round(hb, s[i], &rounds[i], it);
  }
  return PVT_OK;
}
