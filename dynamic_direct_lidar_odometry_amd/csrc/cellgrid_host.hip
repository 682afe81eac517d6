// cellgrid_host.hip — host side of a target's candidate cells: the build
// (cellgrid_build drives cellgrid.hip's kernels and hipcub's select / scan),
// the policy that decides when a target gets its cells (maybe_build_grid,
// declared in cellgrid.hpp) and the two C entry points about them.
#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "capi_internal.hpp"
#include "cellgrid.hpp"

// Candidate cells of a target (cellgrid.hip): coarse cells of
// kGridCell metres over the target's box plus the bound's reach, split up to
// 3 times where lists are longer than kGridListMax points.
namespace {

constexpr double kGridCell = 0.4;
constexpr double kGridMaxReach = 4.0;     // bounds beyond this: cells farther than it use the walk
constexpr int kGridListMax = 32;
constexpr int kGridAutoAligns = 32;       // GICP_GRID_AUTO: built at this align against the same target and bound
constexpr int kGridListCap = kCgCandMax;  // finest level: longer lists are not stored (the walk)
constexpr long kGridMaxCells = 48L << 20; // coarse cells (the directory is 8 B per cell)

gicp_status cellgrid_build(gicp_ctx* c, CloudData& cd, float cap2, std::shared_ptr<CellGridData>* out) {
  hipStream_t s = c->stream;
  auto g = std::make_shared<CellGridData>();
  g->cap2 = cap2;
  *out = g;
  float q[8];
  HIP_TRY(hipMemcpyAsync(q, cd.quant.p, sizeof(float) * 7, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  const double S = kGridCell;
  const double capm = std::sqrt((double)cap2) * (1.0 + 1e-5) + 1e-6;
  const double reach = std::min(capm, kGridMaxReach);
  const int r = (int)std::ceil(reach / S) + 1;
  const double M = (r + 1) * S;   // the box: the target's bbox plus M on every side
  double lo[3], ext[3];
  long dims[3];
  double amax = 0.0;
  for (int a = 0; a < 3; ++a) {
    lo[a] = (double)q[a] - M;
    ext[a] = (double)q[4 + a] - (double)q[a] + 2 * M;
    dims[a] = (long)std::ceil(ext[a] / S) + 1;
    amax = std::max({amax, std::fabs((double)q[a]), std::fabs((double)q[4 + a])});
  }
  const long ncells = dims[0] * dims[1] * dims[2];
  if (ncells > kGridMaxCells || !std::isfinite(ext[0] + ext[1] + ext[2])) return GICP_OK;   // not built: the walk
  const size_t cap_bytes = c->grid_max_mb > 0 ? ((size_t)c->grid_max_mb << 20) : ~(size_t)0;
  if ((size_t)ncells * sizeof(unsigned long long) > cap_bytes)
    return fail(GICP_ENOMEM, "candidate cells: the directory exceeds GICP_OPT_GRID_MAX_MB");
  hipEvent_t e0, e1;
  HIP_TRY(hipEventCreate(&e0));
  HIP_TRY(hipEventCreate(&e1));
  struct EvGuard {
    hipEvent_t a, b;
    ~EvGuard() {
      (void)hipEventDestroy(a);
      (void)hipEventDestroy(b);
    }
  } evg{e0, e1};
  HIP_TRY(hipEventRecord(e0, s));
  CgBuild b{};
  b.tgt = cd.dev();
  // the build's geometry is the lookup's fp32 origin and scale, exactly
  b.fox = (float)lo[0]; b.foy = (float)lo[1]; b.foz = (float)lo[2];
  b.inv_s = (float)(1.0 / S);
  b.ox = b.fox; b.oy = b.foy; b.oz = b.foz;
  b.s = 1.0 / (double)b.inv_s;
  b.nx = (int)dims[0]; b.ny = (int)dims[1]; b.nz = (int)dims[2];
  b.r = r;
  // the lookup maps a query to its cell in fp32: |error| <~ 3 ulp of the
  // coordinate; every box is widened by delta to cover it
  b.delta = 1e-4 + 4e-6 * (amax + M + S);
  b.capm = capm;
  b.nomatch_dist = (r - 1) * S - 1e-3;
  static const int lmax_env = [] {   // development A/B of the list length (DDLO_GRID_LMAX)
    const char* v = dev_getenv("DDLO_GRID_LMAX");
    return v && *v ? std::atoi(v) : 0;
  }();
  b.lmax = lmax_env > 0 ? lmax_env : kGridListMax;
  b.lcap = kGridListCap;
  const bool outside_nomatch = capm <= b.nomatch_dist;
  // scratch
  const long nbx = (dims[0] + 3) / 4, nby = (dims[1] + 3) / 4, nbz = (dims[2] + 3) / 4;
  const long nblocked = nbx * nby * nbz * 64;
  {   // the per-cell scratch and directory (~21 B per coarse cell) must fit in free device memory with room
      // for the lists; otherwise the build is not attempted (the walk answers: maybe_build_grid)
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) == hipSuccess && (size_t)ncells * 21 + ((size_t)256 << 20) > fr)
      return fail(GICP_ENOMEM, "candidate cells: not enough free device memory for the build");
  }
  DevBuf rep, rep_tmp, flags, ctr, band, dnum, cub_tmp, cnn, db_buf;
  HIP_TRY(rep.ensure(sizeof(int) * (size_t)ncells));
  HIP_TRY(rep_tmp.ensure(sizeof(int) * (size_t)ncells));
  HIP_TRY(flags.ensure((size_t)std::max(nblocked, ncells)));
  HIP_TRY(ctr.ensure(sizeof(unsigned) * kCgCtrWords));
  HIP_TRY(band.ensure(sizeof(int) * (size_t)ncells));
  HIP_TRY(dnum.ensure(sizeof(int) * 8));
  HIP_TRY(db_buf.ensure(sizeof(CgBuild)));
  HIP_TRY(g->dir.ensure(sizeof(unsigned long long) * (size_t)ncells));
  b.rep = rep.as<int>();
  b.rep_tmp = rep_tmp.as<int>();
  b.rep_final = rep.as<int>();   // x: rep -> tmp, y: tmp -> rep, z: rep -> tmp; see below
  b.dir = g->dir.as<unsigned long long>();
  b.band = band.as<int>();
  b.ctr = ctr.as<unsigned>();
  CgBuild* db = db_buf.as<CgBuild>();
  auto upload = [&]() -> hipError_t { return hipMemcpyAsync(db, &b, sizeof(CgBuild), hipMemcpyHostToDevice, s); };
  b.rep_final = rep_tmp.as<int>();
  HIP_TRY(upload());
  HIP_TRY(hipMemsetAsync(rep.p, 0x7f, sizeof(int) * (size_t)ncells, s));   // 0x7f7f7f7f: none (> any position)
  HIP_TRY(hipMemsetAsync(ctr.p, 0, sizeof(unsigned) * kCgCtrWords, s));
  launch_cg_occ(s, db, cd.n);
  launch_cg_prop(s, db, 0, b.rep, b.rep_tmp, ncells);
  launch_cg_prop(s, db, 1, b.rep_tmp, b.rep, ncells);
  launch_cg_prop(s, db, 2, b.rep, b.rep_tmp, ncells);   // band: rep_tmp != none
  launch_cg_dir_fill(s, b.dir, b.rep_tmp, ncells, outside_nomatch ? kCgNoMatch : kCgFallback);
  launch_cg_band_flags(s, db, b.rep_tmp, flags.as<unsigned char>(), nblocked);
  HIP_TRY(hipGetLastError());
  // band cells in blocked order (selected blocked ids; k_cg_centers turns them into cell ids)
  auto select = [&](const unsigned char* fl, long n, int* outp, int* nsel) -> gicp_status {
    size_t tb = 0;
    hipcub::CountingInputIterator<int> it(0);
    HIP_TRY(hipcub::DeviceSelect::Flagged(nullptr, tb, it, fl, outp, dnum.as<int>(), (int)n, s));
    HIP_TRY(cub_tmp.ensure(std::max<size_t>(tb, 256)));
    tb = cub_tmp.bytes;
    HIP_TRY(hipcub::DeviceSelect::Flagged(cub_tmp.p, tb, it, fl, outp, dnum.as<int>(), (int)n, s));
    HIP_TRY(hipMemcpyAsync(c->flag_host, dnum.p, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *nsel = *c->flag_host;
    return GICP_OK;
  };
  int nband = 0;
  gicp_status st = select(flags.as<unsigned char>(), nblocked, b.band, &nband);
  if (st) return st;
  g->info.coarse_cells = ncells;
  g->info.band_cells = nband;
  g->info.cell_size = (float)S;
  // level-0 lists
  DevBuf hdr[4], pool[4], cmax[4], sband[4], sparent[4], fin_sel[4], fl_final, fl_next;
  int nfin[4] = {0, 0, 0, 0}, nslot[4] = {0, 0, 0, 0};
  if (nband > 0) {
    HIP_TRY(cnn.ensure(sizeof(int) * (size_t)nband));
    b.cnn = cnn.as<int>();
    HIP_TRY(upload());
    launch_cg_centers(s, db, nband);
    HIP_TRY(hdr[0].ensure(sizeof(uint2) * (size_t)nband));
    HIP_TRY(fl_final.ensure((size_t)nband));
    HIP_TRY(fl_next.ensure((size_t)nband));
    nslot[0] = nband;
  }
  std::vector<unsigned> counters(kCgCtrWords);
  auto read_counters = [&]() -> gicp_status {
    HIP_TRY(hipMemcpyAsync(counters.data(), ctr.p, sizeof(unsigned) * kCgCtrWords, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return GICP_OK;
  };
  for (int l = 0; l <= kCgMaxLevel && nslot[l] > 0; ++l) {
    const long nf = 1L << (3 * l);
    // the level's lists: pools sized from the parent level, doubled on overflow
    // (a wave's chunks leave at most kCgChunk unused entries per shard range)
    size_t used_above = 0;
    if (l > 0)
      for (int k = 0; k < kCgShardsHost; ++k) used_above += counters[(kCgCounters + (l - 1) * kCgShardsHost + k) * 32];
    size_t pcap = l == 0 ? (size_t)nband * 64 + (1u << 23) : 3 * used_above + (size_t)nslot[l] * nf * 4 + (1u << 23);
    for (int attempt = 0;; ++attempt) {
      pcap = std::min<size_t>(pcap, 0xfff00000u);
      HIP_TRY(pool[l].ensure(sizeof(unsigned) * pcap));
      b.lv[l].pool = pool[l].as<unsigned>();
      b.lv[l].pool_cap = (unsigned)(pcap / kCgShardsHost * kCgShardsHost);
      if (l > 0) {
        HIP_TRY(hdr[l].ensure(sizeof(uint2) * (size_t)nslot[l] * nf));
        b.lv[l].hdr = hdr[l].as<uint2>();
      } else {
        b.lv[0].hdr = hdr[0].as<uint2>();
      }
      HIP_TRY(upload());
      HIP_TRY(hipMemsetAsync(ctr.as<unsigned>() + (kCgCounters + l * kCgShardsHost) * 32, 0,
                             sizeof(unsigned) * kCgShardsHost * 32, s));
      HIP_TRY(hipMemsetAsync(ctr.as<unsigned>() + kCtrPoolFull * 32, 0, sizeof(unsigned), s));
      if (l == 0) launch_cg_coarse(s, db, nband);
      else launch_cg_refine(s, db, l, nslot[l]);
      HIP_TRY(hipGetLastError());
      st = read_counters();
      if (st) return st;
      if (!counters[kCtrPoolFull * 32]) break;
      if (attempt >= 4 || pcap >= 0xfff00000u) return fail(GICP_ENOMEM, "candidate cells: list pool overflow");
      pcap *= 2;
    }
    // decisions: final at this level, or split once more
    HIP_TRY(fl_final.ensure((size_t)nslot[l]));
    HIP_TRY(fl_next.ensure((size_t)nslot[l]));
    launch_cg_decide(s, db, l, nslot[l], fl_final.as<unsigned char>(), fl_next.as<unsigned char>());
    HIP_TRY(fin_sel[l].ensure(sizeof(int) * (size_t)nslot[l]));
    st = select(fl_final.as<unsigned char>(), nslot[l], fin_sel[l].as<int>(), &nfin[l]);
    if (st) return st;
    if (l < kCgMaxLevel) {
      HIP_TRY(sparent[l + 1].ensure(sizeof(int) * (size_t)nslot[l] + 64));
      int nn = 0;
      st = select(fl_next.as<unsigned char>(), nslot[l], sparent[l + 1].as<int>(), &nn);
      if (st) return st;
      nslot[l + 1] = nn;
      if (nn > 0) {
        HIP_TRY(sband[l + 1].ensure(sizeof(int) * (size_t)nn));
        HIP_TRY(cmax[l + 1].ensure(sizeof(int) * (size_t)nn));
        b.lv[l + 1].slot_parent = sparent[l + 1].as<int>();
        b.lv[l + 1].slot_band = sband[l + 1].as<int>();
        b.lv[l + 1].cmax = cmax[l + 1].as<int>();
        b.lv[l + 1].slot_cap = nn;
        HIP_TRY(upload());
        launch_cg_slots(s, db, l + 1, nn);
      }
    }
  }
  // emission: per level, list entries and fine cells of each final, scanned
  DevBuf ent_n[4], fine_n[4];
  unsigned ent_base[5] = {0, 0, 0, 0, 0}, fine_base[5] = {0, 0, 0, 0, 0};
  for (int l = 0; l <= kCgMaxLevel; ++l) {
    ent_base[l + 1] = ent_base[l];
    fine_base[l + 1] = fine_base[l];
    g->info.level_cells[l] = nfin[l];
    if (nfin[l] == 0) continue;
    HIP_TRY(ent_n[l].ensure(sizeof(unsigned) * ((size_t)nfin[l] + 1)));
    HIP_TRY(fine_n[l].ensure(sizeof(unsigned) * ((size_t)nfin[l] + 1)));
    launch_cg_emit_count(s, db, l, fin_sel[l].as<int>(), nfin[l], ent_n[l].as<unsigned>(), fine_n[l].as<unsigned>());
    for (DevBuf* v : {&ent_n[l], &fine_n[l]}) {
      // exclusive scan in place over nfin + 1 entries (the last one = the total)
      HIP_TRY(hipMemsetAsync(v->as<unsigned>() + nfin[l], 0, sizeof(unsigned), s));
      size_t tb = 0;
      HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, v->as<unsigned>(), v->as<unsigned>(), nfin[l] + 1, s));
      HIP_TRY(cub_tmp.ensure(std::max<size_t>(tb, 256)));
      tb = cub_tmp.bytes;
      HIP_TRY(hipcub::DeviceScan::ExclusiveSum(cub_tmp.p, tb, v->as<unsigned>(), v->as<unsigned>(), nfin[l] + 1, s));
    }
    unsigned tot[2];
    HIP_TRY(hipMemcpyAsync(&tot[0], ent_n[l].as<unsigned>() + nfin[l], sizeof(unsigned), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&tot[1], fine_n[l].as<unsigned>() + nfin[l], sizeof(unsigned), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    ent_base[l + 1] += tot[0];
    fine_base[l + 1] += tot[1];
  }
  if ((size_t)fine_base[4] >= 0x3ffffffeu) return fail(GICP_ENOMEM, "candidate cells: fine table too large");
  if ((size_t)ncells * sizeof(unsigned long long) + sizeof(uint2) * (size_t)fine_base[4] +
          sizeof(float4) * (size_t)ent_base[4] > cap_bytes)
    return fail(GICP_ENOMEM, "candidate cells: the lists exceed GICP_OPT_GRID_MAX_MB");
  HIP_TRY(g->fine.ensure(sizeof(uint2) * std::max<size_t>(fine_base[4], 1)));
  HIP_TRY(g->ent.ensure(sizeof(float4) * ((size_t)ent_base[4] + kCgEntPad)));   // (the pad: a round's reads past the last list)
  b.fine = g->fine.as<uint2>();
  b.ent = g->ent.as<float4>();
  HIP_TRY(upload());
  for (int l = 0; l <= kCgMaxLevel; ++l)
    if (nfin[l] > 0)
      launch_cg_emit_write(s, db, l, fin_sel[l].as<int>(), nfin[l], ent_n[l].as<unsigned>(), fine_n[l].as<unsigned>(),
                           ent_base[l], fine_base[l]);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(e1, s));
  st = read_counters();   // (waits for the build)
  if (st) return st;
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
  g->info.build_ms = ms;
  g->info.nomatch_cells = nband - nfin[0] - nslot[1];   // band cells neither final at level 0 nor split
  g->info.overflow_cells = counters[kCtrOverflow * 32];
  g->info.fallback_fine = counters[kCtrFineFb * 32];
  g->info.fine_cells = (int64_t)fine_base[4] - g->info.fallback_fine;
  g->info.entries = ent_base[4];
  g->info.bytes = (int64_t)(g->dir.bytes + g->fine.bytes + g->ent.bytes);
  {   // the build's transient scratch at its peak (released on return)
    size_t sb = rep.bytes + rep_tmp.bytes + flags.bytes + ctr.bytes + band.bytes + dnum.bytes + cub_tmp.bytes +
                cnn.bytes + db_buf.bytes + fl_final.bytes + fl_next.bytes;
    for (int l = 0; l <= kCgMaxLevel; ++l)
      sb += hdr[l].bytes + pool[l].bytes + cmax[l].bytes + sband[l].bytes + sparent[l].bytes + fin_sel[l].bytes +
            ent_n[l].bytes + fine_n[l].bytes;
    g->info.scratch_bytes = (int64_t)sb;
  }
  g->info.built = 1;
  CellGridDev& d = g->dev;
  d.dir = g->dir.as<unsigned long long>();
  d.fine = g->fine.as<uint2>();
  d.ent = g->ent.as<float4>();
  d.ox = b.fox;
  d.oy = b.foy;
  d.oz = b.foz;
  d.inv_s = b.inv_s;
  d.nx = b.nx;
  d.ny = b.ny;
  d.nz = b.nz;
  d.outside_nomatch = outside_nomatch ? 1 : 0;
  d.has_fallback = (g->info.fallback_fine > 0 || !outside_nomatch) ? 1 : 0;
  g->info.uses_walk = d.has_fallback;
  g->ok = true;
  return GICP_OK;
}

}  // namespace

// gicp_set_target_grid policy: build the target's candidate cells for this
// ctx's bound (auto: at the kGridAutoAligns-th (32nd) align against the same
// target and bound)
gicp_status ddlo::rt::maybe_build_grid(gicp_ctx* c) {
  if (!c->grid_mode || !c->tgt.cloud) return GICP_OK;
  CloudData& t = *c->tgt.cloud;
  const float cap2 = search_cap2(c->params);
  if (t.grid && t.grid->cap2 == cap2) return GICP_OK;   // built (or found too large) for this bound
  if (t.grid_aligns_cap2 != cap2) {
    t.grid_aligns_cap2 = cap2;
    t.grid_aligns = 0;
  }
  ++t.grid_aligns;
  // auto: only a target aligned against many times pays for its cells (a
  // ~16 ms build for a 500k-point submap against ~0.15 ms saved per align);
  // OdomNode's submaps live ~20 scans (DESIGN.md §4 "Candidate cells")
  if (c->grid_mode == GICP_GRID_AUTO && t.grid_aligns < kGridAutoAligns) return GICP_OK;
  std::shared_ptr<CellGridData> g;
  const gicp_status s = cellgrid_build(c, t, cap2, &g);
  if (s) {
    // The cells are an optional speed-up: a build that fails (pool or table
    // limits, the byte budget, device memory) leaves this target on the walk
    // for this bound and is not retried.  Only a device fault (the stream no
    // longer synchronizes) is the align's error.
    g.reset();   // its partial buffers are released (nothing queued reads them)
    (void)hipGetLastError();
    if (hipStreamSynchronize(c->stream) != hipSuccess) return s;
    auto none = std::make_shared<CellGridData>();
    none->cap2 = cap2;
    none->info.build_status = s;
    t.grid = none;
    g_last_error.clear();
    return GICP_OK;
  }
  t.grid = g;
  return GICP_OK;
}

extern "C" {

gicp_status gicp_set_target_grid(gicp_ctx* c, int mode) {
  if (!c) return fail(GICP_EINVAL, "null ctx");
  if (mode < GICP_GRID_OFF || mode > GICP_GRID_ON) return fail(GICP_EINVAL, "grid mode must be 0 (off), 1 (auto) or 2 (on)");
  c->grid_mode = mode;
  return GICP_OK;
}

gicp_status gicp_get_target_grid_info(gicp_ctx* c, gicp_grid_info* out) {
  if (!c || !out) return fail(GICP_EINVAL, "null argument");
  std::memset(out, 0, sizeof(*out));
  if (!c->tgt.cloud || !c->tgt.cloud->grid) return GICP_OK;
  *out = c->tgt.cloud->grid->info;
  out->built = grid_active(c) ? 1 : 0;
  return GICP_OK;
}

}  // extern "C"
