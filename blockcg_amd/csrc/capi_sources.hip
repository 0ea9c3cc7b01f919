// include/blockcg_hip.h: what goes into a solve and what comes out of it without passing through host memory -- noise fields
// (bcg_field_fill_noise), point and wall sources (bcg_field_set_point_sources, bcg_field_set_wall_sources) and the inner
// product per slice and column (bcg_field_slice_dot); and the per-slice Gram matrices with momentum projection
// (bcg_field_slice_gram).  Kernels: kernels_sources.hip, kernels_slice_gram.hip.
#include "capi_slice.hpp"
#include "kernels_slice_gram.hpp"
#include "kernels_sources.hpp"

namespace bcg_impl {
namespace {

bool colours_ok(const int* colour, int m) {
  for (int j = 0; j < m; ++j)
    if (colour[j] < 0 || colour[j] > 2) return false;
  return true;
}

}  // namespace
}  // namespace bcg_impl

using namespace bcg_impl;

extern "C" {

int bcg_field_fill_noise(bcg_field* f, int kind, uint64_t seed) {
  DeviceScope on_device(f ? f->ctx : nullptr);
  if (!f) return BCG_ERR_INVALID;
  bcg_context* c = f->ctx;
  if (kind != BCG_NOISE_GAUSSIAN && kind != BCG_NOISE_Z2 && kind != BCG_NOISE_Z4)
    BCG_FAIL(c, BCG_ERR_INVALID, "bcg_field_fill_noise: unknown kind of noise");
  {
    ProfScope ps(c, "fill_noise", row_bytes(f, 1));
    bcg::launch_fill_noise(c->stream, f->m, c->lat, c->gdims, f->parity, f->d, kind, seed);
  }
  return check_launch(c, "fill_noise");
}

int bcg_field_set_point_sources(bcg_field* f, const int* coords, const int* colour) {
  DeviceScope on_device(f ? f->ctx : nullptr);
  if (!f || !coords || !colour) return BCG_ERR_INVALID;
  bcg_context* c = f->ctx;
  const bcg::LatticeDev& lat = c->lat;
  if (!colours_ok(colour, f->m)) BCG_FAIL(c, BCG_ERR_INVALID, "bcg_field_set_point_sources: colour outside 0..2");
  bcg::PointOffsets p{};
  for (int j = 0; j < f->m; ++j) {
    const int* x = coords + 4 * j;
    int par = 0;
    bool mine = true;
    for (int mu = 0; mu < 4; ++mu) {
      if (x[mu] < 0 || x[mu] >= c->gdims[mu])  // gdims is 1 beyond ndim: those entries must be 0
        BCG_FAIL(c, BCG_ERR_INVALID, "bcg_field_set_point_sources: coordinate outside the global lattice");
      par += x[mu];
      mine = mine && x[mu] >= lat.origin[mu] && x[mu] < lat.origin[mu] + lat.L[mu];
    }
    if (f->parity >= 0 && (par & 1) != f->parity)
      BCG_FAIL(c, BCG_ERR_INVALID, "bcg_field_set_point_sources: site of the other parity on a half field");
    p.offset[j] = -1;
    if (mine) {
      const int l0 = f->parity >= 0 ? lat.L[0] / 2 : lat.L[0];
      const int x0 = x[0] - lat.origin[0];
      int64_t site = f->parity >= 0 ? x0 / 2 : x0;
      site += static_cast<int64_t>(l0) *
              ((x[1] - lat.origin[1]) + static_cast<int64_t>(lat.L[1]) * ((x[2] - lat.origin[2]) + static_cast<int64_t>(lat.L[2]) * (x[3] - lat.origin[3])));
      p.offset[j] = (site * 3 + colour[j]) * f->m + j;
    }
  }
  {
    ProfScope ps(c, "set_sources", row_bytes(f, 1));
    HIP_TRY(c, hipMemsetAsync(f->d, 0, field_bytes(f), c->stream));
    bcg::launch_set_points(c->stream, f->m, p, f->d);
  }
  return check_launch(c, "set_points");
}

int bcg_field_set_wall_sources(bcg_field* f, int dir, const int* slice, const int* colour, int site_parity) {
  DeviceScope on_device(f ? f->ctx : nullptr);
  if (!f || !slice || !colour) return BCG_ERR_INVALID;
  bcg_context* c = f->ctx;
  BCG_TRY(check_slice_dir(c, "bcg_field_set_wall_sources", dir));
  if (!colours_ok(colour, f->m)) BCG_FAIL(c, BCG_ERR_INVALID, "bcg_field_set_wall_sources: colour outside 0..2");
  if (site_parity < -1 || site_parity > 1 || (f->parity >= 0 && site_parity >= 0 && site_parity != f->parity))
    BCG_FAIL(c, BCG_ERR_INVALID, "bcg_field_set_wall_sources: site_parity must be -1, 0 or 1, and a half field's own");
  bcg::WallColumns w{};
  for (int j = 0; j < f->m; ++j) {
    if (slice[j] < 0 || slice[j] >= c->gdims[dir])
      BCG_FAIL(c, BCG_ERR_INVALID, "bcg_field_set_wall_sources: slice outside the global lattice");
    w.slice[j] = slice[j];
    w.colour[j] = colour[j];
  }
  {
    ProfScope ps(c, "set_sources", row_bytes(f, 1));
    bcg::launch_set_walls(c->stream, f->m, c->lat, f->parity, f->d, dir, w, site_parity);
  }
  return check_launch(c, "set_walls");
}

int bcg_field_slice_dot(const bcg_field* a, const bcg_field* b, int dir, double* out) {
  DeviceScope on_device(a ? a->ctx : nullptr);
  if (!same_shape(a, b) || !out) return BCG_ERR_INVALID;
  bcg_context* c = a->ctx;
  BCG_TRY(check_slice_dir(c, "bcg_field_slice_dot", dir));
  const int m = a->m;
  const int64_t n_out = static_cast<int64_t>(c->gdims[dir]) * m;
  if (n_out > kSliceHalf) BCG_FAIL(c, BCG_ERR_UNSUPPORTED, "bcg_field_slice_dot: too many slices for the context's scratch");
  BCG_TRY(ensure_scratch(c));
  double2* reduced = c->partials + kSliceHalf;
  int nbps;
  {
    ProfScope ps(c, "slice_dot", row_bytes(a, a == b ? 1 : 2));
    nbps = bcg::launch_slice_dot(c->stream, m, c->lat, a->parity, dir, a->d, b->d, c->partials, kSliceHalf);
  }
  if (nbps <= 0) BCG_FAIL(c, BCG_ERR_UNSUPPORTED, "bcg_field_slice_dot: the block partials do not fit the context's scratch");
  BCG_TRY(check_launch(c, "slice_dot"));
  if (c->lat.split[dir])  // the slices of the other ranks: zeros from this one
    HIP_TRY(c, hipMemsetAsync(reduced, 0, static_cast<size_t>(n_out) * sizeof(double2), c->stream));
  {
    ProfScope ps(c, "slice_fold");
    bcg::launch_slice_fold(c->stream, m, c->lat.L[dir], nbps, c->lat.origin[dir], c->partials, reduced);
  }
  BCG_TRY(check_launch(c, "slice_fold"));
  if (c->distributed) {
    if (!c->have_comm || !c->comm.allreduce_sum) BCG_FAIL(c, BCG_ERR_COMM, "lattice is split over ranks but no bcg_comm was set");
    ProfScope ps(c, "allreduce");
    if (c->comm.allreduce_sum(c->comm.user, reduced, static_cast<size_t>(2) * n_out) != 0)
      BCG_FAIL(c, BCG_ERR_COMM, "allreduce_sum callback failed");
  }
  HIP_TRY(c, hipMemcpyAsync(out, reduced, static_cast<size_t>(n_out) * sizeof(double2), hipMemcpyDeviceToHost, c->stream));
  return stream_sync(c);
}

int bcg_field_slice_gram(const bcg_field* a, const bcg_field* b, int dir, int n_mom, const int* momenta, double* out) {
  DeviceScope on_device(a ? a->ctx : nullptr);
  if (!same_shape(a, b) || !out) return BCG_ERR_INVALID;
  bcg_context* c = a->ctx;
  BCG_TRY(check_slice_dir(c, "bcg_field_slice_gram", dir));
  BCG_TRY(check_slice_momenta(c, "bcg_field_slice_gram", dir, n_mom, momenta));
  if (c->distributed && (!c->have_comm || !c->comm.allreduce_sum))
    BCG_FAIL(c, BCG_ERR_COMM, "lattice is split over ranks but no bcg_comm was set");
  const int m = a->m;
  const int Lg = c->gdims[dir];
  const int64_t per = static_cast<int64_t>(Lg) * m * m;  // entries of one momentum
  const bool mfma = fast_rows(c, m);
  bcg::SliceGramPlan plan;
  if (per > kSliceHalf || !bcg::slice_gram_plan(m, mfma, c->lat, a->parity, dir, Lg, n_mom, kSliceHalf, &plan))
    BCG_FAIL(c, BCG_ERR_UNSUPPORTED, "bcg_field_slice_gram: one momentum's slices do not fit the context's scratch");
  BCG_TRY(ensure_scratch(c));
  // c->partials: [phase tables][block partials] in the first half, the reduced [pc][L_dir global][m^2] in the second
  const int64_t tab_entries = bcg::slice_gram_table_entries(plan);
  double2* const tab_dev = c->partials;
  double2* const partials = c->partials + tab_entries;
  double2* const reduced = c->partials + kSliceHalf;
  const int P = n_mom > 0 ? n_mom : 1;
  // the tables of every momentum, and those of a launch's unused momenta
  const int64_t per_tab = static_cast<int64_t>(3) * plan.walk.ltab;
  std::vector<double2> tabs(n_mom > 0 ? static_cast<size_t>(per_tab) * (P + plan.pc) : 0);
  if (n_mom > 0) slice_phase_tables(c, plan.walk, momenta, P, plan.pc, false, tabs.data());
  for (int p0 = 0; p0 < P; p0 += plan.pc) {
    const int n = std::min(plan.pc, P - p0);
    const int pc = bcg::slice_launch_pc(n);
    if (n_mom > 0) BCG_TRY(upload_slice_tables(c, tab_dev, tabs, per_tab, p0, pc));
    {
      ProfScope ps(c, "slice_gram", row_bytes(a, a == b ? 1 : 2), product_flops(a, pc));
      bcg::launch_slice_gram(c->stream, m, mfma, c->lat, a->parity, dir, plan, pc, a->d, b->d, n_mom > 0 ? tab_dev : nullptr, partials);
    }
    BCG_TRY(check_launch(c, "slice_gram"));
    const size_t n_red = static_cast<size_t>(n) * per;
    if (c->lat.split[dir])  // the slices of the other ranks: zeros from this one
      HIP_TRY(c, hipMemsetAsync(reduced, 0, n_red * sizeof(double2), c->stream));
    {
      ProfScope ps(c, "slice_gram_fold");
      bcg::launch_slice_gram_fold(c->stream, m, pc, n, c->lat.L[dir], Lg, plan.walk.nbps, c->lat.origin[dir], partials, reduced);
    }
    BCG_TRY(check_launch(c, "slice_gram_fold"));
    if (c->distributed) {
      ProfScope ps(c, "allreduce");
      if (c->comm.allreduce_sum(c->comm.user, reduced, 2 * n_red) != 0) BCG_FAIL(c, BCG_ERR_COMM, "allreduce_sum callback failed");
    }
    HIP_TRY(c, hipMemcpyAsync(out + 2 * static_cast<size_t>(p0) * per, reduced, n_red * sizeof(double2), hipMemcpyDeviceToHost,
                              c->stream));
  }
  return stream_sync(c);
}

}  // extern "C"
