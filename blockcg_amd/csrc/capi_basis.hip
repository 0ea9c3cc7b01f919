// include/blockcg_hip.h: products between fields of unequal width -- C = V^dagger b (bcg_basis_dot) and y <- beta y + V C
// (bcg_basis_axpy) for a list V of fields whose widths sum to K != m -- and the column copy between widths
// (bcg_field_copy_columns).  Kernels: kernels_basis.hip.  The host walks V in groups of consecutive fields (one launch per
// group, kernels_basis.hpp); the K x m matrix lives in c->dev_basis / c->pin_basis, which grow on demand.  And the dot
// resolved by slice and momentum (bcg_basis_slice_dot; kernels: kernels_basis_slice.hip, plan: slice_plan.hpp), whose
// P x L_dir x K x m result is assembled in the same buffer, and its adjoint, the update by slice (bcg_basis_slice_axpy;
// kernels: kernels_basis_slice_axpy.hip, plan: slice_plan.hpp), whose matrices, phase table and slice lists are uploaded there.
// And the baryon elementals of three lists (bcg_basis_slice_triple; kernels: kernels_basis_slice_triple.hip, plan:
// slice_plan.hpp), whose P x S x K_c x K_b x K_a result is assembled in c->dev_basis from block partials in c->dev_triple.
#include "capi_slice.hpp"
#include "kernels_basis.hpp"
#include "kernels_basis_slice.hpp"
#include "kernels_basis_slice_axpy.hpp"
#include "kernels_basis_slice_triple.hpp"

namespace bcg_impl {
namespace {

// bcg_basis_slice_dot: the phase tables and the block partials take the first half of c->partials (kSliceHalf), as in
// bcg_field_slice_gram; the whole result, P x L_dir x K x m, is at most 2^26 entries (1 GiB) of c->dev_basis
constexpr int64_t kBasisSliceEntries = static_cast<int64_t>(1) << 26;

struct BasisGroup {
  bool mfma;
  int first, count;  // fields V[first .. first + count - 1]
  int K, off;        // its columns off .. off + K - 1 of the basis
};

// V[0 .. nv-1] against a field `like`: one context, parity and site count; returns K, or -1
int64_t basis_columns(const bcg_field* const* V, int nv, const bcg_field* like) {
  if (!V || nv < 1 || !like) return -1;
  int64_t K = 0;
  for (int k = 0; k < nv; ++k) {
    const bcg_field* v = V[k];
    if (!v || v->ctx != like->ctx || v->parity != like->parity || v->sites != like->sites) return -1;
    K += v->m;
  }
  return K;
}

// Consecutive fields of one class (MFMA: m and the width in {16, 32}) up to the form's bound (mfma_blocks blocks of 16
// columns in the MFMA form); max_cols: a further bound on the columns of a group (the dot's block partials must fit
// c->partials: the group shrinks, not the grid)
std::vector<BasisGroup> basis_groups(const bcg_context* c, const bcg_field* const* V, int nv, int m, int mfma_blocks, int max_cols) {
  std::vector<BasisGroup> out;
  const bool fast = !c->force_generic && (m == 16 || m == 32);
  int off = 0;
  for (int k = 0; k < nv;) {
    BasisGroup g{fast && bcg::basis_mfma_width(V[k]->m), k, 0, 0, off};
    const int cols = std::min(max_cols, g.mfma ? 16 * mfma_blocks : bcg::kBasisGenericCols);
    const int fields = g.mfma ? mfma_blocks : bcg::kBasisGenericFields;
    while (k < nv && g.count < fields && (fast && bcg::basis_mfma_width(V[k]->m)) == g.mfma &&
           (g.count == 0 || g.K + V[k]->m <= cols)) {
      g.K += V[k]->m;
      g.count += 1;
      k += 1;
    }
    off += g.K;
    out.push_back(g);
  }
  return out;
}

bcg::BasisBlocks group_blocks(const bcg_field* const* V, const BasisGroup& g, int* nblocks16) {
  bcg::BasisBlocks b{};
  int n = 0;
  for (int k = g.first; k < g.first + g.count; ++k)
    for (int c0 = 0; c0 < V[k]->m; c0 += 16) {
      b.p[n] = V[k]->d + c0;
      b.ld[n] = V[k]->m;
      n += 1;
    }
  *nblocks16 = n;
  return b;
}

bcg::BasisFields group_fields(const bcg_field* const* V, const BasisGroup& g) {
  bcg::BasisFields f{};
  f.nv = g.count;
  f.K = g.K;
  int off = 0;
  for (int k = 0; k < g.count; ++k) {
    f.v[k] = V[g.first + k]->d;
    f.w[k] = V[g.first + k]->m;
    f.off[k] = off;
    off += f.w[k];
  }
  return f;
}

void release_basis(bcg_context* c) {
  if (c->dev_basis) (void)hipFree(c->dev_basis);
  if (c->pin_basis) (void)hipHostFree(c->pin_basis);
  c->dev_basis = nullptr;
  c->pin_basis = nullptr;
  c->basis_entries = 0;
}

int ensure_basis(bcg_context* c, size_t entries) {
  if (!c->basis_uploaded) HIP_TRY(c, hipEventCreateWithFlags(&c->basis_uploaded, hipEventDisableTiming));
  if (entries <= c->basis_entries) return BCG_OK;
  BCG_TRY(stream_sync(c));  // a kernel of an earlier call may still read the old buffer
  release_basis(c);
  HIP_TRY(c, hipMalloc(&c->dev_basis, entries * sizeof(double2)));
  HIP_TRY(c, hipHostMalloc(reinterpret_cast<void**>(&c->pin_basis), entries * sizeof(double2), hipHostMallocDefault));
  c->basis_entries = entries;
  return BCG_OK;
}

// the result assembled in c->dev_basis: summed over ranks, then to `out` through c->pin_basis
int download_basis(bcg_context* c, size_t entries, double* out) {
  if (c->distributed) {
    ProfScope ps(c, "allreduce");
    if (c->comm.allreduce_sum(c->comm.user, c->dev_basis, 2 * entries) != 0) BCG_FAIL(c, BCG_ERR_COMM, "allreduce_sum callback failed");
  }
  HIP_TRY(c, hipEventSynchronize(c->basis_uploaded));  // an upload of bcg_basis_axpy may still read pin_basis
  HIP_TRY(c, hipMemcpyAsync(c->pin_basis, c->dev_basis, entries * sizeof(double2), hipMemcpyDeviceToHost, c->stream));
  BCG_TRY(stream_sync(c));
  std::memcpy(out, c->pin_basis, entries * sizeof(double2));
  return BCG_OK;
}

}  // namespace
}  // namespace bcg_impl

using namespace bcg_impl;

extern "C" {

int bcg_basis_dot(const bcg_field* const* V, int nv, const bcg_field* b, double* out) {
  DeviceScope on_device(b ? b->ctx : nullptr);
  const int64_t K = basis_columns(V, nv, b);
  if (K < 0 || !out) return BCG_ERR_INVALID;
  bcg_context* c = b->ctx;
  if (c->distributed && (!c->have_comm || !c->comm.allreduce_sum))
    BCG_FAIL(c, BCG_ERR_COMM, "lattice is split over ranks but no bcg_comm was set");
  const int m = b->m;
  const size_t entries = static_cast<size_t>(K) * m;
  if (entries > (static_cast<size_t>(1) << 30)) BCG_FAIL(c, BCG_ERR_UNSUPPORTED, "bcg_basis_dot: more than 2^30 entries");
  int rc = ensure_scratch(c);
  if (rc == BCG_OK) rc = ensure_basis(c, entries);
  rc = agree_on_allocation(c, rc, "bcg_basis_dot", "the K x m result");
  if (rc != BCG_OK) {
    if (c->distributed) release_basis(c);  // every rank starts the next call from the same state
    return rc;
  }
  const int64_t room = static_cast<int64_t>(c->partials_bytes / sizeof(double2)) / (static_cast<int64_t>(bcg::kBasisBlocks) * m);
  if (room < 32) BCG_FAIL(c, BCG_ERR_UNSUPPORTED, "bcg_basis_dot: the block partials do not fit the context's scratch");
  for (const BasisGroup& g : basis_groups(c, V, nv, m, bcg::basis_dot_mfma_blocks(m), static_cast<int>(std::min<int64_t>(room, 1 << 20)))) {
    int nblocks;
    {
      ProfScope ps(c, "basis_dot", static_cast<double>(b->sites) * 48.0 * (g.K + m), static_cast<double>(rows_of(b)) * 8.0 * g.K * m);
      ProfScope form(c, g.mfma ? "basis_form_mfma" : "basis_form_generic");
      if (g.mfma) {
        int n16;
        const bcg::BasisBlocks blocks = group_blocks(V, g, &n16);
        nblocks = bcg::launch_basis_dot_mfma(c->stream, m, n16, rows_of(b), blocks, b->d, c->partials);
      } else {
        nblocks = bcg::launch_basis_dot_generic(c->stream, m, rows_of(b), group_fields(V, g), b->d, c->partials);
      }
    }
    BCG_TRY(check_launch(c, "basis_dot"));
    {
      ProfScope ps(c, "basis_fold");
      bcg::launch_basis_fold(c->stream, g.K, m, nblocks, c->partials, c->dev_basis, static_cast<int>(K), g.off);
    }
    BCG_TRY(check_launch(c, "basis_fold"));
  }
  return download_basis(c, entries, out);
}

int bcg_basis_slice_dot(const bcg_field* const* V, int nv, const bcg_field* b, int dir, int n_mom, const int* momenta, double* out) {
  DeviceScope on_device(b ? b->ctx : nullptr);
  const int64_t K = basis_columns(V, nv, b);
  if (K < 0 || !out) return BCG_ERR_INVALID;
  bcg_context* c = b->ctx;
  BCG_TRY(check_slice_dir(c, "bcg_basis_slice_dot", dir));
  BCG_TRY(check_slice_momenta(c, "bcg_basis_slice_dot", dir, n_mom, momenta));
  if (c->distributed && (!c->have_comm || !c->comm.allreduce_sum))
    BCG_FAIL(c, BCG_ERR_COMM, "lattice is split over ranks but no bcg_comm was set");
  const int m = b->m;
  const int P = n_mom > 0 ? n_mom : 1;
  const int Lg = c->gdims[dir], Ll = c->lat.L[dir];
  const int64_t per = static_cast<int64_t>(Lg) * K * m;  // entries of one momentum
  if (per > kBasisSliceEntries / P) BCG_FAIL(c, BCG_ERR_UNSUPPORTED, "bcg_basis_slice_dot: more than 2^26 entries; split the momenta");
  const size_t entries = static_cast<size_t>(per) * P;
  std::vector<int> widths(nv);
  for (int k = 0; k < nv; ++k) widths[k] = V[k]->m;
  bcg::BasisSlicePlan plan;
  if (!bcg::basis_slice_plan(widths.data(), nv, m, !c->force_generic, c->lat, b->parity, dir, n_mom, kSliceHalf, &plan))
    BCG_FAIL(c, BCG_ERR_UNSUPPORTED, "bcg_basis_slice_dot: one launch does not fit the context's scratch");
  int rc = ensure_scratch(c);
  if (rc == BCG_OK) rc = ensure_basis(c, entries);
  rc = agree_on_allocation(c, rc, "bcg_basis_slice_dot", "the P x L_dir x K x m result");
  if (rc != BCG_OK) {
    if (c->distributed) release_basis(c);  // every rank starts the next call from the same state
    return rc;
  }
  // c->partials, first half: [phase tables][block partials]; the result is assembled in c->dev_basis
  double2* const tab_dev = c->partials;
  double2* const partials = c->partials + (n_mom > 0 ? bcg::basis_slice_table_entries(plan) : 0);
  // the tables of every momentum, and those of a launch's unused momenta
  const int64_t per_tab = static_cast<int64_t>(3) * plan.walk.ltab;
  std::vector<double2> tabs(n_mom > 0 ? static_cast<size_t>(per_tab) * (P + plan.pc_max()) : 0);
  if (n_mom > 0) slice_phase_tables(c, plan.walk, momenta, P, plan.pc_max(), false, tabs.data());
  if (c->lat.split[dir])  // the slices of the other ranks: zeros from this one
    HIP_TRY(c, hipMemsetAsync(c->dev_basis, 0, entries * sizeof(double2), c->stream));
  // the 16-column blocks of the MFMA fields of V, in order: an MFMA group is a run of them
  std::vector<const double2*> block_p;
  std::vector<int> block_ld;
  for (int k = 0; k < nv; ++k)
    if (!c->force_generic && (m == 16 || m == 32) && bcg::basis_mfma_width(V[k]->m))
      for (int c0 = 0; c0 < V[k]->m; c0 += 16) {
        block_p.push_back(V[k]->d + c0);
        block_ld.push_back(V[k]->m);
      }
  for (const bcg::BasisSliceGroup& g : plan.groups) {
    const int pc_g = plan.pc_of(g);
    bcg::BasisBlocks blocks{};
    bcg::BasisFields fields{};
    if (g.mfma) {
      for (int q = 0; q < g.count; ++q) {
        blocks.p[q] = block_p[g.first + q];
        blocks.ld[q] = block_ld[g.first + q];
      }
    } else {
      BasisGroup fg{false, g.first, g.count, g.K, g.off};
      fields = group_fields(V, fg);
    }
    for (int p0 = 0; p0 < P; p0 += pc_g) {
      const int n = std::min(pc_g, P - p0);
      const int pc = bcg::slice_launch_pc(n);
      if (n_mom > 0) BCG_TRY(upload_slice_tables(c, tab_dev, tabs, per_tab, p0, pc));
      {
        ProfScope ps(c, "basis_slice_dot", static_cast<double>(b->sites) * 48.0 * (g.K + m), static_cast<double>(rows_of(b)) * 8.0 * g.K * m * pc);
        ProfScope form(c, g.mfma ? "basis_slice_form_mfma" : "basis_slice_form_generic");
        if (g.mfma)
          bcg::launch_basis_slice_dot_mfma(c->stream, m, g.count, c->lat, b->parity, dir, plan, pc, blocks, b->d, n_mom > 0 ? tab_dev : nullptr,
                                           partials);
        else
          bcg::launch_basis_slice_dot_generic(c->stream, m, c->lat, b->parity, dir, plan, pc, fields, b->d, n_mom > 0 ? tab_dev : nullptr,
                                              partials);
      }
      BCG_TRY(check_launch(c, "basis_slice_dot"));
      {
        ProfScope ps(c, "basis_slice_fold");
        bcg::launch_basis_slice_fold(c->stream, g.K, m, pc, n, Ll, Lg, plan.walk.nbps, c->lat.origin[dir], static_cast<int>(K), g.off, p0, partials,
                                     c->dev_basis);
      }
      BCG_TRY(check_launch(c, "basis_slice_fold"));
    }
  }
  return download_basis(c, entries, out);
}

int bcg_basis_axpy(bcg_field* y, const bcg_field* const* V, int nv, const double* C, double beta) {
  DeviceScope on_device(y ? y->ctx : nullptr);
  const int64_t K = basis_columns(V, nv, y);
  if (K < 0 || !C) return BCG_ERR_INVALID;
  bcg_context* c = y->ctx;
  for (int k = 0; k < nv; ++k)
    if (V[k] == y) BCG_FAIL(c, BCG_ERR_INVALID, "bcg_basis_axpy: y is one of the basis fields");
  if (!std::isfinite(beta)) BCG_FAIL(c, BCG_ERR_INVALID, "bcg_basis_axpy: beta is not finite");
  const int m = y->m;
  const size_t entries = static_cast<size_t>(K) * m;
  if (entries > (static_cast<size_t>(1) << 30)) BCG_FAIL(c, BCG_ERR_UNSUPPORTED, "bcg_basis_axpy: more than 2^30 entries");
  BCG_TRY(ensure_basis(c, entries));
  HIP_TRY(c, hipEventSynchronize(c->basis_uploaded));  // the previous upload has left pin_basis
  std::memcpy(c->pin_basis, C, entries * sizeof(double2));
  HIP_TRY(c, hipMemcpyAsync(c->dev_basis, c->pin_basis, entries * sizeof(double2), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipEventRecord(c->basis_uploaded, c->stream));
  bool first = true;
  for (const BasisGroup& g : basis_groups(c, V, nv, m, bcg::basis_axpy_mfma_blocks(m), 1 << 20)) {
    const double bg = first ? beta : 1.0;
    {
      ProfScope ps(c, "basis_axpy", static_cast<double>(y->sites) * 48.0 * (g.K + (bg == 0.0 ? m : 2 * m)),
                   static_cast<double>(rows_of(y)) * 8.0 * g.K * m);
      ProfScope form(c, g.mfma ? "basis_form_mfma" : "basis_form_generic");
      if (g.mfma) {
        int n16;
        const bcg::BasisBlocks blocks = group_blocks(V, g, &n16);
        bcg::launch_basis_axpy_mfma(c->stream, m, n16, rows_of(y), y->d, blocks, c->dev_basis, static_cast<int>(K), g.off, bg);
      } else {
        bcg::launch_basis_axpy_generic(c->stream, m, rows_of(y), y->d, group_fields(V, g), c->dev_basis, static_cast<int>(K), g.off, bg);
      }
    }
    BCG_TRY(check_launch(c, "basis_axpy"));
    first = false;
  }
  return BCG_OK;
}

int bcg_basis_slice_axpy(bcg_field* y, const bcg_field* const* V, int nv, int dir, int n_slices, const int* slices, const double* C,
                         const int* momentum, double beta) {
  DeviceScope on_device(y ? y->ctx : nullptr);
  const int64_t K = basis_columns(V, nv, y);
  if (K < 0 || !C) return BCG_ERR_INVALID;
  bcg_context* c = y->ctx;
  for (int k = 0; k < nv; ++k)
    if (V[k] == y) BCG_FAIL(c, BCG_ERR_INVALID, "bcg_basis_slice_axpy: y is one of the basis fields");
  if (!std::isfinite(beta)) BCG_FAIL(c, BCG_ERR_INVALID, "bcg_basis_slice_axpy: beta is not finite");
  BCG_TRY(check_slice_dir(c, "bcg_basis_slice_axpy", dir));
  if (n_slices < 0 || (n_slices > 0 && !slices)) BCG_FAIL(c, BCG_ERR_INVALID, "bcg_basis_slice_axpy: n_slices slices are needed");
  const int Lg = c->gdims[dir], Ll = c->lat.L[dir], origin = c->lat.origin[dir];
  const int S = n_slices > 0 ? n_slices : Lg;
  // local slice -> index of its matrix in C, or -1: not listed
  std::vector<int> index_of(Ll, -1);
  {
    std::vector<char> seen(Lg, 0);
    for (int s = 0; s < S; ++s) {
      const int t = n_slices > 0 ? slices[s] : s;
      if (t < 0 || t >= Lg) BCG_FAIL(c, BCG_ERR_INVALID, "bcg_basis_slice_axpy: slice outside the lattice");
      if (seen[t]) BCG_FAIL(c, BCG_ERR_INVALID, "bcg_basis_slice_axpy: a slice is listed twice");
      seen[t] = 1;
      if (t >= origin && t < origin + Ll) index_of[t - origin] = s;
    }
  }
  BCG_TRY(check_slice_momenta(c, "bcg_basis_slice_axpy", dir, momentum ? 1 : 0, momentum));
  const int m = y->m;
  if (static_cast<int64_t>(K) * m > kBasisSliceEntries / S) BCG_FAIL(c, BCG_ERR_UNSUPPORTED, "bcg_basis_slice_axpy: more than 2^26 entries");
  const size_t entries = static_cast<size_t>(S) * K * m;
  // the launches' lists: (local slice, index in C) of the listed slices in ascending local slice, then the other slices
  std::vector<int> lists;
  for (int t = 0; t < Ll; ++t)
    if (index_of[t] >= 0) {
      lists.push_back(t);
      lists.push_back(index_of[t]);
    }
  const int nl = static_cast<int>(lists.size() / 2);
  for (int t = 0; t < Ll; ++t)
    if (index_of[t] < 0) lists.push_back(t);
  const int nu = Ll - nl;
  const bool rest = nu > 0 && beta != 1.0;
  if (nl == 0 && !rest) return BCG_OK;  // none of the listed slices is here and the others keep their bits
  bcg::SliceWalk plan{}, plan_rest{};
  if ((nl > 0 && !bcg::basis_slice_axpy_plan(c->lat, y->parity, dir, nl, &plan)) ||
      (rest && !bcg::basis_slice_axpy_plan(c->lat, y->parity, dir, nu, &plan_rest)))
    BCG_FAIL(c, BCG_ERR_UNSUPPORTED, "bcg_basis_slice_axpy: a slice of 2^30 rows or more");
  // c->dev_basis: [C][the phase table, 3 x ltab][the lists]
  const size_t tab_entries = momentum && nl > 0 ? static_cast<size_t>(3) * plan.ltab : 0;
  const size_t list_entries = (lists.size() * sizeof(int) + sizeof(double2) - 1) / sizeof(double2);
  const size_t all = entries + tab_entries + list_entries;
  BCG_TRY(ensure_basis(c, all));
  HIP_TRY(c, hipEventSynchronize(c->basis_uploaded));  // the previous upload has left pin_basis
  std::memcpy(c->pin_basis, C, entries * sizeof(double2));
  if (tab_entries)  // w = conj(w_p)
    slice_phase_tables(c, plan, momentum, 1, 0, true, reinterpret_cast<double2*>(c->pin_basis) + entries);
  std::memcpy(reinterpret_cast<double2*>(c->pin_basis) + entries + tab_entries, lists.data(), lists.size() * sizeof(int));
  HIP_TRY(c, hipMemcpyAsync(c->dev_basis, c->pin_basis, all * sizeof(double2), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipEventRecord(c->basis_uploaded, c->stream));
  const double2* const tab_dev = tab_entries ? c->dev_basis + entries : nullptr;
  const int* const list_dev = reinterpret_cast<const int*>(c->dev_basis + entries + tab_entries);
  if (rest) {
    {
      ProfScope ps(c, "basis_slice_scale", static_cast<double>(y->sites) / Ll * nu * 48.0 * (beta == 0.0 ? m : 2 * m));
      bcg::launch_slice_scale(c->stream, m, c->lat, y->parity, dir, plan_rest, nu, list_dev + 2 * nl, y->d, beta);
    }
    BCG_TRY(check_launch(c, "basis_slice_scale"));
  }
  if (nl == 0) return BCG_OK;
  const double sites = static_cast<double>(y->sites) / Ll * nl;  // of the listed slices
  bool first = true;
  for (const BasisGroup& g : basis_groups(c, V, nv, m, bcg::basis_axpy_mfma_blocks(m), 1 << 20)) {
    const double bg = first ? beta : 1.0;
    {
      ProfScope ps(c, "basis_slice_axpy", sites * 48.0 * (g.K + (bg == 0.0 ? m : 2 * m)), sites * 3.0 * 8.0 * g.K * m);
      ProfScope form(c, g.mfma ? "basis_slice_axpy_form_mfma" : "basis_slice_axpy_form_generic");
      if (g.mfma) {
        int n16;
        const bcg::BasisBlocks blocks = group_blocks(V, g, &n16);
        bcg::launch_basis_slice_axpy_mfma(c->stream, m, n16, c->lat, y->parity, dir, plan, nl, list_dev, y->d, blocks, c->dev_basis,
                                          static_cast<int>(K), g.off, tab_dev, bg);
      } else {
        bcg::launch_basis_slice_axpy_generic(c->stream, m, c->lat, y->parity, dir, plan, nl, list_dev, y->d, group_fields(V, g),
                                             c->dev_basis, static_cast<int>(K), g.off, tab_dev, bg);
      }
    }
    BCG_TRY(check_launch(c, "basis_slice_axpy"));
    first = false;
  }
  return BCG_OK;
}

int bcg_basis_slice_triple(const bcg_field* const* A, int na, const bcg_field* const* B, int nb, const bcg_field* const* C, int nc, int dir,
                           int n_slices, const int* slices, int n_mom, const int* momenta, double* out) {
  const char* const who = "bcg_basis_slice_triple";
  const bcg_field* like = A && na >= 1 ? A[0] : nullptr;
  DeviceScope on_device(like ? like->ctx : nullptr);
  const bcg_field* const* lists[3] = {A, B, C};
  const int counts[3] = {na, nb, nc};
  int64_t K[3];
  for (int l = 0; l < 3; ++l) K[l] = basis_columns(lists[l], counts[l], like);
  if (K[0] < 0 || K[1] < 0 || K[2] < 0 || !out) return BCG_ERR_INVALID;
  bcg_context* c = like->ctx;
  BCG_TRY(check_slice_dir(c, who, dir));
  if (n_slices < 0 || (n_slices > 0 && !slices)) BCG_FAIL(c, BCG_ERR_INVALID, "bcg_basis_slice_triple: n_slices slices are needed");
  const int Lg = c->gdims[dir], Ll = c->lat.L[dir], origin = c->lat.origin[dir];
  const int S = n_slices > 0 ? n_slices : Lg;
  // (local slice, index in the result) of the listed slices that are here, in ascending local slice
  std::vector<int> list;
  {
    std::vector<int> index_of(Ll, -1);
    std::vector<char> seen(Lg, 0);
    for (int s = 0; s < S; ++s) {
      const int t = n_slices > 0 ? slices[s] : s;
      if (t < 0 || t >= Lg) BCG_FAIL(c, BCG_ERR_INVALID, "bcg_basis_slice_triple: slice outside the lattice");
      if (seen[t]) BCG_FAIL(c, BCG_ERR_INVALID, "bcg_basis_slice_triple: a slice is listed twice");
      seen[t] = 1;
      if (t >= origin && t < origin + Ll) index_of[t - origin] = s;
    }
    for (int t = 0; t < Ll; ++t)
      if (index_of[t] >= 0) {
        list.push_back(t);
        list.push_back(index_of[t]);
      }
  }
  const int nl = static_cast<int>(list.size() / 2);
  BCG_TRY(check_slice_momenta(c, who, dir, n_mom, momenta));
  if (c->distributed && (!c->have_comm || !c->comm.allreduce_sum))
    BCG_FAIL(c, BCG_ERR_COMM, "lattice is split over ranks but no bcg_comm was set");
  for (int l = 0; l < 3; ++l)
    if (K[l] > bcg::kTripleMaxColumns) BCG_FAIL(c, BCG_ERR_UNSUPPORTED, "bcg_basis_slice_triple: a list of more than 64 columns");
  const int P = n_mom > 0 ? n_mom : 1;
  const int64_t per = K[0] * K[1] * K[2];  // entries of one slice and momentum
  if (per > kBasisSliceEntries / P / S)
    BCG_FAIL(c, BCG_ERR_UNSUPPORTED, "bcg_basis_slice_triple: more than 2^26 entries; split the slices or the momenta");
  const size_t entries = static_cast<size_t>(per) * P * S;
  bool identical = na == nb && nb == nc;
  for (int k = 0; identical && k < na; ++k) identical = A[k] == B[k] && B[k] == C[k];
  std::vector<int> widths[3];
  for (int l = 0; l < 3; ++l)
    for (int k = 0; k < counts[l]; ++k) widths[l].push_back(lists[l][k]->m);
  // whether a plan exists is decided for the most slices a rank can hold, so that every rank decides alike
  bcg::BasisSliceTriplePlan plan;
  for (const int n : {std::min(S, Ll), nl})
    if (!bcg::basis_slice_triple_plan(widths[0].data(), na, widths[1].data(), nb, widths[2].data(), nc, identical, !c->force_generic, c->lat,
                                      like->parity, dir, n, n_mom, &plan))
      BCG_FAIL(c, BCG_ERR_UNSUPPORTED,
               "bcg_basis_slice_triple: a slice of 2^30 rows or more, or too many listed slices for one block each; split the slices");
  // c->dev_triple: [column table][tiles][slice list][phase tables of every momentum][block partials]
  const auto in_entries = [](size_t bytes) { return (bytes + sizeof(double2) - 1) / sizeof(double2); };
  const size_t col_entries = in_entries(3 * bcg::kTripleMaxColumns * sizeof(bcg::TripleCol));
  const size_t tile_entries = in_entries(plan.tiles.size() * sizeof(int));
  const size_t list_entries = in_entries(list.size() * sizeof(int));
  const size_t per_tab = static_cast<size_t>(3) * plan.walk.ltab;
  const size_t tab_entries = n_mom > 0 ? per_tab * P : 0;
  const size_t head = col_entries + tile_entries + list_entries + tab_entries;
  const size_t need = head + static_cast<size_t>(plan.partial_entries(nl));
  int rc = ensure_basis(c, entries);
  if (rc == BCG_OK && need > c->triple_entries) {
    rc = stream_sync(c);
    if (rc == BCG_OK) {
      if (c->dev_triple) (void)hipFree(c->dev_triple);
      c->dev_triple = nullptr;
      c->triple_entries = 0;
      if (hipMalloc(&c->dev_triple, need * sizeof(double2)) == hipSuccess) {
        c->triple_entries = need;
      } else {
        c->dev_triple = nullptr;
        c->err = "bcg_basis_slice_triple: hipMalloc of the block partials failed";
        rc = BCG_ERR_HIP;
      }
    }
  }
  rc = agree_on_allocation(c, rc, who, "the result and the block partials");
  if (rc != BCG_OK) {
    if (c->distributed) release_basis(c);  // every rank starts the next call from the same state
    return rc;
  }
  std::vector<double2> host(head, make_double2(0.0, 0.0));
  {
    bcg::TripleCol* cols = reinterpret_cast<bcg::TripleCol*>(host.data());
    for (int l = 0; l < 3; ++l) {
      int col = 0;
      for (int k = 0; k < counts[l]; ++k)
        for (int j = 0; j < lists[l][k]->m; ++j) cols[l * bcg::kTripleMaxColumns + col++] = bcg::TripleCol{lists[l][k]->d + j, lists[l][k]->m};
    }
    std::memcpy(host.data() + col_entries, plan.tiles.data(), plan.tiles.size() * sizeof(int));
    if (nl > 0) std::memcpy(host.data() + col_entries + tile_entries, list.data(), list.size() * sizeof(int));
    if (n_mom > 0) slice_phase_tables(c, plan.walk, momenta, P, 0, false, host.data() + col_entries + tile_entries + list_entries);
  }
  // the slices of other ranks, the slices nobody lists twice over and the entries the fold does not write: zeros
  HIP_TRY(c, hipMemsetAsync(c->dev_basis, 0, entries * sizeof(double2), c->stream));
  if (nl > 0) {
    HIP_TRY(c, hipMemcpyAsync(c->dev_triple, host.data(), head * sizeof(double2), hipMemcpyHostToDevice, c->stream));
    const bcg::TripleCol* const cols_dev = reinterpret_cast<const bcg::TripleCol*>(c->dev_triple);
    const int* const tiles_dev = reinterpret_cast<const int*>(c->dev_triple + col_entries);
    const int* const list_dev = reinterpret_cast<const int*>(c->dev_triple + col_entries + tile_entries);
    const double2* const tabs_dev = c->dev_triple + col_entries + tile_entries + list_entries;
    double2* const partials = c->dev_triple + head;
    const double work = static_cast<double>(like->sites) / Ll * nl * plan.n_tiles();  // sites x tiles of a launch
    for (int p = 0; p < P; ++p) {
      {
        ProfScope ps(c, "basis_slice_triple", work * 48.0 * 3.0 * plan.edge, work * 24.0 * static_cast<double>(plan.tile_entries()));
        ProfScope form(c, plan.mfma ? "basis_slice_triple_form_mfma" : "basis_slice_triple_form_generic");
        bcg::launch_basis_slice_triple(c->stream, c->lat, like->parity, dir, plan, nl, cols_dev, static_cast<int>(K[0]), static_cast<int>(K[1]),
                                       static_cast<int>(K[2]), tiles_dev, list_dev, n_mom > 0 ? tabs_dev + p * per_tab : nullptr, partials);
      }
      BCG_TRY(check_launch(c, "basis_slice_triple"));
      {
        ProfScope ps(c, "basis_slice_triple_fold");
        bcg::launch_basis_slice_triple_fold(c->stream, plan, nl, static_cast<int>(K[0]), static_cast<int>(K[1]), static_cast<int>(K[2]), S, p,
                                            tiles_dev, list_dev, partials, c->dev_basis);
      }
      BCG_TRY(check_launch(c, "basis_slice_triple_fold"));
    }
  }
  return download_basis(c, entries, out);
}

int bcg_field_copy_columns(bcg_field* dst, int dst_first, const bcg_field* src, int src_first, int n) {
  DeviceScope on_device(dst ? dst->ctx : nullptr);
  if (!dst || !src || dst == src || dst->ctx != src->ctx || dst->parity != src->parity || dst->sites != src->sites)
    return BCG_ERR_INVALID;
  bcg_context* c = dst->ctx;
  if (n < 1 || dst_first < 0 || src_first < 0 || dst_first > dst->m - n || src_first > src->m - n)
    BCG_FAIL(c, BCG_ERR_INVALID, "bcg_field_copy_columns: column range outside a field");
  {
    ProfScope ps(c, "copy_columns", static_cast<double>(dst->sites) * 48.0 * 2 * n);
    bcg::launch_copy_columns(c->stream, rows_of(dst), dst->d, dst->m, dst_first, src->d, src->m, src_first, n);
  }
  return check_launch(c, "copy_columns");
}

}  // extern "C"
