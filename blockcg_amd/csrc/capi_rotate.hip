// include/blockcg_hip.h: bcg_basis_rotate -- V <- V Q in place for a list V of fields whose widths sum to K <= 64 and a
// K x K matrix Q.  Kernels: kernels_rotate.hip (one launch takes all K columns).  The uploaded Q lives in c->dev_rotate /
// c->pin_rotate (64 x 64 entries, allocated on first use, freed by bcg_context_destroy).  No communication call.
// And bcg_basis_slice_rotate -- V(x) <- V(x) Q_s on the sites of the listed slices, one K x K matrix per slice.  Kernels:
// kernels_basis_slice_rotate.hip on the walk of bcg_basis_slice_axpy (basis_slice_axpy_plan, slice_plan.hpp).  Its matrices
// and its (local slice, matrix index) list go through the same two buffers, grown when a call needs more.
#include "capi_slice.hpp"
#include "kernels_basis.hpp"
#include "kernels_basis_slice_rotate.hpp"
#include "kernels_rotate.hpp"

static_assert(BCG_BASIS_ROTATE_MAX_COLUMNS == bcg::kRotateMaxCols, "the header's constant is the kernels' bound");

namespace bcg_impl {
namespace {

// room for `entries` double2 (64 x 64 at the least) in c->dev_rotate and c->pin_rotate
int ensure_rotate(bcg_context* c, size_t entries) {
  entries = std::max(entries, static_cast<size_t>(bcg::kRotateMaxCols) * bcg::kRotateMaxCols);
  if (!c->rotate_uploaded) HIP_TRY(c, hipEventCreateWithFlags(&c->rotate_uploaded, hipEventDisableTiming));
  if (entries <= c->rotate_entries) return BCG_OK;
  if (c->rotate_entries) BCG_TRY(stream_sync(c));  // a kernel of an earlier call may still read the old buffer
  if (c->dev_rotate) (void)hipFree(c->dev_rotate);
  if (c->pin_rotate) (void)hipHostFree(c->pin_rotate);
  c->dev_rotate = nullptr;
  c->pin_rotate = nullptr;
  c->rotate_entries = 0;
  HIP_TRY(c, hipMalloc(&c->dev_rotate, entries * sizeof(double2)));
  HIP_TRY(c, hipHostMalloc(reinterpret_cast<void**>(&c->pin_rotate), entries * sizeof(double2), hipHostMallocDefault));
  c->rotate_entries = entries;
  return BCG_OK;
}

// V of bcg_basis_rotate: one context, parity and site count, no field twice.  K: the columns; mfma: every width in {16, 32}
int check_rotate_list(const char* who, bcg_field* const* V, int nv, int64_t* K, bool* mfma) {
  const bcg_field* like = V[0];
  bcg_context* c = like->ctx;
  *K = 0;
  *mfma = !c->force_generic;
  for (int k = 0; k < nv; ++k) {
    const bcg_field* v = V[k];
    if (!v || v->ctx != c || v->parity != like->parity || v->sites != like->sites) return BCG_ERR_INVALID;
    for (int l = 0; l < k; ++l)
      if (V[l] == v) BCG_FAIL(c, BCG_ERR_INVALID, std::string(who) + ": a field is listed twice");
    *mfma = *mfma && bcg::basis_mfma_width(v->m);
    *K += v->m;
  }
  if (*K > bcg::kRotateMaxCols) BCG_FAIL(c, BCG_ERR_UNSUPPORTED, std::string(who) + ": more than 64 columns");
  return BCG_OK;
}

bcg::RotateBlocks rotate_blocks(bcg_field* const* V, int nv, int* nblocks16) {
  bcg::RotateBlocks b{};
  int n = 0;
  for (int k = 0; k < nv; ++k)
    for (int c0 = 0; c0 < V[k]->m; c0 += 16) {
      b.p[n] = V[k]->d + c0;
      b.ld[n] = V[k]->m;
      n += 1;
    }
  *nblocks16 = n;
  return b;
}

bcg::RotateFields rotate_fields(bcg_field* const* V, int nv, int K) {
  bcg::RotateFields f{};
  f.nv = nv;
  f.K = K;
  for (int k = 0; k < nv; ++k) {
    f.v[k] = V[k]->d;
    f.w[k] = static_cast<unsigned char>(V[k]->m);
  }
  return f;
}

}  // namespace
}  // namespace bcg_impl

using namespace bcg_impl;

extern "C" {

int bcg_basis_rotate(bcg_field* const* V, int nv, const double* Q) {
  if (!V || nv < 1 || !V[0] || !Q) return BCG_ERR_INVALID;
  const bcg_field* like = V[0];
  DeviceScope on_device(like->ctx);
  bcg_context* c = like->ctx;
  int64_t K;
  bool mfma;
  BCG_TRY(check_rotate_list("bcg_basis_rotate", V, nv, &K, &mfma));
  const size_t entries = static_cast<size_t>(K) * K;
  for (size_t e = 0; e < 2 * entries; ++e)
    if (!std::isfinite(Q[e])) BCG_FAIL(c, BCG_ERR_INVALID, "bcg_basis_rotate: Q is not finite");
  BCG_TRY(ensure_rotate(c, entries));
  HIP_TRY(c, hipEventSynchronize(c->rotate_uploaded));  // the previous upload has left pin_rotate
  std::memcpy(c->pin_rotate, Q, entries * sizeof(double2));
  HIP_TRY(c, hipMemcpyAsync(c->dev_rotate, c->pin_rotate, entries * sizeof(double2), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipEventRecord(c->rotate_uploaded, c->stream));
  {
    ProfScope ps(c, "basis_rotate", static_cast<double>(like->sites) * 96.0 * K, static_cast<double>(rows_of(like)) * 8.0 * K * K);
    ProfScope form(c, mfma ? "basis_rotate_mfma" : "basis_rotate_generic");
    if (mfma) {
      int n;
      const bcg::RotateBlocks b = rotate_blocks(V, nv, &n);
      bcg::launch_basis_rotate_mfma(c->stream, n, rows_of(like), b, c->dev_rotate);
    } else {
      bcg::launch_basis_rotate_generic(c->stream, rows_of(like), rotate_fields(V, nv, static_cast<int>(K)), c->dev_rotate);
    }
  }
  return check_launch(c, "basis_rotate");
}

int bcg_basis_slice_rotate(bcg_field* const* V, int nv, int dir, int n_slices, const int* slices, const double* Q) {
  if (!V || nv < 1 || !V[0] || !Q) return BCG_ERR_INVALID;
  const bcg_field* like = V[0];
  DeviceScope on_device(like->ctx);
  bcg_context* c = like->ctx;
  int64_t K;
  bool mfma;
  BCG_TRY(check_rotate_list("bcg_basis_slice_rotate", V, nv, &K, &mfma));
  BCG_TRY(check_slice_dir(c, "bcg_basis_slice_rotate", dir));
  if (n_slices < 0 || (n_slices > 0 && !slices)) BCG_FAIL(c, BCG_ERR_INVALID, "bcg_basis_slice_rotate: n_slices slices are needed");
  const int Lg = c->gdims[dir], Ll = c->lat.L[dir], origin = c->lat.origin[dir];
  const int S = n_slices > 0 ? n_slices : Lg;
  // the launch's list: (local slice, index of its matrix in Q) of the listed slices held here, in ascending local slice
  std::vector<int> list;
  {
    std::vector<int> index_of(Ll, -1);
    std::vector<char> seen(Lg, 0);
    for (int s = 0; s < S; ++s) {
      const int t = n_slices > 0 ? slices[s] : s;
      if (t < 0 || t >= Lg) BCG_FAIL(c, BCG_ERR_INVALID, "bcg_basis_slice_rotate: slice outside the lattice");
      if (seen[t]) BCG_FAIL(c, BCG_ERR_INVALID, "bcg_basis_slice_rotate: a slice is listed twice");
      seen[t] = 1;
      if (t >= origin && t < origin + Ll) index_of[t - origin] = s;
    }
    for (int t = 0; t < Ll; ++t)
      if (index_of[t] >= 0) {
        list.push_back(t);
        list.push_back(index_of[t]);
      }
  }
  const size_t entries = static_cast<size_t>(S) * K * K;
  for (size_t e = 0; e < 2 * entries; ++e)
    if (!std::isfinite(Q[e])) BCG_FAIL(c, BCG_ERR_INVALID, "bcg_basis_slice_rotate: Q is not finite");
  const int nl = static_cast<int>(list.size() / 2);
  bcg::SliceWalk plan{};  // planned on a rank without a listed slice too: the refusal is the same on every rank
  if (!bcg::basis_slice_axpy_plan(c->lat, like->parity, dir, std::max(nl, 1), &plan))
    BCG_FAIL(c, BCG_ERR_UNSUPPORTED, "bcg_basis_slice_rotate: a slice of 2^30 rows or more");
  if (nl == 0) return BCG_OK;  // none of the listed slices is here
  // c->dev_rotate: [the matrices of the local listed slices, in the list's order][the list]
  const size_t per = static_cast<size_t>(K) * K;
  const size_t mats = static_cast<size_t>(nl) * per;
  const size_t list_entries = (list.size() * sizeof(int) + sizeof(double2) - 1) / sizeof(double2);
  BCG_TRY(ensure_rotate(c, mats + list_entries));
  HIP_TRY(c, hipEventSynchronize(c->rotate_uploaded));  // the previous upload has left pin_rotate
  for (int l = 0; l < nl; ++l) {
    std::memcpy(c->pin_rotate + 2 * per * l, Q + 2 * per * list[2 * l + 1], per * sizeof(double2));
    list[2 * l + 1] = l;
  }
  std::memcpy(c->pin_rotate + 2 * mats, list.data(), list.size() * sizeof(int));
  HIP_TRY(c, hipMemcpyAsync(c->dev_rotate, c->pin_rotate, (mats + list_entries) * sizeof(double2), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipEventRecord(c->rotate_uploaded, c->stream));
  const int* const list_dev = reinterpret_cast<const int*>(c->dev_rotate + mats);
  {
    const double sites = static_cast<double>(like->sites) / Ll * nl;  // of the listed slices
    ProfScope ps(c, "basis_slice_rotate", sites * 96.0 * K, sites * 3.0 * 8.0 * K * K);
    ProfScope form(c, mfma ? "basis_slice_rotate_mfma" : "basis_slice_rotate_generic");
    if (mfma) {
      int n;
      const bcg::RotateBlocks b = rotate_blocks(V, nv, &n);
      bcg::launch_basis_slice_rotate_mfma(c->stream, n, c->lat, like->parity, dir, plan, nl, list_dev, b, c->dev_rotate);
    } else {
      bcg::launch_basis_slice_rotate_generic(c->stream, c->lat, like->parity, dir, plan, nl, list_dev,
                                             rotate_fields(V, nv, static_cast<int>(K)), c->dev_rotate);
    }
  }
  return check_launch(c, "basis_slice_rotate");
}

}  // extern "C"
