// include/blockcg_hip.h: bcg_basis_rotate -- V <- V Q in place for a list V of fields whose widths sum to K <= 64 and a
// K x K matrix Q.  Kernels: kernels_rotate.hip (one launch takes all K columns).  The uploaded Q lives in c->dev_rotate /
// c->pin_rotate (64 x 64 entries, allocated on first use, freed by bcg_context_destroy).  No communication call.
#include "capi_internal.hpp"
#include "kernels_basis.hpp"
#include "kernels_rotate.hpp"

static_assert(BCG_BASIS_ROTATE_MAX_COLUMNS == bcg::kRotateMaxCols, "the header's constant is the kernels' bound");

namespace bcg_impl {
namespace {

int ensure_rotate(bcg_context* c) {
  constexpr size_t bytes = static_cast<size_t>(bcg::kRotateMaxCols) * bcg::kRotateMaxCols * sizeof(double2);
  if (!c->rotate_uploaded) HIP_TRY(c, hipEventCreateWithFlags(&c->rotate_uploaded, hipEventDisableTiming));
  if (!c->dev_rotate) HIP_TRY(c, hipMalloc(&c->dev_rotate, bytes));
  if (!c->pin_rotate) HIP_TRY(c, hipHostMalloc(reinterpret_cast<void**>(&c->pin_rotate), bytes, hipHostMallocDefault));
  return BCG_OK;
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
  int64_t K = 0;
  bool mfma = !c->force_generic;
  for (int k = 0; k < nv; ++k) {
    const bcg_field* v = V[k];
    if (!v || v->ctx != c || v->parity != like->parity || v->sites != like->sites) return BCG_ERR_INVALID;
    for (int l = 0; l < k; ++l)
      if (V[l] == v) BCG_FAIL(c, BCG_ERR_INVALID, "bcg_basis_rotate: a field is listed twice");
    mfma = mfma && bcg::basis_mfma_width(v->m);
    K += v->m;
  }
  if (K > bcg::kRotateMaxCols) BCG_FAIL(c, BCG_ERR_UNSUPPORTED, "bcg_basis_rotate: more than 64 columns");
  const size_t entries = static_cast<size_t>(K) * K;
  for (size_t e = 0; e < 2 * entries; ++e)
    if (!std::isfinite(Q[e])) BCG_FAIL(c, BCG_ERR_INVALID, "bcg_basis_rotate: Q is not finite");
  BCG_TRY(ensure_rotate(c));
  HIP_TRY(c, hipEventSynchronize(c->rotate_uploaded));  // the previous upload has left pin_rotate
  std::memcpy(c->pin_rotate, Q, entries * sizeof(double2));
  HIP_TRY(c, hipMemcpyAsync(c->dev_rotate, c->pin_rotate, entries * sizeof(double2), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipEventRecord(c->rotate_uploaded, c->stream));
  {
    ProfScope ps(c, "basis_rotate", static_cast<double>(like->sites) * 96.0 * K, static_cast<double>(rows_of(like)) * 8.0 * K * K);
    ProfScope form(c, mfma ? "basis_rotate_mfma" : "basis_rotate_generic");
    if (mfma) {
      bcg::RotateBlocks b{};
      int n = 0;
      for (int k = 0; k < nv; ++k)
        for (int c0 = 0; c0 < V[k]->m; c0 += 16) {
          b.p[n] = V[k]->d + c0;
          b.ld[n] = V[k]->m;
          n += 1;
        }
      bcg::launch_basis_rotate_mfma(c->stream, n, rows_of(like), b, c->dev_rotate);
    } else {
      bcg::RotateFields f{};
      f.nv = nv;
      f.K = static_cast<int>(K);
      for (int k = 0; k < nv; ++k) {
        f.v[k] = V[k]->d;
        f.w[k] = static_cast<unsigned char>(V[k]->m);
      }
      bcg::launch_basis_rotate_generic(c->stream, rows_of(like), f, c->dev_rotate);
    }
  }
  return check_launch(c, "basis_rotate");
}

}  // extern "C"
