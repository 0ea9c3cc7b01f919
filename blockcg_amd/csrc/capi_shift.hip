// include/blockcg_hip.h: the covariant nearest-neighbour sum (bcg_dirac_shift_sum) and covariant smearing on top of it
// (bcg_covariant_smear).  Kernels: kernels_shift.hip.  Arguments are checked with global data only
// and before the first exchange or launch, so every rank of a divided lattice returns the same status and a failed call
// leaves its output as it was.
#include <cmath>

#include "capi_internal.hpp"
#include "kernels_shift.hpp"

namespace bcg_impl {
namespace {

bool finite_pair(const double* p) { return std::isfinite(p[0]) && std::isfinite(p[1]); }
bool nonzero_pair(const double* p) { return p[0] != 0.0 || p[1] != 0.0; }

// the coefficients as the kernels take them; false: a non-finite one
bool make_coef(const bcg_context* c, const double* c0, const double* fwd, const double* bwd, int eta, bcg::ShiftCoef* cf) {
  *cf = bcg::ShiftCoef{};
  if (!finite_pair(c0)) return false;
  cf->c0 = make_double2(c0[0], c0[1]);
  cf->use_c0 = nonzero_pair(c0) ? 1 : 0;
  cf->eta = eta != 0 ? 1 : 0;
  for (int mu = 0; mu < 4; ++mu) {
    cf->f[mu] = cf->b[mu] = make_double2(0, 0);
    if (mu >= c->ndim) continue;
    if (fwd) {
      if (!finite_pair(fwd + 2 * mu)) return false;
      cf->f[mu] = make_double2(fwd[2 * mu], fwd[2 * mu + 1]);
      if (nonzero_pair(fwd + 2 * mu)) cf->fa |= 1 << mu;
    }
    if (bwd) {
      if (!finite_pair(bwd + 2 * mu)) return false;
      cf->b[mu] = make_double2(bwd[2 * mu], bwd[2 * mu + 1]);
      if (nonzero_pair(bwd + 2 * mu)) cf->ba |= 1 << mu;
    }
  }
  return true;
}

int count_bits(int v) {
  int n = 0;
  for (; v; v &= v - 1) ++n;
  return n;
}

// out = S in for checked arguments: the gauge ghost if stale, one blocking exchange of in's faces, one launch
int shift_sum(bcg_context* c, const bcg_gauge* g, bcg_field* out, const bcg_field* in, const bcg::ShiftCoef& cf) {
  BCG_TRY(halo_gauge(c, const_cast<bcg_gauge*>(g)));
  BCG_TRY(halo_field(c, in));
  const int m = in->m;
  const bool tile = in->parity < 0 && !c->force_generic && bcg::shift_tile_ok(m, c->lat);
  if (c->profiling) c->prof[tile ? "shift_form_tile" : "shift_form_generic"].count += 1;
  {
    // bytes: `in` and `out` once, 144 B per site and direction with a non-zero coefficient; flops: 72 of the 3 x 3 product
    // and 24 of the scaling per term, site and column, 24 for c0
    const double sites = static_cast<double>(out->sites);
    const int terms = count_bits(cf.fa) + count_bits(cf.ba);
    ProfScope ps(c, "shift_sum", sites * (96.0 * m + 144.0 * count_bits(cf.fa | cf.ba)),
                 sites * m * (96.0 * terms + (cf.use_c0 ? 24.0 : 0.0)));
    if (tile)
      bcg::launch_shift_tile(c->stream, m, c->lat, g->U, g->Ughost, in->d, c->halo_recv, out->d, cf);
    else
      bcg::launch_shift_generic(c->stream, m, c->lat, out->parity, g->U, g->Ughost, in->d, c->halo_recv, out->d, cf);
  }
  return check_launch(c, "shift_sum");
}

struct OwnField {
  bcg_field* f = nullptr;
  ~OwnField() {
    if (f) (void)bcg_field_destroy(f);  // (synchronises the stream first)
  }
};

}  // namespace
}  // namespace bcg_impl

using namespace bcg_impl;

extern "C" {

int bcg_dirac_shift_sum(bcg_context* c, const bcg_gauge* g, bcg_field* out, const bcg_field* in, const double* c0,
                        const double* fwd, const double* bwd, int eta) {
  DeviceScope on_device(c);
  if (!c) return BCG_ERR_INVALID;
  if (!g || !out || !in || !c0) BCG_FAIL(c, BCG_ERR_INVALID, "bcg_dirac_shift_sum: null argument");
  if (out == in) BCG_FAIL(c, BCG_ERR_INVALID, "bcg_dirac_shift_sum: out must not be in");
  if (g->ctx != c || in->ctx != c || out->ctx != c) BCG_FAIL(c, BCG_ERR_INVALID, "bcg_dirac_shift_sum: an argument belongs to another context");
  if (out->m != in->m) BCG_FAIL(c, BCG_ERR_INVALID, "bcg_dirac_shift_sum: out and in differ in width");
  const bool half = in->parity >= 0;
  if (half ? out->parity != 1 - in->parity : out->parity >= 0)
    BCG_FAIL(c, BCG_ERR_INVALID, "bcg_dirac_shift_sum: full fields, or a half field in and out of the opposite parity");
  bcg::ShiftCoef cf;
  if (!make_coef(c, c0, fwd, bwd, eta, &cf)) BCG_FAIL(c, BCG_ERR_INVALID, "bcg_dirac_shift_sum: a coefficient is not finite");
  if (half && cf.use_c0) BCG_FAIL(c, BCG_ERR_INVALID, "bcg_dirac_shift_sum: c0 must be 0 with half fields (in(x) has the other parity)");
  if (c->distributed && (!c->have_comm || !c->comm.halo_exchange))
    BCG_FAIL(c, BCG_ERR_COMM, "bcg_dirac_shift_sum: lattice is split over ranks but no bcg_comm was set");
  return shift_sum(c, g, out, in, cf);
}

int bcg_covariant_smear(bcg_context* c, const bcg_gauge* g, bcg_field* f, bcg_field* work, int dir, double kappa, int n_iter) {
  DeviceScope on_device(c);
  if (!c) return BCG_ERR_INVALID;
  if (!g || !f) BCG_FAIL(c, BCG_ERR_INVALID, "bcg_covariant_smear: null argument");
  if (g->ctx != c || f->ctx != c) BCG_FAIL(c, BCG_ERR_INVALID, "bcg_covariant_smear: an argument belongs to another context");
  if (work && (work == f || work->ctx != c || work->m != f->m || work->parity != f->parity))
    BCG_FAIL(c, BCG_ERR_INVALID, "bcg_covariant_smear: work is f, or of another context, width or parity");
  if (dir < -1 || dir >= c->ndim) BCG_FAIL(c, BCG_ERR_INVALID, "bcg_covariant_smear: dir outside -1 ... ndim - 1");
  if (n_iter < 0) BCG_FAIL(c, BCG_ERR_INVALID, "bcg_covariant_smear: n_iter < 0");
  if (!std::isfinite(kappa)) BCG_FAIL(c, BCG_ERR_INVALID, "bcg_covariant_smear: kappa is not finite");
  if (f->parity >= 0) BCG_FAIL(c, BCG_ERR_UNSUPPORTED, "bcg_covariant_smear: one link flips the parity, so half fields cannot be smeared in place");
  if (c->distributed && (!c->have_comm || !c->comm.halo_exchange))
    BCG_FAIL(c, BCG_ERR_COMM, "bcg_covariant_smear: lattice is split over ranks but no bcg_comm was set");
  if (n_iter == 0) return BCG_OK;

  // the coefficients a caller of bcg_dirac_shift_sum would pass
  const int smeared = c->ndim - (dir >= 0 ? 1 : 0);
  const double c0[2] = {1.0 - 2.0 * kappa * smeared, 0.0};
  double hop[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int mu = 0; mu < c->ndim; ++mu)
    if (mu != dir) hop[2 * mu] = kappa;
  bcg::ShiftCoef cf;
  if (!make_coef(c, c0, hop, hop, 0, &cf)) BCG_FAIL(c, BCG_ERR_INVALID, "bcg_covariant_smear: a coefficient is not finite");

  OwnField own;
  if (!work) {
    const int alloc_rc = create_like(c, f, &own.f);
    BCG_TRY(agree_on_allocation(c, alloc_rc, "bcg_covariant_smear", "the call's work field"));
    work = own.f;
  }
  bcg_field* a = f;
  bcg_field* b = work;
  for (int it = 0; it < n_iter; ++it) {
    BCG_TRY(shift_sum(c, g, b, a, cf));
    std::swap(a, b);
  }
  if (a != f)  // an odd number of steps ended in work
    HIP_TRY(c, hipMemcpyAsync(f->d, a->d, field_bytes(f), hipMemcpyDeviceToDevice, c->stream));
  return BCG_OK;
}

}  // extern "C"
