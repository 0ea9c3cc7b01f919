// include/blockcg_hip.h: the fermion force of multi-shift solutions (bcg_force_accumulate) and the gauge-field calls it needs
// (bcg_gauge_download, bcg_gauge_set_zero).  Y_s = D X_s on the existing stencil paths (hop: the specialised stencil or
// k_hop_generic; half fields: k_hop_half), then kernels_force.hip's k_force over up to kForceMaxShifts shifts per launch.
#include <cmath>

#include "capi_internal.hpp"
#include "kernels_force.hpp"

namespace bcg_impl {
namespace {

// bytes of one field's received ghost faces (half fields: half faces, halo_field)
size_t ghost_bytes(const bcg_context* c, const bcg_field* f) {
  const size_t b = static_cast<size_t>(c->ghost_sites) * 3 * f->m * sizeof(double2);
  return f->parity >= 0 ? b / 2 : b;
}

// Y = D X.  Half fields: X of parity p, Y of parity 1 - p (bcg_dirac_hop_half's launch, timed as the half-volume operator's).
// On a divided lattice the receive buffer holds X's ghost faces afterwards: both paths exchange them before their stencil.
int hop_any(bcg_context* c, const bcg_gauge* U, bcg_field* Y, const bcg_field* X) {
  if (X->parity < 0) return hop(c, U, Y, X, bcg::HOP_PLAIN, nullptr, 0.0);
  BCG_TRY(halo_gauge(c, const_cast<bcg_gauge*>(U)));
  BCG_TRY(halo_field(c, X));
  {
    ProfScope ps(c, "hop_half", alg_bytes(c, X->m, 2, 2, 1, 2), hop_flops(c, X->m, false, 1, 2));
    bcg::launch_hop_half(c->stream, X->m, c->lat, Y->parity, U->U, U->Ughost, X->d, c->halo_recv, Y->d, bcg::HOP_PLAIN, nullptr,
                         0.0);
  }
  return check_launch(c, "hop_half");
}

// a copy of the receive buffer's faces in slot `slot` of the call's ghost buffer (the context has one receive buffer; X's
// faces must outlive Y's exchange)
int keep_ghosts(bcg_context* c, char* ghosts, size_t bytes, size_t slot) {
  HIP_TRY(c, hipMemcpyAsync(ghosts + slot * bytes, c->halo_recv, bytes, hipMemcpyDeviceToDevice, c->stream));
  return BCG_OK;
}

// what the call allocates for itself, released on return (the stream is synchronised first: the kernels may still read it)
struct CallBuffers {
  bcg_context* c;
  bcg_field* own = nullptr;  // the work field when the caller passes none
  char* ghosts = nullptr;    // divided lattice: the kept ghost faces of X_s and Y_s, 2 sets per shift of a launch
  explicit CallBuffers(bcg_context* ctx) : c(ctx) {}
  ~CallBuffers() {
    if (ghosts) {
      (void)hipStreamSynchronize(c->stream);
      (void)hipFree(ghosts);
    }
    if (own) (void)bcg_field_destroy(own);
  }
};

}  // namespace
}  // namespace bcg_impl

using namespace bcg_impl;

extern "C" {

int bcg_gauge_download(const bcg_gauge* g, double* host) {
  DeviceScope on_device(g ? g->ctx : nullptr);
  if (!g || !host) return BCG_ERR_INVALID;
  bcg_context* c = g->ctx;
  HIP_TRY(c, hipMemcpyAsync(host, g->U, static_cast<size_t>(c->lat.V) * c->ndim * 9 * sizeof(double2), hipMemcpyDeviceToHost,
                            c->stream));
  return stream_sync(c);
}

int bcg_gauge_set_zero(bcg_gauge* g) {
  DeviceScope on_device(g ? g->ctx : nullptr);
  if (!g) return BCG_ERR_INVALID;
  bcg_context* c = g->ctx;
  HIP_TRY(c, hipMemsetAsync(g->U, 0, static_cast<size_t>(c->lat.V) * c->ndim * 9 * sizeof(double2), c->stream));
  g->ghost_valid = false;
  return BCG_OK;
}

int bcg_force_accumulate(bcg_context* c, const bcg_gauge* U, bcg_field* const* X, int n_shifts, const double* residue,
                         double scale, int project, bcg_field* const* work, int n_work, bcg_gauge* F) {
  DeviceScope on_device(c);
  if (!c) return BCG_ERR_INVALID;
  // ---- validate everything before anything is allocated or exchanged (a rank that fails here posts no message) ----
  if (!U || !F || !X || !residue || n_shifts < 1 || n_work < 0 || (n_work > 0 && !work))
    BCG_FAIL(c, BCG_ERR_INVALID, "bcg_force_accumulate: null argument, n_shifts < 1 or n_work < 0");
  if (F == U) BCG_FAIL(c, BCG_ERR_INVALID, "bcg_force_accumulate: F must not be the links U");
  if (U->ctx != c || F->ctx != c) BCG_FAIL(c, BCG_ERR_INVALID, "bcg_force_accumulate: U or F belongs to another context");
  if (!std::isfinite(scale)) BCG_FAIL(c, BCG_ERR_INVALID, "bcg_force_accumulate: scale is not finite");
  for (int s = 0; s < n_shifts; ++s) {
    if (!X[s] || X[s]->ctx != c) BCG_FAIL(c, BCG_ERR_INVALID, "bcg_force_accumulate: a field X_s is null or of another context");
    if (X[s]->m != X[0]->m || X[s]->parity != X[0]->parity)
      BCG_FAIL(c, BCG_ERR_INVALID, "bcg_force_accumulate: the fields X_s differ in width or parity");
    if (!std::isfinite(residue[s])) BCG_FAIL(c, BCG_ERR_INVALID, "bcg_force_accumulate: a residue is not finite");
  }
  for (int i = 0; i < n_work; ++i) {
    const bcg_field* w = work[i];
    if (!w || w->ctx != c || w->m != X[0]->m || w->parity != X[0]->parity)
      BCG_FAIL(c, BCG_ERR_INVALID, "bcg_force_accumulate: a work field is null, of another context, or of the wrong width or parity");
    for (int s = 0; s < n_shifts; ++s)
      if (w == X[s]) BCG_FAIL(c, BCG_ERR_INVALID, "bcg_force_accumulate: a work field is one of the X_s");
    for (int k = 0; k < i; ++k)
      if (w == work[k]) BCG_FAIL(c, BCG_ERR_INVALID, "bcg_force_accumulate: a work field is listed twice");
  }
  if (c->lat.V * c->ndim >= (int64_t{1} << 31))
    BCG_FAIL(c, BCG_ERR_UNSUPPORTED, "bcg_force_accumulate: more than 2^31 links on this rank");
  const int m = X[0]->m, parity = X[0]->parity;
  const int per_launch = std::min(std::min(n_work > 0 ? n_work : 1, n_shifts), bcg::kForceMaxShifts);

  // ---- then allocate: the work field, the stencil's scratch, the receive buffer and the kept ghost faces.  On a divided
  // lattice the ranks agree on the outcome before the first exchange (halo_gauge / halo_field below), so that a rank that
  // could not allocate does not leave its peers waiting there: every rank returns the error, with F untouched ----
  CallBuffers buf(c);
  const size_t gbytes = ghost_bytes(c, X[0]);
  int alloc_rc = n_work == 0 ? create_like(c, X[0], &buf.own) : BCG_OK;
  if (alloc_rc == BCG_OK) alloc_rc = ensure_scratch(c);
  if (alloc_rc == BCG_OK && c->distributed) alloc_rc = ensure_halo(c, static_cast<size_t>(c->ghost_sites) * 3 * m * sizeof(double2));
  if (alloc_rc == BCG_OK && c->distributed && gbytes > 0) {
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(&buf.ghosts), 2 * per_launch * gbytes);
    if (e != hipSuccess) {
      buf.ghosts = nullptr;
      c->err = std::string("bcg_force_accumulate: hipMalloc of the ghost faces: ") + hipGetErrorString(e);
      alloc_rc = BCG_ERR_HIP;
    }
  }
  BCG_TRY(agree_on_allocation(c, alloc_rc, "bcg_force_accumulate", "the call's work field or ghost faces"));

  // ---- per launch: Y_s = D X_s for its shifts (ghosts of X_s and Y_s kept aside), then one pass over F ----
  const char* name = project ? "force_project" : "force";
  for (int s0 = 0; s0 < n_shifts; s0 += per_launch) {
    const int n = std::min(per_launch, n_shifts - s0);
    bcg::ForceShifts sh{};
    sh.n = n;
    bcg_field Yv[bcg::kForceMaxShifts];
    for (int i = 0; i < n; ++i) {
      const bcg_field* x = X[s0 + i];
      // a work field is storage of X's shape; Y of a half field has the other parity (same site count)
      Yv[i] = *(n_work > 0 ? work[i] : buf.own);
      if (parity >= 0) Yv[i].parity = 1 - parity;
      BCG_TRY(hop_any(c, U, &Yv[i], x));
      if (c->distributed) {
        BCG_TRY(keep_ghosts(c, buf.ghosts, gbytes, 2 * i));  // X_s's faces, left by the stencil's exchange
        BCG_TRY(halo_field(c, &Yv[i]));
        BCG_TRY(keep_ghosts(c, buf.ghosts, gbytes, 2 * i + 1));
        sh.Xg[i] = reinterpret_cast<const double2*>(buf.ghosts + 2 * i * gbytes);
        sh.Yg[i] = reinterpret_cast<const double2*>(buf.ghosts + (2 * i + 1) * gbytes);
      }
      sh.X[i] = x->d;
      sh.Y[i] = Yv[i].d;
      sh.w[i] = scale * residue[s0 + i];
    }
    {
      // byte model: X_s and Y_s once per shift, F read and written once per launch, U once when projecting
      const double sites = static_cast<double>(X[0]->sites);
      const double links = static_cast<double>(c->lat.V) * 144.0 * c->ndim;
      const double flops = static_cast<double>(c->lat.V) * c->ndim * 9.0 * 8.0 * m * (parity < 0 ? 2.0 : 1.0) * n;
      ProfScope ps(c, name, 2.0 * n * sites * 48.0 * m + (project ? 3.0 : 2.0) * links, flops);
      bcg::launch_force(c->stream, m, c->lat, parity, sh, U->U, F->U, project != 0);
    }
    BCG_TRY(check_launch(c, name));
  }
  F->ghost_valid = false;
  return BCG_OK;  // (the call's own buffers are freed on return, after the stream has drained)
}

}  // extern "C"
