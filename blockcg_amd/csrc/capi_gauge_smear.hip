// include/blockcg_hip.h: stout smearing of the gauge links (bcg_gauge_stout_smear) and the plaquette (bcg_gauge_plaquette).
// Kernels: kernels_gauge_smear.hip.  Arguments are checked with global data only and before the first
// exchange or launch, so every rank of a divided lattice returns the same status and a failed call leaves its output as it
// was.  Divided lattices: per step one exchange of the faces of all ndim links, then one of the backward staples W on the
// high faces (the corner link U_nu(x-nu+mu) never crosses a rank boundary by itself); both sets of received faces live in a
// buffer of the call, not in bcg_gauge::Ughost, whose meaning is the stencil's.
#include <cmath>

#include "capi_internal.hpp"
#include "kernels_gauge_smear.hpp"

namespace bcg_impl {
namespace {

constexpr size_t kLinkBytes = 9 * sizeof(double2);

size_t links_bytes(const bcg_context* c) { return static_cast<size_t>(c->lat.V) * c->ndim * kLinkBytes; }

// what the call allocates for itself, released on return (after the stream has drained: the kernels may still read it)
struct SmearBuffers {
  bcg_context* c;
  bcg_gauge* own = nullptr;  // the work container when the caller passes none
  char* ghosts = nullptr;    // divided lattice: [link faces: ghost_sites * ndim links][W faces: ghost_sites * (ndim - 1)]
  explicit SmearBuffers(bcg_context* ctx) : c(ctx) {}
  ~SmearBuffers() {
    if (ghosts) {
      (void)hipStreamSynchronize(c->stream);
      (void)hipFree(ghosts);
    }
    if (own) (void)bcg_gauge_destroy(own);  // (synchronises the stream first)
  }
};

int alloc_ghosts(bcg_context* c, SmearBuffers& buf, size_t bytes, const char* who) {
  const hipError_t e = hipMalloc(reinterpret_cast<void**>(&buf.ghosts), bytes);
  if (e != hipSuccess) {
    buf.ghosts = nullptr;
    c->err = std::string(who) + ": hipMalloc of the ghost faces: " + hipGetErrorString(e);
    return BCG_ERR_HIP;
  }
  return BCG_OK;
}

// the faces of all ndim links of U, received into `ghost` (a link row is 3 x (3 ndim) complex: the field packer at m = 3 ndim)
int exchange_link_faces(bcg_context* c, const double2* U, char* ghost) {
  const size_t site_bytes = static_cast<size_t>(c->ndim) * kLinkBytes;
  bcg::launch_pack_faces(c->stream, 3 * c->ndim, c->lat, U, c->halo_send);
  BCG_TRY(check_launch(c, "pack_link_faces"));
  BCG_TRY(exchange_faces(c, site_bytes, false, 0, 0, 0, 0));
  HIP_TRY(c, hipMemcpyAsync(ghost, c->halo_recv, static_cast<size_t>(c->ghost_sites) * site_bytes, hipMemcpyDeviceToDevice, c->stream));
  return BCG_OK;
}

}  // namespace
}  // namespace bcg_impl

using namespace bcg_impl;

extern "C" {

int bcg_gauge_stout_smear(bcg_context* c, bcg_gauge* out, const bcg_gauge* in, const double* rho, int n_steps, bcg_gauge* work) {
  DeviceScope on_device(c);
  if (!c) return BCG_ERR_INVALID;
  // ---- checks, on global data only ----
  if (!out || !in || !rho) BCG_FAIL(c, BCG_ERR_INVALID, "bcg_gauge_stout_smear: null argument");
  if (out == in || work == out || (work && work == in))
    BCG_FAIL(c, BCG_ERR_INVALID, "bcg_gauge_stout_smear: out, in and work must be three containers");
  if (out->ctx != c || in->ctx != c || (work && work->ctx != c))
    BCG_FAIL(c, BCG_ERR_INVALID, "bcg_gauge_stout_smear: a container belongs to another context");
  if (n_steps < 0) BCG_FAIL(c, BCG_ERR_INVALID, "bcg_gauge_stout_smear: n_steps < 0");
  const int nd = c->ndim;
  bcg::StoutArgs a{};
  int terms = 0, smeared = 0;
  for (int mu = 0; mu < nd; ++mu)
    for (int nu = 0; nu < nd; ++nu) {
      if (mu == nu) continue;
      const double r = rho[mu * nd + nu];
      if (!std::isfinite(r)) BCG_FAIL(c, BCG_ERR_INVALID, "bcg_gauge_stout_smear: a weight rho[mu][nu] is not finite");
      if (c->gdims[mu] == 1 || c->gdims[nu] == 1 || r == 0.0) continue;  // a direction of extent 1 takes no part
      a.rho[mu * 4 + nu] = r;
      a.smear_mask |= 1 << mu;
      ++terms;
    }
  for (int mu = 0; mu < nd; ++mu) smeared += (a.smear_mask >> mu) & 1;
  if (c->distributed && (!c->have_comm || !c->comm.halo_exchange))
    BCG_FAIL(c, BCG_ERR_COMM, "bcg_gauge_stout_smear: lattice is split over ranks but no bcg_comm was set");
  if (c->lat.V * nd >= (int64_t{1} << 31)) BCG_FAIL(c, BCG_ERR_UNSUPPORTED, "bcg_gauge_stout_smear: more than 2^31 links on this rank");

  // no step, or no term at all: S is the identity, a device copy
  if (n_steps == 0 || a.smear_mask == 0) {
    HIP_TRY(c, hipMemcpyAsync(out->U, in->U, links_bytes(c), hipMemcpyDeviceToDevice, c->stream));
    out->ghost_valid = false;
    return BCG_OK;
  }

  // ---- allocate before the first launch or exchange; the ranks of a divided lattice agree on the outcome ----
  SmearBuffers buf(c);
  const bool ghosts = c->distributed && c->ghost_sites > 0;
  const size_t link_ghost_bytes = static_cast<size_t>(c->ghost_sites) * nd * kLinkBytes;
  const size_t w_ghost_bytes = static_cast<size_t>(c->ghost_sites) * (nd - 1) * kLinkBytes;
  int alloc_rc = BCG_OK;
  if (n_steps >= 2 && !work) {
    alloc_rc = bcg_gauge_create(c, &buf.own);
    if (alloc_rc != BCG_OK) buf.own = nullptr;
    work = buf.own;
  }
  if (alloc_rc == BCG_OK && ghosts) alloc_rc = ensure_halo(c, link_ghost_bytes);
  if (alloc_rc == BCG_OK && ghosts) alloc_rc = alloc_ghosts(c, buf, link_ghost_bytes + w_ghost_bytes, "bcg_gauge_stout_smear");
  BCG_TRY(agree_on_allocation(c, alloc_rc, "bcg_gauge_stout_smear", "the call's work container or ghost faces"));
  const double2* link_ghost = reinterpret_cast<const double2*>(buf.ghosts);
  const double2* w_ghost = ghosts ? reinterpret_cast<const double2*>(buf.ghosts + link_ghost_bytes) : nullptr;

  // ---- the steps alternate between out and work so that the last one writes out ----
  const bcg_gauge* src = in;
  for (int k = 0; k < n_steps; ++k) {
    bcg_gauge* dst = ((n_steps - 1 - k) & 1) ? work : out;
    if (ghosts) {
      BCG_TRY(exchange_link_faces(c, src->U, buf.ghosts));
      bcg::launch_stout_w_faces(c->stream, c->lat, a, src->U, link_ghost, c->halo_send);
      BCG_TRY(check_launch(c, "stout_w_faces"));
      BCG_TRY(exchange_faces(c, static_cast<size_t>(nd - 1) * kLinkBytes, false, 0, 0, 0, 0));
      HIP_TRY(c, hipMemcpyAsync(buf.ghosts + link_ghost_bytes, c->halo_recv, w_ghost_bytes, hipMemcpyDeviceToDevice, c->stream));
    }
    {
      // bytes: every link read once and written once (144 B each way); flops: per evaluated (mu, nu) term four 3 x 3 products
      // (216 each) and two scaled additions (36 each), per smeared link Omega, Q^2 and the final product (216 each) and about
      // 150 for the coefficients and the polynomial
      const double V = static_cast<double>(c->lat.V);
      ProfScope ps(c, "stout_smear", 2.0 * V * 144.0 * nd, V * (terms * 936.0 + smeared * 798.0));
      bcg::launch_stout_step(c->stream, c->lat, a, src->U, link_ghost, w_ghost, dst->U);
    }
    BCG_TRY(check_launch(c, "stout_smear"));
    dst->ghost_valid = false;
    src = dst;
  }
  out->ghost_valid = false;
  return BCG_OK;  // (the call's own buffers are freed on return, after the stream has drained)
}

int bcg_gauge_plaquette(bcg_context* c, const bcg_gauge* g, double* out) {
  DeviceScope on_device(c);
  if (!c) return BCG_ERR_INVALID;
  if (!g || !out) BCG_FAIL(c, BCG_ERR_INVALID, "bcg_gauge_plaquette: null argument");
  if (g->ctx != c) BCG_FAIL(c, BCG_ERR_INVALID, "bcg_gauge_plaquette: the links belong to another context");
  if (c->distributed && (!c->have_comm || !c->comm.halo_exchange || !c->comm.allreduce_sum))
    BCG_FAIL(c, BCG_ERR_COMM, "bcg_gauge_plaquette: lattice is split over ranks but no bcg_comm was set");
  if (c->lat.V * c->ndim >= (int64_t{1} << 31)) BCG_FAIL(c, BCG_ERR_UNSUPPORTED, "bcg_gauge_plaquette: more than 2^31 links on this rank");
  const int nd = c->ndim;
  int active = 0;
  double Vg = 1.0;
  for (int mu = 0; mu < nd; ++mu) {
    if (c->gdims[mu] > 1) active |= 1 << mu;
    Vg *= c->gdims[mu];
  }

  SmearBuffers buf(c);
  const bool ghosts = c->distributed && c->ghost_sites > 0;
  const size_t link_ghost_bytes = static_cast<size_t>(c->ghost_sites) * nd * kLinkBytes;
  int alloc_rc = ensure_scratch(c);
  if (alloc_rc == BCG_OK && ghosts) alloc_rc = ensure_halo(c, link_ghost_bytes);
  if (alloc_rc == BCG_OK && ghosts) alloc_rc = alloc_ghosts(c, buf, link_ghost_bytes, "bcg_gauge_plaquette");
  BCG_TRY(agree_on_allocation(c, alloc_rc, "bcg_gauge_plaquette", "the call's ghost faces"));
  if (ghosts) BCG_TRY(exchange_link_faces(c, g->U, buf.ghosts));

  int nblocks;
  {
    // bytes: the links once; flops: two 3 x 3 products and one trace per plane and site
    const double V = static_cast<double>(c->lat.V);
    int planes = 0;
    for (int mu = 0; mu < nd; ++mu)
      for (int nu = mu + 1; nu < nd; ++nu) planes += ((active >> mu) & 1) && ((active >> nu) & 1);
    ProfScope ps(c, "plaquette", V * 144.0 * nd, V * planes * 468.0);
    nblocks = bcg::launch_plaquette(c->stream, c->lat, active, g->U, reinterpret_cast<const double2*>(buf.ghosts), c->partials, kFastBlocks);
  }
  BCG_TRY(check_launch(c, "plaquette"));
  bcg::launch_reduce_partials(c->stream, bcg::kPlaqValues, nblocks, c->partials, c->dev_gram);
  BCG_TRY(check_launch(c, "reduce_partials"));
  if (c->distributed && c->comm.allreduce_sum(c->comm.user, c->dev_gram, static_cast<size_t>(2) * bcg::kPlaqValues) != 0)
    BCG_FAIL(c, BCG_ERR_COMM, "allreduce_sum callback failed");
  HIP_TRY(c, hipMemcpyAsync(c->pin_gram, c->dev_gram, bcg::kPlaqValues * sizeof(double2), hipMemcpyDeviceToHost, c->stream));
  BCG_TRY(stream_sync(c));
  for (int i = 0; i < nd * nd; ++i) out[i] = 0.0;
  for (int mu = 0; mu < nd; ++mu)
    for (int nu = mu + 1; nu < nd; ++nu) {
      if (!((active >> mu) & 1) || !((active >> nu) & 1)) continue;
      const double p = c->pin_gram[2 * (mu * 4 + nu)] / (3.0 * Vg);
      out[mu * nd + nu] = out[nu * nd + mu] = p;
    }
  return BCG_OK;
}

}  // extern "C"
