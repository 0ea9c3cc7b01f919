// Launchers of stout link smearing and the plaquette (include/blockcg_hip.h, "gauge links: stout smearing and plaquettes";
// DESIGN.md section 8m).  Links: [site][mu < ndim][3x3 column-major].  On a divided lattice
//   link_ghost  the received faces of ALL ndim links of a site (ndim * 9 complex per ghost site, the face numbering and the
//               ghost offsets of LatticeDev; only the plus faces are read), and
//   w_ghost     the received backward staples W_{mu nu}(y) = U_nu(y)^dagger U_mu(y) U_nu(y+mu) of the minus-nu neighbour's
//               high face: (ndim - 1) * 9 complex per ghost site, mu ascending without nu, in the minus ghost of nu.
#pragma once
#include "kernels.hpp"

namespace bcg {

struct StoutArgs {
  double rho[16];  // rho[mu * 4 + nu] as the kernels use it: 0 on the diagonal, beyond ndim and where mu or nu has global extent 1
  int smear_mask;  // bit mu: row mu has a non-zero entry (the other directions are copied)
};

constexpr int kPlaqValues = 16;  // block partials of the plaquette: one complex slot per (mu, nu), mu * 4 + nu, mu < nu filled

// out = one stout step of U
void launch_stout_step(hipStream_t s, const LatticeDev& lat, const StoutArgs& a, const double2* U, const double2* link_ghost,
                       const double2* w_ghost, double2* out);
// W_{mu nu} on the high face of every divided nu, into `send` in face order (the high-face slot of nu; (ndim - 1) * 9 complex
// per site); entries with rho[mu][nu] == 0 are left as they were
void launch_stout_w_faces(hipStream_t s, const LatticeDev& lat, const StoutArgs& a, const double2* U, const double2* link_ghost,
                          double2* send);
// partials[block][kPlaqValues]: sum over the block's sites of Re tr of the plaquette of plane (mu, nu), for the planes with
// both bits set in active_mask; returns the number of blocks (fixed by the volume)
int launch_plaquette(hipStream_t s, const LatticeDev& lat, int active_mask, const double2* U, const double2* link_ghost,
                     double2* partials, int max_blocks);

}  // namespace bcg
