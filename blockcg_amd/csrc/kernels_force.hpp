// Launcher of the fermion-force kernel (kernels_force.hip; include/blockcg_hip.h, bcg_force_accumulate).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.hpp"

namespace bcg {

constexpr int kForceMaxShifts = 8;  // shifts one launch handles (kernel-argument space)

// The operands of one launch: per shift s < n the field X_s, Y_s = D X_s (device layout; half fields: X of the launch's
// parity, Y of the other), the received ghost faces of both (the layout halo_field leaves in the receive buffer, copied
// aside; nullptr on an undivided lattice) and the weight w_s = scale * residue[s].
struct ForceShifts {
  const double2* X[kForceMaxShifts];
  const double2* Y[kForceMaxShifts];
  const double2* Xg[kForceMaxShifts];
  const double2* Yg[kForceMaxShifts];
  double w[kForceMaxShifts];
  int n;
};

// F[site][mu][3x3 column-major] += sum_s w_s G_s(site, mu)         (project = false)
//                               += TA(U_mu(site) sum_s w_s G_s)     (project = true)
//   G_s(x, mu) = eta_mu(x) sum_j [ Y_sj(x+mu) X_sj(x)^dagger - X_sj(x+mu) Y_sj(x)^dagger ]
// over every local site and direction.  parity = -1: full fields; 0 / 1: half fields, X of that parity (the terms whose
// factors live on the other parity vanish).  Any width 1 <= m <= 32.
void launch_force(hipStream_t s, int m, const LatticeDev& lat, int parity, const ForceShifts& sh, const double2* U, double2* F,
                  bool project);

}  // namespace bcg
