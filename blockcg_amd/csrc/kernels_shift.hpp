// Launchers of the covariant nearest-neighbour sum (include/blockcg_hip.h: bcg_dirac_shift_sum)
//
//   out(x) = c0 in(x) + sum_mu s_mu(x) [ f_mu U_mu(x) in(x+mu) + b_mu U_mu(x-mu)^dagger in(x-mu) ]
//
// s_mu(x) = eta_mu(x) (global coordinates) when eta != 0, else 1.  Layouts are those of kernels.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace bcg {

// Coefficients of one call, passed by value (kernel arguments live in scalar registers: the tests on `fa`, `ba` and
// `use_c0` are wave-uniform branches).
struct ShiftCoef {
  double2 c0;
  double2 f[4], b[4];
  int eta;     // != 0: staggered signs
  int use_c0;  // c0 != 0: in(x) is read
  int fa, ba;  // bit mu set: f[mu] resp. b[mu] is not exactly zero; a direction with neither bit reads no link and no row
};

// Generic form: every width 1..32, every ndim <= 4, ghost faces.  parity < 0: full fields; parity = 0 / 1: `out` holds the
// sites of that parity, `in` those of the other one (half ghost faces, as launch_hop_half).
void launch_shift_generic(hipStream_t s, int m, const LatticeDev& lat, int parity, const double2* U, const double2* Ughost,
                          const double2* in, const double2* ghost, double2* out, const ShiftCoef& cf);

// Tile form: a block covers shift_tile_sites(m) = 256 / m consecutive x0 sites and stages their links in LDS.
// shift_tile_ok: m = 8, 16, 32, a 4-D lattice whose local L0 is a multiple of the run and whose direction 0 is not divided.
int shift_tile_sites(int m);
bool shift_tile_ok(int m, const LatticeDev& lat);
void launch_shift_tile(hipStream_t s, int m, const LatticeDev& lat, const double2* U, const double2* Ughost, const double2* in,
                       const double2* ghost, double2* out, const ShiftCoef& cf);

}  // namespace bcg
