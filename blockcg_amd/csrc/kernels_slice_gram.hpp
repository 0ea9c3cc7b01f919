// Launchers of the per-slice Gram kernels (kernels_slice_gram.hip; include/blockcg_hip.h: bcg_field_slice_gram).
//
//   C_p(t)(i, j) = sum_{x : x_dir = t} w_p(x) sum_c conj(a[x, c, i]) b[x, c, j]        over the LOCAL sites,
//   w_p(x) = prod_{mu != dir} tab[p][slot of mu][x_mu]                                 (ascending mu)
//
// The walk over the rows of a slice, and how blocks per slice and chunk follow from the blocks wanted: slice_plan.hpp.
//
// The launch plan (slice_gram_plan, slice_plan.hpp) is a function of (shape, m, parity, dir, n_mom) only:
//   pc     momenta per launch: the largest instantiated count (MFMA m = 16: 1, 2, 4; m = 32 and the generic kernel: 1, 2)
//          that is <= max(n_mom, 1) and whose reduced result pc * L_global * m^2 fits its half of the scratch
//   blocks budget = min(2048, entries left in the partials' half / (pc * m^2)); blocks per slice wanted = budget / L_local
// A call's last launch may carry fewer momenta (the smallest instantiated count that holds them; the tables of the unused
// ones are ones and their results are dropped); nbps and chunk stay those of the plan.  No atomics anywhere: every block
// stores pc matrices of partial sums with plain stores and k_slice_gram_fold adds the blocks of a (p, t) in ascending k.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.hpp"
#include "slice_plan.hpp"

namespace bcg {

// partials[((t * nbps + k) * pc + p) * m^2 + j * m + i], t < L_dir local, k < plan.walk.nbps, p < pc
// tab: [pc][3][plan.walk.ltab] phases of the LOCAL coordinates (device memory), or nullptr: no phase arithmetic (pc = 1)
void launch_slice_gram(hipStream_t s, int m, bool mfma, const LatticeDev& lat, int parity, int dir, const SliceGramPlan& plan, int pc,
                       const double2* a, const double2* b, const double2* tab, double2* partials);
// out[(p * L_global + origin + t) * m^2 + e] = sum_k partials[...] in ascending k, for the first np of the launch's pc momenta
void launch_slice_gram_fold(hipStream_t s, int m, int pc, int np, int L_local, int L_global, int nbps, int origin,
                            const double2* partials, double2* out);

}  // namespace bcg
