// Per-slice products with a basis of another width (kernels_basis_slice.hip; include/blockcg_hip.h: bcg_basis_slice_dot):
//
//   tau_p(t)(i, j) = sum_{x : x_dir = t} w_p(x) sum_c conj(V_i[x, c]) b[x, c, j]       over the LOCAL sites,
//
// V a list of fields whose widths sum to K, b of width m.  The rows of a slice are walked as the per-slice Gram kernels walk
// them (slice_walk.hpp, described in slice_plan.hpp), the operands of a launch are a GROUP of basis columns as in
// the whole-lattice products (kernels_basis.hpp).  A call is a set of launches, each (group of K_g basis columns) x (pc
// momenta); a launch reads 48 (K_g + m) bytes per site, a call ceil(K / K_g) ceil(P / pc) 48 (K_g + m).
//
// Two forms:
//   MFMA     m in {16, 32}, widths in {16, 32}, bcg_force_generic not set.  A group is a run of kb blocks of 16 columns
//            (BasisBlocks) out of the blocks of consecutive MFMA fields: it may begin or end in the middle of a 32-wide
//            field.  kb * pc * (m / 16) accumulator sets of 16 registers are live, and the bound is
//            kb * pc * (m / 16) <= 4 (64 accumulator registers, two waves per SIMD; the table: DESIGN.md section 8i).
//            Instantiated pc: 1, 2, 4 at m = 16; 1, 2 at m = 32.
//   generic  every other field: consecutive generic fields up to kBasisGenericFields fields and `cols` columns
//            (BasisFields), a field alone where it is wider than `cols`.  Instantiated pc: 1, 2.
// A run of fields of one form ends where the form changes; one call may use both.
//
// The launch plan (basis_slice_plan, slice_plan.hpp) is a function of (shape, widths, m, parity, dir, n_mom) and of the scratch it is given:
//   pc     per form, the largest instantiated count <= max(n_mom, 1): momenta first, because a momentum taken in another
//          launch costs a pass over V and b, a column taken in another launch a pass over b only
//   group  MFMA: kb = 4 / (pc * (m / 16)) blocks; generic: cols = kBasisGenericCols.  Without momenta this is the largest
//          group with pc = 1: V = 2 x 32 columns at m = 16 is one launch of 64 columns
//   blocks one grid for every launch of the call, from the launch with the most entries per block, E = max pc * K_g * m:
//          budget = min(2048, entries left of the scratch's half after the phase tables / E) -- 1024 blocks, or one fewer,
//          at E = 1024 --; blocks per slice wanted = budget / L_local; the blocks per slice and the chunk follow from
//          that as in every per-slice plan (slice_plan.hpp)
//   shrink while the budget is below max(L_local, min(256, L_local * rows_of_a_slice / 64)) blocks -- one block per slice
//          at the least, one per compute unit where the slices have the rows -- the form that holds E gives way: first its
//          group (MFMA: one block fewer; generic: cols = half the group's columns, while it has a second field), then
//          its pc (halved).
//          When neither form can give way the grid is what the budget allows; fewer than L_local blocks: no plan.
// A group's last launch may carry fewer momenta (the smallest instantiated count that holds them; the tables of the unused
// ones are ones and their results are dropped); groups, nbps and chunk stay those of the plan.  No atomics: every block
// stores pc matrices K_g x m of partial sums with plain stores and k_basis_slice_fold adds the blocks of a (p, t) in
// ascending k, straight into the call's full result.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.hpp"
#include "kernels_basis.hpp"
#include "slice_plan.hpp"

namespace bcg {

// partials[((t * nbps + k) * pc + p) * K_g m + j * K_g + i], t < L_dir local, k < plan.walk.nbps, p < pc
// tab: [pc][3][plan.ltab] phases of the LOCAL coordinates (device memory), or nullptr: no phase arithmetic (pc = 1)
void launch_basis_slice_dot_mfma(hipStream_t s, int m, int kb, const LatticeDev& lat, int parity, int dir, const BasisSlicePlan& plan,
                                 int pc, const BasisBlocks& v, const double2* b, const double2* tab, double2* partials);
void launch_basis_slice_dot_generic(hipStream_t s, int m, const LatticeDev& lat, int parity, int dir, const BasisSlicePlan& plan,
                                    int pc, const BasisFields& v, const double2* b, const double2* tab, double2* partials);
// out[(((p0 + p) * L_global + origin + t) * m + j) * K + off + i] = sum_k partials[...] in ascending k, for the first np of
// the launch's pc momenta
void launch_basis_slice_fold(hipStream_t s, int Kg, int m, int pc, int np, int L_local, int L_global, int nbps, int origin, int K,
                             int off, int p0, const double2* partials, double2* out);

}  // namespace bcg
