// A basis put onto time slices (kernels_basis_slice_axpy.hip; include/blockcg_hip.h: bcg_basis_slice_axpy), the adjoint of
// the per-slice products of kernels_basis_slice.hpp:
//
//   y_j(x, c) <- beta y_j(x, c) + w(x) sum_i V_i(x, c) C_s(i, j)     on the LOCAL sites of the listed slices,
//   y_j(x, c) <- beta y_j(x, c)                                      on the sites of every other slice,
//
// V a list of fields whose widths sum to K, y of width m, C_s one K x m matrix per listed slice.  The rows of a slice are
// walked as the per-slice Gram kernels walk them (slice_walk.hpp, described in slice_plan.hpp); the operands of a
// launch are a GROUP of basis fields exactly as in bcg_basis_axpy (kernels_basis.hpp: basis_axpy_mfma_blocks blocks of 16
// columns in the MFMA form, kBasisGenericFields fields and kBasisGenericCols columns in the generic one).  The first
// group's launch carries beta, the later ones run at beta = 1.  A launch reads 48 (K_g + m) bytes per listed site and
// writes 48 m (beta == 0: reads 48 K_g).
//
// Two forms, chosen per group as in bcg_basis_axpy:
//   MFMA     m in {16, 32}, every width of the group in {16, 32}, bcg_force_generic not set.  Block (s, k) stages its
//            group's rows of C_s in LDS (K_g x (2 m + 1) doubles, MatLds<M>'s padded layout) and walks chunk k of slice s
//            16 rows per wave step: lane l owns row l & 15 of the step (its own cursor: a step may straddle sites and
//            runs) and the columns (l >> 4) + 4 s of every tile.  A = V C_s is formed from zero by rect_acc, multiplied
//            by w(x) in the phase instantiation, beta y added, stored.  The table: DESIGN.md section 8j.
//   generic  R = min(256 / m, 32) rows of the group's columns staged in LDS, thread (row, j) computes y[row][j]; C_s is
//            staged once per block.
// Rows the half-field walk along direction 0 skips (the other parity's sites) are neither read nor written.
//
// The slices that are not listed are a second kernel on the same walk (k_slice_scale: y <- beta y, or zeros at beta == 0;
// not launched at beta == 1), so that the listed-slice kernels carry no branch and no register for them.
//
// The launch plan (basis_slice_axpy_plan, slice_plan.hpp) is a function of (shape, parity, dir, number of slices of the
// launch) only -- widths and m choose the form and the groups, not the grid -- and nothing but the walk (SliceWalk):
//   blocks per slice wanted = kBasisSliceAxpyBlocks / slices; the blocks per slice and the chunk follow from that as in
//   every per-slice plan (slice_plan.hpp)
// The grid is slices x blocks per slice, so any number of slices is covered (one block per slice at the least); nothing is
// reduced, so no value depends on the plan.  No plan: a slice of 2^30 rows or more.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.hpp"
#include "kernels_basis.hpp"
#include "slice_plan.hpp"

namespace bcg {

// list[2 s] = local slice, list[2 s + 1] = index of its matrix in C, s < n_slices (device memory);
// C[(index * m + j) * K + i] column-major K x m blocks; the group's columns are off .. off + K_g - 1.
// tab: [3][plan.ltab] w of the LOCAL coordinates (device memory), or nullptr: no phase arithmetic.
void launch_basis_slice_axpy_mfma(hipStream_t s, int m, int nblocks16, const LatticeDev& lat, int parity, int dir,
                                  const SliceWalk& plan, int n_slices, const int* list, double2* y, const BasisBlocks& v,
                                  const double2* C, int K, int off, const double2* tab, double beta);
void launch_basis_slice_axpy_generic(hipStream_t s, int m, const LatticeDev& lat, int parity, int dir, const SliceWalk& plan,
                                     int n_slices, const int* list, double2* y, const BasisFields& v, const double2* C, int K, int off,
                                     const double2* tab, double beta);
// y <- beta y (beta == 0: zeros, y is not read) on the slices slices[0 .. n_slices-1] (local, device memory)
void launch_slice_scale(hipStream_t s, int m, const LatticeDev& lat, int parity, int dir, const SliceWalk& plan, int n_slices,
                        const int* slices, double2* y, double beta);

}  // namespace bcg
