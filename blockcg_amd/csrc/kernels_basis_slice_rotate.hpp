// A basis times one small matrix per slice, in place (kernels_basis_slice_rotate.hip; include/blockcg_hip.h:
// bcg_basis_slice_rotate):
//
//   V_j(x, c) <- sum_i V_i(x, c) Q_s(i, j)     on the LOCAL sites of the listed slices; no other site is read or written,
//
// V a list of fields whose widths sum to K <= 64, Q_s one K x K matrix per listed slice.  It is bcg_basis_rotate
// (kernels_rotate.hpp) on the slice walk of the per-slice calls (slice_walk.hpp, described in slice_plan.hpp): every
// output column mixes every input column, so a launch takes ALL K columns; the rows are independent, a 16-row step of all K
// columns is read, the K outputs are formed from that copy and stored over their inputs.  No workspace, no row read after
// it is written, no atomics.  Two forms:
//   MFMA     every width in {16, 32}: KB = K / 16 <= 4 blocks of 16 columns (RotateBlocks).  Block (s, k) stages Q_s whole
//            in LDS (MatLds's padded layout, K x (2 K + 1) doubles: 66 KB at K = 64, two blocks per CU) and walks chunk k
//            of slice s 16 rows per wave step with the per-lane row cursor of k_basis_slice_axpy_mfma: lane l owns row
//            l & 15 of the step (a step may straddle sites and runs) and the columns (l >> 4) + 4 c of every block.
//   generic  every other width list: 16 rows of the K columns and Q_s in LDS, a thread owns a (row, output column) pair
//            (k_basis_rotate_generic on the same walk); Q_s and the column table are staged once per block.
// Rows the half-field walk along direction 0 skips (the other parity's sites) are neither loaded nor stored.
//
// The launch plan is basis_slice_axpy_plan (slice_plan.hpp): a function of (shape, parity, dir, local listed slices) only;
// the grid is slices x blocks per slice and nothing is reduced, so no value depends on it.  The resource table: DESIGN.md
// section 8k.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.hpp"
#include "kernels_rotate.hpp"
#include "slice_plan.hpp"

namespace bcg {

// list[2 s] = local slice, list[2 s + 1] = index of its matrix in Q, s < n_slices (device memory);
// Q[(index * K + j) * K + i]: column-major K x K blocks (device memory).
void launch_basis_slice_rotate_mfma(hipStream_t s, int nblocks16, const LatticeDev& lat, int parity, int dir, const SliceWalk& plan,
                                    int n_slices, const int* list, const RotateBlocks& v, const double2* Q);
void launch_basis_slice_rotate_generic(hipStream_t s, const LatticeDev& lat, int parity, int dir, const SliceWalk& plan, int n_slices,
                                       const int* list, const RotateFields& v, const double2* Q);

}  // namespace bcg
