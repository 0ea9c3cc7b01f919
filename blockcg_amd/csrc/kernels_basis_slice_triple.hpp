// Baryon elementals of a basis, slice by slice (gfx950): for three lists of fields A, B, C (columns numbered through each
// list, K_a, K_b, K_c <= 64 columns)
//   T_p(t; i, j, k) = sum_{x: x_dir = t} w_p(x) sum_{abc} eps_abc A_i(x,a) B_j(x,b) C_k(x,c)
//                   = sum_{(x,a)} D_ij(x,a) [w_p(x) C_k(x,a)],   D_ij(x,a) = (A_i(x) x B_j(x))_a,
// the colour determinant of three columns summed over a slice with a momentum phase.  Kernels:
// kernels_basis_slice_triple.hip; the plan: slice_plan.hpp (basis_slice_triple_plan); the walk over the rows of a slice:
// slice_walk.hpp; the host side: capi_basis.hip (bcg_basis_slice_triple).
//
// A block owns one output TILE, edge columns of each list (edge^3 entries), on one chunk of one listed slice, and writes
// its partial of the tile; the fold sums the partials of a (momentum, slice, tile) in ascending block order into the
// result.  The columns of the lists are described by a table in device memory (TripleCol: where column c of list l begins
// and the row stride of its field), so that neither form depends on where one field ends and the next begins.
//   MFMA     every width of the three lists in {16, 32}, bcg_force_generic not set.  edge = 16.  Wave w holds the
//            accumulators of i = 4 w .. 4 w + 3, 16 j and 16 k (re and im: 64 registers).  A step is four sites: their 12
//            rows of the tile's 48 columns are staged in LDS (9 KB; the next step's rows are in flight in registers
//            meanwhile), C already multiplied by the phase.  Lane (j = l & 15, site = l >> 4) forms D_ij(x, a) from the
//            three colours of A_i and B_j on the VALU (14 flops) and feeds it to v_mfma_f64_16x16x4_f64 as the A operand of
//            k-step a, with w C_k(x, a) of lane (k = l & 15, site = l >> 4) as the B operand: four real products per
//            (i, k-step).  D never leaves the registers.
//   generic  every other width list.  edge = 8.  16 sites of the tile's 24 columns are staged in LDS at a time; thread
//            (i, j, k0) of the 256 forms D_ij once per site and owns the entries (i, j, k0) and (i, j, k0 + 4).
// Both forms: plain stores, no atomics, no scratch; a fixed order of addition (the rows of a chunk in walk order, then the
// blocks in ascending order), so a call gives the same bits every time.
//
// Profile keys.  "basis_slice_triple": bytes = 48 * 3 * edge per site, tile and launch (every block reads its 3 * edge
// columns of every row of its chunk once); executed flops = 24 * edge^3 per site, tile and launch (8 per complex
// multiply-add and (pair, k, colour); the cross product, about a ninth more, runs on the VALU and is not counted).  Tiles
// that identical lists do not launch are not counted, entries of a diagonal tile that the fold drops are.
// "basis_slice_triple_fold"; "basis_slice_triple_form_mfma" / "basis_slice_triple_form_generic" count the launches.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.hpp"
#include "slice_plan.hpp"

namespace bcg {

struct TripleCol {  // column c of a list: element (row, c) at p[row * ld]
  const double2* p;
  int64_t ld;
};

// What a launch reads besides the fields, all in device memory:
//   cols   [3][kTripleMaxColumns], entries beyond a list's width unused
//   tiles  (ta, tb, tc) per tile (plan.tiles)
//   list   (local slice, index of the slice in the result) per listed local slice, n_slices pairs
//   tab    the phase table of the launch's momentum, 3 x walk.ltab, or nullptr (w = 1)
// partials[(tile * n_slices * nbps + s * nbps + k) * edge^3 + (kk * edge + jj) * edge + ii]
void launch_basis_slice_triple(hipStream_t s, const LatticeDev& lat, int parity, int dir, const BasisSliceTriplePlan& plan, int n_slices,
                               const TripleCol* cols, int Ka, int Kb, int Kc, const int* tiles, const int* list, const double2* tab,
                               double2* partials);

// out[((((p * S + list[2 s + 1]) * Kc + k) * Kb + j) * Ka + i] = the sum over the blocks of (s, tile) in ascending order.
// Identical lists: only the entries i < j < k are written, each with its five signed images; every other entry of `out`
// keeps what it holds (the caller has zeroed the result).
void launch_basis_slice_triple_fold(hipStream_t s, const BasisSliceTriplePlan& plan, int n_slices, int Ka, int Kb, int Kc, int S, int p,
                                    const int* tiles, const int* list, const double2* partials, double2* out);

}  // namespace bcg
