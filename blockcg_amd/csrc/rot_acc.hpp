// The product of the in-place rotations (kernels_rotate.hip, kernels_basis_slice_rotate.hip): one 16-column input tile
// times one 16 x 16 block of a K x K matrix staged in LDS in MatLds's padded layout with the rows of the WHOLE matrix.
// Anonymous namespace: each translation unit has its own copy, as with mfma_common.hpp.
#pragma once
#include "mfma_common.hpp"

namespace bcg {

namespace {

// rect_acc<16> of kernels_basis.hip for a matrix whose rows are LD doubles apart: A += in * C, C the 16 x 16 block at Ml
// (Ml[j_in * LD + 2 j_out + comp]).  A.a[0] is the re block of the output tile, A.a[1] its im block.
template <int LD>
__device__ __forceinline__ void rot_acc(Acc<16>& A, const Tile<16>& in, const double* Ml, int lane) {
  const int kq = lane >> 4;
  const int ar = lane & 15;
  const double* base = Ml + kq * LD + 2 * ar;
#pragma unroll
  for (int s_i = 0; s_i < 4; ++s_i) {
    const double a_same = base[s_i * 4 * LD + 0];   // Re C(j_i, j_o)
    const double a_cross = base[s_i * 4 * LD + 1];  // Im C(j_i, j_o)
    A.a[0] = mfma(a_same, in.v[s_i].x, A.a[0]);
    A.a[0] = mfma_nega(a_cross, in.v[s_i].y, A.a[0]);
    A.a[1] = mfma(a_cross, in.v[s_i].x, A.a[1]);
    A.a[1] = mfma(a_same, in.v[s_i].y, A.a[1]);
  }
}

}  // namespace
}  // namespace bcg
