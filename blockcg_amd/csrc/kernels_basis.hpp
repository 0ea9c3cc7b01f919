// Products between fields of unequal width (gfx950): C = V^dagger b (K x m) and y <- beta y + V C, V a list of fields whose
// widths sum to K, and the column copy between fields of different widths.  Kernels: kernels_basis.hip; the host walk over
// groups of basis fields: capi_basis.hip.
//
// A launch takes a GROUP of consecutive basis fields, so that b is read once (dot), or y read and written once (update),
// per group and not per field.  Two forms:
//   MFMA     m in {16, 32} and every width of the group in {16, 32}: the group is a few blocks of 16 columns
//            (basis_dot_mfma_blocks / basis_axpy_mfma_blocks), each given by a pointer to its first column and the row
//            stride of its field.
//   generic  every other combination of widths: at most kBasisGenericFields fields and kBasisGenericCols columns.
// The bounds are the largest at which the compiler's resource remarks still show two waves per SIMD and no scratch: the
// dot carries 16 registers per pair of 16-column blocks, the update the group's input tiles (16 registers per block) and
// K_g x (2m + 1) doubles of LDS.  The table: DESIGN.md section 8g.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace bcg {

constexpr int kBasisMfmaBlocks = 4;      // 64 columns of V per launch at the most
inline int basis_dot_mfma_blocks(int m) { return m == 16 ? 4 : 2; }
inline int basis_axpy_mfma_blocks(int m) { return m == 16 ? 4 : 3; }
constexpr int kBasisGenericFields = 8;
constexpr int kBasisGenericCols = 32;
constexpr int kBasisBlocks = 1024;       // largest grid of either form: its partials fit c->partials at K_g = 64, m = 32

struct BasisBlocks {  // MFMA form: block q is columns p[q][row * ld[q] + 0 .. 15]
  const double2* p[kBasisMfmaBlocks];
  int ld[kBasisMfmaBlocks];
};
struct BasisFields {  // generic form: field k has w[k] columns, the group's columns off[k] .. off[k] + w[k] - 1
  const double2* v[kBasisGenericFields];
  int w[kBasisGenericFields];
  int off[kBasisGenericFields];
  int nv;
  int K;  // columns of the group
};

inline bool basis_mfma_width(int w) { return w == 16 || w == 32; }

namespace {  // device helper of the generic form, shared by kernels_basis.hip and kernels_basis_slice*.hip

// the field that holds column i of a generic group: selects over the (few) fields, no indexed access to the argument
__device__ __forceinline__ const double2* basis_column(const BasisFields& g, int i, int* w, int* o) {
  const double2* p = g.v[0];
  *w = g.w[0];
  *o = 0;
#pragma unroll
  for (int k = 1; k < kBasisGenericFields; ++k)
    if (k < g.nv && i >= g.off[k]) {
      p = g.v[k];
      *w = g.w[k];
      *o = g.off[k];
    }
  return p;
}

}  // namespace

// Block partials of the group's K_g x m product: partials[block][j * K_g + i].  Returns the number of blocks.
int launch_basis_dot_mfma(hipStream_t s, int m, int nblocks16, int64_t rows, const BasisBlocks& g, const double2* b, double2* partials);
int launch_basis_dot_generic(hipStream_t s, int m, int64_t rows, const BasisFields& g, const double2* b, double2* partials);
// out[j * K + off + i] = sum over blocks, in ascending block order, of partials[block][j * K_g + i]
void launch_basis_fold(hipStream_t s, int Kg, int m, int nblocks, const double2* partials, double2* out, int K, int off);

// y <- beta y + sum_i V_i C(off + i, .): C column-major K x m in device memory; beta == 0 does not read y
void launch_basis_axpy_mfma(hipStream_t s, int m, int nblocks16, int64_t rows, double2* y, const BasisBlocks& g, const double2* C,
                            int K, int off, double beta);
void launch_basis_axpy_generic(hipStream_t s, int m, int64_t rows, double2* y, const BasisFields& g, const double2* C, int K, int off,
                               double beta);

// dst[row][dst_first + k] = src[row][src_first + k], k < n
void launch_copy_columns(hipStream_t s, int64_t rows, double2* dst, int md, int dst_first, const double2* src, int ms, int src_first,
                         int n);

}  // namespace bcg
