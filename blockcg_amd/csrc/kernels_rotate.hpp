// A basis times a small matrix, in place (gfx950): V <- V Q for a list V of fields whose widths sum to K <= 64 and a K x K
// complex matrix Q.  Kernels: kernels_rotate.hip; the entry point bcg_basis_rotate: capi_rotate.hip.
//
// Every output column mixes every input column, so a launch takes ALL K columns (the group walk of kernels_basis.hpp does
// not apply).  The rows are independent: a 16-row tile of all K columns is read, the K outputs are formed from that copy and
// stored over their inputs.  No workspace, no row read after it is written, no atomics.  Two forms:
//   MFMA     every width in {16, 32}: the basis is KB = K / 16 <= 4 blocks of 16 columns, each given by a pointer to its
//            first column and the row stride of its field (BasisBlocks of kernels_basis.hpp with mutable pointers).  A wave
//            holds the KB input tiles of its 16 rows in registers (16 per block) and the whole of Q sits in LDS in the
//            padded layout of MatLds (K x (2 K + 1) doubles: 66 KB at K = 64, two blocks per CU).
//   generic  every other width list: 16 rows of the K columns and Q in LDS, a thread owns a (row, output column) pair.
// The resource table: DESIGN.md section 8h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace bcg {

constexpr int kRotateMaxCols = 64;    // BCG_BASIS_ROTATE_MAX_COLUMNS of include/blockcg_hip.h
constexpr int kRotateMfmaBlocks = 4;  // kRotateMaxCols / 16
constexpr int kRotateBlocks = 1024;   // largest grid of either form (every block stages Q once)

struct RotateBlocks {  // MFMA form: block q is columns p[q][row * ld[q] + 0 .. 15]
  double2* p[kRotateMfmaBlocks];
  int ld[kRotateMfmaBlocks];
};
struct RotateFields {  // generic form: field k has w[k] columns, in the order of the list
  double2* v[kRotateMaxCols];
  unsigned char w[kRotateMaxCols];
  int nv;
  int K;
};

// Q: column-major K x K in device memory, element (i, j) at j * K + i
void launch_basis_rotate_mfma(hipStream_t s, int nblocks16, int64_t rows, const RotateBlocks& g, const double2* Q);
void launch_basis_rotate_generic(hipStream_t s, int64_t rows, const RotateFields& g, const double2* Q);

}  // namespace bcg
