// V <- V Q in place (gfx950): the two forms and their layout are in kernels_rotate.hpp.  MFMA form: v_mfma_f64_16x16x4_f64
// in the operand ownership of Tile / rect_acc (kernels_basis.hip), restated here for a row stride of the whole K x K
// matrix; four real products per complex one.  Generic form: lane = (row, output column) with the rows of a tile and Q in
// LDS.  Plain stores, no atomics; 64-bit wherever an element offset is formed.
#include "complex_ops.hpp"
#include "kernels_rotate.hpp"
#include "mfma_common.hpp"
#include "rot_acc.hpp"

namespace bcg {

namespace {

// ---------------------------------------------------------------------------------------------
// MFMA form.  Wave w of a block takes the tiles (16 rows) w, w + 4 NB, ...; lane l owns row l & 15 and the columns
// (l >> 4) + 4 s of every 16-column block.  All KB input tiles are in registers before the first store of the tile.
// ---------------------------------------------------------------------------------------------
template <int KB>
__global__ void __launch_bounds__(256) k_basis_rotate_mfma(int64_t rows, RotateBlocks g, const double2* __restrict__ Q) {
  constexpr int NW = 4, K = 16 * KB, LD = 2 * K + 1;
  extern __shared__ __attribute__((aligned(16))) double smem[];  // K * LD doubles
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int e = tid; e < K * K; e += 256) {
    const int j = e / K, i = e - j * K;
    const double2 v = Q[e];
    smem[i * LD + 2 * j] = v.x;
    smem[i * LD + 2 * j + 1] = v.y;
  }
  __syncthreads();
  const int r = lane & 15, kq = lane >> 4;
  const int64_t ntiles = (rows + 15) / 16;
  for (int64_t tile = static_cast<int64_t>(blockIdx.x) * NW + wave; tile < ntiles; tile += static_cast<int64_t>(gridDim.x) * NW) {
    const int64_t row = tile * 16 + r;
    const bool ok = row < rows;
    Tile<16> tv[KB];
#pragma unroll
    for (int q = 0; q < KB; ++q) {
      const double2* p = g.p[q] + row * g.ld[q] + kq;
#pragma unroll
      for (int s = 0; s < 4; ++s) tv[q].v[s] = ok ? p[4 * s] : make_double2(0.0, 0.0);
    }
#pragma unroll
    for (int jb = 0; jb < KB; ++jb) {
      // KB >= 3: the 2 K^2 / 64 coefficients of a lane are loop-invariant and the compiler would keep them all in registers
      // (KB = 4: 128 of them, 256 + 108 registers, one wave per SIMD); re-read per output block they cost 8 KB
      if constexpr (KB >= 3) asm volatile("" ::: "memory");
      Acc<16> A;
      acc_zero<16>(A);
#pragma unroll
      for (int q = 0; q < KB; ++q) rot_acc<LD>(A, tv[q], smem + 16 * q * LD + 32 * jb, lane);
      Tile<16> to;
      tile_from_acc<16>(to, A);
      double2* p = g.p[jb] + row * g.ld[jb] + kq;
      if (ok) {
#pragma unroll
        for (int s = 0; s < 4; ++s) p[4 * s] = to.v[s];
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Generic form: TR rows of the K columns in LDS; thread p + 256 q owns the pair (row, j) = (p / K, p % K).  The column
// table (first element and row stride of every column) is built once per block by selects over the fields, no indexed
// access to the argument.
// ---------------------------------------------------------------------------------------------
constexpr int kRotateTR = 16;

__global__ void __launch_bounds__(256) k_basis_rotate_generic(int64_t rows, RotateFields g, const double2* __restrict__ Q) {
  constexpr int TR = kRotateTR;
  extern __shared__ __attribute__((aligned(16))) double2 sm[];  // Qs[i * K + j] = Q(i, j) | xs[TR * K]
  __shared__ double2* colp[kRotateMaxCols];
  __shared__ int colw[kRotateMaxCols];
  const int tid = threadIdx.x;
  const int K = g.K;
  double2* const Qs = sm;
  double2* const xs = sm + K * K;
  for (int e = tid; e < K * K; e += 256) {
    const int j = e / K, i = e - j * K;
    Qs[i * K + j] = Q[e];
  }
  if (tid < K) {
    double2* p = g.v[0];
    int w = g.w[0], o = 0, off = 0;
#pragma unroll
    for (int k = 0; k < kRotateMaxCols; ++k) {
      if (k < g.nv && tid >= off) {
        p = g.v[k];
        w = g.w[k];
        o = off;
      }
      off += k < g.nv ? g.w[k] : 0;
    }
    colp[tid] = p + (tid - o);
    colw[tid] = w;
  }
  const int64_t ntiles = (rows + TR - 1) / TR;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t row0 = tile * TR;
    __syncthreads();  // the table (first tile); the products of the tile before have left xs
    for (int x = tid; x < TR * K; x += 256) {
      const int rr = x / K, i = x - rr * K;
      const int64_t row = row0 + rr;
      xs[x] = row < rows ? colp[i][row * colw[i]] : make_double2(0.0, 0.0);
    }
    __syncthreads();  // every load of the tile is done: the stores below overwrite what was read
    for (int x = tid; x < TR * K; x += 256) {
      const int rr = x / K, j = x - rr * K;
      const int64_t row = row0 + rr;
      if (row < rows) {
        double2 acc = make_double2(0.0, 0.0);
        for (int i = 0; i < K; ++i) cfma(acc, xs[rr * K + i], Qs[i * K + j]);
        colp[j][row * colw[j]] = acc;
      }
    }
  }
}

template <int KB>
void rotate_mfma_one(hipStream_t s, int grid, int64_t rows, const RotateBlocks& g, const double2* Q) {
  const size_t lds = static_cast<size_t>(16 * KB) * (32 * KB + 1) * sizeof(double);
  allow_lds(k_basis_rotate_mfma<KB>, lds);
  hipLaunchKernelGGL((k_basis_rotate_mfma<KB>), dim3(grid), dim3(256), lds, s, rows, g, Q);
}

}  // namespace

void launch_basis_rotate_mfma(hipStream_t s, int nblocks16, int64_t rows, const RotateBlocks& g, const double2* Q) {
  const int grid = grid_tiles((rows + 15) / 16, 4, kRotateBlocks);
  switch (nblocks16) {
    case 1: rotate_mfma_one<1>(s, grid, rows, g, Q); break;
    case 2: rotate_mfma_one<2>(s, grid, rows, g, Q); break;
    case 3: rotate_mfma_one<3>(s, grid, rows, g, Q); break;
    default: rotate_mfma_one<4>(s, grid, rows, g, Q); break;
  }
}

void launch_basis_rotate_generic(hipStream_t s, int64_t rows, const RotateFields& g, const double2* Q) {
  const int grid = grid_tiles((rows + kRotateTR - 1) / kRotateTR, 1, kRotateBlocks);
  const size_t lds = (static_cast<size_t>(g.K) * g.K + static_cast<size_t>(kRotateTR) * g.K) * sizeof(double2);
  allow_lds(k_basis_rotate_generic, lds);
  hipLaunchKernelGGL(k_basis_rotate_generic, dim3(grid), dim3(256), lds, s, rows, g, Q);
}

}  // namespace bcg
