// Products between fields of unequal width (gfx950): the group walk, the two forms and their bounds are in
// kernels_basis.hpp.  MFMA form: v_mfma_f64_16x16x4_f64 in the operand ownership of gram_step (dot) and of Tile / rmul_acc
// (update) of mfma_common.hpp, restated here for (16 k, m) blocks instead of square ones; four real products per complex
// one.  Generic form: lane = (row, output column) with the rows of a tile staged in LDS.  Plain stores, no atomics; 64-bit
// wherever an element offset is formed.
#include "complex_ops.hpp"
#include "kernels_basis.hpp"
#include "mfma_common.hpp"

namespace bcg {

namespace {

// ---------------------------------------------------------------------------------------------
// Dot, MFMA form.  Wave w of a block takes the quads (4 rows) w, w + 4 NW, ...; lane l owns row 4 q + (l >> 4) and column
// l & 15 of every 16-column block of V and of b.  Accumulators: KB x (M / 16) pairs of 16 x 16 blocks, re and im.
// ---------------------------------------------------------------------------------------------
template <int M, int KB>
__global__ void __launch_bounds__(256) k_basis_dot_mfma(int64_t rows, BasisBlocks g, const double2* __restrict__ b,
                                                        double2* __restrict__ partials) {
  constexpr int NW = 4, JB = M / 16, U = 2, KG = 16 * KB;
  __shared__ __attribute__((aligned(16))) double red[NW * 8 * 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15;
  d4 re[KB * JB], im[KB * JB];
#pragma unroll
  for (int q = 0; q < KB * JB; ++q) {
    re[q] = d4{0.0, 0.0, 0.0, 0.0};
    im[q] = d4{0.0, 0.0, 0.0, 0.0};
  }
  const int64_t nquads = (rows + 3) / 4;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * NW;
  for (int64_t qd = static_cast<int64_t>(blockIdx.x) * NW + wave; qd < nquads; qd += U * stride) {
    double2 av[U][KB], bv[U][JB];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t row = (qd + u * stride) * 4 + (lane >> 4);
      const bool ok = row < rows;  // also false for a quad past the last
#pragma unroll
      for (int q = 0; q < KB; ++q) av[u][q] = ok ? g.p[q][row * g.ld[q] + col] : make_double2(0.0, 0.0);
#pragma unroll
      for (int jb = 0; jb < JB; ++jb) bv[u][jb] = ok ? b[row * M + 16 * jb + col] : make_double2(0.0, 0.0);
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int q = 0; q < KB; ++q)
#pragma unroll
        for (int jb = 0; jb < JB; ++jb) {  // conj(a) b: gram_step's four products
          const int t = q * JB + jb;
          re[t] = mfma(av[u][q].x, bv[u][jb].x, re[t]);
          re[t] = mfma(av[u][q].y, bv[u][jb].y, re[t]);
          im[t] = mfma(av[u][q].x, bv[u][jb].y, im[t]);
          im[t] = mfma_nega(av[u][q].y, bv[u][jb].x, im[t]);
        }
  }
  // the per-wave fragments summed in wave order, one 16 x 16 block at a time through red
  double2* const dst = partials + static_cast<int64_t>(blockIdx.x) * (KG * M);
#pragma unroll
  for (int t = 0; t < KB * JB; ++t) {
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      red[(wave * 8 + r) * 64 + lane] = re[t][r];
      red[(wave * 8 + 4 + r) * 64 + lane] = im[t][r];
    }
    __syncthreads();
    {
      const int l = tid & 63, r = tid >> 6;  // 256 threads: one element each
      double sr = 0.0, si = 0.0;
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        sr += red[(w * 8 + r) * 64 + l];
        si += red[(w * 8 + 4 + r) * 64 + l];
      }
      const int i = 16 * (t / JB) + (l >> 4) + 4 * r, j = 16 * (t % JB) + (l & 15);
      dst[j * KG + i] = make_double2(sr, si);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Dot, generic form: TR rows of the group's columns and of b in LDS; thread p + 256 q owns the pair (i, j) = (p % K_g, p / K_g).
// ---------------------------------------------------------------------------------------------
constexpr int kBasisTR = 16;

__global__ void __launch_bounds__(256) k_basis_dot_generic(int m, int64_t rows, BasisFields g, const double2* __restrict__ b,
                                                           double2* __restrict__ partials) {
  constexpr int TR = kBasisTR, NPT = kBasisGenericCols * 32 / 256;
  __shared__ double2 As[TR * kBasisGenericCols];
  __shared__ double2 Bs[TR * 32];
  const int tid = threadIdx.x;
  const int Kg = g.K, P = Kg * m;
  double2 acc[NPT];
#pragma unroll
  for (int q = 0; q < NPT; ++q) acc[q] = make_double2(0.0, 0.0);
  const int64_t ntiles = (rows + TR - 1) / TR;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t row0 = tile * TR;
    __syncthreads();
    for (int x = tid; x < TR * Kg; x += 256) {
      const int r = x / Kg, i = x - r * Kg;
      const int64_t row = row0 + r;
      int w, o;
      const double2* p = basis_column(g, i, &w, &o);
      As[x] = row < rows ? p[row * w + (i - o)] : make_double2(0.0, 0.0);
    }
    for (int x = tid; x < TR * m; x += 256) {
      const int r = x / m, j = x - r * m;
      const int64_t row = row0 + r;
      Bs[x] = row < rows ? b[row * m + j] : make_double2(0.0, 0.0);
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NPT; ++q) {
      const int p = tid + 256 * q;
      if (p < P) {
        const int j = p / Kg, i = p - j * Kg;
        for (int r = 0; r < TR; ++r) cfma_conj(acc[q], As[r * Kg + i], Bs[r * m + j]);
      }
    }
  }
#pragma unroll
  for (int q = 0; q < NPT; ++q) {
    const int p = tid + 256 * q;
    if (p < P) partials[static_cast<int64_t>(blockIdx.x) * P + p] = acc[q];
  }
}

__global__ void __launch_bounds__(256) k_basis_fold(int Kg, int m, int nblocks, const double2* __restrict__ partials,
                                                    double2* __restrict__ out, int K, int off) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  const int P = Kg * m;
  if (v >= P) return;
  double sr = 0.0, si = 0.0;
  for (int k = 0; k < nblocks; ++k) {
    const double2 t = partials[static_cast<int64_t>(k) * P + v];
    sr += t.x;
    si += t.y;
  }
  const int j = v / Kg, i = v - j * Kg;
  out[static_cast<int64_t>(j) * K + off + i] = make_double2(sr, si);
}

// ---------------------------------------------------------------------------------------------
// Update, MFMA form.  rect_acc (mfma_common.hpp): rmul_acc's four-product chain for a 16-column input tile and an M-column
// output; the rows of C that belong to the block are staged at Ml[j_in * LD + 2 j_out + comp], LD = 2 M + 1.
// ---------------------------------------------------------------------------------------------
template <int M, int KB>
__global__ void __launch_bounds__(256) k_basis_axpy_mfma(int64_t rows, double2* __restrict__ y, BasisBlocks g,
                                                         const double2* __restrict__ C, int K, int off, double beta) {
  constexpr int NW = 4, KG = 16 * KB, LD = MatLds<M>::LD;
  extern __shared__ __attribute__((aligned(16))) double smem[];  // KG * LD doubles
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int e = tid; e < KG * M; e += 256) {
    const int j = e / KG, i = e - j * KG;
    const double2 v = C[static_cast<int64_t>(j) * K + off + i];
    smem[i * LD + 2 * j] = v.x;
    smem[i * LD + 2 * j + 1] = v.y;
  }
  __syncthreads();
  const bool rd = beta != 0.0;
  const int r = lane & 15, kq = lane >> 4;
  const int64_t ntiles = (rows + 15) / 16;
  for (int64_t tile = static_cast<int64_t>(blockIdx.x) * NW + wave; tile < ntiles; tile += static_cast<int64_t>(gridDim.x) * NW) {
    const int64_t row = tile * 16 + r;
    const bool ok = row < rows;
    Tile<M> ty;
    tile_load<M>(ty, y, row, kq, ok && rd);
    Tile<16> tv[KB];
#pragma unroll
    for (int q = 0; q < KB; ++q) {
      const double2* p = g.p[q] + row * g.ld[q] + kq;
#pragma unroll
      for (int s = 0; s < 4; ++s) tv[q].v[s] = ok ? p[4 * s] : make_double2(0.0, 0.0);
    }
    Acc<M> A;
    if (rd) {
#pragma unroll
      for (int s = 0; s < M / 4; ++s) ty.v[s] = make_double2(beta * ty.v[s].x, beta * ty.v[s].y);
      acc_from_tile<M>(A, ty);
    } else {
      acc_zero<M>(A);
    }
#pragma unroll
    for (int q = 0; q < KB; ++q) rect_acc<M>(A, tv[q], smem + 16 * q * LD, lane);
    tile_from_acc<M>(ty, A);
    tile_store<M>(ty, y, row, kq, ok);
  }
}

// ---------------------------------------------------------------------------------------------
// Update, generic form: thread (rl, j) computes y[row][j]; R rows of the group's columns and its rows of C sit in LDS.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_basis_axpy_generic(int m, int64_t rows, double2* __restrict__ y, BasisFields g,
                                                            const double2* __restrict__ C, int K, int off, double beta) {
  constexpr int RMAX = 32;
  __shared__ double2 Ct[kBasisGenericCols * 32];  // Ct[i * m + j] = C(off + i, j)
  __shared__ double2 xs[RMAX * kBasisGenericCols];
  const int tid = threadIdx.x;
  const int Kg = g.K;
  for (int e = tid; e < Kg * m; e += 256) {
    const int i = e / m, j = e - i * m;
    Ct[e] = C[static_cast<int64_t>(j) * K + off + i];
  }
  const int R = 256 / m < RMAX ? 256 / m : RMAX;
  const int rl = tid / m, j = tid - rl * m;
  const bool rd = beta != 0.0;
  const int64_t ntiles = (rows + R - 1) / R;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t row0 = tile * R;
    __syncthreads();
    for (int x = tid; x < R * Kg; x += 256) {
      const int rr = x / Kg, i = x - rr * Kg;
      const int64_t row = row0 + rr;
      int w, o;
      const double2* p = basis_column(g, i, &w, &o);
      xs[x] = row < rows ? p[row * w + (i - o)] : make_double2(0.0, 0.0);
    }
    __syncthreads();
    const int64_t row = row0 + rl;
    if (rl < R && row < rows) {
      double2 acc = make_double2(0.0, 0.0);
      if (rd) {
        const double2 yv = y[row * m + j];
        acc = make_double2(beta * yv.x, beta * yv.y);
      }
      for (int i = 0; i < Kg; ++i) cfma(acc, xs[rl * Kg + i], Ct[i * m + j]);
      y[row * m + j] = acc;
    }
  }
}

__global__ void __launch_bounds__(256) k_copy_columns(int64_t rows, double2* __restrict__ dst, int md, int dst_first,
                                                      const double2* __restrict__ src, int ms, int src_first, int n) {
  const int64_t total = rows * n;
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; e < total; e += static_cast<int64_t>(gridDim.x) * 256) {
    const int64_t row = e / n;
    const int k = static_cast<int>(e - row * n);
    dst[row * md + dst_first + k] = src[row * ms + src_first + k];
  }
}

template <int M>
void dot_mfma(hipStream_t s, int kb, int grid, int64_t rows, const BasisBlocks& g, const double2* b, double2* partials) {
  switch (kb) {
    case 1: hipLaunchKernelGGL((k_basis_dot_mfma<M, 1>), dim3(grid), dim3(256), 0, s, rows, g, b, partials); break;
    case 2: hipLaunchKernelGGL((k_basis_dot_mfma<M, 2>), dim3(grid), dim3(256), 0, s, rows, g, b, partials); break;
    default:  // 3 and 4 blocks: m = 16 only (basis_dot_mfma_blocks)
      if constexpr (M == 16) {
        if (kb == 3) hipLaunchKernelGGL((k_basis_dot_mfma<M, 3>), dim3(grid), dim3(256), 0, s, rows, g, b, partials);
        else hipLaunchKernelGGL((k_basis_dot_mfma<M, 4>), dim3(grid), dim3(256), 0, s, rows, g, b, partials);
      }
      break;
  }
}

template <int M, int KB>
void axpy_mfma_one(hipStream_t s, int grid, int64_t rows, double2* y, const BasisBlocks& g, const double2* C, int K, int off,
                   double beta) {
  const size_t lds = static_cast<size_t>(16 * KB) * MatLds<M>::LD * sizeof(double);
  allow_lds(k_basis_axpy_mfma<M, KB>, lds);
  hipLaunchKernelGGL((k_basis_axpy_mfma<M, KB>), dim3(grid), dim3(256), lds, s, rows, y, g, C, K, off, beta);
}
template <int M>
void axpy_mfma(hipStream_t s, int kb, int grid, int64_t rows, double2* y, const BasisBlocks& g, const double2* C, int K, int off,
               double beta) {
  switch (kb) {
    case 1: axpy_mfma_one<M, 1>(s, grid, rows, y, g, C, K, off, beta); break;
    case 2: axpy_mfma_one<M, 2>(s, grid, rows, y, g, C, K, off, beta); break;
    case 3: axpy_mfma_one<M, 3>(s, grid, rows, y, g, C, K, off, beta); break;
    default:  // 4 blocks: m = 16 only (basis_axpy_mfma_blocks)
      if constexpr (M == 16) axpy_mfma_one<M, 4>(s, grid, rows, y, g, C, K, off, beta);
      break;
  }
}

}  // namespace

int launch_basis_dot_mfma(hipStream_t s, int m, int nblocks16, int64_t rows, const BasisBlocks& g, const double2* b, double2* partials) {
  const int grid = grid_tiles((rows + 3) / 4, 4, kBasisBlocks);
  if (m == 16) dot_mfma<16>(s, nblocks16, grid, rows, g, b, partials);
  else dot_mfma<32>(s, nblocks16, grid, rows, g, b, partials);
  return grid;
}

int launch_basis_dot_generic(hipStream_t s, int m, int64_t rows, const BasisFields& g, const double2* b, double2* partials) {
  const int grid = grid_tiles((rows + kBasisTR - 1) / kBasisTR, 1, kBasisBlocks);
  hipLaunchKernelGGL(k_basis_dot_generic, dim3(grid), dim3(256), 0, s, m, rows, g, b, partials);
  return grid;
}

void launch_basis_fold(hipStream_t s, int Kg, int m, int nblocks, const double2* partials, double2* out, int K, int off) {
  hipLaunchKernelGGL(k_basis_fold, dim3((Kg * m + 255) / 256), dim3(256), 0, s, Kg, m, nblocks, partials, out, K, off);
}

void launch_basis_axpy_mfma(hipStream_t s, int m, int nblocks16, int64_t rows, double2* y, const BasisBlocks& g, const double2* C,
                            int K, int off, double beta) {
  const int grid = grid_tiles((rows + 15) / 16, 4, kBasisBlocks);
  if (m == 16) axpy_mfma<16>(s, nblocks16, grid, rows, y, g, C, K, off, beta);
  else axpy_mfma<32>(s, nblocks16, grid, rows, y, g, C, K, off, beta);
}

void launch_basis_axpy_generic(hipStream_t s, int m, int64_t rows, double2* y, const BasisFields& g, const double2* C, int K, int off,
                               double beta) {
  const int R = 256 / m < 32 ? 256 / m : 32;
  const int grid = grid_tiles((rows + R - 1) / R, 1, 4 * kBasisBlocks);
  hipLaunchKernelGGL(k_basis_axpy_generic, dim3(grid), dim3(256), 0, s, m, rows, y, g, C, K, off, beta);
}

void launch_copy_columns(hipStream_t s, int64_t rows, double2* dst, int md, int dst_first, const double2* src, int ms, int src_first,
                         int n) {
  const int grid = grid_tiles(rows * n, 256, 4 * kBasisBlocks);
  hipLaunchKernelGGL(k_copy_columns, dim3(grid), dim3(256), 0, s, rows, dst, md, dst_first, src, ms, src_first, n);
}

}  // namespace bcg
