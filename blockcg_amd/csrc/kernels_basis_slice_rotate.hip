// V <- V Q_s on the listed slices, in place (gfx950): the two forms and their layout are in kernels_basis_slice_rotate.hpp;
// the walk over the rows of a slice: slice_walk.hpp.  MFMA form: k_basis_rotate_mfma's tiles and product (rot_acc.hpp) under
// the row cursor of k_basis_slice_axpy_mfma.  Generic form: k_basis_rotate_generic's tile and thread mapping on the same
// walk.  Plain stores, no atomics; 64-bit wherever an element offset is formed.
#include "complex_ops.hpp"
#include "kernels_basis_slice_rotate.hpp"
#include "mfma_common.hpp"
#include "rot_acc.hpp"
#include "slice_walk.hpp"

namespace bcg {

namespace {

// ---------------------------------------------------------------------------------------------
// MFMA form.  Wave w of block (s, k) takes the steps w, w + 4, ... of 16 rows of the chunk; lane l owns row l & 15 of a step
// and derives its own row's address and validity.  All KB input tiles are in registers before the first store of the step.
// ---------------------------------------------------------------------------------------------
template <int KB>
__global__ void __launch_bounds__(256) k_basis_slice_rotate_mfma(SGGeom g, const int* __restrict__ list, RotateBlocks v,
                                                                 const double2* __restrict__ Q) {
  constexpr int NW = 4, K = 16 * KB, LD = 2 * K + 1;
  extern __shared__ __attribute__((aligned(16))) double smem[];  // K * LD doubles
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int s = blockIdx.x / g.nbps;
  const SGBlock bk = sg_block(g, s, list[2 * s]);
  const double2* const Qs = Q + static_cast<int64_t>(list[2 * s + 1]) * K * K;
  for (int e = tid; e < K * K; e += 256) {
    const int j = e / K, i = e - j * K;
    const double2 q = Qs[e];
    smem[i * LD + 2 * j] = q.x;
    smem[i * LD + 2 * j + 1] = q.y;
  }
  __syncthreads();
  const int kq = lane >> 4;
  int vr = bk.r0 + 16 * wave + (lane & 15);
  int o = vr / g.run, e = vr - o * g.run;
  const int step_o = (16 * NW) / g.run, step_e = (16 * NW) % g.run;
  for (int base = bk.r0 + 16 * wave; base < bk.r1; base += 16 * NW) {  // wave-uniform: every lane reaches the matrix pipe
    const SGRow rw = sg_row<false>(g, bk.t, bk.teff, o, e, vr < bk.r1);
    vr += 16 * NW;
    o += step_o;
    e += step_e;
    if (e >= g.run) {
      e -= g.run;
      o += 1;
    }
    Tile<16> tv[KB];
#pragma unroll
    for (int q = 0; q < KB; ++q) {
      const double2* p = v.p[q] + rw.row * v.ld[q] + kq;
#pragma unroll
      for (int c = 0; c < 4; ++c) tv[q].v[c] = rw.ok ? p[4 * c] : make_double2(0.0, 0.0);
    }
#pragma unroll
    for (int jb = 0; jb < KB; ++jb) {
      // KB >= 3: keep the loop-invariant coefficients out of registers, as k_basis_rotate_mfma does
      if constexpr (KB >= 3) asm volatile("" ::: "memory");
      Acc<16> A;
      acc_zero<16>(A);
#pragma unroll
      for (int q = 0; q < KB; ++q) rot_acc<LD>(A, tv[q], smem + 16 * q * LD + 32 * jb, lane);
      Tile<16> to;
      tile_from_acc<16>(to, A);
      double2* p = v.p[jb] + rw.row * v.ld[jb] + kq;
      if (rw.ok) {
#pragma unroll
        for (int c = 0; c < 4; ++c) p[4 * c] = to.v[c];
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Generic form: TR rows of the K columns in LDS; thread p + 256 q owns the pair (row, j) = (p / K, p % K).  The column
// table is built once per block by selects over the fields, and so are the TR rows' addresses once per tile.
// ---------------------------------------------------------------------------------------------
constexpr int kSliceRotateTR = 16;

__global__ void __launch_bounds__(256) k_basis_slice_rotate_generic(SGGeom g, const int* __restrict__ list, RotateFields v,
                                                                    const double2* __restrict__ Q) {
  constexpr int TR = kSliceRotateTR;
  extern __shared__ __attribute__((aligned(16))) double2 sm[];  // Qs[i * K + j] = Q_s(i, j) | xs[TR * K]
  __shared__ double2* colp[kRotateMaxCols];
  __shared__ int colw[kRotateMaxCols];
  __shared__ int64_t rowat[TR];  // the field row of the tile's row, or -1: not live, or a site the half field skips
  const int tid = threadIdx.x;
  const int K = v.K;
  double2* const Qs = sm;
  double2* const xs = sm + K * K;
  const int s = blockIdx.x / g.nbps;
  const SGBlock bk = sg_block(g, s, list[2 * s]);
  const double2* const Qg = Q + static_cast<int64_t>(list[2 * s + 1]) * K * K;
  for (int e = tid; e < K * K; e += 256) {
    const int j = e / K, i = e - j * K;
    Qs[i * K + j] = Qg[e];
  }
  if (tid < K) {
    double2* p = v.v[0];
    int w = v.w[0], o = 0, off = 0;
#pragma unroll
    for (int k = 0; k < kRotateMaxCols; ++k) {
      if (k < v.nv && tid >= off) {
        p = v.v[k];
        w = v.w[k];
        o = off;
      }
      off += k < v.nv ? v.w[k] : 0;
    }
    colp[tid] = p + (tid - o);
    colw[tid] = w;
  }
  for (int base = bk.r0; base < bk.r1; base += TR) {
    __syncthreads();  // the table (first tile); the products of the tile before have left xs and rowat
    if (tid < TR) {
      const SGRow rw = sg_row_at<false>(g, bk, base + tid);
      rowat[tid] = rw.ok ? rw.row : -1;
    }
    __syncthreads();
    for (int x = tid; x < TR * K; x += 256) {
      const int rr = x / K, i = x - rr * K;
      const int64_t row = rowat[rr];
      xs[x] = row >= 0 ? colp[i][row * colw[i]] : make_double2(0.0, 0.0);
    }
    __syncthreads();  // every load of the tile is done: the stores below overwrite what was read
    for (int x = tid; x < TR * K; x += 256) {
      const int rr = x / K, j = x - rr * K;
      const int64_t row = rowat[rr];
      if (row >= 0) {
        double2 acc = make_double2(0.0, 0.0);
        for (int i = 0; i < K; ++i) cfma(acc, xs[rr * K + i], Qs[i * K + j]);
        colp[j][row * colw[j]] = acc;
      }
    }
  }
}

template <int KB>
void slice_rotate_mfma_one(hipStream_t s, unsigned blocks, const SGGeom& g, const int* list, const RotateBlocks& v, const double2* Q) {
  const size_t lds = static_cast<size_t>(16 * KB) * (32 * KB + 1) * sizeof(double);
  allow_lds(k_basis_slice_rotate_mfma<KB>, lds);
  hipLaunchKernelGGL((k_basis_slice_rotate_mfma<KB>), dim3(blocks), dim3(256), lds, s, g, list, v, Q);
}

}  // namespace

void launch_basis_slice_rotate_mfma(hipStream_t s, int nblocks16, const LatticeDev& lat, int parity, int dir, const SliceWalk& plan,
                                    int n_slices, const int* list, const RotateBlocks& v, const double2* Q) {
  const SGGeom g = slice_geom(lat, parity, dir, plan);
  const unsigned blocks = static_cast<unsigned>(plan.nbps) * static_cast<unsigned>(n_slices);
  switch (nblocks16) {
    case 1: slice_rotate_mfma_one<1>(s, blocks, g, list, v, Q); break;
    case 2: slice_rotate_mfma_one<2>(s, blocks, g, list, v, Q); break;
    case 3: slice_rotate_mfma_one<3>(s, blocks, g, list, v, Q); break;
    default: slice_rotate_mfma_one<4>(s, blocks, g, list, v, Q); break;
  }
}

void launch_basis_slice_rotate_generic(hipStream_t s, const LatticeDev& lat, int parity, int dir, const SliceWalk& plan, int n_slices,
                                       const int* list, const RotateFields& v, const double2* Q) {
  const SGGeom g = slice_geom(lat, parity, dir, plan);
  const unsigned blocks = static_cast<unsigned>(plan.nbps) * static_cast<unsigned>(n_slices);
  const size_t lds = (static_cast<size_t>(v.K) * v.K + static_cast<size_t>(kSliceRotateTR) * v.K) * sizeof(double2);
  allow_lds(k_basis_slice_rotate_generic, lds);
  hipLaunchKernelGGL(k_basis_slice_rotate_generic, dim3(blocks), dim3(256), lds, s, g, list, v, Q);
}

}  // namespace bcg
