// A basis put onto time slices (gfx950): y <- beta y + w V C_s on the sites of the listed slices, y <- beta y elsewhere.
// The forms, the launch plan and the layouts: kernels_basis_slice_axpy.hpp; the walk over the rows of a slice:
// slice_walk.hpp.  MFMA form: v_mfma_f64_16x16x4_f64 in the operand ownership of Tile / rect_acc (mfma_common.hpp), as in
// k_basis_axpy_mfma.  Generic form: the rows of a tile staged in LDS, thread = (row, output column).  Plain stores, no
// atomics; 64-bit wherever an element offset is formed.
#include "kernels_basis_slice_axpy.hpp"
#include "mfma_common.hpp"
#include "slice_walk.hpp"

namespace bcg {

namespace {

// ---------------------------------------------------------------------------------------------
// MFMA form.  Wave w of block (s, k) takes the steps w, w + 4, ... of 16 rows of the chunk; lane l owns row l & 15 of a
// step and derives its own row's address, validity and phase (k_slice_gram_mfma's cursor, 16 rows apart instead of 4).
// ---------------------------------------------------------------------------------------------
template <int M, int KB, bool PHASE>
__global__ void __launch_bounds__(256) k_basis_slice_axpy_mfma(SGGeom g, const int* __restrict__ list, double2* __restrict__ y,
                                                               BasisBlocks v, const double2* __restrict__ C, int K, int off,
                                                               const double2* __restrict__ tab, double beta) {
  constexpr int NW = 4, KG = 16 * KB, LD = MatLds<M>::LD;
  extern __shared__ __attribute__((aligned(16))) double smem[];  // KG * LD doubles
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int s = blockIdx.x / g.nbps, k = blockIdx.x - s * g.nbps;
  const int t = list[2 * s];
  const double2* const Cs = C + static_cast<int64_t>(list[2 * s + 1]) * M * K;
  for (int e = tid; e < KG * M; e += 256) {
    const int j = e / KG, i = e - j * KG;
    const double2 c = Cs[static_cast<int64_t>(j) * K + off + i];
    smem[i * LD + 2 * j] = c.x;
    smem[i * LD + 2 * j + 1] = c.y;
  }
  __syncthreads();
  const int teff = g.half0 ? t >> 1 : t;
  const int r0 = k * g.chunk;
  const int r1 = r0 + g.chunk < g.n_virtual ? r0 + g.chunk : g.n_virtual;
  const bool rd = beta != 0.0;
  const int kq = lane >> 4;
  int vr = r0 + 16 * wave + (lane & 15);
  int o = vr / g.run, e = vr - o * g.run;
  const int step_o = (16 * NW) / g.run, step_e = (16 * NW) % g.run;
  for (int base = r0 + 16 * wave; base < r1; base += 16 * NW) {  // wave-uniform: every lane reaches the matrix pipe
    const SGRow rw = sg_row<PHASE>(g, t, teff, o, e, vr < r1);
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
    Tile<M> ty;
    tile_load<M>(ty, y, rw.row, kq, rw.ok && rd);
    Acc<M> A;
    acc_zero<M>(A);
#pragma unroll
    for (int q = 0; q < KB; ++q) rect_acc<M>(A, tv[q], smem + 16 * q * LD, lane);
    Tile<M> ta;
    tile_from_acc<M>(ta, A);
    if (PHASE) {
      const double2 w = sg_phase(tab, g.ltab, 0, rw.x);
#pragma unroll
      for (int c = 0; c < M / 4; ++c) ta.v[c] = cmul(ta.v[c], w);
    }
    if (rd) {
#pragma unroll
      for (int c = 0; c < M / 4; ++c) ta.v[c] = make_double2(fma(beta, ty.v[c].x, ta.v[c].x), fma(beta, ty.v[c].y, ta.v[c].y));
    }
    tile_store<M>(ta, y, rw.row, kq, rw.ok);
  }
}

// ---------------------------------------------------------------------------------------------
// Generic form: k_basis_axpy_generic on the slice walk.  Thread (rl, j) computes y[row][j]; R rows of the group's columns
// and its rows of C_s sit in LDS.
// ---------------------------------------------------------------------------------------------
template <bool PHASE>
__global__ void __launch_bounds__(256) k_basis_slice_axpy_generic(int m, SGGeom g, const int* __restrict__ list, double2* __restrict__ y,
                                                                  BasisFields v, const double2* __restrict__ C, int K, int off,
                                                                  const double2* __restrict__ tab, double beta) {
  constexpr int RMAX = 32;
  __shared__ double2 Ct[kBasisGenericCols * 32];  // Ct[i * m + j] = C_s(off + i, j)
  __shared__ double2 xs[RMAX * kBasisGenericCols];
  const int tid = threadIdx.x;
  const int Kg = v.K;
  const int s = blockIdx.x / g.nbps;
  const int t = list[2 * s];
  const double2* const Cs = C + static_cast<int64_t>(list[2 * s + 1]) * m * K;
  for (int e = tid; e < Kg * m; e += 256) {
    const int i = e / m, j = e - i * m;
    Ct[e] = Cs[static_cast<int64_t>(j) * K + off + i];
  }
  const SGBlock bk = sg_block(g, s, t);
  const int teff = bk.teff, r0 = bk.r0, r1 = bk.r1;
  const int R = 256 / m < RMAX ? 256 / m : RMAX;
  const int rl = tid / m, j = tid - rl * m;
  const bool rd = beta != 0.0;
  for (int base = r0; base < r1; base += R) {
    __syncthreads();
    for (int x = tid; x < R * Kg; x += 256) {
      const int rr = x / Kg, i = x - rr * Kg;
      const int vr = base + rr;
      const bool live = vr < r1;
      const int vv = live ? vr : r0;
      const int o = vv / g.run, e = vv - o * g.run;
      const SGRow rw = sg_row<false>(g, t, teff, o, e, live);
      int w, fo;
      const double2* f = basis_column(v, i, &w, &fo);
      xs[x] = rw.ok ? f[rw.row * w + (i - fo)] : make_double2(0.0, 0.0);
    }
    __syncthreads();
    const int vr = base + rl;
    if (rl < R && vr < r1) {
      const int o = vr / g.run, e = vr - o * g.run;
      const SGRow rw = sg_row<PHASE>(g, t, teff, o, e, true);
      if (rw.ok) {
        double2 acc = make_double2(0.0, 0.0);
        for (int i = 0; i < Kg; ++i) cfma(acc, xs[rl * Kg + i], Ct[i * m + j]);
        if (PHASE) acc = cmul(acc, sg_phase(tab, g.ltab, 0, rw.x));
        if (rd) {
          const double2 yv = y[rw.row * m + j];
          acc = make_double2(fma(beta, yv.x, acc.x), fma(beta, yv.y, acc.y));
        }
        y[rw.row * m + j] = acc;
      }
    }
  }
}

// the slices that are not listed: y <- beta y, or zeros; the elements of a chunk in row order, one per thread and step
template <bool ZERO>
__global__ void __launch_bounds__(256) k_slice_scale(int m, SGGeom g, const int* __restrict__ slices, double2* __restrict__ y, double beta) {
  const int s = blockIdx.x / g.nbps;
  const SGBlock bk = sg_block(g, s, slices[s]);
  const int64_t n = static_cast<int64_t>(bk.r1 - bk.r0) * m;
  for (int64_t x = threadIdx.x; x < n; x += 256) {
    const int rr = static_cast<int>(x / m), j = static_cast<int>(x - static_cast<int64_t>(rr) * m);
    const int vr = bk.r0 + rr;
    const int o = vr / g.run, e = vr - o * g.run;
    const SGRow rw = sg_row<false>(g, bk.t, bk.teff, o, e, true);
    if (rw.ok) {
      double2* const p = y + rw.row * m + j;
      if (ZERO) {
        *p = make_double2(0.0, 0.0);
      } else {
        const double2 yv = *p;
        *p = make_double2(beta * yv.x, beta * yv.y);
      }
    }
  }
}

template <int M, int KB>
void slice_axpy_mfma_one(hipStream_t s, unsigned blocks, const SGGeom& g, const int* list, double2* y, const BasisBlocks& v,
                         const double2* C, int K, int off, const double2* tab, double beta) {
  const size_t lds = static_cast<size_t>(16 * KB) * MatLds<M>::LD * sizeof(double);
  if (tab) {
    allow_lds(k_basis_slice_axpy_mfma<M, KB, true>, lds);
    hipLaunchKernelGGL((k_basis_slice_axpy_mfma<M, KB, true>), dim3(blocks), dim3(256), lds, s, g, list, y, v, C, K, off, tab, beta);
  } else {
    allow_lds(k_basis_slice_axpy_mfma<M, KB, false>, lds);
    hipLaunchKernelGGL((k_basis_slice_axpy_mfma<M, KB, false>), dim3(blocks), dim3(256), lds, s, g, list, y, v, C, K, off, tab, beta);
  }
}
template <int M>
void slice_axpy_mfma(hipStream_t s, int kb, unsigned blocks, const SGGeom& g, const int* list, double2* y, const BasisBlocks& v,
                     const double2* C, int K, int off, const double2* tab, double beta) {
  switch (kb) {
    case 1: slice_axpy_mfma_one<M, 1>(s, blocks, g, list, y, v, C, K, off, tab, beta); break;
    case 2: slice_axpy_mfma_one<M, 2>(s, blocks, g, list, y, v, C, K, off, tab, beta); break;
    case 3: slice_axpy_mfma_one<M, 3>(s, blocks, g, list, y, v, C, K, off, tab, beta); break;
    default:  // 4 blocks: m = 16 only (basis_axpy_mfma_blocks)
      if constexpr (M == 16) slice_axpy_mfma_one<M, 4>(s, blocks, g, list, y, v, C, K, off, tab, beta);
      break;
  }
}

}  // namespace

void launch_basis_slice_axpy_mfma(hipStream_t s, int m, int nblocks16, const LatticeDev& lat, int parity, int dir,
                                  const SliceWalk& plan, int n_slices, const int* list, double2* y, const BasisBlocks& v,
                                  const double2* C, int K, int off, const double2* tab, double beta) {
  const SGGeom g = slice_geom(lat, parity, dir, plan);
  const unsigned blocks = static_cast<unsigned>(plan.nbps) * static_cast<unsigned>(n_slices);
  if (m == 16) slice_axpy_mfma<16>(s, nblocks16, blocks, g, list, y, v, C, K, off, tab, beta);
  else slice_axpy_mfma<32>(s, nblocks16, blocks, g, list, y, v, C, K, off, tab, beta);
}

void launch_basis_slice_axpy_generic(hipStream_t s, int m, const LatticeDev& lat, int parity, int dir, const SliceWalk& plan,
                                     int n_slices, const int* list, double2* y, const BasisFields& v, const double2* C, int K, int off,
                                     const double2* tab, double beta) {
  const SGGeom g = slice_geom(lat, parity, dir, plan);
  const unsigned blocks = static_cast<unsigned>(plan.nbps) * static_cast<unsigned>(n_slices);
  if (tab) hipLaunchKernelGGL((k_basis_slice_axpy_generic<true>), dim3(blocks), dim3(256), 0, s, m, g, list, y, v, C, K, off, tab, beta);
  else hipLaunchKernelGGL((k_basis_slice_axpy_generic<false>), dim3(blocks), dim3(256), 0, s, m, g, list, y, v, C, K, off, tab, beta);
}

void launch_slice_scale(hipStream_t s, int m, const LatticeDev& lat, int parity, int dir, const SliceWalk& plan, int n_slices,
                        const int* slices, double2* y, double beta) {
  const SGGeom g = slice_geom(lat, parity, dir, plan);
  const unsigned blocks = static_cast<unsigned>(plan.nbps) * static_cast<unsigned>(n_slices);
  if (beta == 0.0) hipLaunchKernelGGL((k_slice_scale<true>), dim3(blocks), dim3(256), 0, s, m, g, slices, y, beta);
  else hipLaunchKernelGGL((k_slice_scale<false>), dim3(blocks), dim3(256), 0, s, m, g, slices, y, beta);
}

}  // namespace bcg
