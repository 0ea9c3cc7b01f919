// Per-slice products with a basis of another width (gfx950): tau_p(t) = sum_{x_dir = t} w_p(x) V(x)^dagger b(x), K x m per
// slice and momentum.  The forms, the launch plan and the layouts: kernels_basis_slice.hpp; the walk over the rows of a slice:
// slice_walk.hpp.  MFMA form: v_mfma_f64_16x16x4_f64 in the operand ownership of gram_step (mfma_common.hpp), four real
// products per pair of 16-column blocks as in k_basis_dot_mfma.  Generic form: the rows of a chunk staged in LDS, each thread
// its (i, j) pairs.  Plain stores, no atomics; 64-bit wherever an element offset is formed.
#include "kernels_basis_slice.hpp"
#include "mfma_common.hpp"
#include "slice_walk.hpp"

namespace bcg {

namespace {

// ---------------------------------------------------------------------------------------------
// MFMA form.  Wave w of block (t, k) takes the quads w, w + 4, ... of the chunk; lane l owns row 4 q + (l >> 4) of a quad and
// column l & 15 of every 16-column block of V and of b (k_slice_gram_mfma's cursor: a quad may straddle sites and runs, so
// every lane derives its own row's address, validity and phase).  b is multiplied by the PC phases of its site before it
// goes to the matrix pipe.  Accumulators: PC x KB x (M / 16) pairs of 16 x 16 blocks, re and im.
// ---------------------------------------------------------------------------------------------
template <int M, int KB, int PC, bool PHASE>
__global__ void __launch_bounds__(256) k_basis_slice_dot_mfma(SGGeom g, BasisBlocks v, const double2* __restrict__ b,
                                                              const double2* __restrict__ tab, double2* __restrict__ partials) {
  constexpr int NW = 4, JB = M / 16, U = 2, KG = 16 * KB, NT = KB * JB;
  static_assert(KB * PC * JB <= 4, "64 accumulator registers at the most");
  __shared__ __attribute__((aligned(16))) double red[NW * 8 * 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int t = blockIdx.x / g.nbps;
  const SGBlock bk = sg_block(g, t, t);
  const int teff = bk.teff, r0 = bk.r0, r1 = bk.r1;
  const int nq = (r1 - r0 + 3) >> 2;
  const int col = lane & 15;
  d4 re[PC][NT], im[PC][NT];
#pragma unroll
  for (int p = 0; p < PC; ++p)
#pragma unroll
    for (int q = 0; q < NT; ++q) {
      re[p][q] = d4{0.0, 0.0, 0.0, 0.0};
      im[p][q] = d4{0.0, 0.0, 0.0, 0.0};
    }
  int vr = r0 + 4 * wave + (lane >> 4);
  int o = vr / g.run, e = vr - o * g.run;
  const int step_o = (4 * NW) / g.run, step_e = (4 * NW) % g.run;
  for (int q = wave; q < nq; q += NW * U) {
    SGRow rw[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      rw[u] = sg_row<PHASE>(g, t, teff, o, e, vr < r1);
      vr += 4 * NW;
      o += step_o;
      e += step_e;
      if (e >= g.run) {
        e -= g.run;
        o += 1;
      }
    }
    double2 av[U][KB], bv[U][JB];
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
      for (int q16 = 0; q16 < KB; ++q16) av[u][q16] = rw[u].ok ? v.p[q16][rw[u].row * v.ld[q16] + col] : make_double2(0.0, 0.0);
#pragma unroll
      for (int jb = 0; jb < JB; ++jb) bv[u][jb] = rw[u].ok ? b[rw[u].row * M + 16 * jb + col] : make_double2(0.0, 0.0);
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int p = 0; p < PC; ++p) {
        double2 bw[JB];
        if (PHASE) {
          const double2 w = sg_phase(tab, g.ltab, p, rw[u].x);
#pragma unroll
          for (int jb = 0; jb < JB; ++jb) bw[jb] = cmul(bv[u][jb], w);
        } else {
#pragma unroll
          for (int jb = 0; jb < JB; ++jb) bw[jb] = bv[u][jb];
        }
#pragma unroll
        for (int q16 = 0; q16 < KB; ++q16)
#pragma unroll
          for (int jb = 0; jb < JB; ++jb) {  // conj(a) b: gram_step's four products
            const int s = q16 * JB + jb;
            re[p][s] = mfma(av[u][q16].x, bw[jb].x, re[p][s]);
            re[p][s] = mfma(av[u][q16].y, bw[jb].y, re[p][s]);
            im[p][s] = mfma(av[u][q16].x, bw[jb].y, im[p][s]);
            im[p][s] = mfma_nega(av[u][q16].y, bw[jb].x, im[p][s]);
          }
      }
  }
  // the per-wave fragments summed in wave order, one 16 x 16 block at a time through red
#pragma unroll
  for (int p = 0; p < PC; ++p) {
    double2* const dst = partials + (static_cast<int64_t>(blockIdx.x) * PC + p) * (KG * M);
#pragma unroll
    for (int s = 0; s < NT; ++s) {
      __syncthreads();
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        red[(wave * 8 + r) * 64 + lane] = re[p][s][r];
        red[(wave * 8 + 4 + r) * 64 + lane] = im[p][s][r];
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
        const int i = 16 * (s / JB) + (l >> 4) + 4 * r, j = 16 * (s % JB) + (l & 15);
        dst[j * KG + i] = make_double2(sr, si);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Generic form.  R rows of the chunk at a time are staged in LDS: the group's columns, and b already multiplied by the PC
// phases of its site; thread p + 256 q owns the pair (i, j) = (p % K_g, p / K_g) and walks the staged rows.
// ---------------------------------------------------------------------------------------------
constexpr int kBSRows = 16;

template <int PC, bool PHASE>
__global__ void __launch_bounds__(256) k_basis_slice_dot_generic(int m, SGGeom g, BasisFields v, const double2* __restrict__ b,
                                                                 const double2* __restrict__ tab, double2* __restrict__ partials) {
  constexpr int R = kBSRows, NPT = kBasisGenericCols * 32 / 256;
  __shared__ double2 As[R * kBasisGenericCols];
  __shared__ double2 Bs[PC][R * 32];
  const int tid = threadIdx.x;
  const int t = blockIdx.x / g.nbps;
  const SGBlock bk = sg_block(g, t, t);
  const int Kg = v.K, P = Kg * m;
  double2 acc[PC][NPT];
#pragma unroll
  for (int p = 0; p < PC; ++p)
#pragma unroll
    for (int q = 0; q < NPT; ++q) acc[p][q] = make_double2(0.0, 0.0);
  for (int base = bk.r0; base < bk.r1; base += R) {
    __syncthreads();
    for (int x = tid; x < R * Kg; x += 256) {
      const int r = x / Kg, i = x - r * Kg;
      const SGRow rw = sg_row_at<false>(g, bk, base + r);
      int w, off;
      const double2* f = basis_column(v, i, &w, &off);
      As[x] = rw.ok ? f[rw.row * w + (i - off)] : make_double2(0.0, 0.0);
    }
    for (int x = tid; x < R * m; x += 256) {
      const int r = x / m, j = x - r * m;
      const SGRow rw = sg_row_at<PHASE>(g, bk, base + r);
      const double2 bv = rw.ok ? b[rw.row * m + j] : make_double2(0.0, 0.0);
#pragma unroll
      for (int p = 0; p < PC; ++p) Bs[p][x] = PHASE ? cmul(bv, sg_phase(tab, g.ltab, p, rw.x)) : bv;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NPT; ++q) {
      const int pr = tid + 256 * q;
      if (pr < P) {
        const int j = pr / Kg, i = pr - j * Kg;
        for (int r = 0; r < R; ++r) {
          const double2 a = As[r * Kg + i];
#pragma unroll
          for (int p = 0; p < PC; ++p) cfma_conj(acc[p][q], a, Bs[p][r * m + j]);
        }
      }
    }
  }
#pragma unroll
  for (int p = 0; p < PC; ++p)
#pragma unroll
    for (int q = 0; q < NPT; ++q) {
      const int pr = tid + 256 * q;
      if (pr < P) partials[(static_cast<int64_t>(blockIdx.x) * PC + p) * P + pr] = acc[p][q];
    }
}

// k_slice_gram_fold for a K_g x m block that lands at column offset `off` of a K x m matrix, momentum p0 + p
__global__ void __launch_bounds__(256) k_basis_slice_fold(int Kg, int m, int pc, int np, int L_local, int L_global, int nbps,
                                                          int origin, int K, int off, int p0, const double2* __restrict__ partials,
                                                          double2* __restrict__ out) {
  const int P = Kg * m;
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (idx >= static_cast<int64_t>(np) * L_local * P) return;
  const int e = static_cast<int>(idx % P);
  const int64_t r = idx / P;
  const int t = static_cast<int>(r % L_local), p = static_cast<int>(r / L_local);
  double2 s = make_double2(0.0, 0.0);
  for (int k = 0; k < nbps; ++k) {
    const double2 x = partials[((static_cast<int64_t>(t) * nbps + k) * pc + p) * P + e];
    s.x += x.x;
    s.y += x.y;
  }
  const int j = e / Kg, i = e - j * Kg;
  out[((static_cast<int64_t>(p0 + p) * L_global + origin + t) * m + j) * K + off + i] = s;
}

template <int M, int KB>
void slice_dot_mfma(hipStream_t s, unsigned blocks, int pc, const SGGeom& g, const BasisBlocks& v, const double2* b, const double2* tab,
                    double2* partials) {
  constexpr int JB = M / 16;
  if (!tab) {
    hipLaunchKernelGGL((k_basis_slice_dot_mfma<M, KB, 1, false>), dim3(blocks), dim3(256), 0, s, g, v, b, tab, partials);
  } else if (pc == 1) {
    hipLaunchKernelGGL((k_basis_slice_dot_mfma<M, KB, 1, true>), dim3(blocks), dim3(256), 0, s, g, v, b, tab, partials);
  } else if (pc == 2) {
    if constexpr (KB * 2 * JB <= 4) hipLaunchKernelGGL((k_basis_slice_dot_mfma<M, KB, 2, true>), dim3(blocks), dim3(256), 0, s, g, v, b, tab, partials);
  } else {
    if constexpr (KB * 4 * JB <= 4) hipLaunchKernelGGL((k_basis_slice_dot_mfma<M, KB, 4, true>), dim3(blocks), dim3(256), 0, s, g, v, b, tab, partials);
  }
}

}  // namespace

void launch_basis_slice_dot_mfma(hipStream_t s, int m, int kb, const LatticeDev& lat, int parity, int dir, const BasisSlicePlan& plan,
                                 int pc, const BasisBlocks& v, const double2* b, const double2* tab, double2* partials) {
  const SGGeom g = slice_geom(lat, parity, dir, plan.walk);
  const unsigned blocks = static_cast<unsigned>(plan.walk.nbps) * static_cast<unsigned>(lat.L[dir]);
  if (m == 16) {
    switch (kb) {
      case 1: slice_dot_mfma<16, 1>(s, blocks, pc, g, v, b, tab, partials); break;
      case 2: slice_dot_mfma<16, 2>(s, blocks, pc, g, v, b, tab, partials); break;
      case 3: slice_dot_mfma<16, 3>(s, blocks, pc, g, v, b, tab, partials); break;
      default: slice_dot_mfma<16, 4>(s, blocks, pc, g, v, b, tab, partials); break;
    }
  } else {
    if (kb == 1) slice_dot_mfma<32, 1>(s, blocks, pc, g, v, b, tab, partials);
    else slice_dot_mfma<32, 2>(s, blocks, pc, g, v, b, tab, partials);
  }
}

void launch_basis_slice_dot_generic(hipStream_t s, int m, const LatticeDev& lat, int parity, int dir, const BasisSlicePlan& plan,
                                    int pc, const BasisFields& v, const double2* b, const double2* tab, double2* partials) {
  const SGGeom g = slice_geom(lat, parity, dir, plan.walk);
  const unsigned blocks = static_cast<unsigned>(plan.walk.nbps) * static_cast<unsigned>(lat.L[dir]);
  if (!tab) hipLaunchKernelGGL((k_basis_slice_dot_generic<1, false>), dim3(blocks), dim3(256), 0, s, m, g, v, b, tab, partials);
  else if (pc == 1) hipLaunchKernelGGL((k_basis_slice_dot_generic<1, true>), dim3(blocks), dim3(256), 0, s, m, g, v, b, tab, partials);
  else hipLaunchKernelGGL((k_basis_slice_dot_generic<2, true>), dim3(blocks), dim3(256), 0, s, m, g, v, b, tab, partials);
}

void launch_basis_slice_fold(hipStream_t s, int Kg, int m, int pc, int np, int L_local, int L_global, int nbps, int origin, int K,
                             int off, int p0, const double2* partials, double2* out) {
  const int64_t n = static_cast<int64_t>(np) * L_local * Kg * m;
  hipLaunchKernelGGL(k_basis_slice_fold, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, s, Kg, m, pc, np, L_local,
                     L_global, nbps, origin, K, off, p0, partials, out);
}

}  // namespace bcg
