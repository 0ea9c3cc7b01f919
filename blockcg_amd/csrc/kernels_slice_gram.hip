// Per-slice Gram matrices with momentum projection (gfx950): C_p(t) = sum_{x_dir = t} w_p(x) a(x)^dagger b(x), all column
// pairs, PC momenta per pass over the operands.  The launch plan and the layouts: kernels_slice_gram.hpp; the walk:
// slice_plan.hpp, slice_walk.hpp.
// m = 16 and 32: v_mfma_f64_16x16x4_f64 through gram_step / GramAcc of mfma_common.hpp; every other width: one VALU
// kernel with the rows of a chunk staged in LDS.  Plain stores, no atomics; 64-bit wherever an element offset is formed.
#include "kernels_slice_gram.hpp"
#include "mfma_common.hpp"
#include "slice_walk.hpp"

namespace bcg {

namespace {

// gram_block_store of mfma_common.hpp with the destination given: the per-wave fragments summed in wave order, one 16 x 16
// block at a time through red (NW * 8 * 64 doubles), dst[j * M + i]
template <int M, int NW>
__device__ __forceinline__ void sg_block_store(const GramAcc<M>& G, double* red, double2* __restrict__ dst, int tid) {
  constexpr int JB = M / 16;
  const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
  for (int q = 0; q < JB * JB; ++q) {
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      red[(wave * 8 + r) * 64 + lane] = G.re[q][r];
      red[(wave * 8 + 4 + r) * 64 + lane] = G.im[q][r];
    }
    __syncthreads();
    for (int e = tid; e < 4 * 64; e += NW * 64) {
      const int l = e & 63, r = (e >> 6) & 3;
      double sr = 0.0, si = 0.0;
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        sr += red[(w * 8 + r) * 64 + l];
        si += red[(w * 8 + 4 + r) * 64 + l];
      }
      const int i = 16 * (q / JB) + (l >> 4) + 4 * r, j = 16 * (q % JB) + (l & 15);
      dst[j * M + i] = make_double2(sr, si);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// m = 16, 32.  Wave w of block (t, k) takes the quads w, w + 4, ... of the chunk; lane l owns row 4 q + (l >> 4) of a quad
// and column (l & 15) + 16 jb.  A quad may straddle sites and runs, so every lane derives its own row's address, validity
// and phase; the loop bound is the chunk's quad count, the same for all lanes of a wave.
// ---------------------------------------------------------------------------------------------
template <int M, int PC, bool PHASE, bool SELF>
__global__ void __launch_bounds__(256) k_slice_gram_mfma(SGGeom g, const double2* __restrict__ a, const double2* __restrict__ b,
                                                         const double2* __restrict__ tab, double2* __restrict__ partials) {
  constexpr int NW = 4, JB = M / 16, U = M == 16 ? 4 : 2;
  __shared__ __attribute__((aligned(16))) double red[NW * 8 * 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int t = blockIdx.x / g.nbps;
  const SGBlock bk = sg_block(g, t, t);
  const int teff = bk.teff, r0 = bk.r0, r1 = bk.r1;
  const int nq = (r1 - r0 + 3) >> 2;
  const int col = lane & 15;
  GramAcc<M> G[PC];
#pragma unroll
  for (int p = 0; p < PC; ++p) gram_zero(G[p]);
  int v = r0 + 4 * wave + (lane >> 4);
  int o = v / g.run, e = v - o * g.run;
  const int step_o = (4 * NW) / g.run, step_e = (4 * NW) % g.run;
  for (int q = wave; q < nq; q += NW * U) {
    SGRow rw[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      rw[u] = sg_row<PHASE>(g, t, teff, o, e, v < r1);
      v += 4 * NW;
      o += step_o;
      e += step_e;
      if (e >= g.run) {
        e -= g.run;
        o += 1;
      }
    }
    double2 av[U][JB], bv[U][JB];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int jb = 0; jb < JB; ++jb) {
        const int64_t ad = rw[u].row * M + 16 * jb + col;
        av[u][jb] = rw[u].ok ? a[ad] : make_double2(0.0, 0.0);
        bv[u][jb] = SELF ? av[u][jb] : (rw[u].ok ? b[ad] : make_double2(0.0, 0.0));
      }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int p = 0; p < PC; ++p) {
        if (PHASE) {
          const double2 w = sg_phase(tab, g.ltab, p, rw[u].x);
          double2 bw[JB];
#pragma unroll
          for (int jb = 0; jb < JB; ++jb) bw[jb] = cmul(bv[u][jb], w);
          gram_step<M>(G[p], av[u], bw);
        } else {
          gram_step<M>(G[p], av[u], bv[u]);
        }
      }
  }
#pragma unroll
  for (int p = 0; p < PC; ++p)
    sg_block_store<M, NW>(G[p], red, partials + (static_cast<int64_t>(blockIdx.x) * PC + p) * (M * M), tid);
}

// ---------------------------------------------------------------------------------------------
// Every other width.  R rows of the chunk at a time are staged in LDS (b already multiplied by the PC phases of its site),
// lane `tid` owns a 2 x 2 tile of (i, j) pairs (four operand reads per staged row for its four products) and walks the
// staged rows.
// ---------------------------------------------------------------------------------------------
constexpr int kSGRows = 16;

template <int PC, bool PHASE, bool SELF>
__global__ void __launch_bounds__(256) k_slice_gram_generic(int m, SGGeom g, const double2* __restrict__ a,
                                                            const double2* __restrict__ b, const double2* __restrict__ tab,
                                                            double2* __restrict__ partials) {
  constexpr int R = kSGRows;
  __shared__ double2 As[R * 32];
  __shared__ double2 Bs[PC][R * 32];
  const int tid = threadIdx.x;
  const int t = blockIdx.x / g.nbps, k = blockIdx.x - t * g.nbps;
  const int teff = g.half0 ? t >> 1 : t;
  const int r0 = k * g.chunk;
  const int r1 = r0 + g.chunk < g.n_virtual ? r0 + g.chunk : g.n_virtual;
  const int mm = m * m;
  // the lane's pairs: the 2 x 2 tile (i0 + di, j0 + dj), u = 2 dj + di, of the (m + 1) / 2 squared tiles (at most 256)
  const int mt = (m + 1) >> 1;
  const int j0 = 2 * (tid / mt), i0 = 2 * (tid - (tid / mt) * mt);
  const bool mine = tid < mt * mt;
  const int i1 = i0 + 1 < m ? i0 + 1 : i0, j1 = j0 + 1 < m ? j0 + 1 : j0;  // clamped: the pair is dropped at the store
  double2 acc[PC][4];
#pragma unroll
  for (int p = 0; p < PC; ++p)
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[p][u] = make_double2(0.0, 0.0);
  for (int base = r0; base < r1; base += R) {
    __syncthreads();
    for (int x = tid; x < R * m; x += 256) {
      const int r = x / m, j = x - r * m;
      const int v = base + r;
      const bool live = v < r1;
      const int vv = live ? v : r0;
      const int o = vv / g.run, e = vv - o * g.run;
      const SGRow rw = sg_row<PHASE>(g, t, teff, o, e, live);
      const int64_t ad = rw.row * m + j;
      const double2 av = rw.ok ? a[ad] : make_double2(0.0, 0.0);
      const double2 bv = SELF ? av : (rw.ok ? b[ad] : make_double2(0.0, 0.0));
      As[x] = av;
#pragma unroll
      for (int p = 0; p < PC; ++p) Bs[p][x] = PHASE ? cmul(bv, sg_phase(tab, g.ltab, p, rw.x)) : bv;
    }
    __syncthreads();
    if (mine) {
      for (int r = 0; r < R; ++r) {
        const double2 a0 = As[r * m + i0], a1 = As[r * m + i1];
#pragma unroll
        for (int p = 0; p < PC; ++p) {
          const double2 b0 = Bs[p][r * m + j0], b1 = Bs[p][r * m + j1];
          cfma_conj(acc[p][0], a0, b0);
          cfma_conj(acc[p][1], a1, b0);
          cfma_conj(acc[p][2], a0, b1);
          cfma_conj(acc[p][3], a1, b1);
        }
      }
    }
  }
#pragma unroll
  for (int p = 0; p < PC; ++p)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = i0 + (u & 1), j = j0 + (u >> 1);
      if (mine && i < m && j < m) partials[(static_cast<int64_t>(blockIdx.x) * PC + p) * mm + j * m + i] = acc[p][u];
    }
}

__global__ void __launch_bounds__(256) k_slice_gram_fold(int mm, int pc, int np, int L_local, int L_global, int nbps, int origin,
                                                         const double2* __restrict__ partials, double2* __restrict__ out) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= static_cast<int64_t>(np) * L_local * mm) return;
  const int e = static_cast<int>(i % mm);
  const int64_t r = i / mm;
  const int t = static_cast<int>(r % L_local), p = static_cast<int>(r / L_local);
  double2 s = make_double2(0.0, 0.0);
  for (int k = 0; k < nbps; ++k) {
    const double2 v = partials[((static_cast<int64_t>(t) * nbps + k) * pc + p) * mm + e];
    s.x += v.x;
    s.y += v.y;
  }
  out[(static_cast<int64_t>(p) * L_global + origin + t) * mm + e] = s;
}

template <int M, int PC, bool PHASE>
void launch_mfma(hipStream_t s, unsigned blocks, const SGGeom& g, const double2* a, const double2* b, const double2* tab,
                 double2* partials) {
  if (a == b) hipLaunchKernelGGL((k_slice_gram_mfma<M, PC, PHASE, true>), dim3(blocks), dim3(256), 0, s, g, a, b, tab, partials);
  else hipLaunchKernelGGL((k_slice_gram_mfma<M, PC, PHASE, false>), dim3(blocks), dim3(256), 0, s, g, a, b, tab, partials);
}
template <int PC, bool PHASE>
void launch_generic(hipStream_t s, unsigned blocks, int m, const SGGeom& g, const double2* a, const double2* b, const double2* tab,
                    double2* partials) {
  if (a == b) hipLaunchKernelGGL((k_slice_gram_generic<PC, PHASE, true>), dim3(blocks), dim3(256), 0, s, m, g, a, b, tab, partials);
  else hipLaunchKernelGGL((k_slice_gram_generic<PC, PHASE, false>), dim3(blocks), dim3(256), 0, s, m, g, a, b, tab, partials);
}

bool use_mfma(int m, bool mfma) { return mfma && (m == 16 || m == 32); }

}  // namespace

void launch_slice_gram(hipStream_t s, int m, bool mfma, const LatticeDev& lat, int parity, int dir, const SliceGramPlan& plan, int pc,
                       const double2* a, const double2* b, const double2* tab, double2* partials) {
  const SGGeom g = slice_geom(lat, parity, dir, plan.walk);
  const unsigned blocks = static_cast<unsigned>(plan.walk.nbps) * static_cast<unsigned>(lat.L[dir]);
  if (use_mfma(m, mfma)) {
    if (m == 16) {
      if (!tab) launch_mfma<16, 1, false>(s, blocks, g, a, b, tab, partials);
      else if (pc == 1) launch_mfma<16, 1, true>(s, blocks, g, a, b, tab, partials);
      else if (pc == 2) launch_mfma<16, 2, true>(s, blocks, g, a, b, tab, partials);
      else launch_mfma<16, 4, true>(s, blocks, g, a, b, tab, partials);
    } else {
      if (!tab) launch_mfma<32, 1, false>(s, blocks, g, a, b, tab, partials);
      else if (pc == 1) launch_mfma<32, 1, true>(s, blocks, g, a, b, tab, partials);
      else launch_mfma<32, 2, true>(s, blocks, g, a, b, tab, partials);
    }
  } else {
    if (!tab) launch_generic<1, false>(s, blocks, m, g, a, b, tab, partials);
    else if (pc == 1) launch_generic<1, true>(s, blocks, m, g, a, b, tab, partials);
    else launch_generic<2, true>(s, blocks, m, g, a, b, tab, partials);
  }
}

void launch_slice_gram_fold(hipStream_t s, int m, int pc, int np, int L_local, int L_global, int nbps, int origin,
                            const double2* partials, double2* out) {
  const int64_t n = static_cast<int64_t>(np) * L_local * m * m;
  hipLaunchKernelGGL(k_slice_gram_fold, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, s, m * m, pc, np, L_local, L_global,
                     nbps, origin, partials, out);
}

}  // namespace bcg
