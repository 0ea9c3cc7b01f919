// Baryon elementals of a basis, slice by slice (gfx950): T_p(t; i, j, k) = sum_x w_p(x) det[A_i(x), B_j(x), C_k(x)] over the
// sites of a slice.  The forms, the layouts and the profile models: kernels_basis_slice_triple.hpp; the plan: slice_plan.hpp;
// the walk over the rows of a slice: slice_walk.hpp.  Plain stores, no atomics; 64-bit wherever an element offset is formed.
#include "kernels_basis_slice_triple.hpp"
#include "mfma_common.hpp"
#include "slice_walk.hpp"

namespace bcg {

namespace {

__device__ __forceinline__ double2 czero() { return make_double2(0.0, 0.0); }
// a b - c d
__device__ __forceinline__ double2 cross_term(double2 a, double2 b, double2 c, double2 d) {
  double2 r;
  r.x = a.x * b.x - a.y * b.y - (c.x * d.x - c.y * d.y);
  r.y = a.x * b.y + a.y * b.x - (c.x * d.y + c.y * d.x);
  return r;
}

// ---------------------------------------------------------------------------------------------
// MFMA form.  Block (s, k; tile): the k-th chunk of listed slice s, the 16 columns 16 ta .. of A, 16 tb .. of B, 16 tc .. of C.
// A step is four sites.  Threads 0 .. 191 stage it: thread (row r = tid >> 4 of the 12, column tid & 15) loads its element
// of the three lists (one walk cursor for the three) and multiplies C's by the phase of the site; the loads of step n + 1
// are issued before the products of step n.  LDS: [colour][site][column], A's rows padded to 17 so that the four sites of
// a broadcast read fall on different banks.  K-step a of a step takes colour a of the four sites: lane (l & 15, l >> 4)
// supplies D_ij(site l >> 4, colour a) for j = l & 15 as the A operand and w C_k(site l >> 4, colour a) for k = l & 15 as the
// B operand, so that register r of the accumulator of i holds (j = (l >> 4) + 4 r, k = l & 15).
// ---------------------------------------------------------------------------------------------
constexpr int kTripleLdA = 17;

template <bool PHASE>
__global__ void __launch_bounds__(256, 2) k_basis_slice_triple_mfma(SGGeom g, const TripleCol* __restrict__ cols, const int* __restrict__ tiles,
                                                                    const int* __restrict__ list, const double2* __restrict__ tab,
                                                                    double2* __restrict__ partials) {
  constexpr int E = kTripleEdgeMfma, KMAX = kTripleMaxColumns;
  __shared__ double2 sA[3 * 4 * kTripleLdA];
  __shared__ double2 sB[3 * 4 * E];
  __shared__ double2 sC[3 * 4 * E];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int s = blockIdx.x / g.nbps;
  const SGBlock bk = sg_block(g, s, list[2 * s]);
  const int ta = tiles[3 * blockIdx.y], tb = tiles[3 * blockIdx.y + 1], tc = tiles[3 * blockIdx.y + 2];
  // the staging role: element (site lsx of the step, colour lcol, column lc) of each list
  const bool loader = tid < 192;
  const int lc = tid & 15, lr = loader ? tid >> 4 : 0, lsx = lr / 3, lcol = lr - 3 * lsx;
  const TripleCol ca = cols[E * ta + lc], cb = cols[KMAX + E * tb + lc], cc = cols[2 * KMAX + E * tc + lc];
  d4 re[4], im[4];
#pragma unroll
  for (int ii = 0; ii < 4; ++ii) {
    re[ii] = d4{0.0, 0.0, 0.0, 0.0};
    im[ii] = d4{0.0, 0.0, 0.0, 0.0};
  }
  const int nsteps = (bk.r1 - bk.r0 + 11) / 12;
  double2 ga = czero(), gb = czero(), gc = czero();
  auto fetch = [&](int step) {
    ga = gb = gc = czero();
    if (loader) {
      const SGRow rw = sg_row_at<PHASE>(g, bk, bk.r0 + 12 * step + 3 * lsx);
      if (rw.ok) {
        const int64_t row = rw.row + lcol;
        ga = ca.p[row * ca.ld];
        gb = cb.p[row * cb.ld];
        gc = cc.p[row * cc.ld];
        if (PHASE) gc = cmul(gc, sg_phase(tab, g.ltab, 0, rw.x));
      }
    }
  };
  fetch(0);
  const int sx = lane >> 4, c16 = lane & 15;
  for (int step = 0; step < nsteps; ++step) {
    __syncthreads();  // the products of the step before have read the buffers
    if (loader) {
      sA[(lcol * 4 + lsx) * kTripleLdA + lc] = ga;
      sB[(lcol * 4 + lsx) * E + lc] = gb;
      sC[(lcol * 4 + lsx) * E + lc] = gc;
    }
    __syncthreads();
    if (step + 1 < nsteps) fetch(step + 1);
    double2 a[4][3], b[3], cw[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      b[c] = sB[(c * 4 + sx) * E + c16];
      cw[c] = sC[(c * 4 + sx) * E + c16];
#pragma unroll
      for (int ii = 0; ii < 4; ++ii) a[ii][c] = sA[(c * 4 + sx) * kTripleLdA + 4 * wave + ii];
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const int q1 = (q + 1) % 3, q2 = (q + 2) % 3;
#pragma unroll
      for (int ii = 0; ii < 4; ++ii) {
        const double2 D = cross_term(a[ii][q1], b[q2], a[ii][q2], b[q1]);
        re[ii] = mfma(D.x, cw[q].x, re[ii]);
        re[ii] = mfma_nega(D.y, cw[q].y, re[ii]);
        im[ii] = mfma(D.x, cw[q].y, im[ii]);
        im[ii] = mfma(D.y, cw[q].x, im[ii]);
      }
    }
  }
  double2* const dst = partials + (static_cast<int64_t>(blockIdx.y) * gridDim.x + blockIdx.x) * (E * E * E);
#pragma unroll
  for (int ii = 0; ii < 4; ++ii)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = 4 * wave + ii, j = sx + 4 * r, k = c16;
      dst[(k * E + j) * E + i] = make_double2(re[ii][r], im[ii][r]);
    }
}

// ---------------------------------------------------------------------------------------------
// Generic form.  Block (s, k; tile): 8 columns of each list (fewer at a list's end: zeros).  16 sites of the chunk at a time
// are staged in LDS, [list][site][colour][column], C multiplied by the phase; thread (i = tid & 7, j = (tid >> 3) & 7,
// k0 = tid >> 6) forms D_ij of a site once and adds to its entries (i, j, k0) and (i, j, k0 + 4).
// ---------------------------------------------------------------------------------------------
constexpr int kTripleGenericSites = 16;

template <bool PHASE>
__global__ void __launch_bounds__(256) k_basis_slice_triple_generic(SGGeom g, const TripleCol* __restrict__ cols, int Ka, int Kb, int Kc,
                                                                    const int* __restrict__ tiles, const int* __restrict__ list,
                                                                    const double2* __restrict__ tab, double2* __restrict__ partials) {
  constexpr int E = kTripleEdgeGeneric, R = kTripleGenericSites, KMAX = kTripleMaxColumns, PER = R * 3 * E;
  __shared__ double2 sh[3 * PER];
  const int tid = threadIdx.x;
  const int s = blockIdx.x / g.nbps;
  const SGBlock bk = sg_block(g, s, list[2 * s]);
  const int t0[3] = {E * tiles[3 * blockIdx.y], E * tiles[3 * blockIdx.y + 1], E * tiles[3 * blockIdx.y + 2]};
  const int ii = tid & 7, jj = (tid >> 3) & 7, k0 = tid >> 6;
  double2 acc0 = czero(), acc1 = czero();
  for (int base = bk.r0; base < bk.r1; base += 3 * R) {
    __syncthreads();
    for (int x = tid; x < 3 * PER; x += 256) {
      const int l = x / PER, y = x - l * PER;
      const int site = y / (3 * E), z = y - site * (3 * E);
      const int colour = z / E, col = z - colour * E;
      const int column = (l == 0 ? t0[0] : l == 1 ? t0[1] : t0[2]) + col;
      const int K = l == 0 ? Ka : l == 1 ? Kb : Kc;
      double2 v = czero();
      if (column < K) {
        const SGRow rw = sg_row_at<PHASE>(g, bk, base + 3 * site);
        if (rw.ok) {
          const TripleCol c = cols[l * KMAX + column];
          v = c.p[(rw.row + colour) * c.ld];
          if (PHASE && l == 2) v = cmul(v, sg_phase(tab, g.ltab, 0, rw.x));
        }
      }
      sh[x] = v;
    }
    __syncthreads();
    for (int r = 0; r < R; ++r) {
      const double2* A = sh + r * 3 * E + ii;
      const double2* B = sh + PER + r * 3 * E + jj;
      const double2* C = sh + 2 * PER + r * 3 * E + k0;
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const int q1 = (q + 1) % 3, q2 = (q + 2) % 3;
        const double2 D = cross_term(A[q1 * E], B[q2 * E], A[q2 * E], B[q1 * E]);
        cfma(acc0, D, C[q * E]);
        cfma(acc1, D, C[q * E + 4]);
      }
    }
  }
  double2* const dst = partials + (static_cast<int64_t>(blockIdx.y) * gridDim.x + blockIdx.x) * (E * E * E);
  dst[(k0 * E + jj) * E + ii] = acc0;
  dst[((k0 + 4) * E + jj) * E + ii] = acc1;
}

// One thread per (listed slice, tile, entry of the tile)
__global__ void __launch_bounds__(256) k_basis_slice_triple_fold(int E, int n_tiles, int n_slices, int nbps, int identical, int Ka, int Kb,
                                                                 int Kc, int S, int p, const int* __restrict__ tiles,
                                                                 const int* __restrict__ list, const double2* __restrict__ partials,
                                                                 double2* __restrict__ out) {
  const int E3 = E * E * E;
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (idx >= static_cast<int64_t>(n_slices) * n_tiles * E3) return;
  const int e = static_cast<int>(idx % E3);
  const int64_t r = idx / E3;
  const int tile = static_cast<int>(r % n_tiles), s = static_cast<int>(r / n_tiles);
  const int kk = e / (E * E), jj = (e / E) % E, ii = e % E;
  const int i = E * tiles[3 * tile] + ii, j = E * tiles[3 * tile + 1] + jj, k = E * tiles[3 * tile + 2] + kk;
  if (i >= Ka || j >= Kb || k >= Kc) return;
  if (identical && !(i < j && j < k)) return;
  const double2* src = partials + ((static_cast<int64_t>(tile) * n_slices + s) * nbps) * E3 + e;
  double2 v = make_double2(0.0, 0.0);
  for (int b = 0; b < nbps; ++b) {
    const double2 x = src[static_cast<int64_t>(b) * E3];
    v.x += x.x;
    v.y += x.y;
  }
  double2* const o = out + (static_cast<int64_t>(p) * S + list[2 * s + 1]) * (static_cast<int64_t>(Ka) * Kb * Kc);
  o[(static_cast<int64_t>(k) * Kb + j) * Ka + i] = v;
  if (identical) {  // Ka == Kb == Kc
    const double2 m = make_double2(-v.x, -v.y);
    o[(static_cast<int64_t>(i) * Kb + k) * Ka + j] = v;  // (j, k, i)
    o[(static_cast<int64_t>(j) * Kb + i) * Ka + k] = v;  // (k, i, j)
    o[(static_cast<int64_t>(k) * Kb + i) * Ka + j] = m;  // (j, i, k)
    o[(static_cast<int64_t>(j) * Kb + k) * Ka + i] = m;  // (i, k, j)
    o[(static_cast<int64_t>(i) * Kb + j) * Ka + k] = m;  // (k, j, i)
  }
}

}  // namespace

void launch_basis_slice_triple(hipStream_t s, const LatticeDev& lat, int parity, int dir, const BasisSliceTriplePlan& plan, int n_slices,
                               const TripleCol* cols, int Ka, int Kb, int Kc, const int* tiles, const int* list, const double2* tab,
                               double2* partials) {
  const SGGeom g = slice_geom(lat, parity, dir, plan.walk);
  const dim3 grid(static_cast<unsigned>(plan.walk.nbps) * static_cast<unsigned>(n_slices), static_cast<unsigned>(plan.n_tiles()));
  if (plan.mfma) {
    if (tab) hipLaunchKernelGGL((k_basis_slice_triple_mfma<true>), grid, dim3(256), 0, s, g, cols, tiles, list, tab, partials);
    else hipLaunchKernelGGL((k_basis_slice_triple_mfma<false>), grid, dim3(256), 0, s, g, cols, tiles, list, tab, partials);
  } else {
    if (tab) hipLaunchKernelGGL((k_basis_slice_triple_generic<true>), grid, dim3(256), 0, s, g, cols, Ka, Kb, Kc, tiles, list, tab, partials);
    else hipLaunchKernelGGL((k_basis_slice_triple_generic<false>), grid, dim3(256), 0, s, g, cols, Ka, Kb, Kc, tiles, list, tab, partials);
  }
}

void launch_basis_slice_triple_fold(hipStream_t s, const BasisSliceTriplePlan& plan, int n_slices, int Ka, int Kb, int Kc, int S, int p,
                                    const int* tiles, const int* list, const double2* partials, double2* out) {
  const int64_t n = static_cast<int64_t>(n_slices) * plan.n_tiles() * plan.tile_entries();
  hipLaunchKernelGGL(k_basis_slice_triple_fold, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, s, plan.edge, plan.n_tiles(),
                     n_slices, plan.walk.nbps, plan.identical ? 1 : 0, Ka, Kb, Kc, S, p, tiles, list, partials, out);
}

}  // namespace bcg
