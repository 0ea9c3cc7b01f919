// The covariant nearest-neighbour sum for gfx950 (include/blockcg_hip.h: bcg_dirac_shift_sum):
//
//   out(x) = c0 in(x) + sum_mu s_mu(x) [ f_mu U_mu(x) in(x+mu) + b_mu U_mu(x-mu)^dagger in(x-mu) ]
//
// Two forms with the same arithmetic per output element (term by term in the order mu = 0 forward, 0 backward, 1 forward
// ..., then c0), so they return the same bits:
//   k_shift_generic  lane = (site, column), three colour outputs, every link entry a global load (the addressing of
//                    k_hop_generic / k_hop_half, restated here because those files do not change)
//   k_shift_tile     m = 8, 16, 32 on 4-D full fields: a block covers 256 / m consecutive x0 sites; their forward links
//                    are one contiguous stretch of 576 B per site, staged with the backward links of the active directions
//                    into LDS by 16-byte cooperative loads; every lane then reads a link entry once from LDS.  Neighbour
//                    rows are 16-byte global loads, those of direction mu + 1 issued before the FMAs of direction mu.
// A direction whose two coefficients are exactly zero is skipped by a wave-uniform branch (the coefficients are kernel
// arguments): neither its links nor its neighbour rows are read.
#include <hip/hip_runtime.h>

#include "complex_ops.hpp"
#include "kernels_shift.hpp"

namespace bcg {

namespace {

// acc += w * (U psi): u[k * 3 + r] = U(r, k), the links' column-major storage
__device__ __forceinline__ void term_fwd(double2 acc[3], double2 w, const double2* u, const double2 psi[3]) {
  double2 t[3] = {make_double2(0, 0), make_double2(0, 0), make_double2(0, 0)};
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int r = 0; r < 3; ++r) cfma(t[r], u[k * 3 + r], psi[k]);
#pragma unroll
  for (int r = 0; r < 3; ++r) cfma(acc[r], w, t[r]);
}
// acc += w * (U^dagger psi): (U^dagger)(r, k) = conj(U(k, r)) = conj(u[r * 3 + k])
__device__ __forceinline__ void term_bwd(double2 acc[3], double2 w, const double2* u, const double2 psi[3]) {
  double2 t[3] = {make_double2(0, 0), make_double2(0, 0), make_double2(0, 0)};
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int r = 0; r < 3; ++r) cfma_conj(t[r], u[r * 3 + k], psi[k]);
#pragma unroll
  for (int r = 0; r < 3; ++r) cfma(acc[r], w, t[r]);
}

__device__ __forceinline__ void site_coords(const LatticeDev& lat, int64_t site, int x[4]) {
  x[0] = static_cast<int>(site % lat.L[0]); site /= lat.L[0];
  x[1] = static_cast<int>(site % lat.L[1]); site /= lat.L[1];
  x[2] = static_cast<int>(site % lat.L[2]); site /= lat.L[2];
  x[3] = static_cast<int>(site);
}
// half site h of parity `parity` -> coordinates (the numbering of k_hop_half: x0 compact)
__device__ __forceinline__ void half_coords(const LatticeDev& lat, int64_t h, int parity, int x[4]) {
  const int h0 = lat.L[0] >> 1;
  const int k = static_cast<int>(h % h0); h /= h0;
  x[1] = static_cast<int>(h % lat.L[1]); h /= lat.L[1];
  x[2] = static_cast<int>(h % lat.L[2]); h /= lat.L[2];
  x[3] = static_cast<int>(h);
  const int o = lat.origin[0] + lat.origin[1] + lat.origin[2] + lat.origin[3];
  x[0] = 2 * k + ((x[1] + x[2] + x[3] + parity + o) & 1);
}
__device__ __forceinline__ int64_t full_index(const LatticeDev& lat, const int x[4]) {
  return x[0] + static_cast<int64_t>(lat.L[0]) * (x[1] + static_cast<int64_t>(lat.L[1]) * (x[2] + static_cast<int64_t>(lat.L[2]) * x[3]));
}
__device__ __forceinline__ int64_t half_index(const LatticeDev& lat, const int x[4]) {
  return (x[0] >> 1) + static_cast<int64_t>(lat.L[0] >> 1) * (x[1] + static_cast<int64_t>(lat.L[1]) * (x[2] + static_cast<int64_t>(lat.L[2]) * x[3]));
}
// lexicographic index of x over all directions except mu (the numbering of the ghost faces)
template <int MU>
__device__ __forceinline__ int64_t face_index(const LatticeDev& lat, const int x[4]) {
  int64_t f = 0, st = 1;
#pragma unroll
  for (int nu = 0; nu < 4; ++nu) {
    if (nu == MU) continue;
    f += x[nu] * st;
    st *= lat.L[nu];
  }
  return f;
}
// index (full or half numbering) of the site x with x[MU] replaced by v
template <int MU, bool HALF>
__device__ __forceinline__ int64_t index_with(const LatticeDev& lat, const int x[4], int v) {
  int y[4] = {x[0], x[1], x[2], x[3]};
  y[MU] = v;
  return HALF ? half_index(lat, y) : full_index(lat, y);
}

// ---------------------------------------------------------------------------------------------
// Generic form.  One direction of one lane: rows and links straight from global memory.
// ---------------------------------------------------------------------------------------------
template <int M, bool HALF, int MU>
__device__ __forceinline__ void generic_dir(const LatticeDev& lat, const int x[4], int64_t site, int j, int par,
                                            const double2* __restrict__ U, const double2* __restrict__ Ughost,
                                            const double2* __restrict__ in, const double2* __restrict__ ghost,
                                            const ShiftCoef& cf, double2 acc[3]) {
  const bool fa = (cf.fa >> MU) & 1, ba = (cf.ba >> MU) & 1;
  if (!(fa || ba)) return;  // wave-uniform: nothing of this direction is read
  const double sg = (cf.eta != 0 && (par & 1)) ? -1.0 : 1.0;
  const int Lm = lat.L[MU];
  const bool hi = x[MU] + 1 == Lm, lo = x[MU] == 0;
  const bool split = lat.split[MU] != 0;
  const int64_t fi = split ? face_index<MU>(lat, x) : 0;
  if (fa) {
    const double2* pf;
    if (hi && split) pf = ghost + (HALF ? (lat.ghost_off[MU][1] >> 1) + (fi >> 1) : lat.ghost_off[MU][1] + fi) * 3 * M;
    else pf = in + index_with<MU, HALF>(lat, x, hi ? 0 : x[MU] + 1) * 3 * M;
    const double2 psi[3] = {pf[j], pf[M + j], pf[2 * M + j]};
    const double2 w = make_double2(sg * cf.f[MU].x, sg * cf.f[MU].y);
    term_fwd(acc, w, U + (site * lat.ndim + MU) * 9, psi);
  }
  if (ba) {
    const double2* pb;
    const double2* ub;
    if (lo && split) {
      pb = ghost + (HALF ? (lat.ghost_off[MU][0] >> 1) + (fi >> 1) : lat.ghost_off[MU][0] + fi) * 3 * M;
      ub = Ughost + (lat.ghost_off[MU][0] + fi) * 9;  // the gauge ghost keeps the full face numbering
    } else {
      const int xb = lo ? Lm - 1 : x[MU] - 1;
      pb = in + index_with<MU, HALF>(lat, x, xb) * 3 * M;
      ub = U + (index_with<MU, false>(lat, x, xb) * lat.ndim + MU) * 9;
    }
    const double2 psi[3] = {pb[j], pb[M + j], pb[2 * M + j]};
    const double2 w = make_double2(sg * cf.b[MU].x, sg * cf.b[MU].y);
    term_bwd(acc, w, ub, psi);
  }
}

template <int M, bool HALF>
__global__ void __launch_bounds__(256) k_shift_generic(LatticeDev lat, int parity, const double2* __restrict__ U,
                                                       const double2* __restrict__ Ughost, const double2* __restrict__ in,
                                                       const double2* __restrict__ ghost, double2* __restrict__ out,
                                                       ShiftCoef cf) {
  constexpr int SPB = 256 / M;  // sites per block
  const int sl = threadIdx.x / M;
  const int j = threadIdx.x - sl * M;
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * SPB + sl;  // site of `out` in its own numbering
  if (sl >= SPB || idx >= (HALF ? lat.V / 2 : lat.V)) return;
  int x[4];
  if (HALF) half_coords(lat, idx, parity, x);
  else site_coords(lat, idx, x);
  const int64_t site = HALF ? full_index(lat, x) : idx;
  double2 acc[3] = {make_double2(0, 0), make_double2(0, 0), make_double2(0, 0)};
  int par = 0;  // x_0 + ... + x_{mu-1} (global)
  generic_dir<M, HALF, 0>(lat, x, site, j, par, U, Ughost, in, ghost, cf, acc);
  par += x[0] + lat.origin[0];
  if (lat.ndim > 1) generic_dir<M, HALF, 1>(lat, x, site, j, par, U, Ughost, in, ghost, cf, acc);
  par += x[1] + lat.origin[1];
  if (lat.ndim > 2) generic_dir<M, HALF, 2>(lat, x, site, j, par, U, Ughost, in, ghost, cf, acc);
  par += x[2] + lat.origin[2];
  if (lat.ndim > 3) generic_dir<M, HALF, 3>(lat, x, site, j, par, U, Ughost, in, ghost, cf, acc);
  if (!HALF && cf.use_c0) {
#pragma unroll
    for (int r = 0; r < 3; ++r) cfma(acc[r], cf.c0, in[(idx * 3 + r) * M + j]);
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) out[(idx * 3 + r) * M + j] = acc[r];
}

// ---------------------------------------------------------------------------------------------
// Tile form.  R = 256 / M consecutive x0 sites per block (L0 a multiple of R, direction 0 not divided, 4-D full fields).
// LDS: lf[s * 36 + mu * 9 + e] the forward links in their storage order, lb[(mu * R + s) * 9 + e] = U_mu(x_s - mu).
// ---------------------------------------------------------------------------------------------
struct NbrRows {
  double2 f[3], b[3];
};

template <int M, int MU>
__device__ __forceinline__ NbrRows tile_rows(const LatticeDev& lat, const int x[4], int j, const double2* __restrict__ in,
                                             const double2* __restrict__ ghost, const ShiftCoef& cf) {
  NbrRows n;
#pragma unroll
  for (int k = 0; k < 3; ++k) n.f[k] = n.b[k] = make_double2(0, 0);
  const bool fa = (cf.fa >> MU) & 1, ba = (cf.ba >> MU) & 1;
  if (!(fa || ba)) return n;
  const int Lm = lat.L[MU];
  const bool hi = x[MU] + 1 == Lm, lo = x[MU] == 0;
  const bool split = MU > 0 && lat.split[MU] != 0;  // (the tile form declines a divided direction 0)
  const int64_t fi = split ? face_index<MU>(lat, x) : 0;
  if (fa) {
    const double2* pf;
    if (hi && split) pf = ghost + (lat.ghost_off[MU][1] + fi) * 3 * M;
    else pf = in + index_with<MU, false>(lat, x, hi ? 0 : x[MU] + 1) * 3 * M;
#pragma unroll
    for (int k = 0; k < 3; ++k) n.f[k] = pf[k * M + j];
  }
  if (ba) {
    const double2* pb;
    if (lo && split) pb = ghost + (lat.ghost_off[MU][0] + fi) * 3 * M;
    else pb = in + index_with<MU, false>(lat, x, lo ? Lm - 1 : x[MU] - 1) * 3 * M;
#pragma unroll
    for (int k = 0; k < 3; ++k) n.b[k] = pb[k * M + j];
  }
  return n;
}

template <int R, int MU>
__device__ __forceinline__ void tile_terms(const NbrRows& n, int sl, int par, const double2* lf, const double2* lb,
                                           const ShiftCoef& cf, double2 acc[3]) {
  const bool fa = (cf.fa >> MU) & 1, ba = (cf.ba >> MU) & 1;
  if (!(fa || ba)) return;
  const double sg = (cf.eta != 0 && (par & 1)) ? -1.0 : 1.0;
  if (fa) term_fwd(acc, make_double2(sg * cf.f[MU].x, sg * cf.f[MU].y), lf + sl * 36 + MU * 9, n.f);
  if (ba) term_bwd(acc, make_double2(sg * cf.b[MU].x, sg * cf.b[MU].y), lb + (MU * R + sl) * 9, n.b);
}

template <int M>
__global__ void __launch_bounds__(256) k_shift_tile(LatticeDev lat, const double2* __restrict__ U,
                                                    const double2* __restrict__ Ughost, const double2* __restrict__ in,
                                                    const double2* __restrict__ ghost, double2* __restrict__ out,
                                                    ShiftCoef cf) {
  constexpr int R = 256 / M;
  __shared__ double2 lf[R * 36];
  __shared__ double2 lb[4 * R * 9];
  const int tid = threadIdx.x;
  const int64_t first = static_cast<int64_t>(blockIdx.x) * R;  // first site of the run; the grid is exactly V / R blocks
  int x0[4];                                                   // its coordinates
  site_coords(lat, first, x0);

  // ---- stage the links: forward ones in storage order (contiguous when every direction is active), then U_mu(x - mu) ----
  if (cf.fa) {
    const double2* src = U + first * 36;
    for (int u = tid; u < R * 36; u += 256) {
      const int mu = (u % 36) / 9;
      if ((cf.fa >> mu) & 1) lf[u] = src[u];
    }
  }
  if (cf.ba) {
    for (int v = tid; v < 4 * R * 9; v += 256) {
      const int mu = v / (R * 9);
      if (!((cf.ba >> mu) & 1)) continue;
      const int rem = v - mu * (R * 9);
      const int s = rem / 9, e = rem - s * 9;
      int y[4] = {x0[0] + s, x0[1], x0[2], x0[3]};
      const int ym = mu == 0 ? y[0] : (mu == 1 ? y[1] : (mu == 2 ? y[2] : y[3]));
      const int Lm = mu == 0 ? lat.L[0] : (mu == 1 ? lat.L[1] : (mu == 2 ? lat.L[2] : lat.L[3]));
      const bool split = mu > 0 && (mu == 1 ? lat.split[1] : (mu == 2 ? lat.split[2] : lat.split[3])) != 0;
      const double2* p;
      if (ym == 0 && split) {
        int64_t fi;
        int64_t off;
        if (mu == 1) { fi = face_index<1>(lat, y); off = lat.ghost_off[1][0]; }
        else if (mu == 2) { fi = face_index<2>(lat, y); off = lat.ghost_off[2][0]; }
        else { fi = face_index<3>(lat, y); off = lat.ghost_off[3][0]; }
        p = Ughost + (off + fi) * 9 + e;
      } else {
        const int yb = ym == 0 ? Lm - 1 : ym - 1;
        if (mu == 0) y[0] = yb;
        else if (mu == 1) y[1] = yb;
        else if (mu == 2) y[2] = yb;
        else y[3] = yb;
        p = U + (full_index(lat, y) * 4 + mu) * 9 + e;
      }
      lb[v] = *p;
    }
  }

  const int sl = tid / M;
  const int j = tid - sl * M;
  const int x[4] = {x0[0] + sl, x0[1], x0[2], x0[3]};
  const int64_t site = first + sl;
  const int p1 = x[0] + lat.origin[0];
  const int p2 = p1 + x[1] + lat.origin[1];
  const int p3 = p2 + x[2] + lat.origin[2];
  double2 self[3] = {make_double2(0, 0), make_double2(0, 0), make_double2(0, 0)};
  if (cf.use_c0) {
#pragma unroll
    for (int r = 0; r < 3; ++r) self[r] = in[(site * 3 + r) * M + j];
  }
  // rows of direction mu + 1 are in flight while the terms of direction mu run
  NbrRows n0 = tile_rows<M, 0>(lat, x, j, in, ghost, cf);
  NbrRows n1 = tile_rows<M, 1>(lat, x, j, in, ghost, cf);
  __syncthreads();  // the links are in LDS
  double2 acc[3] = {make_double2(0, 0), make_double2(0, 0), make_double2(0, 0)};
  tile_terms<R, 0>(n0, sl, 0, lf, lb, cf, acc);
  n0 = tile_rows<M, 2>(lat, x, j, in, ghost, cf);
  tile_terms<R, 1>(n1, sl, p1, lf, lb, cf, acc);
  n1 = tile_rows<M, 3>(lat, x, j, in, ghost, cf);
  tile_terms<R, 2>(n0, sl, p2, lf, lb, cf, acc);
  tile_terms<R, 3>(n1, sl, p3, lf, lb, cf, acc);
  if (cf.use_c0) {
#pragma unroll
    for (int r = 0; r < 3; ++r) cfma(acc[r], cf.c0, self[r]);
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) out[(site * 3 + r) * M + j] = acc[r];
}

#define BCG_SHIFT_CASE(MM, ...) \
  case MM: {                    \
    constexpr int M = MM;       \
    __VA_ARGS__;                \
    break;                      \
  }
#define BCG_SHIFT_DISPATCH_M(m, ...)                                                                                      \
  switch (m) {                                                                                                            \
    BCG_SHIFT_CASE(1, __VA_ARGS__) BCG_SHIFT_CASE(2, __VA_ARGS__) BCG_SHIFT_CASE(3, __VA_ARGS__) BCG_SHIFT_CASE(4, __VA_ARGS__)     \
    BCG_SHIFT_CASE(5, __VA_ARGS__) BCG_SHIFT_CASE(6, __VA_ARGS__) BCG_SHIFT_CASE(7, __VA_ARGS__) BCG_SHIFT_CASE(8, __VA_ARGS__)     \
    BCG_SHIFT_CASE(9, __VA_ARGS__) BCG_SHIFT_CASE(10, __VA_ARGS__) BCG_SHIFT_CASE(11, __VA_ARGS__) BCG_SHIFT_CASE(12, __VA_ARGS__)  \
    BCG_SHIFT_CASE(13, __VA_ARGS__) BCG_SHIFT_CASE(14, __VA_ARGS__) BCG_SHIFT_CASE(15, __VA_ARGS__) BCG_SHIFT_CASE(16, __VA_ARGS__) \
    BCG_SHIFT_CASE(17, __VA_ARGS__) BCG_SHIFT_CASE(18, __VA_ARGS__) BCG_SHIFT_CASE(19, __VA_ARGS__) BCG_SHIFT_CASE(20, __VA_ARGS__) \
    BCG_SHIFT_CASE(21, __VA_ARGS__) BCG_SHIFT_CASE(22, __VA_ARGS__) BCG_SHIFT_CASE(23, __VA_ARGS__) BCG_SHIFT_CASE(24, __VA_ARGS__) \
    BCG_SHIFT_CASE(25, __VA_ARGS__) BCG_SHIFT_CASE(26, __VA_ARGS__) BCG_SHIFT_CASE(27, __VA_ARGS__) BCG_SHIFT_CASE(28, __VA_ARGS__) \
    BCG_SHIFT_CASE(29, __VA_ARGS__) BCG_SHIFT_CASE(30, __VA_ARGS__) BCG_SHIFT_CASE(31, __VA_ARGS__) BCG_SHIFT_CASE(32, __VA_ARGS__) \
    default: break;                                                                                                       \
  }

}  // namespace

void launch_shift_generic(hipStream_t s, int m, const LatticeDev& lat, int parity, const double2* U, const double2* Ughost,
                          const double2* in, const double2* ghost, double2* out, const ShiftCoef& cf) {
  BCG_SHIFT_DISPATCH_M(m, {
    constexpr int SPB = 256 / M;
    const int64_t n = parity >= 0 ? lat.V / 2 : lat.V;
    const unsigned grid = static_cast<unsigned>((n + SPB - 1) / SPB);
    if (parity >= 0)
      hipLaunchKernelGGL((k_shift_generic<M, true>), dim3(grid), dim3(SPB * M), 0, s, lat, parity, U, Ughost, in, ghost, out, cf);
    else
      hipLaunchKernelGGL((k_shift_generic<M, false>), dim3(grid), dim3(SPB * M), 0, s, lat, parity, U, Ughost, in, ghost, out, cf);
  });
}

int shift_tile_sites(int m) { return (m == 8 || m == 16 || m == 32) ? 256 / m : 0; }

bool shift_tile_ok(int m, const LatticeDev& lat) {
  const int r = shift_tile_sites(m);
  return r > 0 && lat.ndim == 4 && lat.L[0] % r == 0 && !lat.split[0];
}

void launch_shift_tile(hipStream_t s, int m, const LatticeDev& lat, const double2* U, const double2* Ughost, const double2* in,
                       const double2* ghost, double2* out, const ShiftCoef& cf) {
  const unsigned grid = static_cast<unsigned>(lat.V / shift_tile_sites(m));
  if (m == 8) hipLaunchKernelGGL((k_shift_tile<8>), dim3(grid), dim3(256), 0, s, lat, U, Ughost, in, ghost, out, cf);
  else if (m == 16) hipLaunchKernelGGL((k_shift_tile<16>), dim3(grid), dim3(256), 0, s, lat, U, Ughost, in, ghost, out, cf);
  else hipLaunchKernelGGL((k_shift_tile<32>), dim3(grid), dim3(256), 0, s, lat, U, Ughost, in, ghost, out, cf);
}

}  // namespace bcg
