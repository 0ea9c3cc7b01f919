// The fermion force of a multi-shift solve (include/blockcg_hip.h, bcg_force_accumulate) for gfx950:
//
//   F(x, mu) += sum_s w_s G_s(x, mu),   G_s(x, mu) = eta_mu(x) sum_j [ Y_sj(x+mu) X_sj(x)^dagger - X_sj(x+mu) Y_sj(x)^dagger ]
//
// (or TA(U_mu(x) sum_s w_s G_s)), a 3 x 3 colour outer product per link summed over the m block columns.  A streaming
// kernel: per shift it reads X and Y at every site (the x + mu re-reads are left to the caches), and F once per launch.
//
// Work split: a GROUP of P lanes (P = m rounded up to a power of two, P <= 32 divides the wavefront) per (site, mu); lane j
// holds column j, so the loads of a row are 16 B per lane at consecutive addresses, and forms the 9 (or 18, full fields)
// complex products of its column for every shift of the launch, weighted, in registers.  The column sum is a butterfly over
// the group's lanes at the end (every lane then holds G); lane k % P writes element k of the link.  The neighbours of a
// group's site come from the ghost faces across a divided direction (full-field face numbering as in k_hop_generic, half
// faces as in k_hop_half).  FMAs on the VALU: about 3.5 flop per byte at m = 16, far below the fp64 ridge.
#include <hip/hip_runtime.h>

#include "kernels_force.hpp"

namespace bcg {

namespace {

// Site coordinates in 32-bit arithmetic
__device__ __forceinline__ void coords32(const LatticeDev& lat, unsigned site, int x[4]) {
  const unsigned L0 = lat.L[0], L1 = lat.L[1], L2 = lat.L[2];
  x[0] = static_cast<int>(site % L0); site /= L0;
  x[1] = static_cast<int>(site % L1); site /= L1;
  x[2] = static_cast<int>(site % L2); site /= L2;
  x[3] = static_cast<int>(site);
}
// lexicographic index of x over all directions except mu (the face numbering of the halo exchange)
__device__ __forceinline__ int64_t face_of(const LatticeDev& lat, const int x[4], int mu) {
  int64_t f = 0, st = 1;
#pragma unroll
  for (int nu = 0; nu < 4; ++nu) {
    if (nu == mu) continue;
    f += x[nu] * st;
    st *= lat.L[nu];
  }
  return f;
}
template <class T>
__device__ __forceinline__ T pick(const T (&a)[4], int mu) {
  return mu == 0 ? a[0] : mu == 1 ? a[1] : mu == 2 ? a[2] : a[3];
}
// a parity-compact (half) field's index of full-lattice site x (kernels_generic.hip, "Half-volume fields")
__device__ __forceinline__ int64_t half_of(const LatticeDev& lat, const int x[4]) {
  return (x[0] >> 1) + static_cast<int64_t>(lat.L[0] >> 1) * (x[1] + static_cast<int64_t>(lat.L[1]) * (x[2] + static_cast<int64_t>(lat.L[2]) * x[3]));
}

template <int P, bool HALF, bool PROJECT>
__global__ void __launch_bounds__(256) k_force(LatticeDev lat, int m, int parity, ForceShifts sh, const double2* __restrict__ U,
                                               double2* __restrict__ F) {
  const int lane = threadIdx.x & (P - 1);
  const int64_t groups = lat.V * lat.ndim;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * (blockDim.x / P);
  const int col = lane < m ? lane : 0;
  const double live = lane < m ? 1.0 : 0.0;
  const int row = 3 * m;
  const int origin_par = lat.origin[0] + lat.origin[1] + lat.origin[2] + lat.origin[3];
  for (int64_t g = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) / P; g < groups; g += stride) {
    const unsigned g32 = static_cast<unsigned>(g);  // (the host guarantees V_local * ndim < 2^31)
    const unsigned s32 = g32 / static_cast<unsigned>(lat.ndim);
    const int mu = static_cast<int>(g32 - s32 * lat.ndim);
    const int64_t site = s32;  // (row offsets in 64 bits)
    int x[4];
    coords32(lat, s32, x);
    const int64_t link = g;  // [site][mu]
    // (mu differs between the groups of a wavefront: entries of mu picked by selects, no dynamically indexed arrays)
    int eta_par = 0, xmu = 0;
#pragma unroll
    for (int nu = 0; nu < 4; ++nu) {
      if (nu < mu) eta_par += x[nu] + lat.origin[nu];
      if (nu == mu) xmu = x[nu];
    }
    const double eta = (eta_par & 1) ? -1.0 : 1.0;
    const int Lmu = pick(lat.L, mu);
    const bool at_end = xmu + 1 == Lmu;
    const bool ghost = at_end && pick(lat.split, mu);
    int xf[4];
#pragma unroll
    for (int nu = 0; nu < 4; ++nu) xf[nu] = nu == mu ? (at_end ? 0 : xmu + 1) : x[nu];
    const int64_t fi = ghost ? face_of(lat, x, mu) : 0;
    const int64_t plus_ghost = mu == 0 ? lat.ghost_off[0][1] : mu == 1 ? lat.ghost_off[1][1] : mu == 2 ? lat.ghost_off[2][1] : lat.ghost_off[3][1];

    double2 acc[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k] = make_double2(0.0, 0.0);
    // acc(r, c) += coef * a_r conj(b_c), this lane's column
    auto outer = [&](const double2* a, const double2* b, double coef) {
      double2 av[3], bv[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) {  // (lanes j >= m read column 0, in bounds, and drop it)
        av[r] = a[r * m + col];
        bv[r] = b[r * m + col];
        av[r].x *= coef * live;
        av[r].y *= coef * live;
      }
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          double2& t = acc[r * 3 + c];
          t.x = fma(av[r].x, bv[c].x, t.x);
          t.x = fma(av[r].y, bv[c].y, t.x);
          t.y = fma(av[r].y, bv[c].x, t.y);
          t.y = fma(-av[r].x, bv[c].y, t.y);
        }
    };

    if (!HALF) {
      const int64_t nb = site + (at_end ? -static_cast<int64_t>(Lmu - 1) : 1) * pick(lat.stride, mu);
      for (int s = 0; s < sh.n; ++s) {
        const double2* x0 = sh.X[s] + site * row;
        const double2* y0 = sh.Y[s] + site * row;
        const double2* x1 = ghost ? sh.Xg[s] + (plus_ghost + fi) * row : sh.X[s] + nb * row;
        const double2* y1 = ghost ? sh.Yg[s] + (plus_ghost + fi) * row : sh.Y[s] + nb * row;
        const double w = sh.w[s] * eta;
        outer(y1, x0, w);
        outer(x1, y0, -w);
      }
    } else {
      // x of the fields' parity: G = eta Y(x+mu) X(x)^dagger;  else G = -eta X(x+mu) Y(x)^dagger
      const bool on_x = ((x[0] + x[1] + x[2] + x[3] + origin_par) & 1) == parity;
      const int64_t h0 = half_of(lat, x);
      const int64_t h1 = ghost ? (plus_ghost >> 1) + (fi >> 1) : half_of(lat, xf);
      for (int s = 0; s < sh.n; ++s) {
        const double2* near = on_x ? sh.X[s] : sh.Y[s];
        const double2* far = ghost ? (on_x ? sh.Yg[s] : sh.Xg[s]) : (on_x ? sh.Y[s] : sh.X[s]);
        outer(far + h1 * row, near + h0 * row, on_x ? sh.w[s] * eta : -sh.w[s] * eta);
      }
    }
    // column sum over the group's lanes: every lane ends with G
#pragma unroll
    for (int off = 1; off < P; off <<= 1)
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        acc[k].x += __shfl_xor(acc[k].x, off, P);
        acc[k].y += __shfl_xor(acc[k].y, off, P);
      }
    double2* f = F + link * 9;  // [site][mu][9]
    if (PROJECT) {
      // M = U G;  TA(M) = (M - M^dagger) / 2 - tr(M - M^dagger) / 6
      const double2* u = U + link * 9;  // U(r, k) at k * 3 + r
      double2 M[9];
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          double2 t = make_double2(0.0, 0.0);
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            const double2 a = u[k * 3 + r], b = acc[k * 3 + c];
            t.x = fma(a.x, b.x, t.x);
            t.x = fma(-a.y, b.y, t.x);
            t.y = fma(a.x, b.y, t.y);
            t.y = fma(a.y, b.x, t.y);
          }
          M[r * 3 + c] = t;
        }
      const double tr3 = (M[0].y + M[4].y + M[8].y) / 3.0;  // tr(M - M^dagger) / 6 = i (sum Im M_rr) / 3
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const double2 a = M[r * 3 + c], b = M[c * 3 + r];
          acc[r * 3 + c] = make_double2(0.5 * (a.x - b.x), 0.5 * (a.y + b.y) - (r == c ? tr3 : 0.0));
        }
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c)
        if ((c * 3 + r) % P == lane) {  // column-major element (r, c)
          double2 v = f[c * 3 + r];
          v.x += acc[r * 3 + c].x;
          v.y += acc[r * 3 + c].y;
          f[c * 3 + r] = v;
        }
  }
}

template <int P>
void launch_p(hipStream_t s, int m, const LatticeDev& lat, int parity, const ForceShifts& sh, const double2* U, double2* F,
              bool project) {
  const int64_t threads = lat.V * lat.ndim * P;
  const int64_t want = (threads + 255) / 256;
  const unsigned grid = static_cast<unsigned>(want < 16384 ? want : 16384);
  if (parity < 0) {
    if (project) hipLaunchKernelGGL((k_force<P, false, true>), dim3(grid), dim3(256), 0, s, lat, m, parity, sh, U, F);
    else hipLaunchKernelGGL((k_force<P, false, false>), dim3(grid), dim3(256), 0, s, lat, m, parity, sh, U, F);
  } else {
    if (project) hipLaunchKernelGGL((k_force<P, true, true>), dim3(grid), dim3(256), 0, s, lat, m, parity, sh, U, F);
    else hipLaunchKernelGGL((k_force<P, true, false>), dim3(grid), dim3(256), 0, s, lat, m, parity, sh, U, F);
  }
}

}  // namespace

void launch_force(hipStream_t s, int m, const LatticeDev& lat, int parity, const ForceShifts& sh, const double2* U, double2* F,
                  bool project) {
  if (m <= 1) launch_p<1>(s, m, lat, parity, sh, U, F, project);
  else if (m <= 2) launch_p<2>(s, m, lat, parity, sh, U, F, project);
  else if (m <= 4) launch_p<4>(s, m, lat, parity, sh, U, F, project);
  else if (m <= 8) launch_p<8>(s, m, lat, parity, sh, U, F, project);
  else if (m <= 16) launch_p<16>(s, m, lat, parity, sh, U, F, project);
  else launch_p<32>(s, m, lat, parity, sh, U, F, project);
}

}  // namespace bcg
