// Stout link smearing and the plaquette for gfx950 (include/blockcg_hip.h, "gauge links: stout smearing and plaquettes";
// DESIGN.md section 8m):
//
//   C_mu(x)  = sum_{nu != mu} rho[mu][nu] [ U_nu(x) U_mu(x+nu) U_nu(x+mu)^dagger + W_{mu nu}(x-nu) ],
//   W_{mu nu}(y) = U_nu(y)^dagger U_mu(y) U_nu(y+mu),
//   Omega = C_mu(x) U_mu(x)^dagger,  Q = (i/2)(Omega^dagger - Omega) - (i/6) tr(Omega^dagger - Omega),  U'_mu(x) = exp(iQ) U_mu(x).
//
// Work split: one thread per site; it walks mu and nu (uniform over the launch, so a zero rho[mu][nu] is a uniform branch
// that reads nothing) and keeps the staple sum, one product and one operand in registers: 3 x 3 complex products as FMAs on
// the VALU, no LDS.  The neighbours are read straight through the caches: the links of a site are one 144 ndim byte row, and
// consecutive lanes hold consecutive sites, so a wavefront's loads of one matrix cover whole rows between them.
// exp(iQ) in the Cayley-Hamilton form of Morningstar and Peardon, f0 + f1 Q + f2 Q^2, with the guards of the header comment.
// Index arithmetic: 32-bit site decomposition, 64-bit row offsets, per-direction entries picked by selects.
#include <hip/hip_runtime.h>

#include "kernels_gauge_smear.hpp"

namespace bcg {

namespace {

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
__device__ __forceinline__ int64_t site_of_face(const LatticeDev& lat, int64_t f, int mu, int xmu, int x[4]) {
  int64_t site = 0;
#pragma unroll
  for (int nu = 0; nu < 4; ++nu) {
    int v;
    if (nu == mu) {
      v = xmu;
    } else {
      v = static_cast<int>(f % lat.L[nu]);
      f /= lat.L[nu];
    }
    x[nu] = v;
    site += v * lat.stride[nu];
  }
  return site;
}
template <class T>
__device__ __forceinline__ T pick(const T (&a)[4], int mu) {
  return mu == 0 ? a[0] : mu == 1 ? a[1] : mu == 2 ? a[2] : a[3];
}
__device__ __forceinline__ int coord(const int x[4], int mu) { return mu == 0 ? x[0] : mu == 1 ? x[1] : mu == 2 ? x[2] : x[3]; }
__device__ __forceinline__ int64_t ghost_first(const LatticeDev& lat, int mu, int side) {
  return mu == 0 ? lat.ghost_off[0][side] : mu == 1 ? lat.ghost_off[1][side] : mu == 2 ? lat.ghost_off[2][side] : lat.ghost_off[3][side];
}

// rho[mu][nu] by selects (mu and nu are uniform, the table sits in scalar registers: no dynamically indexed copy of it)
__device__ __forceinline__ double rho_of(const StoutArgs& a, int mu, int nu) {
  double r = 0.0;
#pragma unroll
  for (int k = 0; k < 16; ++k) r = (mu * 4 + nu == k) ? a.rho[k] : r;
  return r;
}

// ---- 3 x 3 complex matrices in registers, e[r * 3 + c] ------------------------------------------------------------------
struct M3 {
  double2 e[9];
};
__device__ __forceinline__ M3 load(const double2* __restrict__ p) {  // memory: column-major, M(r, c) at c * 3 + r
  M3 m;
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int r = 0; r < 3; ++r) m.e[r * 3 + c] = p[c * 3 + r];
  return m;
}
__device__ __forceinline__ void store(double2* __restrict__ p, const M3& m) {
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int r = 0; r < 3; ++r) p[c * 3 + r] = m.e[r * 3 + c];
}
// t += a * b  /  t += a * conj(b)  /  t += conj(a) * b
__device__ __forceinline__ void cfma(double2& t, const double2 a, const double2 b) {
  t.x = fma(a.x, b.x, t.x);
  t.x = fma(-a.y, b.y, t.x);
  t.y = fma(a.x, b.y, t.y);
  t.y = fma(a.y, b.x, t.y);
}
__device__ __forceinline__ void cfma_cb(double2& t, const double2 a, const double2 b) {
  t.x = fma(a.x, b.x, t.x);
  t.x = fma(a.y, b.y, t.x);
  t.y = fma(a.y, b.x, t.y);
  t.y = fma(-a.x, b.y, t.y);
}
__device__ __forceinline__ M3 mul(const M3& a, const M3& b) {  // a b
  M3 o;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      double2 t = make_double2(0.0, 0.0);
#pragma unroll
      for (int k = 0; k < 3; ++k) cfma(t, a.e[r * 3 + k], b.e[k * 3 + c]);
      o.e[r * 3 + c] = t;
    }
  return o;
}
__device__ __forceinline__ M3 mul_nd(const M3& a, const M3& b) {  // a b^dagger
  M3 o;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      double2 t = make_double2(0.0, 0.0);
#pragma unroll
      for (int k = 0; k < 3; ++k) cfma_cb(t, a.e[r * 3 + k], b.e[c * 3 + k]);
      o.e[r * 3 + c] = t;
    }
  return o;
}
__device__ __forceinline__ M3 mul_dn(const M3& a, const M3& b) {  // a^dagger b
  M3 o;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      double2 t = make_double2(0.0, 0.0);
#pragma unroll
      for (int k = 0; k < 3; ++k) cfma_cb(t, b.e[k * 3 + c], a.e[k * 3 + r]);
      o.e[r * 3 + c] = t;
    }
  return o;
}
__device__ __forceinline__ void add_scaled(M3& acc, double w, const M3& m) {
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    acc.e[k].x = fma(w, m.e[k].x, acc.e[k].x);
    acc.e[k].y = fma(w, m.e[k].y, acc.e[k].y);
  }
}

// U_comp(x + d): the row of the plus neighbour in direction d of site x (periodic, or the plus ghost of a divided direction)
__device__ __forceinline__ const double2* plus_link(const LatticeDev& lat, const double2* __restrict__ U,
                                                    const double2* __restrict__ link_ghost, int64_t site, const int x[4], int d,
                                                    int comp) {
  const int nd = lat.ndim;
  const int Ld = pick(lat.L, d);
  const int64_t st = pick(lat.stride, d);
  if (coord(x, d) + 1 == Ld) {
    if (pick(lat.split, d)) return link_ghost + ((ghost_first(lat, d, 1) + face_of(lat, x, d)) * nd + comp) * 9;
    return U + ((site - static_cast<int64_t>(Ld - 1) * st) * nd + comp) * 9;
  }
  return U + ((site + st) * nd + comp) * 9;
}

// W_{mu nu}(y) = U_nu(y)^dagger U_mu(y) U_nu(y+mu)
__device__ __forceinline__ M3 backward_staple(const LatticeDev& lat, const double2* __restrict__ U,
                                              const double2* __restrict__ link_ghost, int64_t ysite, const int y[4], int mu, int nu) {
  const int nd = lat.ndim;
  const M3 a = load(U + (ysite * nd + nu) * 9);
  const M3 b = load(U + (ysite * nd + mu) * 9);
  const M3 t = mul_dn(a, b);
  const M3 d = load(plus_link(lat, U, link_ghost, ysite, y, mu, nu));
  return mul(t, d);
}

// exp(iQ) = f0 + f1 Q + f2 Q^2 for Hermitian traceless Q (Morningstar and Peardon, Phys. Rev. D 69, 054501, eqs. 19-33)
__device__ __forceinline__ M3 exp_iq(const M3& Q) {
  const M3 Q2 = mul(Q, Q);
  // c0 = det Q (real), c1 = tr Q^2 / 2
  auto cm = [](const double2 a, const double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); };
  const double2 m0 = cm(Q.e[4], Q.e[8]), m0b = cm(Q.e[5], Q.e[7]);
  const double2 m1 = cm(Q.e[3], Q.e[8]), m1b = cm(Q.e[5], Q.e[6]);
  const double2 m2 = cm(Q.e[3], Q.e[7]), m2b = cm(Q.e[4], Q.e[6]);
  const double2 d0 = make_double2(m0.x - m0b.x, m0.y - m0b.y);
  const double2 d1 = make_double2(m1.x - m1b.x, m1.y - m1b.y);
  const double2 d2 = make_double2(m2.x - m2b.x, m2.y - m2b.y);
  const double c0 = cm(Q.e[0], d0).x - cm(Q.e[1], d1).x + cm(Q.e[2], d2).x;
  double c1 = 0.5 * (Q2.e[0].x + Q2.e[4].x + Q2.e[8].x);
  c1 = c1 > 0.0 ? c1 : 0.0;
  const double third = c1 / 3.0;
  const double c0max = 2.0 * third * sqrt(third);
  double f0r = 1.0, f0i = 0.0, f1r = 0.0, f1i = 0.0, f2r = 0.0, f2i = 0.0;
  if (c0max > 0.0) {
    double ratio = fabs(c0) / c0max;
    ratio = ratio < 1.0 ? ratio : 1.0;
    ratio = ratio > 0.0 ? ratio : 0.0;  // (also takes a NaN to 0)
    const double theta = acos(ratio);
    const double u = sqrt(third) * cos(theta / 3.0);
    const double w = sqrt(c1) * sin(theta / 3.0);
    const double u2 = u * u, w2 = w * w;
    double sw, cw;
    sincos(w, &sw, &cw);
    const double xi0 = fabs(w) < 0.05 ? 1.0 - w2 / 6.0 * (1.0 - w2 / 20.0 * (1.0 - w2 / 42.0)) : sw / w;
    double s2, c2, s1, c1u;
    sincos(2.0 * u, &s2, &c2);  // e^{2iu}
    sincos(u, &s1, &c1u);       // e^{-iu} = (c1u, -s1)
    // h0 = (u2 - w2) e^{2iu} + e^{-iu} [ 8 u2 cos w + 2 i u (3 u2 + w2) xi0 ]
    const double a0 = 8.0 * u2 * cw, b0 = 2.0 * u * (3.0 * u2 + w2) * xi0;
    const double h0r = (u2 - w2) * c2 + (c1u * a0 + s1 * b0);
    const double h0i = (u2 - w2) * s2 + (c1u * b0 - s1 * a0);
    // h1 = 2 u e^{2iu} - e^{-iu} [ 2 u cos w - i (3 u2 - w2) xi0 ]
    const double a1 = 2.0 * u * cw, b1 = -(3.0 * u2 - w2) * xi0;
    const double h1r = 2.0 * u * c2 - (c1u * a1 + s1 * b1);
    const double h1i = 2.0 * u * s2 - (c1u * b1 - s1 * a1);
    // h2 = e^{2iu} - e^{-iu} [ cos w + 3 i u xi0 ]
    const double a2 = cw, b2 = 3.0 * u * xi0;
    const double h2r = c2 - (c1u * a2 + s1 * b2);
    const double h2i = s2 - (c1u * b2 - s1 * a2);
    const double den = 9.0 * u2 - w2;
    if (den > 0.0) {
      const double inv = 1.0 / den;
      // c0 < 0: f_j(-c0) = (-1)^j conj f_j(c0)
      const double sg = c0 < 0.0 ? -1.0 : 1.0;
      f0r = h0r * inv; f0i = sg * h0i * inv;
      f1r = sg * h1r * inv; f1i = h1i * inv;
      f2r = h2r * inv; f2i = sg * h2i * inv;
    }
  }
  M3 E;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const double2 q = Q.e[k], q2 = Q2.e[k];
    double2 t = make_double2((k % 4 == 0) ? f0r : 0.0, (k % 4 == 0) ? f0i : 0.0);
    cfma(t, make_double2(f1r, f1i), q);
    cfma(t, make_double2(f2r, f2i), q2);
    E.e[k] = t;
  }
  return E;
}

// (mu and nu are unrolled at compile time: every per-direction entry of the geometry is then a scalar register, where a
// run-time direction makes hipcc keep a dynamically indexed copy of the whole struct in scratch)
template <int NDIM>
__global__ void __launch_bounds__(256) k_stout_step(LatticeDev lat, StoutArgs a, const double2* __restrict__ U,
                                                    const double2* __restrict__ link_ghost, const double2* __restrict__ w_ghost,
                                                    double2* __restrict__ out) {
  constexpr int nd = NDIM;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t s = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; s < lat.V; s += stride) {
    int x[4];
    coords32(lat, static_cast<unsigned>(s), x);  // (the host guarantees V_local * ndim < 2^31)
#pragma unroll
    for (int mu = 0; mu < nd; ++mu) {
      const double2* um = U + (s * nd + mu) * 9;
      double2* om = out + (s * nd + mu) * 9;
      if (!((a.smear_mask >> mu) & 1)) {  // copied bit for bit
#pragma unroll
        for (int k = 0; k < 9; ++k) om[k] = um[k];
        continue;
      }
      M3 C;
#pragma unroll
      for (int k = 0; k < 9; ++k) C.e[k] = make_double2(0.0, 0.0);
#pragma unroll
      for (int nu = 0; nu < nd; ++nu) {
        const double r = rho_of(a, mu, nu);
        if (nu == mu || r == 0.0) continue;
        {  // forward: U_nu(x) U_mu(x+nu) U_nu(x+mu)^dagger
          const M3 p = load(U + (s * nd + nu) * 9);
          const M3 q = load(plus_link(lat, U, link_ghost, s, x, nu, mu));
          const M3 t = mul(p, q);
          const M3 d = load(plus_link(lat, U, link_ghost, s, x, mu, nu));
          add_scaled(C, r, mul_nd(t, d));
        }
        // backward: W_{mu nu}(x - nu), from the minus neighbour's rank across a divided nu
        const int xn = coord(x, nu);
        if (xn == 0 && pick(lat.split, nu)) {
          const int slot = mu < nu ? mu : mu - 1;
          add_scaled(C, r, load(w_ghost + ((ghost_first(lat, nu, 0) + face_of(lat, x, nu)) * (nd - 1) + slot) * 9));
        } else {
          const int Ln = pick(lat.L, nu);
          const int64_t ys = s + (xn == 0 ? static_cast<int64_t>(Ln - 1) : -1) * pick(lat.stride, nu);
          int y[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) y[k] = k == nu ? (xn == 0 ? Ln - 1 : xn - 1) : x[k];
          add_scaled(C, r, backward_staple(lat, U, link_ghost, ys, y, mu, nu));
        }
      }
      const M3 Um = load(um);
      const M3 Om = mul_nd(C, Um);
      // Q = (i/2)(Omega^dagger - Omega) - (i/6) tr(Omega^dagger - Omega): Hermitian and traceless for any Omega
      const double tr3 = (Om.e[0].y + Om.e[4].y + Om.e[8].y) / 3.0;
      M3 Q;
#pragma unroll
      for (int rr = 0; rr < 3; ++rr)
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) {
          const double2 o = Om.e[rr * 3 + cc], ot = Om.e[cc * 3 + rr];
          // (i/2) (conj(ot) - o)
          Q.e[rr * 3 + cc] = make_double2(0.5 * (ot.y + o.y) - (rr == cc ? tr3 : 0.0), 0.5 * (ot.x - o.x));
        }
      store(om, mul(exp_iq(Q), Um));
    }
  }
}

// W on the high face of the divided direction NU: one thread per face site
template <int NDIM, int NU>
__device__ __forceinline__ void w_face(const LatticeDev& lat, const StoutArgs& a, const double2* __restrict__ U,
                                       const double2* __restrict__ link_ghost, double2* __restrict__ send) {
  constexpr int nd = NDIM;
  const int64_t n = lat.face_sites[NU];
  double2* dst = send + lat.ghost_off[NU][1] * (nd - 1) * 9;  // the high-face slot of the send buffer
  for (int64_t f = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; f < n; f += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    int y[4];
    const int64_t ys = site_of_face(lat, f, NU, lat.L[NU] - 1, y);
#pragma unroll
    for (int mu = 0; mu < nd; ++mu) {
      if (mu == NU || rho_of(a, mu, NU) == 0.0) continue;
      const int slot = mu < NU ? mu : mu - 1;
      store(dst + (f * (nd - 1) + slot) * 9, backward_staple(lat, U, link_ghost, ys, y, mu, NU));
    }
  }
}
// grid.y: the k-th divided direction
template <int NDIM>
__global__ void __launch_bounds__(256) k_stout_w_faces(LatticeDev lat, StoutArgs a, const double2* __restrict__ U,
                                                       const double2* __restrict__ link_ghost, double2* __restrict__ send) {
  int nu = -1, k = blockIdx.y;
#pragma unroll
  for (int d = 0; d < NDIM; ++d) {
    if (!lat.split[d]) continue;
    if (k == 0 && nu < 0) nu = d;
    --k;
  }
  if (nu == 0) w_face<NDIM, 0>(lat, a, U, link_ghost, send);
  if (NDIM > 1 && nu == 1) w_face<NDIM, 1 % NDIM>(lat, a, U, link_ghost, send);
  if (NDIM > 2 && nu == 2) w_face<NDIM, 2 % NDIM>(lat, a, U, link_ghost, send);
  if (NDIM > 3 && nu == 3) w_face<NDIM, 3 % NDIM>(lat, a, U, link_ghost, send);
}

// Re tr[ U_mu(x) U_nu(x+mu) (U_nu(x) U_mu(x+nu))^dagger ] summed over the block's sites, plane by plane: fixed blocks, the
// sites of a thread in ascending order, a butterfly over the wavefront and the waves of a block in ascending order
template <int NDIM>
__global__ void __launch_bounds__(256) k_plaquette(LatticeDev lat, int active_mask, const double2* __restrict__ U,
                                                   const double2* __restrict__ link_ghost, double2* __restrict__ partials) {
  constexpr int NP = NDIM * (NDIM - 1) / 2 > 0 ? NDIM * (NDIM - 1) / 2 : 1;
  __shared__ double wave_sum[4][NP];
  double acc[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) acc[p] = 0.0;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t s = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; s < lat.V; s += stride) {
    int x[4];
    coords32(lat, static_cast<unsigned>(s), x);
    int p = 0;
#pragma unroll
    for (int mu = 0; mu < NDIM; ++mu)
#pragma unroll
      for (int nu = mu + 1; nu < NDIM; ++nu, ++p) {
        if (!((active_mask >> mu) & 1) || !((active_mask >> nu) & 1)) continue;
        const M3 um = load(U + (s * NDIM + mu) * 9);
        const M3 t1 = mul(um, load(plus_link(lat, U, link_ghost, s, x, mu, nu)));
        const M3 un = load(U + (s * NDIM + nu) * 9);
        const M3 t2 = mul(un, load(plus_link(lat, U, link_ghost, s, x, nu, mu)));
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          t = fma(t1.e[k].x, t2.e[k].x, t);
          t = fma(t1.e[k].y, t2.e[k].y, t);
        }
        acc[p] += t;
      }
  }
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    double v = acc[p];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6][p] = v;
  }
  __syncthreads();
  if (threadIdx.x < kPlaqValues) {
    double v = 0.0;
    int p = 0;
#pragma unroll
    for (int mu = 0; mu < NDIM; ++mu)
#pragma unroll
      for (int nu = mu + 1; nu < NDIM; ++nu, ++p)
        if (static_cast<int>(threadIdx.x) == mu * 4 + nu) v = ((wave_sum[0][p] + wave_sum[1][p]) + wave_sum[2][p]) + wave_sum[3][p];
    partials[static_cast<int64_t>(blockIdx.x) * kPlaqValues + threadIdx.x] = make_double2(v, 0.0);
  }
}

unsigned site_grid(const LatticeDev& lat, int64_t max_blocks) {
  const int64_t want = (lat.V + 255) / 256;
  return static_cast<unsigned>(want < max_blocks ? want : max_blocks);
}

}  // namespace

void launch_stout_step(hipStream_t s, const LatticeDev& lat, const StoutArgs& a, const double2* U, const double2* link_ghost,
                       const double2* w_ghost, double2* out) {
  const dim3 grid(site_grid(lat, 65536));
  switch (lat.ndim) {  // (ndim = 1 has no staple: the host copies)
    case 2: hipLaunchKernelGGL(k_stout_step<2>, grid, dim3(256), 0, s, lat, a, U, link_ghost, w_ghost, out); break;
    case 3: hipLaunchKernelGGL(k_stout_step<3>, grid, dim3(256), 0, s, lat, a, U, link_ghost, w_ghost, out); break;
    case 4: hipLaunchKernelGGL(k_stout_step<4>, grid, dim3(256), 0, s, lat, a, U, link_ghost, w_ghost, out); break;
    default: break;
  }
}

void launch_stout_w_faces(hipStream_t s, const LatticeDev& lat, const StoutArgs& a, const double2* U, const double2* link_ghost,
                          double2* send) {
  int ns = 0;
  int64_t face = 0;
  for (int mu = 0; mu < lat.ndim; ++mu)
    if (lat.split[mu]) {
      ++ns;
      if (lat.face_sites[mu] > face) face = lat.face_sites[mu];
    }
  if (ns == 0 || lat.ndim < 2) return;
  const int64_t want = (face + 255) / 256;
  const dim3 grid(static_cast<unsigned>(want < 4096 ? want : 4096), ns);
  switch (lat.ndim) {
    case 2: hipLaunchKernelGGL(k_stout_w_faces<2>, grid, dim3(256), 0, s, lat, a, U, link_ghost, send); break;
    case 3: hipLaunchKernelGGL(k_stout_w_faces<3>, grid, dim3(256), 0, s, lat, a, U, link_ghost, send); break;
    case 4: hipLaunchKernelGGL(k_stout_w_faces<4>, grid, dim3(256), 0, s, lat, a, U, link_ghost, send); break;
    default: break;
  }
}

int launch_plaquette(hipStream_t s, const LatticeDev& lat, int active_mask, const double2* U, const double2* link_ghost,
                     double2* partials, int max_blocks) {
  const unsigned grid = site_grid(lat, max_blocks);
  switch (lat.ndim) {
    case 1: hipLaunchKernelGGL(k_plaquette<1>, dim3(grid), dim3(256), 0, s, lat, active_mask, U, link_ghost, partials); break;
    case 2: hipLaunchKernelGGL(k_plaquette<2>, dim3(grid), dim3(256), 0, s, lat, active_mask, U, link_ghost, partials); break;
    case 3: hipLaunchKernelGGL(k_plaquette<3>, dim3(grid), dim3(256), 0, s, lat, active_mask, U, link_ghost, partials); break;
    default: hipLaunchKernelGGL(k_plaquette<4>, dim3(grid), dim3(256), 0, s, lat, active_mask, U, link_ghost, partials); break;
  }
  return static_cast<int>(grid);
}

}  // namespace bcg
