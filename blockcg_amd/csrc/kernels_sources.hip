// Sources and sinks on the device (gfx950): noise fields, point / wall sources and the slice-resolved inner product.
// All of them stream the device layout [site][colour][rhs] with 16 B per lane and lanes along the contiguous rhs index;
// none uses the matrix pipe.  Element indices and byte offsets are 64-bit.
#include <hip/hip_runtime.h>

#include "complex_ops.hpp"
#include "kernels_sources.hpp"

namespace bcg {

namespace {

// The counter generator and the site arithmetic of kernels_generic.hip, restated: they are file-local there, and that
// translation unit stays as it is.  Bit-identical to oracle::uniform_pm1 / oracle::field_counter.
__device__ __forceinline__ uint64_t splitmix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ double uniform_pm1(uint64_t seed_mixed, uint64_t counter) {
  const uint64_t h = splitmix64(seed_mixed ^ (counter * 0xD1342543DE82EF95ull + 0x632BE59BD9B4E019ull));
  return static_cast<double>(h >> 11) * (2.0 / 9007199254740992.0) - 1.0;
}
inline uint64_t splitmix64_host(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

struct GDims {
  int d[4];
};

// local coordinates of site `s` of a field of the given parity (-1: full field, s is the lexicographic site; 0 / 1: half
// field, s = k + (L0/2) (x1 + L1 (x2 + L2 x3)) with x0 = 2 k + ((x1 + x2 + x3 + parity + origin parity) & 1))
__device__ __forceinline__ void coords_of(const LatticeDev& lat, int parity, int64_t s, int x[4]) {
  const int l0 = parity < 0 ? lat.L[0] : lat.L[0] >> 1;
  const int k = static_cast<int>(s % l0); s /= l0;
  x[1] = static_cast<int>(s % lat.L[1]); s /= lat.L[1];
  x[2] = static_cast<int>(s % lat.L[2]); s /= lat.L[2];
  x[3] = static_cast<int>(s);
  if (parity < 0) {
    x[0] = k;
  } else {
    const int o = lat.origin[0] + lat.origin[1] + lat.origin[2] + lat.origin[3];
    x[0] = 2 * k + ((x[1] + x[2] + x[3] + parity + o) & 1);
  }
}
__device__ __forceinline__ int64_t global_index(const LatticeDev& lat, const GDims& g, const int x[4]) {
  int64_t gx = 0, st = 1;
#pragma unroll
  for (int nu = 0; nu < 4; ++nu) {
    gx += (x[nu] + lat.origin[nu]) * st;
    st *= g.d[nu];
  }
  return gx;
}

// ---------------------------------------------------------------------------------------------
// Noise: k_fill_field's loop with a transform of the two uniforms.  Write-only; the Gaussian costs one log, one sqrt and
// one sincospi per 16 bytes stored.
// ---------------------------------------------------------------------------------------------
template <int KIND>
__global__ void __launch_bounds__(256) k_fill_noise(int m, LatticeDev lat, GDims g, int parity, int64_t sites,
                                                    double2* __restrict__ f, uint64_t seed_mixed) {
  const int row = 3 * m;
  const int64_t n = sites * row;
  for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int64_t site = i / row;
    const int e = static_cast<int>(i - site * row);
    const int c = e / m, j = e - c * m;
    int x[4];
    coords_of(lat, parity, site, x);
    const uint64_t gx = static_cast<uint64_t>(global_index(lat, g, x));
    const uint64_t cnt = ((gx * m + j) * 3 + c) * 2;  // oracle::field_counter
    const double a = uniform_pm1(seed_mixed, cnt), b = uniform_pm1(seed_mixed, cnt + 1);
    double2 z;
    if (KIND == 0) {
      const double w = (1.0 - a) * 0.5;  // exact, in (0, 1]
      const double r = sqrt(-log(w));
      double sn, cs;
      sincospi(b, &sn, &cs);
      z = make_double2(r * cs, r * sn);
    } else if (KIND == 1) {
      z = make_double2(a < 0.0 ? -1.0 : 1.0, 0.0);
    } else {
      constexpr double h = 1.0 / 1.4142135623730951;  // fl(1 / fl(sqrt 2)): the division as written, what numpy gives too
      z = make_double2(a < 0.0 ? -h : h, b < 0.0 ? -h : h);
    }
    f[i] = z;
  }
}

__global__ void k_set_points(int n, PointOffsets p, double2* __restrict__ f) {
  const int j = threadIdx.x;
  if (j < n && p.offset[j] >= 0) f[p.offset[j]] = make_double2(1.0, 0.0);
}

__global__ void __launch_bounds__(256) k_set_walls(int m, LatticeDev lat, int parity, int64_t sites, double2* __restrict__ f,
                                                   int dir, WallColumns w, int site_parity) {
  const int row = 3 * m;
  const int64_t n = sites * row;
  for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int64_t site = i / row;
    const int e = static_cast<int>(i - site * row);
    const int c = e / m, j = e - c * m;
    int x[4];
    coords_of(lat, parity, site, x);
    int par = 0;
#pragma unroll
    for (int nu = 0; nu < 4; ++nu) par += x[nu] + lat.origin[nu];
    int xd = 0;  // global x_dir (selects, not an indexed register array)
#pragma unroll
    for (int nu = 0; nu < 4; ++nu) xd = nu == dir ? x[nu] + lat.origin[nu] : xd;
    const bool on = xd == w.slice[j] && c == w.colour[j] && (site_parity < 0 || (par & 1) == site_parity);
    f[i] = make_double2(on ? 1.0 : 0.0, 0.0);
  }
}

// ---------------------------------------------------------------------------------------------
// Slice dot.  For a direction `dir` the local lattice is [outer][x_dir][inner]: the elements of slice t are n_outer runs
// of `run` contiguous complex numbers (run = inner sites x 3 m; dir = ndim - 1 has one run, the whole slice), run o at
// element (o * L + t) * run.  Block (t, k) takes the k-th chunk of the run-by-run concatenation of slice t.  Chunks start
// at multiples of G = (256 / m) m and lane `tid` walks them with stride G, so a lane keeps its column j = tid % m and sums
// it in registers; the lanes of one column are added in a fixed tree in LDS at the end.  Every block writes m partial sums;
// k_slice_fold adds the blocks of a slice in ascending order: no atomics, the same bits on every run.
// Half field along direction 0: x0 = t is held by every second (x1, x2, x3) only, at half site o * L0/2 + t/2; the block
// walks all o and skips the others (no memory is touched for them).
// ---------------------------------------------------------------------------------------------
struct SliceGeom {
  int64_t n_virtual;  // n_outer * run: elements of one slice (half0: counting the skipped runs)
  int64_t run;        // elements per run, a multiple of m
  int64_t chunk;      // elements per block, a multiple of G
  int64_t step_o;     // G / run
  int64_t step_e;     // G % run
  int Leff;           // runs between those of consecutive o: L (half0: L0 / 2)
  int nbps;           // blocks per slice
  int half0;          // half field, dir = 0
  int L1, L2;         // half0: extents for the parity of o = x1 + L1 (x2 + L2 x3)
  int par_off;        // half0: field parity + parity of the local origin
};

struct SliceCursor {
  int64_t o, e, addr;
};
__device__ __forceinline__ void advance(SliceCursor& c, const SliceGeom& g) {
  c.o += g.step_o;
  c.e += g.step_e;
  c.addr += (g.step_o * g.Leff) * g.run + g.step_e;
  if (c.e >= g.run) {
    c.e -= g.run;
    c.o += 1;
    c.addr += static_cast<int64_t>(g.Leff - 1) * g.run;
  }
}
__device__ __forceinline__ bool held(const SliceCursor& c, const SliceGeom& g, int t) {
  if (!g.half0) return true;
  const int64_t q = c.o / g.L1;
  const int x1 = static_cast<int>(c.o - q * g.L1);
  const int x2 = static_cast<int>(q % g.L2), x3 = static_cast<int>(q / g.L2);
  return ((x1 + x2 + x3 + g.par_off + t) & 1) == 0;
}

template <bool SELF>
__global__ void __launch_bounds__(256) k_slice_dot(int m, SliceGeom g, const double2* __restrict__ a,
                                                   const double2* __restrict__ b, double2* __restrict__ partials) {
  __shared__ double2 red[256];
  const int tid = threadIdx.x;
  const int groups = 256 / m;
  const int G = groups * m;
  const int t = blockIdx.x / g.nbps, k = blockIdx.x - t * g.nbps;
  const int teff = g.half0 ? t >> 1 : t;
  const int64_t v0 = k * g.chunk;
  const int64_t v1 = v0 + g.chunk < g.n_virtual ? v0 + g.chunk : g.n_virtual;
  double2 acc[4] = {make_double2(0, 0), make_double2(0, 0), make_double2(0, 0), make_double2(0, 0)};
  if (tid < G) {  // widths that do not divide 256 leave the last lanes idle
    int64_t v = v0 + tid;
    SliceCursor c;
    c.o = v / g.run;
    c.e = v - c.o * g.run;
    c.addr = (c.o * g.Leff + teff) * g.run + c.e;
    for (; v + 3 * static_cast<int64_t>(G) < v1; v += 4 * static_cast<int64_t>(G)) {
      int64_t ad[4];
      bool on[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        ad[u] = c.addr;
        on[u] = held(c, g, t);
        advance(c, g);
      }
      double2 av[4], bv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        av[u] = on[u] ? a[ad[u]] : make_double2(0, 0);
        bv[u] = SELF ? av[u] : (on[u] ? b[ad[u]] : make_double2(0, 0));
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) cfma_conj(acc[u], av[u], bv[u]);
    }
    for (; v < v1; v += G) {
      if (held(c, g, t)) {
        const double2 av = a[c.addr];
        const double2 bv = SELF ? av : b[c.addr];
        cfma_conj(acc[0], av, bv);
      }
      advance(c, g);
    }
  }
  red[tid] = make_double2((acc[0].x + acc[1].x) + (acc[2].x + acc[3].x), (acc[0].y + acc[1].y) + (acc[2].y + acc[3].y));
  __syncthreads();
  // the `groups` lanes of a column: tree over the group index, the same pairs on every run
  int span = 1;
  while (span < groups) span <<= 1;
  const int grp = tid / m;
  for (int s = span >> 1; s >= 1; s >>= 1) {
    if (tid < G && grp < s && grp + s < groups) {
      const double2 o = red[tid + s * m];
      red[tid].x += o.x;
      red[tid].y += o.y;
    }
    __syncthreads();
  }
  if (tid < m) partials[static_cast<int64_t>(blockIdx.x) * m + tid] = red[tid];
}

__global__ void k_slice_fold(int m, int L_local, int nbps, int origin, const double2* __restrict__ partials,
                             double2* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= L_local * m) return;
  const int t = i / m, j = i - t * m;
  double2 s = make_double2(0, 0);
  for (int k = 0; k < nbps; ++k) {
    const double2 p = partials[(static_cast<int64_t>(t) * nbps + k) * m + j];
    s.x += p.x;
    s.y += p.y;
  }
  out[static_cast<int64_t>(origin + t) * m + j] = s;
}

int grid_for(int64_t n, int per_block, int cap) {
  int64_t g = (n + per_block - 1) / per_block;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return static_cast<int>(g);
}

}  // namespace

void launch_fill_noise(hipStream_t s, int m, const LatticeDev& lat, const int* gdims, int parity, double2* f, int kind,
                       uint64_t seed) {
  GDims g{{gdims[0], gdims[1], gdims[2], gdims[3]}};
  const int64_t sites = parity < 0 ? lat.V : lat.V / 2;
  const dim3 grid(grid_for(sites * 3 * m, 256, 16384));
  const uint64_t sm = splitmix64_host(seed);
  if (kind == 0) hipLaunchKernelGGL(k_fill_noise<0>, grid, dim3(256), 0, s, m, lat, g, parity, sites, f, sm);
  else if (kind == 1) hipLaunchKernelGGL(k_fill_noise<1>, grid, dim3(256), 0, s, m, lat, g, parity, sites, f, sm);
  else hipLaunchKernelGGL(k_fill_noise<2>, grid, dim3(256), 0, s, m, lat, g, parity, sites, f, sm);
}

void launch_set_points(hipStream_t s, int n, const PointOffsets& p, double2* f) {
  hipLaunchKernelGGL(k_set_points, dim3(1), dim3(64), 0, s, n, p, f);
}

void launch_set_walls(hipStream_t s, int m, const LatticeDev& lat, int parity, double2* f, int dir, const WallColumns& w,
                      int site_parity) {
  const int64_t sites = parity < 0 ? lat.V : lat.V / 2;
  hipLaunchKernelGGL(k_set_walls, dim3(grid_for(sites * 3 * m, 256, 16384)), dim3(256), 0, s, m, lat, parity, sites, f, dir, w,
                     site_parity);
}

int launch_slice_dot(hipStream_t s, int m, const LatticeDev& lat, int parity, int dir, const double2* a, const double2* b,
                     double2* partials, int64_t max_partials) {
  const int L = lat.L[dir];
  const int64_t G = (256 / m) * m;
  SliceGeom g{};
  g.half0 = parity >= 0 && dir == 0;
  int64_t n_outer;
  if (g.half0) {
    n_outer = lat.V / L;  // every (x1, x2, x3); half of them hold x0 = t
    g.run = 3 * m;
    g.Leff = L / 2;
    g.L1 = lat.L[1];
    g.L2 = lat.L[2];
    g.par_off = parity + ((lat.origin[0] + lat.origin[1] + lat.origin[2] + lat.origin[3]) & 1);
  } else {
    const int64_t inner = parity >= 0 ? lat.stride[dir] / 2 : lat.stride[dir];  // sites of one run (half: x0 is compact)
    n_outer = lat.V / (lat.stride[dir] * L);
    g.run = inner * 3 * m;
    g.Leff = L;
  }
  g.n_virtual = n_outer * g.run;
  g.step_o = G / g.run;
  g.step_e = G % g.run;
  // about 2048 blocks in all (8 per compute unit), none with less than four passes of its lanes, slices never shared
  int64_t nbps = (2048 + L - 1) / L;
  const int64_t most = (g.n_virtual + 4 * G - 1) / (4 * G);
  if (nbps > most) nbps = most;
  if (nbps < 1) nbps = 1;
  g.chunk = ((g.n_virtual + nbps - 1) / nbps + G - 1) / G * G;
  nbps = (g.n_virtual + g.chunk - 1) / g.chunk;
  g.nbps = static_cast<int>(nbps);
  const int64_t blocks = nbps * L;
  if (blocks * m > max_partials || blocks > 0x7fffffff) return 0;
  if (a == b) hipLaunchKernelGGL(k_slice_dot<true>, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, s, m, g, a, b, partials);
  else hipLaunchKernelGGL(k_slice_dot<false>, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, s, m, g, a, b, partials);
  return g.nbps;
}

void launch_slice_fold(hipStream_t s, int m, int L_local, int nbps, int origin, const double2* partials, double2* out) {
  hipLaunchKernelGGL(k_slice_fold, dim3((L_local * m + 255) / 256), dim3(256), 0, s, m, L_local, nbps, origin, partials, out);
}

}  // namespace bcg
