// The slice walk shared by the per-slice Gram kernels (kernels_slice_gram.hip), the per-slice basis products
// (kernels_basis_slice.hip), their adjoint (kernels_basis_slice_axpy.hip) and the rotation by slice
// (kernels_basis_slice_rotate.hip): which rows of a field belong to slice t of a
// direction, in which order a block takes them, the coordinates of a row's site and its momentum phase.  The walk itself and
// the plans that size it are described in slice_plan.hpp.  Everything lives in an anonymous namespace: each translation
// unit has its own copy, as with mfma_common.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "complex_ops.hpp"
#include "kernels.hpp"
#include "slice_plan.hpp"

namespace bcg {

namespace {

struct SGGeom {
  int n_virtual;  // rows of one slice (half0: counting the skipped sites)
  int run;        // rows per run
  int inner;      // sites per run
  int chunk;      // rows per block
  int Leff;       // runs between those of consecutive o: L (half0: L0 / 2)
  int nbps;       // blocks per slice
  int half0;      // half field, dir = 0
  int half;       // half field, dir > 0: slot 0 is the compact x0
  int e0, e1;     // extents of slots 0 and 1 in the slice's site index c0 + e0 (c1 + e1 c2)
  int par_off;    // half fields: field parity + parity of the local origin
  int ltab;       // entries per phase table
};

struct SGRow {
  int64_t row;  // row of the field
  bool ok;      // it exists and the field holds it
  int x[3];     // local coordinates of its site along the three slots (0 where !ok)
};

// What a block walks: the virtual rows r0 .. r1 - 1 of slice t (teff: the slice in the row address)
struct SGBlock {
  int t, teff, r0, r1;
};
// the block's slice is the s-th of the grid (s = blockIdx.x / g.nbps) and slice t of the field
__device__ __forceinline__ SGBlock sg_block(const SGGeom& g, int s, int t) {
  SGBlock b;
  const int k = blockIdx.x - s * g.nbps;
  b.t = t;
  b.teff = g.half0 ? t >> 1 : t;
  b.r0 = k * g.chunk;
  b.r1 = b.r0 + g.chunk < g.n_virtual ? b.r0 + g.chunk : g.n_virtual;
  return b;
}

// virtual row v = o * run + e of slice t; live: v is inside the block's chunk
template <bool COORDS>
__device__ __forceinline__ SGRow sg_row(const SGGeom& g, int t, int teff, int o, int e, bool live) {
  SGRow r;
  r.ok = live;
  r.row = (static_cast<int64_t>(o) * g.Leff + teff) * g.run + e;
  r.x[0] = r.x[1] = r.x[2] = 0;
  if (COORDS || g.half0) {
    const int idx = live ? o * g.inner + e / 3 : 0;
    const int q = idx / g.e0;
    const int c0 = idx - q * g.e0;
    const int c2 = q / g.e1;
    const int c1 = q - c2 * g.e1;
    if (g.half0) r.ok = live && ((c0 + c1 + c2 + g.par_off + t) & 1) == 0;
    r.x[0] = g.half ? 2 * c0 + ((c1 + c2 + t + g.par_off) & 1) : c0;
    r.x[1] = c1;
    r.x[2] = c2;
  }
  return r;
}

// the staging loops' virtual row v of the block's slice: not live past the chunk's end, where (o, e) are those of row r0
template <bool COORDS>
__device__ __forceinline__ SGRow sg_row_at(const SGGeom& g, const SGBlock& b, int v) {
  const bool live = v < b.r1;
  const int vv = live ? v : b.r0;
  const int o = vv / g.run, e = vv - o * g.run;
  return sg_row<COORDS>(g, b.t, b.teff, o, e, live);
}

// w_p of a site: the three table entries multiplied in ascending direction
__device__ __forceinline__ double2 sg_phase(const double2* __restrict__ tab, int ltab, int p, const int x[3]) {
  const double2* tp = tab + static_cast<int64_t>(p) * 3 * ltab;
  return cmul(cmul(tp[x[0]], tp[ltab + x[1]]), tp[2 * ltab + x[2]]);
}

// the kernels' view of a launch
inline SGGeom slice_geom(const LatticeDev& lat, int parity, int dir, const SliceWalk& walk) {
  int64_t n_virtual, run, inner;
  slice_rows(lat, parity, dir, &n_virtual, &run, &inner);
  SGGeom g{};
  g.n_virtual = static_cast<int>(n_virtual);
  g.run = static_cast<int>(run);
  g.inner = static_cast<int>(inner);
  g.chunk = walk.chunk;
  g.nbps = walk.nbps;
  g.half0 = parity >= 0 && dir == 0;
  g.half = parity >= 0 && dir != 0;
  g.Leff = g.half0 ? lat.L[0] / 2 : lat.L[dir];
  g.e0 = g.half ? lat.L[0] / 2 : lat.L[walk.mu[0]];
  g.e1 = lat.L[walk.mu[1]];
  g.par_off = parity >= 0 ? parity + ((lat.origin[0] + lat.origin[1] + lat.origin[2] + lat.origin[3]) & 1) : 0;
  g.ltab = walk.ltab;
  return g;
}

}  // namespace
}  // namespace bcg
