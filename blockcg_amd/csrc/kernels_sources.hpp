// Launchers of the source and sink kernels (kernels_sources.hip; include/blockcg_hip.h: bcg_field_fill_noise,
// bcg_field_set_point_sources, bcg_field_set_wall_sources, bcg_field_slice_dot).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.hpp"

namespace bcg {

constexpr int kMaxWidth = 32;

// Noise from the counter generator of launch_fill_field: with (a, b) the two uniforms in [-1, 1) that generator gives a
// complex element (same seed, same GLOBAL element index),
//   kind 0 (Gaussian): sqrt(-ln((1 - a) / 2)) * (cos(pi b), sin(pi b))      density exp(-|z|^2)
//   kind 1 (Z2)      : (a < 0 ? -1 : +1, 0)
//   kind 2 (Z4)      : ((a < 0 ? -1 : +1), (b < 0 ? -1 : +1)) / sqrt(2)
// parity = -1: full field; 0 / 1: half field (the values the full field has on those sites).
void launch_fill_noise(hipStream_t s, int m, const LatticeDev& lat, const int* gdims, int parity, double2* f, int kind,
                       uint64_t seed);

// f[offset[j]] = 1 for j < n (offset < 0: the site lives on another rank); f has been zeroed by the caller
struct PointOffsets {
  int64_t offset[kMaxWidth];
};
void launch_set_points(hipStream_t s, int n, const PointOffsets& p, double2* f);

// One pass that writes the whole field: column j is 1 in colour[j] on the sites with GLOBAL x_dir = slice[j] whose global
// parity matches site_parity (-1: all), 0 elsewhere.
struct WallColumns {
  int slice[kMaxWidth];
  int colour[kMaxWidth];
};
void launch_set_walls(hipStream_t s, int m, const LatticeDev& lat, int parity, double2* f, int dir, const WallColumns& w,
                      int site_parity);

// Slice sums  out[t][j] = sum_{x: x_dir = t} sum_c conj(a[x,c,j]) b[x,c,j]  over the LOCAL sites, in two steps:
//   launch_slice_dot   partials[(t * nbps + k) * m + j], t < L_dir local, k < nbps blocks per slice (the return value; a
//                      function of the shape only).  Returns 0 if the partials would not fit max_partials entries.
//   launch_slice_fold  out[(origin_dir + t) * m + j] = sum_k partials[...] in ascending k
// a == b reads the field once.  parity as above (both operands of one parity).
int launch_slice_dot(hipStream_t s, int m, const LatticeDev& lat, int parity, int dir, const double2* a, const double2* b,
                     double2* partials, int64_t max_partials);
void launch_slice_fold(hipStream_t s, int m, int L_local, int nbps, int origin, const double2* partials, double2* out);

}  // namespace bcg
