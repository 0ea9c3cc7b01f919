// Launchers of the per-slice Gram kernels (kernels_slice_gram.hip; include/blockcg_hip.h: bcg_field_slice_gram).
//
//   C_p(t)(i, j) = sum_{x : x_dir = t} w_p(x) sum_c conj(a[x, c, i]) b[x, c, j]        over the LOCAL sites,
//   w_p(x) = prod_{mu != dir} tab[p][slot of mu][x_mu]                                 (ascending mu)
//
// The walk.  For a direction `dir` the local lattice is [outer][x_dir][inner]: the rows (row = site * 3 + colour, m complex
// each) of slice t are n_outer runs of `run` contiguous rows (run = inner sites x 3), run o at row (o * L + t) * run.
// Block (t, k) takes the k-th chunk of the run-by-run concatenation of slice t's rows -- k_slice_dot's virtual walk in
// units of rows.  Half field along direction 0: a run is one site, every (x1, x2, x3) is walked and the sites of the other
// parity are skipped (zero operands, no memory touched).
//
// The launch plan (slice_gram_plan) is a function of (shape, m, parity, dir, n_mom) only:
//   pc     momenta per launch: the largest instantiated count (MFMA m = 16: 1, 2, 4; m = 32 and the generic kernel: 1, 2)
//          that is <= max(n_mom, 1) and whose reduced result pc * L_global * m^2 fits its half of the scratch
//   blocks budget = min(2048, entries left in the partials' half / (pc * m^2)); blocks per slice = budget / L_local, at most
//          rows_of_a_slice / 64 (no block with less than four quads of 4 rows per wave: 64 rows), at least 1
//   chunk  rows per block = rows_of_a_slice / blocks per slice, rounded up to a multiple of 16 (one quad per wave); the
//          blocks per slice are then recounted from the chunk.  A block never holds rows of two slices.
// A call's last launch may carry fewer momenta (the smallest instantiated count that holds them; the tables of the unused
// ones are ones and their results are dropped); nbps and chunk stay those of the plan.  No atomics anywhere: every block
// stores pc matrices of partial sums with plain stores and k_slice_gram_fold adds the blocks of a (p, t) in ascending k.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.hpp"

namespace bcg {

struct SliceGramPlan {
  int pc;         // momenta per launch
  int nbps;       // blocks per slice
  int chunk;      // rows per block, a multiple of 16
  int ltab;       // entries per phase table: the largest local extent among the directions != dir
  int mu[3];      // the directions != dir in ascending order (table slots 0..2)
};

// m = 16 and m = 32 take the MFMA kernel when mfma is set; every other width, and mfma = false, the generic VALU kernel.
// table_entries(plan) double2 are taken off `half_entries` (the partials' half of the scratch) for the phase tables.
// Returns false when the plan does not fit: pc * L_global * m^2 > half_entries for pc = 1, the block partials of one
// block per slice do not fit, or a slice has 2^30 rows or more.
bool slice_gram_plan(int m, bool mfma, const LatticeDev& lat, int parity, int dir, int L_global, int n_mom, int64_t half_entries,
                     SliceGramPlan* plan);
inline int64_t slice_gram_table_entries(const SliceGramPlan& p) { return static_cast<int64_t>(p.pc) * 3 * p.ltab; }
// the smallest instantiated momentum count >= n (n <= plan.pc)
int slice_gram_launch_pc(int n);

// partials[((t * nbps + k) * pc + p) * m^2 + j * m + i], t < L_dir local, k < plan.nbps, p < pc
// tab: [pc][3][plan.ltab] phases of the LOCAL coordinates (device memory), or nullptr: no phase arithmetic (pc = 1)
void launch_slice_gram(hipStream_t s, int m, bool mfma, const LatticeDev& lat, int parity, int dir, const SliceGramPlan& plan, int pc,
                       const double2* a, const double2* b, const double2* tab, double2* partials);
// out[(p * L_global + origin + t) * m^2 + e] = sum_k partials[...] in ascending k, for the first np of the launch's pc momenta
void launch_slice_gram_fold(hipStream_t s, int m, int pc, int np, int L_local, int L_global, int nbps, int origin,
                            const double2* partials, double2* out);

}  // namespace bcg
