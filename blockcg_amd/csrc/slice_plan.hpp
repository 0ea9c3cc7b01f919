// The launch plans of the calls that walk a field slice by slice (slice_plan.cpp, host only: no HIP call, no device memory
// touched; tests/cpp/slice_plan_probe.cpp links its object alone): bcg_field_slice_gram (kernels_slice_gram.hpp),
// bcg_basis_slice_dot (kernels_basis_slice.hpp) and bcg_basis_slice_axpy (kernels_basis_slice_axpy.hpp).  A caller plans,
// then launches; the launchers turn the plan's SliceWalk into the kernels' SGGeom (slice_walk.hpp).
//
// The walk.  For a direction `dir` the local lattice is [outer][x_dir][inner]: the rows (row = site * 3 + colour, m complex
// each) of slice t are n_outer runs of `run` contiguous rows (run = inner sites x 3), run o at row (o * L + t) * run.
// Block (t, k) takes the k-th chunk of the run-by-run concatenation of slice t's rows -- k_slice_dot's virtual walk in
// units of rows.  Half field along direction 0: a run is one site, every (x1, x2, x3) is walked and the sites of the other
// parity are skipped (zero operands, no memory touched).
//
// What every plan shares (SliceWalk), given the blocks per slice its call would like:
//   blocks per slice  at most rows_of_a_slice / 64 (no block with less than four quads of 4 rows per wave: 64 rows), at
//                     least 1
//   chunk             rows per block = rows_of_a_slice / blocks per slice, rounded up to a multiple of 16 (one quad per
//                     wave); the blocks per slice are then recounted from the chunk.  A block never holds rows of two slices.
// The plans differ in where the blocks per slice wanted come from (a budget of scratch entries, or a grid aimed at) and in
// when they give up; that is told in the three kernel headers.  No plan of any call: a slice of 2^30 rows or more.
#pragma once
#include <cstdint>
#include <vector>

#include "kernels.hpp"
#include "kernels_basis.hpp"

namespace bcg {

struct SliceWalk {
  int nbps;   // blocks per slice
  int chunk;  // rows per block, a multiple of 16
  int ltab;   // entries per phase table: the largest local extent among the directions != dir
  int mu[3];  // the directions != dir in ascending order (table slots 0..2)
};

// rows of one slice (half field along direction 0: counting the skipped sites), rows and sites per run
void slice_rows(const LatticeDev& lat, int parity, int dir, int64_t* n_virtual, int64_t* run, int64_t* inner);
// mu and ltab
void slice_walk_directions(const LatticeDev& lat, int dir, SliceWalk* plan);
inline int64_t slice_most_blocks(int64_t n_virtual) { return (n_virtual + 63) / 64; }
// nbps and chunk from the rows of a slice and the blocks per slice wanted
void slice_walk_blocks(int64_t n_virtual, int64_t blocks_per_slice, SliceWalk* plan);
// the smallest instantiated momentum count >= n (n <= the pc of the plan, or of the form)
int slice_launch_pc(int n);

// ---- bcg_field_slice_gram (kernels_slice_gram.hpp) -------------------------------------------------
struct SliceGramPlan {
  int pc;  // momenta per launch
  SliceWalk walk;
};

// m = 16 and m = 32 take the MFMA kernel when mfma is set; every other width, and mfma = false, the generic VALU kernel.
// table_entries(plan) double2 are taken off `half_entries` (the partials' half of the scratch) for the phase tables.
// Returns false when the plan does not fit: pc * L_global * m^2 > half_entries for pc = 1, the block partials of one
// block per slice do not fit, or a slice has 2^30 rows or more.
bool slice_gram_plan(int m, bool mfma, const LatticeDev& lat, int parity, int dir, int L_global, int n_mom, int64_t half_entries,
                     SliceGramPlan* plan);
inline int64_t slice_gram_table_entries(const SliceGramPlan& p) { return static_cast<int64_t>(p.pc) * 3 * p.walk.ltab; }

// ---- bcg_basis_slice_dot (kernels_basis_slice.hpp) -------------------------------------------------
struct BasisSliceGroup {
  bool mfma;
  int first;   // MFMA: first 16-column block, counted over the blocks of all MFMA fields of V in order; generic: first field
  int count;   // MFMA: blocks; generic: fields
  int K, off;  // its columns off .. off + K - 1 of the basis
};

struct BasisSlicePlan {
  int pc_mfma, kb;       // momenta per launch and blocks per group of the MFMA form
  int pc_generic, cols;  // momenta per launch and the column bound of the generic form
  SliceWalk walk;
  std::vector<BasisSliceGroup> groups;
  int pc_of(const BasisSliceGroup& g) const { return g.mfma ? pc_mfma : pc_generic; }
  int pc_max() const;  // over the groups
};

// widths[0 .. nv-1]: the widths of V; fast: the MFMA form is allowed (bcg_force_generic not set).  half_entries: the double2
// the phase tables (table_entries) and the block partials may take.  Returns false when no plan fits: one block per slice
// of (one block of 16 columns or one generic field, pc = 1) does not fit, or a slice has 2^30 rows or more.
bool basis_slice_plan(const int* widths, int nv, int m, bool fast, const LatticeDev& lat, int parity, int dir, int n_mom,
                      int64_t half_entries, BasisSlicePlan* plan);
inline int64_t basis_slice_table_entries(const BasisSlicePlan& p) { return static_cast<int64_t>(p.pc_max()) * 3 * p.walk.ltab; }

// ---- bcg_basis_slice_axpy (kernels_basis_slice_axpy.hpp) and bcg_basis_slice_rotate (kernels_basis_slice_rotate.hpp):
// ---- their plan is the walk and nothing else ----------------------------------------------------------
constexpr int kBasisSliceAxpyBlocks = 2048;  // the grid aimed at, as in the per-slice products

// n_slices: the local slices the launch walks (>= 1).  Returns false when a slice has 2^30 rows or more.
bool basis_slice_axpy_plan(const LatticeDev& lat, int parity, int dir, int n_slices, SliceWalk* plan);

// ---- bcg_basis_slice_triple (kernels_basis_slice_triple.hpp) ----------------------------------------
// A block owns one output tile of edge^3 entries (edge columns of each list) on one chunk of one listed slice.  The walk
// differs from the other plans' in its unit: a step is four whole sites (12 rows: three k-steps of the matrix instruction,
// or one colour triple per site), and the chunk is a whole number of 16-site rounds (48 rows, which is also a multiple of
// the 16 rows every SliceWalk keeps).
constexpr int kTripleMaxColumns = 64;             // total width of a list
constexpr int kTripleEdgeMfma = 16;               // tile edge of the MFMA form
constexpr int kTripleEdgeGeneric = 8;             // and of the generic form
constexpr int kTripleChunkRows = 48;              // the chunk is a multiple of it
constexpr int kTripleBlocks = 1024;               // the grid aimed at: two blocks per CU, twice over
constexpr int64_t kTriplePartialEntries = int64_t(1) << 24;  // block partials of one launch at the most (256 MiB)

struct BasisSliceTriplePlan {
  bool mfma;               // every width of the three lists in {16, 32} and the MFMA form allowed
  bool identical;          // the three lists are one list: only tiles ta <= tb <= tc
  int edge;                // tile edge
  int pc;                  // momenta per launch: 1 (the accumulators of one momentum fill the MFMA form's budget)
  SliceWalk walk;          // nbps: blocks per (slice, tile)
  std::vector<int> tiles;  // (ta, tb, tc) per tile, in ascending (ta, tb, tc): columns edge * t .. of each list
  int n_tiles() const { return static_cast<int>(tiles.size() / 3); }
  int64_t tile_entries() const { return static_cast<int64_t>(edge) * edge * edge; }
  // block partials of one launch over n_slices local slices
  int64_t partial_entries(int n_slices) const { return static_cast<int64_t>(n_slices) * n_tiles() * walk.nbps * tile_entries(); }
};

// widths of the three lists; identical: they are the same list; fast: bcg_force_generic not set; n_slices: the listed
// slices that are local (>= 0; 0 plans as for one).  A pure function of its arguments.  Returns false when a list is
// wider than kTripleMaxColumns, a slice has 2^30 rows or more, or one block per (slice, tile) already needs more than
// kTriplePartialEntries of partials (the caller lists fewer slices).
bool basis_slice_triple_plan(const int* wa, int na, const int* wb, int nb, const int* wc, int nc, bool identical, bool fast,
                             const LatticeDev& lat, int parity, int dir, int n_slices, int n_mom, BasisSliceTriplePlan* plan);

}  // namespace bcg
