// The launch plans of the per-slice calls (slice_plan.hpp): integers in, integers out.  Host code only, as hop_plan.cpp.
#include "slice_plan.hpp"

#include <algorithm>

namespace bcg {

void slice_rows(const LatticeDev& lat, int parity, int dir, int64_t* n_virtual, int64_t* run, int64_t* inner) {
  const int L = lat.L[dir];
  if (parity >= 0 && dir == 0) {
    *inner = 1;
    *run = 3;
    *n_virtual = lat.V / L * 3;  // every (x1, x2, x3); half of them hold x0 = t
  } else {
    *inner = parity >= 0 ? lat.stride[dir] / 2 : lat.stride[dir];  // half: x0 is compact
    *run = *inner * 3;
    *n_virtual = lat.V / (lat.stride[dir] * L) * *run;
  }
}

void slice_walk_directions(const LatticeDev& lat, int dir, SliceWalk* plan) {
  int n = 0;
  plan->ltab = 1;
  for (int mu = 0; mu < 4; ++mu)
    if (mu != dir) {
      plan->mu[n++] = mu;
      if (lat.L[mu] > plan->ltab) plan->ltab = lat.L[mu];
    }
}

void slice_walk_blocks(int64_t n_virtual, int64_t blocks_per_slice, SliceWalk* plan) {
  int64_t nbps = std::min(blocks_per_slice, slice_most_blocks(n_virtual));
  if (nbps < 1) nbps = 1;
  const int64_t chunk = ((n_virtual + nbps - 1) / nbps + 15) / 16 * 16;
  plan->nbps = static_cast<int>((n_virtual + chunk - 1) / chunk);
  plan->chunk = static_cast<int>(chunk);
}

int slice_launch_pc(int n) { return n <= 1 ? 1 : n <= 2 ? 2 : 4; }

namespace {

// what every planner begins with: the walk's directions and the rows of a slice; false: 2^30 rows or more
bool slice_walk_begin(const LatticeDev& lat, int parity, int dir, SliceWalk* walk, int64_t* n_virtual) {
  slice_walk_directions(lat, dir, walk);
  int64_t run, inner;
  slice_rows(lat, parity, dir, n_virtual, &run, &inner);
  return *n_virtual < (int64_t(1) << 30);
}

int mfma_pc(int m, int P) { return m == 16 && P >= 4 ? 4 : P >= 2 ? 2 : 1; }

// the groups of a call: MFMA runs cut into kb blocks, generic runs into groups of at most `cols` columns
std::vector<BasisSliceGroup> slice_groups(const int* widths, int nv, bool fast, int kb, int cols) {
  std::vector<BasisSliceGroup> out;
  int off = 0, block = 0;
  for (int k = 0; k < nv;) {
    const bool mf = fast && basis_mfma_width(widths[k]);
    if (mf) {
      int nb = 0;
      for (; k < nv && basis_mfma_width(widths[k]); ++k) nb += widths[k] / 16;
      for (int q = 0; q < nb; q += kb) {
        const int n = nb - q < kb ? nb - q : kb;
        out.push_back(BasisSliceGroup{true, block + q, n, 16 * n, off + 16 * q});
      }
      block += nb;
      off += 16 * nb;
    } else {
      BasisSliceGroup g{false, k, 0, 0, off};
      while (k < nv && !(fast && basis_mfma_width(widths[k])) && g.count < kBasisGenericFields &&
             (g.count == 0 || g.K + widths[k] <= cols)) {
        g.K += widths[k];
        g.count += 1;
        k += 1;
      }
      off += g.K;
      out.push_back(g);
    }
  }
  return out;
}

}  // namespace

bool slice_gram_plan(int m, bool mfma, const LatticeDev& lat, int parity, int dir, int L_global, int n_mom, int64_t half_entries,
                     SliceGramPlan* plan) {
  const int64_t mm = static_cast<int64_t>(m) * m;
  const int L = lat.L[dir];
  const int pc_max = mfma && m == 16 ? 4 : 2;
  int pc = 1;
  while (2 * pc <= pc_max && 2 * pc <= n_mom && 2 * pc * L_global * mm <= half_entries) pc *= 2;
  if (pc * L_global * mm > half_entries) return false;
  plan->pc = pc;
  int64_t n_virtual;
  if (!slice_walk_begin(lat, parity, dir, &plan->walk, &n_virtual)) return false;
  const int64_t room = half_entries - slice_gram_table_entries(*plan);
  if (room <= 0) return false;
  const int64_t budget = std::min<int64_t>(room / (pc * mm), 2048);
  slice_walk_blocks(n_virtual, budget / L, &plan->walk);
  return static_cast<int64_t>(plan->walk.nbps) * L <= budget;
}

int BasisSlicePlan::pc_max() const {
  int pc = 1;
  for (const BasisSliceGroup& g : groups) pc = pc_of(g) > pc ? pc_of(g) : pc;
  return pc;
}

bool basis_slice_plan(const int* widths, int nv, int m, bool fast, const LatticeDev& lat, int parity, int dir, int n_mom,
                      int64_t half_entries, BasisSlicePlan* plan) {
  fast = fast && (m == 16 || m == 32);
  const int L = lat.L[dir];
  int64_t n_virtual;
  if (!slice_walk_begin(lat, parity, dir, &plan->walk, &n_virtual)) return false;
  const int64_t want = std::max<int64_t>(L, std::min<int64_t>(256, L * slice_most_blocks(n_virtual)));
  const int P = n_mom > 0 ? n_mom : 1;
  plan->pc_mfma = fast ? mfma_pc(m, P) : 1;
  plan->kb = fast ? 4 / (plan->pc_mfma * (m / 16)) : 1;
  plan->pc_generic = P >= 2 ? 2 : 1;
  plan->cols = kBasisGenericCols;
  int64_t budget;
  for (;;) {
    plan->groups = slice_groups(widths, nv, fast, plan->kb, plan->cols);
    int64_t E = 0;
    const BasisSliceGroup* top = nullptr;
    for (const BasisSliceGroup& g : plan->groups) {
      const int64_t e = static_cast<int64_t>(plan->pc_of(g)) * g.K * m;
      if (e > E) {
        E = e;
        top = &g;
      }
    }
    const int64_t room = half_entries - (n_mom > 0 ? basis_slice_table_entries(*plan) : 0);
    budget = room > 0 ? room / E : 0;
    if (budget >= want) break;
    if (top->mfma) {
      if (plan->kb > 1) plan->kb -= 1;
      else if (plan->pc_mfma > 1) plan->pc_mfma /= 2;
      else break;
    } else {
      if (top->count > 1) plan->cols = top->K / 2;
      else if (plan->pc_generic > 1) plan->pc_generic = 1;
      else break;
    }
  }
  if (budget < L) return false;
  slice_walk_blocks(n_virtual, std::min<int64_t>(budget, 2048) / L, &plan->walk);
  return true;
}

bool basis_slice_axpy_plan(const LatticeDev& lat, int parity, int dir, int n_slices, SliceWalk* plan) {
  int64_t n_virtual;
  if (!slice_walk_begin(lat, parity, dir, plan, &n_virtual)) return false;
  slice_walk_blocks(n_virtual, kBasisSliceAxpyBlocks / (n_slices > 0 ? n_slices : 1), plan);
  return true;
}

bool basis_slice_triple_plan(const int* wa, int na, const int* wb, int nb, const int* wc, int nc, bool identical, bool fast,
                             const LatticeDev& lat, int parity, int dir, int n_slices, int n_mom, BasisSliceTriplePlan* plan) {
  (void)n_mom;  // one momentum per launch whatever their number
  const int* w[3] = {wa, wb, wc};
  const int n[3] = {na, nb, nc};
  int K[3] = {0, 0, 0};
  bool mfma = fast;
  for (int l = 0; l < 3; ++l)
    for (int k = 0; k < n[l]; ++k) {
      K[l] += w[l][k];
      mfma = mfma && basis_mfma_width(w[l][k]);
      if (K[l] > kTripleMaxColumns) return false;
    }
  plan->mfma = mfma;
  plan->identical = identical;
  plan->edge = mfma ? kTripleEdgeMfma : kTripleEdgeGeneric;
  plan->pc = 1;
  int nt[3];
  for (int l = 0; l < 3; ++l) nt[l] = (K[l] + plan->edge - 1) / plan->edge;
  plan->tiles.clear();
  for (int ta = 0; ta < nt[0]; ++ta)
    for (int tb = identical ? ta : 0; tb < nt[1]; ++tb)
      for (int tc = identical ? tb : 0; tc < nt[2]; ++tc) {
        plan->tiles.push_back(ta);
        plan->tiles.push_back(tb);
        plan->tiles.push_back(tc);
      }
  int64_t n_virtual;
  if (!slice_walk_begin(lat, parity, dir, &plan->walk, &n_virtual)) return false;
  const int64_t per_slice = static_cast<int64_t>(n_slices > 0 ? n_slices : 1) * plan->n_tiles();  // blocks at nbps = 1
  const int64_t room = kTriplePartialEntries / plan->tile_entries();
  if (per_slice > room) return false;
  const int64_t most = (n_virtual + kTripleChunkRows - 1) / kTripleChunkRows;
  int64_t nbps = std::min<int64_t>(std::min<int64_t>(std::max<int64_t>(kTripleBlocks / per_slice, 1), room / per_slice), most);
  if (nbps < 1) nbps = 1;
  const int64_t chunk = ((n_virtual + nbps - 1) / nbps + kTripleChunkRows - 1) / kTripleChunkRows * kTripleChunkRows;
  plan->walk.chunk = static_cast<int>(chunk);
  plan->walk.nbps = static_cast<int>((n_virtual + chunk - 1) / chunk);
  return true;
}

}  // namespace bcg
