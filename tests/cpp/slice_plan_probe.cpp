// Prints what the planners of the per-slice calls decide for every request of a case file (tests/slice_plan_cases.py writes
// it: one request per line, integers), one line per request.  Host only: links blockcg_amd/csrc/slice_plan.cpp's object and
// nothing else.  A request begins with the planner (0 slice_gram_plan, 1 basis_slice_plan, 2 basis_slice_axpy_plan) and the
// lattice: L[4] origin[4] parity dir.
//   no plan | [pc=.. | pc_mfma=.. kb=.. pc_generic=.. cols=..] nbps=.. chunk=.. ltab=.. mu=a,b,c [groups=mfma:first:count:K:off;..]
#include <cstdio>
#include <vector>

#include "../../blockcg_amd/csrc/slice_plan.hpp"

using namespace bcg;

static void print_walk(const SliceWalk& w) {
  std::printf("nbps=%d chunk=%d ltab=%d mu=%d,%d,%d", w.nbps, w.chunk, w.ltab, w.mu[0], w.mu[1], w.mu[2]);
}

int main(int argc, char** argv) {
  FILE* f = argc > 1 ? std::fopen(argv[1], "r") : stdin;
  if (!f) return 2;
  int kind, parity, dir;
  LatticeDev lat{};
  while (std::fscanf(f, "%d %d %d %d %d %d %d %d %d %d %d", &kind, &lat.L[0], &lat.L[1], &lat.L[2], &lat.L[3], &lat.origin[0],
                     &lat.origin[1], &lat.origin[2], &lat.origin[3], &parity, &dir) == 11) {
    lat.ndim = 4;
    lat.V = 1;
    for (int mu = 0; mu < 4; ++mu) {
      lat.stride[mu] = lat.V;
      lat.V *= lat.L[mu];
    }
    if (kind == 0) {
      int m, mfma, L_global, n_mom;
      long long half_entries;
      if (std::fscanf(f, "%d %d %d %d %lld", &m, &mfma, &L_global, &n_mom, &half_entries) != 5) return 3;
      SliceGramPlan plan;
      if (!slice_gram_plan(m, mfma != 0, lat, parity, dir, L_global, n_mom, half_entries, &plan)) {
        std::puts("no plan");
        continue;
      }
      std::printf("pc=%d ", plan.pc);
      print_walk(plan.walk);
    } else if (kind == 1) {
      int m, fast, n_mom, nv;
      long long half_entries;
      if (std::fscanf(f, "%d %d %d %lld %d", &m, &fast, &n_mom, &half_entries, &nv) != 5) return 3;
      std::vector<int> widths(nv);
      for (int k = 0; k < nv; ++k)
        if (std::fscanf(f, "%d", &widths[k]) != 1) return 3;
      BasisSlicePlan plan;
      if (!basis_slice_plan(widths.data(), nv, m, fast != 0, lat, parity, dir, n_mom, half_entries, &plan)) {
        std::puts("no plan");
        continue;
      }
      std::printf("pc_mfma=%d kb=%d pc_generic=%d cols=%d ", plan.pc_mfma, plan.kb, plan.pc_generic, plan.cols);
      print_walk(plan.walk);
      std::printf(" groups=");
      for (const BasisSliceGroup& g : plan.groups) std::printf("%d:%d:%d:%d:%d;", g.mfma ? 1 : 0, g.first, g.count, g.K, g.off);
    } else {
      int n_slices;
      if (std::fscanf(f, "%d", &n_slices) != 1) return 3;
      SliceWalk plan;
      if (!basis_slice_axpy_plan(lat, parity, dir, n_slices, &plan)) {
        std::puts("no plan");
        continue;
      }
      print_walk(plan);
    }
    std::puts("");
  }
  return 0;
}
