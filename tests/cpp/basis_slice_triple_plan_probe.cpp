// Prints what basis_slice_triple_plan (blockcg_amd/csrc/slice_plan.hpp) decides for every request of a case file
// (tests/test_basis_slice_triple_cpu.py writes it), one line per request.  Host only: links slice_plan.cpp's object and nothing
// else, so it also runs under the host sanitizers.  A request is one line of integers:
//   L[4] origin[4] parity dir identical fast n_slices n_mom  na wa..  nb wb..  nc wc..
// and its answer
//   no plan | mfma=.. edge=.. pc=.. nbps=.. chunk=.. n_virtual=.. partials=.. tiles=a:b:c;...
#include <cstdio>
#include <vector>

#include "../../blockcg_amd/csrc/slice_plan.hpp"

using namespace bcg;

int main(int argc, char** argv) {
  FILE* f = argc > 1 ? std::fopen(argv[1], "r") : stdin;
  if (!f) return 2;
  LatticeDev lat{};
  int parity, dir, identical, fast, n_slices, n_mom;
  while (std::fscanf(f, "%d %d %d %d %d %d %d %d %d %d %d %d %d %d", &lat.L[0], &lat.L[1], &lat.L[2], &lat.L[3], &lat.origin[0],
                     &lat.origin[1], &lat.origin[2], &lat.origin[3], &parity, &dir, &identical, &fast, &n_slices, &n_mom) == 14) {
    lat.ndim = 4;
    lat.V = 1;
    for (int mu = 0; mu < 4; ++mu) {
      lat.stride[mu] = lat.V;
      lat.V *= lat.L[mu];
    }
    std::vector<int> w[3];
    for (int l = 0; l < 3; ++l) {
      int n;
      if (std::fscanf(f, "%d", &n) != 1 || n < 0 || n > 1024) return 3;
      w[l].resize(n);
      for (int k = 0; k < n; ++k)
        if (std::fscanf(f, "%d", &w[l][k]) != 1) return 3;
    }
    BasisSliceTriplePlan plan;
    if (!basis_slice_triple_plan(w[0].data(), static_cast<int>(w[0].size()), w[1].data(), static_cast<int>(w[1].size()), w[2].data(),
                                 static_cast<int>(w[2].size()), identical != 0, fast != 0, lat, parity, dir, n_slices, n_mom, &plan)) {
      std::puts("no plan");
      continue;
    }
    int64_t n_virtual, run, inner;
    slice_rows(lat, parity, dir, &n_virtual, &run, &inner);
    std::printf("mfma=%d edge=%d pc=%d nbps=%d chunk=%d n_virtual=%lld partials=%lld tiles=", plan.mfma ? 1 : 0, plan.edge, plan.pc,
                plan.walk.nbps, plan.walk.chunk, static_cast<long long>(n_virtual), static_cast<long long>(plan.partial_entries(n_slices)));
    for (int t = 0; t < plan.n_tiles(); ++t) std::printf("%d:%d:%d;", plan.tiles[3 * t], plan.tiles[3 * t + 1], plan.tiles[3 * t + 2]);
    std::puts("");
  }
  return 0;
}
