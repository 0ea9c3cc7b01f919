// Host-only probe of the stencil planner for the two requests of the pair with phase B inside (HOP_FACT1G, HOP_FACT2B):
// reads "m L0 L1 L2 L3 patch0 patch1 patch2 blocks bundle_walk cls x3_n ring cb mode gram" per line and prints
// "<form> <lds> <grid>" (form 0 = declined).  tests/test_fused_plan_cpu.py links it with hop_plan.o alone.
#include <cstdio>

#include "../../blockcg_amd/csrc/hop_plan.hpp"

int main() {
  int m, L[4], p[3], blocks, bundle, cls, x3n, ring, cb, mode, gram;
  while (std::scanf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d", &m, &L[0], &L[1], &L[2], &L[3], &p[0], &p[1], &p[2], &blocks,
                    &bundle, &cls, &x3n, &ring, &cb, &mode, &gram) == 16) {
    bcg::LatticeDev lat{};
    lat.ndim = 4;
    lat.V = 1;
    for (int mu = 0; mu < 4; ++mu) {
      lat.L[mu] = L[mu];
      lat.stride[mu] = lat.V;
      lat.V *= L[mu];
    }
    for (int mu = 0; mu < 4; ++mu) lat.face_sites[mu] = lat.V / L[mu];
    bcg::HopTuning tune;
    for (int k = 0; k < 3; ++k) tune.patch[k] = p[k];
    tune.blocks = blocks;
    tune.sync.bundle_walk = bundle;
    bcg::HopRequest rq;
    rq.m = m;
    rq.mode = static_cast<bcg::HopMode>(mode);
    rq.gram = gram != 0;
    rq.tile_class = cls;
    rq.win = bcg::HopWindow{0, x3n, ring, cb, 0};
    const bcg::HopLaunchPlan pl = bcg::hop_plan(lat, 1024, tune, rq);
    std::printf("%d %zu %d\n", static_cast<int>(pl.form), pl.lds, pl.grid);
  }
  return 0;
}
