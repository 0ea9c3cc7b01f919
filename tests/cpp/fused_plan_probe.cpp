// Host-only probe of the stencil planner for the requests of the factored pair (HOP_FACT1, HOP_FACT2; with phase B inside:
// HOP_FACT1G, HOP_FACT2B) and of the pair planner that spells them.  Every line starts with the lattice and the tuning,
// "m L0 L1 L2 L3 patch0 patch1 patch2 blocks bundle_walk"; then
//   (no argument)  "cls x3_n ring cb mode gram"       prints "<form> <lds> <grid>" of hop_plan (form 0 = declined)
//   full           "cls x3_n ring cb mode gram fold"  prints every field of the plan (print_plan)
//   pair           "with_phase_b fold"                prints "<taken>", then every field of both plans of hop_plan_pair
// full and pair plan with pacing counters and fold buffers present, as on a context after its scratch is allocated.
// tests/test_fused_plan_cpu.py links it with hop_plan.o alone.
#include <cstdio>
#include <cstring>

#include "../../blockcg_amd/csrc/hop_plan.hpp"

static unsigned counters[1], tickets[1];  // (named by the plans, never dereferenced)
static double2 fold_out[1];

// form, LDS, grid, tiles, the walk, the pacing, the fold flag
static void print_plan(const bcg::HopLaunchPlan& pl) {
  std::printf(" %d %zu %d %d %d %d %d %d %d %d %d %d %d %d", static_cast<int>(pl.form), pl.lds, pl.grid, pl.ntiles, pl.p0, pl.p1, pl.p2,
              pl.xcd_split, pl.super, pl.sync != nullptr, pl.sync_window, pl.sync_stride, pl.sync_limit, pl.fold.out != nullptr);
}

int main(int argc, char** argv) {
  const bool pair = argc > 1 && !std::strcmp(argv[1], "pair"), full = argc > 1 && !std::strcmp(argv[1], "full");
  int m, L[4], p[3], blocks, bundle, cls, x3n, ring, cb, mode, gram, fold = 0, with_b;
  while (std::scanf("%d %d %d %d %d %d %d %d %d %d", &m, &L[0], &L[1], &L[2], &L[3], &p[0], &p[1], &p[2], &blocks, &bundle) == 10) {
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
    if (pair || full) {
      tune.sync.counters = counters;
      tune.sync.stride = 8192;
      tune.fold = bcg::GramFold{fold_out, tickets};
    }
    if (pair) {
      if (std::scanf("%d %d", &with_b, &fold) != 2) return 1;
      const bcg::HopPairPlan pp = bcg::hop_plan_pair(lat, 1024, tune, m, with_b != 0, fold != 0);
      std::printf("%d", pp.taken ? 1 : 0);
      print_plan(pp.f1);
      print_plan(pp.f2);
      std::printf("\n");
      continue;
    }
    if (std::scanf("%d %d %d %d %d %d", &cls, &x3n, &ring, &cb, &mode, &gram) != 6 || (full && std::scanf("%d", &fold) != 1)) return 1;
    bcg::HopRequest rq;
    rq.m = m;
    rq.mode = static_cast<bcg::HopMode>(mode);
    rq.gram = gram != 0;
    rq.tile_class = cls;
    rq.win = bcg::HopWindow{0, x3n, ring, cb, 0};
    rq.fold_target = fold != 0;
    const bcg::HopLaunchPlan pl = bcg::hop_plan(lat, 1024, tune, rq);
    if (full) print_plan(pl), std::printf("\n");
    else std::printf("%d %zu %d\n", static_cast<int>(pl.form), pl.lds, pl.grid);
  }
  return 0;
}
