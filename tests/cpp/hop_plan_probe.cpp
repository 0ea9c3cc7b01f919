// Prints what bcg::hop_plan decides for every request of a case file (tests/hop_plan_cases.py writes it: one request per
// line, integers), one line per request.  Host only: links blockcg_amd/csrc/hop_plan.cpp's object and nothing else.
//   declined | empty | <kernel instantiation> lds=.. pace=.. fold=.. grid=.. walk=p0,p1,p2,xcd_split,super win=lo,n,ring
#include <cstdio>
#include <string>

#include "../../blockcg_amd/csrc/hop_plan.hpp"

using namespace bcg;

// the instantiation hop_launch (kernels_stencil.hip) dispatches a plan to
static std::string instantiation(const HopLaunchPlan& pl) {
  static const char* modes[] = {"HOP_PLAIN", "HOP_SHIFTED", "HOP_RESID", "HOP_FACT1", "HOP_FACT2"};
  const std::string head = std::to_string(pl.req.m) + "," + modes[pl.req.mode] + "," + (pl.req.gram ? "true" : "false");
  const char* ring = pl.win.ring > 0 ? "true" : "false";
  const int cls = pl.win.ring > 0 || pl.tile_list ? 0 : pl.req.tile_class;
  switch (pl.form) {
    case HOP_FORM_BUNDLE_CB: return "k_hop4b<" + head + ",false,true>";
    case HOP_FORM_BUNDLE: return "k_hop4b<" + head + "," + ring + ",false>";
    case HOP_FORM_COLUMN:
      return pl.capped_interior ? "k_hop4c_interior<" + head + ">" : "k_hop4c<" + head + "," + std::to_string(cls) + "," + ring + ">";
    default: return "k_hop4<" + head + ",true," + std::to_string(cls) + "," + ring + ">";
  }
}

int main(int argc, char** argv) {
  FILE* f = argc > 1 ? std::fopen(argv[1], "r") : stdin;
  if (!f) return 2;
  static unsigned counters[1];
  static int tiles[1];
  static double2 gram_out[1];
  int m, L[4], split[4], patch_walk, patch[3], blocks, column_walk, bundle_walk, bundle_window, super_patch, window, cls, list_n,
      lo, n, ring, cb, mode, gram, fold;
  while (std::fscanf(f, "%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d", &m, &L[0], &L[1], &L[2],
                     &L[3], &split[0], &split[1], &split[2], &split[3], &patch_walk, &patch[0], &patch[1], &patch[2], &blocks,
                     &column_walk, &bundle_walk, &bundle_window, &super_patch, &window, &cls, &list_n, &lo, &n, &ring, &cb, &mode,
                     &gram, &fold) == 28) {
    LatticeDev lat{};
    lat.ndim = 4;
    lat.V = 1;
    for (int mu = 0; mu < 4; ++mu) {
      lat.L[mu] = L[mu];
      lat.split[mu] = split[mu];
      lat.stride[mu] = lat.V;
      lat.V *= L[mu];
    }
    for (int mu = 0; mu < 4; ++mu) lat.face_sites[mu] = L[mu] ? lat.V / L[mu] : 0;
    HopTuning tune;
    tune.patch_walk = patch_walk != 0;
    for (int k = 0; k < 3; ++k) tune.patch[k] = patch[k];
    tune.blocks = blocks;
    tune.super_patch = super_patch;
    tune.sync.counters = counters;  // as the context allocates them
    tune.sync.stride = 8192;
    tune.sync.window = window;
    tune.sync.column_walk = column_walk != 0;
    tune.sync.bundle_walk = bundle_walk;
    tune.sync.bundle_window = bundle_window;
    if (list_n >= 0) {
      tune.boundary_list = tiles;
      tune.boundary_n = list_n;
    }
    if (fold) tune.fold = GramFold{gram_out, counters};
    HopRequest rq;
    rq.m = m;
    rq.mode = static_cast<HopMode>(mode);
    rq.gram = gram != 0;
    rq.tile_class = cls;
    rq.win.x3_lo = lo;
    rq.win.x3_n = n;
    rq.win.ring = ring;
    rq.win.cb = cb;
    rq.fold_target = fold != 0;
    const HopLaunchPlan pl = hop_plan(lat, 1024, tune, rq);
    if (pl.form == HOP_FORM_NONE) std::puts("declined");
    else if (pl.grid == 0) std::puts("empty");
    else
      std::printf("%s lds=%zu pace=%d fold=%d grid=%d walk=%d,%d,%d,%d,%d win=%d,%d,%d\n", instantiation(pl).c_str(), pl.lds,
                  pl.sync ? pl.sync_window : 0, pl.fold.out != nullptr, pl.grid, pl.p0, pl.p1, pl.p2, pl.xcd_split, pl.super,
                  pl.win.x3_lo, pl.win.x3_n, pl.win.ring);
  }
  return 0;
}
