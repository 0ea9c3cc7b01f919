// Host-only: which kernel of the specialised 4-D stencil serves a launch, and with what grid, LDS, walk and pacing.
// The one place that decides; hop_launch (kernels_stencil.hip) executes what is decided here.
#include "hop_layout.hpp"
#include "hop_plan.hpp"

namespace bcg {

bool hop_fast_width(int m) { return m == 8 || m == 16 || m == 32; }
// tile = spb consecutive x0 sites of one row, 32-bit site arithmetic
bool hop_can_split_tiles(int m, const LatticeDev& lat) {
  const int spb = 4 * (64 / m);
  return hop_fast_width(m) && lat.ndim == 4 && lat.L[0] % spb == 0 && lat.V < (int64_t(1) << 31) - 2 * lat.stride[3];
}

namespace {
// column: k_hop4c (column sweep, scalar row pointers) instead of k_hop4; list: k_hop4 over an explicit tile list (boundary class)
struct Walk { bool valid = false, column = false, list = false; };

// window, tile count, walk, grid and the column form's pacing of `pl`
Walk plan_hop4(HopLaunchPlan& pl, int m, const LatticeDev& lat, int max_blocks, const HopTuning& tune, int cls, HopWindow win) {
  Walk w;
  const int SPB = 4 * (64 / m);
  // patch extent in x0: one tile unless set (a patch slice then has p1*p2 = 64 tiles = the blocks of an XCD at every width)
  const int walk = tune.patch_walk ? 3 : 0, p0 = tune.patch[0] > 0 ? tune.patch[0] : SPB, p1 = tune.patch[1], p2 = tune.patch[2];
  if (win.x3_n <= 0) win.x3_lo = 0, win.x3_n = lat.L[3];
  if (win.x3_lo < 0 || win.x3_lo + win.x3_n > lat.L[3]) return w;
  // ring addressing: whole tiles only (no interior/boundary split), direction 3 undivided, ring | L3
  if (win.ring > 0 && (cls != 0 || lat.split[3] || win.ring < 3 || lat.L[3] % win.ring != 0)) return w;
  pl.win = win;
  pl.ntiles = static_cast<int>(lat.V / lat.L[3] * win.x3_n / SPB);
  const bool list = cls == 2 && tune.boundary_list != nullptr;  // the boundary class from its tile list: lexicographic
  const bool ok3 = !list && walk == 3 && p0 > 0 && p1 > 0 && p2 > 0 && p0 % SPB == 0 && lat.L[0] % p0 == 0 && lat.L[1] % p1 == 0 &&
                   lat.L[2] % p2 == 0 && pl.ntiles % 8 == 0 && max_blocks % 8 == 0 && pl.ntiles / 8 >= max_blocks / 8;
  pl.p0 = lat.L[0], pl.p1 = lat.L[1], pl.p2 = lat.L[2], pl.xcd_split = 0;  // lexicographic = one patch
  if (ok3) pl.p0 = p0, pl.p1 = p1, pl.p2 = p2, pl.xcd_split = 1;
  if (ok3 && tune.super_patch && (lat.L[0] / p0) % 2 == 0 && (lat.L[1] / p1) % 2 == 0 && (lat.L[2] / p2) % 2 == 0) pl.super = 1;
  if (list) {  // dealt to the blocks round-robin
    pl.tile_list = tune.boundary_list, pl.list_n = tune.boundary_n;
    pl.grid = tune.boundary_n < max_blocks ? tune.boundary_n : max_blocks;
    w.list = w.valid = true;
    return w;
  }
  pl.grid = pl.ntiles < max_blocks ? pl.ntiles : max_blocks;
  if (pl.xcd_split) pl.grid &= ~7;
  // column form of the walk: one block per tile of a patch slice, whole patches per XCD class
  w.column = tune.sync.column_walk && pl.xcd_split && pl.grid / 8 == (p0 / SPB) * p1 * p2 &&
             ((lat.L[0] / p0) * (lat.L[1] / p1) * (lat.L[2] / p2)) % 8 == 0;
  if (w.column && tune.sync.window > 0 && tune.sync.counters != nullptr) {
    const int steps = pl.ntiles / pl.grid;  // tiles per block (every block has the same number)
    if (steps <= tune.sync.stride)
      pl.sync = tune.sync.counters, pl.sync_window = tune.sync.window, pl.sync_stride = tune.sync.stride, pl.sync_limit = tune.sync.limit_ticks;
  }
  w.valid = true;
  return w;
}

// k_hop4b (2 x 2 column bundles) serves whole launches of the column form whose patches are made of whole bundle tiles
// (at m = 8 the plain form only unless bundle_walk = 2: measured at 32^4, 0.36 vs 0.41 ms plain, 0.50 vs 0.44 ms with the Gram product)
bool bundle_ok(int m, const LatticeDev& lat, const HopTuning& tune, const HopLaunchPlan& pl, const Walk& w, int cls, bool plain) {
  const int spw = 64 / m;
  // short x3 windows (capacity ring 8: 6 slices) do not repay the bundle's column prologue -- two row loads before the
  // first step -- (measured at 64^3 x 128: ring 8 144.6 vs 142.6 ms per iteration, ring 16 140.4 vs 141.1 ms)
  if (pl.win.ring > 0 && pl.win.x3_n < 10 && tune.sync.bundle_walk < 2) return false;
  return w.valid && w.column && tune.sync.bundle_walk && cls == 0 && (m != 8 || plain || tune.sync.bundle_walk > 1) &&
         lat.L[1] % 2 == 0 && lat.L[2] % 2 == 0 && pl.p1 % 2 == 0 && pl.p2 % 2 == 0 && pl.p0 % spw == 0 &&
         (pl.p0 / spw) * (pl.p1 / 2) * (pl.p2 / 2) == pl.grid / 8;
}

// The bundle sweep is paced only where it is free: whole-field launches of at least 256 steps per block.  Measured
// (profiles/r03_pacing_ab_other_shapes.txt): at 64^4 (2048 steps) paced = unpaced in time with 20 % less fabric traffic; at
// 32^4, m = 8 (64 steps) the paced plain hop takes 0.376 vs 0.360 ms; capacity-mode windows (15-30 slices) 22.3 vs 21.6 ms.
// BCG_HOP_BUNDLE_SYNC < 0 forces pacing with window |value| everywhere (tests).
// Round 4: with the software-pipelined step (m = 16, 32) the capacity-mode windows gain from pacing too -- 64^3 x 128 share, ring
// 32: hop_ring 18.2 vs 18.8 ms, with the Gram product 23.8 vs 24.4, 107.6-108.1 vs 108.8 ms per iteration
// (profiles/r04_cap128_pacing_ab.txt) -- so there only the step count decides.
bool bundle_paced(int m, int ntiles, int grid, const HopWindow& win) {
  const bool pipelined = BCG_HOP4B_PIPE != 0 && hop4b_share_images(m) && win.cb == 0;
  return (win.ring == 0 || pipelined) && grid > 0 && ntiles / grid >= 256;
}

// pacing of the bundle sweep: the column form's counters with a window of its own, long sweeps only (bundle_paced)
void pace_bundle(HopLaunchPlan& pl, int m, const HopTuning& tune) {
  const int bw = tune.sync.bundle_window;
  if (bw != 0 && pl.sync && (bw < 0 || bundle_paced(m, pl.ntiles, pl.grid, pl.win))) pl.sync_window = bw < 0 ? -bw : bw;
  else pl.sync = nullptr;
}

}  // namespace

HopLaunchPlan hop_plan(const LatticeDev& lat, int max_blocks, const HopTuning& tune, const HopRequest& rq) {
  HopLaunchPlan pl;
  pl.req = rq;
  pl.lat = lat;
  const HopLaunchPlan none = pl;
  const int m = rq.m, cls = rq.tile_class, mode = rq.mode;
  const bool gram = rq.gram;
  if (!hop_can_split_tiles(m, lat)) return none;
  const Walk w = plan_hop4(pl, m, lat, tune.blocks > 0 ? tune.blocks : max_blocks, tune, cls, rq.win);
  if (!w.valid) return none;
  // whole launches of the column forms fold their Gram partials
  if (gram && w.column && cls == 0 && rq.fold_target) pl.fold = tune.fold;
  const size_t lds_g = gram ? kHopGramLdsBytes : 0;
  auto accept = [&](HopForm form, size_t lds_u) {
    pl.form = form;
    pl.lds = lds_u > lds_g ? lds_u : lds_g;
    return pl;
  };
  if (w.list && pl.grid == 0) return accept(HOP_FORM_ROW, 0);  // no boundary tiles
  // the factored pair exists in the bundle sweep only: whole full-volume fields at m = 16, FACT2 with its Gram product
  // (HOP_FACT1G, HOP_FACT2B -- the pair with phase B in the second factor: requests of their own, always with their Gram
  // products, in the pipelined step only; the fused factor keeps 8 KB of LDS for its two matrices behind the sweep's)
  const bool fused = mode == HOP_FACT1G || mode == HOP_FACT2B;
  const bool fact = mode == HOP_FACT1 || mode == HOP_FACT2 || fused;
  if (fused && BCG_HOP4B_PIPE == 0) return none;
  if (fact && (m != 16 || pl.win.cb || pl.win.ring > 0 || cls != 0 || gram != (mode != HOP_FACT1))) return none;
  // the fused residual form: m = 16 with its Gram product, whole fields
  if (mode == HOP_RESID && (m != 16 || !gram || pl.win.ring > 0 || pl.win.cb)) return none;
  // the other Gram product is HOP_SHIFTED's: at m = 16 in every form, at m = 8 in the column and bundle forms
  if (gram && !fact && mode != HOP_RESID && (mode != HOP_SHIFTED || (m != 16 && m != 8))) return none;
  // checkerboard form (half-volume fields): the bundle sweep at m = 16, 32 -- the widths with two link images per wave (the DMA
  // needs the one that is not being read) -- on a lattice whose direction 0 is not divided over ranks (lat: the compact
  // lattice, with the half ghost faces' offsets; divided, a compact row's end sites would read the ghost face in one row
  // parity only -- not built), or nothing (the caller then runs the generic half-volume kernel)
  if (pl.win.cb) {
    if (!hop4b_share_images(m) || (gram && m != 16) || pl.win.ring > 0 || cls != 0 || lat.split[0] ||
        !bundle_ok(m, lat, tune, pl, w, cls, true))
      return none;
    pace_bundle(pl, m, tune);
    return accept(HOP_FORM_BUNDLE_CB, hop4b_lds_bytes(m, true));
  }
  // k_hop4b: the column sweep over 2 x 2 bundles (whole launches only: the tile classes stay with k_hop4c)
  if (bundle_ok(m, lat, tune, pl, w, cls, mode == HOP_PLAIN)) {
    pace_bundle(pl, m, tune);
    return accept(HOP_FORM_BUNDLE, hop4b_lds_bytes(m, false) + (mode == HOP_FACT2B ? hop4b_fusedB_mats_bytes(m) : 0));
  }
  if (mode == HOP_RESID || fact) return none;  // the fused residual form and the factored pair exist in the bundle sweep only
  if (w.column) {
    // interior variants over 256 VGPRs: register-capped entry point
    pl.capped_interior = pl.win.ring == 0 && cls == 1 && (gram || m == 8);
    return accept(HOP_FORM_COLUMN, hop4_lds_bytes(m, 2));
  }
  if (gram && m != 16) return none;  // the row form's Gram product: m = 16
  return accept(HOP_FORM_ROW, hop4_lds_bytes(m, gram ? 3 : 2));
}

// the one place that spells the pair's four requests
HopPairPlan hop_plan_pair(const LatticeDev& lat, int max_blocks, const HopTuning& tune, int m, bool with_phase_b, bool fold) {
  HopPairPlan pp;
  const HopRequest first = {m, HOP_FACT1, false}, first_g = {m, HOP_FACT1G, true, 0, HopWindow(), fold};
  pp.f1 = hop_plan(lat, max_blocks, tune, with_phase_b ? first_g : first);
  pp.f2 = hop_plan(lat, max_blocks, tune, {m, with_phase_b ? HOP_FACT2B : HOP_FACT2, true, 0, HopWindow(), fold});
  pp.taken = pp.f1.form == HOP_FORM_BUNDLE && pp.f2.form == HOP_FORM_BUNDLE;
  return pp;
}

}  // namespace bcg
