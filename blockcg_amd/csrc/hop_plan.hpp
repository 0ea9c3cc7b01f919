// The specialised 4-D stencil, host side: hop_plan (hop_plan.cpp, host only) says what one launch will be, hop_launch
// (kernels_stencil.hip) executes it.  A caller plans before it launches -- every launch of a pair before the first one runs.
#pragma once
#include "kernels_mfma.hpp"

namespace bcg {

enum HopForm {
  HOP_FORM_NONE = 0,   // declined: no specialised kernel honours the whole request (the caller runs a generic kernel)
  HOP_FORM_ROW,        // k_hop4: tile counter, or the boundary class from its tile list
  HOP_FORM_COLUMN,     // k_hop4c: column sweep
  HOP_FORM_BUNDLE,     // k_hop4b: 2 x 2 column bundles
  HOP_FORM_BUNDLE_CB,  // k_hop4b, checkerboard form (half-volume fields)
};

struct HopRequest {
  int m = 0;
  HopMode mode = HOP_PLAIN;
  bool gram = false;         // the fused Gram product (HOP_SHIFTED: p^dagger out; HOP_RESID, HOP_FACT2, HOP_FACT1G and HOP_FACT2B carry theirs)
  int tile_class = 0;        // 0 whole launch, 1 interior tiles, 2 boundary tiles (HopTuning::boundary_list)
  HopWindow win;
  bool fold_target = false;  // HopTuning::fold may be used: fold the Gram partials in the kernel where the form can
};

// Everything hop_launch needs besides the operands.  Plain data: the pointers are the tuning's, never dereferenced here.
struct HopLaunchPlan {
  HopForm form = HOP_FORM_NONE;
  HopRequest req;                 // width, mode, gram and class select the instantiation
  LatticeDev lat{};
  HopWindow win;                  // the effective window (all slices spelled out)
  bool capped_interior = false;   // k_hop4c's interior class through its register-capped entry point
  int grid = 0, ntiles = 0;       // grid 0: an empty tile list, nothing is launched
  size_t lds = 0;                 // dynamic LDS, bytes
  int p0 = 0, p1 = 0, p2 = 0, xcd_split = 0, super = 0;  // the walk (HopWalk)
  const int* tile_list = nullptr;  // the boundary class's tiles (k_hop4)
  int list_n = 0;
  unsigned* sync = nullptr;       // pacing counters, zeroed by the launcher (nullptr: unpaced)
  int sync_window = 0, sync_stride = 0, sync_limit = 0;
  GramFold fold;                  // fold.out != nullptr: the launch folds its Gram partials
};

// Pure (no HIP call, no device memory touched).  Never honours part of a request: a Gram product the chosen form does not
// have, a mode or a window it cannot serve give HOP_FORM_NONE.
HopLaunchPlan hop_plan(const LatticeDev& lat, int max_blocks, const HopTuning& tune, const HopRequest& request);

// Both launches of the factored pair (A + sigma0 = (mu + D)(mu - D), whole full-volume fields at m = 16), planned together:
// HOP_FACT1 then HOP_FACT2, or with phase B of SBCGrQ inside the second factor HOP_FACT1G then HOP_FACT2B (kernels.hpp).
// fold: HopRequest::fold_target of the launches that carry a Gram product.  Pure, like hop_plan.
struct HopPairPlan {
  HopLaunchPlan f1, f2;
  bool taken = false;  // the pair exists in the bundle sweep only: both plans are HOP_FORM_BUNDLE
};
HopPairPlan hop_plan_pair(const LatticeDev& lat, int max_blocks, const HopTuning& tune, int m, bool with_phase_b, bool fold);
// Launches a plan whose form is not HOP_FORM_NONE; returns the grid (= the blocks that wrote Gram partials).
int hop_launch(hipStream_t s, const HopLaunchPlan& plan, const double2* U, const double2* Ughost, const double2* in,
               const double2* ghost, double2* out, const double2* p, double c0, double2* partials,
               const double2* mats = nullptr, int has_rinv = 0);  // (HOP_FACT2B: [-alpha][rho_prev^-1], kernels.hpp)

}  // namespace bcg
