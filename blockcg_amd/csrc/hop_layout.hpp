// What the specialised stencil's kernels (kernels_stencil.hip) and their planner (hop_plan.cpp) must agree on: the switch
// that selects the bundle sweep's schedule and the LDS layout of each form (counts of complex numbers, 16 bytes each).
#pragma once
#include <cstddef>

// PIPE: the software-pipelined schedule of the bundle sweep (m = 16, 32) -- see "PIPE" in hop4b_body.
// -DBCG_HOP4B_PIPE=0 is the A/B build: the step of rounds 1-3 (still what m = 8 and the residual form run).
#ifndef BCG_HOP4B_PIPE
#define BCG_HOP4B_PIPE 1
#endif
#ifdef __HIP__
#define BCG_LAYOUT_FN __host__ __device__ constexpr
#else
#define BCG_LAYOUT_FN constexpr
#endif

namespace bcg {
// k_hop4b: two link images per wave (partner waves read each other's forward links) where two blocks per CU still fit the
// 160 KB of LDS: m = 16 (73.7 KB per block) and m = 32 (70 KB); at m = 8 (two images: 100 KB) one image, own links only.
BCG_LAYOUT_FN bool hop4b_share_images(int m) { return m >= 16; }
// k_hop4 / k_hop4c, one link image of a tile of spb = 4 * (64 / m) sites: forward links of sites -1 .. spb - 1 (all four
// directions), backward links of directions 1..3.  k_hop4c holds two images; k_hop4 three with the fused Gram product.
BCG_LAYOUT_FN int hop4_fwd_links(int m) { return (4 * (64 / m) + 1) * 36; }
BCG_LAYOUT_FN int hop4_bwd_links(int m) { return 3 * 4 * (64 / m) * 9; }
BCG_LAYOUT_FN size_t hop4_lds_bytes(int m, int images) { return size_t(16) * images * (hop4_fwd_links(m) + hop4_bwd_links(m)); }
// k_hop4b, per wave (spw = 64 / m sites): a row slot (halo site, spw sites, halo site); a link image: the slot of the site
// to the left (U_0 only) and the forward links, then the backward links of directions 1..3 (checkerboard form: and 0).
// A block: [2 slots][4 waves] rows, then [1 or 2 images][4 waves] links.
BCG_LAYOUT_FN int hop4b_row_slot(int m) { return (64 / m + 2) * 3 * m; }
BCG_LAYOUT_FN int hop4b_fwd_links(int m) { return (64 / m + 1) * 36; }
BCG_LAYOUT_FN int hop4b_bwd_links(int m, bool cb) { return (cb ? 4 : 3) * (64 / m) * 9; }
BCG_LAYOUT_FN size_t hop4b_lds_bytes(int m, bool cb) {
  return size_t(16) * 4 * (2 * hop4b_row_slot(m) + (hop4b_share_images(m) ? 2 : 1) * (hop4b_fwd_links(m) + hop4b_bwd_links(m, cb)));
}
// k_hop4b_fusedB (m = 16): behind the sweep's 73 728 B, -alpha and rho_prev^-1 unpadded, 16 bytes per entry: 8 192 B, which
// makes a block exactly half of a CU's 160 KB
BCG_LAYOUT_FN size_t hop4b_fusedB_mats_bytes(int m) { return size_t(16) * 2 * m * m; }
static_assert(2 * (hop4b_lds_bytes(16, false) + hop4b_fusedB_mats_bytes(16)) == 160 * 1024, "fused phase B: two blocks per CU");
// every form: the block reduction of the fused Gram product re-uses the memory (4 waves x 8 x 64 doubles)
constexpr size_t kHopGramLdsBytes = 8 * 4 * 8 * 64;
}  // namespace bcg
