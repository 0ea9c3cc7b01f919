// The front end the per-slice calls share (bcg_field_slice_gram in capi_sources.hip; bcg_basis_slice_dot and
// bcg_basis_slice_axpy in capi_basis.hip): the checks of direction and momenta, the momentum phase tables and their upload.
#pragma once
#include "capi_internal.hpp"
#include "slice_plan.hpp"

namespace bcg_impl {

// c->partials (ensure_scratch) as the per-slice calls use it: phase tables and block partials in the first half; the slice
// dot and the slice Gram reduce, and all-reduce in place, in the second
constexpr int64_t kSliceHalf = static_cast<int64_t>(kMaxGramBlocks) * 32 * 32 / 2;

inline int check_slice_dir(bcg_context* c, const char* who, int dir) {
  if (dir < 0 || dir >= c->ndim) BCG_FAIL(c, BCG_ERR_INVALID, std::string(who) + ": direction outside the lattice");
  return BCG_OK;
}

// n momenta of 4 integers each: none along dir, none beyond the lattice's dimensions
inline int check_slice_momenta(bcg_context* c, const char* who, int dir, int n, const int* momenta) {
  if (n < 0 || (n > 0 && !momenta)) BCG_FAIL(c, BCG_ERR_INVALID, std::string(who) + ": n_mom momenta are needed");
  for (int p = 0; p < n; ++p)
    for (int mu = 0; mu < 4; ++mu)
      if ((mu == dir || mu >= c->ndim) && momenta[4 * p + mu] != 0)
        BCG_FAIL(c, BCG_ERR_INVALID, std::string(who) + ": " + "momentum component along dir or beyond the lattice's dimensions");
  return BCG_OK;
}

// tabs[p][slot][walk.ltab], p < n + pad: the phases of the n momenta along the walk's three directions, from GLOBAL
// coordinates (nothing depends on the grid), conjugated where conj; then pad tables of ones (a launch's unused momenta)
inline void slice_phase_tables(const bcg_context* c, const bcg::SliceWalk& walk, const int* momenta, int n, int pad, bool conj,
                               double2* tabs) {
  const int64_t per_tab = static_cast<int64_t>(3) * walk.ltab;
  for (int64_t e = 0; e < per_tab * (n + pad); ++e) tabs[e] = make_double2(1.0, 0.0);
  for (int p = 0; p < n; ++p)
    for (int s = 0; s < 3; ++s) {
      const int mu = walk.mu[s];
      for (int x = 0; x < c->lat.L[mu]; ++x) {
        const double2 w = momentum_phase(momenta[4 * p + mu], c->lat.origin[mu] + x, c->gdims[mu]);
        tabs[p * per_tab + static_cast<int64_t>(s) * walk.ltab + x] = conj ? make_double2(w.x, -w.y) : w;
      }
    }
}

// the pc tables of the launch that begins with momentum p0
inline int upload_slice_tables(bcg_context* c, double2* tab_dev, const std::vector<double2>& tabs, int64_t per_tab, int p0, int pc) {
  HIP_TRY(c, hipMemcpyAsync(tab_dev, tabs.data() + p0 * per_tab, static_cast<size_t>(pc * per_tab) * sizeof(double2),
                            hipMemcpyHostToDevice, c->stream));
  return BCG_OK;
}

}  // namespace bcg_impl
