// Compile-only: blockcg/lowmodes.hpp -- the mutable basis, the in-place rotation, the bound and both overloads of
// lowest_modes -- and the three C entries with the documented signatures.
#include <cstdint>
#include <vector>

#include "blockcg/lowmodes.hpp"

double use(const dirac_op& D, block_fermion_field<32>& v0, block_fermion_field<16>& v1, block_fermion_field<16>& w,
           block_fermion_field<8>& B, std::vector<block_fermion_field<8>>& X) {
  blockcg::mutable_basis V;
  V.push_back(v0);
  V.push_back(v1);
  blockcg::basis_matrix Q(static_cast<size_t>(V.K()) * V.K());
  blockcg::basis_rotate(V, Q);
  const double ub = blockcg::spectral_bound(D) + blockcg::spectral_bound(D, 10, 3ULL, 0);
  blockcg::lowest_modes_result r = blockcg::lowest_modes(V, D, 32, ub);
  blockcg::mutable_basis W;
  W.push_back(w);
  const blockcg::lowest_modes_result r2 = blockcg::lowest_modes(W, V.as_basis(), D, 8, ub, 16, 1e-10, 50);
  std::vector<double> sigma(X.size(), 0.0);
  const int its = blockcg::SBCGrQ_deflated(X, B, D, sigma, V.as_basis(), r.evals, 1e-10, 1e-10, 1000);
  return r.resid[0] + r2.evals[0] + r.iterations + static_cast<double>(r2.applications) + its;
}

static_assert(BCG_BASIS_ROTATE_MAX_COLUMNS == 64, "the width limit is a named constant");
int (*p_rotate)(bcg_field* const*, int, const double*) = &bcg_basis_rotate;
int (*p_bound)(bcg_context*, const bcg_gauge*, double, int, int, uint64_t, double*) = &bcg_spectral_bound;
int (*p_modes)(bcg_context*, const bcg_gauge*, double, bcg_field* const*, int, const bcg_field* const*, int, int, int, double,
               double, int, double*, double*, int*, int64_t*) = &bcg_lowest_modes;

int main() { return p_rotate && p_bound && p_modes ? 0 : 1; }
