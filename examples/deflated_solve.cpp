// examples/deflated_solve.cpp -- a deflated multi-shift solve whose low modes never leave the device: the spectral bound from
// a short Lanczos run, 48 eigenvectors from Chebyshev-filtered subspace iteration in two stages (blockcg/lowmodes.hpp: the
// lowest 32 of a block of 48, then 16 more from a block of 32 kept orthogonal to those -- the columns a stage carries
// beyond the wanted ones are what gives its filter a gap), then SBCGrQ_deflated on the 48 against the plain solve.  Prints
// the operator applications of both and DEFLATED_SOLVE_OK when every true residual is within 100 eps and the deflated solve
// needed fewer applications.
//   deflated_solve [L0 L1 L2 L3 [mass]]      default 4 4 4 2, mass 0.05
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "blockcg/lowmodes.hpp"

int main(int argc, char** argv) {
  std::vector<int> dims = {4, 4, 4, 2};
  if (argc >= 5)
    for (int mu = 0; mu < 4; ++mu) dims[mu] = std::atoi(argv[1 + mu]);
  const double mass = argc >= 6 ? std::atof(argv[5]) : 0.05;
  const double eps = 1e-10;
  blockcg::lattice lat(dims);
  dirac_op D(lat, mass, /*seed=*/7ull);

  const double ub = blockcg::spectral_bound(D, 10, /*seed=*/3ull);
  block_fermion_field<32> v0(lat);
  block_fermion_field<16> v1(lat);
  v0.setGaussian(21);
  v1.setGaussian(22);
  blockcg::mutable_basis V;
  V.push_back(v0);
  V.push_back(v1);
  const double tol = 1e-10;
  const blockcg::lowest_modes_result first = blockcg::lowest_modes(V, D, 32, ub, 16, tol, 100);
  // the second stage: v0 (the 32 converged columns) locked, 16 wanted of a fresh block of 32
  block_fermion_field<16> w0(lat), w1(lat);
  w0.setGaussian(23);
  w1.setGaussian(24);
  blockcg::mutable_basis W;
  W.push_back(w0);
  W.push_back(w1);
  blockcg::basis locked;
  locked.push_back(v0);
  const blockcg::lowest_modes_result second = blockcg::lowest_modes(W, locked, D, 16, ub, 16, tol, 100);
  blockcg::basis modes;  // the 48 converged columns
  modes.push_back(v0);
  modes.push_back(w0);
  std::vector<double> evals(first.evals.begin(), first.evals.begin() + 32);
  evals.insert(evals.end(), second.evals.begin(), second.evals.begin() + 16);
  double worst_mode = 0.0;
  for (int i = 0; i < 32; ++i) worst_mode = std::fmax(worst_mode, first.resid[i]);
  for (int i = 0; i < 16; ++i) worst_mode = std::fmax(worst_mode, second.resid[i]);
  std::printf("# %dx%dx%dx%d, mass %g: bound %.6g, %d + %d outer iterations, %lld + %lld block applications\n", dims[0], dims[1],
              dims[2], dims[3], mass, ub, first.iterations, second.iterations, static_cast<long long>(first.applications),
              static_cast<long long>(second.applications));
  std::printf("# eigenvalues %.6e .. %.6e, worst residual %.3e\n", evals.front(), evals.back(), worst_mode);

  block_fermion_field<8> B(lat);
  B.setGaussian(5);
  std::vector<double> sigma = {0.0, 0.05, 0.5};
  std::vector<block_fermion_field<8>> X(sigma.size(), block_fermion_field<8>(lat)), Xp(sigma.size(), block_fermion_field<8>(lat));
  const int deflated = blockcg::SBCGrQ_deflated(X, B, D, sigma, modes, evals, eps, eps);
  const int plain = SBCGrQ(Xp, B, D, sigma, eps, eps);
  std::vector<bcg_field*> Xh(X.size());
  for (size_t s = 0; s < X.size(); ++s) Xh[s] = X[s].handle();
  std::vector<double> res(sigma.size() * 8);
  blockcg::check(bcg_true_residuals(lat.ctx(), D.handle(), D.mass, Xh.data(), B.handle(), static_cast<int>(sigma.size()), sigma.data(),
                                    res.data()),
                 lat.ctx(), "true_residuals");
  double worst = 0.0;
  for (double r : res) worst = std::fmax(worst, r);
  std::printf("operator applications: %d deflated, %d plain; worst true residual %.3e\n", deflated, plain, worst);
  const bool ok = worst_mode <= tol * ub && worst <= 100.0 * eps && deflated < plain;
  std::printf("%s\n", ok ? "DEFLATED_SOLVE_OK" : "DEFLATED_SOLVE_FAILED");
  return ok ? 0 : 1;
}
