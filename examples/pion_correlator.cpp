// examples/pion_correlator.cpp -- a measurement that never moves a field through host memory: point sources in the three
// colours at the origin, one SBCGrQ solve, and the sum per time slice and column of |X|^2 (block_fermion_field::slice_dot),
// C_j(t) = sum_{x: x_3 = t} sum_c |X_j(x, c)|^2.  Prints C(t) = sum_j C_j(t); exit code 0 = every C(t) is positive and the
// sum over t equals the diagonal of hermitian_dot.
//   pion_correlator [L0 L1 L2 L3 [mass]]      default 8 8 8 16, mass 0.5
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "blockcg/block_solvers.hpp"

int main(int argc, char** argv) {
  std::vector<int> dims = {8, 8, 8, 16};
  if (argc >= 5)
    for (int mu = 0; mu < 4; ++mu) dims[mu] = std::atoi(argv[1 + mu]);
  const double mass = argc >= 6 ? std::atof(argv[5]) : 0.5;
  blockcg::lattice lat(dims);
  dirac_op D(lat, mass, /*seed=*/7ull);
  block_fermion_field<3> B(lat);
  B.setPointSources({{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}}, {0, 1, 2});
  std::vector<block_fermion_field<3>> X(1, B);
  std::vector<double> sigma = {0.0};
  const int iterations = SBCGrQ(X, B, D, sigma, 1e-12, 1e-12);
  const std::vector<std::complex<double>> C = X[0].slice_dot(X[0], 3);
  const block_matrix<3> G = X[0].hermitian_dot(X[0]);
  std::printf("# point sources at the origin, %dx%dx%dx%d, mass %g: %d iterations\n# t  C(t)\n", dims[0], dims[1], dims[2], dims[3],
              mass, iterations);
  bool ok = iterations > 0;
  double total[3] = {0.0, 0.0, 0.0};
  for (int t = 0; t < dims[3]; ++t) {
    double c = 0.0;
    for (int j = 0; j < 3; ++j) {
      c += C[t * 3 + j].real();
      total[j] += C[t * 3 + j].real();
    }
    ok = ok && c > 0.0;
    std::printf("%3d  %.12e\n", t, c);
  }
  for (int j = 0; j < 3; ++j) ok = ok && std::fabs(total[j] - G(j, j).real()) <= 1e-12 * G(j, j).real();
  std::printf("%s\n", ok ? "CORRELATOR_OK" : "CORRELATOR_FAILED");
  return ok ? 0 : 1;
}
