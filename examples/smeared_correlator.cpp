// examples/smeared_correlator.cpp -- a smeared-smeared two-point function without moving a field through host memory:
// point sources in the three colours at the origin, smeared along the three spatial directions (blockcg::smear: n steps of
// 1 + kappa Lap_3 with the operator's links), one SBCGrQ solve, the solution smeared with the same call at the sink, and the
// per-slice Gram matrices along time for the 3 x 3 correlator matrix between source colours,
//   C_ij(t) = sum_{x: x_3 = t} sum_c conj(X_i(x, c)) X_j(x, c).
// Prints t and the nine entries (re im, row-major); exit code 0 = the smeared source stayed on its time slice, every C(t) is
// Hermitian with a positive diagonal, and the sum over t is hermitian_dot.
//   smeared_correlator [L0 L1 L2 L3 [mass [kappa [steps]]]]      default 8 8 8 16, mass 0.5, kappa 0.1, 4 steps
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
  const double kappa = argc >= 7 ? std::atof(argv[6]) : 0.1;
  const int steps = argc >= 8 ? std::atoi(argv[7]) : 4;
  blockcg::lattice lat(dims);
  dirac_op D(lat, mass, /*seed=*/7ull);
  block_fermion_field<3> B(lat), work(lat);
  B.setPointSources({{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}}, {0, 1, 2});
  blockcg::smear(B, D, /*dir=*/3, kappa, steps, &work);  // the source, smeared in space
  const int T = dims[3];
  const std::vector<block_matrix<3>> S = B.slice_gram(B, 3);
  bool ok = S.size() == static_cast<size_t>(T);
  for (int t = 1; ok && t < T; ++t)
    for (int i = 0; i < 3; ++i) ok = ok && S[t](i, i) == std::complex<double>(0.0, 0.0);  // nothing left its time slice
  std::vector<block_fermion_field<3>> X(1, B);
  std::vector<double> sigma = {0.0};
  const int iterations = SBCGrQ(X, B, D, sigma, 1e-12, 1e-12);
  blockcg::smear(X[0], D, 3, kappa, steps, &work);  // the sink, by the same call
  const std::vector<block_matrix<3>> C = X[0].slice_gram(X[0], 3);
  const block_matrix<3> G = X[0].hermitian_dot(X[0]);
  std::printf("# smeared point sources at the origin (kappa %g, %d steps), %dx%dx%dx%d, mass %g: %d iterations\n", kappa, steps,
              dims[0], dims[1], dims[2], dims[3], mass, iterations);
  std::printf("# t  C_00 re im  C_01 re im ... C_22 re im\n");
  ok = ok && iterations > 0 && C.size() == static_cast<size_t>(T);
  double norm = 0.0;
  for (int i = 0; i < 3; ++i) norm += G(i, i).real();
  std::complex<double> total[3][3] = {};
  for (int t = 0; ok && t < T; ++t) {
    std::printf("%3d", t);
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        total[i][j] += C[t](i, j);
        ok = ok && std::abs(C[t](i, j) - std::conj(C[t](j, i))) <= 1e-12 * norm;
        std::printf("  %.14e %.14e", C[t](i, j).real(), C[t](i, j).imag());
      }
    std::printf("\n");
    for (int i = 0; i < 3; ++i) ok = ok && C[t](i, i).real() > 0.0;
  }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) ok = ok && std::abs(total[i][j] - G(i, j)) <= 1e-12 * norm;
  std::printf("%s\n", ok ? "SMEARED_CORRELATOR_OK" : "SMEARED_CORRELATOR_FAILED");
  return ok ? 0 : 1;
}
