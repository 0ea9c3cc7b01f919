// examples/momentum_correlator.cpp -- a momentum-projected two-point function without moving a field through host memory:
// point sources in the three colours at the origin, one SBCGrQ solve, and the per-slice Gram matrices of the solution with
// itself along time (block_fermion_field::slice_gram) at the momenta (0,0,0), (1,0,0) and (-1,0,0),
//   C_p(t) = sum_i sum_{x: x_3 = t} exp(-2 pi i p.x / L) sum_c |X_i(x, c)|^2.
// Prints t, C_0(t), C_{+1}(t), C_{-1}(t) (re and im each); exit code 0 = C_0(t) is real and positive, C_{-p} = conj(C_p),
// and the sum over t of the p = 0 matrices is hermitian_dot.
//   momentum_correlator [L0 L1 L2 L3 [mass]]      default 8 8 8 16, mass 0.5
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
  const int T = dims[3];
  const std::vector<block_matrix<3>> C = X[0].slice_gram(X[0], 3, {{0, 0, 0, 0}, {1, 0, 0, 0}, {-1, 0, 0, 0}});
  const block_matrix<3> G = X[0].hermitian_dot(X[0]);
  std::printf("# point sources at the origin, %dx%dx%dx%d, mass %g: %d iterations\n", dims[0], dims[1], dims[2], dims[3], mass,
              iterations);
  std::printf("# t  C_0(t) re im  C_+1(t) re im  C_-1(t) re im\n");
  bool ok = iterations > 0 && C.size() == static_cast<size_t>(3 * T);
  std::complex<double> total[3][3] = {};
  for (int t = 0; ok && t < T; ++t) {
    std::complex<double> c[3];
    for (int p = 0; p < 3; ++p)
      for (int i = 0; i < 3; ++i) c[p] += C[p * T + t](i, i);
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) total[i][j] += C[t](i, j);
    ok = ok && c[0].real() > 0.0 && std::abs(c[0].imag()) <= 1e-13 * c[0].real();
    ok = ok && std::abs(c[1] - std::conj(c[2])) <= 1e-13 * c[0].real();
    std::printf("%3d  %.14e %.14e  %.14e %.14e  %.14e %.14e\n", t, c[0].real(), c[0].imag(), c[1].real(), c[1].imag(), c[2].real(),
                c[2].imag());
  }
  double norm = 0.0;
  for (int i = 0; i < 3; ++i) norm += G(i, i).real();
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) ok = ok && std::abs(total[i][j] - G(i, j)) <= 1e-12 * norm;
  std::printf("%s\n", ok ? "MOMENTUM_CORRELATOR_OK" : "MOMENTUM_CORRELATOR_FAILED");
  return ok ? 0 : 1;
}
