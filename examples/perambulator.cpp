// examples/perambulator.cpp -- a perambulator against a basis that never leaves the device: 16 orthonormal columns V (noise,
// orthonormalised; a distillation basis from blockcg/lowmodes.hpp goes in the same way), the sources B = V restricted to the
// time slice t0, one SBCGrQ solve, and the solution taken against the basis slice by slice (blockcg/basis.hpp),
//   tau(t)(i, j) = sum_{x: x_3 = t} sum_c conj(V_i(x, c)) X_j(x, c).
// A self-check that needs no solve comes first: with b = the sources themselves the result is exactly zero off the source
// slice and V(t0)^dagger V(t0) -- the slice's Gram matrix of V -- on it.  Prints t and the trace of tau(t); exit code 0 and
// PERAMBULATOR_OK = the self-check holds and the sum over t of tau(t) is basis_dot(V, X).
//   perambulator [L0 L1 L2 L3 [mass [t0]]]      default 8 8 8 16, mass 0.5, t0 = 1
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "blockcg/basis.hpp"

int main(int argc, char** argv) {
  typedef std::complex<double> cd;
  const int N = 16;
  std::vector<int> dims = {8, 8, 8, 16};
  if (argc >= 5)
    for (int mu = 0; mu < 4; ++mu) dims[mu] = std::atoi(argv[1 + mu]);
  const double mass = argc >= 6 ? std::atof(argv[5]) : 0.5;
  const int T = dims[3], t0 = argc >= 7 ? std::atoi(argv[6]) % T : 1 % T;
  blockcg::lattice lat(dims);
  dirac_op D(lat, mass, /*seed=*/7ull);

  block_fermion_field<N> q(lat);
  q.setGaussian(41);
  block_matrix<N> R;
  q.thinQR(R);
  blockcg::basis V;
  V.push_back(q);

  // B = V on the slice x_3 = t0, zero elsewhere (written through the host mirror; sites are lexicographic, x_0 fastest)
  const block_fermion_field<N>& cq = q;
  block_fermion_field<N> B(lat);
  const int per_slice = B.V / T;
  for (int x = 0; x < B.V; ++x)
    for (int j = 0; j < N; ++j)
      for (int c = 0; c < 3; ++c) B[x](c, j) = x / per_slice == t0 ? cq[x](c, j) : cd(0.0, 0.0);

  // the self-check: V(t)^dagger B is zero off the source slice and V(t0)^dagger V(t0) on it
  const std::vector<blockcg::basis_matrix> self = blockcg::basis_slice_dot(V, B, 3);
  const std::vector<block_matrix<N>> G = cq.slice_gram(cq, 3);
  bool ok = self.size() == static_cast<size_t>(T);
  double off_slice = 0.0, on_slice = 0.0;
  for (int t = 0; ok && t < T; ++t)
    for (int j = 0; j < N; ++j)
      for (int i = 0; i < N; ++i) {
        const cd got = self[t][j * N + i];
        if (t == t0) on_slice = std::fmax(on_slice, std::abs(got - G[t0](i, j)) / std::sqrt(G[t0](i, i).real() * G[t0](j, j).real()));
        else off_slice = std::fmax(off_slice, std::abs(got));
      }
  ok = ok && off_slice == 0.0 && on_slice <= 1e-13;
  std::printf("# self-check: largest entry off the source slice %.3e, error on it %.3e\n", off_slice, on_slice);

  std::vector<block_fermion_field<N>> X(1, block_fermion_field<N>(lat));
  std::vector<double> sigma = {0.0};
  const int iterations = SBCGrQ(X, B, D, sigma, 1e-12, 1e-12);
  const std::vector<blockcg::basis_matrix> tau = blockcg::basis_slice_dot(V, X[0], 3);
  const blockcg::basis_matrix whole = blockcg::basis_dot(V, X[0]);
  std::printf("# %dx%dx%dx%d, mass %g, sources on t0 = %d: %d iterations\n# t  tr tau(t) re im\n", dims[0], dims[1], dims[2], dims[3],
              mass, t0, iterations);
  ok = ok && iterations > 0 && tau.size() == static_cast<size_t>(T);
  std::vector<cd> total(whole.size());
  double size = 0.0;
  for (int t = 0; ok && t < T; ++t) {
    cd tr = 0.0;
    for (int i = 0; i < N; ++i) tr += tau[t][i * N + i];
    for (size_t k = 0; k < total.size(); ++k) total[k] += tau[t][k];
    std::printf("%3d  %.14e %.14e\n", t, tr.real(), tr.imag());
  }
  for (const cd& z : whole) size = std::fmax(size, std::abs(z));
  for (size_t k = 0; ok && k < total.size(); ++k) ok = std::abs(total[k] - whole[k]) <= 1e-12 * size;
  std::printf("%s\n", ok ? "PERAMBULATOR_OK" : "PERAMBULATOR_FAILED");
  return ok ? 0 : 1;
}
