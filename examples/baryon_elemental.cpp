// examples/baryon_elemental.cpp -- the baryon elementals of a distillation basis, the trilinear counterpart of the meson
// elementals of examples/laplacian_distillation.cpp:
//   T(t; i, j, k) = sum_{x: x_3 = t} sum_{abc} eps_abc A_i(x,a) B_j(x,b) C_k(x,c)
//   1. unitary links, one dirac_op over them
//   2. the basis V: 16 columns of noise, laplacian_modes along direction 3
//   3. T for (V, V, V): the same list three times, so only i < j < k is computed and the rest are signed images
//   4. T for (V, V, W) with W = U_0(x) V(x + 0), covariant_shift of V: a displaced operand, the general path
//   5. V(t) <- V(t) Q(t) with Q(t) = diag(Q3(t), 1, ..., 1), Q3(t) unitary: T(t; 0, 1, 2) is multiplied by det Q3(t).
// Self-check: the antisymmetry defect of step 3, max |T(i,j,k) + T(j,i,k)|, |T(i,j,k) + T(i,k,j)|, |T(i,j,k) + T(k,j,i)| over
// all entries, is exactly 0 (so are the entries with two equal indices); step 4 with W = V reproduces step 3 to 1e-13; the
// covariance of step 5 holds to 1e-12 (the columns have unit norm on a slice, so |T| <= 1).  Exit code 0 and
// BARYON_ELEMENTAL_OK = all of it holds.
//   baryon_elemental [L0 L1 L2 L3]      default 8 8 8 16
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "blockcg/lowmodes.hpp"

namespace {
typedef std::complex<double> cd;
const int N = 16;

// [matrix][3 x 3 column-major]: the columns of a pseudo-random matrix orthonormalised one after another
std::vector<cd> unitary_matrices(size_t matrices, unsigned long long seed) {
  unsigned long long state = seed;
  auto draw = [&state]() {
    state = state * 6364136223846793005ULL + 1442695040888963407ULL;
    return static_cast<double>(state >> 11) / 9007199254740992.0 - 0.5;
  };
  std::vector<cd> U(matrices * 9);
  for (size_t k = 0; k < matrices; ++k) {
    cd* u = &U[k * 9];
    for (int j = 0; j < 3; ++j) {
      for (int i = 0; i < 3; ++i) u[3 * j + i] = cd(draw(), draw());
      for (int pass = 0; pass < 2; ++pass)
        for (int l = 0; l < j; ++l) {
          cd s = 0.0;
          for (int i = 0; i < 3; ++i) s += std::conj(u[3 * l + i]) * u[3 * j + i];
          for (int i = 0; i < 3; ++i) u[3 * j + i] -= s * u[3 * l + i];
        }
      double n = 0.0;
      for (int i = 0; i < 3; ++i) n += std::norm(u[3 * j + i]);
      for (int i = 0; i < 3; ++i) u[3 * j + i] /= std::sqrt(n);
    }
  }
  return U;
}

size_t at(int i, int j, int k) { return (static_cast<size_t>(k) * N + j) * N + i; }
}  // namespace

int main(int argc, char** argv) {
  std::vector<int> dims = {8, 8, 8, 16};
  if (argc >= 5)
    for (int mu = 0; mu < 4; ++mu) dims[mu] = std::atoi(argv[1 + mu]);
  const int T = dims[3];
  blockcg::lattice lat(dims);
  const std::vector<cd> links = unitary_matrices(static_cast<size_t>(lat.V()) * 4, 7ULL);
  dirac_op D(lat, 0.5, links.data());

  // 2. the basis
  block_fermion_field<N> v(lat);
  v.setGaussian(41);
  blockcg::mutable_basis Vm;
  Vm.push_back(v);
  const blockcg::laplacian_modes_result modes = blockcg::laplacian_modes(Vm, D, 3, N, 12.0, 16, 1e-10, 60);
  const blockcg::basis& V = Vm.as_basis();
  bool ok = modes.evals.size() == static_cast<size_t>(T);
  std::printf("# %dx%dx%dx%d: a basis of %d Laplacian modes per slice, %d outer iterations\n", dims[0], dims[1], dims[2], dims[3], N,
              modes.iterations);

  // 3. the elementals of the basis
  const std::vector<blockcg::basis_matrix> E = blockcg::basis_slice_triple(V, V, V, 3);
  ok = ok && E.size() == static_cast<size_t>(T);
  double defect = 0.0;
  std::printf("# t  T(t; 0,1,2) re im\n");
  for (int t = 0; ok && t < T; ++t) {
    const blockcg::basis_matrix& M = E[t];
    for (int k = 0; k < N; ++k)
      for (int j = 0; j < N; ++j)
        for (int i = 0; i < N; ++i) {
          const cd x = M[at(i, j, k)];
          defect = std::fmax(defect, std::fmax(std::abs(x + M[at(j, i, k)]), std::fmax(std::abs(x + M[at(i, k, j)]), std::abs(x + M[at(k, j, i)]))));
        }
    std::printf("%3d  %.14e %.14e\n", t, M[at(0, 1, 2)].real(), M[at(0, 1, 2)].imag());
  }
  ok = ok && defect == 0.0;
  std::printf("antisymmetry defect %g\n", defect);

  // 4. a displaced third operand; and the general path on the basis itself
  double general = 0.0;
  if (ok) {
    block_fermion_field<N> w(lat);
    blockcg::covariant_shift(w, v, D, 0, +1);
    blockcg::basis W, Vcopy;
    W.push_back(w);
    const std::vector<blockcg::basis_matrix> F = blockcg::basis_slice_triple(V, V, W, 3);
    ok = F.size() == static_cast<size_t>(T);
    std::printf("# t  T_displaced(t; 0,1,2) re im\n");
    for (int t = 0; ok && t < T; ++t) std::printf("%3d  %.14e %.14e\n", t, F[t][at(0, 1, 2)].real(), F[t][at(0, 1, 2)].imag());
    block_fermion_field<N> copy(lat);
    blockcg::copy_columns(copy, 0, v, 0, N);
    Vcopy.push_back(copy);
    const std::vector<blockcg::basis_matrix> G = blockcg::basis_slice_triple(V, V, Vcopy, 3);
    for (int t = 0; ok && t < T; ++t)
      for (size_t e = 0; e < G[t].size(); ++e) general = std::fmax(general, std::abs(G[t][e] - E[t][e]));
    ok = ok && general <= 1e-13;
  }
  std::printf("# general path against identical lists: %.3e (bound 1e-13)\n", general);

  // 5. covariance
  double covariance = 0.0;
  if (ok) {
    const std::vector<cd> q3 = unitary_matrices(static_cast<size_t>(T), 11ULL);
    std::vector<blockcg::basis_matrix> Q(static_cast<size_t>(T), blockcg::basis_matrix(static_cast<size_t>(N) * N));
    std::vector<cd> det(static_cast<size_t>(T));
    for (int t = 0; t < T; ++t) {
      const cd* u = &q3[static_cast<size_t>(t) * 9];  // column-major, as Q
      for (int j = 0; j < N; ++j) Q[t][static_cast<size_t>(j) * N + j] = 1.0;
      for (int j = 0; j < 3; ++j)
        for (int i = 0; i < 3; ++i) Q[t][static_cast<size_t>(j) * N + i] = u[3 * j + i];
      det[t] = u[0] * (u[4] * u[8] - u[7] * u[5]) - u[3] * (u[1] * u[8] - u[7] * u[2]) + u[6] * (u[1] * u[5] - u[4] * u[2]);
    }
    blockcg::basis_slice_rotate(Vm, 3, std::vector<int>(), Q);
    const std::vector<blockcg::basis_matrix> R = blockcg::basis_slice_triple(V, V, V, 3);
    for (int t = 0; t < T; ++t) covariance = std::fmax(covariance, std::abs(R[t][at(0, 1, 2)] - det[t] * E[t][at(0, 1, 2)]));
    ok = covariance <= 1e-12;
  }
  std::printf("# covariance: |T'(0,1,2) - det Q T(0,1,2)| = %.3e (bound 1e-12)\n", covariance);
  std::printf("%s\n", ok ? "BARYON_ELEMENTAL_OK" : "BARYON_ELEMENTAL_FAILED");
  return ok ? 0 : 1;
}
