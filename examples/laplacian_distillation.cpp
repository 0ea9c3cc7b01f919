// examples/laplacian_distillation.cpp -- the distillation chain of examples/distillation.cpp with a real basis: the lowest
// modes of the three-dimensional covariant Laplacian on every time slice, computed on the device (blockcg/lowmodes.hpp).
//   1. unitary links (Gram-Schmidt of pseudo-random 3 x 3 matrices on the host), one dirac_op over them
//   2. the basis V: 16 columns of noise, laplacian_modes along direction 3 -- all 16 wanted, so the call carries its guard
//      block; 12 = 4 (ndim - 1) bounds the spectrum of -Lap_3 for unitary links
//   3. the sources B_j = V_j on the slice x_3 = t0, zero elsewhere: distillation_source
//   4. one SBCGrQ solve
//   5. the perambulator tau(t) = V(t)^dagger X: basis_slice_dot
//   6. the smeared sink V(t) V(t)^dagger X on every slice: basis_slice_axpy with tau as the coefficients.
// Self-check: the residuals of step 2 within tol * 12 on every slice, V(t)^dagger V(t) = 1 on every slice, Ritz values
// ascending inside (0, 12); sum_j |B_j|^2 = 16 and B exactly zero off t0; the true residual of the solve; the projector of
// step 6 applied twice gives what it gives once.  Prints the lowest and the highest Ritz value of every slice and the trace of
// tau(t); exit code 0 and LAPLACIAN_DISTILLATION_OK = all of it holds.
//   laplacian_distillation [L0 L1 L2 L3 [mass [t0]]]      default 8 8 8 16, mass 0.5, t0 = 1
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "blockcg/lowmodes.hpp"

namespace {
typedef std::complex<double> cd;
const int N = 16;

// [site][mu][3 x 3 column-major]: the columns of a pseudo-random matrix orthonormalised one after another
std::vector<cd> unitary_links(size_t matrices, unsigned long long seed) {
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

double trace_re(const block_matrix<N>& M) {
  double s = 0.0;
  for (int j = 0; j < N; ++j) s += M(j, j).real();
  return s;
}
}  // namespace

int main(int argc, char** argv) {
  std::vector<int> dims = {8, 8, 8, 16};
  if (argc >= 5)
    for (int mu = 0; mu < 4; ++mu) dims[mu] = std::atoi(argv[1 + mu]);
  const double mass = argc >= 6 ? std::atof(argv[5]) : 0.5, eps = 1e-10, tol = 1e-10, ub = 12.0;
  const int T = dims[3], t0 = argc >= 7 ? std::atoi(argv[6]) % T : 1 % T;
  blockcg::lattice lat(dims);
  const std::vector<cd> links = unitary_links(static_cast<size_t>(lat.V()) * 4, 7ULL);
  dirac_op D(lat, mass, links.data());
  const std::vector<int> all_slices, no_momentum;

  // 2. the basis
  block_fermion_field<N> v(lat);
  v.setGaussian(41);
  blockcg::mutable_basis Vm;
  Vm.push_back(v);
  const blockcg::laplacian_modes_result modes = blockcg::laplacian_modes(Vm, D, 3, N, ub, 16, tol, 60);
  const blockcg::basis& V = Vm.as_basis();
  bool ok = modes.evals.size() == static_cast<size_t>(T);
  double worst = 0.0, orth = 0.0;
  const block_fermion_field<N>& cv = v;
  const std::vector<block_matrix<N>> G = cv.slice_gram(cv, 3);
  std::printf("# %d outer iterations, %lld applications of the Laplacian\n# t  theta_1(t) theta_%d(t)\n", modes.iterations,
              static_cast<long long>(modes.applications), N);
  for (int t = 0; ok && t < T; ++t) {
    std::printf("%3d  %.14e %.14e\n", t, modes.evals[t][0], modes.evals[t][N - 1]);
    ok = modes.evals[t][0] > 0.0 && modes.evals[t][N - 1] < ub;
    for (int i = 0; i < N; ++i) {
      worst = std::fmax(worst, modes.resid[t][i]);
      if (i > 0) ok = ok && modes.evals[t][i] >= modes.evals[t][i - 1];
      for (int j = 0; j < N; ++j) orth = std::fmax(orth, std::abs(G[t](i, j) - (i == j ? cd(1.0) : cd(0.0))));
    }
  }
  ok = ok && worst <= tol * ub && orth <= 1e-12;
  std::printf("# basis: worst residual %.3e (bound %.1e), largest entry of V(t)^dagger V(t) - 1 %.3e\n", worst, tol * ub, orth);

  // 3. the sources: all 16 columns of V on t0
  block_fermion_field<N> B(lat);
  blockcg::distillation_source(B, V, 3, t0, 0);
  const block_fermion_field<N>& cB = B;
  const std::vector<block_matrix<N>> GB = cB.slice_gram(cB, 3);
  double off_slice = 0.0;
  for (int t = 0; t < T; ++t)
    if (t != t0)
      for (int j = 0; j < N; ++j)
        for (int i = 0; i < N; ++i) off_slice = std::fmax(off_slice, std::abs(GB[t](i, j)));
  const double norm = trace_re(GB[t0]);
  ok = ok && off_slice == 0.0 && std::fabs(norm - N) <= 1e-12 * N;
  std::printf("# sources: sum_j |B_j|^2 = %.15g (K_src = %d), largest entry off the source slice %.3e\n", norm, N, off_slice);

  // 4. the solve and its true residual
  std::vector<block_fermion_field<N>> X(1, block_fermion_field<N>(lat));
  std::vector<double> sigma = {0.0};
  const int iterations = SBCGrQ(X, B, D, sigma, eps, eps);
  double residual = 0.0;
  {
    block_fermion_field<N> R(lat);
    D.op(R, X[0]);
    R -= B;
    const block_matrix<N> r2 = R.hermitian_dot(R), b2 = cB.hermitian_dot(cB);
    for (int j = 0; j < N; ++j) residual = std::fmax(residual, std::sqrt(r2(j, j).real() / b2(j, j).real()));
  }
  ok = ok && iterations > 0 && residual < 2 * eps;
  std::printf("# %dx%dx%dx%d, mass %g, sources on t0 = %d: %d iterations, worst true residual %.3e\n", dims[0], dims[1], dims[2], dims[3],
              mass, t0, iterations, residual);

  // 5. the perambulator
  const std::vector<blockcg::basis_matrix> tau = blockcg::basis_slice_dot(V, X[0], 3);
  ok = ok && tau.size() == static_cast<size_t>(T);
  std::printf("# t  tr tau(t) re im\n");
  for (int t = 0; ok && t < T; ++t) {
    cd tr = 0.0;
    for (int i = 0; i < N; ++i) tr += tau[t][i * N + i];
    std::printf("%3d  %.14e %.14e\n", t, tr.real(), tr.imag());
  }

  // 6. the smeared sink, and the projector once more on top of it
  double idempotent = 0.0;
  if (ok) {
    block_fermion_field<N> S(lat), S2(lat);
    blockcg::basis_slice_axpy(S, V, 3, all_slices, tau, no_momentum, 0.0);
    blockcg::basis_slice_axpy(S2, V, 3, all_slices, blockcg::basis_slice_dot(V, S, 3), no_momentum, 0.0);
    S2 -= S;
    const double d2 = trace_re(S2.hermitian_dot(S2)), s2 = trace_re(S.hermitian_dot(S));
    idempotent = std::sqrt(d2 / s2);
    ok = s2 > 0.0 && idempotent <= 1e-12;
  }
  std::printf("# projector: |P P X - P X| / |P X| = %.3e\n", idempotent);
  std::printf("%s\n", ok ? "LAPLACIAN_DISTILLATION_OK" : "LAPLACIAN_DISTILLATION_FAILED");
  return ok ? 0 : 1;
}
