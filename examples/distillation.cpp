// examples/distillation.cpp -- the distillation chain with the basis never leaving the device (blockcg/basis.hpp):
//   1. a basis V of 16 columns, orthonormal on every time slice: Gaussian noise q, its per-slice Gram matrices G(t) = R(t)^dagger R(t)
//      (Cholesky on the host, 16 x 16 per slice) and V = q R(t)^-1 slice by slice -- one basis_slice_axpy over all slices.  (A
//      distillation basis from blockcg/lowmodes.hpp goes in the same way.)
//   2. the sources B_j = V_j on the slice x_3 = t0, zero elsewhere: distillation_source, basis_slice_axpy with one slice and beta = 0
//   3. one SBCGrQ solve
//   4. the perambulator tau(t) = V(t)^dagger X: basis_slice_dot
//   5. the smeared sink V(t) tau(t) = V(t) V(t)^dagger X on every slice: basis_slice_axpy with tau as the coefficients.
// Self-check: sum_j |B_j|^2 = 16 (V is orthonormal on t0) and B is exactly zero off t0; the true residual of the solve; the
// projector of step 5 applied twice gives what it gives once.  Prints t and the trace of tau(t); exit code 0 and
// DISTILLATION_OK = all of it holds.
//   distillation [L0 L1 L2 L3 [mass [t0]]]      default 8 8 8 16, mass 0.5, t0 = 1
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "blockcg/basis.hpp"

namespace {
typedef std::complex<double> cd;
const int N = 16;

// G = R^dagger R (R upper triangular): R^-1, column-major; false where G is not positive definite
bool inverse_factor(const block_matrix<N>& G, blockcg::basis_matrix& Rinv) {
  std::vector<cd> L(N * N, cd(0.0, 0.0)), Li(N * N, cd(0.0, 0.0));  // G = L L^dagger, L = R^dagger; element (i, j) at j * N + i
  for (int j = 0; j < N; ++j)
    for (int i = j; i < N; ++i) {
      cd s = G(i, j);
      for (int k = 0; k < j; ++k) s -= L[k * N + i] * std::conj(L[k * N + j]);
      if (i == j) {
        if (!(s.real() > 0.0)) return false;
        L[j * N + j] = std::sqrt(s.real());
      } else {
        L[j * N + i] = s / L[j * N + j].real();
      }
    }
  for (int j = 0; j < N; ++j) {
    Li[j * N + j] = 1.0 / L[j * N + j].real();
    for (int i = j + 1; i < N; ++i) {
      cd s = 0.0;
      for (int k = j; k < i; ++k) s += L[k * N + i] * Li[j * N + k];
      Li[j * N + i] = -s / L[i * N + i].real();
    }
  }
  Rinv.assign(N * N, cd(0.0, 0.0));
  for (int j = 0; j < N; ++j)
    for (int i = 0; i <= j; ++i) Rinv[j * N + i] = std::conj(Li[i * N + j]);  // R^-1 = (L^-1)^dagger
  return true;
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
  const double mass = argc >= 6 ? std::atof(argv[5]) : 0.5, eps = 1e-10;
  const int T = dims[3], t0 = argc >= 7 ? std::atoi(argv[6]) % T : 1 % T;
  blockcg::lattice lat(dims);
  dirac_op D(lat, mass, /*seed=*/7ull);
  const std::vector<int> all_slices, no_momentum;

  // 1. V = q R(t)^-1 on every slice
  block_fermion_field<N> q(lat), v(lat);
  q.setGaussian(41);
  const block_fermion_field<N>& cq = q;
  const std::vector<block_matrix<N>> G = cq.slice_gram(cq, 3);
  std::vector<blockcg::basis_matrix> Rinv(T);
  bool ok = G.size() == static_cast<size_t>(T);
  for (int t = 0; ok && t < T; ++t) ok = inverse_factor(G[t], Rinv[t]);
  if (!ok) {
    std::printf("DISTILLATION_FAILED (a slice has fewer rows than the basis has columns)\n");
    return 1;
  }
  blockcg::basis Q, V;
  Q.push_back(q);
  blockcg::basis_slice_axpy(v, Q, 3, all_slices, Rinv, no_momentum, 0.0);
  V.push_back(v);

  // 2. the sources: all 16 columns of V on t0
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
  ok = off_slice == 0.0 && std::fabs(norm - N) <= 1e-12 * N;
  std::printf("# sources: sum_j |B_j|^2 = %.15g (K_src = %d), largest entry off the source slice %.3e\n", norm, N, off_slice);

  // 3. the solve and its true residual
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

  // 4. the perambulator
  const std::vector<blockcg::basis_matrix> tau = blockcg::basis_slice_dot(V, X[0], 3);
  ok = ok && tau.size() == static_cast<size_t>(T);
  std::printf("# t  tr tau(t) re im\n");
  for (int t = 0; ok && t < T; ++t) {
    cd tr = 0.0;
    for (int i = 0; i < N; ++i) tr += tau[t][i * N + i];
    std::printf("%3d  %.14e %.14e\n", t, tr.real(), tr.imag());
  }

  // 5. the smeared sink, and the projector once more on top of it
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
  std::printf("%s\n", ok ? "DISTILLATION_OK" : "DISTILLATION_FAILED");
  return ok ? 0 : 1;
}
