// Host-side eigen-decomposition of a small Hermitian matrix (the reduced problem of bcg_lowest_modes, K <= 64, and the
// tridiagonal matrix of bcg_spectral_bound): cyclic complex Jacobi on a CMat of small_matrix.hpp.  A = Z diag(theta) Z^dagger
// with theta ascending and Z unitary.  Jacobi is chosen for its accuracy on the small eigenvalues of a graded matrix and
// for having no special cases; at K = 64 a decomposition is about ten sweeps of K^2 / 2 rotations of 6 K complex
// multiplications each, a few milliseconds per outer iteration of the eigensolver.
#pragma once
#include <algorithm>
#include <numeric>

#include "small_matrix.hpp"

namespace bcg {

// Only the Hermitian part of A is used (the strict upper triangle and the real parts of the diagonal).  Returns false when A
// holds a non-finite entry or the sweeps do not converge (60 of them; ten is typical): theta and Z are then not to be used.
inline bool hermitian_eig(const CMat& A, std::vector<double>& theta, CMat& Z) {
  const int n = A.dim();
  theta.assign(static_cast<size_t>(n), 0.0);
  Z = CMat::identity(n);
  if (!A.all_finite()) return false;
  CMat W(n);
  for (int j = 0; j < n; ++j) {
    W(j, j) = A(j, j).real();
    for (int i = 0; i < j; ++i) {
      W(i, j) = A(i, j);
      W(j, i) = std::conj(A(i, j));
    }
  }
  double total = 0.0;
  for (int j = 0; j < n; ++j)
    for (int i = 0; i < n; ++i) total += std::norm(W(i, j));
  bool converged = n < 2 || total == 0.0;
  for (int sweep = 0; sweep < 60 && !converged; ++sweep) {
    double off = 0.0;
    for (int j = 1; j < n; ++j)
      for (int i = 0; i < j; ++i) off += 2.0 * std::norm(W(i, j));
    if (off <= 1e-34 * total) {
      converged = true;
      break;
    }
    for (int p = 0; p < n - 1; ++p)
      for (int q = p + 1; q < n; ++q) {
        const cd apq = W(p, q);
        const double g = std::abs(apq);
        if (g == 0.0) continue;
        const double app = W(p, p).real(), aqq = W(q, q).real();
        if (g <= 1e-300 || g * g <= 1e-40 * std::abs(app * aqq)) {  // below every rounding of the diagonal
          W(p, q) = W(q, p) = 0.0;
          continue;
        }
        // D = diag(1, conj(phase)) makes the pivot real, then the real rotation [[c, s], [-s, c]]: J = D R
        const cd phase = apq / g;
        const double tau = (aqq - app) / (2.0 * g);
        const double t = (tau >= 0.0 ? 1.0 : -1.0) / (std::abs(tau) + std::sqrt(1.0 + tau * tau));
        const double cs = 1.0 / std::sqrt(1.0 + t * t), sn = t * cs;
        const cd jpp = cs, jpq = sn, jqp = -sn * std::conj(phase), jqq = cs * std::conj(phase);
        for (int k = 0; k < n; ++k) {  // W <- W J
          const cd wp = W(k, p), wq = W(k, q);
          W(k, p) = wp * jpp + wq * jqp;
          W(k, q) = wp * jpq + wq * jqq;
        }
        for (int k = 0; k < n; ++k) {  // W <- J^dagger W
          const cd wp = W(p, k), wq = W(q, k);
          W(p, k) = std::conj(jpp) * wp + std::conj(jqp) * wq;
          W(q, k) = std::conj(jpq) * wp + std::conj(jqq) * wq;
        }
        for (int k = 0; k < n; ++k) {  // Z <- Z J
          const cd zp = Z(k, p), zq = Z(k, q);
          Z(k, p) = zp * jpp + zq * jqp;
          Z(k, q) = zp * jpq + zq * jqq;
        }
        W(p, q) = W(q, p) = 0.0;
        W(p, p) = W(p, p).real();
        W(q, q) = W(q, q).real();
      }
  }
  if (!converged || !W.all_finite() || !Z.all_finite()) return false;
  std::vector<int> order(static_cast<size_t>(n));
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return W(a, a).real() < W(b, b).real(); });
  CMat Zs(n);
  for (int j = 0; j < n; ++j) {
    theta[static_cast<size_t>(j)] = W(order[static_cast<size_t>(j)], order[static_cast<size_t>(j)]).real();
    for (int i = 0; i < n; ++i) Zs(i, j) = Z(i, order[static_cast<size_t>(j)]);
  }
  Z = Zs;
  return true;
}

}  // namespace bcg
