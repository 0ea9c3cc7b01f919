// blockcg/basis.hpp -- products between a solve block and a basis of another width, and deflation on top of them
// (include/blockcg_hip.h: bcg_basis_dot, bcg_basis_axpy, bcg_basis_slice_dot, bcg_basis_slice_axpy, bcg_basis_slice_triple,
// bcg_field_copy_columns).
//
//   basis V;  V.push_back(f)                     a list of fields of any widths 1 .. 32; K = the sum of the widths
//   basis_dot(V, b)                              C = V^dagger b, K x m column-major (element (i, j) at j * K + i)
//   basis_axpy(y, V, C, beta = 1)                y <- beta y + V C; beta == 0 does not read y
//   basis_slice_dot(V, b, dir[, momenta])        V^dagger b by slice of dir (and momentum): L_dir matrices K x m per momentum
//   basis_slice_axpy(y, V, dir, slices, C, momentum, beta)   its adjoint: y <- beta y + w V C[s] on the listed slices
//   distillation_source(y, V, dir, t0, first)    y = columns first .. of V on the slice t0, zero elsewhere
//   basis_slice_triple(A, B, C, dir, slices, momenta)   baryon elementals: sum over a slice of det[A_i(x), B_j(x), C_k(x)]
//   copy_columns(dst, dst_first, src, src_first, n)   n columns between fields of different widths
//   deflate(B, V)                                B <- B - V (V^dagger B); returns C = V^dagger B
//   low_mode_solution(X, V, evals, C, sigma)     X_s += V (Lambda + sigma_s)^-1 C
//   SBCGrQ_deflated(X, B, D, sigma, V, evals, ...)    copies B, deflates the copy, runs SBCGrQ, adds the low-mode part
//
// Contract of the last three: V is orthonormal and evals are its Ritz values of dirac_op::op.  (A + sigma_s)^-1 is
// diagonal on eigenvectors of A for every shift at once, which is what makes deflating a multi-shift solve cheap.  With
// inexact eigenvectors the result is inexact by their residuals; the reference's true-residual measure is the check.
// The reference has none of these; they are extensions in the blockcg namespace, host compiler only like the other headers.
#ifndef BLOCKCG_BASIS_HPP
#define BLOCKCG_BASIS_HPP
#include <algorithm>
#include <complex>
#include <functional>
#include <stdexcept>
#include <vector>

#include "block_solvers.hpp"
#include "dirac_op.hpp"
#include "fields.hpp"

namespace blockcg {

// A list of fields of one lattice, parity and site count.  The fields are referred to, not copied: they outlive the basis.
class basis {
 public:
  template <int W>
  void push_back(const block_fermion_field<W>& f) {
    static_assert(W >= 1 && W <= 32, "a basis field has 1 .. 32 columns");
    const block_fermion_field<W>* p = &f;
    h_.push_back(f.handle());
    flush_.push_back([p] { p->flush(); });
    K_ += W;
    lat_ = &f.lat();
  }
  int K() const { return K_; }
  int size() const { return static_cast<int>(h_.size()); }
  const bcg_field* const* handles() const { return h_.data(); }
  lattice& lat() const {
    if (!lat_) throw std::invalid_argument("basis: empty");
    return *lat_;
  }
  void flush() const {
    for (const auto& f : flush_) f();
  }

 private:
  std::vector<const bcg_field*> h_;
  std::vector<std::function<void()>> flush_;
  int K_ = 0;
  lattice* lat_ = nullptr;
};

typedef std::vector<std::complex<double>> basis_matrix;  // K x m, column-major

template <int N_rhs>
basis_matrix basis_dot(const basis& V, const block_fermion_field<N_rhs>& b) {
  V.flush();
  b.flush();
  basis_matrix C(static_cast<size_t>(V.K()) * N_rhs);
  check(bcg_basis_dot(V.handles(), V.size(), b.handle(), reinterpret_cast<double*>(C.data())), V.lat().ctx(), "basis_dot");
  return C;
}

// V^dagger b resolved by slice and momentum (bcg_basis_slice_dot): entry p * L_dir + t of the result is the K x m
// column-major matrix tau_p(t)(i, j) = sum_{x_dir = t} w_p(x) V_i(x)^dagger b_j(x), t over the GLOBAL extent of dir
template <int N_rhs>
std::vector<basis_matrix> basis_slice_dot_call(const basis& V, const block_fermion_field<N_rhs>& b, int dir, int n_mom,
                                               const int* momenta) {
  if (dir < 0 || dir >= static_cast<int>(V.lat().dims().size())) throw std::runtime_error("basis_slice_dot: direction outside the lattice");
  V.flush();
  b.flush();
  const size_t L = static_cast<size_t>(V.lat().dims()[dir]), KM = static_cast<size_t>(V.K()) * N_rhs;
  const size_t P = n_mom > 0 ? static_cast<size_t>(n_mom) : 1;
  std::vector<std::complex<double>> buf(P * L * KM);
  check(bcg_basis_slice_dot(V.handles(), V.size(), b.handle(), dir, n_mom, momenta, reinterpret_cast<double*>(buf.data())),
        V.lat().ctx(), "basis_slice_dot");
  std::vector<basis_matrix> out(P * L);
  for (size_t k = 0; k < P * L; ++k) out[k].assign(buf.begin() + k * KM, buf.begin() + (k + 1) * KM);
  return out;
}

template <int N_rhs>
std::vector<basis_matrix> basis_slice_dot(const basis& V, const block_fermion_field<N_rhs>& b, int dir) {
  return basis_slice_dot_call(V, b, dir, 0, nullptr);
}

// momenta: integer momenta of up to 4 components each (missing ones are 0; the component along dir must be 0)
template <int N_rhs>
std::vector<basis_matrix> basis_slice_dot(const basis& V, const block_fermion_field<N_rhs>& b, int dir,
                                          const std::vector<std::vector<int>>& momenta) {
  if (momenta.empty()) throw std::runtime_error("basis_slice_dot: no momenta");
  std::vector<int> n(4 * momenta.size(), 0);
  for (size_t p = 0; p < momenta.size(); ++p) {
    if (momenta[p].size() > 4) throw std::runtime_error("basis_slice_dot: a momentum has up to 4 components");
    for (size_t mu = 0; mu < momenta[p].size(); ++mu) n[4 * p + mu] = momenta[p][mu];
  }
  return basis_slice_dot_call(V, b, dir, static_cast<int>(momenta.size()), n.data());
}

template <int N_rhs>
void basis_axpy(block_fermion_field<N_rhs>& y, const basis& V, const basis_matrix& C, double beta = 1.0) {
  if (C.size() != static_cast<size_t>(V.K()) * N_rhs) throw std::invalid_argument("basis_axpy: C is K x m");
  V.flush();
  y.flush();
  check(bcg_basis_axpy(y.handle(), V.handles(), V.size(), reinterpret_cast<const double*>(C.data()), beta), V.lat().ctx(),
        "basis_axpy");
  y.device_written();
}

// The adjoint of basis_slice_dot (bcg_basis_slice_axpy): y <- beta y + w V C[s] on the sites with GLOBAL x_dir = slices[s],
// y <- beta y on every other site.  slices empty: all L_dir slices in ascending order, so that one momentum block of
// basis_slice_dot's result goes straight in as C.  momentum empty: w = 1; else up to 4 integers (the component along dir 0),
// w(x) = exp(+2 pi i sum_mu n_mu x_mu / L_mu).  beta == 0 does not read y; beta == 1 leaves the other slices alone.
template <int N_rhs>
void basis_slice_axpy(block_fermion_field<N_rhs>& y, const basis& V, int dir, const std::vector<int>& slices,
                      const std::vector<basis_matrix>& C, const std::vector<int>& momentum = std::vector<int>(), double beta = 1.0) {
  if (dir < 0 || dir >= static_cast<int>(V.lat().dims().size())) throw std::runtime_error("basis_slice_axpy: direction outside the lattice");
  const size_t S = slices.empty() ? static_cast<size_t>(V.lat().dims()[dir]) : slices.size(), KM = static_cast<size_t>(V.K()) * N_rhs;
  if (C.size() != S) throw std::invalid_argument("basis_slice_axpy: one matrix per listed slice");
  if (momentum.size() > 4) throw std::invalid_argument("basis_slice_axpy: a momentum has up to 4 components");
  std::vector<std::complex<double>> buf(S * KM);
  for (size_t s = 0; s < S; ++s) {
    if (C[s].size() != KM) throw std::invalid_argument("basis_slice_axpy: C[s] is K x m");
    std::copy(C[s].begin(), C[s].end(), buf.begin() + s * KM);
  }
  int n[4] = {0, 0, 0, 0};
  for (size_t mu = 0; mu < momentum.size(); ++mu) n[mu] = momentum[mu];
  V.flush();
  y.flush();
  check(bcg_basis_slice_axpy(y.handle(), V.handles(), V.size(), dir, static_cast<int>(slices.size()), slices.empty() ? nullptr : slices.data(),
                             reinterpret_cast<const double*>(buf.data()), momentum.empty() ? nullptr : n, beta),
        V.lat().ctx(), "basis_slice_axpy");
  y.device_written();
}

// A distillation source: y_j = V_{first + j} on the slice x_dir = t0 and zero elsewhere, j < N_rhs (basis_slice_axpy with one
// slice, beta = 0 and C the column selection)
template <int N_rhs>
void distillation_source(block_fermion_field<N_rhs>& y, const basis& V, int dir, int t0, int first) {
  if (first < 0 || first + N_rhs > V.K()) throw std::invalid_argument("distillation_source: columns outside the basis");
  std::vector<basis_matrix> C(1, basis_matrix(static_cast<size_t>(V.K()) * N_rhs));
  for (int j = 0; j < N_rhs; ++j) C[0][static_cast<size_t>(j) * V.K() + first + j] = 1.0;
  basis_slice_axpy(y, V, dir, std::vector<int>(1, t0), C, std::vector<int>(), 0.0);
}

// Baryon elementals (bcg_basis_slice_triple): entry p * S + s of the result is the Ka x Kb x Kc tensor
// T_p(s)(i, j, k) = sum_{x_dir = slices[s]} w_p(x) det[A_i(x), B_j(x), C_k(x)], element (i, j, k) at (k * Kb + j) * Ka + i.
// slices empty: all L_dir slices in ascending order (S = L_dir); momenta empty: the single momentum 0, no phase arithmetic.
// The same basis three times gives a result that is antisymmetric bit for bit.
inline std::vector<basis_matrix> basis_slice_triple(const basis& A, const basis& B, const basis& C, int dir,
                                                    const std::vector<int>& slices = std::vector<int>(),
                                                    const std::vector<std::vector<int>>& momenta = std::vector<std::vector<int>>()) {
  if (dir < 0 || dir >= static_cast<int>(A.lat().dims().size())) throw std::runtime_error("basis_slice_triple: direction outside the lattice");
  std::vector<int> n(4 * momenta.size(), 0);
  for (size_t p = 0; p < momenta.size(); ++p) {
    if (momenta[p].size() > 4) throw std::runtime_error("basis_slice_triple: a momentum has up to 4 components");
    for (size_t mu = 0; mu < momenta[p].size(); ++mu) n[4 * p + mu] = momenta[p][mu];
  }
  A.flush();
  B.flush();
  C.flush();
  const size_t S = slices.empty() ? static_cast<size_t>(A.lat().dims()[dir]) : slices.size();
  const size_t P = momenta.empty() ? 1 : momenta.size(), E = static_cast<size_t>(A.K()) * B.K() * C.K();
  std::vector<std::complex<double>> buf(P * S * E);
  check(bcg_basis_slice_triple(A.handles(), A.size(), B.handles(), B.size(), C.handles(), C.size(), dir, static_cast<int>(slices.size()),
                               slices.empty() ? nullptr : slices.data(), static_cast<int>(momenta.size()), momenta.empty() ? nullptr : n.data(),
                               reinterpret_cast<double*>(buf.data())),
        A.lat().ctx(), "basis_slice_triple");
  std::vector<basis_matrix> out(P * S);
  for (size_t k = 0; k < P * S; ++k) out[k].assign(buf.begin() + k * E, buf.begin() + (k + 1) * E);
  return out;
}

template <int N_dst, int N_src>
void copy_columns(block_fermion_field<N_dst>& dst, int dst_first, const block_fermion_field<N_src>& src, int src_first, int n) {
  src.flush();
  dst.flush();
  check(bcg_field_copy_columns(dst.handle(), dst_first, src.handle(), src_first, n), src.lat().ctx(), "copy_columns");
  dst.device_written();
}

template <int N_rhs>
basis_matrix deflate(block_fermion_field<N_rhs>& B, const basis& V) {
  basis_matrix C = basis_dot(V, B), minus(C.size());
  for (size_t e = 0; e < C.size(); ++e) minus[e] = -C[e];
  basis_axpy(B, V, minus, 1.0);
  return C;
}

template <int N_rhs>
void low_mode_solution(std::vector<block_fermion_field<N_rhs>>& X, const basis& V, const std::vector<double>& evals,
                       const basis_matrix& C, const std::vector<double>& sigma) {
  const size_t K = static_cast<size_t>(V.K());
  if (evals.size() != K || C.size() != K * N_rhs || sigma.size() != X.size())
    throw std::invalid_argument("low_mode_solution: one eigenvalue per basis column, C of size K x m, one shift per X_s");
  basis_matrix W(C.size());
  for (size_t s = 0; s < X.size(); ++s) {
    for (size_t j = 0; j < static_cast<size_t>(N_rhs); ++j)
      for (size_t i = 0; i < K; ++i) W[j * K + i] = C[j * K + i] / (evals[i] + sigma[s]);
    basis_axpy(X[s], V, W, 1.0);
  }
}

// Returns the operator applications of the inner solve.
template <int N_rhs>
int SBCGrQ_deflated(std::vector<block_fermion_field<N_rhs>>& X, const block_fermion_field<N_rhs>& B, const dirac_op& D,
                    std::vector<double>& sigma, const basis& V, const std::vector<double>& evals, double eps = 1.e-15,
                    double eps_shifts = 1.e-15, int max_iterations = 1e6) {
  block_fermion_field<N_rhs> Bp(B);
  const basis_matrix C = deflate(Bp, V);
  const int iterations = SBCGrQ_consuming_source(X, Bp, D, sigma, eps, eps_shifts, max_iterations);
  low_mode_solution(X, V, evals, C, sigma);
  return iterations;
}

}  // namespace blockcg

#endif
