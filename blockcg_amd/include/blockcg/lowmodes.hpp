// blockcg/lowmodes.hpp -- the low modes of dirac_op::op computed on the device, and the in-place basis rotation under them
// (include/blockcg_hip.h: bcg_basis_rotate, bcg_spectral_bound, bcg_lowest_modes).
//
//   mutable_basis V;  V.push_back(f)             a list of fields the calls below write to (blockcg::basis holds const ones);
//                                                V.as_basis() is the same list for basis_dot / deflate / SBCGrQ_deflated
//   basis_rotate(V, Q)                           V <- V Q in place, Q K x K column-major (element (i, j) at j * K + i), K <= 64
//   spectral_bound(D, steps = 10, seed = 1, parity = -1)   an upper bound on the largest eigenvalue (Lanczos, safeguarded)
//   lowest_modes(V, D, n_want, upper_bound, degree = 16, tol = 1e-10, max_iterations = 100)
//   lowest_modes(V, locked, D, ...)              the same, V kept orthogonal to the converged vectors `locked`
//
// lowest_modes takes the start block in V (fill it with noise) and leaves orthonormal Ritz vectors with ascending Ritz
// values; the first n_want columns decide convergence (residual <= tol * upper_bound).  Reaching max_iterations is no
// error: the residuals in the result tell.  The wanted columns need columns beyond them (the top of a block converges
// slowly); with n_want == K the call carries a guard block of its own.  Chebyshev-filtered subspace iteration; DESIGN.md
// section 8h.
//
//   basis_slice_rotate(V, dir, slices, Q)        V(x) <- V(x) Q[s] in place on the listed slices of dir, one matrix per slice
//   laplacian_modes(V, links, dir, n_want, upper_bound, degree = 16, tol = 1e-10, max_iterations = 100)
//   laplacian_modes(V, locked, links, dir, ...)  the lowest modes of -Lap_dir on every slice of dir at once: a distillation
//                                                basis (bcg_basis_slice_rotate, bcg_laplacian_modes)
// The reference has none of these; they are extensions in the blockcg namespace, host compiler only like the other headers.
#ifndef BLOCKCG_LOWMODES_HPP
#define BLOCKCG_LOWMODES_HPP
#include <cstdint>
#include <functional>
#include <stdexcept>
#include <vector>

#include "basis.hpp"

namespace blockcg {

// A list of fields of one lattice, parity and site count that a call may overwrite.  Referred to, not copied.
class mutable_basis {
 public:
  template <int W>
  void push_back(block_fermion_field<W>& f) {
    static_assert(W >= 1 && W <= 32, "a basis field has 1 .. 32 columns");
    block_fermion_field<W>* p = &f;
    h_.push_back(f.handle());
    flush_.push_back([p] { p->flush(); });
    written_.push_back([p] { p->device_written(); });
    const_.push_back(f);
    K_ += W;
    lat_ = &f.lat();
  }
  int K() const { return K_; }
  int size() const { return static_cast<int>(h_.size()); }
  bcg_field* const* handles() const { return h_.data(); }
  const basis& as_basis() const { return const_; }
  lattice& lat() const {
    if (!lat_) throw std::invalid_argument("mutable_basis: empty");
    return *lat_;
  }
  void flush() const {
    for (const auto& f : flush_) f();
  }
  void device_written() const {
    for (const auto& f : written_) f();
  }

 private:
  std::vector<bcg_field*> h_;
  std::vector<std::function<void()>> flush_, written_;
  basis const_;
  int K_ = 0;
  lattice* lat_ = nullptr;
};

inline void basis_rotate(mutable_basis& V, const basis_matrix& Q) {
  if (Q.size() != static_cast<size_t>(V.K()) * V.K()) throw std::invalid_argument("basis_rotate: Q is K x K");
  V.flush();
  check(bcg_basis_rotate(V.handles(), V.size(), reinterpret_cast<const double*>(Q.data())), V.lat().ctx(), "basis_rotate");
  V.device_written();
}

inline double spectral_bound(const dirac_op& D, int steps = 10, unsigned long long seed = 1, int parity = -1) {
  double bound = 0.0;
  check(bcg_spectral_bound(D.lat().ctx(), D.handle(), D.mass, parity, steps, seed, &bound), D.lat().ctx(), "spectral_bound");
  return bound;
}

struct lowest_modes_result {
  std::vector<double> evals, resid;  // K each: Ritz values (ascending) and ||A v - theta v||
  int iterations = 0;                // filter applications
  std::int64_t applications = 0;     // calls of the block operator, one per field (the guard block included) and application
};

inline lowest_modes_result lowest_modes(mutable_basis& V, const basis* locked, const dirac_op& D, int n_want, double upper_bound,
                                        int degree, double tol, int max_iterations) {
  lowest_modes_result r;
  r.evals.assign(static_cast<size_t>(V.K()), 0.0);
  r.resid.assign(static_cast<size_t>(V.K()), 0.0);
  V.flush();
  if (locked) locked->flush();
  const int rc = bcg_lowest_modes(D.lat().ctx(), D.handle(), D.mass, V.handles(), V.size(), locked ? locked->handles() : nullptr,
                                  locked ? locked->size() : 0, n_want, degree, upper_bound, tol, max_iterations, r.evals.data(),
                                  r.resid.data(), &r.iterations, &r.applications);
  V.device_written();
  check(rc, D.lat().ctx(), "lowest_modes");
  return r;
}

inline lowest_modes_result lowest_modes(mutable_basis& V, const dirac_op& D, int n_want, double upper_bound, int degree = 16,
                                        double tol = 1e-10, int max_iterations = 100) {
  return lowest_modes(V, nullptr, D, n_want, upper_bound, degree, tol, max_iterations);
}

inline lowest_modes_result lowest_modes(mutable_basis& V, const basis& locked, const dirac_op& D, int n_want, double upper_bound,
                                        int degree = 16, double tol = 1e-10, int max_iterations = 100) {
  return lowest_modes(V, &locked, D, n_want, upper_bound, degree, tol, max_iterations);
}

// V(x) <- V(x) Q[s] in place on the sites with GLOBAL x_dir = slices[s] (bcg_basis_slice_rotate): basis_rotate with one
// K x K column-major matrix per listed slice.  slices empty: all L_dir slices in ascending order.  The other slices are
// neither read nor written.
inline void basis_slice_rotate(mutable_basis& V, int dir, const std::vector<int>& slices, const std::vector<basis_matrix>& Q) {
  if (dir < 0 || dir >= static_cast<int>(V.lat().dims().size())) throw std::runtime_error("basis_slice_rotate: direction outside the lattice");
  const size_t S = slices.empty() ? static_cast<size_t>(V.lat().dims()[dir]) : slices.size(), KK = static_cast<size_t>(V.K()) * V.K();
  if (Q.size() != S) throw std::invalid_argument("basis_slice_rotate: one matrix per listed slice");
  std::vector<std::complex<double>> buf(S * KK);
  for (size_t s = 0; s < S; ++s) {
    if (Q[s].size() != KK) throw std::invalid_argument("basis_slice_rotate: Q[s] is K x K");
    std::copy(Q[s].begin(), Q[s].end(), buf.begin() + s * KK);
  }
  V.flush();
  check(bcg_basis_slice_rotate(V.handles(), V.size(), dir, static_cast<int>(slices.size()), slices.empty() ? nullptr : slices.data(),
                               reinterpret_cast<const double*>(buf.data())),
        V.lat().ctx(), "basis_slice_rotate");
  V.device_written();
}

struct laplacian_modes_result {
  std::vector<std::vector<double>> evals, resid;  // [L_dir][K]: per slice, Ritz values (ascending) and ||A v - theta v|| on it
  int iterations = 0;                             // filter applications
  std::int64_t applications = 0;                  // shift_sum calls, one per field (the guard block included) and application
};

// The lowest eigenpairs of -Lap_dir on every slice of dir at once (bcg_laplacian_modes): a distillation basis.  links: a
// dirac_op or a gauge_field; V, locked (orthonormal per slice), n_want, degree, tol and max_iterations as in lowest_modes;
// upper_bound: 4 (ndim - 1) for unitary links.
template <class Links>
laplacian_modes_result laplacian_modes(mutable_basis& V, const basis* locked, const Links& links, int dir, int n_want, double upper_bound,
                                       int degree, double tol, int max_iterations) {
  if (dir < 0 || dir >= static_cast<int>(links.lat().dims().size())) throw std::runtime_error("laplacian_modes: direction outside the lattice");
  const size_t L = static_cast<size_t>(links.lat().dims()[dir]), K = static_cast<size_t>(V.K());
  std::vector<double> evals(L * K, 0.0), resid(L * K, 0.0);
  laplacian_modes_result r;
  V.flush();
  if (locked) locked->flush();
  const int rc = bcg_laplacian_modes(links.lat().ctx(), links.handle(), dir, V.handles(), V.size(), locked ? locked->handles() : nullptr,
                                     locked ? locked->size() : 0, n_want, degree, upper_bound, tol, max_iterations, evals.data(),
                                     resid.data(), &r.iterations, &r.applications);
  V.device_written();
  check(rc, links.lat().ctx(), "laplacian_modes");
  for (size_t t = 0; t < L; ++t) {
    r.evals.push_back(std::vector<double>(evals.begin() + t * K, evals.begin() + (t + 1) * K));
    r.resid.push_back(std::vector<double>(resid.begin() + t * K, resid.begin() + (t + 1) * K));
  }
  return r;
}

template <class Links>
laplacian_modes_result laplacian_modes(mutable_basis& V, const Links& links, int dir, int n_want, double upper_bound, int degree = 16,
                                       double tol = 1e-10, int max_iterations = 100) {
  return laplacian_modes(V, static_cast<const basis*>(nullptr), links, dir, n_want, upper_bound, degree, tol, max_iterations);
}

template <class Links>
laplacian_modes_result laplacian_modes(mutable_basis& V, const basis& locked, const Links& links, int dir, int n_want, double upper_bound,
                                       int degree = 16, double tol = 1e-10, int max_iterations = 100) {
  return laplacian_modes(V, &locked, links, dir, n_want, upper_bound, degree, tol, max_iterations);
}

}  // namespace blockcg

#endif
