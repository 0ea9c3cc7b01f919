// include/blockcg_hip.h: the low-mode eigensolver -- bcg_spectral_bound (a k-step Lanczos bound on the largest eigenvalue
// of dirac_op::op) and bcg_lowest_modes (Chebyshev-filtered subspace iteration, Zhou & Saad).  Host composition only: the
// block operator (apply_shifted), bcg_basis_dot / bcg_basis_axpy for projected matrices and the projection against locked
// vectors, bcg_basis_rotate for the orthonormalisation and the Ritz rotation, the K x K work on the host (small_matrix.hpp,
// hermitian_eig.hpp).  Every branch is taken on all-reduced data (the results of bcg_basis_dot and of gram are identical on
// every rank), so the ranks of a divided lattice make the same calls in the same order.  DESIGN.md section 8h.
// And bcg_laplacian_modes, the same iteration on every slice of a direction at once for A = -Lap_dir (the distillation
// basis): bcg_dirac_shift_sum, the per-slice products and bcg_basis_slice_rotate.  DESIGN.md section 8k.
#include "capi_internal.hpp"
#include "hermitian_eig.hpp"
#include "kernels_rotate.hpp"

namespace bcg_impl {
namespace {

// a field of width m in the storage of a work field at least as wide
bcg_field view_of(const bcg_field* work, int m) {
  bcg_field v = *work;
  v.m = m;
  return v;
}

struct LowModes {
  bcg_context* c;
  const bcg_gauge* g;
  double mass;
  bcg_field* const* V;
  int nv, K;
  const bcg_field* const* locked;
  int nlocked, KL;
  bcg_field* work[3];
  int64_t applications = 0;
  std::vector<double> buf;  // a column block of a projected matrix, as the ABI returns it

  int apply(bcg_field* out, const bcg_field* in, double sigma0) {
    applications += 1;
    return apply_shifted(c, g, mass, sigma0, out, in);
  }

  // columns off .. off + b->m - 1 of M (K x K) = V^dagger b
  int project(const bcg_field* b, int off, CMat& M) {
    buf.resize(static_cast<size_t>(2) * K * b->m);
    BCG_TRY(bcg_basis_dot(V, nv, b, buf.data()));
    for (int j = 0; j < b->m; ++j)
      for (int i = 0; i < K; ++i) M(i, off + j) = cd(buf[2 * (static_cast<size_t>(j) * K + i)], buf[2 * (static_cast<size_t>(j) * K + i) + 1]);
    return BCG_OK;
  }

  // V_f <- V_f - L (L^dagger V_f) for every field
  int project_out_locked() {
    if (nlocked < 1) return BCG_OK;
    for (int f = 0; f < nv; ++f) {
      buf.resize(static_cast<size_t>(2) * KL * V[f]->m);
      BCG_TRY(bcg_basis_dot(locked, nlocked, V[f], buf.data()));
      for (double& x : buf) x = -x;
      BCG_TRY(bcg_basis_axpy(V[f], locked, nlocked, buf.data(), 1.0));
    }
    return BCG_OK;
  }

  int rotate(const CMat& Q) {
    std::vector<double> q(static_cast<size_t>(2) * K * K);
    Q.store(q.data());
    return bcg_basis_rotate(V, nv, q.data());
  }

  // The orthonormalise-and-Ritz step: the projection and the Cholesky rotation twice (CholQR2), the second rotation
  // carrying the eigenvectors of the reduced problem as well.  theta: the K Ritz values, ascending.
  int ortho_ritz(std::vector<double>& theta) {
    for (int pass = 0; pass < 2; ++pass) {
      BCG_TRY(project_out_locked());
      CMat G(K), H(K);
      int off = 0;
      for (int f = 0; f < nv; ++f) {
        BCG_TRY(project(V[f], off, G));
        if (pass == 1) {
          bcg_field T = view_of(work[0], V[f]->m);
          BCG_TRY(apply(&T, V[f], 0.0));
          BCG_TRY(project(&T, off, H));
        }
        off += V[f]->m;
      }
      G += G.adjoint();
      G *= 0.5;
      CMat R;
      if (!G.all_finite() || !cholesky_upper(G, R))
        BCG_FAIL(c, BCG_ERR_NUMERIC, "bcg_lowest_modes: V^dagger V is not positive definite (the block lost rank)");
      const CMat Rinv = upper_triangular_inverse(R);
      if (pass == 0) {
        BCG_TRY(rotate(Rinv));
        continue;
      }
      H += H.adjoint();
      H *= 0.5;
      const CMat Hr = Rinv.adjoint() * H * Rinv;
      CMat Z;
      if (!hermitian_eig(Hr, theta, Z)) BCG_FAIL(c, BCG_ERR_NUMERIC, "bcg_lowest_modes: the reduced eigenproblem did not converge");
      BCG_TRY(rotate(Rinv * Z));
    }
    return BCG_OK;
  }

  // resid_i = || A v_i - theta_i v_i ||, from the vector itself (not from ||A v||^2 - theta^2, which cancels)
  int residuals(const std::vector<double>& theta, double* resid) {
    int off = 0;
    for (int f = 0; f < nv; ++f) {
      const int m = V[f]->m;
      bcg_field W = view_of(work[0], m);
      BCG_TRY(apply(&W, V[f], 0.0));
      CMat D(m);
      for (int j = 0; j < m; ++j) D(j, j) = -theta[static_cast<size_t>(off + j)];
      BCG_TRY(rmul(c, &W, V[f], D, 0.0, bcg::RMUL_ADD, "block_axpy"));
      CMat N;
      BCG_TRY(gram(c, &W, &W, N));
      for (int j = 0; j < m; ++j) resid[off + j] = std::sqrt(std::max(0.0, N(j, j).real()));
      off += m;
    }
    return BCG_OK;
  }

  // V_f <- p(A) V_f, p the scaled Chebyshev polynomial of the given degree that is small on [lo, ub] and 1 at theta_1.
  // Three work fields: the operator's output becomes the next iterate in place (one axpby), the oldest is freed.
  int filter(int degree, double theta_1, double lo, double ub) {
    const double cen = 0.5 * (ub + lo), e = 0.5 * (ub - lo), sigma1 = e / (theta_1 - cen);
    for (int f = 0; f < nv; ++f) {
      const int m = V[f]->m;
      bcg_field w0 = view_of(work[0], m), w1 = view_of(work[1], m), w2 = view_of(work[2], m);
      bcg_field *T = &w0, *cur = &w1, *spare = &w2;
      const bcg_field* prev = V[f];
      BCG_TRY(apply(cur, V[f], -cen));
      BCG_TRY(axpby(c, cur, sigma1 / e, cur, 0.0, "axpby"));
      double sigma = sigma1;
      for (int k = 2; k <= degree; ++k) {
        const double sigma_n = 1.0 / (2.0 / sigma1 - sigma);
        BCG_TRY(apply(T, cur, -cen));
        BCG_TRY(axpby(c, T, 2.0 * sigma_n / e, prev, -sigma * sigma_n, "axpby"));
        bcg_field* freed = prev == V[f] ? spare : const_cast<bcg_field*>(prev);
        prev = cur;
        cur = T;
        T = freed;
        sigma = sigma_n;
      }
      BCG_TRY(bcg_field_copy(V[f], cur));
    }
    return BCG_OK;
  }
};

constexpr int kGuardColumns = 16;                    // the guard block of a call with n_want == K (bcg_lowest_modes)
constexpr uint64_t kGuardSeed = 0x6775617264ULL;     // its noise: a function of the global site, the same on every rank

// one context, parity and site count, no field twice; returns the columns, or -1
int64_t list_columns(const bcg_field* const* F, int n, const bcg_field* like) {
  int64_t K = 0;
  for (int k = 0; k < n; ++k) {
    if (!F[k] || F[k]->ctx != like->ctx || F[k]->parity != like->parity || F[k]->sites != like->sites) return -1;
    for (int l = 0; l < k; ++l)
      if (F[l] == F[k]) return -1;
    K += F[k]->m;
  }
  return K;
}

// bcg_laplacian_modes: LowModes slice by slice.  A = -Lap_dir is block-diagonal over the L slices of dir, so every K x K
// matrix of LowModes becomes L of them (bcg_basis_slice_dot), every rotation one bcg_basis_slice_rotate over all slices, and
// the residual norms come by slice (bcg_field_slice_dot).  The filter is ONE polynomial for all slices: its coefficients
// are global, and a step is one bcg_dirac_shift_sum with the factor and the centre folded into its coefficients.
struct LaplacianModes {
  bcg_context* c;
  const bcg_gauge* g;
  int dir, L;  // L: the GLOBAL extent of dir
  bcg_field* const* V;
  int nv, K;
  const bcg_field* const* locked;
  int nlocked, KL;
  bcg_field* work[3];
  int64_t applications = 0;
  std::vector<double> buf;  // per-slice column blocks, as the ABI returns and takes them

  // out <- a (A + shift) in:  c0 = a (2 (ndim-1) + shift), every hop off dir -a
  int apply(bcg_field* out, const bcg_field* in, double a, double shift) {
    applications += 1;
    const double c0[2] = {a * (2.0 * (c->ndim - 1) + shift), 0.0};
    double hop[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int mu = 0; mu < c->ndim; ++mu)
      if (mu != dir) hop[2 * mu] = -a;
    return bcg_dirac_shift_sum(c, g, out, in, c0, hop, hop, 0);
  }

  // columns off .. off + b->m - 1 of M[t] (K x K) = V(t)^dagger b(t), every slice t
  int project(const bcg_field* b, int off, std::vector<CMat>& M) {
    const int m = b->m;
    buf.resize(static_cast<size_t>(2) * L * K * m);
    BCG_TRY(bcg_basis_slice_dot(V, nv, b, dir, 0, nullptr, buf.data()));
    for (int t = 0; t < L; ++t)
      for (int j = 0; j < m; ++j)
        for (int i = 0; i < K; ++i) {
          const size_t e = (static_cast<size_t>(t) * m + j) * K + i;
          M[static_cast<size_t>(t)](i, off + j) = cd(buf[2 * e], buf[2 * e + 1]);
        }
    return BCG_OK;
  }

  // V_f(t) <- V_f(t) - L(t) (L(t)^dagger V_f(t)) for every field and slice
  int project_out_locked() {
    if (nlocked < 1) return BCG_OK;
    for (int f = 0; f < nv; ++f) {
      buf.resize(static_cast<size_t>(2) * L * KL * V[f]->m);
      BCG_TRY(bcg_basis_slice_dot(locked, nlocked, V[f], dir, 0, nullptr, buf.data()));
      for (double& x : buf) x = -x;
      BCG_TRY(bcg_basis_slice_axpy(V[f], locked, nlocked, dir, 0, nullptr, buf.data(), nullptr, 1.0));
    }
    return BCG_OK;
  }

  int rotate(const std::vector<CMat>& Q) {
    const size_t per = static_cast<size_t>(2) * K * K;
    std::vector<double> q(per * L);
    for (int t = 0; t < L; ++t) Q[static_cast<size_t>(t)].store(q.data() + per * t);
    return bcg_basis_slice_rotate(V, nv, dir, 0, nullptr, q.data());
  }

  // LowModes::ortho_ritz with a Cholesky factor and a reduced eigenproblem per slice.  theta[t * K + i]: ascending in i.
  int ortho_ritz(std::vector<double>& theta) {
    theta.assign(static_cast<size_t>(L) * K, 0.0);
    for (int pass = 0; pass < 2; ++pass) {
      BCG_TRY(project_out_locked());
      std::vector<CMat> G(static_cast<size_t>(L), CMat(K)), H(pass == 1 ? static_cast<size_t>(L) : 0, CMat(K)), Q(static_cast<size_t>(L));
      int off = 0;
      for (int f = 0; f < nv; ++f) {
        BCG_TRY(project(V[f], off, G));
        if (pass == 1) {
          bcg_field T = view_of(work[0], V[f]->m);
          BCG_TRY(apply(&T, V[f], 1.0, 0.0));
          BCG_TRY(project(&T, off, H));
        }
        off += V[f]->m;
      }
      for (int t = 0; t < L; ++t) {
        CMat& Gt = G[static_cast<size_t>(t)];
        Gt += Gt.adjoint();
        Gt *= 0.5;
        CMat R;
        if (!Gt.all_finite() || !cholesky_upper(Gt, R))
          BCG_FAIL(c, BCG_ERR_NUMERIC, "bcg_laplacian_modes: V(t)^dagger V(t) is not positive definite on a slice (the block lost rank)");
        const CMat Rinv = upper_triangular_inverse(R);
        if (pass == 0) {
          Q[static_cast<size_t>(t)] = Rinv;
          continue;
        }
        CMat& Ht = H[static_cast<size_t>(t)];
        Ht += Ht.adjoint();
        Ht *= 0.5;
        const CMat Hr = Rinv.adjoint() * Ht * Rinv;
        std::vector<double> th;
        CMat Z;
        if (!hermitian_eig(Hr, th, Z)) BCG_FAIL(c, BCG_ERR_NUMERIC, "bcg_laplacian_modes: a reduced eigenproblem did not converge");
        std::copy(th.begin(), th.end(), theta.begin() + static_cast<size_t>(t) * K);
        Q[static_cast<size_t>(t)] = Rinv * Z;
      }
      BCG_TRY(rotate(Q));
    }
    return BCG_OK;
  }

  // resid[t * K + i] = || A v_i - theta_i(t) v_i || over the sites of slice t, from the vector itself
  int residuals(const std::vector<double>& theta, double* resid) {
    int off = 0;
    std::vector<double> d, n2;
    for (int f = 0; f < nv; ++f) {
      const int m = V[f]->m;
      bcg_field W = view_of(work[0], m);
      BCG_TRY(apply(&W, V[f], 1.0, 0.0));
      d.assign(static_cast<size_t>(2) * L * m * m, 0.0);  // one m x m diagonal matrix per slice: -theta(t)
      for (int t = 0; t < L; ++t)
        for (int j = 0; j < m; ++j) d[2 * ((static_cast<size_t>(t) * m + j) * m + j)] = -theta[static_cast<size_t>(t) * K + off + j];
      const bcg_field* one[1] = {V[f]};
      BCG_TRY(bcg_basis_slice_axpy(&W, one, 1, dir, 0, nullptr, d.data(), nullptr, 1.0));
      n2.resize(static_cast<size_t>(2) * L * m);
      BCG_TRY(bcg_field_slice_dot(&W, &W, dir, n2.data()));
      for (int t = 0; t < L; ++t)
        for (int j = 0; j < m; ++j)
          resid[static_cast<size_t>(t) * K + off + j] = std::sqrt(std::max(0.0, n2[2 * (static_cast<size_t>(t) * m + j)]));
      off += m;
    }
    return BCG_OK;
  }

  // LowModes::filter: the operator's output arrives scaled and centred, so a step is one apply and one axpby
  int filter(int degree, double theta_1, double lo, double ub) {
    const double cen = 0.5 * (ub + lo), e = 0.5 * (ub - lo), sigma1 = e / (theta_1 - cen);
    for (int f = 0; f < nv; ++f) {
      const int m = V[f]->m;
      bcg_field w0 = view_of(work[0], m), w1 = view_of(work[1], m), w2 = view_of(work[2], m);
      bcg_field *T = &w0, *cur = &w1, *spare = &w2;
      const bcg_field* prev = V[f];
      BCG_TRY(apply(cur, V[f], sigma1 / e, -cen));
      double sigma = sigma1;
      for (int k = 2; k <= degree; ++k) {
        const double sigma_n = 1.0 / (2.0 / sigma1 - sigma);
        BCG_TRY(apply(T, cur, 2.0 * sigma_n / e, -cen));
        BCG_TRY(axpby(c, T, 1.0, prev, -sigma * sigma_n, "axpby"));
        bcg_field* freed = prev == V[f] ? spare : const_cast<bcg_field*>(prev);
        prev = cur;
        cur = T;
        T = freed;
        sigma = sigma_n;
      }
      BCG_TRY(bcg_field_copy(V[f], cur));
    }
    return BCG_OK;
  }
};

}  // namespace
}  // namespace bcg_impl

using namespace bcg_impl;

extern "C" {

int bcg_spectral_bound(bcg_context* c, const bcg_gauge* g, double mass, int parity, int steps, uint64_t seed, double* bound_out) {
  DeviceScope on_device(c);
  if (!c || !g || g->ctx != c || !bound_out) return BCG_ERR_INVALID;
  if (steps < 2 || steps > 64 || parity < -1 || parity > 1 || !std::isfinite(mass))
    BCG_FAIL(c, BCG_ERR_INVALID, "bcg_spectral_bound: steps outside 2 .. 64, parity outside -1 .. 1 or a non-finite mass");
  bcg_field* f[3] = {nullptr, nullptr, nullptr};
  int rc = BCG_OK;
  for (int k = 0; k < 3 && rc == BCG_OK; ++k)
    rc = parity >= 0 ? bcg_field_create_half(c, 1, parity, &f[k]) : bcg_field_create(c, 1, &f[k]);
  if (rc == BCG_OK) rc = reserve_operator_scratch(c, f[0]);
  if (rc == BCG_OK || rc == BCG_ERR_HIP) rc = agree_on_allocation(c, rc, "bcg_spectral_bound", "its three work fields");
  auto run = [&]() -> int {
    bcg_field *v = f[0], *vp = f[1], *w = f[2];
    BCG_TRY(bcg_field_fill_noise(v, BCG_NOISE_GAUSSIAN, seed));
    CMat N;
    BCG_TRY(gram(c, v, v, N));
    const double n0 = std::sqrt(N(0, 0).real());
    if (!(n0 > 0.0) || !std::isfinite(n0)) BCG_FAIL(c, BCG_ERR_NUMERIC, "bcg_spectral_bound: the start vector has no norm");
    BCG_TRY(axpby(c, v, 1.0 / n0, v, 0.0, "axpby"));
    std::vector<double> alpha, beta;
    for (int j = 0; j < steps; ++j) {
      BCG_TRY(apply_shifted(c, g, mass, 0.0, w, v));
      if (j > 0) BCG_TRY(axpby(c, w, 1.0, vp, -beta.back(), "axpby"));
      BCG_TRY(gram(c, v, w, N, false));
      alpha.push_back(N(0, 0).real());
      BCG_TRY(axpby(c, w, 1.0, v, -alpha.back(), "axpby"));
      BCG_TRY(gram(c, w, w, N));
      beta.push_back(std::sqrt(std::max(0.0, N(0, 0).real())));
      if (!std::isfinite(alpha.back()) || !std::isfinite(beta.back())) BCG_FAIL(c, BCG_ERR_NUMERIC, "bcg_spectral_bound: a non-finite Lanczos coefficient");
      if (beta.back() <= 1e-14 * std::abs(alpha.front())) break;  // an invariant subspace: T's largest eigenvalue is exact
      BCG_TRY(axpby(c, w, 1.0 / beta.back(), w, 0.0, "axpby"));
      bcg_field* t = vp;
      vp = v;
      v = w;
      w = t;
    }
    const int k = static_cast<int>(alpha.size());
    CMat T(k);
    for (int j = 0; j < k; ++j) {
      T(j, j) = alpha[static_cast<size_t>(j)];
      if (j + 1 < k) T(j, j + 1) = T(j + 1, j) = beta[static_cast<size_t>(j)];
    }
    std::vector<double> theta;
    CMat Z;
    if (!bcg::hermitian_eig(T, theta, Z)) BCG_FAIL(c, BCG_ERR_NUMERIC, "bcg_spectral_bound: the tridiagonal eigenproblem did not converge");
    *bound_out = theta.back() + beta.back();
    return BCG_OK;
  };
  if (rc == BCG_OK) rc = run();
  if (rc != BCG_OK) (void)hipStreamSynchronize(c->stream);
  for (int k = 0; k < 3; ++k)
    if (f[k]) (void)bcg_field_destroy(f[k]);
  return rc;
}

int bcg_lowest_modes(bcg_context* c, const bcg_gauge* g, double mass, bcg_field* const* V, int nv, const bcg_field* const* locked,
                     int nlocked, int n_want, int degree, double upper_bound, double tol, int max_iterations, double* evals_out,
                     double* resid_out, int* iterations_out, int64_t* applications_out) {
  DeviceScope on_device(c);
  if (!c || !g || g->ctx != c || !V || nv < 1 || !V[0] || V[0]->ctx != c || !evals_out || !resid_out) return BCG_ERR_INVALID;
  const int64_t K = list_columns(V, nv, V[0]);
  if (K < 0) BCG_FAIL(c, BCG_ERR_INVALID, "bcg_lowest_modes: V holds a NULL, a field twice, or mixed contexts, parities or site counts");
  if (nlocked < 0 || (nlocked > 0 && !locked)) BCG_FAIL(c, BCG_ERR_INVALID, "bcg_lowest_modes: nlocked < 0 or no list of locked fields");
  const int64_t KL = nlocked > 0 ? list_columns(const_cast<const bcg_field* const*>(locked), nlocked, V[0]) : 0;
  if (KL < 0) BCG_FAIL(c, BCG_ERR_INVALID, "bcg_lowest_modes: the locked fields do not match V (context, parity, site count) or repeat");
  for (int l = 0; l < nlocked; ++l)
    for (int k = 0; k < nv; ++k)
      if (locked[l] == V[k]) BCG_FAIL(c, BCG_ERR_INVALID, "bcg_lowest_modes: a locked field is also in V");
  if (K > bcg::kRotateMaxCols) BCG_FAIL(c, BCG_ERR_UNSUPPORTED, "bcg_lowest_modes: more than 64 columns (lock them and call again)");
  if (n_want < 1 || n_want > K || degree < 2 || max_iterations < 0 || !std::isfinite(mass) || !std::isfinite(tol) || !(tol > 0.0) ||
      !std::isfinite(upper_bound) || !(upper_bound > 0.0))
    BCG_FAIL(c, BCG_ERR_INVALID, "bcg_lowest_modes: n_want outside 1 .. K, degree < 2, or a tolerance or bound that is not positive and finite");
  if (c->distributed && (!c->have_comm || !c->comm.allreduce_sum))
    BCG_FAIL(c, BCG_ERR_COMM, "lattice is split over ranks but no bcg_comm was set");

  // The filter damps [theta_K', ub], K' the columns the iteration carries: the top columns of the block gain nothing per
  // iteration, so the wanted ones converge only when there are columns beyond them.  A caller who asks for all K columns
  // (n_want == K) brings none, and the call carries a guard block of its own: one more field of min(16, 64 - K) columns of
  // noise, filtered, orthonormalised and rotated with V and dropped at the end.  K == 64 leaves no room for one.
  const int guard = n_want == K ? std::min<int>(kGuardColumns, bcg::kRotateMaxCols - static_cast<int>(K)) : 0;
  std::vector<bcg_field*> fields(V, V + nv);
  int wmax = guard;
  for (int k = 0; k < nv; ++k) wmax = std::max(wmax, V[k]->m);
  bcg_field like = *V[0];  // the shape (context, parity, site count) of everything the call allocates
  bcg_field* guard_field = nullptr;
  bcg_field* work[3] = {nullptr, nullptr, nullptr};
  int rc = BCG_OK;
  like.m = wmax;
  for (int k = 0; k < 3 && rc == BCG_OK; ++k) rc = create_like(c, &like, &work[k]);
  if (guard > 0 && rc == BCG_OK) {
    like.m = guard;
    rc = create_like(c, &like, &guard_field);
    if (rc == BCG_OK) fields.push_back(guard_field);
  }
  const int nf = static_cast<int>(fields.size()), Kc = static_cast<int>(K) + (guard_field ? guard : 0);
  for (int k = 0; k < nf && rc == BCG_OK; ++k) rc = reserve_operator_scratch(c, fields[k]);
  if (rc == BCG_OK) rc = ensure_scratch(c);
  if (rc == BCG_OK || rc == BCG_ERR_HIP) rc = agree_on_allocation(c, rc, "bcg_lowest_modes", "its work fields");
  LowModes s{c, g, mass, fields.data(), nf, Kc, locked, nlocked, static_cast<int>(KL), {work[0], work[1], work[2]}};

  int iterations = 0;
  auto run = [&]() -> int {
    if (guard_field) BCG_TRY(bcg_field_fill_noise(guard_field, BCG_NOISE_GAUSSIAN, kGuardSeed));
    std::vector<double> theta, resid(static_cast<size_t>(Kc));
    for (;;) {
      BCG_TRY(s.ortho_ritz(theta));
      BCG_TRY(s.residuals(theta, resid.data()));
      std::copy(theta.begin(), theta.begin() + K, evals_out);  // ascending over all Kc columns: V holds the lowest K
      std::copy(resid.begin(), resid.begin() + K, resid_out);
      double worst = 0.0;
      bool finite = true;
      for (int i = 0; i < n_want; ++i) {
        worst = std::max(worst, resid[static_cast<size_t>(i)]);
        finite = finite && std::isfinite(resid[static_cast<size_t>(i)]);
      }
      if (!finite) BCG_FAIL(c, BCG_ERR_NUMERIC, "bcg_lowest_modes: a residual is not finite");
      if (worst <= tol * upper_bound || iterations >= max_iterations) return BCG_OK;
      const double lo = theta.back();
      if (!(lo < upper_bound)) BCG_FAIL(c, BCG_ERR_NUMERIC, "bcg_lowest_modes: a Ritz value is not below upper_bound (the bound is too small)");
      if (!(theta.front() < lo)) BCG_FAIL(c, BCG_ERR_NUMERIC, "bcg_lowest_modes: the Ritz values do not spread (a degenerate block)");
      BCG_TRY(s.filter(degree, theta.front(), lo, upper_bound));
      iterations += 1;
    }
  };
  if (rc == BCG_OK) rc = run();
  if (rc != BCG_OK) (void)hipStreamSynchronize(c->stream);
  else rc = stream_sync(c);  // the work fields are freed below
  for (int k = 0; k < 3; ++k)
    if (work[k]) (void)bcg_field_destroy(work[k]);
  if (guard_field) (void)bcg_field_destroy(guard_field);
  if (iterations_out) *iterations_out = iterations;
  if (applications_out) *applications_out = s.applications;
  return rc;
}

int bcg_laplacian_modes(bcg_context* c, const bcg_gauge* g, int dir, bcg_field* const* V, int nv, const bcg_field* const* locked,
                        int nlocked, int n_want, int degree, double upper_bound, double tol, int max_iterations, double* evals_out,
                        double* resid_out, int* iterations_out, int64_t* applications_out) {
  DeviceScope on_device(c);
  if (!c || !g || g->ctx != c || !V || nv < 1 || !V[0] || V[0]->ctx != c || !evals_out || !resid_out) return BCG_ERR_INVALID;
  const int64_t K = list_columns(V, nv, V[0]);
  if (K < 0) BCG_FAIL(c, BCG_ERR_INVALID, "bcg_laplacian_modes: V holds a NULL, a field twice, or mixed contexts, parities or site counts");
  if (nlocked < 0 || (nlocked > 0 && !locked)) BCG_FAIL(c, BCG_ERR_INVALID, "bcg_laplacian_modes: nlocked < 0 or no list of locked fields");
  const int64_t KL = nlocked > 0 ? list_columns(const_cast<const bcg_field* const*>(locked), nlocked, V[0]) : 0;
  if (KL < 0) BCG_FAIL(c, BCG_ERR_INVALID, "bcg_laplacian_modes: the locked fields do not match V (context, parity, site count) or repeat");
  for (int l = 0; l < nlocked; ++l)
    for (int k = 0; k < nv; ++k)
      if (locked[l] == V[k]) BCG_FAIL(c, BCG_ERR_INVALID, "bcg_laplacian_modes: a locked field is also in V");
  if (dir < 0 || dir >= c->ndim) BCG_FAIL(c, BCG_ERR_INVALID, "bcg_laplacian_modes: dir outside 0 .. ndim-1");
  if (K > bcg::kRotateMaxCols) BCG_FAIL(c, BCG_ERR_UNSUPPORTED, "bcg_laplacian_modes: more than 64 columns (lock them and call again)");
  if (n_want < 1 || n_want > K || degree < 2 || max_iterations < 0 || !std::isfinite(tol) || !(tol > 0.0) || !std::isfinite(upper_bound) ||
      !(upper_bound > 0.0))
    BCG_FAIL(c, BCG_ERR_INVALID, "bcg_laplacian_modes: n_want outside 1 .. K, degree < 2, or a tolerance or bound that is not positive and finite");
  if (V[0]->parity >= 0) BCG_FAIL(c, BCG_ERR_UNSUPPORTED, "bcg_laplacian_modes: one hop flips the parity, so half fields have no modes of their own");
  if (c->distributed && (!c->have_comm || !c->comm.allreduce_sum || !c->comm.halo_exchange))
    BCG_FAIL(c, BCG_ERR_COMM, "lattice is split over ranks but no bcg_comm was set");

  // the guard block of bcg_lowest_modes, with its rules
  const int guard = n_want == K ? std::min<int>(kGuardColumns, bcg::kRotateMaxCols - static_cast<int>(K)) : 0;
  std::vector<bcg_field*> fields(V, V + nv);
  int wmax = guard;
  for (int k = 0; k < nv; ++k) wmax = std::max(wmax, V[k]->m);
  bcg_field like = *V[0];
  bcg_field* guard_field = nullptr;
  bcg_field* work[3] = {nullptr, nullptr, nullptr};
  int rc = BCG_OK;
  like.m = wmax;
  for (int k = 0; k < 3 && rc == BCG_OK; ++k) rc = create_like(c, &like, &work[k]);
  if (guard > 0 && rc == BCG_OK) {
    like.m = guard;
    rc = create_like(c, &like, &guard_field);
    if (rc == BCG_OK) fields.push_back(guard_field);
  }
  const int nf = static_cast<int>(fields.size()), Kc = static_cast<int>(K) + (guard_field ? guard : 0);
  if (rc == BCG_OK) rc = ensure_scratch(c);
  if (rc == BCG_OK || rc == BCG_ERR_HIP) rc = agree_on_allocation(c, rc, "bcg_laplacian_modes", "its work fields");
  const int L = c->gdims[dir];
  LaplacianModes s{c, g, dir, L, fields.data(), nf, Kc, locked, nlocked, static_cast<int>(KL), {work[0], work[1], work[2]}};

  int iterations = 0;
  auto run = [&]() -> int {
    if (guard_field) BCG_TRY(bcg_field_fill_noise(guard_field, BCG_NOISE_GAUSSIAN, kGuardSeed));
    std::vector<double> theta, resid(static_cast<size_t>(L) * Kc);
    for (;;) {
      BCG_TRY(s.ortho_ritz(theta));
      BCG_TRY(s.residuals(theta, resid.data()));
      double worst = 0.0, lo = theta[static_cast<size_t>(Kc) - 1], theta_1 = theta[0];
      bool finite = true;
      for (int t = 0; t < L; ++t) {
        const double* th = theta.data() + static_cast<size_t>(t) * Kc;
        const double* rs = resid.data() + static_cast<size_t>(t) * Kc;
        std::copy(th, th + K, evals_out + static_cast<size_t>(t) * K);  // ascending over all Kc columns: V holds the lowest K
        std::copy(rs, rs + K, resid_out + static_cast<size_t>(t) * K);
        for (int i = 0; i < n_want; ++i) {
          worst = std::max(worst, rs[i]);
          finite = finite && std::isfinite(rs[i]);
        }
        lo = std::max(lo, th[Kc - 1]);
        theta_1 = std::min(theta_1, th[0]);
      }
      if (!finite) BCG_FAIL(c, BCG_ERR_NUMERIC, "bcg_laplacian_modes: a residual is not finite");
      if (worst <= tol * upper_bound || iterations >= max_iterations) return BCG_OK;
      if (!(lo < upper_bound)) BCG_FAIL(c, BCG_ERR_NUMERIC, "bcg_laplacian_modes: a Ritz value is not below upper_bound (the bound is too small)");
      if (!(theta_1 < lo)) BCG_FAIL(c, BCG_ERR_NUMERIC, "bcg_laplacian_modes: the Ritz values do not spread (a degenerate block)");
      BCG_TRY(s.filter(degree, theta_1, lo, upper_bound));
      iterations += 1;
    }
  };
  if (rc == BCG_OK) rc = run();
  if (rc != BCG_OK) (void)hipStreamSynchronize(c->stream);
  else rc = stream_sync(c);  // the work fields are freed below
  for (int k = 0; k < 3; ++k)
    if (work[k]) (void)bcg_field_destroy(work[k]);
  if (guard_field) (void)bcg_field_destroy(guard_field);
  if (iterations_out) *iterations_out = iterations;
  if (applications_out) *applications_out = s.applications;
  return rc;
}

}  // extern "C"
