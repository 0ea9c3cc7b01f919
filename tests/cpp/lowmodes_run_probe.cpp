// GPU probe of blockcg/lowmodes.hpp on a [4,4,4,2] lattice (random links of seed 7, mass 0.05): basis_rotate against host
// sums in long double through the host mirror (V = 16 + 5 columns), spectral_bound against the Rayleigh quotients of the
// computed vectors, lowest_modes on 32 + 16 columns (orthonormality and residuals recomputed with dirac_op::op and
// hermitian_dot), and the locked overload.  Exit code 0 and a final LOWMODES_PROBE_OK = every check within its bound.
#include <cmath>
#include <complex>
#include <cstdio>
#include <vector>

#include "blockcg/lowmodes.hpp"

namespace {
typedef std::complex<double> cd;
typedef std::complex<long double> cl;
typedef std::vector<std::vector<cd>> columns_t;  // [column][3 x + c]

int failures = 0;

void expect(bool ok, const char* what, double figure, double bound) {
  std::printf("%-62s %.3e (bound %.1e) %s\n", what, figure, bound, ok ? "ok" : "FAILED");
  if (!ok) ++failures;
}

template <int W>
columns_t columns(const block_fermion_field<W>& f) {
  columns_t out(W, std::vector<cd>(3 * f.V));
  for (int x = 0; x < f.V; ++x)
    for (int j = 0; j < W; ++j)
      for (int c = 0; c < 3; ++c) out[j][3 * x + c] = f[x](c, j);
  return out;
}

// max_i || A v_i - theta_i v_i || with A through dirac_op::op, and || V^dagger V - 1 ||_F of one field
template <int W>
void check_field(const dirac_op& D, block_fermion_field<W>& v, const double* theta, const double* resid, double* worst_resid_gap,
                 double* orth) {
  block_fermion_field<W> T(v);
  D.op(T, v);
  block_matrix<W> M;
  M.setZero();
  for (int j = 0; j < W; ++j) M(j, j) = -theta[j];
  T.add(v, M);
  const block_matrix<W> N = T.hermitian_dot(T), G = v.hermitian_dot(v);
  double o = 0.0;
  for (int j = 0; j < W; ++j) {
    const double r = std::sqrt(std::fmax(0.0, N(j, j).real()));
    *worst_resid_gap = std::fmax(*worst_resid_gap, std::fabs(r - resid[j]) - 0.1 * r);
    for (int i = 0; i < W; ++i) o += std::norm(G(i, j) - (i == j ? cd(1.0) : cd(0.0)));
  }
  *orth = std::fmax(*orth, std::sqrt(o));
}
}  // namespace

int main() {
  blockcg::lattice lat(std::vector<int>{4, 4, 4, 2});
  dirac_op D(lat, 0.05, 7ULL);

  // ---- basis_rotate: V = 16 + 5 columns (the generic form), Q full and not unitary
  {
    block_fermion_field<16> a(lat);
    block_fermion_field<5> b(lat);
    a.setGaussian(11);
    b.setGaussian(12);
    columns_t Vh = columns(a);
    const columns_t bh = columns(b);
    Vh.insert(Vh.end(), bh.begin(), bh.end());
    const size_t K = 21;
    blockcg::basis_matrix Q(K * K);
    for (size_t j = 0; j < K; ++j)
      for (size_t i = 0; i < K; ++i) Q[j * K + i] = cd(std::cos(0.3 * (i + 1) * (j + 2)), std::sin(0.7 * (i + 2) * (j + 1)));
    blockcg::mutable_basis V;
    V.push_back(a);
    V.push_back(b);
    blockcg::basis_rotate(V, Q);
    columns_t got = columns(a);
    const columns_t gb = columns(b);
    got.insert(got.end(), gb.begin(), gb.end());
    long double d = 0.0L, n = 0.0L;
    for (size_t j = 0; j < K; ++j)
      for (size_t r = 0; r < Vh[0].size(); ++r) {
        cl s = 0.0L;
        for (size_t i = 0; i < K; ++i) s += cl(Vh[i][r]) * cl(Q[j * K + i]);
        d += std::norm(cl(got[j][r]) - s);
        n += std::norm(s);
      }
    const double e = d == d ? static_cast<double>(std::sqrt(d / n)) : 1.0;
    expect(e <= 1e-13, "basis_rotate, V = 16 + 5 columns, host mirror both ways", e, 1e-13);
    bool thrown = false;
    try {
      blockcg::basis_rotate(V, blockcg::basis_matrix(K * K - 1));
    } catch (const std::invalid_argument&) {
      thrown = true;
    }
    expect(thrown, "basis_rotate refuses a Q that is not K x K", thrown ? 0.0 : 1.0, 0.0);
  }

  // ---- spectral_bound and lowest_modes, 32 + 16 columns, 32 wanted
  const double ub = blockcg::spectral_bound(D, 10, 5ULL);
  std::printf("SPECTRAL_BOUND %.17g\n", ub);
  block_fermion_field<32> v0(lat);
  block_fermion_field<16> v1(lat);
  v0.setGaussian(21);
  v1.setGaussian(22);
  blockcg::mutable_basis V;
  V.push_back(v0);
  V.push_back(v1);
  const double tol = 1e-10;
  const blockcg::lowest_modes_result r = blockcg::lowest_modes(V, D, 32, ub, 16, tol, 60);
  std::printf("LOWEST_MODES iterations %d applications %lld\n", r.iterations, static_cast<long long>(r.applications));
  double worst = 0.0, gap = -1.0, orth = 0.0;
  for (int i = 0; i < 32; ++i) worst = std::fmax(worst, r.resid[i]);
  expect(worst <= tol * ub, "lowest_modes: residuals of the 32 wanted columns", worst, tol * ub);
  expect(r.applications == 2LL * (2 * (r.iterations + 1) + 16 * r.iterations), "applications = nv (2 (it + 1) + degree it)",
         static_cast<double>(r.applications), 0.0);
  check_field(D, v0, r.evals.data(), r.resid.data(), &gap, &orth);
  check_field(D, v1, r.evals.data() + 32, r.resid.data() + 32, &gap, &orth);
  expect(gap <= 1e-13 * ub, "reported residuals against dirac_op::op (beyond 10 %)", gap, 1e-13 * ub);
  expect(orth <= 1e-12, "|V^dagger V - 1| per field", orth, 1e-12);
  bool ascending = r.evals[0] > 0.0 && r.evals[47] < ub;
  for (int i = 1; i < 48; ++i) ascending = ascending && r.evals[i] >= r.evals[i - 1];
  expect(ascending, "Ritz values ascending inside (0, bound)", ascending ? 0.0 : 1.0, 0.0);

  // ---- the locked overload: 16 + 16 more columns against the 32 + 16 above, 8 wanted
  block_fermion_field<16> w0(lat), w1(lat);
  w0.setGaussian(23);
  w1.setGaussian(24);
  blockcg::mutable_basis W;
  W.push_back(w0);
  W.push_back(w1);
  blockcg::basis L;
  L.push_back(v0);
  const blockcg::lowest_modes_result r2 = blockcg::lowest_modes(W, L, D, 8, ub, 16, tol, 60);
  worst = 0.0;
  for (int i = 0; i < 8; ++i) worst = std::fmax(worst, r2.resid[i]);
  expect(worst <= tol * ub, "locked stage: residuals of the 8 wanted columns", worst, tol * ub);
  double cross = 0.0;
  for (const cd& z : blockcg::basis_dot(L, w0)) cross += std::norm(z);
  for (const cd& z : blockcg::basis_dot(L, w1)) cross += std::norm(z);
  expect(std::sqrt(cross) <= 1e-12, "locked stage: |L^dagger W|", std::sqrt(cross), 1e-12);
  // min-max: a Ritz value of a block orthogonal to the 32 lowest eigenvectors is no smaller than the 32nd eigenvalue
  const double below = r.evals[31] - r2.evals[0];
  expect(below <= 10.0 * tol * ub, "locked stage: lowest Ritz value not below the locked ones", below, 10.0 * tol * ub);

  std::printf("%s\n", failures == 0 ? "LOWMODES_PROBE_OK" : "LOWMODES_PROBE_MISMATCH");
  return failures == 0 ? 0 : 1;
}
