// GPU probe of the per-slice calls of blockcg/lowmodes.hpp on a [4,4,4,2] lattice with diagonal unitary links:
// basis_slice_rotate against host sums in long double through the host mirror (V = 16 + 5 columns, one listed slice, the
// other slice bit for bit), laplacian_modes on 32 + 16 columns along direction 3 (orthonormality per slice by slice_gram,
// residuals recomputed with blockcg::laplacian, basis_slice_axpy and slice_gram), and the locked overload.  Exit code 0 and a
// final LAPLACIAN_MODES_PROBE_OK = every check within its bound.
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstring>
#include <vector>

#include "blockcg/lowmodes.hpp"
#include "blockcg/shift.hpp"

namespace {
typedef std::complex<double> cd;
typedef std::complex<long double> cl;
typedef std::vector<std::vector<cd>> columns_t;  // [column][3 x + c]

int failures = 0;

void expect(bool ok, const char* what, double figure, double bound) {
  std::printf("%-66s %.3e (bound %.1e) %s\n", what, figure, bound, ok ? "ok" : "FAILED");
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

// per slice: || A v_i - theta_i(t) v_i || against the reported residual (beyond 10 %), and || V(t)^dagger V(t) - 1 ||_F
template <int W>
void check_field(const dirac_op& D, block_fermion_field<W>& v, const blockcg::laplacian_modes_result& r, int off, double* worst_resid_gap,
                 double* orth) {
  const int T = static_cast<int>(r.evals.size());
  block_fermion_field<W> Av(v);
  blockcg::laplacian(Av, v, D, 3);  // Lap_3 v = -A v
  blockcg::basis one;
  one.push_back(v);
  std::vector<blockcg::basis_matrix> theta(T, blockcg::basis_matrix(static_cast<size_t>(W) * W));
  for (int t = 0; t < T; ++t)
    for (int j = 0; j < W; ++j) theta[t][static_cast<size_t>(j) * W + j] = r.evals[t][off + j];
  blockcg::basis_slice_axpy(Av, one, 3, std::vector<int>(), theta);  // -(A v - theta v)
  const block_fermion_field<W>&cA = Av, &cv = v;
  const std::vector<block_matrix<W>> N = cA.slice_gram(cA, 3), G = cv.slice_gram(cv, 3);
  for (int t = 0; t < T; ++t) {
    double o = 0.0;
    for (int j = 0; j < W; ++j) {
      const double res = std::sqrt(std::fmax(0.0, N[t](j, j).real()));
      *worst_resid_gap = std::fmax(*worst_resid_gap, std::fabs(res - r.resid[t][off + j]) - 0.1 * res);
      for (int i = 0; i < W; ++i) o += std::norm(G[t](i, j) - (i == j ? cd(1.0) : cd(0.0)));
    }
    *orth = std::fmax(*orth, std::sqrt(o));
  }
}
}  // namespace

int main() {
  const std::vector<int> dims = {4, 4, 4, 2};
  blockcg::lattice lat(dims);
  // U_mu(x) = diag(exp(i a), exp(i b), exp(-i (a + b))): unitary, so 12 bounds the spectrum of -Lap_3
  std::vector<cd> links(static_cast<size_t>(lat.V()) * 4 * 9, cd(0.0, 0.0));
  for (size_t k = 0; k < links.size() / 9; ++k) {
    const double a = 1.7 * std::sin(0.9 * k + 0.3), b = 2.3 * std::cos(1.3 * k);
    links[9 * k + 0] = std::polar(1.0, a);
    links[9 * k + 4] = std::polar(1.0, b);
    links[9 * k + 8] = std::polar(1.0, -a - b);
  }
  dirac_op D(lat, 0.05, links.data());
  const double ub = 12.0, tol = 1e-10;

  // ---- basis_slice_rotate: V = 16 + 5 columns (the generic form), the slice x_3 = 1 only, Q full and not unitary
  {
    block_fermion_field<16> a(lat);
    block_fermion_field<5> b(lat);
    a.setGaussian(11);
    b.setGaussian(12);
    columns_t Vh = columns(a);
    const columns_t bh = columns(b);
    Vh.insert(Vh.end(), bh.begin(), bh.end());
    const size_t K = 21;
    std::vector<blockcg::basis_matrix> Q(1, blockcg::basis_matrix(K * K));
    for (size_t j = 0; j < K; ++j)
      for (size_t i = 0; i < K; ++i) Q[0][j * K + i] = cd(std::cos(0.3 * (i + 1) * (j + 2)), std::sin(0.7 * (i + 2) * (j + 1)));
    blockcg::mutable_basis V;
    V.push_back(a);
    V.push_back(b);
    blockcg::basis_slice_rotate(V, 3, std::vector<int>(1, 1), Q);
    columns_t got = columns(a);
    const columns_t gb = columns(b);
    got.insert(got.end(), gb.begin(), gb.end());
    const size_t slice_rows = 3 * 4 * 4 * 4;  // x_0 fastest: the rows of x_3 = 0 come first
    long double d = 0.0L, n = 0.0L;
    bool untouched = true;
    for (size_t j = 0; j < K; ++j)
      for (size_t r = 0; r < Vh[0].size(); ++r) {
        if (r < slice_rows) {
          untouched = untouched && std::memcmp(&got[j][r], &Vh[j][r], sizeof(cd)) == 0;
          continue;
        }
        cl s = 0.0L;
        for (size_t i = 0; i < K; ++i) s += cl(Vh[i][r]) * cl(Q[0][j * K + i]);
        d += std::norm(cl(got[j][r]) - s);
        n += std::norm(s);
      }
    const double e = d == d ? static_cast<double>(std::sqrt(d / n)) : 1.0;
    expect(e <= 1e-13, "basis_slice_rotate, V = 16 + 5 columns, slice 1, host mirror both ways", e, 1e-13);
    expect(untouched, "basis_slice_rotate leaves slice 0 bit for bit", untouched ? 0.0 : 1.0, 0.0);
    bool thrown = false;
    try {
      blockcg::basis_slice_rotate(V, 3, std::vector<int>(), Q);  // two slices, one matrix
    } catch (const std::invalid_argument&) {
      thrown = true;
    }
    expect(thrown, "basis_slice_rotate refuses fewer matrices than slices", thrown ? 0.0 : 1.0, 0.0);
  }

  // ---- laplacian_modes, 32 + 16 columns, 32 wanted
  block_fermion_field<32> v0(lat);
  block_fermion_field<16> v1(lat);
  v0.setGaussian(21);
  v1.setGaussian(22);
  blockcg::mutable_basis V;
  V.push_back(v0);
  V.push_back(v1);
  const blockcg::laplacian_modes_result r = blockcg::laplacian_modes(V, D, 3, 32, ub, 16, tol, 60);
  std::printf("LAPLACIAN_MODES iterations %d applications %lld\n", r.iterations, static_cast<long long>(r.applications));
  expect(r.evals.size() == 2 && r.resid.size() == 2 && r.evals[0].size() == 48, "one row of 48 Ritz values per slice", 0.0, 0.0);
  double worst = 0.0, gap = -1.0, orth = 0.0;
  bool ascending = true;
  for (int t = 0; t < 2; ++t) {
    ascending = ascending && r.evals[t][0] > 0.0 && r.evals[t][47] < ub;
    for (int i = 0; i < 32; ++i) worst = std::fmax(worst, r.resid[t][i]);
    for (int i = 1; i < 48; ++i) ascending = ascending && r.evals[t][i] >= r.evals[t][i - 1];
  }
  expect(worst <= tol * ub, "laplacian_modes: residuals of the 32 wanted columns, every slice", worst, tol * ub);
  expect(r.applications == 2LL * (2 * (r.iterations + 1) + 16 * r.iterations), "applications = nv (2 (it + 1) + degree it)",
         static_cast<double>(r.applications), 0.0);
  check_field(D, v0, r, 0, &gap, &orth);
  check_field(D, v1, r, 32, &gap, &orth);
  expect(gap <= 1e-13 * ub, "reported residuals against blockcg::laplacian (beyond 10 %)", gap, 1e-13 * ub);
  expect(orth <= 1e-12, "|V(t)^dagger V(t) - 1| per field and slice", orth, 1e-12);
  expect(ascending, "Ritz values ascending inside (0, bound) on every slice", ascending ? 0.0 : 1.0, 0.0);

  // ---- the locked overload: 16 + 16 more columns against the 32 above, 8 wanted
  block_fermion_field<16> w0(lat), w1(lat);
  w0.setGaussian(23);
  w1.setGaussian(24);
  blockcg::mutable_basis W;
  W.push_back(w0);
  W.push_back(w1);
  blockcg::basis L;
  L.push_back(v0);
  const blockcg::laplacian_modes_result r2 = blockcg::laplacian_modes(W, L, D, 3, 8, ub, 16, tol, 60);
  worst = 0.0;
  double cross = 0.0, below = -1.0;
  for (int t = 0; t < 2; ++t) {
    for (int i = 0; i < 8; ++i) worst = std::fmax(worst, r2.resid[t][i]);
    below = std::fmax(below, r.evals[t][31] - r2.evals[t][0]);  // min-max, slice by slice
  }
  for (const blockcg::basis_matrix& M : blockcg::basis_slice_dot(L, w0, 3))
    for (const cd& z : M) cross += std::norm(z);
  for (const blockcg::basis_matrix& M : blockcg::basis_slice_dot(L, w1, 3))
    for (const cd& z : M) cross += std::norm(z);
  expect(worst <= tol * ub, "locked stage: residuals of the 8 wanted columns", worst, tol * ub);
  expect(std::sqrt(cross) <= 1e-12, "locked stage: |L(t)^dagger W(t)| over the slices", std::sqrt(cross), 1e-12);
  expect(below <= 10.0 * tol * ub, "locked stage: lowest Ritz value not below the locked ones", below, 10.0 * tol * ub);

  std::printf("%s\n", failures == 0 ? "LAPLACIAN_MODES_PROBE_OK" : "LAPLACIAN_MODES_PROBE_MISMATCH");
  return failures == 0 ? 0 : 1;
}
