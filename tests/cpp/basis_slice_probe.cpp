// GPU probe of blockcg/basis.hpp's basis_slice_dot on a [4,2,4,2] lattice: V = 32 + 16 + 5 columns against m = 8, along
// direction 2 with two momenta, against plain host sums in long double taken through operator[] (the lazily synchronised host
// mirror): entry p * L + t of the result is the K x m matrix of slice t and momentum p, element (i, j) at j * K + i.  Also the
// sum over t against basis_dot, the call without momenta against the zero momentum, and the mirror around the call.
// Exit code 0 and a final BASIS_SLICE_PROBE_OK = every check within its bound (1e-13, the bound of tests/test_basis_slice.py).
#include <cmath>
#include <complex>
#include <cstdio>
#include <vector>

#include "blockcg/basis.hpp"

namespace {
typedef std::complex<double> cd;
typedef std::complex<long double> cl;

int failures = 0;
const int dims[4] = {4, 2, 4, 2};

void expect(bool ok, const char* what, double figure, double bound) {
  std::printf("%-58s %.3e (bound %.1e) %s\n", what, figure, bound, ok ? "ok" : "FAILED");
  if (!ok) ++failures;
}

// [column][site][colour] through the const operator[]
template <int W>
void append_columns(std::vector<std::vector<cd>>& all, const block_fermion_field<W>& f) {
  for (int j = 0; j < W; ++j) {
    std::vector<cd> col(3 * f.V);
    for (int x = 0; x < f.V; ++x)
      for (int c = 0; c < 3; ++c) col[3 * x + c] = f[x](c, j);
    all.push_back(col);
  }
}

// largest |tau_p(t)(i, j) - host sum| / (|V_i|_slice |b_j|_slice) over all entries
double slice_error(const std::vector<blockcg::basis_matrix>& tau, const std::vector<std::vector<cd>>& V,
                   const std::vector<std::vector<cd>>& b, int dir, const std::vector<std::vector<int>>& momenta) {
  const size_t K = V.size(), m = b.size(), L = dims[dir], sites = b[0].size() / 3;
  if (tau.size() != momenta.size() * L) return 1.0;
  const long double two_pi = 2.0L * std::acos(-1.0L);
  double worst = 0.0;
  for (size_t p = 0; p < momenta.size(); ++p)
    for (size_t t = 0; t < L; ++t) {
      const blockcg::basis_matrix& M = tau[p * L + t];
      if (M.size() != K * m) return 1.0;
      for (size_t j = 0; j < m; ++j)
        for (size_t i = 0; i < K; ++i) {
          cl s = 0.0L;
          long double nv = 0.0L, nb = 0.0L;
          for (size_t x = 0; x < sites; ++x) {
            int xc[4], r = static_cast<int>(x);
            for (int mu = 0; mu < 4; ++mu) {
              xc[mu] = r % dims[mu];
              r /= dims[mu];
            }
            if (xc[dir] != static_cast<int>(t)) continue;
            long double frac = 0.0L;
            for (int mu = 0; mu < 4; ++mu) {
              const int n = ((momenta[p][mu] % dims[mu]) + dims[mu]) % dims[mu];
              frac += static_cast<long double>((n * xc[mu]) % dims[mu]) / dims[mu];
            }
            const cl w(std::cos(two_pi * frac), -std::sin(two_pi * frac));
            for (int c = 0; c < 3; ++c) {
              s += w * std::conj(cl(V[i][3 * x + c])) * cl(b[j][3 * x + c]);
              nv += std::norm(cl(V[i][3 * x + c]));
              nb += std::norm(cl(b[j][3 * x + c]));
            }
          }
          const long double e = std::abs(cl(M[j * K + i]) - s) / std::sqrt(nv * nb);
          worst = std::fmax(worst, static_cast<double>(e));
        }
    }
  return worst;
}
}  // namespace

int main() {
  const double tol = 1e-13;
  blockcg::lattice lat(std::vector<int>{4, 2, 4, 2});
  block_fermion_field<32> v0(lat);
  block_fermion_field<16> v1(lat);
  block_fermion_field<5> v2(lat);
  block_fermion_field<8> B(lat);
  v0.setGaussian(201);
  v1.setGaussian(202);
  v2.setGaussian(203);
  B.setGaussian(204);
  const block_fermion_field<8>& cB = B;
  blockcg::basis V;
  V.push_back(v0);
  V.push_back(v1);
  V.push_back(v2);
  const size_t K = static_cast<size_t>(V.K());
  std::vector<std::vector<cd>> Vh, Bh;
  append_columns(Vh, v0);
  append_columns(Vh, v1);
  append_columns(Vh, v2);
  append_columns(Bh, B);

  const int dir = 2;
  const std::vector<std::vector<int>> momenta{{1, -1, 0, 3}, {0, 0, 0, 0}};
  std::vector<blockcg::basis_matrix> tau = blockcg::basis_slice_dot(V, B, dir, momenta);
  double e = slice_error(tau, Vh, Bh, dir, momenta);
  expect(e <= tol, "basis_slice_dot, V = 32 + 16 + 5, m = 8, two momenta", e, tol);

  // without momenta: L matrices, those of the zero momentum
  const std::vector<blockcg::basis_matrix> plain = blockcg::basis_slice_dot(V, B, dir);
  e = slice_error(plain, Vh, Bh, dir, {{0, 0, 0, 0}});
  expect(plain.size() == 4 && e <= tol, "basis_slice_dot without momenta", e, tol);

  // its sum over t is basis_dot
  const blockcg::basis_matrix C = blockcg::basis_dot(V, B);
  double worst = 0.0;
  for (size_t j = 0; j < 8; ++j)
    for (size_t i = 0; i < K; ++i) {
      cl s = 0.0L;
      long double nv = 0.0L, nb = 0.0L;
      for (const blockcg::basis_matrix& M : plain) s += cl(M[j * K + i]);
      for (const cd& z : Vh[i]) nv += std::norm(cl(z));
      for (const cd& z : Bh[j]) nb += std::norm(cl(z));
      worst = std::fmax(worst, static_cast<double>(std::abs(s - cl(C[j * K + i])) / std::sqrt(nv * nb)));
    }
  expect(worst <= tol, "sum over t against basis_dot", worst, tol);

  // the mirror, host to device: a write through operator[] reaches the call; the const read afterwards still sees it
  B[5](2, 3) = cd(3.0, -4.0);
  Bh.clear();
  append_columns(Bh, B);
  tau = blockcg::basis_slice_dot(V, B, dir, momenta);
  e = slice_error(tau, Vh, Bh, dir, momenta);
  expect(e <= tol && cB[5](2, 3) == cd(3.0, -4.0), "basis_slice_dot after a host write of B[5]", e, tol);

  bool thrown = false;
  try {
    blockcg::basis_slice_dot(V, B, 4);
  } catch (const std::runtime_error&) {
    thrown = true;
  }
  expect(thrown, "basis_slice_dot refuses a direction outside the lattice", thrown ? 0.0 : 1.0, 0.0);

  std::printf("%s\n", failures == 0 ? "BASIS_SLICE_PROBE_OK" : "BASIS_SLICE_PROBE_MISMATCH");
  return failures == 0 ? 0 : 1;
}
