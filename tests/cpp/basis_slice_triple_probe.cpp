// GPU probe of blockcg/basis.hpp's basis_slice_triple on a [4,2,4,2] lattice: A = 16 + 5 columns, B = 8, C = 3 along direction
// 2 with two momenta and two listed slices, and one basis of 16 + 5 columns three times, against plain host sums in long
// double taken through operator[] (the lazily synchronised host mirror): entry p * S + s of the result is the Ka x Kb x Kc
// tensor of slice slices[s] and momentum p, element (i, j, k) at (k * Kb + j) * Ka + i.  Exit code 0 and a final
// BASIS_SLICE_TRIPLE_PROBE_OK = every check within its bound (1e-13 of sum_x |A_i(x)| |B_j(x)| |C_k(x)|, the bound of
// tests/test_basis_slice_triple.py).
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
  std::printf("%-62s %.3e (bound %.1e) %s\n", what, figure, bound, ok ? "ok" : "FAILED");
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

long double norm3(const std::vector<cd>& col, size_t x) {
  return std::sqrt(std::norm(cl(col[3 * x])) + std::norm(cl(col[3 * x + 1])) + std::norm(cl(col[3 * x + 2])));
}

// largest |T_p(s)(i, j, k) - host sum| / sum_x |A_i(x)| |B_j(x)| |C_k(x)| over all entries
double triple_error(const std::vector<blockcg::basis_matrix>& T, const std::vector<std::vector<cd>>& A, const std::vector<std::vector<cd>>& B,
                    const std::vector<std::vector<cd>>& C, int dir, const std::vector<int>& slices,
                    const std::vector<std::vector<int>>& momenta) {
  const size_t Ka = A.size(), Kb = B.size(), Kc = C.size(), S = slices.size(), sites = A[0].size() / 3;
  if (T.size() != momenta.size() * S) return 1.0;
  const long double two_pi = 2.0L * std::acos(-1.0L);
  double worst = 0.0;
  for (size_t p = 0; p < momenta.size(); ++p)
    for (size_t s = 0; s < S; ++s) {
      const blockcg::basis_matrix& M = T[p * S + s];
      if (M.size() != Ka * Kb * Kc) return 1.0;
      // the sites of the slice and their phases
      std::vector<size_t> xs;
      std::vector<cl> ws;
      for (size_t x = 0; x < sites; ++x) {
        int xc[4], r = static_cast<int>(x);
        for (int mu = 0; mu < 4; ++mu) {
          xc[mu] = r % dims[mu];
          r /= dims[mu];
        }
        if (xc[dir] != slices[s]) continue;
        long double frac = 0.0L;
        for (int mu = 0; mu < 4; ++mu) {
          const int n = ((momenta[p][mu] % dims[mu]) + dims[mu]) % dims[mu];
          frac += static_cast<long double>((n * xc[mu]) % dims[mu]) / dims[mu];
        }
        xs.push_back(x);
        ws.push_back(cl(std::cos(two_pi * frac), -std::sin(two_pi * frac)));
      }
      for (size_t k = 0; k < Kc; ++k)
        for (size_t j = 0; j < Kb; ++j)
          for (size_t i = 0; i < Ka; ++i) {
            cl sum = 0.0L;
            long double scale = 0.0L;
            for (size_t q = 0; q < xs.size(); ++q) {
              const size_t x = xs[q];
              cl a[3], b[3], c[3];
              for (int col = 0; col < 3; ++col) {
                a[col] = cl(A[i][3 * x + col]);
                b[col] = cl(B[j][3 * x + col]);
                c[col] = cl(C[k][3 * x + col]);
              }
              const cl det = a[0] * (b[1] * c[2] - b[2] * c[1]) + a[1] * (b[2] * c[0] - b[0] * c[2]) + a[2] * (b[0] * c[1] - b[1] * c[0]);
              sum += ws[q] * det;
              scale += norm3(A[i], x) * norm3(B[j], x) * norm3(C[k], x);
            }
            worst = std::fmax(worst, static_cast<double>(std::abs(cl(M[(k * Kb + j) * Ka + i]) - sum) / scale));
          }
    }
  return worst;
}
}  // namespace

int main() {
  const double tol = 1e-13;
  blockcg::lattice lat(std::vector<int>{4, 2, 4, 2});
  block_fermion_field<16> a0(lat);
  block_fermion_field<5> a1(lat);
  block_fermion_field<8> b0(lat);
  block_fermion_field<3> c0(lat);
  a0.setGaussian(211);
  a1.setGaussian(212);
  b0.setGaussian(213);
  c0.setGaussian(214);
  blockcg::basis A, B, C;
  A.push_back(a0);
  A.push_back(a1);
  B.push_back(b0);
  C.push_back(c0);
  std::vector<std::vector<cd>> Ah, Bh, Ch;
  append_columns(Ah, a0);
  append_columns(Ah, a1);
  append_columns(Bh, b0);
  append_columns(Ch, c0);

  const int dir = 2;
  const std::vector<std::vector<int>> momenta{{1, -1, 0, 3}, {0, 0, 0, 0}};
  const std::vector<int> slices{3, 1};
  std::vector<blockcg::basis_matrix> T = blockcg::basis_slice_triple(A, B, C, dir, slices, momenta);
  double e = triple_error(T, Ah, Bh, Ch, dir, slices, momenta);
  expect(e <= tol, "basis_slice_triple, 16 + 5 x 8 x 3, two slices, two momenta", e, tol);

  // without slices and momenta: L tensors, those of the zero momentum
  const std::vector<blockcg::basis_matrix> plain = blockcg::basis_slice_triple(A, B, C, dir);
  e = triple_error(plain, Ah, Bh, Ch, dir, {0, 1, 2, 3}, {{0, 0, 0, 0}});
  expect(plain.size() == 4 && e <= tol, "basis_slice_triple without slices and momenta", e, tol);
  expect(plain[1] == T[slices.size() + 1] && plain[3] == T[slices.size()], "the listed slices are those of the full call, bit for bit", 0.0, 0.0);

  // one basis three times: within the bound, and antisymmetric with exact zeros
  const std::vector<blockcg::basis_matrix> same = blockcg::basis_slice_triple(A, A, A, dir);
  e = triple_error(same, Ah, Ah, Ah, dir, {0, 1, 2, 3}, {{0, 0, 0, 0}});
  expect(e <= tol, "one basis of 21 columns three times", e, tol);
  const size_t K = static_cast<size_t>(A.K());
  double defect = 0.0;
  for (const blockcg::basis_matrix& M : same)
    for (size_t k = 0; k < K; ++k)
      for (size_t j = 0; j < K; ++j)
        for (size_t i = 0; i < K; ++i) {
          const cd v = M[(k * K + j) * K + i];
          defect = std::fmax(defect, std::abs(v + M[(k * K + i) * K + j]));
          defect = std::fmax(defect, std::abs(v + M[(j * K + k) * K + i]));
          defect = std::fmax(defect, std::abs(v + M[(i * K + j) * K + k]));
        }
  expect(defect == 0.0, "antisymmetry defect of the identical lists", defect, 0.0);

  // the mirror, host to device: a write through operator[] reaches the call
  c0[5](2, 1) = cd(3.0, -4.0);
  Ch.clear();
  append_columns(Ch, c0);
  T = blockcg::basis_slice_triple(A, B, C, dir, slices, momenta);
  e = triple_error(T, Ah, Bh, Ch, dir, slices, momenta);
  expect(e <= tol, "basis_slice_triple after a host write of C[5]", e, tol);

  bool thrown = false;
  try {
    blockcg::basis_slice_triple(A, B, C, 4);
  } catch (const std::runtime_error&) {
    thrown = true;
  }
  expect(thrown, "basis_slice_triple refuses a direction outside the lattice", thrown ? 0.0 : 1.0, 0.0);

  if (failures) {
    std::printf("%d check(s) FAILED\n", failures);
    return 1;
  }
  std::puts("BASIS_SLICE_TRIPLE_PROBE_OK");
  return 0;
}
