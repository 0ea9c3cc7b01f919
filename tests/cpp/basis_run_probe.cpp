// GPU probe of blockcg/basis.hpp on a [4,2,4,2] lattice: basis_dot, basis_axpy and copy_columns between fields of 32, 16, 5
// and 8 columns against plain host sums in long double taken through operator[] (the lazily synchronised host mirror), the
// mirror in both directions around each call, deflate, and SBCGrQ_deflated on a basis of 16 orthonormal columns -- whose
// results are printed for tests/test_basis.py to compare with the same calls through the Python bindings.
// Exit code 0 and a final BASIS_PROBE_OK = every check within its bound (1e-13, the bounds of tests/test_basis.py).
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstring>
#include <vector>

#include "blockcg/basis.hpp"

namespace {
typedef std::complex<double> cd;
typedef std::complex<long double> cl;
typedef std::vector<std::vector<cd>> columns_t;  // [column][3 x + c]

int failures = 0;

void expect(bool ok, const char* what, double figure, double bound) {
  std::printf("%-58s %.3e (bound %.1e) %s\n", what, figure, bound, ok ? "ok" : "FAILED");
  if (!ok) ++failures;
}

bool same_bits(cd a, cd b) { return std::memcmp(&a, &b, sizeof(cd)) == 0; }

// the columns of a field, read through the const operator[] (which leaves the mirror clean)
template <int W>
columns_t columns(const block_fermion_field<W>& f) {
  columns_t out(W, std::vector<cd>(3 * f.V));
  for (int x = 0; x < f.V; ++x)
    for (int j = 0; j < W; ++j)
      for (int c = 0; c < 3; ++c) out[j][3 * x + c] = f[x](c, j);
  return out;
}

void append(columns_t& all, const columns_t& more) { all.insert(all.end(), more.begin(), more.end()); }

long double norm(const std::vector<cd>& v) {
  long double s = 0.0L;
  for (const cd& z : v) s += std::norm(cl(z));
  return std::sqrt(s);
}

// largest |C(i, j) - V_i^dagger b_j| / (|V_i| |b_j|), C column-major K x m: element (i, j) at j * K + i
double dot_error(const blockcg::basis_matrix& C, const columns_t& V, const columns_t& b) {
  const size_t K = V.size(), m = b.size();
  if (C.size() != K * m) return 1.0;
  double worst = 0.0;
  for (size_t j = 0; j < m; ++j)
    for (size_t i = 0; i < K; ++i) {
      cl s = 0.0L;
      for (size_t r = 0; r < b[j].size(); ++r) s += std::conj(cl(V[i][r])) * cl(b[j][r]);
      const long double e = std::abs(cl(C[j * K + i]) - s) / (norm(V[i]) * norm(b[j]));
      worst = std::fmax(worst, static_cast<double>(e));
    }
  return worst;
}

// beta y + V C, column by column
columns_t axpy_expected(const columns_t& y, const columns_t& V, const blockcg::basis_matrix& C, double beta) {
  const size_t K = V.size(), m = y.size();
  columns_t out(m, std::vector<cd>(y[0].size()));
  for (size_t j = 0; j < m; ++j)
    for (size_t r = 0; r < y[j].size(); ++r) {
      cl s = beta == 0.0 ? cl(0.0L) : cl(static_cast<long double>(beta)) * cl(y[j][r]);
      for (size_t i = 0; i < K; ++i) s += cl(V[i][r]) * cl(C[j * K + i]);
      out[j][r] = cd(static_cast<double>(s.real()), static_cast<double>(s.imag()));
    }
  return out;
}

double frobenius_error(const columns_t& got, const columns_t& want) {
  long double d = 0.0L, n = 0.0L;
  for (size_t j = 0; j < want.size(); ++j)
    for (size_t r = 0; r < want[j].size(); ++r) {
      d += std::norm(cl(got[j][r]) - cl(want[j][r]));
      n += std::norm(cl(want[j][r]));
    }
  return d == d ? static_cast<double>(std::sqrt(d / n)) : 1.0;  // NaN in the result: an error of 1
}

template <int W>
void poison(block_fermion_field<W>& f) {
  const double nan = std::nan("");
  for (int x = 0; x < f.V; ++x)
    for (int j = 0; j < W; ++j)
      for (int c = 0; c < 3; ++c) f[x](c, j) = cd(nan, nan);
}
}  // namespace

int main() {
  const double tol = 1e-13;
  blockcg::lattice lat(std::vector<int>{4, 2, 4, 2});
  block_fermion_field<32> v0(lat);
  block_fermion_field<16> v1(lat);
  block_fermion_field<5> v2(lat);
  block_fermion_field<8> B(lat), y(lat);
  v0.setGaussian(101);
  v1.setGaussian(102);
  v2.setGaussian(103);
  B.setGaussian(104);
  y.setGaussian(105);
  const block_fermion_field<8>& cB = B;
  const block_fermion_field<8>& cy = y;
  const block_fermion_field<16>& cv1 = v1;
  const block_fermion_field<5>& cv2 = v2;
  blockcg::basis V;
  V.push_back(v0);
  V.push_back(v1);
  V.push_back(v2);
  const size_t K = static_cast<size_t>(V.K());
  if (K != 53 || V.size() != 3) {
    std::printf("basis: K = %zu, %d fields\n", K, V.size());
    return 1;
  }
  columns_t Vh = columns(v0);
  append(Vh, columns(v1));
  append(Vh, columns(v2));

  // ---- basis_dot: element (i, j) at C[j * K + i]
  blockcg::basis_matrix C = blockcg::basis_dot(V, B);
  double e = dot_error(C, Vh, columns(B));
  expect(e <= tol, "basis_dot, V = 32 + 16 + 5 columns, m = 8", e, tol);
  // the mirror, host to device: a write through operator[] reaches basis_dot
  B[3](1, 2) = cd(3.0, -4.0);
  const blockcg::basis_matrix C_written = blockcg::basis_dot(V, B);
  e = dot_error(C_written, Vh, columns(B));
  expect(e <= tol && cB[3](1, 2) == cd(3.0, -4.0), "basis_dot after a host write of B[3]", e, tol);
  double moved = 0.0;
  for (size_t k = 0; k < C.size(); ++k) moved = std::fmax(moved, std::abs(C_written[k] - C[k]));
  expect(moved > 1.0, "... which changed the product by", moved, 1.0);

  // ---- basis_axpy, beta = 0 (y poisoned through the mirror beforehand) and beta = -0.5
  blockcg::basis_matrix Cm(K * 8);
  for (size_t j = 0; j < 8; ++j)
    for (size_t i = 0; i < K; ++i) Cm[j * K + i] = cd(std::cos(0.37 * (i + 1) * (j + 2)), std::sin(0.11 * (i + 3) * (j + 1)));
  const columns_t y0 = columns(y);
  poison(y);
  blockcg::basis_axpy(y, V, Cm, 0.0);
  e = frobenius_error(columns(y), axpy_expected(y0, Vh, Cm, 0.0));
  expect(e <= tol, "basis_axpy, beta = 0 over a y of NaN", e, tol);
  // the mirror, device to host: y[0] read, the update, y[0] read again
  const columns_t y1 = columns(y);
  const cd before = cy[0](0, 0);
  blockcg::basis_axpy(y, V, Cm, -0.5);
  const cd after = cy[0](0, 0);
  const columns_t want = axpy_expected(y1, Vh, Cm, -0.5);
  e = frobenius_error(columns(y), want);
  expect(e <= tol, "basis_axpy, beta = -0.5", e, tol);
  e = std::abs(after - want[0][0]) / std::abs(want[0][0]);
  expect(e <= tol && !same_bits(after, before), "y[0] read again after basis_axpy shows the update", e, tol);
  // the default beta = 1 and the size check
  const columns_t y2 = columns(y);
  blockcg::basis_axpy(y, V, Cm);
  e = frobenius_error(columns(y), axpy_expected(y2, Vh, Cm, 1.0));
  expect(e <= tol, "basis_axpy, default beta = 1", e, tol);
  bool thrown = false;
  try {
    blockcg::basis_axpy(y, V, blockcg::basis_matrix(K * 8 - 1), 1.0);
  } catch (const std::invalid_argument&) {
    thrown = true;
  }
  expect(thrown, "basis_axpy refuses a C that is not K x m", thrown ? 0.0 : 1.0, 0.0);

  // ---- copy_columns, bit for bit, with the mirror of the destination and of the source
  {
    const columns_t s0 = columns(v0);
    const cd d_before = cv1[0](0, 0);
    blockcg::copy_columns(v1, 0, v0, 16, 16);
    const columns_t got = columns(v1);
    int bad = 0;
    for (int j = 0; j < 16; ++j)
      for (size_t r = 0; r < got[j].size(); ++r) bad += !same_bits(got[j][r], s0[16 + j][r]);
    expect(bad == 0, "copy_columns(v1, 0, v0, 16, 16): elements that differ", bad, 0.0);
    expect(same_bits(cv1[0](0, 0), s0[16][0]) && !same_bits(cv1[0](0, 0), d_before), "v1[0] read again shows the copy", 0.0, 0.0);
    v1[7](2, 4) = cd(-1.25, 2.5);  // column 4 is copied below: a host write of the source reaches the device
    const columns_t s1 = columns(v1);
    blockcg::copy_columns(v2, 0, v1, 3, 5);
    const columns_t got2 = columns(v2);
    bad = 0;
    for (int j = 0; j < 5; ++j)
      for (size_t r = 0; r < got2[j].size(); ++r) bad += !same_bits(got2[j][r], s1[3 + j][r]);
    expect(bad == 0, "copy_columns(v2, 0, v1, 3, 5): elements that differ", bad, 0.0);
    expect(same_bits(cv2[7](2, 1), cd(-1.25, 2.5)), "... and the host write of v1[7] arrived", 0.0, 0.0);
    // part of a target: the other columns keep their bits
    const columns_t t0 = columns(v0);
    blockcg::copy_columns(v0, 27, v2, 0, 5);
    const columns_t got0 = columns(v0);
    bad = 0;
    for (int j = 0; j < 32; ++j)
      for (size_t r = 0; r < got0[j].size(); ++r) bad += !same_bits(got0[j][r], j < 27 ? t0[j][r] : got2[j - 27][r]);
    expect(bad == 0, "copy_columns(v0, 27, v2, 0, 5): elements that differ", bad, 0.0);
  }

  // ---- deflate and SBCGrQ_deflated on V = {q}, q orthonormal.  With evals = 1 .. 16 the result is no solution of the
  // system, but a fixed function of its inputs: tests/test_basis.py repeats the calls through the Python bindings.
  block_fermion_field<16> q(lat);
  q.setGaussian(31);
  block_matrix<16> R;
  q.thinQR(R);
  blockcg::basis Vq;
  Vq.push_back(q);
  std::vector<double> evals(16), sigma{0.0, 0.05, 0.5};
  for (int i = 0; i < 16; ++i) evals[i] = i + 1.0;
  dirac_op D(lat, 0.5, 7ULL);
  block_fermion_field<8> Bs(lat);
  Bs.setGaussian(32);
  {
    block_fermion_field<8> Bd(Bs);
    const columns_t b0 = columns(Bd), qh = columns(q);
    const blockcg::basis_matrix Cq = blockcg::deflate(Bd, Vq);
    e = dot_error(Cq, qh, b0);
    expect(e <= tol, "deflate returns V^dagger B", e, tol);
    blockcg::basis_matrix minus(Cq.size());
    for (size_t k = 0; k < Cq.size(); ++k) minus[k] = -Cq[k];
    e = frobenius_error(columns(Bd), axpy_expected(b0, qh, minus, 1.0));
    expect(e <= tol, "deflate leaves B - V (V^dagger B)", e, tol);
    const blockcg::basis_matrix left = blockcg::basis_dot(Vq, Bd);
    long double l2 = 0.0L, b2 = 0.0L;
    for (const cd& z : left) l2 += std::norm(cl(z));
    for (const std::vector<cd>& col : b0) b2 += norm(col) * norm(col);
    e = static_cast<double>(std::sqrt(l2 / b2));
    expect(e <= tol, "|V^dagger B_deflated| / |B|", e, tol);
  }
  std::vector<block_fermion_field<8>> X(sigma.size(), block_fermion_field<8>(lat));
  const int applications = blockcg::SBCGrQ_deflated(X, Bs, D, sigma, Vq, evals, 1e-10, 1e-10);
  std::printf("DEFLATED_APPLICATIONS %d\n", applications);
  for (size_t s = 0; s < sigma.size(); ++s) {
    const block_matrix<8> H = Bs.hermitian_dot(X[s]);  // column-major, like the C ABI's
    std::printf("HDOT %zu", s);
    for (int k = 0; k < 64; ++k) std::printf(" %.17g %.17g", H.data()[k].real(), H.data()[k].imag());
    std::printf("\n");
  }
  std::printf("%s\n", failures == 0 ? "BASIS_PROBE_OK" : "BASIS_PROBE_MISMATCH");
  return failures == 0 ? 0 : 1;
}
