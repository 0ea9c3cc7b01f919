// GPU probe of the drop-in headers' sum mode (blockcg::SBCGrQ_sum): the same solve as SBCGrQ on the same inputs, the
// shifted solutions summed into one field.  Y must match c0 B + sum_s a_s X_s of the ordinary solve to 1e-12 relative to
// |c0| |B| + sum_s |a_s| |X_s|, with the same iteration count.  Exit code 0 = passed.
#include <cmath>
#include <cstdio>

#include "blockcg/block_solvers.hpp"

template <int N>
static double norm(const block_fermion_field<N>& f) {
  return std::sqrt(f.hermitian_dot(f).diagonal().real().sum());
}

int main() {
  constexpr int N = 16;
  std::vector<int> dims = {16, 4, 4, 4};
  blockcg::lattice lat(dims);
  dirac_op D(lat, 0.2, /*seed=*/41);
  block_fermion_field<N> B(lat);
  B.setRandomDevice(42);
  std::vector<double> shifts = {0.0, 1e-3, 0.1, 2.0};
  const std::vector<double> residues = {0.7, -1.3, 2.5, 0.25};
  const double c0 = 0.4, eps = 1e-10, eps_shifts = 1e-12;
  std::vector<block_fermion_field<N>> X;
  for (size_t s = 0; s < shifts.size(); ++s) X.emplace_back(lat);
  const int it = SBCGrQ(X, B, D, shifts, eps, eps_shifts);
  block_fermion_field<N> Y(lat);
  const int it_sum = blockcg::SBCGrQ_sum(Y, B, D, shifts, residues, c0, eps, eps_shifts);
  block_fermion_field<N> Z(lat);  // c0 B + sum_s a_s X_s from the ordinary solve
  Z.setZero();
  Z.add(B, c0);
  double scale = std::fabs(c0) * norm(B);
  for (size_t s = 0; s < shifts.size(); ++s) {
    Z.add(X[s], residues[s]);
    scale += std::fabs(residues[s]) * norm(X[s]);
  }
  Z -= Y;
  const double err = norm(Z) / scale;
  const bool ok = it == it_sum && err < 1e-12;
  std::printf("SBCGrQ %d, SBCGrQ_sum %d operator applications; |Y - (c0 B + sum a_s X_s)| / scale = %.3e\n", it, it_sum, err);
  std::printf("%s\n", ok ? "SUM_OK" : "SUM_FAILED");
  return ok ? 0 : 1;
}
