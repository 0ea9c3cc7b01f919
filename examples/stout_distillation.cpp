// examples/stout_distillation.cpp -- a distillation basis over stout-smeared links, the links never leaving the device
// (blockcg/gauge.hpp, blockcg/lowmodes.hpp).
//   1. unitary links (Gram-Schmidt of pseudo-random 3 x 3 matrices on the host) uploaded into a gauge_field
//   2. the plaquette of the thin links
//   3. spatial stout smearing, rho = 0.1 on the pairs not involving direction 3, 3 steps, and the plaquette again
//   4. laplacian_modes along direction 3 with the smeared container as the links (stout smearing keeps unitary links
//      unitary, so 12 = 4 (ndim - 1) still bounds the spectrum)
// Self-check: every spatial plaquette rises and stays below 1, direction 3 is copied bit for bit; the residuals of step 4
// within tol * 12; the smeared container's Laplacian, applied through blockcg::laplacian, reproduces the Ritz values:
// |v_i(t)^dagger (-Lap_3 v_i)(t) - theta_i(t)| <= tol * 12 on every slice.  Exit code 0 and STOUT_DISTILLATION_OK = all of it.
//   stout_distillation [L0 L1 L2 L3]      default 8 8 8 8
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "blockcg/force.hpp"
#include "blockcg/lowmodes.hpp"

namespace {
typedef std::complex<double> cd;
const int N = 8;

// [site][mu][3 x 3 column-major]: the columns of a pseudo-random matrix orthonormalised one after another
std::vector<cd> unitary_links(size_t matrices, unsigned long long seed) {
  unsigned long long state = seed;
  auto draw = [&state]() {
    state = state * 6364136223846793005ULL + 1442695040888963407ULL;
    return static_cast<double>(state >> 11) / 9007199254740992.0 - 0.5;
  };
  std::vector<cd> U(matrices * 9);
  for (size_t k = 0; k < matrices; ++k) {
    cd* u = &U[k * 9];
    for (int j = 0; j < 3; ++j) {
      for (int i = 0; i < 3; ++i) u[3 * j + i] = cd(draw(), draw());
      for (int pass = 0; pass < 2; ++pass)
        for (int l = 0; l < j; ++l) {
          cd s = 0.0;
          for (int i = 0; i < 3; ++i) s += std::conj(u[3 * l + i]) * u[3 * j + i];
          for (int i = 0; i < 3; ++i) u[3 * j + i] -= s * u[3 * l + i];
        }
      double n = 0.0;
      for (int i = 0; i < 3; ++i) n += std::norm(u[3 * j + i]);
      for (int i = 0; i < 3; ++i) u[3 * j + i] /= std::sqrt(n);
    }
  }
  return U;
}

void print_plaquette(const char* what, const std::vector<double>& P) {
  std::printf("# plaquette, %s:", what);
  for (int mu = 0; mu < 4; ++mu)
    for (int nu = mu + 1; nu < 4; ++nu) std::printf("  P%d%d = %.12f", mu, nu, P[mu * 4 + nu]);
  std::printf("\n");
}
}  // namespace

int main(int argc, char** argv) {
  std::vector<int> dims = {8, 8, 8, 8};
  if (argc >= 5)
    for (int mu = 0; mu < 4; ++mu) dims[mu] = std::atoi(argv[1 + mu]);
  const double tol = 1e-10, ub = 12.0;
  const int T = dims[3];
  blockcg::lattice lat(dims);
  const std::vector<cd> links = unitary_links(static_cast<size_t>(lat.V()) * 4, 7ULL);

  // 1 - 3. thin links, their plaquette, the smeared links and theirs
  blockcg::gauge_field thin(lat), smeared(lat);
  thin.upload(links.data());
  const std::vector<double> P0 = blockcg::plaquette(thin);
  print_plaquette("thin links", P0);
  blockcg::stout_smear(smeared, thin, 0.1, 3, 3);
  const std::vector<double> P1 = blockcg::plaquette(smeared);
  print_plaquette("3 spatial stout steps at rho = 0.1", P1);
  bool ok = true;
  for (int mu = 0; mu < 3; ++mu)
    for (int nu = mu + 1; nu < 3; ++nu) ok = ok && P1[mu * 4 + nu] > P0[mu * 4 + nu] && P1[mu * 4 + nu] < 1.0;
  {
    const std::vector<cd> out = smeared.download();
    size_t moved = 0;
    for (size_t s = 0; s < static_cast<size_t>(lat.V()); ++s)
      for (int k = 0; k < 9; ++k) moved += out[(s * 4 + 3) * 9 + k] != links[(s * 4 + 3) * 9 + k];
    ok = ok && moved == 0;
    std::printf("# entries of the direction-3 links that changed: %zu\n", moved);
  }

  // 4. the basis over the smeared links
  block_fermion_field<N> v(lat);
  v.setGaussian(41);
  blockcg::mutable_basis Vm;
  Vm.push_back(v);
  const blockcg::laplacian_modes_result modes = blockcg::laplacian_modes(Vm, smeared, 3, N, ub, 16, tol, 60);
  ok = ok && modes.evals.size() == static_cast<size_t>(T);
  block_fermion_field<N> Lv(lat);
  blockcg::laplacian(Lv, v, smeared, 3);
  const block_fermion_field<N>& cv = v;
  const std::vector<block_matrix<N>> G = cv.slice_gram(Lv, 3);
  double worst = 0.0, ritz = 0.0;
  std::printf("# %d outer iterations\n# t  theta_1(t) theta_%d(t)\n", modes.iterations, N);
  for (int t = 0; ok && t < T; ++t) {
    std::printf("%3d  %.14e %.14e\n", t, modes.evals[t][0], modes.evals[t][N - 1]);
    for (int i = 0; i < N; ++i) {
      worst = std::fmax(worst, modes.resid[t][i]);
      ritz = std::fmax(ritz, std::abs(-G[t](i, i) - cd(modes.evals[t][i])));
    }
  }
  ok = ok && worst <= tol * ub && ritz <= tol * ub;
  std::printf("# basis: worst residual %.3e, worst |v^dagger (-Lap) v - theta| %.3e (bound %.1e)\n", worst, ritz, tol * ub);
  std::printf("%s\n", ok ? "STOUT_DISTILLATION_OK" : "STOUT_DISTILLATION_FAILED");
  return ok ? 0 : 1;
}
