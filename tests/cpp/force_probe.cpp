// GPU probe of the drop-in headers' fermion force (blockcg/force.hpp): F starts from the device generator, then
// blockcg::fermion_force adds the force of four random fields X_s (m = 8) on a 4-D lattice, plain (with four work fields)
// and projected (the library's own work field) into a second field.  Both are written to the file named by argv[1] (raw complex<double>, F then the projected one) for
// tests/test_force.py to compare with the Python interface on the same inputs.  Exit code 0 = ran.
#include <cstdio>
#include <vector>

#include "blockcg/force.hpp"

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: force_probe OUT\n");
    return 2;
  }
  constexpr int N = 8;
  std::vector<int> dims = {8, 4, 4, 6};
  blockcg::lattice lat(dims);
  dirac_op D(lat, 0.3, /*seed=*/51);
  std::vector<block_fermion_field<N>> X;
  for (int s = 0; s < 4; ++s) {
    X.emplace_back(lat);
    X.back().setRandomDevice(52 + s);
  }
  const std::vector<double> residues = {0.7, -1.3, 2.5, 0.25};
  blockcg::gauge_field F(lat), P(lat);
  F.setRandomDevice(60);
  P.setZero();
  std::vector<block_fermion_field<N>> work;  // one pass over F for all four shifts
  for (int s = 0; s < 4; ++s) work.emplace_back(lat);
  blockcg::fermion_force(F, X, D, residues, 0.5, /*project=*/false, &work);
  blockcg::fermion_force(P, X, D, residues, 0.5, /*project=*/true);
  const std::vector<std::complex<double>> f = F.download(), p = P.download();
  std::FILE* out = std::fopen(argv[1], "wb");
  if (!out) return 3;
  const bool ok = std::fwrite(f.data(), sizeof(f[0]), f.size(), out) == f.size() &&
                  std::fwrite(p.data(), sizeof(p[0]), p.size(), out) == p.size();
  std::fclose(out);
  std::printf("%zu links written\n%s\n", f.size(), ok ? "FORCE_OK" : "FORCE_FAILED");
  return ok ? 0 : 1;
}
