// Probe for blockcg_amd/csrc/hermitian_eig.hpp (tests/test_lowmodes_cpu.py): reads an n x n complex matrix (column-major,
// interleaved) from stdin, writes theta (n doubles) and Z (n x n, column-major, interleaved) to stdout.  Exit status 1 when
// the decomposition reports failure, 2 on a short read.  Host code only; built plain and with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hermitian_eig.hpp"

int main(int argc, char** argv) {
  const int n = argc > 1 ? std::atoi(argv[1]) : 0;
  if (n < 1 || n > 4096) return 2;
  std::vector<double> in(static_cast<size_t>(2) * n * n);
  if (std::fread(in.data(), sizeof(double), in.size(), stdin) != in.size()) return 2;
  const bcg::CMat A(n, in.data());
  std::vector<double> theta;
  bcg::CMat Z;
  if (!bcg::hermitian_eig(A, theta, Z)) return 1;
  std::vector<double> out(in.size());
  Z.store(out.data());
  std::fwrite(theta.data(), sizeof(double), theta.size(), stdout);
  std::fwrite(out.data(), sizeof(double), out.size(), stdout);
  return 0;
}
