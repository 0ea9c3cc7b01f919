// Compile-only: the basis products, the column copy and the deflated solve of blockcg/basis.hpp exist for fields of unequal
// widths, and the three C entries have the documented signatures.
#include <vector>

#include "blockcg/basis.hpp"

typedef block_fermion_field<8> F;

int use(std::vector<F>& X, F& B, const dirac_op& D, block_fermion_field<32>& v0, block_fermion_field<16>& v1,
        block_fermion_field<5>& narrow) {
  blockcg::basis V;
  V.push_back(v0);
  V.push_back(v1);
  blockcg::basis_matrix C = blockcg::basis_dot(V, B);
  blockcg::basis_axpy(B, V, C, 0.0);
  blockcg::basis_axpy(B, V, C);
  blockcg::copy_columns(v1, 0, v0, 16, 16);
  blockcg::copy_columns(narrow, 0, v1, 3, 5);
  C = blockcg::deflate(B, V);
  std::vector<double> sigma(X.size(), 0.0), evals(V.K(), 1.0);
  blockcg::low_mode_solution(X, V, evals, C, sigma);
  return blockcg::SBCGrQ_deflated(X, B, D, sigma, V, evals, 1e-10, 1e-10, 1000);
}

int (*p_dot)(const bcg_field* const*, int, const bcg_field*, double*) = &bcg_basis_dot;
int (*p_axpy)(bcg_field*, const bcg_field* const*, int, const double*, double) = &bcg_basis_axpy;
int (*p_copy)(bcg_field*, int, const bcg_field*, int, int) = &bcg_field_copy_columns;

int main() { return p_dot && p_axpy && p_copy ? 0 : 1; }
