// Compile-only: the per-slice Gram members exist on block_fermion_field<12> with the documented signatures, and the C entry.
#include <vector>

#include "blockcg/fields.hpp"

typedef block_fermion_field<12> F;
std::vector<block_matrix<12>> (F::*p_gram)(const F&, int) const = &F::slice_gram;
std::vector<block_matrix<12>> (F::*p_gram_mom)(const F&, int, const std::vector<std::vector<int>>&) const = &F::slice_gram;
int (*p_entry)(const bcg_field*, const bcg_field*, int, int, const int*, double*) = &bcg_field_slice_gram;

int main() { return p_gram && p_gram_mom && p_entry ? 0 : 1; }
