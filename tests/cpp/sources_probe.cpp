// Compile-only: the source / sink members exist on block_fermion_field<12> with the documented signatures.
#include <complex>
#include <vector>

#include "blockcg/fields.hpp"

typedef block_fermion_field<12> F;
void (F::*p_gauss)(unsigned long long) = &F::setGaussian;
void (F::*p_z2)(unsigned long long) = &F::setZ2;
void (F::*p_z4)(unsigned long long) = &F::setZ4;
void (F::*p_point)(const std::vector<std::vector<int>>&, const std::vector<int>&) = &F::setPointSources;
void (F::*p_wall)(int, const std::vector<int>&, const std::vector<int>&, int) = &F::setWallSources;
std::vector<std::complex<double>> (F::*p_dot)(const F&, int) const = &F::slice_dot;

int main() { return p_gauss && p_z2 && p_z4 && p_point && p_wall && p_dot ? 0 : 1; }
