// Compile-only: blockcg::shift_sum, covariant_shift, laplacian and smear exist for a dirac_op and for a gauge_field, and the
// two C entries have the documented signatures.
#include <complex>
#include <vector>

#include "blockcg/dirac_op.hpp"
#include "blockcg/force.hpp"

typedef block_fermion_field<12> F;
typedef std::vector<std::complex<double>> V;

template <class Links>
void use(F& out, const F& in, const Links& links) {
  blockcg::shift_sum(out, in, links, std::complex<double>(1.0, 2.0), V(4, 1.0), V(), true);
  blockcg::covariant_shift(out, in, links, 1, -1);
  blockcg::laplacian(out, in, links);
  blockcg::laplacian(out, in, links, 3);
  blockcg::smear(out, links, 3, 0.1, 5);
  blockcg::smear(out, links, -1, 0.1, 5, &out);
}
template void use<dirac_op>(F&, const F&, const dirac_op&);
template void use<blockcg::gauge_field>(F&, const F&, const blockcg::gauge_field&);

int (*p_shift)(bcg_context*, const bcg_gauge*, bcg_field*, const bcg_field*, const double*, const double*, const double*, int) =
    &bcg_dirac_shift_sum;
int (*p_smear)(bcg_context*, const bcg_gauge*, bcg_field*, bcg_field*, int, double, int) = &bcg_covariant_smear;

int main() { return p_shift && p_smear ? 0 : 1; }
