// blockcg/shift.hpp -- covariant shifts, the covariant Laplacian and source smearing on the device
// (include/blockcg_hip.h: bcg_dirac_shift_sum, bcg_covariant_smear).  Included by blockcg/dirac_op.hpp.
//
//   shift_sum(out, in, links, c0, fwd, bwd, eta)
//       out(x) = c0 in(x) + sum_mu s_mu(x) [fwd[mu] U_mu(x) in(x+mu) + bwd[mu] U_mu(x-mu)^dagger in(x-mu)]
//   covariant_shift(out, in, links, mu, sign)   one term of it: U_mu(x) in(x+mu) (sign > 0) or U_mu(x-mu)^dagger in(x-mu)
//   laplacian(out, in, links, dir = -1)         sum_{mu != dir} [U in(x+mu) + U^dagger in(x-mu) - 2 in(x)]
//   smear(f, links, dir, kappa, n_iter, work)   f <- (1 + kappa Lap_dir)^n_iter f
//
// `links` is a dirac_op or a blockcg::gauge_field (blockcg/force.hpp): anything with handle() -> bcg_gauge* and lat().  The
// reference has none of these; they are extensions in the blockcg namespace, host compiler only like the other headers.
#ifndef BLOCKCG_SHIFT_HPP
#define BLOCKCG_SHIFT_HPP
#include <complex>
#include <stdexcept>
#include <vector>

#include "fields.hpp"

namespace blockcg {

// fwd, bwd: one coefficient per direction of the lattice, or empty (all 0); a term whose coefficient is exactly 0 is not
// evaluated.  eta: s_mu(x) = (-1)^(x_0+...+x_{mu-1}) instead of 1.  Half fields: in of parity p, out of parity 1 - p, c0 = 0.
template <int N_rhs, class Links>
void shift_sum(block_fermion_field<N_rhs>& out, const block_fermion_field<N_rhs>& in, const Links& links, std::complex<double> c0,
               const std::vector<std::complex<double>>& fwd, const std::vector<std::complex<double>>& bwd, bool eta = false) {
  const size_t ndim = links.lat().dims().size();
  if ((!fwd.empty() && fwd.size() != ndim) || (!bwd.empty() && bwd.size() != ndim))
    throw std::invalid_argument("shift_sum: one coefficient per direction, or none");
  in.flush();
  const double c[2] = {c0.real(), c0.imag()};
  check(bcg_dirac_shift_sum(links.lat().ctx(), links.handle(), out.handle(), in.handle(), c,
                            fwd.empty() ? nullptr : reinterpret_cast<const double*>(fwd.data()),
                            bwd.empty() ? nullptr : reinterpret_cast<const double*>(bwd.data()), eta ? 1 : 0),
        links.lat().ctx(), "shift_sum");
  out.device_written();
}

template <int N_rhs, class Links>
void covariant_shift(block_fermion_field<N_rhs>& out, const block_fermion_field<N_rhs>& in, const Links& links, int mu, int sign) {
  const size_t ndim = links.lat().dims().size();
  if (mu < 0 || static_cast<size_t>(mu) >= ndim || sign == 0) throw std::invalid_argument("covariant_shift: mu outside the lattice, or sign 0");
  std::vector<std::complex<double>> one(ndim, 0.0), none;
  one[mu] = 1.0;
  shift_sum(out, in, links, 0.0, sign > 0 ? one : none, sign > 0 ? none : one);
}

template <int N_rhs, class Links>
void laplacian(block_fermion_field<N_rhs>& out, const block_fermion_field<N_rhs>& in, const Links& links, int dir = -1) {
  const int ndim = static_cast<int>(links.lat().dims().size());
  if (dir < -1 || dir >= ndim) throw std::invalid_argument("laplacian: dir outside -1 ... ndim - 1");
  std::vector<std::complex<double>> hop(ndim, 1.0);
  if (dir >= 0) hop[dir] = 0.0;
  shift_sum(out, in, links, -2.0 * (ndim - (dir >= 0 ? 1 : 0)), hop, hop);
}

// work: a field of f's shape, overwritten (nullptr: the library allocates one for the call)
template <int N_rhs, class Links>
void smear(block_fermion_field<N_rhs>& f, const Links& links, int dir, double kappa, int n_iter,
           block_fermion_field<N_rhs>* work = nullptr) {
  f.flush();
  check(bcg_covariant_smear(links.lat().ctx(), links.handle(), f.handle(), work ? work->handle() : nullptr, dir, kappa, n_iter),
        links.lat().ctx(), "smear");
  if (n_iter > 0) f.device_written();
  if (work && n_iter > 0) work->device_written();
}

}  // namespace blockcg

#endif
