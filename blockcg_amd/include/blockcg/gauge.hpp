// blockcg/gauge.hpp -- stout smearing of the gauge links and the plaquette on the device
// (include/blockcg_hip.h: bcg_gauge_stout_smear, bcg_gauge_plaquette).  Included by blockcg/dirac_op.hpp.
//
//   stout_smear(out, in, rho, n_steps, dir, work)   out = S^n_steps(in); scalar rho on all pairs not involving dir
//   stout_smear(out, in, rho_table, n_steps, work)  the same with an ndim x ndim table rho[mu * ndim + nu]
//   plaquette(links)                                ndim x ndim, row-major: sum_x Re tr(plaquette) / (3 V_global)
//
// `out` and `work` are blockcg::gauge_field (blockcg/force.hpp); `in` and `links` are a dirac_op or a gauge_field: anything
// with handle() -> bcg_gauge* and lat().  The reference has none of these; they are extensions in the blockcg namespace, host
// compiler only like the other headers.
#ifndef BLOCKCG_GAUGE_HPP
#define BLOCKCG_GAUGE_HPP
#include <stdexcept>
#include <vector>

#include "fields.hpp"

namespace blockcg {

// rho: ndim x ndim weights, row-major; the diagonal is ignored and a zero entry is not evaluated.  work: a container the
// steps alternate with, overwritten (nullptr: the library allocates one for the call when n_steps >= 2).
template <class Gauge, class Links>
void stout_smear(Gauge& out, const Links& in, const std::vector<double>& rho, int n_steps = 1, Gauge* work = nullptr) {
  const size_t ndim = in.lat().dims().size();
  if (rho.size() != ndim * ndim) throw std::invalid_argument("stout_smear: rho is an ndim x ndim table");
  check(bcg_gauge_stout_smear(in.lat().ctx(), out.handle(), in.handle(), rho.data(), n_steps, work ? work->handle() : nullptr),
        in.lat().ctx(), "stout_smear");
}

// rho on all pairs (mu, nu) not involving dir; dir = -1: all pairs.  dir = 3 on a 4-D lattice is spatial smearing.
template <class Gauge, class Links>
void stout_smear(Gauge& out, const Links& in, double rho, int n_steps = 1, int dir = -1, Gauge* work = nullptr) {
  const int ndim = static_cast<int>(in.lat().dims().size());
  if (dir < -1 || dir >= ndim) throw std::invalid_argument("stout_smear: dir outside -1 ... ndim - 1");
  std::vector<double> table(static_cast<size_t>(ndim) * ndim, 0.0);
  for (int mu = 0; mu < ndim; ++mu)
    for (int nu = 0; nu < ndim; ++nu)
      if (mu != nu && mu != dir && nu != dir) table[mu * ndim + nu] = rho;
  stout_smear(out, in, table, n_steps, work);
}

// P[mu * ndim + nu] = P[nu * ndim + mu]; 0 on the diagonal and for directions of extent 1.  The same bits on every call.
template <class Links>
std::vector<double> plaquette(const Links& links) {
  const size_t ndim = links.lat().dims().size();
  std::vector<double> P(ndim * ndim, 0.0);
  check(bcg_gauge_plaquette(links.lat().ctx(), links.handle(), P.data()), links.lat().ctx(), "plaquette");
  return P;
}

}  // namespace blockcg

#endif
