// blockcg/force.hpp -- the fermion force of multi-shift solutions (include/blockcg_hip.h, bcg_force_accumulate).
//
// blockcg::gauge_field is a link-shaped device field of a lattice ([site][mu][3x3 column-major], the layout of the links
// dirac_op takes); blockcg::fermion_force adds  scale * sum_s residues[s] G(X_s)  to it, or TA(U G) per link with project.
// The reference has no force; these are extensions in the blockcg namespace, host compiler only like the other headers.
#ifndef BLOCKCG_FORCE_HPP
#define BLOCKCG_FORCE_HPP
#include <complex>
#include <memory>
#include <stdexcept>
#include <vector>

#include "dirac_op.hpp"
#include "fields.hpp"

namespace blockcg {

class gauge_field {
 public:
  explicit gauge_field(lattice& lat) : lat_(&lat) {
    rand_state_guard keep_callers_rand_sequence;
    bcg_gauge* g = nullptr;
    check(bcg_gauge_create(lat.ctx(), &g), lat.ctx(), "bcg_gauge_create");
    g_ = std::unique_ptr<bcg_gauge, int (*)(bcg_gauge*)>(g, bcg_gauge_destroy);
  }
  // matrices held: local sites x ndim
  size_t size() const { return static_cast<size_t>(lat_->V()) * lat_->dims().size(); }
  void setZero() { check(bcg_gauge_set_zero(g_.get()), lat_->ctx(), "bcg_gauge_set_zero"); }
  // i.i.d. uniform [-1,1) per real component, the generator of dirac_op(lat, mass, seed)
  void setRandomDevice(unsigned long long seed) { check(bcg_gauge_fill_random(g_.get(), seed), lat_->ctx(), "bcg_gauge_fill_random"); }
  void upload(const std::complex<double>* links) {
    check(bcg_gauge_upload(g_.get(), reinterpret_cast<const double*>(links)), lat_->ctx(), "bcg_gauge_upload");
  }
  // 9 complex per matrix, size() matrices
  std::vector<std::complex<double>> download() const {
    std::vector<std::complex<double>> out(size() * 9);
    check(bcg_gauge_download(g_.get(), reinterpret_cast<double*>(out.data())), lat_->ctx(), "bcg_gauge_download");
    return out;
  }
  bcg_gauge* handle() const { return g_.get(); }
  lattice& lat() const { return *lat_; }

 private:
  lattice* lat_;
  std::unique_ptr<bcg_gauge, int (*)(bcg_gauge*)> g_{nullptr, bcg_gauge_destroy};
};

// F += scale * sum_s residues[s] G(X_s)  (project: TA(U G)), the links those of D.  X: fields of one width and parity.
// work: fields of X's width and parity for D X_s, overwritten.  With X.size() of them F is read and written once per call;
// nullptr (or an empty vector) lets the library allocate one field for the call and run one pass over F per shift.
template <int N_rhs>
void fermion_force(gauge_field& F, const std::vector<block_fermion_field<N_rhs>>& X, const dirac_op& D,
                   const std::vector<double>& residues, double scale = 1.0, bool project = false,
                   std::vector<block_fermion_field<N_rhs>>* work = nullptr) {
  if (residues.size() != X.size()) throw std::invalid_argument("number of residues does not match number of fields");
  std::vector<bcg_field*> Xh(X.size()), Wh;
  for (size_t s = 0; s < X.size(); ++s) {
    X[s].flush();
    Xh[s] = X[s].handle();
  }
  if (work)
    for (auto& w : *work) Wh.push_back(w.handle());
  check(bcg_force_accumulate(D.lat().ctx(), D.handle(), Xh.data(), static_cast<int>(X.size()), residues.data(), scale,
                             project ? 1 : 0, Wh.empty() ? nullptr : Wh.data(), static_cast<int>(Wh.size()), F.handle()),
        D.lat().ctx(), "fermion_force");
  if (work)
    for (auto& w : *work) w.device_written();
}

}  // namespace blockcg

#endif
