// quatro_place.hpp — the place index over the process-wide handle of quatro_hip_cxx.hpp: one Scan Context descriptor per
// keyframe on the device, and "the k entries most similar to this keyframe, with their yaw" — the candidates that
// register_one_to_many (quatro_keyframe.hpp) then registers against.  A query only reads the index; add and query on the
// same index must not overlap.
// Host code only; link with -lquatro_hip.
#ifndef QUATRO_PLACE_H
#define QUATRO_PLACE_H

#include <vector>

#include "quatro_keyframe.hpp"

namespace quatro_hip {

inline qtr_place_params default_place_params() {
  qtr_place_params p;
  qtr_default_place_params(&p);
  return p;
}

// RAII owner of one qtr_place_index of default_handle(); move-only.
class PlaceIndex {
 public:
  PlaceIndex() = default;
  explicit PlaceIndex(int capacity, const qtr_place_params& p = default_place_params()) {
    check(default_handle(), qtr_place_index_create(default_handle(), &p, capacity, &ix_));
  }
  ~PlaceIndex() { reset(); }
  PlaceIndex(PlaceIndex&& o) noexcept : ix_(o.ix_) { o.ix_ = nullptr; }
  PlaceIndex& operator=(PlaceIndex&& o) noexcept {
    if (this != &o) {
      reset();
      ix_ = o.ix_;
      o.ix_ = nullptr;
    }
    return *this;
  }
  PlaceIndex(const PlaceIndex&) = delete;
  PlaceIndex& operator=(const PlaceIndex&) = delete;

  void reset() {
    if (ix_) qtr_place_index_destroy(default_handle(), ix_);
    ix_ = nullptr;
  }
  explicit operator bool() const { return ix_ != nullptr; }
  const qtr_place_index* get() const { return ix_; }
  qtr_place_index_info info() const {
    qtr_place_index_info i{};
    check(default_handle(), qtr_place_index_get_info(ix_, &i));
    return i;
  }
  int size() const { return info().size; }

  // the keyframe's descriptor becomes the next entry; returns its id (0, 1, 2, ...)
  int add(const Keyframe& kf) {
    SlotLease lease;
    int id = -1;
    check(default_handle(), qtr_place_index_add(default_handle(), lease.slot, ix_, kf.get(), &id));
    return id;
  }
  // a descriptor made earlier (fetch of a saved index): num_rings * num_sectors floats in host memory
  int add(const std::vector<float>& desc) {
    const qtr_place_index_info i = info();
    if (desc.size() != static_cast<size_t>(i.params.num_rings) * static_cast<size_t>(i.params.num_sectors))
      throw std::invalid_argument("[quatro_hip] PlaceIndex::add: descriptor size");
    SlotLease lease;
    int id = -1;
    check(default_handle(), qtr_place_index_add_desc(default_handle(), lease.slot, ix_, desc.data(), QTR_MEM_HOST, &id));
    return id;
  }
  // QTR_PLACE_DESC / QTR_PLACE_COLNORM2 of entry `id`
  std::vector<float> fetch(int id, int what = QTR_PLACE_DESC) const {
    const long long bytes = qtr_place_index_fetch(default_handle(), ix_, id, what, nullptr, 0);
    if (bytes < 0) throw std::invalid_argument("[quatro_hip] qtr_place_index_fetch");
    std::vector<float> out(static_cast<size_t>(bytes) / 4);
    if (bytes > 0) qtr_place_index_fetch(default_handle(), ix_, id, what, out.data(), static_cast<size_t>(bytes));
    return out;
  }
  // the min(k, candidates) entries of [id_lo, id_hi) most similar to the keyframe, ascending (distance, id); k: 1 .. 64
  std::vector<qtr_place_match> query(const Keyframe& kf, int k, int id_lo = 0, int id_hi = 0x7fffffff) const {
    SlotLease lease;
    qtr_place_match m[64];
    int n = 0;
    check(default_handle(), qtr_place_query(default_handle(), lease.slot, ix_, kf.get(), id_lo, id_hi, k, m, &n));
    return std::vector<qtr_place_match>(m, m + n);
  }

 private:
  qtr_place_index* ix_ = nullptr;
};

}  // namespace quatro_hip
#endif  // QUATRO_PLACE_H
