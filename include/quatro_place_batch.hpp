// quatro_place_batch.hpp — the grouped place query over quatro_place.hpp: Q queries against one PlaceIndex in one chain of
// launches and one host wait (include/quatro_place_batch.h).  Query q is the single query of its source, range and k.
// Host code only; link with -lquatro_hip -lquatro_ext.
#ifndef QUATRO_PLACE_BATCH_H
#define QUATRO_PLACE_BATCH_H

#include <vector>

#include "quatro_place.hpp"
#include "quatro_place_batch.h"

namespace quatro_hip {

// the items of a call: each is a keyframe, a host descriptor or an entry of an index, with a range of its own
inline qtr_place_query_item place_item(const Keyframe& kf, int id_lo = 0, int id_hi = 0x7fffffff) {
  qtr_place_query_item it{};
  it.kf = kf.get();
  it.entry = -1;
  it.id_lo = id_lo;
  it.id_hi = id_hi;
  return it;
}
// desc: num_rings * num_sectors floats in host memory, alive until the call returns
inline qtr_place_query_item place_item(const float* desc, int id_lo = 0, int id_hi = 0x7fffffff) {
  qtr_place_query_item it{};
  it.desc = desc;
  it.mem = QTR_MEM_HOST;
  it.entry = -1;
  it.id_lo = id_lo;
  it.id_hi = id_hi;
  return it;
}
// entry `entry` of the searched index itself
inline qtr_place_query_item place_entry_item(int entry, int id_lo = 0, int id_hi = 0x7fffffff) {
  qtr_place_query_item it{};
  it.entry = entry;
  it.id_lo = id_lo;
  it.id_hi = id_hi;
  return it;
}
// entry `entry` of another index of the same shape
inline qtr_place_query_item place_entry_item(const PlaceIndex& from, int entry, int id_lo = 0, int id_hi = 0x7fffffff) {
  qtr_place_query_item it = place_entry_item(entry, id_lo, id_hi);
  it.from = from.get();
  return it;
}

// one vector of matches per item: the min(k, entries of its range) most similar, ascending (distance, id); k: 1 .. 64
inline std::vector<std::vector<qtr_place_match>> query_batch(const PlaceIndex& index, const std::vector<qtr_place_query_item>& items,
                                                             int k) {
  std::vector<std::vector<qtr_place_match>> out(items.size());
  if (items.empty()) return out;
  std::vector<qtr_place_match> m(items.size() * static_cast<size_t>(k > 0 ? k : 0));
  std::vector<int> n(items.size(), 0);
  SlotLease lease;
  check(default_handle(), qtr_place_query_batch(default_handle(), lease.slot, index.get(), items.data(),
                                                static_cast<int>(items.size()), k, m.data(), n.data()));
  for (size_t q = 0; q < items.size(); ++q)
    out[q].assign(m.begin() + static_cast<long>(q) * k, m.begin() + static_cast<long>(q) * k + n[q]);
  return out;
}

// loop detection over a finished run: entry i of [first, last) against the entries [0, i - min_gap] of its own index, in
// chunks that keep both caps of a call
inline std::vector<std::vector<qtr_place_match>> find_loops(const PlaceIndex& index, int min_gap, int k, int first = 0,
                                                            int last = 0x7fffffff) {
  const int size = index.size();
  if (last > size) last = size;
  if (first < 0) first = 0;
  std::vector<std::vector<qtr_place_match>> out;
  for (int a = first; a < last;) {
    int b = a + QTR_PLACE_BATCH_MAX < last ? a + QTR_PLACE_BATCH_MAX : last;
    while (b - a > 1 && static_cast<long long>(b - a) * (b > min_gap ? b - min_gap : 0) > QTR_PLACE_BATCH_MAX_PAIRS) --b;
    std::vector<qtr_place_query_item> items;
    for (int i = a; i < b; ++i) items.push_back(place_entry_item(i, 0, i - min_gap + 1));
    for (auto& row : query_batch(index, items, k)) out.push_back(std::move(row));
    a = b;
  }
  return out;
}

}  // namespace quatro_hip
#endif  // QUATRO_PLACE_BATCH_H
