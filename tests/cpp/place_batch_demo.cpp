// place_batch_demo.cpp — the grouped place query written against include/quatro_place_batch.hpp: every map scan becomes a
// keyframe and an entry of the place index; the query scans' keyframes, and entry 0 of the index itself, are looked up in ONE
// call; then every entry is looked up among the entries at least one behind it (find_loops).
// usage: place_batch_demo k n_queries query0.bin [...] map0.bin [map1.bin ...]   (.bin = float32 x,y,z,intensity records)
// Prints "query q match r id i shift s distance_bits xxxxxxxx" per query and candidate, then "loop i match r id ..." likewise.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "quatro_place_batch.hpp"

static void print_rows(const char* what, const std::vector<std::vector<qtr_place_match>>& rows) {
  for (size_t q = 0; q < rows.size(); ++q)
    for (size_t r = 0; r < rows[q].size(); ++r) {
      unsigned bits = 0;
      std::memcpy(&bits, &rows[q][r].distance, 4);
      std::printf("%s %zu match %zu id %d shift %d distance_bits %08x\n", what, q, r, rows[q][r].id, rows[q][r].shift, bits);
    }
}

int main(int argc, char** argv) {
  const int nq = argc > 2 ? std::atoi(argv[2]) : 0;
  if (argc < 5 || nq < 1 || argc < 4 + nq) {
    std::fprintf(stderr, "usage: %s k n_queries query0.bin [...] map0.bin [map1.bin ...]\n", argv[0]);
    return 2;
  }
  const int k = std::atoi(argv[1]);
  qtr_frontend_params fp;
  qtr_default_frontend_params(&fp);
  std::vector<float> buffer(1000000);
  auto load = [&](const char* path) {
    int n = 0;
    if (qtr_read_kitti_bin(path, buffer.data(), 250000, &n) != QTR_OK) {
      std::fprintf(stderr, "cannot read %s\n", path);
      std::exit(1);
    }
    return quatro_hip::Keyframe(buffer.data(), n, fp);
  };
  std::vector<quatro_hip::Keyframe> queries, map;
  for (int a = 3; a < 3 + nq; ++a) queries.push_back(load(argv[a]));
  quatro_hip::PlaceIndex index(argc - 3 - nq);
  for (int a = 3 + nq; a < argc; ++a) {
    map.push_back(load(argv[a]));
    index.add(map.back());
  }
  std::vector<qtr_place_query_item> items;
  for (const quatro_hip::Keyframe& q : queries) items.push_back(quatro_hip::place_item(q));
  const int first = 0;
  items.push_back(quatro_hip::place_entry_item(first, 1));  // entry 0 among the entries from 1 on
  print_rows("query", quatro_hip::query_batch(index, items, k));
  print_rows("loop", quatro_hip::find_loops(index, 1, k));
  return 0;
}
