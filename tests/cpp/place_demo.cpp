// place_demo.cpp — loop closing written against include/quatro_place.hpp: every map scan becomes a keyframe and an entry of
// the place index; the query scan's keyframe is looked up, its best candidates are registered as one batched job.
// usage: place_demo k query.bin map0.bin map1.bin [...]   (.bin = float32 x,y,z,intensity records)
// Prints "match r id i shift s distance_bits xxxxxxxx" per candidate, then "best i valid v n_final n" and the winner's
// 4x4 as the hex bits of every double.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "quatro_place.hpp"

int main(int argc, char** argv) {
  if (argc < 4) {
    std::fprintf(stderr, "usage: %s k query.bin map0.bin [map1.bin ...]\n", argv[0]);
    return 2;
  }
  const int k = std::atoi(argv[1]);
  qtr_frontend_params fp;
  qtr_default_frontend_params(&fp);
  qtr_params prm;
  qtr_demo_params(&prm);
  std::vector<float> buffer(1000000);
  auto load = [&](const char* path) {
    int n = 0;
    if (qtr_read_kitti_bin(path, buffer.data(), 250000, &n) != QTR_OK) {
      std::fprintf(stderr, "cannot read %s\n", path);
      std::exit(1);
    }
    return quatro_hip::Keyframe(buffer.data(), n, fp);
  };
  std::vector<quatro_hip::Keyframe> map;
  quatro_hip::PlaceIndex index(argc - 3);
  for (int a = 3; a < argc; ++a) {
    map.push_back(load(argv[a]));
    index.add(map.back());
  }
  const quatro_hip::Keyframe query = load(argv[2]);
  const std::vector<qtr_place_match> found = index.query(query, k);
  std::vector<const quatro_hip::Keyframe*> candidates;
  for (size_t r = 0; r < found.size(); ++r) {
    unsigned bits = 0;
    std::memcpy(&bits, &found[r].distance, 4);
    std::printf("match %zu id %d shift %d distance_bits %08x\n", r, found[r].id, found[r].shift, bits);
    candidates.push_back(&map[static_cast<size_t>(found[r].id)]);
  }
  int best = -1;
  const std::vector<qtr_result> recs = quatro_hip::register_one_to_many(query, candidates, fp, prm, &best);
  if (best < 0) {
    std::printf("best -1\n");
    return 0;
  }
  const qtr_result& w = recs[static_cast<size_t>(best)];
  std::printf("best %d valid %d n_final %d\n", found[static_cast<size_t>(best)].id, w.valid, w.n_final);
  for (int i = 0; i < 4; ++i)
    for (int c = 0; c < 4; ++c) {
      unsigned long long b = 0;
      std::memcpy(&b, &w.T[4 * i + c], 8);
      std::printf("%016llx%c", b, c == 3 ? '\n' : ' ');
    }
  return 0;
}
