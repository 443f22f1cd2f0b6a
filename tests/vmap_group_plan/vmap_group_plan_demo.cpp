// Drives quatro_amd/csrc/vmap_group_plan.h from stdin, one group per line (tests/test_vmap_group_plan_cpu.py), laid out as the
// two users lay theirs out: H head sections, every item's M own sections, then the staged clouds.
//   g H B M  h_1 .. h_H  then per item: host src nrm n  p_1 .. p_M      (src / nrm: addresses as integers, never read)
//   -> "need  o_h_1 .. o_h_H  then per item: o_p_1 .. o_p_M same_as o_src o_nrm"
//   u BYTES -> "qtr_up256(BYTES)"
#include <cstdint>
#include <cstdio>
#include <vector>

#include "vmap_group_plan.h"

int main() {
  char op;
  while (scanf(" %c", &op) == 1) {
    if (op == 'u') {
      unsigned long long b;
      if (scanf("%llu", &b) != 1) return 2;
      printf("%llu\n", (unsigned long long)qtr_up256((size_t)b));
    } else if (op == 'g') {
      int H, B, M;
      if (scanf("%d %d %d", &H, &B, &M) != 3 || H < 0 || B < 0 || M < 0) return 2;
      VmapCursor cur;
      std::vector<size_t> head((size_t)H), own((size_t)B * M);
      for (int k = 0; k < H; ++k) {
        unsigned long long b;
        if (scanf("%llu", &b) != 1) return 2;
        head[k] = cur.take((size_t)b);
      }
      std::vector<VmapGroupItem> it((size_t)B);  // (a heap array: a step past the B items is the sanitizer's to find)
      for (int i = 0; i < B; ++i) {
        int host;
        unsigned long long src, nrm;
        if (scanf("%d %llu %llu %d", &host, &src, &nrm, &it[i].n) != 4) return 2;
        it[i].host = host != 0;
        it[i].src = (const void*)(uintptr_t)src;
        it[i].nrm = (const void*)(uintptr_t)nrm;
        it[i].same_as = 12345, it[i].o_src = it[i].o_nrm = 777;  // (stale values: the plan must not depend on them)
        for (int k = 0; k < M; ++k) {
          unsigned long long b;
          if (scanf("%llu", &b) != 1) return 2;
          own[(size_t)i * M + k] = cur.take((size_t)b);
        }
      }
      vmap_group_plan(it.data(), B, cur);
      printf("%zu", cur.need);
      for (int k = 0; k < H; ++k) printf(" %zu", head[k]);
      for (int i = 0; i < B; ++i) {
        for (int k = 0; k < M; ++k) printf(" %zu", own[(size_t)i * M + k]);
        const bool staged = it[i].host && it[i].n > 0;
        printf(" %d %lld %lld", it[i].same_as, staged ? (long long)it[i].o_src : -1LL, staged ? (long long)it[i].o_nrm : -1LL);
      }
      printf("\n");
    } else {
      return 2;
    }
  }
  return 0;
}
