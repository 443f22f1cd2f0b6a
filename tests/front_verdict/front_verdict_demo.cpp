// Drives quatro_amd/csrc/front_verdict.h from stdin, one call per line (tests/test_front_verdict_cpu.py):
//   v NVOX OVERFLOW P MAX_VOXELS              -> "n passed reason"
//   p VOX_PASSES VOX_FEWER BITS LAUNCHED ATT  -> "rerun vox_passes vox_fewer"
//   l LONG LINES t0 c0 o0 t1 c1 o1            -> "verdict"   (t / c / o: CNT_VOX_TAILERR / _NBR_CAPACITY / _NBR_OVERFLOW)
#include <cstdio>
#include <vector>

#include "front_verdict.h"

int main() {
  char op;
  while (scanf(" %c", &op) == 1) {
    if (op == 'v') {
      int nvox, ovf, P, maxv;
      if (scanf("%d %d %d %d", &nvox, &ovf, &P, &maxv) != 4) return 2;
      std::vector<int> c(16, 0);  // (a heap line: a read past a counter line is the sanitizer's to find)
      c[CNT_NVOX] = nvox;
      c[CNT_VOX_OVERFLOW] = ovf;
      const VoxVerdict v = vox_verdict(c.data(), P, maxv);
      printf("%d %d %d\n", v.n, v.passed ? 1 : 0, (int)v.reason);
    } else if (op == 'p') {
      int passes, fewer, bits, launched, attempt;
      if (scanf("%d %d %d %d %d", &passes, &fewer, &bits, &launched, &attempt) != 5) return 2;
      const bool rerun = vox_passes_next(passes, fewer, bits, launched, attempt);
      printf("%d %d %d\n", rerun ? 1 : 0, passes, fewer);
    } else if (op == 'l') {
      int long_lists, lines, w[6];
      if (scanf("%d %d %d %d %d %d %d %d", &long_lists, &lines, w, w + 1, w + 2, w + 3, w + 4, w + 5) != 8) return 2;
      std::vector<int> c0(16, 0), c1(16, 0);
      c0[CNT_VOX_TAILERR] = w[0], c0[CNT_NBR_CAPACITY] = w[1], c0[CNT_NBR_OVERFLOW] = w[2];
      c1[CNT_VOX_TAILERR] = w[3], c1[CNT_NBR_CAPACITY] = w[4], c1[CNT_NBR_OVERFLOW] = w[5];
      printf("%d\n", (int)lists_verdict(c0.data(), lines == 2 ? c1.data() : nullptr, long_lists != 0));
    } else {
      return 2;
    }
  }
  return 0;
}
