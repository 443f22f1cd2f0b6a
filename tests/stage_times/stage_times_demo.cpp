// The table of quatro_amd/csrc/stage_times.h, walked the way compute_times (capi.hip) walks it, on synthetic event times:
// event id k happened at 2^k ms, so every (from, to) pair gives another difference.  One line per call shape:
//   <shape> <sync event> <nn 0|1> <voxelize> <fpfh> <match> <graph> <clique> <solve> <total>
#include <cstdio>

#include "stage_times.h"

int main() {
  for (int shape = 0; shape < TIMES_SHAPES; ++shape) {
    const ShapeTimes& sh = k_shape_times[shape];
    long field[SF_COUNT] = {};
    for (int r = 0; r < sh.nrows; ++r) {
      const StageRow& row = sh.rows[r];
      if (row.field < 0 || row.field >= SF_COUNT || row.from < 0 || row.from >= EV_COUNT || row.to < 0 || row.to >= EV_COUNT)
        return 1;
      field[row.field] = (1L << row.to) - (1L << row.from);
    }
    printf("%d %d %d", shape, sh.sync, sh.nn ? 1 : 0);
    for (int f = 0; f < SF_COUNT; ++f) printf(" %ld", field[f]);
    printf("\n");
  }
  return 0;
}
