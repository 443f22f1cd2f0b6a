// qtr_place_math.h — the arithmetic of the Scan Context place index (Kim & Kim, IROS 2018), shared by the gfx950 kernels
// (quatro_amd/csrc/place.hip) and any host restatement, in the style of qtr_math.h / qtr_icp_math.h: binary32 + - * /
// sqrt only (qm_atan2f evaluates in binary64 and rounds once), evaluated in the order written.  Both sides compile with
// -ffp-contract=off: NO product-sum below is fused, so a plain float32 restatement reproduces every bit.
//
// Descriptor: an R x S image (rings x sectors, row-major: cell = ring * S + sector) of the maximum height.
//   per point (x, y, z), all three finite:
//     zh   = z + height_offset                      skip unless zh > 0
//     r    = sqrt(x * x + y * y)                    skip unless r < max_range
//     ring = (int)((r * (float)R) / max_range)      at most R - 1
//     a    = qm_atan2f(y, x) + QTR_PLACE_PI_F       in [0, 2 pi]
//     sec  = (int)((a * (float)S) / QTR_PLACE_TWO_PI_F)   at most S - 1 (the last bin is closed at 2 pi)
//     cell = max(cell, zh)                          an empty cell is 0
//   A maximum does not depend on the order of the points: the descriptor is a function of the point SET.
// Column norms: n2[j] = sum over rings 0 .. R-1, in that order, of d[r][j] * d[r][j], starting from 0.
// Distance of a query q to an entry c at column shift s (qtr_place_shift_distance):
//   for j = 0 .. S-1, in that order, with jc = (j + s) mod S:
//     den = sqrt(qn2[j] * cn2[jc])                  the column counts only if den > 0, i.e. both norms are non-zero
//                                                   (norms whose squared product underflows float32, below about 1e-11 m,
//                                                   count as zero)
//     dot = sum over rings 0 .. R-1, in that order, of q[r][j] * c[r][jc], starting from 0
//     t   = 1 - dot / den                           taken as 0 unless t > 0 (rounding can put the cosine just above 1)
//     sum = sum + t, cnt = cnt + 1
//   d(s) = sum / (float)cnt, or 1 when no column counted.  d(s) >= 0 always; a descriptor against itself gives exactly 0
//   at shift 0 (dot == n2 and sqrt(n2 * n2) == n2).
// distance = min over s of d(s), ties to the lowest s (qtr_place_key orders (distance bits, s) as one integer: the bit
// pattern of a non-negative float is monotone).  yaw = qtr_place_yaw(shift, S): shift * 2 pi / S wrapped to (-pi, pi], the
// yaw of the transform that maps the QUERY into the ENTRY's frame — the entry's image is the query's moved `shift` columns
// towards larger azimuth.
#pragma once
#include "qtr_math.h"

#define QTR_PLACE_PI_F 3.14159274f      // (float)pi
#define QTR_PLACE_TWO_PI_F 6.28318548f  // (float)(2 pi)
#define QTR_PLACE_MAX_RINGS 32
#define QTR_PLACE_MAX_SECTORS 64
#define QTR_PLACE_MAX_K 64

// the cell of one point, or -1 when the point takes no part; *zh_out: the value the cell is maximised with
QM_HD int qtr_place_cell(float x, float y, float z, int R, int S, float max_range, float height_offset, float* zh_out) {
  if ((x - x) != 0.0f || (y - y) != 0.0f || (z - z) != 0.0f) return -1;  // NaN or infinite
  const float zh = z + height_offset;
  if (!(zh > 0.0f)) return -1;
  const float r = sqrtf(x * x + y * y);
  if (!(r < max_range)) return -1;
  int ring = (int)((r * (float)R) / max_range);
  if (ring > R - 1) ring = R - 1;
  const float a = qm_atan2f(y, x) + QTR_PLACE_PI_F;
  int sec = (int)((a * (float)S) / QTR_PLACE_TWO_PI_F);
  if (sec > S - 1) sec = S - 1;
  if (sec < 0) sec = 0;
  *zh_out = zh;
  return ring * S + sec;
}

// squared norm of column j of an R x S image
QM_HD float qtr_place_colnorm2(const float* d, int R, int S, int j) {
  float acc = 0.0f;
  for (int r = 0; r < R; ++r) acc = acc + d[r * S + j] * d[r * S + j];
  return acc;
}

// d(s): q / c are R x S images, qn2 / cn2 their S squared column norms
QM_HD float qtr_place_shift_distance(const float* q, const float* qn2, const float* c, const float* cn2, int R, int S, int s) {
  float sum = 0.0f;
  int cnt = 0;
  for (int j = 0; j < S; ++j) {
    const float a2 = qn2[j];
    if (!(a2 > 0.0f)) continue;
    int jc = j + s;
    if (jc >= S) jc -= S;
    const float den = sqrtf(a2 * cn2[jc]);
    float dot = 0.0f;
    for (int r = 0; r < R; ++r) dot = dot + q[r * S + j] * c[r * S + jc];
    float t = 1.0f - dot / den;
    if (!(t > 0.0f)) t = 0.0f;
    if (den > 0.0f) {
      sum = sum + t;
      cnt = cnt + 1;
    }
  }
  return cnt > 0 ? sum / (float)cnt : 1.0f;
}

// (distance, low word) as one ascending integer key; distance >= 0
QM_HD uint64_t qtr_place_key(float distance, uint32_t low) {
  union {
    float f;
    uint32_t u;
  } b;
  b.f = distance;
  return ((uint64_t)b.u << 32) | (uint64_t)low;
}

QM_HD float qtr_place_yaw(int shift, int S) {
  float y = ((float)shift * QTR_PLACE_TWO_PI_F) / (float)S;
  if (y > QTR_PLACE_PI_F) y = y - QTR_PLACE_TWO_PI_F;
  return y;
}
