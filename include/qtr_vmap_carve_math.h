// qtr_vmap_carve_math.h — the contract of the voxel map's visibility carving, shared by the gfx950 kernels
// (quatro_amd/csrc/voxelmap_carve.hip), the g++ harness of the tests (tests/vmap_carve_ref) and their numpy restatement, on
// top of qtr_vmap_math.h, which stays as it is.  Plain C, binary64, + - * / sqrt floor only, evaluated in the order written
// (every side compiles with -ffp-contract=off); angles are qm_atan2d of qtr_math.h.  This header is the definition.
//
//   image    one per scan, in the scan's OWN frame (no pose), rows x cols pixels of uint32, QTR_CARVE_EMPTY where nothing
//            fell.  A point (x, y, z), taken to binary64:  h2 = x x + y y,  h = sqrt(h2),  r = sqrt(h2 + z z),
//            el = qm_atan2d(z, h),  az = qm_atan2d(y, x),
//              row = floor(((fov_up - el) rows) / (fov_up - fov_down))       the product first, then ONE division
//              col = floor(((az + pi) cols) / (2 pi))                        likewise; col == cols (az = pi) folds to 0
//            with fov_up = (fov_up_deg pi) / 180, fov_down likewise.  The point is skipped when a coordinate is not finite,
//            when x = y = 0 (the z axis has no azimuth), when row lies outside [0, rows), or when r lies outside
//            [min_range, max_range].  The pixel keeps the MINIMUM of (float) r, rounded once: the minimum of the floats' bit
//            patterns, which for positive floats is the minimum of the floats, whatever the order of the points.
//   verdict  of a voxel with mean mu (the QTR_VMAP_RECORDS mean, as stored) against the scan taken at pose P (rows 0 - 2 of
//            16 row-major doubles, scan frame -> map frame):  d = mu - t,  p = R^T d  ((R0j d0 + R1j d1) + R2j d2), and
//            r_v, row, col of p by the rule above.  NO VOTE if p is skipped by that rule or the centre pixel is empty.
//            Otherwise the limit is  (r_v + margin_abs) + margin_rel r_v  and the scan votes SEEN THROUGH iff no filled pixel
//            of the (2 w + 1)^2 window around (row, col) holds a range <= limit: columns wrap, rows outside the image and
//            empty pixels are neutral, the stored float is compared as a double, equality keeps the voxel (OCCUPIED).
//   carve    a voxel leaves the map iff its SEEN THROUGH votes over the call's scans reach min_votes.
//
// The rule needs the centre pixel filled, so an image FINER than the sensor carves nothing where the sensor left holes: a
// quarter of the pixels of a 64 x 1800 image of a 64 x 1800 sweep with noise are empty.  Choose rows x cols no finer than
// the sensor (the defaults, 64 x 1024 over [-25.5, 2.5] degrees, suit a 64-beam sweep of 1800 or more columns).  A window
// of 0 removes ground at grazing incidence, where neighbouring beams differ by metres: keep w >= 1.
#pragma once
#include "qtr_vmap_math.h"

#define QTR_CARVE_EMPTY 0xffffffffu
#define QTR_CARVE_MAX_ROWS 256
#define QTR_CARVE_MIN_COLS 8  // above 2 w + 1 for every window: a window never meets a pixel twice
#define QTR_CARVE_MAX_COLS 4096
#define QTR_CARVE_MAX_WINDOW 3
#define QTR_CARVE_MAX_SCANS 64

#define QTR_CARVE_NO_VOTE 0
#define QTR_CARVE_OCCUPIED 1
#define QTR_CARVE_SEEN_THROUGH 2

// why a set of parameters is refused (qtr_carve_cfg_make)
#define QTR_CARVE_OK 0
#define QTR_CARVE_BAD_ROWS 1
#define QTR_CARVE_BAD_COLS 2
#define QTR_CARVE_BAD_FOV 3
#define QTR_CARVE_BAD_WINDOW 4
#define QTR_CARVE_BAD_VOTES 5
#define QTR_CARVE_BAD_MARGIN 6
#define QTR_CARVE_BAD_RANGE 7

typedef struct QtrCarveCfg {
  int rows, cols, window, min_votes;
  double fov_up, fov_span;  // radians: the top of the image and fov_up - fov_down
  double margin_abs, margin_rel, min_range, max_range;
} QtrCarveCfg;

// The checked parameters of a call with n_scans scans on a map of side voxel_size (margin_abs = 0 means voxel_size).
QM_HD int qtr_carve_cfg_make(int rows, int cols, double fov_up_deg, double fov_down_deg, int window, int min_votes,
                             double margin_abs, double margin_rel, double min_range, double max_range, int n_scans,
                             double voxel_size, QtrCarveCfg* c) {
  if (rows < 1 || rows > QTR_CARVE_MAX_ROWS) return QTR_CARVE_BAD_ROWS;
  if (cols < QTR_CARVE_MIN_COLS || cols > QTR_CARVE_MAX_COLS) return QTR_CARVE_BAD_COLS;
  if (!qtr_vmap_finite(fov_up_deg) || !qtr_vmap_finite(fov_down_deg) || !(fov_up_deg > fov_down_deg)) return QTR_CARVE_BAD_FOV;
  if (window < 0 || window > QTR_CARVE_MAX_WINDOW) return QTR_CARVE_BAD_WINDOW;
  if (min_votes < 1 || min_votes > n_scans) return QTR_CARVE_BAD_VOTES;
  if (!qtr_vmap_finite(margin_abs) || !(margin_abs >= 0.0) || !qtr_vmap_finite(margin_rel) || !(margin_rel >= 0.0))
    return QTR_CARVE_BAD_MARGIN;
  if (!qtr_vmap_finite(min_range) || !qtr_vmap_finite(max_range) || !(min_range < max_range)) return QTR_CARVE_BAD_RANGE;
  c->rows = rows;
  c->cols = cols;
  c->window = window;
  c->min_votes = min_votes;
  c->fov_up = (fov_up_deg * QM_PI) / 180.0;
  c->fov_span = c->fov_up - (fov_down_deg * QM_PI) / 180.0;
  if (!(c->fov_span > 0.0)) return QTR_CARVE_BAD_FOV;  // (two angles an ulp apart)
  c->margin_abs = margin_abs == 0.0 ? voxel_size : margin_abs;
  c->margin_rel = margin_rel;
  c->min_range = min_range;
  c->max_range = max_range;
  return QTR_CARVE_OK;
}

// range and pixel of a point in the scan's frame; false: the point is skipped
QM_HD bool qtr_carve_pixel(const QtrCarveCfg* c, double x, double y, double z, double* r, int* row, int* col) {
  if (!(qtr_vmap_finite(x) && qtr_vmap_finite(y) && qtr_vmap_finite(z))) return false;
  if (x == 0.0 && y == 0.0) return false;
  const double h2 = x * x + y * y;
  const double h = sqrt(h2);
  const double rr = sqrt(h2 + z * z);
  const double el = qm_atan2d(z, h);
  const double az = qm_atan2d(y, x);
  const double fr = floor(((c->fov_up - el) * (double)c->rows) / c->fov_span);
  if (!(fr >= 0.0 && fr < (double)c->rows)) return false;
  const double fc = floor(((az + QM_PI) * (double)c->cols) / (2.0 * QM_PI));
  if (!(fc >= 0.0 && fc <= (double)c->cols)) return false;  // (never for a finite point: az lies in [-pi, pi])
  if (!(rr >= c->min_range && rr <= c->max_range)) return false;
  *r = rr;
  *row = (int)fr;
  *col = (int)fc == c->cols ? 0 : (int)fc;
  return true;
}

// what a pixel stores for range r (r >= 0: the pattern orders as the float does)
QM_HD unsigned qtr_carve_bits(double r) {
  union {
    float f;
    unsigned u;
  } v;
  v.f = (float)r;
  return v.u;
}

QM_HD double qtr_carve_range(unsigned bits) {
  union {
    float f;
    unsigned u;
  } v;
  v.u = bits;
  return (double)v.f;
}

// a voxel mean in the frame of the scan taken at P: p = R^T (mu - t)
QM_HD void qtr_carve_to_scan(const double* P, const double* mu, double* p) {
  const double d0 = mu[0] - P[3], d1 = mu[1] - P[7], d2 = mu[2] - P[11];
  p[0] = (P[0] * d0 + P[4] * d1) + P[8] * d2;
  p[1] = (P[1] * d0 + P[5] * d1) + P[9] * d2;
  p[2] = (P[2] * d0 + P[6] * d1) + P[10] * d2;
}

// the vote of the scan at P, whose image is img[rows x cols], on the voxel with mean mu
QM_HD int qtr_carve_verdict(const QtrCarveCfg* c, const double* P, const double* mu, const unsigned* img) {
  double p[3], rv = 0.0;
  int row = 0, col = 0;
  qtr_carve_to_scan(P, mu, p);
  if (!qtr_carve_pixel(c, p[0], p[1], p[2], &rv, &row, &col)) return QTR_CARVE_NO_VOTE;
  if (img[row * c->cols + col] == QTR_CARVE_EMPTY) return QTR_CARVE_NO_VOTE;
  const double limit = (rv + c->margin_abs) + c->margin_rel * rv;
  for (int dr = -c->window; dr <= c->window; ++dr) {
    const int rr = row + dr;
    if (rr < 0 || rr >= c->rows) continue;
    for (int dc = -c->window; dc <= c->window; ++dc) {
      int cc = col + dc;
      if (cc < 0) cc += c->cols;
      if (cc >= c->cols) cc -= c->cols;
      const unsigned v = img[rr * c->cols + cc];
      if (v == QTR_CARVE_EMPTY) continue;
      if (qtr_carve_range(v) <= limit) return QTR_CARVE_OCCUPIED;
    }
  }
  return QTR_CARVE_SEEN_THROUGH;
}
