// vmap_carve_ref.cpp — include/qtr_vmap_carve_math.h under g++ for the tests: the header's own functions over arrays, nothing
// restated.  The numpy restatement (tests/vmap_carve_restate.py) is compared with what these return, bit for bit.
// Built by the tests with g++ -O2 -ffp-contract=off -shared -fPIC.
#include <cstring>
#include <vector>

#include "qtr_vmap_carve_math.h"

extern "C" {

// prm: rows, cols, window, min_votes;  dprm: fov_up_deg, fov_down_deg, margin_abs, margin_rel, min_range, max_range.
// Returns the header's refusal code (0: accepted) and the checked parameters in *cfg (sizeof(QtrCarveCfg) bytes).
int carve_ref_cfg(const int* prm, const double* dprm, int n_scans, double voxel_size, void* cfg) {
  QtrCarveCfg c;
  memset(&c, 0, sizeof(c));
  const int why = qtr_carve_cfg_make(prm[0], prm[1], dprm[0], dprm[1], prm[2], prm[3], dprm[2], dprm[3], dprm[4], dprm[5], n_scans,
                                     voxel_size, &c);
  memcpy(cfg, &c, sizeof(c));
  return why;
}
int carve_ref_cfg_bytes(void) { return (int)sizeof(QtrCarveCfg); }

// per point of xyz (n x 3 doubles): ok[i] (0 skipped), r[i], row[i], col[i]
void carve_ref_pixels(const void* cfg, const double* xyz, int n, int* ok, double* r, int* row, int* col) {
  const QtrCarveCfg* c = (const QtrCarveCfg*)cfg;
  for (int i = 0; i < n; ++i) {
    r[i] = 0.0;
    row[i] = col[i] = -1;
    ok[i] = qtr_carve_pixel(c, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], &r[i], &row[i], &col[i]) ? 1 : 0;
  }
}

// the image (rows x cols, cleared here) of n float4 points
void carve_ref_image(const void* cfg, const float* xyz4, int n, unsigned* img) {
  const QtrCarveCfg* c = (const QtrCarveCfg*)cfg;
  for (int i = 0; i < c->rows * c->cols; ++i) img[i] = QTR_CARVE_EMPTY;
  for (int i = 0; i < n; ++i) {
    double r;
    int row, col;
    if (!qtr_carve_pixel(c, (double)xyz4[4 * i], (double)xyz4[4 * i + 1], (double)xyz4[4 * i + 2], &r, &row, &col)) continue;
    const unsigned b = qtr_carve_bits(r);
    unsigned* px = img + row * c->cols + col;
    if (b < *px) *px = b;
  }
}

// votes[v x B]: the verdict of scan b (pose: 16 doubles each, image: rows x cols each) on voxel v (mu: 3 doubles each)
void carve_ref_verdicts(const void* cfg, const double* poses16, const unsigned* imgs, int B, const double* mu, int nv, int* votes) {
  const QtrCarveCfg* c = (const QtrCarveCfg*)cfg;
  const size_t px = (size_t)c->rows * c->cols;
  for (int v = 0; v < nv; ++v)
    for (int b = 0; b < B; ++b) votes[(size_t)v * B + b] = qtr_carve_verdict(c, poses16 + 16 * (size_t)b, mu + 3 * (size_t)v, imgs + px * b);
}

}  // extern "C"
