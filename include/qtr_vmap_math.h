// qtr_vmap_math.h — the arithmetic of the persistent Gaussian voxel map, shared by the gfx950 kernels
// (quatro_amd/csrc/voxelmap.hip) and the host restatement of the tests (g++), in the style of qtr_icp_math.h: binary64
// + - * / sqrt only, evaluated in the order written (both sides compile with -ffp-contract=off), so host and device agree
// bit for bit.  qtr_icp_transform, qtr_icp_finite3, qtr_icp_normal_ok, qtr_icp_voxel_finish, qtr_icp_vgicp_terms,
// qtr_icp_step and the fold functions are qtr_icp_math.h's, unchanged.
//
//   grid     side c = the map's voxel_size; voxel coordinate of a world coordinate X: i = floor(X / c) as a double, valid
//            only for -2^20 <= i < 2^20 (compared as double before any cast: NaN and huge values fail).  No bounding box
//            and no origin: the grid depends on nothing that was inserted.
//   key      ((kz 2^21) + ky) 2^21 + kx with k = i + 2^20.
//   member   of an insert (point p, normal a, pose P: rows 0 - 2 of 16 row-major doubles): p finite, a passes
//            qtr_icp_normal_ok, X = qtr_icp_transform(P, p) — kept in binary64, NOT rounded to float — finite, all three
//            voxel coordinates of X valid.  World normal m = R (a / |a|): normalised first, then rotated, in the
//            association qtr_icp_vgicp_terms uses for its m; no second normalisation.  Everything else is silently not a
//            member.
//   record   n = members, acc[9] = sum X (3) and sum m m^T (00 01 02 11 12 22), folded from 0.0 over the inserts in call
//            order and inside an insert in ascending point index (qtr_vmap_add); an insert into an existing voxel continues
//            the stored acc.  The finished record is qtr_icp_voxel_finish(acc, n, 0, .).  n = 0: the voxel does not exist.
//   match    of a source point p with normal a under T: p finite, a passes qtr_icp_normal_ok, q = T p, all voxel
//            coordinates of q valid, the voxel exists.  No distance test, no clamping.  Terms: qtr_icp_vgicp_terms; fold,
//            solve, increment and stopping: method 3's.
#pragma once
#include "qtr_icp_math.h"

#define QTR_VMAP_HALF 1048576.0             // 2^20: voxel coordinates lie in [-2^20, 2^20)
#define QTR_VMAP_EMPTY 0xffffffffffffffffULL  // no key (keys are < 2^63)

QM_HD bool qtr_vmap_finite(double x) { return (x - x) == 0.0; }

// voxel coordinate of one world coordinate; false: outside the grid (or not a number)
QM_HD bool qtr_vmap_coord(double x, double c, int* i) {
  const double f = floor(x / c);
  if (!(f >= -QTR_VMAP_HALF && f < QTR_VMAP_HALF)) return false;
  *i = (int)f;
  return true;
}

QM_HD unsigned long long qtr_vmap_key(int ix, int iy, int iz) {
  const unsigned long long kx = (unsigned long long)(ix + 1048576), ky = (unsigned long long)(iy + 1048576),
                           kz = (unsigned long long)(iz + 1048576);
  return ((kz << 21) + ky) * 2097152ULL + kx;
}

QM_HD void qtr_vmap_key_coords(unsigned long long key, int* c /* [3] */) {
  c[0] = (int)(key & 2097151ULL) - 1048576;
  c[1] = (int)((key >> 21) & 2097151ULL) - 1048576;
  c[2] = (int)((key >> 42) & 2097151ULL) - 1048576;
}

// the key of a world position; false: some coordinate lies outside the grid
QM_HD bool qtr_vmap_key_of(const double* X, double c, unsigned long long* key) {
  int i[3];
  for (int a = 0; a < 3; ++a)
    if (!qtr_vmap_coord(X[a], c, &i[a])) return false;
  *key = qtr_vmap_key(i[0], i[1], i[2]);
  return true;
}

// where a key's probe chain starts in a table of mask + 1 slots (a power of two); the chain goes on at (s + 1) & mask.
// (the finaliser of splitmix64; nothing observable depends on it)
QM_HD unsigned long long qtr_vmap_hash(unsigned long long key, unsigned long long mask) {
  unsigned long long z = key + 0x9e3779b97f4a7c15ULL;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
  z = z ^ (z >> 31);
  return z & mask;
}

// the member test of an insert: true, and its world position X and world normal m, for a member
QM_HD bool qtr_vmap_member(const double* P, float px, float py, float pz, float ax, float ay, float az, double c, double* X,
                           double* m, unsigned long long* key) {
  if (!qtr_icp_finite3(px, py, pz) || !qtr_icp_normal_ok(ax, ay, az)) return false;
  qtr_icp_transform(P, px, py, pz, X);
  if (!(qtr_vmap_finite(X[0]) && qtr_vmap_finite(X[1]) && qtr_vmap_finite(X[2]))) return false;
  if (!qtr_vmap_key_of(X, c, key)) return false;
  double a0 = (double)ax, a1 = (double)ay, a2 = (double)az;
  const double la = sqrt((a0 * a0 + a1 * a1) + a2 * a2);
  a0 = a0 / la;
  a1 = a1 / la;
  a2 = a2 / la;
  m[0] = (P[0] * a0 + P[1] * a1) + P[2] * a2;
  m[1] = (P[4] * a0 + P[5] * a1) + P[6] * a2;
  m[2] = (P[8] * a0 + P[9] * a1) + P[10] * a2;
  return true;
}

// one member into the running sums acc[9] (qtr_icp_voxel_add's places, from binary64 inputs)
QM_HD void qtr_vmap_add(double* acc, const double* X, const double* m) {
  acc[0] = acc[0] + X[0];
  acc[1] = acc[1] + X[1];
  acc[2] = acc[2] + X[2];
  acc[3] = acc[3] + m[0] * m[0];
  acc[4] = acc[4] + m[0] * m[1];
  acc[5] = acc[5] + m[0] * m[2];
  acc[6] = acc[6] + m[1] * m[1];
  acc[7] = acc[7] + m[1] * m[2];
  acc[8] = acc[8] + m[2] * m[2];
}

// the source side of a match: true, and q = T p and the key of its voxel, when the point can have a correspondence
QM_HD bool qtr_vmap_query(const double* T, float px, float py, float pz, float ax, float ay, float az, double c, double* q,
                          unsigned long long* key) {
  if (!qtr_icp_finite3(px, py, pz) || !qtr_icp_normal_ok(ax, ay, az)) return false;
  qtr_icp_transform(T, px, py, pz, q);
  return qtr_vmap_key_of(q, c, key);
}
