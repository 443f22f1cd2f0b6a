// vmap_ref.cpp — host restatement of the device voxel map (quatro_amd/csrc/voxelmap.hip) for the tests: the same
// include/qtr_vmap_math.h arithmetic (grid rule, member test, the running fold, qtr_icp_voxel_finish, qtr_icp_vgicp_terms,
// qtr_icp_step) and the same fixed-shape sums as the device iteration.  The table is a std::map keyed by the contract's
// key, so nothing of the device's hashing is restated; the hash and the key are exported for the tests that build crowded
// tables.  Built by the tests with g++ -O2 -ffp-contract=off -shared -fPIC.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <vector>

#include "qtr_vmap_math.h"

namespace {
struct Rec {
  int n = 0;
  double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
};
struct RefMap {
  double side = 1.0;
  int capacity = 0;
  std::map<unsigned long long, Rec> vox;
};
const double kIdentity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
}  // namespace

extern "C" {

void* vmap_ref_new(double side, int capacity) {
  RefMap* m = new RefMap();
  m->side = side;
  m->capacity = capacity;
  return m;
}
void vmap_ref_free(void* p) { delete (RefMap*)p; }
void vmap_ref_clear(void* p) { ((RefMap*)p)->vox.clear(); }
int vmap_ref_size(void* p) { return (int)((RefMap*)p)->vox.size(); }

unsigned long long vmap_ref_hash(unsigned long long key, unsigned long long mask) { return qtr_vmap_hash(key, mask); }
unsigned long long vmap_ref_key(int ix, int iy, int iz) { return qtr_vmap_key(ix, iy, iz); }
// 1 and *i: the voxel coordinate of x on a grid of side c; 0: outside
int vmap_ref_coord(double x, double c, int* i) { return qtr_vmap_coord(x, c, i) ? 1 : 0; }

// info: n_points, n_members, n_new_voxels, n_touched_voxels.  Returns 0, or 3 (QTR_ERR_CAPACITY) with the map untouched.
int vmap_ref_insert(void* p, const float* pts4, const float* nrm4, int n, const double* pose, int* info) {
  RefMap* m = (RefMap*)p;
  const double* P = pose ? pose : kIdentity;
  std::map<unsigned long long, Rec> add;  // this call's own fold, continued from the stored records
  int members = 0, fresh = 0;
  for (int i = 0; i < n; ++i) {  // ascending point index
    double X[3], w[3];
    unsigned long long key = 0;
    if (!qtr_vmap_member(P, pts4[4 * i], pts4[4 * i + 1], pts4[4 * i + 2], nrm4[4 * i], nrm4[4 * i + 1], nrm4[4 * i + 2],
                         m->side, X, w, &key))
      continue;
    auto it = add.find(key);
    if (it == add.end()) {
      auto old = m->vox.find(key);
      if (old == m->vox.end()) ++fresh;
      it = add.emplace(key, old == m->vox.end() ? Rec() : old->second).first;
    }
    qtr_vmap_add(it->second.acc, X, w);
    it->second.n += 1;
    ++members;
  }
  info[0] = n;
  info[1] = members;
  info[2] = fresh;
  info[3] = (int)add.size();
  if ((long long)m->vox.size() + fresh > (long long)m->capacity) return 3;
  for (auto& kv : add) m->vox[kv.first] = kv.second;
  return 0;
}

// every section in ascending key order; any pointer may be null
void vmap_ref_fetch(void* p, int* coords, int* count, double* sums, double* records, float* cloud) {
  RefMap* m = (RefMap*)p;
  size_t j = 0;
  for (auto& kv : m->vox) {
    QtrIcpVoxel vx;
    qtr_icp_voxel_finish(kv.second.acc, kv.second.n, 0, &vx);
    if (coords) qtr_vmap_key_coords(kv.first, coords + 3 * j);
    if (count) count[j] = kv.second.n;
    if (sums) memcpy(sums + 9 * j, kv.second.acc, 72);
    if (records) {
      for (int a = 0; a < 3; ++a) records[9 * j + a] = vx.mu[a];
      for (int a = 0; a < 6; ++a) records[9 * j + 3 + a] = vx.C[a];
    }
    if (cloud) {
      for (int a = 0; a < 3; ++a) cloud[4 * j + a] = (float)vx.mu[a];
      cloud[4 * j + 3] = (float)vx.n;
    }
    ++j;
  }
}

// the registration loop: method 3's with the map lookup.  corr_at (ns or null): 0 matched / -1 none at evaluation corr_iter
// (< 0: the last one evaluated).
void vmap_ref_register(void* p, const float* src4, int ns, const float* src_nrm4, const double* guess, double teps, double feps,
                       int max_iter, int min_corr, double* T_out, int* info /* iterations, reason, valid, converged, n_corr */,
                       double* fit_rmse /* 2 */, double* trace /* max_iter x 18 */, int* corr_at, int corr_iter) {
  RefMap* m = (RefMap*)p;
  QtrIcpCfg cfg;
  cfg.max_d2 = m->side * m->side;
  cfg.trans_eps = teps;
  cfg.fit_eps = feps;
  cfg.max_iterations = max_iter;
  cfg.method = 3;
  cfg.min_corr = min_corr > 0 ? min_corr : 4;
  cfg.pad = 0;
  double g[16];
  for (int k = 0; k < 16; ++k) g[k] = k < 12 ? guess[k] : kIdentity[k];  // (row 3 is taken as 0 0 0 1)
  QtrIcpState st;
  qtr_icp_init(&st, g);
  st.reason = ns > 0 ? QTR_ICP_RUNNING : QTR_ICP_STOP_TOO_FEW;
  std::map<unsigned long long, QtrIcpVoxel> rec;
  for (auto& kv : m->vox) qtr_icp_voxel_finish(kv.second.acc, kv.second.n, 0, &rec[kv.first]);
  const int nchunk = (ns + QTR_ICP_CHUNK - 1) / QTR_ICP_CHUNK;
  std::vector<double> terms((size_t)nchunk * QTR_ICP_CHUNK * QTR_ICP_NT, 0.0);
  for (int eval = 0; st.reason == QTR_ICP_RUNNING; ++eval) {
    std::fill(terms.begin(), terms.end(), 0.0);
    for (int i = 0; i < ns; ++i) {
      const float* s = src4 + 4 * i;
      const float* a = src_nrm4 + 4 * i;
      int best = -1;
      double q[3];
      unsigned long long key = 0;
      if (qtr_vmap_query(st.T, s[0], s[1], s[2], a[0], a[1], a[2], m->side, q, &key)) {
        auto it = rec.find(key);
        if (it != rec.end() && it->second.n > 0) {
          best = 0;
          qtr_icp_vgicp_terms(st.T, q, a[0], a[1], a[2], &it->second, &terms[(size_t)i * QTR_ICP_NT]);
        }
      }
      if (corr_at && (eval == corr_iter || corr_iter < 0)) corr_at[i] = best;
    }
    double S[QTR_ICP_NT];
    for (int k = 0; k < QTR_ICP_NT; ++k) {
      double acc = 0.0;
      for (int c = 0; c < nchunk; ++c) {
        double w[4];
        for (int wv = 0; wv < 4; ++wv) {
          double p64[64];
          for (int l = 0; l < 64; ++l) p64[l] = terms[((size_t)c * QTR_ICP_CHUNK + wv * 64 + l) * QTR_ICP_NT + k];
          w[wv] = qtr_icp_fold64(p64);
        }
        const double part = qtr_icp_chunk_sum(w);
        acc = (c == 0) ? part : acc + part;
      }
      S[k] = k <= QTR_ICP_T_W ? acc : 0.0;
    }
    double* tr = trace ? trace + (size_t)st.iterations * 18 : nullptr;
    qtr_icp_step(&cfg, S, &st, tr);
  }
  for (int k = 0; k < 16; ++k) T_out[k] = st.T[k];
  info[0] = st.iterations;
  info[1] = st.reason;
  info[2] = st.valid;
  info[3] = st.converged;
  info[4] = st.n_corr;
  fit_rmse[0] = st.fitness;
  fit_rmse[1] = st.rmse;
}

}  // extern "C"
