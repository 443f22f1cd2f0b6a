// quatro_pgo.hpp — robust pose-graph optimisation over the process-wide handle of quatro_hip_cxx.hpp: from the edges (T,
// Omega) that registration and evaluation emit to corrected keyframe poses (qtr_pgo_optimize: Levenberg-Marquardt with the
// line process of Choi et al. 2015 over the uncertain edges, on the device).  Poses and transforms are row-major 4 x 4
// doubles — std::array<double, 16>, which an Eigen::Matrix<double, 4, 4, Eigen::RowMajor>::data() copies into — so the
// header needs neither Eigen nor pcl.  Host code only; link with -lquatro_hip.
#ifndef QUATRO_PGO_H
#define QUATRO_PGO_H

#include <array>
#include <vector>

#include "quatro_eval.hpp"

namespace quatro_hip {

using Pose = std::array<double, 16>;         // row-major 4 x 4, keyframe frame -> map frame
using Information = std::array<double, 36>;  // row-major 6 x 6, [omega | v] (qtr_eval_result::information)

inline qtr_pgo_params default_pgo_params(double line_process_weight = 0.0) {
  qtr_pgo_params p;
  qtr_default_pgo_params(&p);
  p.line_process_weight = line_process_weight;
  return p;
}

struct PgoOutcome {
  qtr_pgo_result result{};
  std::vector<Pose> poses;
  std::vector<double> weights;  // one per edge
  std::vector<int> pruned;      // uncertain edges whose weight fell below edge_prune_threshold
};

// poses: one per node; fixed: one flag per node or empty (node 0 is held); edge e: Z[e] maps keyframe src[e]'s frame into
// keyframe dst[e]'s frame, info[e] is its information matrix, uncertain[e] puts it under the line process (empty: none).
inline PgoOutcome optimize_pose_graph(const std::vector<Pose>& poses, const std::vector<unsigned char>& fixed,
                                      const std::vector<int>& src, const std::vector<int>& dst, const std::vector<Pose>& Z,
                                      const std::vector<Information>& info, const std::vector<unsigned char>& uncertain,
                                      const qtr_pgo_params& prm = default_pgo_params()) {
  const int N = (int)poses.size(), E = (int)src.size();
  if (dst.size() != src.size() || Z.size() != src.size() || info.size() != src.size() ||
      (!uncertain.empty() && uncertain.size() != src.size()) || (!fixed.empty() && fixed.size() != poses.size()))
    throw std::invalid_argument("optimize_pose_graph: array sizes do not agree");
  PgoOutcome out;
  out.poses.resize(poses.size());
  out.weights.resize(src.size());
  SlotLease lease;
  check(default_handle(),
        qtr_pgo_optimize(default_handle(), lease.slot, N, N ? poses[0].data() : nullptr, fixed.empty() ? nullptr : fixed.data(), E,
                         src.data(), dst.data(), E ? Z[0].data() : nullptr, E ? info[0].data() : nullptr,
                         uncertain.empty() ? nullptr : uncertain.data(), &prm, N ? out.poses[0].data() : nullptr,
                         out.weights.data(), &out.result));
  for (int e = 0; e < E; ++e)
    if (!uncertain.empty() && uncertain[e] && out.weights[e] < prm.edge_prune_threshold) out.pruned.push_back(e);
  return out;
}

// The graph a caller grows keyframe by keyframe.
class PoseGraph {
 public:
  int add_node(const Pose& pose, bool fixed = false) {
    poses_.push_back(pose);
    fixed_.push_back(fixed ? 1 : 0);
    return (int)poses_.size() - 1;
  }
  // T maps keyframe s's frame into keyframe t's frame: a registration's T with s the source and t the target
  int add_edge(int s, int t, const double T[16], const double information[36], bool uncertain = false) {
    if (s < 0 || t < 0 || s >= (int)poses_.size() || t >= (int)poses_.size() || s == t)
      throw std::invalid_argument("PoseGraph::add_edge: the edge does not join two different nodes");
    Pose z;
    Information w;
    for (int k = 0; k < 16; ++k) z[k] = T[k];
    for (int k = 0; k < 36; ++k) w[k] = information[k];
    src_.push_back(s);
    dst_.push_back(t);
    Z_.push_back(z);
    info_.push_back(w);
    uncertain_.push_back(uncertain ? 1 : 0);
    return (int)src_.size() - 1;
  }
  // an edge from an evaluation record: its T and its information
  int add_edge(int s, int t, const qtr_eval_result& e, bool uncertain = false) { return add_edge(s, t, e.T, e.information, uncertain); }
  // optimises and writes the poses back
  PgoOutcome optimize(const qtr_pgo_params& prm = default_pgo_params()) {
    bool any = false;
    for (unsigned char f : fixed_) any = any || f;
    PgoOutcome out = optimize_pose_graph(poses_, any ? fixed_ : std::vector<unsigned char>(), src_, dst_, Z_, info_, uncertain_, prm);
    poses_ = out.poses;
    return out;
  }
  const std::vector<Pose>& poses() const { return poses_; }
  int n_edges() const { return (int)src_.size(); }

 private:
  std::vector<Pose> poses_, Z_;
  std::vector<Information> info_;
  std::vector<unsigned char> fixed_, uncertain_;
  std::vector<int> src_, dst_;
};

}  // namespace quatro_hip
#endif  // QUATRO_PGO_H
