// capi.hip — implementation of the C ABI declared in include/quatro_hip.h.
// Host-side orchestration only: arenas, stream slots, staging copies, kernel sequencing.
#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <memory>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include "common.h"
#include "frontend.h"
#include "solver.h"
#include "stage_times.h"

struct RcclIdByValue {  // ncclUniqueId: passed by value to ncclCommInitRank
  char internal[QTR_COMM_ID_BYTES];
};

struct Slot {
  hipStream_t stream = nullptr;
  hipStream_t stream2 = nullptr;  // second cloud's front end runs concurrently
  hipEvent_t ev[EV_COUNT] = {};  // by name: SlotEvent (stage_times.h)
  hipEvent_t ev_vox = nullptr;    // voxel centroids complete (stream) -> Matcher means may start (stream2)
  // qtr_register_pair_corr: the back end of the caller's correspondences runs BESIDE the front end, on a third stream
  // (created on the slot's first such call: ensure_stream3)
  hipStream_t stream3 = nullptr;
  hipEvent_t ev_fork = nullptr;   // stream -> stream3 at the call's start: what the slot's stream held before it (no timing)
  hipEvent_t ev_join = nullptr;   // stream3 -> stream (no timing)
  void* solver_arena = nullptr;
  void* front_arena = nullptr;
  SolverBufs sb;
  FrontBufs fb;
  float4* in_src = nullptr;  // staging for host-resident inputs (max_points each)
  float4* in_tgt = nullptr;
  float4* m_src = nullptr;  // matched keypoints (max_corr each)
  float4* m_tgt = nullptr;
  int* pinned_i32 = nullptr;     // >= 64 ints
  qtr_result* pinned_res = nullptr;
  SegBufs seg;                   // range-image segmentation arena (allocated on first use)
  void* seg_arena = nullptr;
  ExactBufs exb;                 // exact clique search arena (allocated / grown on demand)
  void* ex_arena = nullptr;
  size_t ex_bytes = 0;
  PwBufs pwb;                    // ground segmentation arena (allocated on first use)
  void* pw_arena = nullptr;
  int* mail = nullptr;           // pinned host mailbox the phase-ending kernels write into (frontend.h MAIL_*)
  int seq = 0;                   // last sequence number handed to a phase-ending kernel
  unsigned long long exact_nodes = 0;  // search-tree nodes of the last PMC_EXACT run
  int exact_aborted = 0;               // 1: its time limit was hit (heuristic clique returned)
  TimesShape times_pending = TIMES_NONE;  // the shape of the last call: its stage times are read off the events lazily, by
                                          // the table of stage_times.h (compute_times)
  int nn_pending = 0;            // the nearest-neighbour events of the last match have not been added to the totals yet
  int nn_timed_last = 0;         // the last match had its event pairs attached (qtr_set_nn_event_stride)
  long long n_matches = 0;       // matches this slot has run
  float nn_dir_ms[2] = {0, 0};   // qtr_get_nn_dir_times: the two launches of the last timed match apart
  double nn_total_ms = 0;        // qtr_get_nn_totals
  long long nn_total_launches = 0;
  qtr_stage_times times = {};
  int last_L = 0;  // correspondences of the last solve
  int last_Wb = 0; // row stride (words) of the bit matrix it left behind (solver.h SolverView::Wb)
  int last_n = 0;  // points of the last qtr_fpfh
  int last_ns = 0, last_nt = 0;
  IcpBufs icp;                   // ICP arena (allocated on first use: icp.hip)
  EvalBufs eval;                 // evaluation arena (allocated on first use, grown on demand: eval.hip)
  PgoBufs pgo;                   // pose-graph optimisation arena (allocated on first use, grown on demand: pgo.hip)
  int reg_ready = 0;             // 1: the last call on this slot was a registration (qtr_refine_pair may use its clouds)
  double reg_T[16] = {};         // ... and its transform
  int icp_ns = 0, icp_iters = 0; // source points and updates of the last ICP call (debug ids)
  float icp_ms[2] = {0, 0};      // its grid build and its iterations, milliseconds
  PlaceScratch place;            // place-index scratch (allocated / grown on the first query or add: place.hip)
  KfGatherMember* merge_pin = nullptr;  // qtr_keyframe_merge: the member table in pinned host memory and its device copy
  KfGatherMember* merge_dev = nullptr;  // (QTR_SUBMAP_MAX_KEYFRAMES records each, allocated on the slot's first merge)
  void* deskew_pin = nullptr;  // deskew.hip: the knot table and the counters' read-back in pinned host memory, and the device
  void* deskew_dev = nullptr;  // copy of the table with the counters behind it (allocated on the slot's first deskew)
  struct VmapBatch* vbatch = nullptr;  // voxelmap_batch.hip: the slot's batch arena (allocated on the slot's first batch)
  struct VmapEval* veval = nullptr;    // voxelmap_eval.hip: the slot's map-evaluation arena (allocated on its first evaluation)
  struct PlaceBatch* pbatch = nullptr;  // place_batch.hip: the slot's grouped-query arena (allocated on its first batch)
  struct VmapCtBufs* vct = nullptr;     // voxelmap_ct.hip: staged times and the census counters (allocated on its first call)
};

// What a batch lane is waiting for: the mail of the chain it enqueued last (lane_poll).
enum LanePhase { LANE_IDLE = 0, LANE_VOXELS, LANE_MATCH, LANE_SOLVE, LANE_REFINE_BOXES, LANE_REFINE_ITER };

// One lane of the batch driver (qtr_submit_batch): a contiguous group of slots stepped through the three launch
// chains in lockstep on the first slot's streams.
struct Lane {
  int first_slot = 0, cap = 0;  // slots [first_slot, first_slot + cap)
  ViewStage stage;              // views of the group (pinned host + device)
  LanePhase phase = LANE_IDLE;
  int first_pair = 0, count = 0;  // pairs [first_pair, first_pair + count) of the job are on this lane
  std::vector<int> active;      // indices g (0..count) of the pairs still alive after each chain's checks
  std::vector<int> ns, nt, L;   // per g
  std::vector<int> corr_only;   // g of the pairs that bring their own correspondences and no scans: solver chain only
  std::vector<const float4*> csrc, ctgt;  // per g: the matched clouds the solver reads (slot's m_src / m_tgt or the caller's)
  std::vector<const float4*> raw_s, raw_t;  // per g: the clouds the voxel grid read (device pointers) and their sizes
  std::vector<int> Ps, Pt;
  bool long_lists = false;      // the chunk's FPFH chain included k2_neighbors_big
  // refine phases (qtr_submit_batch_refine): ln.active = the refining pairs
  std::vector<IcpView> iv;      // per position in ln.active: the pair's ICP view (its slot's arena, its clouds, its grid)
  const IcpView* ref_views = nullptr;  // the same views in the stage (device)
  int ref_it = 0, ref_nchunk = 1;      // iterations enqueued so far; the group's widest iteration launch
};
// A device-resident keyframe (keyframe.hip): one allocation sized to the scan, read-only after qtr_keyframe_create.
struct qtr_keyframe {
  qtr_handle* owner = nullptr;
  void* dev = nullptr;
  qtr_keyframe_info info = {};
};

// A place index (place.hip): capacity entries of `stride` floats, entries [0, size) filled.
struct qtr_place_index {
  qtr_handle* owner = nullptr;
  float* dev = nullptr;
  int stride = 0;
  qtr_place_index_info info = {};
};

struct qtr_voxel_map;  // (voxelmap.hip)

struct BatchJob {
  const qtr_pair_desc* pairs = nullptr;
  int B = 0, next = 0, done = 0;
  qtr_frontend_params fp;
  qtr_params prm;
  qtr_result* results = nullptr;
  int mem = QTR_MEM_HOST;
  bool active = false;
  std::vector<unsigned char> finished;  // per pair: its record is final (result or per-pair failure)
  bool refine = false;                  // qtr_submit_batch_refine: the lanes refine their pairs after the solver chain
  qtr_icp_params icp;
  qtr_icp_result* refined = nullptr;
  std::vector<unsigned char> ref_state; // per pair: 0 not refined, 1 refinement under way, 2 refined record final
  // qtr_submit_batch_keyframes: the pairs travel through the lanes as pair descriptors whose scan pointers are the two
  // qtr_keyframe objects and whose sizes are their voxel counts (`pairs` points at this copy); the lanes load the keyframes
  // into the slots where a raw-scan job runs the voxel grid and the FPFH chain
  bool kf = false;
  std::vector<qtr_pair_desc> kf_shadow;
};

struct qtr_handle {
  int device = 0;
  qtr_limits lim;
  std::vector<Slot> slots;
  std::vector<Lane> lanes;
  BatchJob job;
  void* comm = nullptr;        // ncclComm_t of this rank (qtr_comm_init)
  int comm_rank = 0, comm_world = 1;
  void* comm_buf = nullptr;    // device staging of the gather
  size_t comm_bytes = 0;
  std::atomic<int> solves_in_flight{0};  // back-end chains enqueued and not yet read back (slot calls from several threads)
  int spin_wait = 1;  // QTR_HOST_WAIT=block turns the mailbox polling off
  bool pre_on = false;      // qtr_set_batch_preprocess: the batched entry takes RAW sweeps (ground removal + range-image
  qtr_pw_params pre_pw;     // segmentation in front of the voxel grid)
  qtr_ip_params pre_ip;
  std::atomic<bool> long_lists{false};  // some cloud of the whole-path entry points had a point with more than QTR_KMAX
                            // neighbours: from then on their FPFH chains include k2_neighbors_big (lists_verdict); written
                            // by whichever slot call meets such a cloud first (calls from several threads)
  // LIVE host threads that have run a back-end chain on this handle (InFlight): the block outlives the handle as long as a
  // thread still holds it, so a thread that ends after qtr_destroy can still take itself off the count
  struct Callers {
    std::atomic<int> live{0};
  };
  std::shared_ptr<Callers> callers = std::make_shared<Callers>();
  std::mutex share_mu;                 // guards share_val / share_gen
  int share_val = 1, share_gen = 0;    // the share in force and how often it has changed
  std::atomic<int> gen_inflight[4] = {};  // chains in flight per generation of the share (gen & 3)
  unsigned long long uid = 0;     // process-unique id of this handle (a thread remembers the handle it registered with)
  int stage_events = 1;  // QTR_STAGE_EVENTS=0: only the first/last event of a call are recorded (stage times read 0)
  int corr_overlap = 1;  // QTR_CORR_OVERLAP=0: qtr_register_pair_corr runs its back end BEHIND the front end, as before
  int nn_event_stride = 1;  // every n-th match of a slot carries the nearest-neighbour event pairs (0: none)
  int icp_block = 0;  // QTR_ICP_BLOCK=n: ICP launches enqueued between two read-backs of the stop flag (0: all at once)
  std::mutex kf_mu;                    // guards `keyframes` (qtr_keyframe_create / _destroy from several threads)
  std::vector<qtr_keyframe*> keyframes;  // the live keyframes of this handle: qtr_destroy frees what the caller forgot
  std::vector<qtr_place_index*> place_indexes;  // the live place indexes, likewise (under kf_mu)
  std::vector<qtr_voxel_map*> voxel_maps;       // the live voxel maps, likewise (voxelmap.hip)
  char err[512];
};

static std::atomic<unsigned long long> g_handle_uid{0};
static void vmap_free_all(qtr_handle* h);  // (voxelmap.hip)
static void vmap_batch_free(Slot& s);      // (voxelmap_batch.hip)
static void vmap_eval_free(Slot& s);       // (voxelmap_eval.hip)
static void place_batch_free(Slot& s);     // (place_batch.hip)
static void vmap_ct_free(Slot& s);         // (voxelmap_ct.hip)

#define QTR_TRY(expr)                  \
  do {                                 \
    const int rc_ = (expr);            \
    if (rc_ != QTR_OK) return rc_;     \
  } while (0)

// ---- RCCL, opened at run time (the soname torch ships resolves to the copy that is already loaded)
struct RcclApi {
  void* lib = nullptr;
  int (*GetUniqueId)(void*) = nullptr;
  int (*CommInitRank)(void**, int, RcclIdByValue, int) = nullptr;
  int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
};
static RcclApi* rccl_api(char* err, size_t errn) {
  static RcclApi api;
  static int state = 0;  // 0 untried, 1 ok, -1 failed
  static char why[256] = "symbols missing";  // dlerror() is read ONCE per failure (a second call returns NULL)
  if (state == 0) {
    // QTR_RCCL_LIB: a site's own RCCL build, tried first (tests/test_gpu_multi.py points it at a transport double so
    // that several processes sharing one GPU can run the gather end to end)
    const char* names[] = {getenv("QTR_RCCL_LIB"), "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char* n : names) {
      if (api.lib) break;
      if (!n || !*n) continue;
      api.lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
      if (!api.lib) {
        const char* e = dlerror();
        if (e) snprintf(why, sizeof(why), "%s", e);
      }
    }
    if (api.lib) {
      snprintf(why, sizeof(why), "symbols missing");
      api.GetUniqueId = (int (*)(void*))dlsym(api.lib, "ncclGetUniqueId");
      api.CommInitRank = (int (*)(void**, int, RcclIdByValue, int))dlsym(api.lib, "ncclCommInitRank");
      api.AllGather = (int (*)(const void*, void*, size_t, int, void*, hipStream_t))dlsym(api.lib, "ncclAllGather");
      api.CommDestroy = (int (*)(void*))dlsym(api.lib, "ncclCommDestroy");
      api.GetErrorString = (const char* (*)(int))dlsym(api.lib, "ncclGetErrorString");
      const char* e = dlerror();
      if (e) snprintf(why, sizeof(why), "%s", e);
    }
    state = (api.lib && api.GetUniqueId && api.CommInitRank && api.AllGather && api.CommDestroy) ? 1 : -1;
  }
  if (state != 1) {
    if (err) snprintf(err, errn, "librccl could not be opened (%s)", why);
    return nullptr;
  }
  return &api;
}

extern "C" {

int qtr_comm_unique_id(char id[QTR_COMM_ID_BYTES]) {
  RcclApi* a = rccl_api(nullptr, 0);
  if (!a || !id) return QTR_ERR_HIP;
  return a->GetUniqueId(id) == 0 ? QTR_OK : QTR_ERR_HIP;
}

int qtr_comm_init(qtr_handle* h, const char id[QTR_COMM_ID_BYTES], int rank, int world) {
  if (!h || !id || world < 1 || rank < 0 || rank >= world) return QTR_ERR_BAD_ARG;
  RcclApi* a = rccl_api(h->err, sizeof(h->err));
  if (!a) return QTR_ERR_HIP;
  QTR_HIP_TRY(h, hipSetDevice(h->device));
  qtr_comm_destroy(h);
  RcclIdByValue v;
  memcpy(v.internal, id, QTR_COMM_ID_BYTES);
  const int rc = a->CommInitRank(&h->comm, world, v, rank);
  if (rc != 0) {
    snprintf(h->err, sizeof(h->err), "ncclCommInitRank: %s", a->GetErrorString ? a->GetErrorString(rc) : "error");
    h->comm = nullptr;
    return QTR_ERR_HIP;
  }
  h->comm_rank = rank;
  h->comm_world = world;
  return QTR_OK;
}

// one all-gather of `bytes` per rank from d_send into d_recv (rank order), on slot 0's stream
static int comm_allgather(qtr_handle* h, RcclApi* a, const void* d_send, void* d_recv, size_t bytes, hipStream_t st) {
  const int rc = a->AllGather(d_send, d_recv, bytes, /* ncclChar */ 0, h->comm, st);
  if (rc != 0) {
    snprintf(h->err, sizeof(h->err), "ncclAllGather: %s", a->GetErrorString ? a->GetErrorString(rc) : "error");
    return QTR_ERR_HIP;
  }
  return QTR_OK;
}

// require_equal: qtr_gather_results — blocks of different lengths are refused.  Every decision to leave before the second
// collective is taken from the GATHERED line (counts, capacities, flags: identical on every rank), never from a rank's
// own arguments: a rank that bailed out alone would leave the others waiting in ncclAllGather for good.
static int gather_impl(qtr_handle* h, const qtr_result* local, int n_local, qtr_result* all, int cap_all, int* counts,
                       int* n_all, bool require_equal) {
  if (!h || n_local < 0 || (n_local > 0 && !local) || cap_all < 0 || (cap_all > 0 && !all)) return QTR_ERR_BAD_ARG;
  if (!h->comm) {
    snprintf(h->err, sizeof(h->err), "qtr_gather_results: call qtr_comm_init first");
    return QTR_ERR_BAD_ARG;
  }
  RcclApi* a = rccl_api(h->err, sizeof(h->err));
  if (!a) return QTR_ERR_HIP;
  QTR_HIP_TRY(h, hipSetDevice(h->device));
  const int world = h->comm_world;
  hipStream_t st = h->slots[0].stream;
  auto reserve = [&](size_t bytes) -> int {
    if (h->comm_bytes >= bytes) return QTR_OK;
    if (h->comm_buf) (void)hipFree(h->comm_buf);
    h->comm_buf = nullptr;
    h->comm_bytes = 0;
    QTR_HIP_TRY(h, hipMalloc(&h->comm_buf, bytes));
    h->comm_bytes = bytes;
    return QTR_OK;
  };
  // 1. every rank's record count, the room it has for the result and whether it insists on equal blocks (a collective:
  //    ranks with nothing to send take part too)
  QTR_TRY(reserve(256 + 256 * (size_t)world));
  std::vector<int> cnt((size_t)world * 64, 0);  // one 256-byte line per rank
  int mine_line[64] = {n_local, cap_all, require_equal ? 1 : 0};
  QTR_HIP_TRY(h, hipMemcpyAsync(h->comm_buf, mine_line, 256, hipMemcpyHostToDevice, st));
  QTR_TRY(comm_allgather(h, a, h->comm_buf, (char*)h->comm_buf + 256, 256, st));
  QTR_HIP_TRY(h, hipMemcpyAsync(cnt.data(), (char*)h->comm_buf + 256, 256 * (size_t)world, hipMemcpyDeviceToHost, st));
  QTR_HIP_TRY(h, hipStreamSynchronize(st));
  int nmax = 0, nmin = 0x7fffffff;
  long long total = 0;
  bool want_equal = false;
  for (int r = 0; r < world; ++r) {
    const int c = cnt[(size_t)r * 64];
    if (counts) counts[r] = c;
    nmax = std::max(nmax, c);
    nmin = std::min(nmin, c);
    total += c;
    want_equal = want_equal || cnt[(size_t)r * 64 + 2] != 0;
  }
  if (n_all) *n_all = (int)total;
  if (want_equal && nmin != nmax) {  // (the same verdict on every rank)
    snprintf(h->err, sizeof(h->err), "qtr_gather_results: ranks hold different record counts (%d .. %d; use qtr_gather_results_v)",
             nmin, nmax);
    return QTR_ERR_BAD_ARG;
  }
  for (int r = 0; r < world; ++r)
    if (total > cnt[(size_t)r * 64 + 1]) {  // some rank has no room: every rank leaves here, together
      snprintf(h->err, sizeof(h->err), "qtr_gather_results: %lld records, rank %d has room for %d", total, r,
               cnt[(size_t)r * 64 + 1]);
      return QTR_ERR_CAPACITY;
    }
  if (nmax == 0) return QTR_OK;
  // 2. the records, every block padded to the longest (fixed-size collective), trimmed on the way out
  const size_t block = (size_t)nmax * sizeof(qtr_result);
  QTR_TRY(reserve(block * (size_t)(world + 1)));
  char* d_send = (char*)h->comm_buf;
  char* d_recv = d_send + block;
  QTR_HIP_TRY(h, hipMemsetAsync(d_send, 0, block, st));
  if (n_local > 0)
    QTR_HIP_TRY(h, hipMemcpyAsync(d_send, local, (size_t)n_local * sizeof(qtr_result), hipMemcpyHostToDevice, st));
  QTR_TRY(comm_allgather(h, a, d_send, d_recv, block, st));
  size_t off = 0;
  for (int r = 0; r < world; ++r) {
    const int c = cnt[(size_t)r * 64];
    if (c > 0)
      QTR_HIP_TRY(h, hipMemcpyAsync(all + off, d_recv + (size_t)r * block, (size_t)c * sizeof(qtr_result),
                                    hipMemcpyDeviceToHost, st));
    off += (size_t)c;
  }
  QTR_HIP_TRY(h, hipStreamSynchronize(st));
  return QTR_OK;
}

int qtr_gather_results_v(qtr_handle* h, const qtr_result* local, int n_local, qtr_result* all, int cap_all, int* counts,
                         int* n_all) {
  return gather_impl(h, local, n_local, all, cap_all, counts, n_all, false);
}

int qtr_gather_results(qtr_handle* h, const qtr_result* local, int n_local, qtr_result* all) {
  if (!h || n_local < 0 || (n_local > 0 && (!local || !all))) return QTR_ERR_BAD_ARG;
  // the caller sized `all` for world * n_local records: blocks of another length are refused (on every rank), not overrun
  const long long room = (long long)n_local * std::max(h->comm_world, 1);
  return gather_impl(h, local, n_local, all, (int)std::min<long long>(room, 0x7fffffff), nullptr, nullptr, true);
}

void qtr_comm_destroy(qtr_handle* h) {
  if (!h) return;
  if (h->comm) {
    RcclApi* a = rccl_api(nullptr, 0);
    if (a) (void)a->CommDestroy(h->comm);
    h->comm = nullptr;
  }
  if (h->comm_buf) {
    (void)hipFree(h->comm_buf);
    h->comm_buf = nullptr;
    h->comm_bytes = 0;
  }
}

int qtr_exact_stats(qtr_handle* h, int slot, unsigned long long* nodes, int* aborted) {
  if (!h || slot < 0 || slot >= (int)h->slots.size()) return QTR_ERR_BAD_ARG;
  if (nodes) *nodes = h->slots[slot].exact_nodes;
  if (aborted) *aborted = h->slots[slot].exact_aborted;
  return QTR_OK;
}

void qtr_default_limits(qtr_limits* l) {
  l->max_points = 262144;
  l->max_voxels = 65536;
  l->max_corr = 24576;
  l->n_slots = 1;
  l->max_long_neighbors = 0;  // = 128 * max_voxels
}

void qtr_default_params(qtr_params* p) {  // Quatro::Params defaults, reference include/quatro.hpp:202-268
  memset(p, 0, sizeof(*p));
  p->noise_bound = 0.3;
  p->cbar2 = 1.0;
  p->rotation_gnc_factor = 1.4;
  p->rotation_cost_threshold = 1e-6;
  p->kcore_heuristic_threshold = 0.5;
  p->cote_noise_bound = 0.3;
  p->ryrx[0] = p->ryrx[4] = p->ryrx[8] = 1.0;
  p->rotation_max_iterations = 100;
  p->inlier_selection_mode = QTR_INLIER_PMC_HEU;
  p->cote_median = 1;
  p->max_clique_time_limit = 3600;
}

void qtr_demo_params(qtr_params* p) {  // reference config/params.yaml:22-44
  qtr_default_params(p);
  p->rotation_cost_threshold = 1.1e-4;
  p->rotation_max_iterations = 50;
}

void qtr_default_frontend_params(qtr_frontend_params* p) {
  p->voxel_size = 0.3f;
  p->normal_radius = 0.5f;
  p->fpfh_radius = 0.75f;
  p->tuple_scale = 0.95f;
  p->use_crosscheck = 1;
  p->use_tuple_test = 1;
  p->seed = 0;
}

const char* qtr_last_error(const qtr_handle* h) { return h ? h->err : "null handle"; }
int qtr_num_slots(const qtr_handle* h) { return h ? (int)h->slots.size() : 0; }
void* qtr_slot_stream(qtr_handle* h, int slot) {
  if (!h || slot < 0 || slot >= (int)h->slots.size()) return nullptr;
  return (void*)h->slots[slot].stream;
}

void qtr_destroy(qtr_handle* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  qtr_comm_destroy(h);
  for (qtr_keyframe* kf : h->keyframes) {  // (keyframes the caller did not destroy)
    if (kf->dev) (void)hipFree(kf->dev);
    delete kf;
  }
  h->keyframes.clear();
  for (qtr_place_index* ix : h->place_indexes) {
    if (ix->dev) (void)hipFree(ix->dev);
    delete ix;
  }
  h->place_indexes.clear();
  vmap_free_all(h);
  for (auto& l : h->lanes) {
    if (l.stage.h) (void)hipHostFree(l.stage.h);
    if (l.stage.d) (void)hipFree(l.stage.d);
  }
  for (auto& s : h->slots) {
    if (s.stream) (void)hipStreamSynchronize(s.stream);
    if (s.stream2) (void)hipStreamSynchronize(s.stream2);
    if (s.stream3) (void)hipStreamSynchronize(s.stream3);
    for (auto& e : s.ev)
      if (e) (void)hipEventDestroy(e);
    if (s.ev_vox) (void)hipEventDestroy(s.ev_vox);
    for (hipEvent_t e : {s.ev_fork, s.ev_join})
      if (e) (void)hipEventDestroy(e);
    for (auto& e : s.fb.ev_nn)
      if (e) (void)hipEventDestroy(e);
    if (s.solver_arena) (void)hipFree(s.solver_arena);
    if (s.front_arena) (void)hipFree(s.front_arena);
    for (int c = 0; c < 2; ++c) {
      if (s.fb.cloud[c].nbr_big_idx) (void)hipFree(s.fb.cloud[c].nbr_big_idx);
      if (s.fb.cloud[c].nbr_big_d2) (void)hipFree(s.fb.cloud[c].nbr_big_d2);
    }
    if (s.in_src) (void)hipFree(s.in_src);
    if (s.in_tgt) (void)hipFree(s.in_tgt);
    if (s.m_src) (void)hipFree(s.m_src);
    if (s.m_tgt) (void)hipFree(s.m_tgt);
    if (s.pinned_i32) (void)hipHostFree(s.pinned_i32);
    if (s.pinned_res) (void)hipHostFree(s.pinned_res);
    if (s.mail) (void)hipHostFree(s.mail);
    if (s.seg_arena) (void)hipFree(s.seg_arena);
    if (s.pw_arena) (void)hipFree(s.pw_arena);
    if (s.ex_arena) (void)hipFree(s.ex_arena);
    icp_free(s.icp);
    eval_free(s.eval);
    pgo_free(s.pgo);
    if (s.place.arena) (void)hipFree(s.place.arena);
    if (s.place.pin) (void)hipHostFree(s.place.pin);
    if (s.merge_pin) (void)hipHostFree(s.merge_pin);
    if (s.merge_dev) (void)hipFree(s.merge_dev);
    if (s.deskew_pin) (void)hipHostFree(s.deskew_pin);
    if (s.deskew_dev) (void)hipFree(s.deskew_dev);
    vmap_batch_free(s);
    vmap_eval_free(s);
    place_batch_free(s);
    vmap_ct_free(s);
    if (s.stream) (void)hipStreamDestroy(s.stream);
    if (s.stream2) (void)hipStreamDestroy(s.stream2);
    if (s.stream3) (void)hipStreamDestroy(s.stream3);
  }
  delete h;
}

static int create_impl(qtr_handle* h) {
  QTR_HIP_TRY(h, hipSetDevice(h->device));
  QTR_HIP_TRY(h, solver_init_attributes());
  QTR_HIP_TRY(h, frontend_init_attributes());
  // A slot's second stream carries what must run BESIDE the first one's chain (the matcher's sequential means: 70 - 200 us of
  // one workgroup per cloud).  HIP multiplexes a process's streams onto a few hardware queues, and two streams that land on
  // the same one do not overlap: a handle created after another one (or after a framework's own streams) read the dense step
  // at 2.11 instead of 1.93 ms for that reason alone — its FPFH stage was chain + means, 0.48 ms, not their maximum, 0.27
  // (profiles/r6_ab.txt section 19).  Streams of different PRIORITY come from different queue pools, so the second stream
  // is created at the highest priority: its few small kernels are also the ones that should never wait behind a chain.
  int prio_least = 0, prio_greatest = 0;
  QTR_HIP_TRY(h, hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
  for (auto& s : h->slots) {
    QTR_HIP_TRY(h, hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
    if (prio_greatest != prio_least) QTR_HIP_TRY(h, hipStreamCreateWithPriority(&s.stream2, hipStreamNonBlocking, prio_greatest));
    else QTR_HIP_TRY(h, hipStreamCreateWithFlags(&s.stream2, hipStreamNonBlocking));
    for (auto& e : s.ev) QTR_HIP_TRY(h, hipEventCreate(&e));
    QTR_HIP_TRY(h, hipEventCreateWithFlags(&s.ev_vox, hipEventDisableTiming));
    for (auto& e : s.fb.ev_nn) QTR_HIP_TRY(h, hipEventCreate(&e));
    const size_t sbytes = solver_scratch_bytes(h->lim.max_corr) + 65536;
    QTR_HIP_TRY(h, hipMalloc(&s.solver_arena, sbytes));
    solver_carve(s.sb, s.solver_arena, h->lim.max_corr);
    const size_t fbytes = frontend_scratch_bytes(h->lim.max_points, h->lim.max_voxels) + 65536;
    QTR_HIP_TRY(h, hipMalloc(&s.front_arena, fbytes));
    {
      hipEvent_t keep[4] = {s.fb.ev_nn[0], s.fb.ev_nn[1], s.fb.ev_nn[2], s.fb.ev_nn[3]};
      frontend_carve(s.fb, s.front_arena, h->lim.max_points, h->lim.max_voxels);
      for (int q = 0; q < 4; ++q) s.fb.ev_nn[q] = keep[q];
      s.fb.nn_events = h->stage_events;
      // (the neighbour grid's cell counters start at zero and are left at zero by every chain that uses them: k2_cell_scan)
      for (int c = 0; c < 2; ++c) QTR_HIP_TRY(h, hipMemset(s.fb.cloud[c].cell_cnt, 0, (size_t)(QTR_CELL_CAP + 4096) * 4));
    }
    // (the long-list arenas — lists of more than QTR_KMAX neighbours: 8 bytes x max_long_neighbors per cloud, 134 MB per
    // slot at the defaults — are allocated the first time a chain with k2_neighbors_big is enqueued: ensure_long_arenas)
    QTR_HIP_TRY(h, hipMalloc((void**)&s.in_src, (size_t)h->lim.max_points * 16));
    QTR_HIP_TRY(h, hipMalloc((void**)&s.in_tgt, (size_t)h->lim.max_points * 16));
    QTR_HIP_TRY(h, hipMalloc((void**)&s.m_src, (size_t)h->lim.max_corr * 16));
    QTR_HIP_TRY(h, hipMalloc((void**)&s.m_tgt, (size_t)h->lim.max_corr * 16));
    QTR_HIP_TRY(h, hipHostMalloc((void**)&s.pinned_i32, 256 * sizeof(int)));
    QTR_HIP_TRY(h, hipHostMalloc((void**)&s.pinned_res, sizeof(qtr_result)));
    QTR_HIP_TRY(h, hipHostMalloc((void**)&s.mail, MAIL_INTS * sizeof(int), hipHostMallocMapped));
    memset(s.mail, 0, MAIL_INTS * sizeof(int));
    {
      void* dv = nullptr;
      QTR_HIP_TRY(h, hipHostGetDevicePointer(&dv, s.mail, 0));
      s.fb.mail = (int*)dv;
      s.sb.mail = (int*)dv;
      s.fb.m_src = s.m_src;
      s.fb.m_tgt = s.m_tgt;
      s.fb.m_cap = h->lim.max_corr;
    }
  }
  // batch lanes: two groups of slots that alternate (one's kernels cover the other's host read-back)
  const int S = (int)h->slots.size();
  int NL = S >= 2 ? 2 : 1;
  if (const char* e = QTR_ENGINE_ENV("QTR_BATCH_LANES")) {  // experiment knob: more, smaller groups in flight
    const int v = atoi(e);
    if (v >= 1 && v <= 8 && v <= S) NL = v;
  }
  h->lanes.resize((size_t)NL);
  for (int l = 0; l < NL; ++l) {
    Lane& ln = h->lanes[l];
    ln.cap = min(S / NL, 64);  // a launch chain serves at most 64 pairs (match.hip NN_MAXG)
    ln.first_slot = l * (S / NL);
    ln.stage.cap = (size_t)64 * 1024 + (size_t)ln.cap * 8192;
    QTR_HIP_TRY(h, hipHostMalloc((void**)&ln.stage.h, ln.stage.cap));
    QTR_HIP_TRY(h, hipMalloc((void**)&ln.stage.d, ln.stage.cap));
  }
  // experiment knob (test build only): the lanes' launch streams on DISJOINT sets of compute
  // units (hipExtStreamCreateWithCUMask; on this part bit k of the mask is compute unit k / 8 of XCD k % 8).
  //   QTR_LANE_CU_MASK=halves   lane l of NL takes the l-th NL-th of every XCD's units
  //   QTR_LANE_CU_MASK=xcd      lane l takes XCDs [8 l / NL, 8 (l + 1) / NL)
  // measured and NOT adopted: profiles/r6_ab.txt
  if (const char* e = QTR_ENGINE_ENV("QTR_LANE_CU_MASK")) {
    for (int l = 0; l < NL && NL > 1; ++l) {
      unsigned mask[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      for (int k = 0; k < 256; ++k) {
        const int xcd = k % 8, cu = k / 8;
        const bool mine = (strcmp(e, "xcd") == 0) ? (xcd * NL / 8 == l) : (cu * NL / 32 == l);
        if (mine) mask[k >> 5] |= 1u << (k & 31);
      }
      Slot& lead = h->slots[h->lanes[l].first_slot];
      (void)hipStreamDestroy(lead.stream);
      (void)hipStreamDestroy(lead.stream2);
      QTR_HIP_TRY(h, hipExtStreamCreateWithCUMask(&lead.stream, 8, mask));
      QTR_HIP_TRY(h, hipExtStreamCreateWithCUMask(&lead.stream2, 8, mask));
    }
  }
  return QTR_OK;
}

int qtr_create(int device, const qtr_limits* limits, qtr_handle** out) {
  if (!out) return QTR_ERR_BAD_ARG;
  *out = nullptr;
  qtr_handle* h = new (std::nothrow) qtr_handle();
  if (!h) return QTR_ERR_CAPACITY;
  h->err[0] = 0;
  h->device = device;
  h->uid = g_handle_uid.fetch_add(1, std::memory_order_relaxed) + 1;
  {
    const char* hw = getenv("QTR_HOST_WAIT");
    h->spin_wait = (hw && strcmp(hw, "block") == 0) ? 0 : 1;
    const char* se = getenv("QTR_STAGE_EVENTS");
    h->stage_events = (se && atoi(se) == 0) ? 0 : 1;
    h->nn_event_stride = h->stage_events ? 1 : 0;
    const char* co = getenv("QTR_CORR_OVERLAP");
    h->corr_overlap = (co && atoi(co) == 0) ? 0 : 1;
    const char* ib = getenv("QTR_ICP_BLOCK");
    h->icp_block = ib ? std::max(0, atoi(ib)) : 0;
  }
  if (limits)
    h->lim = *limits;
  else
    qtr_default_limits(&h->lim);
  if (h->lim.max_points < 64 || h->lim.max_voxels < 64 || h->lim.max_corr < 64 || h->lim.n_slots < 1 ||
      h->lim.max_corr > 32768 || h->lim.max_voxels > h->lim.max_points || h->lim.max_long_neighbors < 0 ||
      h->lim.max_voxels > QTR_NN_MAX_ROWS) {  // (k_recheck_filter's lists pack a base row into 20 bits: match.hip)
    delete h;
    return QTR_ERR_BAD_ARG;
  }
  if (h->lim.max_long_neighbors == 0)
    h->lim.max_long_neighbors = (int)std::min<long long>(128LL * h->lim.max_voxels, 1LL << 30);
  h->lim.max_long_neighbors = (h->lim.max_long_neighbors + 63) & ~63;
  h->slots.resize((size_t)h->lim.n_slots);
  const int rc = create_impl(h);
  *out = h;  // returned even on failure so that qtr_last_error can be read; caller destroys it
  return rc;
}

// adds the nearest-neighbour kernel times of the last match (events on its launch stream) to the slot's totals; called
// before the events are recorded again and by qtr_get_nn_totals
static void flush_nn_totals(Slot& s) {
  if (!s.nn_pending) return;
  s.nn_pending = 0;
  float a = 0, b = 0;
  if (hipEventElapsedTime(&a, s.fb.ev_nn[0], s.fb.ev_nn[1]) == hipSuccess &&
      hipEventElapsedTime(&b, s.fb.ev_nn[2], s.fb.ev_nn[3]) == hipSuccess) {
    s.nn_total_ms += (double)a + (double)b;
    s.nn_total_launches += 2;
  }
  (void)hipGetLastError();
}

static void fill_nn_times(Slot& s) {
  float a = 0, b = 0;
  s.nn_dir_ms[0] = s.nn_dir_ms[1] = 0.f;
  if (!s.nn_timed_last) return;  // (the fields keep their zeros)
  if (hipEventElapsedTime(&a, s.fb.ev_nn[0], s.fb.ev_nn[1]) == hipSuccess &&
      hipEventElapsedTime(&b, s.fb.ev_nn[2], s.fb.ev_nn[3]) == hipSuccess) {
    s.times.nn_kernel = a + b;
    s.times.nn_launches = 2;
    s.nn_dir_ms[0] = a;
    s.nn_dir_ms[1] = b;
  }
}

// Waits until the phase-ending kernel has published `seq` in mailbox word `idx` (frontend.h MAIL_SEQ_*).  The
// default is to WATCH the pinned word — the store crosses PCIe in ~1-2 us, the runtime's stream wait costs
// 20-30 us per phase boundary (three per registration) — and to fall back to the runtime every 64k polls so
// that a failed launch or a lost device ends the wait.  QTR_HOST_WAIT=block uses hipStreamSynchronize only.  `st`: the stream
// the phase-ending kernel was enqueued on — the one that is queried and synchronised, whichever slot or lane owns it.
// the payload a sequence word announces is consumed only once its tag matches (common.h, mail_store_line): the
// sequence word can reach host memory before the counters
static bool mail_payload_ok(const Slot& s, int idx, int seq) {
  auto line_ok = [&](int base) {
    const volatile int* l = s.mail + base;
    int x = 0;
    for (int i = 0; i < 15; ++i) x ^= l[i];
    return l[15] == (seq ^ x ^ MAIL_TAG_SALT);
  };
  auto solver_ok = [&]() {
    const volatile int* m = s.mail + MAIL_SOLVER;
    int x = 0, y = 0;
    for (int i = 0; i < (int)(sizeof(qtr_result) / 4); ++i) x ^= m[i];
    for (int i = 0; i < (int)(sizeof(SolverState) / 4); ++i) y ^= m[64 + i];
    return m[63] == (seq ^ x ^ MAIL_TAG_SALT) && m[96] == (seq ^ y ^ MAIL_TAG_SALT);
  };
  switch (idx) {
    case MAIL_SEQ_VOX0: return line_ok(MAIL_VOX0);
    case MAIL_SEQ_VOX1: return line_ok(MAIL_VOX1);
    case MAIL_SEQ_MATCH: return line_ok(MAIL_MATCH) && line_ok(MAIL_CNT0) && line_ok(MAIL_CNT1);
    case MAIL_SEQ_SOLVE: return solver_ok();
    case MAIL_SEQ_ICP_BOX: return line_ok(MAIL_ICP_BOX);
    case MAIL_SEQ_ICP: return line_ok(MAIL_ICP) && line_ok(MAIL_ICP + 16) && line_ok(MAIL_ICP + 32);
    default: return true;
  }
}
// non-blocking: has the phase-ending kernel published `seq` in word `idx`, payload complete?
static bool mail_ready(const Slot& s, int idx, int seq) {
  if (__atomic_load_n((volatile int*)(s.mail + idx), __ATOMIC_ACQUIRE) != seq) return false;
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
  return mail_payload_ok(s, idx, seq);
}

static int wait_mail(qtr_handle* h, Slot& s, hipStream_t st, int idx, int seq) {
  volatile int* p = s.mail + idx;
  if (!h->spin_wait) {
    QTR_HIP_TRY(h, hipStreamSynchronize(st));
  } else {
    for (unsigned long spins = 1;; ++spins) {
      if (__atomic_load_n(p, __ATOMIC_ACQUIRE) == seq) break;  // now make sure the payload it announces is complete
      if ((spins & 0xffff) == 0) {
        const hipError_t q = hipStreamQuery(st);
        if (q == hipSuccess) break;  // stream drained: the word must be there now (checked below)
        if (q != hipErrorNotReady) QTR_HIP_TRY(h, q);
        (void)hipGetLastError();  // hipErrorNotReady is not an error of ours
      }
      __builtin_ia32_pause();
    }
  }
  if (__atomic_load_n(p, __ATOMIC_ACQUIRE) != seq) {
    snprintf(h->err, sizeof(h->err), "mailbox word %d holds %d, expected %d (phase kernel did not run)", idx, (int)*p, seq);
    return QTR_ERR_HIP;
  }
  auto payload_ok = [&]() { return mail_payload_ok(s, idx, seq); };
  bool drained = false;
  for (unsigned long spins = 1;; ++spins) {
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    if (payload_ok()) return QTR_OK;
    if ((spins & 0x3fff) == 0) {
      if (drained) break;  // the stream was idle one round ago and the payload still does not add up
      const hipError_t q = hipStreamSynchronize(st);
      if (q != hipSuccess) QTR_HIP_TRY(h, q);
      drained = true;
    }
    __builtin_ia32_pause();
  }
  snprintf(h->err, sizeof(h->err), "mailbox payload of word %d does not match its tag (sequence %d)", idx, seq);
  return QTR_ERR_HIP;
}

// The stage times of the slot's last call, read off its events by the rows of its shape (stage_times.h).
static void compute_times(Slot& s) {
  if (s.times_pending == TIMES_NONE) return;
  static float qtr_stage_times::*const field[SF_COUNT] = {
      &qtr_stage_times::voxelize, &qtr_stage_times::fpfh,  &qtr_stage_times::match, &qtr_stage_times::graph,
      &qtr_stage_times::clique,   &qtr_stage_times::solve, &qtr_stage_times::total};
  const ShapeTimes& sh = k_shape_times[s.times_pending];
  if (sh.sync >= 0) (void)hipEventSynchronize(s.ev[sh.sync]);
  s.times = qtr_stage_times{};
  float ms = 0;
  for (int r = 0; r < sh.nrows; ++r)
    if (hipEventElapsedTime(&ms, s.ev[sh.rows[r].from], s.ev[sh.rows[r].to]) == hipSuccess) s.times.*field[sh.rows[r].field] = ms;
  if (sh.nn) fill_nn_times(s);
  (void)hipGetLastError();
  s.times_pending = TIMES_NONE;
}

// the stage times of a call that is ONE stage: EV_STAGE_BEGIN -> EV_STAGE_END, into `field` (null: none) and the total
static void times_one_stage(Slot& s, float qtr_stage_times::*field) {
  float ms = 0;
  s.times_pending = TIMES_NONE;
  s.times = qtr_stage_times{};
  if (hipEventElapsedTime(&ms, s.ev[EV_STAGE_BEGIN], s.ev[EV_STAGE_END]) != hipSuccess) return;
  s.times.total = ms;
  if (field) s.times.*field = ms;
}

// The long-list arenas of a slot's two clouds, allocated on first need: voxel-grid centroids at the demo's leaf never have
// more than QTR_KMAX neighbours, so most handles never pay for them.
static int ensure_long_arenas(qtr_handle* h, Slot& s) {
  for (int c = 0; c < 2; ++c) {
    CloudBufs& cb = s.fb.cloud[c];
    // (each pointer on its own: a failed second allocation must not make the next call allocate the first one again)
    if (!cb.nbr_big_idx) QTR_HIP_TRY(h, hipMalloc((void**)&cb.nbr_big_idx, (size_t)h->lim.max_long_neighbors * 4));
    if (!cb.nbr_big_d2) QTR_HIP_TRY(h, hipMalloc((void**)&cb.nbr_big_d2, (size_t)h->lim.max_long_neighbors * 4));
    cb.nbr_big_cap = h->lim.max_long_neighbors;
  }
  return QTR_OK;
}

// inspection calls (qtr_debug_fetch, timings) look at a slot without ending what its last call left behind
static Slot* peek_slot(qtr_handle* h, int slot) {
  if (!h) return nullptr;
  if (slot < 0 || slot >= (int)h->slots.size()) {
    snprintf(h->err, sizeof(h->err), "slot %d out of range", slot);
    return nullptr;
  }
  return &h->slots[slot];
}
// every working call: the slot's clouds are no longer those of a registration (qtr_refine_pair refuses them)
static Slot* get_slot(qtr_handle* h, int slot) {
  Slot* s = peek_slot(h, slot);
  if (s) s->reg_ready = 0;
  return s;
}

static int check_params(qtr_handle* h, const qtr_params* prm) {
  if (!prm) {
    snprintf(h->err, sizeof(h->err), "params is NULL");
    return QTR_ERR_BAD_ARG;
  }
  if (prm->inlier_selection_mode == QTR_INLIER_NONE) {
    snprintf(h->err, sizeof(h->err), "inlier_selection_mode NONE not supported (undefined behaviour in the reference)");
    return QTR_ERR_UNSUPPORTED;
  }
  if (prm->reg_mode != QTR_REG_QUATRO && prm->reg_mode != QTR_REG_TEASER) {
    snprintf(h->err, sizeof(h->err), "[solveForRotation] The param is wrong! It should be 'TEASER' or 'Quatro'");
    return QTR_ERR_BAD_ARG;
  }
  if (prm->reg_mode == QTR_REG_TEASER && prm->using_pre_estimated_ryrx) {  // reference include/quatro.hpp:424-426
    snprintf(h->err, sizeof(h->err), "Wrong reg type name is coming!");
    return QTR_ERR_BAD_ARG;
  }
  if (prm->inlier_selection_mode < 0 || prm->inlier_selection_mode > 3 || !(prm->noise_bound > 0) ||
      !(prm->rotation_gnc_factor > 1) || prm->rotation_max_iterations < 1) {
    snprintf(h->err, sizeof(h->err), "invalid solver parameter");
    return QTR_ERR_BAD_ARG;
  }
  // COTE's range is cote_noise_bound * sqrt(cbar2) (reference include/quatro.hpp:585-616): a negative or NaN range has
  // no meaning there (intervals that close before they open, NaN sort keys); 0 is computed with under IEEE rules
  if (!(prm->cote_noise_bound >= 0)) {
    snprintf(h->err, sizeof(h->err), "invalid solver parameter: cote_noise_bound must be >= 0");
    return QTR_ERR_BAD_ARG;
  }
  if (!(prm->cbar2 >= 0)) {
    snprintf(h->err, sizeof(h->err), "invalid solver parameter: cbar2 must be >= 0");
    return QTR_ERR_BAD_ARG;
  }
  return QTR_OK;
}

// the back end's bound on the correspondences it is handed
static int check_max_corr(qtr_handle* h, int L) {
  if (L <= h->lim.max_corr) return QTR_OK;
  snprintf(h->err, sizeof(h->err), "L=%d exceeds max_corr=%d", L, h->lim.max_corr);
  return QTR_ERR_CAPACITY;
}

// PMC_EXACT after the heuristic has finished (state `hs` = the device SolverState as the host last saw it): proves the
// heuristic clique maximum or replaces it (exact.hip).  *improved tells the caller that st->mc / best_r / picks changed.
// time_limit: Params::max_clique_time_limit of THIS call, seconds (reference include/quatro.hpp:267,800; <= 0: none).
// Enqueued and waited for on `st`, the stream of the chain that left the state.
static int exact_phase(qtr_handle* h, Slot& s, hipStream_t st, int L, const SolverState& hs, bool* improved,
                       double time_limit) {
  *improved = false;
  s.exact_nodes = 0;
  s.exact_aborted = 0;
  if (L <= 0 || hs.mc >= hs.ub || hs.mc < 1) return QTR_OK;  // lb == ub: reference src/graph.cc:100-102
  const int W = (L + 63) / 64;
  if (exact_nw(W) == 0) {
    snprintf(h->err, sizeof(h->err), "PMC_EXACT supports at most 32768 vertices (L=%d)", L);
    return QTR_ERR_CAPACITY;
  }
  const int depth_cap = hs.ub + 1;
  const size_t small_lds = exact_small_lds(L, W, hs.t0, depth_cap);
  int nwaves = small_lds ? 1024 : 2048;
  while (nwaves > 64 && exact_scratch_bytes(W, depth_cap, nwaves) > ((size_t)768 << 20)) nwaves >>= 1;
  if (!small_lds && nwaves > L) nwaves = L < 1 ? 1 : L;
  const size_t need = exact_scratch_bytes(W, depth_cap, nwaves);
  if (need > s.ex_bytes) {
    if (s.ex_arena) (void)hipFree(s.ex_arena);
    s.ex_arena = nullptr;
    s.ex_bytes = 0;
    QTR_HIP_TRY(h, hipMalloc(&s.ex_arena, need));
    s.ex_bytes = need;
  }
  exact_carve(s.exb, s.ex_arena, depth_cap, nwaves);
  const long long ticks = time_limit > 0 ? (long long)(time_limit * 1e8) : 0;  // 100 MHz counter
  hipLaunchKernelGGL(k_exact_init, dim3(1), dim3(1), 0, st, s.sb.Kp, L, s.sb.st, s.exb.ctl);
  exact_launch_search(s.sb, s.exb, L, depth_cap, nwaves, 0, ticks, st, hs.t0, small_lds);
  ExactCtl* hc = (ExactCtl*)(s.pinned_i32 + 192);
  QTR_HIP_TRY(h, hipMemcpyAsync(hc, s.exb.ctl, sizeof(ExactCtl), hipMemcpyDeviceToHost, st));
  QTR_HIP_TRY(h, hipStreamSynchronize(st));
  s.exact_nodes = hc->nodes;
  if (hc->abort) {  // time limit: the heuristic clique stands (the reference returns PMC's best so far)
    s.exact_aborted = 1;
    return QTR_OK;
  }
  if (hc->gbest <= hs.mc) return QTR_OK;
  QTR_HIP_TRY(h, hipMemsetAsync(s.exb.cliq, 0xff, (size_t)nwaves * (depth_cap + 2) * sizeof(int), st));
  hipLaunchKernelGGL(k_exact_phase_b, dim3(1), dim3(1), 0, st, s.sb.Kp, L, s.exb.ctl);
  exact_launch_search(s.sb, s.exb, L, depth_cap, nwaves, 1, ticks, st, hs.t0, small_lds);
  hipLaunchKernelGGL(k_exact_commit, dim3(1), dim3(256), 0, st, s.exb.ctl, s.exb.cliq, nwaves, depth_cap, s.sb.st,
                     s.sb.picks);
  QTR_HIP_TRY(h, hipMemcpyAsync(hc, s.exb.ctl, sizeof(ExactCtl), hipMemcpyDeviceToHost, st));
  QTR_HIP_TRY(h, hipStreamSynchronize(st));
  s.exact_nodes += hc->nodes;
  if (hc->abort || hc->winner < 0) {
    s.exact_aborted = 1;
    return QTR_OK;
  }
  *improved = true;
  return QTR_OK;
}

// the cells of the larger of a pair's two neighbour-search grids (CNT_NCELL words of the voxel stage's mail) when BOTH fit the
// dense cell table of the FPFH chain, else 0 = sort packed cell keys (frontend.hip, d_cell_count)
static int cell_table_cells(int ncell_s, int ncell_t) {
  static const bool off = QTR_ENGINE_ENV("QTR_CELL_TABLE") != nullptr && atoi(QTR_ENGINE_ENV("QTR_CELL_TABLE")) == 0;
  if (off || ncell_s <= 0 || ncell_t <= 0 || ncell_s > QTR_CELL_CAP || ncell_t > QTR_CELL_CAP) return 0;
  return std::max(ncell_s, ncell_t);
}

// k_hcore_async's workgroups of one chain have to be resident together, so chains that may overlap must not ask for more
// than the compute units between them.  Who may overlap is decided by WHO CALLS, not by what happens to be in flight at
// the moment of the call (round 4 looked at the in-flight count: the first of several threads took the whole device and
// the others' launches were only partly resident until a residency timeout sent them to the peeling fallback): every
// host thread registers with the handle on its first back-end call, and from the moment a second thread has registered
// every chain takes 1 / min(LIVE threads, slots) of the units: a thread leaves the count when it ends (a pool of short-lived
// threads that run one at a time keeps the whole device), and whenever the share CHANGES — a third thread arriving, one
// leaving — the chains enqueued under the old share are waited for once (1/2 + 1/2 + 1/3 would oversubscribe as surely as
// 1 + 1/2).  A single-threaded caller never pays anything.  (QTR_DBG_CORE and the floor statistics
// st[22] / st[29] depend on timing either way: the floor is decided by what has been published 200 us into the launch.)
// (the handles a thread has registered with; its destructor — the thread's end — takes the thread off their counts)
struct ThreadCallerList {
  struct Entry {
    unsigned long long uid;
    std::shared_ptr<qtr_handle::Callers> c;
  };
  std::vector<Entry> e;
  ~ThreadCallerList() {
    for (Entry& x : e) x.c->live.fetch_sub(1, std::memory_order_acq_rel);
  }
  void enter(qtr_handle* h) {
    for (const Entry& x : e)
      if (x.uid == h->uid) return;  // (a thread that works with several handles in turn is ONE caller of each, once)
    if (e.size() >= 64) {  // handles come and go: keep the list short — drop the entries of destroyed handles first; if
      size_t victim = 0;   // every one is alive the oldest goes AND leaves its handle's count (it re-registers if it returns)
      for (size_t i = 0; i < e.size(); ++i)
        if (e[i].c.use_count() == 1) {
          victim = i;
          break;
        }
      e[victim].c->live.fetch_sub(1, std::memory_order_acq_rel);
      e.erase(e.begin() + (long)victim);
    }
    h->callers->live.fetch_add(1, std::memory_order_acq_rel);
    e.push_back(Entry{h->uid, h->callers});
  }
};

struct InFlight {
  qtr_handle* h;
  int gen;
  explicit InFlight(qtr_handle* h_) : h(h_) {
    static thread_local ThreadCallerList t_callers;
    t_callers.enter(h);
    const int want = std::max(1, std::min(h->callers->live.load(std::memory_order_acquire), (int)h->slots.size()));
    bool changed = false;
    {
      std::lock_guard<std::mutex> lk(h->share_mu);
      if (want != h->share_val) {  // a thread came or went: chains enqueued under the old share drain before this one starts
        h->share_val = want;
        ++h->share_gen;
        changed = true;
      }
      gen = h->share_gen;
      h->gen_inflight[gen & 3].fetch_add(1, std::memory_order_acq_rel);
    }
    h->solves_in_flight.fetch_add(1, std::memory_order_acq_rel);
    if (changed)  // (bounded: a chain another thread never reads back must not hang this one; three generations back is every
      for (int back = 1; back <= 3; ++back)  // chain that can still be in flight under an older share)
        for (int spins = 0; h->gen_inflight[(gen - back) & 3].load(std::memory_order_acquire) > 0 && spins < 2000000; ++spins)
          std::this_thread::yield();
    solver_set_hca_share(want);
  }
  ~InFlight() {
    h->gen_inflight[gen & 3].fetch_sub(1, std::memory_order_acq_rel);
    h->solves_in_flight.fetch_sub(1, std::memory_order_acq_rel);
  }
};

// What follows the solver's mail for one pair (k_finalize left the record and the state in the slot's mailbox): more clique
// rounds when the state says so (rare), PMC_EXACT's search and a second estimate when it found a larger clique.  Everything
// is enqueued on `st` and waited for there — the stream of the solver chain, which need not be the slot's own (a lane's, the
// third stream); record_end: the end of each follow-up chain is the call's EV_SOLVE.
static int solve_followup(qtr_handle* h, Slot& s, const float4* c_src, const float4* c_tgt, int L, const qtr_params* prm,
                          hipStream_t st, bool record_end) {
  if (L <= 0) return QTR_OK;
  const SolverState* ms = (const SolverState*)(s.mail + MAIL_SOLVER + 64);
  if (!ms->done) {
    s.sb.mail_seq = ++s.seq;
    QTR_HIP_TRY(h, solver_continue(s.sb, c_src, c_tgt, L, *prm, st, s.pinned_i32 + 128, ms->redo_cores));
    if (record_end) QTR_HIP_TRY(h, hipEventRecord(s.ev[EV_SOLVE], st));
    QTR_TRY(wait_mail(h, s, st, MAIL_SEQ_SOLVE, s.seq));
  }
  if (prm->inlier_selection_mode != QTR_INLIER_PMC_EXACT) return QTR_OK;
  SolverState hs;
  memcpy(&hs, ms, sizeof(hs));
  bool improved = false;
  QTR_TRY(exact_phase(h, s, st, L, hs, &improved, prm->max_clique_time_limit));
  if (!improved) return QTR_OK;
  s.sb.mail_seq = ++s.seq;  // estimate again from the larger clique
  QTR_HIP_TRY(h, solver_refinalize(s.sb, c_src, c_tgt, L, *prm, st));
  if (record_end) QTR_HIP_TRY(h, hipEventRecord(s.ev[EV_SOLVE], st));
  return wait_mail(h, s, st, MAIL_SEQ_SOLVE, s.seq);
}

// the result record out of the slot's mailbox; the counts the front end wrote into *res stay
static void result_from_mail(const Slot& s, qtr_result* res) {
  const int keep_ns = res->n_src, keep_nt = res->n_tgt, keep_nc = res->n_corr;
  memcpy(res, s.mail + MAIL_SOLVER, sizeof(qtr_result));
  res->n_src = keep_ns;
  res->n_tgt = keep_nt;
  res->n_corr = keep_nc;
}

// The caller's n correspondences where the back end reads them: device pointers as they are, host clouds copied into the
// slot's matched-cloud buffers on `st` (the lanes: lead.stream).  A matcher that runs on the slot gathers its own matched
// clouds into m_src / m_tgt (the fused tails of match.hip, through FrontBufs::m_src), so whoever stages on the stream of a
// front end stages BEHIND it; qtr_register_pair_corr stages BESIDE its front end, on the third stream, and takes the
// buffers away from that front end's matcher for the call (front_device, CorrEarly: nobody reads its gathered clouds).
static int corr_stage(qtr_handle* h, Slot& s, const float* src4, const float* tgt4, int n, int mem, hipStream_t st,
                      const float4** cs, const float4** ct) {
  *cs = (const float4*)src4;
  *ct = (const float4*)tgt4;
  if (mem != QTR_MEM_HOST) return QTR_OK;
  if (n > 0) {
    QTR_HIP_TRY(h, hipMemcpyAsync(s.m_src, src4, (size_t)n * 16, hipMemcpyHostToDevice, st));
    QTR_HIP_TRY(h, hipMemcpyAsync(s.m_tgt, tgt4, (size_t)n * 16, hipMemcpyHostToDevice, st));
  }
  *cs = s.m_src;
  *ct = s.m_tgt;
  return QTR_OK;
}

// Runs the back end on device-resident matched clouds and brings the result record to the host.
static int solve_device(qtr_handle* h, Slot& s, const float4* d_src, const float4* d_tgt, int L, const qtr_params* prm,
                        qtr_result* res, bool reset_done = false) {
  s.last_L = L;
  s.last_Wb = (((L + 63) / 64) + 3) & ~3;
  s.sb.mail_seq = ++s.seq;
  // k_hcore_async's workgroups have to be resident together: a chain that starts while another slot's is in flight (calls
  // from several threads) takes its share of the compute units only (solver.hip, solver_set_hca_share)
  InFlight in_flight(h);
  QTR_HIP_TRY(h, solver_enqueue(s.sb, d_src, d_tgt, L, *prm, s.stream, h->stage_events ? s.ev[EV_GRAPH] : nullptr,
                                h->stage_events ? s.ev[EV_CLIQUE] : nullptr, reset_done));
  if (h->stage_events) QTR_HIP_TRY(h, hipEventRecord(s.ev[EV_SOLVE], s.stream));
  QTR_TRY(wait_mail(h, s, s.stream, MAIL_SEQ_SOLVE, s.seq));
  QTR_TRY(solve_followup(h, s, d_src, d_tgt, L, prm, s.stream, h->stage_events != 0));
  result_from_mail(s, res);
  return res->status;
}

// One index list of a record to where the caller wants it, enqueued on `st`: QTR_ERR_CAPACITY when its n entries do not
// fit `cap` (nothing is enqueued then); *copies counts the copies enqueued.
static int list_out_enqueue(qtr_handle* h, int* dst, const int* src, int n, int cap, int mem, hipStream_t st, int* copies) {
  if (!dst || n <= 0) return QTR_OK;
  if (n > cap) return QTR_ERR_CAPACITY;
  const hipMemcpyKind kind = (mem == QTR_MEM_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  QTR_HIP_TRY(h, hipMemcpyAsync(dst, src, sizeof(int) * (size_t)n, kind, st));
  ++*copies;
  return QTR_OK;
}

// The tail every blocking registration shares once its record is in *res (rc = its status): QTR_OK or
// QTR_ERR_CLIQUE_TOO_SMALL goes on, anything else is returned as it is.  The call's shape for the stage times; the lists out
// on `st`, complete on return, stopping at the first one that does not fit (it becomes the record's status).  (A lane marks
// the pair, goes on with the next list and synchronises once for its group: lane_after_solve.)
static int finish_registration(qtr_handle* h, Slot& s, int rc, TimesShape shape, qtr_result* res, int* clique,
                               int* rot_inliers, int* final_inliers, int cap, int mem, hipStream_t st) {
  if (rc != QTR_OK && rc != QTR_ERR_CLIQUE_TOO_SMALL) return rc;
  s.times_pending = h->stage_events ? shape : TIMES_EVENTS_OFF;
  auto lists_out = [&]() -> int {
    int copies = 0;
    QTR_TRY(list_out_enqueue(h, clique, s.sb.clique, res->n_clique, cap, mem, st, &copies));
    QTR_TRY(list_out_enqueue(h, rot_inliers, s.sb.rot_inl, res->n_rot_inliers, cap, mem, st, &copies));
    QTR_TRY(list_out_enqueue(h, final_inliers, s.sb.final_inl, res->n_final, cap, mem, st, &copies));
    QTR_HIP_TRY(h, hipStreamSynchronize(st));
    return QTR_OK;
  };
  const int rc2 = lists_out();
  return rc2 != QTR_OK ? (res->status = rc2) : rc;
}

int qtr_solve(qtr_handle* h, int slot, const float* src4, const float* tgt4, int L, const qtr_params* prm,
              qtr_result* res, int* clique, int* rot_inliers, int* final_inliers, int cap, int mem) {
  Slot* sp = get_slot(h, slot);
  if (!sp || !res) return QTR_ERR_BAD_ARG;
  Slot& s = *sp;
  memset(res, 0, sizeof(*res));
  int rc = check_params(h, prm);
  if (rc != QTR_OK) return res->status = rc;
  if (L < 0 || (L > 0 && (!src4 || !tgt4))) {
    snprintf(h->err, sizeof(h->err), "bad input clouds");
    return res->status = QTR_ERR_BAD_ARG;
  }
  if ((rc = check_max_corr(h, L)) != QTR_OK) return res->status = rc;
  QTR_HIP_TRY(h, hipSetDevice(h->device));
  const float4 *d_src = nullptr, *d_tgt = nullptr;
  // (an event record is a marker packet the queue has to retire before the next launch starts: with the stage events
  // off a call records none at all, and every field of qtr_stage_times reads 0)
  const bool ev_on = h->stage_events != 0;
  if (ev_on) QTR_HIP_TRY(h, hipEventRecord(s.ev[EV_BEGIN], s.stream));
  QTR_TRY(corr_stage(h, s, src4, tgt4, L, mem, s.stream, &d_src, &d_tgt));
  if (ev_on) QTR_HIP_TRY(h, hipEventRecord(s.ev[EV_STAGED], s.stream));
  res->n_corr = L;
  rc = solve_device(h, s, d_src, d_tgt, L, prm, res);
  return finish_registration(h, s, rc, TIMES_SOLVE, res, clique, rot_inliers, final_inliers, cap, mem, s.stream);
}

int qtr_max_clique(qtr_handle* h, int slot, const unsigned long long* adj, int L, int mode, double kcore_thr,
                   double time_limit, int* clique, int cap, int* n_out, int* max_core_out, int mem) {
  Slot* sp = get_slot(h, slot);
  if (!sp || !n_out || L < 0 || (L > 0 && (!adj || !clique))) return QTR_ERR_BAD_ARG;
  Slot& s = *sp;
  *n_out = 0;
  if (max_core_out) *max_core_out = 0;
  if (mode != QTR_INLIER_PMC_HEU && mode != QTR_INLIER_KCORE_HEU && mode != QTR_INLIER_PMC_EXACT) {
    snprintf(h->err, sizeof(h->err), "clique solver mode %d not supported", mode);
    return QTR_ERR_UNSUPPORTED;
  }
  QTR_TRY(check_max_corr(h, L));
  if (L == 0) return QTR_OK;
  QTR_HIP_TRY(h, hipSetDevice(h->device));
  const int W = (L + 63) / 64;
  const u64* d_adj = (const u64*)adj;
  if (mem == QTR_MEM_HOST) {
    QTR_HIP_TRY(h, hipMemcpyAsync(s.sb.bm, adj, (size_t)L * W * 8, hipMemcpyHostToDevice, s.stream));
    d_adj = s.sb.bm;
  }
  s.last_L = L;
  s.last_Wb = (L + 63) / 64;  // the caller's packed layout
  InFlight in_flight(h);
  QTR_HIP_TRY(h, clique_only_enqueue(s.sb, d_adj, L, mode, kcore_thr, s.stream));
  QTR_HIP_TRY(h, hipMemcpyAsync(s.pinned_i32 + 128, s.sb.st, sizeof(SolverState), hipMemcpyDeviceToHost, s.stream));
  QTR_HIP_TRY(h, hipStreamSynchronize(s.stream));
  if (!((const SolverState*)(s.pinned_i32 + 128))->done) {
    qtr_params dummy;
    qtr_default_params(&dummy);
    QTR_HIP_TRY(h, solver_continue(s.sb, nullptr, nullptr, L, dummy, s.stream, s.pinned_i32 + 128,
                                   ((const SolverState*)(s.pinned_i32 + 128))->redo_cores));
  }
  if (mode == QTR_INLIER_PMC_EXACT) {
    SolverState hs;
    memcpy(&hs, s.pinned_i32 + 128, sizeof(hs));
    bool improved = false;
    QTR_TRY(exact_phase(h, s, s.stream, L, hs, &improved, time_limit));
  }
  s.sb.mail_seq = ++s.seq;
  QTR_HIP_TRY(h, clique_only_finish(s.sb, L, s.stream));
  QTR_TRY(wait_mail(h, s, s.stream, MAIL_SEQ_SOLVE, s.seq));
  memcpy(s.pinned_res, s.mail + MAIL_SOLVER, sizeof(qtr_result));
  const int M = s.pinned_res->n_clique;
  if (max_core_out) *max_core_out = s.pinned_res->max_core;
  *n_out = M;
  if (M > cap) return QTR_ERR_CAPACITY;
  if (M > 0) {
    const hipMemcpyKind kind = (mem == QTR_MEM_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    QTR_HIP_TRY(h, hipMemcpyAsync(clique, s.sb.clique, sizeof(int) * (size_t)M, kind, s.stream));
    QTR_HIP_TRY(h, hipStreamSynchronize(s.stream));
  }
  return QTR_OK;
}

// ------------------------------------------------------------------------------------------------
// individually callable stages (stages.hip).  All staging goes through the slot's solver arena.
static bool stage_fits(qtr_handle* h, Slot& s, size_t doubles, size_t ints) {
  if (doubles <= (size_t)72 * s.sb.Lcap && ints <= (size_t)24 * s.sb.Lcap) return true;
  snprintf(h->err, sizeof(h->err), "stage call needs %zu doubles / %zu ints of scratch; raise max_corr (now %d)",
           doubles, ints, s.sb.Lcap);
  return false;
}

int qtr_compute_tims(qtr_handle* h, int slot, const double* v3n, int N, double* tims3k, int* map2k) {
  Slot* sp = get_slot(h, slot);
  if (!sp || N < 0 || (N > 1 && (!v3n || !tims3k || !map2k))) return QTR_ERR_BAD_ARG;
  Slot& s = *sp;
  const long long K = (long long)N * (N - 1) / 2;
  if (K <= 0) return QTR_OK;
  if (!stage_fits(h, s, (size_t)3 * N + (size_t)3 * K, (size_t)2 * K)) return QTR_ERR_CAPACITY;
  QTR_HIP_TRY(h, hipSetDevice(h->device));
  double* d_v = s.sb.f64;
  double* d_t = d_v + (size_t)3 * N;
  QTR_HIP_TRY(h, hipMemcpyAsync(d_v, v3n, sizeof(double) * 3 * (size_t)N, hipMemcpyHostToDevice, s.stream));
  hipLaunchKernelGGL(k_compute_tims, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, s.stream, d_v, N, K, d_t, s.sb.i32);
  QTR_HIP_TRY(h, hipGetLastError());
  QTR_HIP_TRY(h, hipMemcpyAsync(tims3k, d_t, sizeof(double) * 3 * (size_t)K, hipMemcpyDeviceToHost, s.stream));
  QTR_HIP_TRY(h, hipMemcpyAsync(map2k, s.sb.i32, sizeof(int) * 2 * (size_t)K, hipMemcpyDeviceToHost, s.stream));
  QTR_HIP_TRY(h, hipStreamSynchronize(s.stream));
  return QTR_OK;
}

int qtr_scale_mask(qtr_handle* h, int slot, const double* a, const double* b, long long K, double noise_bound,
                   double cbar2, unsigned char* mask) {
  Slot* sp = get_slot(h, slot);
  if (!sp || K < 0 || (K > 0 && (!a || !b || !mask)) || !(noise_bound > 0)) return QTR_ERR_BAD_ARG;
  Slot& s = *sp;
  if (K == 0) return QTR_OK;
  if (!stage_fits(h, s, (size_t)6 * K, (size_t)(K + 3) / 4)) return QTR_ERR_CAPACITY;
  QTR_HIP_TRY(h, hipSetDevice(h->device));
  double* d_a = s.sb.f64;
  double* d_b = d_a + (size_t)3 * K;
  unsigned char* d_m = (unsigned char*)s.sb.i32;
  QTR_HIP_TRY(h, hipMemcpyAsync(d_a, a, sizeof(double) * 3 * (size_t)K, hipMemcpyHostToDevice, s.stream));
  QTR_HIP_TRY(h, hipMemcpyAsync(d_b, b, sizeof(double) * 3 * (size_t)K, hipMemcpyHostToDevice, s.stream));
  const double beta = 2 * noise_bound * sqrt(cbar2);
  hipLaunchKernelGGL(k_scale_mask, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, s.stream, d_a, d_b, K, beta, d_m);
  QTR_HIP_TRY(h, hipGetLastError());
  QTR_HIP_TRY(h, hipMemcpyAsync(mask, d_m, (size_t)K, hipMemcpyDeviceToHost, s.stream));
  QTR_HIP_TRY(h, hipStreamSynchronize(s.stream));
  return QTR_OK;
}

int qtr_gnc_rotation2d(qtr_handle* h, int slot, const double* src2m, const double* dst2m, int M, double noise_bound,
                       double gnc_factor, int max_iterations, double cost_threshold, double* R4, double* cost,
                       int* iterations, unsigned char* inliers) {
  Slot* sp = get_slot(h, slot);
  if (!sp || M < 1 || !src2m || !dst2m || !R4 || !(gnc_factor > 1) || max_iterations < 1) return QTR_ERR_BAD_ARG;
  Slot& s = *sp;
  if (!stage_fits(h, s, (size_t)5 * M + 8, (size_t)(M + 3) / 4)) return QTR_ERR_CAPACITY;
  QTR_HIP_TRY(h, hipSetDevice(h->device));
  double* d_s = s.sb.f64;
  double* d_d = d_s + (size_t)2 * M;
  double* d_w = d_d + (size_t)2 * M;
  double* d_o = d_w + (size_t)M;
  unsigned char* d_i = (unsigned char*)s.sb.i32;
  QTR_HIP_TRY(h, hipMemcpyAsync(d_s, src2m, sizeof(double) * 2 * (size_t)M, hipMemcpyHostToDevice, s.stream));
  QTR_HIP_TRY(h, hipMemcpyAsync(d_d, dst2m, sizeof(double) * 2 * (size_t)M, hipMemcpyHostToDevice, s.stream));
  hipLaunchKernelGGL(k_gnc_only, dim3(1), dim3(64), 0, s.stream, d_s, d_d, M, noise_bound, gnc_factor, max_iterations,
                     cost_threshold, d_w, d_o, d_i);
  QTR_HIP_TRY(h, hipGetLastError());
  double out[6];
  QTR_HIP_TRY(h, hipMemcpyAsync(out, d_o, sizeof(out), hipMemcpyDeviceToHost, s.stream));
  if (inliers) QTR_HIP_TRY(h, hipMemcpyAsync(inliers, d_i, (size_t)M, hipMemcpyDeviceToHost, s.stream));
  QTR_HIP_TRY(h, hipStreamSynchronize(s.stream));
  for (int i = 0; i < 4; ++i) R4[i] = out[i];
  if (cost) *cost = out[4];
  if (iterations) *iterations = (int)out[5];
  return QTR_OK;
}

int qtr_gnc_rotation3d(qtr_handle* h, int slot, const double* src3m, const double* dst3m, int M, double noise_bound,
                       double gnc_factor, int max_iterations, double cost_threshold, double* R9, double* cost,
                       int* iterations, unsigned char* inliers) {
  Slot* sp = get_slot(h, slot);
  if (!sp || M < 1 || !src3m || !dst3m || !R9 || !(gnc_factor > 1) || max_iterations < 1) return QTR_ERR_BAD_ARG;
  Slot& s = *sp;
  if (!stage_fits(h, s, (size_t)7 * M + 16, (size_t)(M + 3) / 4)) return QTR_ERR_CAPACITY;
  QTR_HIP_TRY(h, hipSetDevice(h->device));
  double* d_s = s.sb.f64;
  double* d_d = d_s + (size_t)3 * M;
  double* d_w = d_d + (size_t)3 * M;
  double* d_o = d_w + (size_t)M;
  unsigned char* d_i = (unsigned char*)s.sb.i32;
  QTR_HIP_TRY(h, hipMemcpyAsync(d_s, src3m, sizeof(double) * 3 * (size_t)M, hipMemcpyHostToDevice, s.stream));
  QTR_HIP_TRY(h, hipMemcpyAsync(d_d, dst3m, sizeof(double) * 3 * (size_t)M, hipMemcpyHostToDevice, s.stream));
  hipLaunchKernelGGL(k_gnc3d_only, dim3(1), dim3(64), 0, s.stream, d_s, d_d, M, noise_bound, gnc_factor, max_iterations,
                     cost_threshold, d_w, d_o, d_i);
  QTR_HIP_TRY(h, hipGetLastError());
  double out[11];
  QTR_HIP_TRY(h, hipMemcpyAsync(out, d_o, sizeof(out), hipMemcpyDeviceToHost, s.stream));
  if (inliers) QTR_HIP_TRY(h, hipMemcpyAsync(inliers, d_i, (size_t)M, hipMemcpyDeviceToHost, s.stream));
  QTR_HIP_TRY(h, hipStreamSynchronize(s.stream));
  for (int i = 0; i < 9; ++i) R9[i] = out[i];
  if (cost) *cost = out[9];
  if (iterations) *iterations = (int)out[10];
  return QTR_OK;
}

static int cote_impl(qtr_handle* h, int slot, const double* X, const double* ranges, int N, double range,
                     int median_selection, double* estimate, unsigned char* inliers, int* n_card) {
  Slot* sp = get_slot(h, slot);
  if (!sp || N < 1 || !X) return QTR_ERR_BAD_ARG;
  Slot& s = *sp;
  if (!stage_fits(h, s, (size_t)16 * N + 8, (size_t)2 * N + (size_t)(N + 3) / 4)) return QTR_ERR_CAPACITY;
  QTR_HIP_TRY(h, hipSetDevice(h->device));
  double* d_x = s.sb.f64;
  double* d_r = d_x + (size_t)N;
  double* d_f = d_r + (size_t)N;
  double* d_o = d_f + (size_t)14 * N;
  int* d_si = s.sb.i32;
  unsigned char* d_i = (unsigned char*)(d_si + (size_t)2 * N);
  QTR_HIP_TRY(h, hipMemcpyAsync(d_x, X, sizeof(double) * (size_t)N, hipMemcpyHostToDevice, s.stream));
  if (ranges) QTR_HIP_TRY(h, hipMemcpyAsync(d_r, ranges, sizeof(double) * (size_t)N, hipMemcpyHostToDevice, s.stream));
  hipLaunchKernelGGL(k_cote_only, dim3(1), dim3(256), 0, s.stream, d_x, N, range, ranges ? d_r : (const double*)nullptr,
                     median_selection ? 1 : 0, d_f, d_si, d_o, d_i);
  QTR_HIP_TRY(h, hipGetLastError());
  double out[2];
  QTR_HIP_TRY(h, hipMemcpyAsync(out, d_o, sizeof(out), hipMemcpyDeviceToHost, s.stream));
  if (inliers) QTR_HIP_TRY(h, hipMemcpyAsync(inliers, d_i, (size_t)N, hipMemcpyDeviceToHost, s.stream));
  QTR_HIP_TRY(h, hipStreamSynchronize(s.stream));
  if (estimate) *estimate = out[0];
  if (n_card) *n_card = (int)out[1];
  return QTR_OK;
}

int qtr_cote_estimate(qtr_handle* h, int slot, const double* X, int N, double range, int median_selection,
                      double* estimate, unsigned char* inliers, int* n_card) {
  if (!(range > 0)) return QTR_ERR_BAD_ARG;
  return cote_impl(h, slot, X, nullptr, N, range, median_selection, estimate, inliers, n_card);
}

int qtr_cote_estimate_ranges(qtr_handle* h, int slot, const double* X, const double* ranges, int N, int median_selection,
                             double* estimate, unsigned char* inliers, int* n_card) {
  if (!ranges || N < 1) return QTR_ERR_BAD_ARG;
  for (int i = 0; i < N; ++i)
    if (!(ranges[i] > 0)) return QTR_ERR_BAD_ARG;
  return cote_impl(h, slot, X, ranges, N, ranges[0], median_selection, estimate, inliers, n_card);
}

// ------------------------------------------------------------------------------------------------
// Patchwork ground segmentation (patchwork.hip)
void qtr_pw_default_params(qtr_pw_params* p) {  // reference config/patchwork_params.yaml
  memset(p, 0, sizeof(*p));
  p->sensor_height = 1.723;
  p->num_iter = 3;
  p->num_lpr = 20;
  p->num_min_pts = 80;
  p->th_seeds = 0.25;
  p->th_dist = 0.125;
  p->max_range = 80.0;
  p->min_range = 2.7;
  p->uprightness_thr = 0.707;
  p->adaptive_seed_selection_margin = -1.1;
  p->using_global_thr = 0;
  p->global_elevation_thr = -0.5;
  p->num_zones = 4;
  const int ns[4] = {16, 32, 54, 32}, nr[4] = {2, 4, 4, 4};
  const double mr[4] = {2.7, 12.3625, 22.025, 41.35};
  const double et[4] = {-1.2, -0.9984, -0.851, -0.605}, ft[4] = {0.0001, 0.000125, 0.000185, 0.000185};
  for (int i = 0; i < 4; ++i) {
    p->num_sectors_each_zone[i] = ns[i];
    p->num_rings_each_zone[i] = nr[i];
    p->min_ranges[i] = mr[i];
    p->elevation_thr[i] = et[i];
    p->flatness_thr[i] = ft[i];
  }
  p->num_thr = 4;
}

// Ground segmentation of one scan in two halves, so that a batch can keep several slots' scans in flight: pw_begin
// validates and enqueues (the two output counts follow the kernels into the slot's pinned words, EV_STAGE_END marks the
// end), pw_end reads them once the stream has got there.
static int pw_begin(qtr_handle* h, Slot& s, const float* xyz4, int P, const qtr_pw_params* pw, int mem) {
  if (!pw || P < 0 || (P > 0 && !xyz4)) return QTR_ERR_BAD_ARG;
  // check_input_parameters_are_correct (:588-614) + what the kernels rely on
  bool ok = pw->num_zones >= 1 && pw->num_zones <= 4 && pw->num_thr >= 0 && pw->num_thr <= 8 && pw->num_iter >= 1 &&
            pw->num_lpr >= 1 && pw->min_range == pw->min_ranges[0] && pw->max_range > pw->min_range;
  int npatch = 0, nrings = 0;
  for (int k = 0; ok && k < pw->num_zones; ++k) {
    ok = pw->num_sectors_each_zone[k] >= 1 && pw->num_rings_each_zone[k] >= 1 &&
         (k == 0 || pw->min_ranges[k] > pw->min_ranges[k - 1]) && pw->min_ranges[k] < pw->max_range;
    npatch += pw->num_sectors_each_zone[k] * pw->num_rings_each_zone[k];
    nrings += pw->num_rings_each_zone[k];
  }
  if (ok) {  // the reference indexes the threshold vectors with ring + 2 * zone (:395)
    for (int k = 0, ci = 0; k < pw->num_zones; ++k)
      for (int r = 0; r < pw->num_rings_each_zone[k]; ++r, ++ci)
        if (ci < pw->num_thr && r + 2 * k >= pw->num_thr) ok = false;
  }
  if (!ok || npatch > 1024) {
    snprintf(h->err, sizeof(h->err), "Some parameters are wrong! the size of parameters should be same");
    return QTR_ERR_BAD_ARG;
  }
  if (P > h->lim.max_points) {
    snprintf(h->err, sizeof(h->err), "P=%d exceeds max_points=%d", P, h->lim.max_points);
    return QTR_ERR_CAPACITY;
  }
  QTR_HIP_TRY(h, hipSetDevice(h->device));
  if (!s.pw_arena) {
    QTR_HIP_TRY(h, hipMalloc(&s.pw_arena, patchwork_scratch_bytes(h->lim.max_points)));
    patchwork_carve(s.pwb, s.pw_arena, h->lim.max_points);
  }
  const float4* d_in = (const float4*)xyz4;
  if (mem == QTR_MEM_HOST && P > 0) {
    QTR_HIP_TRY(h, hipMemcpyAsync(s.in_src, xyz4, (size_t)P * 16, hipMemcpyHostToDevice, s.stream));
    d_in = s.in_src;
  }
  PwDev d;
  memset(&d, 0, sizeof(d));
  d.sensor_height = pw->sensor_height;
  d.num_iter = pw->num_iter;
  d.num_lpr = pw->num_lpr;
  d.num_min_pts = pw->num_min_pts;
  d.th_seeds = pw->th_seeds;
  d.th_dist = pw->th_dist;
  d.max_range = pw->max_range;
  d.min_range = pw->min_range;
  d.uprightness_thr = pw->uprightness_thr;
  d.margin = (pw->sensor_height == 0.0) ? -0.1 : pw->adaptive_seed_selection_margin * pw->sensor_height;  // :294
  d.using_global_thr = pw->using_global_thr;
  d.global_elevation_thr = pw->global_elevation_thr;
  d.num_zones = pw->num_zones;
  d.num_thr = pw->num_thr;
  for (int k = 0, rb = 0; k < pw->num_zones; ++k) {
    d.nsec[k] = pw->num_sectors_each_zone[k];
    d.nring[k] = pw->num_rings_each_zone[k];
    d.min_ranges[k] = pw->min_ranges[k];
    const double hi = (k + 1 < pw->num_zones) ? pw->min_ranges[k + 1] : pw->max_range;
    d.ring_size[k] = (hi - pw->min_ranges[k]) / pw->num_rings_each_zone[k];
    d.sector_size[k] = 2 * M_PI / pw->num_sectors_each_zone[k];
    d.base[k + 1] = d.base[k] + d.nring[k] * d.nsec[k];
    d.ring_base[k] = rb;
    rb += d.nring[k];
  }
  for (int i = 0; i < 8; ++i) {
    d.elevation_thr[i] = pw->elevation_thr[i];
    d.flatness_thr[i] = pw->flatness_thr[i];
  }
  QTR_HIP_TRY(h, hipEventRecord(s.ev[EV_STAGE_BEGIN], s.stream));
  QTR_HIP_TRY(h, patchwork_enqueue(s.fb, s.pwb, d_in, P, d, s.stream));
  QTR_HIP_TRY(h, hipMemcpyAsync(s.pinned_i32, s.pwb.offs + 2 * 1024, 2 * sizeof(int), hipMemcpyDeviceToHost, s.stream));
  QTR_HIP_TRY(h, hipEventRecord(s.ev[EV_STAGE_END], s.stream));
  return QTR_OK;
}
static void pw_end(Slot& s, int* n_ground, int* n_nonground) {  // (after s.ev[EV_STAGE_END] has completed)
  *n_ground = s.pinned_i32[0];
  *n_nonground = s.pinned_i32[1];
}

int qtr_patchwork(qtr_handle* h, int slot, const float* xyz4, int P, const qtr_pw_params* pw, float* ground_xyzw,
                  int cap_ground, int* n_ground, float* nonground_xyzw, int cap_nonground, int* n_nonground, int mem) {
  Slot* sp = get_slot(h, slot);
  if (!sp || !pw || !n_ground || !n_nonground || P < 0 || (P > 0 && !xyz4)) return QTR_ERR_BAD_ARG;
  Slot& s = *sp;
  *n_ground = *n_nonground = 0;
  QTR_TRY(pw_begin(h, s, xyz4, P, pw, mem));
  QTR_HIP_TRY(h, hipStreamSynchronize(s.stream));
  int ng = 0, nn = 0;
  pw_end(s, &ng, &nn);
  *n_ground = ng;
  *n_nonground = nn;
  if ((ground_xyzw && ng > cap_ground) || (nonground_xyzw && nn > cap_nonground)) {
    snprintf(h->err, sizeof(h->err), "output capacity too small (%d ground, %d non-ground)", ng, nn);
    return QTR_ERR_CAPACITY;
  }
  const hipMemcpyKind kout = mem == QTR_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
  if (ground_xyzw && ng > 0) QTR_HIP_TRY(h, hipMemcpyAsync(ground_xyzw, s.pwb.out_g, (size_t)ng * 16, kout, s.stream));
  if (nonground_xyzw && nn > 0) QTR_HIP_TRY(h, hipMemcpyAsync(nonground_xyzw, s.pwb.out_n, (size_t)nn * 16, kout, s.stream));
  QTR_HIP_TRY(h, hipStreamSynchronize(s.stream));
  times_one_stage(s, nullptr);
  return QTR_OK;
}

// ------------------------------------------------------------------------------------------------
// range-image projection + sub-cluster rejection (segment.hip)
int qtr_ip_default_params(const char* lidar, const char* nbr, qtr_ip_params* p) {
  if (!lidar || !nbr || !p) return QTR_ERR_BAD_ARG;
  struct Row {
    const char* name;
    int ns, hs;
    float rx, ry, ab;
  };
  const Row rows[] = {  // reference include/imageProjection.hpp:85-131
      {"Velodyne-64-HDE", 64, 1800, 360.0f / 1800.0f, 26.9f / 63.0f, 25.0f},
      {"VLP-16", 16, 1800, 0.2f, 2.0f, (float)(15.0 + 0.1)},
      {"HDL-32E", 32, 1800, 360.0f / 1800.0f, 41.33f / 31.0f, 30.67f},
      {"Ouster-OS1-16", 16, 1024, 360.0f / 1024.0f, 33.2f / 15.0f, (float)(16.6 + 0.1)},
      {"Ouster-OS1-64", 64, 1024, 360.0f / 1024.0f, 33.2f / 63.0f, (float)(16.6 + 0.1)},
  };
  const Row* r = nullptr;
  for (const Row& q : rows)
    if (strcmp(q.name, lidar) == 0) r = &q;
  int mode = -1;
  if (strcmp(nbr, "4Neighbor") == 0) mode = 0;
  if (strcmp(nbr, "8Neighbor") == 0) mode = 1;
  if (strcmp(nbr, "4CrossNeighbor") == 0) mode = 2;
  if (!r || mode < 0) return QTR_ERR_BAD_ARG;
  p->n_scan = r->ns;
  p->horizon_scan = r->hs;
  p->ang_res_x = r->rx;
  p->ang_res_y = r->ry;
  p->ang_bottom = r->ab;
  p->neighbor_mode = mode;
  p->num_min_pts = 30;
  p->segment_theta = (float)(60.0 / 180.0 * M_PI);
  p->valid_point_num = 5;
  p->valid_line_num = 3;
  return QTR_OK;
}

// (the same split as pw_begin / pw_end: three counts — valid points, outliers, segments — into the slot's pinned words)
static int seg_begin(qtr_handle* h, Slot& s, const float* xyz4, int P, const qtr_ip_params* ip, int mem) {
  if (!ip || P < 0 || (P > 0 && !xyz4)) return QTR_ERR_BAD_ARG;
  if (ip->n_scan < 1 || ip->n_scan > 64 || ip->horizon_scan < 4 || ip->horizon_scan > 8192 || !(ip->ang_res_x > 0) ||
      !(ip->ang_res_y > 0) || ip->neighbor_mode < 0 || ip->neighbor_mode > 2) {
    snprintf(h->err, sizeof(h->err), "[ImageProjection]:Check your paramter. (n_scan <= 64, horizon_scan <= 8192)");
    return QTR_ERR_BAD_ARG;
  }
  if (P > h->lim.max_points) {
    snprintf(h->err, sizeof(h->err), "P=%d exceeds max_points=%d", P, h->lim.max_points);
    return QTR_ERR_CAPACITY;
  }
  QTR_HIP_TRY(h, hipSetDevice(h->device));
  const int NP = ip->n_scan * ip->horizon_scan;
  if (!s.seg_arena || s.seg.np_cap < NP) {
    if (s.seg_arena) QTR_HIP_TRY(h, hipFree(s.seg_arena));
    s.seg_arena = nullptr;
    QTR_HIP_TRY(h, hipMalloc(&s.seg_arena, segment_scratch_bytes(NP)));
    segment_carve(s.seg, s.seg_arena, NP);
  }
  const float4* d_in = (const float4*)xyz4;
  if (mem == QTR_MEM_HOST && P > 0) {
    QTR_HIP_TRY(h, hipMemcpyAsync(s.in_src, xyz4, (size_t)P * 16, hipMemcpyHostToDevice, s.stream));
    d_in = s.in_src;
  }
  IpDev d;
  d.n_scan = ip->n_scan;
  d.horizon_scan = ip->horizon_scan;
  d.ang_res_x = ip->ang_res_x;
  d.ang_res_y = ip->ang_res_y;
  d.ang_bottom = ip->ang_bottom;
  d.neighbor_mode = ip->neighbor_mode;
  d.num_min_pts = ip->num_min_pts;
  d.segment_theta = ip->segment_theta;
  d.valid_point_num = ip->valid_point_num;
  d.valid_line_num = ip->valid_line_num;
  {  // segmentAlphaX / Y = ang_res / 180 * pi stored in float (:132-133); their sin / cos through qtr_math.h
    const float ax = (float)((double)ip->ang_res_x / 180.0 * M_PI), ay = (float)((double)ip->ang_res_y / 180.0 * M_PI);
    qm_sincosf(ax, &d.sx, &d.cx);
    qm_sincosf(ay, &d.sy, &d.cy);
  }
  QTR_HIP_TRY(h, hipEventRecord(s.ev[EV_STAGE_BEGIN], s.stream));
  int* d_tot = s.seg.blk + 3 * ((NP + 1023) / 1024 + 1);
  QTR_HIP_TRY(h, segment_enqueue(s.seg, d_in, P, d, d_tot, s.stream));
  QTR_HIP_TRY(h, hipMemcpyAsync(s.pinned_i32, d_tot, 3 * sizeof(int), hipMemcpyDeviceToHost, s.stream));
  QTR_HIP_TRY(h, hipEventRecord(s.ev[EV_STAGE_END], s.stream));
  return QTR_OK;
}

int qtr_segment_cloud(qtr_handle* h, int slot, const float* xyz4, int P, const qtr_ip_params* ip, float* valid_xyzl,
                      int cap_valid, int* n_valid, float* outl_xyzi, int cap_outl, int* n_outl, int* n_segments,
                      int* labelmat, int mem) {
  Slot* sp = get_slot(h, slot);
  if (!sp || !ip || !n_valid || P < 0 || (P > 0 && !xyz4)) return QTR_ERR_BAD_ARG;
  Slot& s = *sp;
  *n_valid = 0;
  if (n_outl) *n_outl = 0;
  if (n_segments) *n_segments = 0;
  QTR_TRY(seg_begin(h, s, xyz4, P, ip, mem));
  QTR_HIP_TRY(h, hipStreamSynchronize(s.stream));
  const int NP = ip->n_scan * ip->horizon_scan;
  const int nv = s.pinned_i32[0], no = s.pinned_i32[1], nseg = s.pinned_i32[2];
  *n_valid = nv;
  if (n_outl) *n_outl = no;
  if (n_segments) *n_segments = nseg;
  if ((valid_xyzl && nv > cap_valid) || (outl_xyzi && no > cap_outl)) {
    snprintf(h->err, sizeof(h->err), "output capacity too small (%d valid, %d outliers)", nv, no);
    return QTR_ERR_CAPACITY;
  }
  const hipMemcpyKind kout = mem == QTR_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
  if (valid_xyzl && nv > 0) QTR_HIP_TRY(h, hipMemcpyAsync(valid_xyzl, s.seg.out_valid, (size_t)nv * 16, kout, s.stream));
  if (outl_xyzi && no > 0) QTR_HIP_TRY(h, hipMemcpyAsync(outl_xyzi, s.seg.out_outl, (size_t)no * 16, kout, s.stream));
  if (labelmat) QTR_HIP_TRY(h, hipMemcpyAsync(labelmat, s.seg.labelmat, (size_t)NP * 4, hipMemcpyDeviceToHost, s.stream));
  QTR_HIP_TRY(h, hipStreamSynchronize(s.stream));
  times_one_stage(s, nullptr);
  return QTR_OK;
}

int qtr_set_stage_events(qtr_handle* h, int on) {
  if (!h) return QTR_ERR_BAD_ARG;
  h->stage_events = on ? 1 : 0;
  return QTR_OK;
}

int qtr_set_nn_event_stride(qtr_handle* h, int every) {
  if (!h || every < 0) return QTR_ERR_BAD_ARG;
  h->nn_event_stride = every;
  for (auto& s : h->slots) s.n_matches = 0;  // the next match of every slot is a timed one
  return QTR_OK;
}

int qtr_get_nn_dir_times(qtr_handle* h, int slot, float* dir1_ms, float* dir2_ms) {
  Slot* sp = peek_slot(h, slot);
  if (!sp) return QTR_ERR_BAD_ARG;
  if (sp->times_pending) {  // (the events of the last call are read on demand, like qtr_get_stage_times does)
    qtr_stage_times t;
    (void)qtr_get_stage_times(h, slot, &t);
  }
  if (dir1_ms) *dir1_ms = sp->nn_dir_ms[0];
  if (dir2_ms) *dir2_ms = sp->nn_dir_ms[1];
  return QTR_OK;
}

int qtr_get_nn_totals(qtr_handle* h, int slot, double* total_ms, long long* launches, int reset) {
  Slot* sp = peek_slot(h, slot);
  if (!sp) return QTR_ERR_BAD_ARG;
  (void)hipStreamSynchronize(sp->stream);
  flush_nn_totals(*sp);
  if (total_ms) *total_ms = sp->nn_total_ms;
  if (launches) *launches = sp->nn_total_launches;
  if (reset) {
    sp->nn_total_ms = 0;
    sp->nn_total_launches = 0;
  }
  return QTR_OK;
}

int qtr_get_stage_times(qtr_handle* h, int slot, qtr_stage_times* out) {
  Slot* sp = peek_slot(h, slot);
  if (!sp || !out) return QTR_ERR_BAD_ARG;
  compute_times(*sp);
  *out = sp->times;
  return QTR_OK;
}

// ------------------------------------------------------------------------------------------------
// front end
int qtr_voxelize(qtr_handle* h, int slot, const float* xyz4, int P, float leaf, float* out_xyz4, int cap, int* n_out,
                 int mem) {
  Slot* sp = get_slot(h, slot);
  if (!sp || !n_out || P < 0 || (P > 0 && (!xyz4 || !out_xyz4)) || !(leaf > 0)) return QTR_ERR_BAD_ARG;
  Slot& s = *sp;
  *n_out = 0;
  if (P == 0) return QTR_OK;
  if (P > h->lim.max_points) {
    snprintf(h->err, sizeof(h->err), "P=%d exceeds max_points=%d", P, h->lim.max_points);
    return QTR_ERR_CAPACITY;
  }
  QTR_HIP_TRY(h, hipSetDevice(h->device));
  const float4* d_in = (const float4*)xyz4;
  if (mem == QTR_MEM_HOST) {
    QTR_HIP_TRY(h, hipMemcpyAsync(s.in_src, xyz4, (size_t)P * 16, hipMemcpyHostToDevice, s.stream));
    d_in = s.in_src;
  }
  QTR_HIP_TRY(h, hipEventRecord(s.ev[EV_STAGE_BEGIN], s.stream));
  CloudBufs& cb = s.fb.cloud[0];
  {
    const float4* raws[1] = {d_in};
    const int Ps[1] = {P};
    QTR_HIP_TRY(h, voxelize_enqueue(s.fb, 1, raws, Ps, leaf, s.stream));
  }
  QTR_HIP_TRY(h, hipEventRecord(s.ev[EV_STAGE_END], s.stream));
  QTR_HIP_TRY(h, hipMemcpyAsync(s.pinned_i32, cb.counts, 16 * sizeof(int), hipMemcpyDeviceToHost, s.stream));
  QTR_HIP_TRY(h, hipStreamSynchronize(s.stream));
  const VoxVerdict v = vox_verdict(s.pinned_i32, P, h->lim.max_voxels);
  if (v.reason == VOX_TIMEOUT || s.pinned_i32[CNT_VOX_TAILERR]) {  // (the sticky word: ANY tile gave up, not only the last)
    snprintf(h->err, sizeof(h->err), "voxel grid: look-back timed out");
    return QTR_ERR_HIP;
  }
  // (a cloud that passed through goes out as it came in, whatever its size, and an empty result is no error here: the
  // bound below is the caller's capacity)
  const int n = v.n;
  const float4* d_out = v.passed ? d_in : cb.vox;
  if (v.reason == VOX_TOO_MANY) {
    snprintf(h->err, sizeof(h->err), "voxel count %d exceeds max_voxels=%d", n, h->lim.max_voxels);
    return QTR_ERR_CAPACITY;
  }
  if (n > cap) {
    snprintf(h->err, sizeof(h->err), "voxel count %d exceeds output capacity %d", n, cap);
    *n_out = n;
    return QTR_ERR_CAPACITY;
  }
  QTR_HIP_TRY(h, hipMemcpyAsync(out_xyz4, d_out, (size_t)n * 16,
                                mem == QTR_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, s.stream));
  QTR_HIP_TRY(h, hipStreamSynchronize(s.stream));
  *n_out = n;
  times_one_stage(s, &qtr_stage_times::voxelize);
  return QTR_OK;
}

int qtr_fpfh(qtr_handle* h, int slot, const float* xyz4, int n, float r_normal, float r_fpfh, float* normals4,
             float* desc33, int mem) {
  Slot* sp = get_slot(h, slot);
  if (!sp || n < 0 || (n > 0 && (!xyz4 || !desc33))) return QTR_ERR_BAD_ARG;
  if (r_normal > r_fpfh || !(r_normal > 0)) {  // reference include/fpfh_manager.hpp:99-102
    snprintf(h->err, sizeof(h->err), "[FPFHManager]: Normal should be lower than fpfh_radius!!!!");
    return QTR_ERR_BAD_ARG;
  }
  Slot& s = *sp;
  s.last_n = n;
  if (n == 0) return QTR_OK;
  if (n > h->lim.max_voxels) {
    snprintf(h->err, sizeof(h->err), "n=%d exceeds max_voxels=%d", n, h->lim.max_voxels);
    return QTR_ERR_CAPACITY;
  }
  QTR_HIP_TRY(h, hipSetDevice(h->device));
  CloudBufs& cb = s.fb.cloud[0];
  const hipMemcpyKind kin = mem == QTR_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
  const hipMemcpyKind kout = mem == QTR_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
  QTR_HIP_TRY(h, hipMemcpyAsync(cb.vox, xyz4, (size_t)n * 16, kin, s.stream));
  QTR_HIP_TRY(h, hipMemsetAsync(cb.counts, 0, 16 * sizeof(int), s.stream));
  QTR_HIP_TRY(h, set_count_enqueue(cb, CNT_NVOX, n, s.stream));
  QTR_HIP_TRY(h, hipEventRecord(s.ev[EV_STAGE_BEGIN], s.stream));
  {
    const int ns1[1] = {n};
    // an arbitrary cloud (dense mode: no voxel grid in front): lists of any length
    QTR_TRY(ensure_long_arenas(h, s));
    QTR_HIP_TRY(h, fpfh_enqueue(s.fb, 0, 1, ns1, r_normal, r_fpfh, s.stream, true, false, true));
  }
  QTR_HIP_TRY(h, hipEventRecord(s.ev[EV_STAGE_END], s.stream));
  QTR_HIP_TRY(h, hipMemcpyAsync(s.pinned_i32, cb.counts, 16 * sizeof(int), hipMemcpyDeviceToHost, s.stream));
  QTR_HIP_TRY(h, hipStreamSynchronize(s.stream));
  if (s.pinned_i32[CNT_NBR_CAPACITY]) {
    snprintf(h->err, sizeof(h->err), "radius-neighbour lists longer than %d entries need %d entries of the long-list arena "
             "(longest list %d); qtr_limits.max_long_neighbors is %d", QTR_KMAX, s.pinned_i32[CNT_NBR_ARENA],
             s.pinned_i32[CNT_KMAX], h->lim.max_long_neighbors);
    return QTR_ERR_CAPACITY;
  }
  if (normals4) QTR_HIP_TRY(h, hipMemcpyAsync(normals4, cb.normals, (size_t)n * 16, kout, s.stream));
  QTR_HIP_TRY(h, hipMemcpyAsync(desc33, cb.fpfh, (size_t)n * 33 * 4, kout, s.stream));
  QTR_HIP_TRY(h, hipStreamSynchronize(s.stream));
  times_one_stage(s, &qtr_stage_times::fpfh);
  return QTR_OK;
}

// Matching on device-resident clouds/descriptors held in fb.cloud[0] (source) and fb.cloud[1] (target).
// gather: the fused tail also leaves the matched clouds in s.m_src / s.m_tgt (match.hip, match_enqueue)
static int match_device(qtr_handle* h, Slot& s, int ns, int nt, const qtr_frontend_params* fp, int* L_out,
                        bool init_done = false, bool prep_done = false, bool tolerate_tail = false, bool gather = true) {
  flush_nn_totals(s);
  // (an event pair attached to a launch costs ~5 us of queue time on either side of it: a caller that only wants the
  // average duration of the launches — the bench's roofline — has every n-th match timed, qtr_set_nn_event_stride)
  const int stride = h->nn_event_stride;
  s.fb.nn_events = (stride > 0 && (s.n_matches++ % stride) == 0) ? 1 : 0;
  s.nn_timed_last = (s.fb.nn_events && s.fb.nn_engine != 0) ? 1 : 0;
  s.nn_pending = s.nn_timed_last;
  s.fb.mail_seq = ++s.seq;
  QTR_HIP_TRY(h, match_enqueue(s.fb, ns, nt, *fp, s.stream, init_done, prep_done, gather));
  QTR_TRY(wait_mail(h, s, s.stream, MAIL_SEQ_MATCH, s.seq));  // k_corr_compact2 left the counters in the mailbox
  *L_out = s.mail[MAIL_MATCH + MC_NCORR];
  if (*L_out < 0) {  // a multi-workgroup compaction of the tail gave up waiting for a predecessor's count (match.hip)
    if (tolerate_tail) return QTR_OK;  // (nobody reads the matcher's list: the caller reports -1 as the matched count)
    *L_out = 0;
    (void)hipStreamSynchronize(s.stream);
    snprintf(h->err, sizeof(h->err), "matcher tail: look-back timed out (no correspondences were written)");
    return QTR_ERR_HIP;
  }
  return QTR_OK;
}

int qtr_match(qtr_handle* h, int slot, const float* xyz4_s, int n_s, const float* desc33_s, const float* xyz4_t,
              int n_t, const float* desc33_t, const qtr_frontend_params* fp, int* corr2, int cap, int* L_out, int mem) {
  Slot* sp = get_slot(h, slot);
  if (!sp || !fp || !L_out || n_s < 0 || n_t < 0) return QTR_ERR_BAD_ARG;
  Slot& s = *sp;
  *L_out = 0;
  s.last_ns = n_s;
  s.last_nt = n_t;
  if (n_s == 0 || n_t == 0) return QTR_OK;
  if (!xyz4_s || !xyz4_t || !desc33_s || !desc33_t || !corr2) return QTR_ERR_BAD_ARG;
  if (n_s > h->lim.max_voxels || n_t > h->lim.max_voxels) {
    snprintf(h->err, sizeof(h->err), "cloud size exceeds max_voxels=%d", h->lim.max_voxels);
    return QTR_ERR_CAPACITY;
  }
  QTR_HIP_TRY(h, hipSetDevice(h->device));
  const hipMemcpyKind kin = mem == QTR_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
  const hipMemcpyKind kout = mem == QTR_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
  QTR_HIP_TRY(h, hipMemcpyAsync(s.fb.cloud[0].vox, xyz4_s, (size_t)n_s * 16, kin, s.stream));
  QTR_HIP_TRY(h, hipMemcpyAsync(s.fb.cloud[1].vox, xyz4_t, (size_t)n_t * 16, kin, s.stream));
  QTR_HIP_TRY(h, hipMemcpyAsync(s.fb.cloud[0].fpfh, desc33_s, (size_t)n_s * 132, kin, s.stream));
  QTR_HIP_TRY(h, hipMemcpyAsync(s.fb.cloud[1].fpfh, desc33_t, (size_t)n_t * 132, kin, s.stream));
  QTR_HIP_TRY(h, hipEventRecord(s.ev[EV_STAGE_BEGIN], s.stream));
  {
    const int n2[2] = {n_s, n_t};  // Matcher::normalizePoints means of the two clouds handed in
    QTR_HIP_TRY(h, mean_enqueue(s.fb, 0, 2, n2, s.stream));
  }
  int L = 0;
  int rc = match_device(h, s, n_s, n_t, fp, &L);
  if (rc != QTR_OK) return rc;
  QTR_HIP_TRY(h, hipEventRecord(s.ev[EV_STAGE_END], s.stream));
  *L_out = L;
  if (L > cap) {
    snprintf(h->err, sizeof(h->err), "L=%d exceeds output capacity %d", L, cap);
    return QTR_ERR_CAPACITY;
  }
  if (L > 0) QTR_HIP_TRY(h, hipMemcpyAsync(corr2, s.fb.corr, (size_t)L * 8, kout, s.stream));
  QTR_HIP_TRY(h, hipStreamSynchronize(s.stream));
  times_one_stage(s, &qtr_stage_times::match);
  fill_nn_times(s);
  return QTR_OK;
}

// The slot's third stream and its events, on the slot's first qtr_register_pair_corr (not in every slot of a batch handle).
// The front end is the critical path and the second stream already has the highest priority: this one takes the LOWEST
// (a queue pool of its own, and the front end's workgroups go first wherever both wait for a unit).
static int ensure_stream3(qtr_handle* h, Slot& s) {
  if (s.stream3) return QTR_OK;
  int prio_least = 0, prio_greatest = 0;
  QTR_HIP_TRY(h, hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
  if (!s.ev_fork) QTR_HIP_TRY(h, hipEventCreateWithFlags(&s.ev_fork, hipEventDisableTiming));
  if (!s.ev_join) QTR_HIP_TRY(h, hipEventCreateWithFlags(&s.ev_join, hipEventDisableTiming));
  if (prio_greatest != prio_least) QTR_HIP_TRY(h, hipStreamCreateWithPriority(&s.stream3, hipStreamNonBlocking, prio_least));
  else QTR_HIP_TRY(h, hipStreamCreateWithFlags(&s.stream3, hipStreamNonBlocking));
  return QTR_OK;
}

// qtr_register_pair_corr's back end, enqueued by front_device right behind the voxel stage's launches: it reads the
// caller's correspondences alone, so it runs on the third stream while the front end runs on the other two.
struct CorrEarly {
  const float* src = nullptr;  // the caller's correspondences (mem: where they live)
  const float* tgt = nullptr;
  int n = 0, mem = QTR_MEM_HOST;
  const qtr_params* prm = nullptr;
  bool enqueued = false;       // once per call: not again when the voxel sort or the long-list verdict goes round
  int seq = 0;                 // the sequence number its k_finalize publishes (the front end advances s.seq afterwards)
  const float4 *cs = nullptr, *ct = nullptr;  // where the back end reads them
  std::unique_ptr<InFlight> in_flight;        // held until its mail is in (or the chain has drained)
};
static int corr_early_enqueue(qtr_handle* h, Slot& s, CorrEarly& ce) {
  ce.enqueued = true;
  const bool ev_on = h->stage_events != 0;
  // The back end used to run on s.stream, behind everything the slot's stream already held: the device outputs of an earlier
  // call on the slot (qtr_feature_pair's keypoints, still being copied out of m_src / m_tgt), a caller's own matcher that
  // writes the correspondences on qtr_slot_stream.  It still does: the third stream waits for the event front_device
  // recorded on s.stream at the call's start — earlier work on the slot, not this call's voxel stage.
  QTR_HIP_TRY(h, hipStreamWaitEvent(s.stream3, s.ev_fork, 0));
  if (ev_on) QTR_HIP_TRY(h, hipEventRecord(s.ev[EV_BE0], s.stream3));
  QTR_TRY(corr_stage(h, s, ce.src, ce.tgt, ce.n, ce.mem, s.stream3, &ce.cs, &ce.ct));
  // (the slot's record of its last solve follows the solver's buffers, which this chain fills even when the front end
  // then fails and the call returns counts and status only; the serial order leaves it untouched on such a failure)
  s.last_L = ce.n;
  s.last_Wb = (((ce.n + 63) / 64) + 3) & ~3;
  s.sb.mail_seq = ce.seq = ++s.seq;
  ce.in_flight.reset(new InFlight(h));
  // (the state's clean slate rides on the graph build, as in qtr_solve: the matcher's k_match_init leaves it alone)
  QTR_HIP_TRY(h, solver_enqueue(s.sb, ce.cs, ce.ct, ce.n, *ce.prm, s.stream3, ev_on ? s.ev[EV_GRAPH] : nullptr,
                                ev_on ? s.ev[EV_CLIQUE] : nullptr, false, true));
  if (ev_on) QTR_HIP_TRY(h, hipEventRecord(s.ev[EV_SOLVE], s.stream3));
  return QTR_OK;
}

// ---- what the pair path (front_device) and the one-cloud path (front_one_chain) share: nc = 2 or 1 clouds ----
// the counts of a front end's nc clouds for a refusal's text: "a", or the pair's form of "a" and "b"
struct CountsText {
  char s[40];
  CountsText(int nc, int a, int b, const char* pair_form = "%d / %d") { snprintf(s, sizeof(s), nc > 1 ? pair_form : "%d", a, b); }
};

// The voxel stage of nc clouds on the slot's stream, the radix passes of the voxel sort speculated (vox_passes_next): the
// launch, behind() once per attempt right behind it (what the caller runs beside the stage), the wait for the nc voxel
// mails.  k2_vox_centroids publishes the counters from its first block while other blocks may still be reading the raw
// scans: a failed wait drains the stream before it hands the scans back to the caller (who may free them).
extern "C++" {  // (a template, inside this file's extern "C")
template <class Behind>
static int voxel_stage(qtr_handle* h, Slot& s, int nc, const float4* const* raws, const int* P, const qtr_frontend_params* fp,
                       Behind behind) {
  for (int attempt = 0;; ++attempt) {
    const int launched = s.fb.vox_passes;
    const int vox_seq = s.fb.mail_seq = ++s.seq;  // (kept: behind() may take the next number)
    QTR_HIP_TRY(h, voxelize_enqueue(s.fb, nc, raws, P, fp->voxel_size, s.stream, launched, fp->fpfh_radius * 1.001f));
    QTR_TRY(behind());
    int bits = 0;
    for (int c = 0; c < nc; ++c) {
      const int rc = wait_mail(h, s, s.stream, c ? MAIL_SEQ_VOX1 : MAIL_SEQ_VOX0, vox_seq);
      if (rc != QTR_OK) {
        (void)hipStreamSynchronize(s.stream);
        return rc;
      }
      const int b = s.mail[(c ? MAIL_VOX1 : MAIL_VOX0) + CNT_SORT_BITS];
      bits = c ? std::max(bits, b) : b;
    }
    if (!vox_passes_next(s.fb.vox_passes, s.fb.vox_fewer, bits, launched, attempt)) return QTR_OK;
  }
}
}  // extern "C++"

// The voxel stage's refusal from the verdicts of its nc clouds of P[] points, the reasons in vox_verdict's order (QTR_OK:
// none).  empty_is_error: an empty result is one — a keyframe; the pair path does not look at it.  A refusal drains the
// stream first, like a failed wait above.
static int vox_refusal(qtr_handle* h, Slot& s, int nc, const VoxVerdict* v, const int* P, bool empty_is_error) {
  auto any = [&](VoxReason r) { return v[0].reason == r || v[nc - 1].reason == r; };
  int rc = QTR_OK;
  if (any(VOX_TIMEOUT)) {
    snprintf(h->err, sizeof(h->err), "voxel grid: look-back timed out");
    rc = QTR_ERR_HIP;
  } else if (any(VOX_PASS_TOO_LARGE)) {
    snprintf(h->err, sizeof(h->err), "voxel grid would overflow int32 (leaf too small): the cloud passes through as it "
             "is (pcl::VoxelGrid), and its %s points exceed max_voxels=%d", CountsText(nc, P[0], P[nc - 1]).s, h->lim.max_voxels);
    rc = QTR_ERR_CAPACITY;
  } else if (any(VOX_TOO_MANY)) {
    snprintf(h->err, sizeof(h->err), "voxel count %s exceeds max_voxels=%d", CountsText(nc, v[0].n, v[nc - 1].n, "(%d,%d)").s,
             h->lim.max_voxels);
    rc = QTR_ERR_CAPACITY;
  } else if (empty_is_error && any(VOX_EMPTY)) {
    snprintf(h->err, sizeof(h->err), "Invalid or empty point cloud dataset given!");
    rc = QTR_ERR_BAD_ARG;
  }
  if (rc != QTR_OK) (void)hipStreamSynchronize(s.stream);
  return rc;
}

// The neighbour lists' refusal after an FPFH chain, from the counter lines of its nc clouds (lists_verdict).  *again: a
// point has more than QTR_KMAX neighbours and the chain ran without k2_neighbors_big — from now on the handle's chains
// include it, and the caller goes round again (its input is where it was: nothing of the chain writes it).
static int lists_refusal(qtr_handle* h, int nc, const int* cnt0, const int* cnt1, bool* again) {
  *again = false;
  switch (lists_verdict(cnt0, nc > 1 ? cnt1 : nullptr, h->long_lists)) {
    case LISTS_TILE_ERROR:
      snprintf(h->err, sizeof(h->err), "voxel grid: look-back timed out in a tile (centroids incomplete)");
      return QTR_ERR_HIP;
    case LISTS_CAPACITY:
      snprintf(h->err, sizeof(h->err), "radius-neighbour lists longer than %d entries (longest %s) exceed the long-list "
               "arena: qtr_limits.max_long_neighbors is %d", QTR_KMAX,
               CountsText(nc, cnt0[CNT_KMAX], nc > 1 ? cnt1[CNT_KMAX] : 0).s, h->lim.max_long_neighbors);
      return QTR_ERR_CAPACITY;
    case LISTS_NEED_LONG: h->long_lists = *again = true; break;
    case LISTS_OK: break;
  }
  return QTR_OK;
}

// Front end of one pair on one slot: voxel grid x2 -> FPFH x2 -> reciprocal matching -> matched keypoint clouds gathered
// into s.m_src / s.m_tgt (device).  What the reference does in `voxelize` x2 (include/quatro.hpp:49-68) +
// FPFHManager::setFeaturePair (include/fpfh_manager.hpp:98-153).  Counts go to *ns_out / *nt_out / *L_out; with
// `for_solver` the solver's clean slate is enqueued beside the FPFH chain (qtr_register_pair).  An error return leaves
// nothing in flight that still reads the caller's scans.
static int front_device(qtr_handle* h, Slot& s, const float* src_raw4, int Ps, const float* tgt_raw4, int Pt,
                        const qtr_frontend_params* fp, int mem, bool for_solver, int* ns_out, int* nt_out, int* L_out,
                        bool corr_given = false, CorrEarly* early = nullptr) {
  // corr_given: the back end will run on the CALLER's correspondences — the matcher's list is only counted (*L_out; -1 when
  // its tail gave up), so neither a list longer than max_corr nor a tail failure fails the registration, and the matched
  // clouds are not gathered.
  // early (with corr_given, for_solver = false): that back end is enqueued HERE, on the third stream, behind the first voxel
  // stage's launches — after every check that returns with nothing in flight, and while the host would only wait for the
  // voxel mail.  The caller waits for its mail, joins the streams and drains the third one on an error return.
  if (fp->normal_radius > fp->fpfh_radius) {
    snprintf(h->err, sizeof(h->err), "[FPFHManager]: Normal should be lower than fpfh_radius!!!!");
    return QTR_ERR_BAD_ARG;
  }
  if (Ps <= 0 || Pt <= 0 || !src_raw4 || !tgt_raw4) {
    snprintf(h->err, sizeof(h->err), "Invalid or empty point cloud dataset given!");
    return QTR_ERR_BAD_ARG;
  }
  if (Ps > h->lim.max_points || Pt > h->lim.max_points) {
    snprintf(h->err, sizeof(h->err), "cloud exceeds max_points=%d", h->lim.max_points);
    return QTR_ERR_CAPACITY;
  }
  QTR_HIP_TRY(h, hipSetDevice(h->device));
  if (early && !early->enqueued) {  // the fork of the third stream: in front of everything this call puts on s.stream
    QTR_TRY(ensure_stream3(h, s));
    QTR_HIP_TRY(h, hipEventRecord(s.ev_fork, s.stream));
  }
  const float4 *d_s = (const float4*)src_raw4, *d_t = (const float4*)tgt_raw4;
  if (mem == QTR_MEM_HOST) {
    QTR_HIP_TRY(h, hipMemcpyAsync(s.in_src, src_raw4, (size_t)Ps * 16, hipMemcpyHostToDevice, s.stream));
    QTR_HIP_TRY(h, hipMemcpyAsync(s.in_tgt, tgt_raw4, (size_t)Pt * 16, hipMemcpyHostToDevice, s.stream));
    d_s = s.in_src;
    d_t = s.in_tgt;
  }
  if (h->stage_events) QTR_HIP_TRY(h, hipEventRecord(s.ev[EV_BEGIN], s.stream));
  // both clouds go through every front-end kernel together (blockIdx.y = cloud)
  const float4* raws[2] = {d_s, d_t};
  const int P2[2] = {Ps, Pt};
  auto beside_voxels = [&]() -> int {
    // block 0 of k2_vox_centroids publishes the counters while other blocks are still writing centroids: anything
    // that reads the centroids from another stream has to wait for the kernel itself
    QTR_HIP_TRY(h, hipEventRecord(s.ev_vox, s.stream));
    // The matcher's sequential means (70 us of one dependent chain per cloud: as long as the whole FPFH chain since round
    // 6's cuts) start right behind the centroids, on the second stream, with the voxel counts read on the device — not
    // after the mail, the host's checks and the FPFH chain's ten launches.
    const int on_device[2] = {-1, -1};
    QTR_HIP_TRY(h, hipStreamWaitEvent(s.stream2, s.ev_vox, 0));
    QTR_HIP_TRY(h, mean_enqueue(s.fb, 0, 2, on_device, s.stream2, h->lim.max_voxels));
    if (early && !early->enqueued) QTR_TRY(corr_early_enqueue(h, s, *early));
    return QTR_OK;
  };
  QTR_TRY(voxel_stage(h, s, 2, raws, P2, fp, beside_voxels));
  // (a cloud that passes through is BASELINE's dense mode — "no voxel downsample" — through the whole-path entry; an empty
  // voxel result is not looked at on this path)
  const VoxVerdict v2[2] = {vox_verdict(s.mail + MAIL_VOX0, Ps, h->lim.max_voxels),
                            vox_verdict(s.mail + MAIL_VOX1, Pt, h->lim.max_voxels)};
  QTR_TRY(vox_refusal(h, s, 2, v2, P2, false));
  const VoxVerdict &vs = v2[0], &vt = v2[1];
  const int ns = vs.n, nt = vt.n;
  const bool passed_through = vs.passed || vt.passed;
  if (vs.passed) QTR_HIP_TRY(h, hipMemcpyAsync(s.fb.cloud[0].vox, d_s, (size_t)Ps * 16, hipMemcpyDeviceToDevice, s.stream));
  if (vt.passed) QTR_HIP_TRY(h, hipMemcpyAsync(s.fb.cloud[1].vox, d_t, (size_t)Pt * 16, hipMemcpyDeviceToDevice, s.stream));
  if (passed_through) QTR_HIP_TRY(h, hipEventRecord(s.ev_vox, s.stream));  // (the second stream's means wait for the clouds)
  *ns_out = ns;
  *nt_out = nt;
  s.last_ns = ns;
  s.last_nt = nt;
  if (h->stage_events) QTR_HIP_TRY(h, hipEventRecord(s.ev[EV_VOX], s.stream));
  {
    const int n2[2] = {ns, nt};
    // Beside the FPFH chain, on the second stream: the matcher's sequential means (already running: enqueued behind the
    // voxel stage above; a cloud that passed through is summed again from the copy), and the matcher's and the solver's
    // clean slates (they depend on the voxel counts alone).
    if (passed_through) {
      QTR_HIP_TRY(h, hipStreamWaitEvent(s.stream2, s.ev_vox, 0));
      QTR_HIP_TRY(h, mean_enqueue(s.fb, 0, 2, n2, s.stream2));
    }
    if (h->long_lists) QTR_TRY(ensure_long_arenas(h, s));
    // (k2_fpfh also does the matcher's per-descriptor preparation: norms, hashes, duplicate table — see frontend.hip)
    QTR_HIP_TRY(h, fpfh_enqueue(s.fb, 0, 2, n2, fp->normal_radius, fp->fpfh_radius, s.stream, false, true, h->long_lists, true,
                                cell_table_cells(s.mail[MAIL_VOX0 + CNT_NCELL], s.mail[MAIL_VOX1 + CNT_NCELL])));
    // (the solver's clean slate rides in the matcher's: one launch fewer beside the FPFH chain)
    QTR_HIP_TRY(h, match_init_enqueue(s.fb, ns, nt, *fp, s.stream2, false, for_solver ? (int*)s.sb.st : nullptr,
                                      (int)(sizeof(SolverState) / 4)));
    QTR_HIP_TRY(h, hipEventRecord(s.ev[EV_JOIN2], s.stream2));
    QTR_HIP_TRY(h, hipStreamWaitEvent(s.stream, s.ev[EV_JOIN2], 0));
  }
  if (h->stage_events) QTR_HIP_TRY(h, hipEventRecord(s.ev[EV_FPFH], s.stream));
  int L = 0;
  // (with the back end beside this chain the matcher's tail does not gather its matched clouds: nobody reads them, and
  // host correspondences are staged in m_src / m_tgt while it runs)
  QTR_TRY(match_device(h, s, ns, nt, fp, &L, true, true, corr_given, early == nullptr));
  bool again = false;
  QTR_TRY(lists_refusal(h, 2, s.mail + MAIL_CNT0, s.mail + MAIL_CNT1, &again));  // (the matcher's tail mails the lines)
  if (again)  // (the early back end is not enqueued a second time: CorrEarly::enqueued)
    return front_device(h, s, src_raw4, Ps, tgt_raw4, Pt, fp, mem, for_solver, ns_out, nt_out, L_out, corr_given, early);
  *L_out = L;
  if (corr_given) {
    if (h->stage_events) QTR_HIP_TRY(h, hipEventRecord(s.ev[EV_MATCH], s.stream));  // (stage times: the matcher's end)
    return QTR_OK;
  }
  s.last_L = L;
  QTR_TRY(check_max_corr(h, L));
  QTR_HIP_TRY(h, gather_matched_enqueue(s.fb, L, s.m_src, s.m_tgt, s.stream));
  if (h->stage_events) QTR_HIP_TRY(h, hipEventRecord(s.ev[EV_MATCH], s.stream));
  return QTR_OK;
}

// a registration that got through its front end leaves its voxel clouds, the target normals and T for qtr_refine_pair
static void mark_registration(Slot& s, int rc, const qtr_result* res) {
  if (rc != QTR_OK && rc != QTR_ERR_CLIQUE_TOO_SMALL) return;
  s.reg_ready = 1;
  for (int k = 0; k < 16; ++k) s.reg_T[k] = res->T[k];
}

// The whole path on one slot.  mem_in: where the scans live; mem_out: where the index lists go and where the caller's
// correspondences are.  corr_src / corr_tgt (n_corr >= 0): the back end runs on THESE matched clouds instead of the
// matcher's output (qtr_register_pair_corr, the batched entry's "scans + pre-matched correspondences" pairs), and the
// record's n_corr is n_corr whatever happens; *n_matched (may be null) then receives the matcher's count (-1: its tail gave
// up — its list is not used).  n_corr < 0: the matcher's own correspondences.
// That back end needs nothing of the front end, so it is enqueued on the slot's third stream as soon as the voxel stage
// is on its way (front_device, CorrEarly) and the two chains share the device; the streams are joined before anything on
// s.stream reads the solver's buffers, and before every return.  QTR_CORR_OVERLAP=0 (read at qtr_create) keeps the serial
// order: staged and enqueued behind the front end, on s.stream.
static int register_pair_impl(qtr_handle* h, Slot& s, const float* src_raw4, int Ps, const float* tgt_raw4, int Pt,
                              const qtr_frontend_params* fp, const qtr_params* prm, qtr_result* res, int* clique,
                              int* final_inliers, int cap, int mem_in, int mem_out, const float* corr_src,
                              const float* corr_tgt, int n_corr, int* n_matched = nullptr) {
  const bool given = n_corr >= 0;
  int L = 0;
  if (given && h->corr_overlap) {
    CorrEarly ce{corr_src, corr_tgt, n_corr, mem_out, prm};
    int rc = front_device(h, s, src_raw4, Ps, tgt_raw4, Pt, fp, mem_in, false, &res->n_src, &res->n_tgt, &L, true, &ce);
    if (n_matched) *n_matched = L;
    res->n_corr = n_corr;
    if (!ce.enqueued) return res->status = rc;  // (a check in front of the first launch: nothing is in flight)
    // every return from here on leaves the third stream drained: the caller may free or overwrite the correspondences,
    // and nothing else on the slot waits for that stream (the successful return has synchronised s.stream behind the join)
    struct DrainOnReturn {
      hipStream_t st;
      bool armed = true;
      ~DrainOnReturn() {
        if (armed) (void)hipStreamSynchronize(st);
      }
    } drain{s.stream3};
    // the third stream's work is waited for and watched there
    if (rc == QTR_OK) rc = wait_mail(h, s, s.stream3, MAIL_SEQ_SOLVE, ce.seq);
    if (rc == QTR_OK) rc = solve_followup(h, s, ce.cs, ce.ct, n_corr, prm, s.stream3, h->stage_events != 0);
    if (rc != QTR_OK) {
      // The front end failed behind the back end's enqueue (capacity, a look-back timeout, the long-list arena), or a wait
      // did: today's record — counts and status — and nothing of the solver.  The abandoned chain drains before the
      // caller gets its correspondences back (drain), and its mail carries a sequence number no later call waits for.
      return res->status = rc;
    }
    ce.in_flight.reset();
    result_from_mail(s, res);
    rc = res->status;
    // the next call on the slot, qtr_refine_pair and device outputs are ordered on s.stream: it sees the finished back end
    QTR_HIP_TRY(h, hipEventRecord(s.ev_join, s.stream3));
    QTR_HIP_TRY(h, hipStreamWaitEvent(s.stream, s.ev_join, 0));
    if (h->stage_events) QTR_HIP_TRY(h, hipEventRecord(s.ev[EV_END], s.stream));
    rc = finish_registration(h, s, rc, TIMES_PAIR_OVERLAP, res, clique, nullptr, final_inliers, cap, mem_out, s.stream);
    // (a record whose lists are out has synchronised s.stream, which waited for the join)
    drain.armed = rc != QTR_OK && rc != QTR_ERR_CLIQUE_TOO_SMALL;
    return rc;
  }
  int rc = front_device(h, s, src_raw4, Ps, tgt_raw4, Pt, fp, mem_in, true, &res->n_src, &res->n_tgt, &L, given);
  if (n_matched) *n_matched = L;
  res->n_corr = given ? n_corr : L;
  if (rc != QTR_OK) return res->status = rc;
  const float4 *cs = s.m_src, *ct = s.m_tgt;
  if (given) QTR_TRY(corr_stage(h, s, corr_src, corr_tgt, n_corr, mem_out, s.stream, &cs, &ct));
  rc = solve_device(h, s, cs, ct, res->n_corr, prm, res, true);
  return finish_registration(h, s, rc, TIMES_PAIR, res, clique, nullptr, final_inliers, cap, mem_out, s.stream);
}

int qtr_register_pair(qtr_handle* h, int slot, const float* src_raw4, int Ps, const float* tgt_raw4, int Pt,
                      const qtr_frontend_params* fp, const qtr_params* prm, qtr_result* res, int* clique,
                      int* final_inliers, int cap, int mem) {
  Slot* sp = get_slot(h, slot);
  if (!sp || !res || !fp) return QTR_ERR_BAD_ARG;
  memset(res, 0, sizeof(*res));
  const int rc = check_params(h, prm);
  if (rc != QTR_OK) return res->status = rc;
  const int rc2 = register_pair_impl(h, *sp, src_raw4, Ps, tgt_raw4, Pt, fp, prm, res, clique, final_inliers, cap, mem, mem,
                                     nullptr, nullptr, -1);
  mark_registration(*sp, rc2, res);
  return rc2;
}

int qtr_register_pair_corr(qtr_handle* h, int slot, const float* src_raw4, int Ps, const float* tgt_raw4, int Pt,
                           const qtr_frontend_params* fp, const float* corr_src4, const float* corr_tgt4, int n_corr,
                           const qtr_params* prm, qtr_result* res, int* n_matched, int* clique, int* final_inliers, int cap,
                           int mem) {
  Slot* sp = get_slot(h, slot);
  if (!sp || !res || !fp) return QTR_ERR_BAD_ARG;
  Slot& s = *sp;
  memset(res, 0, sizeof(*res));
  if (n_matched) *n_matched = 0;
  int rc = check_params(h, prm);
  if (rc != QTR_OK) return res->status = rc;
  if (n_corr < 0 || (n_corr > 0 && (!corr_src4 || !corr_tgt4))) {
    snprintf(h->err, sizeof(h->err), "bad correspondence clouds");
    return res->status = QTR_ERR_BAD_ARG;
  }
  if (n_corr > h->lim.max_corr) {
    snprintf(h->err, sizeof(h->err), "n_corr=%d exceeds max_corr=%d", n_corr, h->lim.max_corr);
    return res->status = QTR_ERR_CAPACITY;
  }
  rc = register_pair_impl(h, s, src_raw4, Ps, tgt_raw4, Pt, fp, prm, res, clique, final_inliers, cap, mem, mem, corr_src4,
                          corr_tgt4, n_corr, n_matched);
  mark_registration(s, rc, res);
  return rc;
}

int qtr_feature_pair(qtr_handle* h, int slot, const float* src_raw4, int Ps, const float* tgt_raw4, int Pt,
                     const qtr_frontend_params* fp, int* n_src, int* n_tgt, int* L_out, float* src_kps4, float* tgt_kps4,
                     int* corr2, int cap, int mem) {
  Slot* sp = get_slot(h, slot);
  if (!sp || !fp || !L_out) return QTR_ERR_BAD_ARG;
  Slot& s = *sp;
  int ns = 0, nt = 0, L = 0;
  *L_out = 0;
  const int rc = front_device(h, s, src_raw4, Ps, tgt_raw4, Pt, fp, mem, false, &ns, &nt, &L);
  if (n_src) *n_src = ns;
  if (n_tgt) *n_tgt = nt;
  *L_out = L;
  if (rc != QTR_OK) return rc;
  s.times_pending = h->stage_events ? TIMES_FRONT : TIMES_EVENTS_OFF;
  if ((src_kps4 || tgt_kps4 || corr2) && L > cap) {
    snprintf(h->err, sizeof(h->err), "L=%d exceeds output capacity %d", L, cap);
    return QTR_ERR_CAPACITY;
  }
  const hipMemcpyKind kout = mem == QTR_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
  if (L > 0) {
    if (src_kps4) QTR_HIP_TRY(h, hipMemcpyAsync(src_kps4, s.m_src, (size_t)L * 16, kout, s.stream));
    if (tgt_kps4) QTR_HIP_TRY(h, hipMemcpyAsync(tgt_kps4, s.m_tgt, (size_t)L * 16, kout, s.stream));
    if (corr2) QTR_HIP_TRY(h, hipMemcpyAsync(corr2, s.fb.corr, (size_t)L * 8, kout, s.stream));
  }
  // host outputs are complete on return; device outputs are ordered on the slot's stream (qtr_slot_stream), like the
  // next call on this slot
  if (mem == QTR_MEM_HOST) QTR_HIP_TRY(h, hipStreamSynchronize(s.stream));
  return QTR_OK;
}

// ------------------------------------------------------------------------------------------------
// keyframes (keyframe.hip): one scan's front end, kept on the device
// The one-cloud front end on cloud[0] of a slot: voxel grid -> mean -> FPFH chain with the matcher's per-descriptor
// preparation, decided by the verdicts front_device uses (front_verdict.h).  The
// counters a whole-path call receives in its matcher's mail are read back here: nothing runs a matcher.
// What the one-cloud front end refuses before anything is enqueued.
static int front_one_check(qtr_handle* h, bool have_cloud, int P, const qtr_frontend_params* fp) {
  if (fp->normal_radius > fp->fpfh_radius) {
    snprintf(h->err, sizeof(h->err), "[FPFHManager]: Normal should be lower than fpfh_radius!!!!");
    return QTR_ERR_BAD_ARG;
  }
  if (P <= 0 || !have_cloud) {
    snprintf(h->err, sizeof(h->err), "Invalid or empty point cloud dataset given!");
    return QTR_ERR_BAD_ARG;
  }
  if (P > h->lim.max_points) {
    snprintf(h->err, sizeof(h->err), "cloud exceeds max_points=%d", h->lim.max_points);
    return QTR_ERR_CAPACITY;
  }
  return QTR_OK;
}

// The chain itself, on P points that are in device memory — or on their way there on the slot's stream (a staged host scan,
// the gathered voxels of a merge): front_one_check passed and the device is set.
static int front_one_chain(qtr_handle* h, Slot& s, const float4* d_raw, int P, const qtr_frontend_params* fp, int* n_out,
                           int* passed_out) {
  QTR_TRY(voxel_stage(h, s, 1, &d_raw, &P, fp, [] { return (int)QTR_OK; }));
  const VoxVerdict v = vox_verdict(s.mail + MAIL_VOX0, P, h->lim.max_voxels);
  QTR_TRY(vox_refusal(h, s, 1, &v, &P, true));
  const int n = v.n;
  if (v.passed) QTR_HIP_TRY(h, hipMemcpyAsync(s.fb.cloud[0].vox, d_raw, (size_t)P * 16, hipMemcpyDeviceToDevice, s.stream));
  s.last_ns = s.last_n = n;
  s.last_nt = 0;
  QTR_HIP_TRY(h, mean_enqueue(s.fb, 0, 1, &n, s.stream));
  if (h->long_lists) QTR_TRY(ensure_long_arenas(h, s));
  const int ncell = s.mail[MAIL_VOX0 + CNT_NCELL];
  QTR_HIP_TRY(h, fpfh_enqueue(s.fb, 0, 1, &n, fp->normal_radius, fp->fpfh_radius, s.stream, false, true, h->long_lists, true,
                              cell_table_cells(ncell, ncell)));
  QTR_HIP_TRY(h, hipMemcpyAsync(s.pinned_i32, s.fb.cloud[0].counts, 16 * sizeof(int), hipMemcpyDeviceToHost, s.stream));
  QTR_HIP_TRY(h, hipStreamSynchronize(s.stream));
  bool again = false;
  QTR_TRY(lists_refusal(h, 1, s.pinned_i32, nullptr, &again));
  if (again) return front_one_chain(h, s, d_raw, P, fp, n_out, passed_out);
  *n_out = n;
  *passed_out = v.passed ? 1 : 0;
  return QTR_OK;
}

static int front_one_device(qtr_handle* h, Slot& s, const float* raw4, int P, const qtr_frontend_params* fp, int mem,
                            int* n_out, int* passed_out) {
  QTR_TRY(front_one_check(h, raw4 != nullptr, P, fp));
  QTR_HIP_TRY(h, hipSetDevice(h->device));
  const float4* d_raw = (const float4*)raw4;
  if (mem == QTR_MEM_HOST) {
    QTR_HIP_TRY(h, hipMemcpyAsync(s.in_src, raw4, (size_t)P * 16, hipMemcpyHostToDevice, s.stream));
    d_raw = s.in_src;
  }
  return front_one_chain(h, s, d_raw, P, fp, n_out, passed_out);
}

// The front end's products on cloud[0] of the slot -> a keyframe of their size (the pack), complete on return.
static int keyframe_pack(qtr_handle* h, Slot& s, const qtr_frontend_params* fp, int P, int n, int passed, qtr_keyframe** out) {
  qtr_keyframe* kf = new (std::nothrow) qtr_keyframe();
  if (!kf) return QTR_ERR_CAPACITY;
  const KfLayout lay = kf_layout(n);
  if (hipMalloc(&kf->dev, lay.total) != hipSuccess) {
    (void)hipGetLastError();
    delete kf;
    snprintf(h->err, sizeof(h->err), "keyframe: no device memory for %zu bytes", lay.total);
    return QTR_ERR_HIP;
  }
  hipError_t e = kf_pack_enqueue(s.fb, kf->dev, n, s.stream);
  if (e == hipSuccess) e = hipStreamSynchronize(s.stream);
  if (e != hipSuccess) {
    (void)hipFree(kf->dev);
    delete kf;
    snprintf(h->err, sizeof(h->err), "keyframe pack: %s", hipGetErrorString(e));
    return QTR_ERR_HIP;
  }
  kf->owner = h;
  kf->info.n_points = P;
  kf->info.n_voxels = n;
  kf->info.voxel_size = fp->voxel_size;
  kf->info.normal_radius = fp->normal_radius;
  kf->info.fpfh_radius = fp->fpfh_radius;
  kf->info.passed_through = passed;
  kf->info.device_bytes = (unsigned long long)lay.total;
  {
    std::lock_guard<std::mutex> lk(h->kf_mu);
    h->keyframes.push_back(kf);
  }
  *out = kf;
  return QTR_OK;
}

int qtr_keyframe_create(qtr_handle* h, int slot, const float* raw4, int P, const qtr_frontend_params* fp, int mem,
                        qtr_keyframe** out) {
  if (out) *out = nullptr;
  Slot* sp = get_slot(h, slot);
  if (!sp || !fp || !out) return QTR_ERR_BAD_ARG;
  Slot& s = *sp;
  s.times_pending = TIMES_NONE;
  int n = 0, passed = 0;
  QTR_TRY(front_one_device(h, s, raw4, P, fp, mem, &n, &passed));
  return keyframe_pack(h, s, fp, P, n, passed, out);
}

// K keyframes under K poses -> one keyframe: the members' stored voxels are gathered on the device into the slot's raw-cloud
// buffer (k_kf_gather, one launch), and from there on the call is qtr_keyframe_create on a cloud that is already staged.
int qtr_keyframe_merge(qtr_handle* h, int slot, const qtr_keyframe* const* kfs, const double* poses, int K,
                       const qtr_frontend_params* fp, qtr_keyframe** out) {
  if (out) *out = nullptr;
  Slot* sp = get_slot(h, slot);
  if (!sp || !fp || !out) return QTR_ERR_BAD_ARG;
  Slot& s = *sp;
  s.times_pending = TIMES_NONE;
  if (K < 1 || K > QTR_SUBMAP_MAX_KEYFRAMES || !kfs) {
    snprintf(h->err, sizeof(h->err), "keyframe merge: %d members (1 .. %d)", K, QTR_SUBMAP_MAX_KEYFRAMES);
    return QTR_ERR_BAD_ARG;
  }
  long long N = 0;
  int max_n = 0;
  for (int k = 0; k < K; ++k) {
    if (!kfs[k]) {
      snprintf(h->err, sizeof(h->err), "keyframe merge: member %d is NULL", k);
      return QTR_ERR_BAD_ARG;
    }
    if (kfs[k]->owner != h) {
      snprintf(h->err, sizeof(h->err), "keyframe belongs to another handle");
      return QTR_ERR_BAD_ARG;
    }
    if (poses && !qtr_submap_pose_finite(poses + 16 * k)) {
      snprintf(h->err, sizeof(h->err), "keyframe merge: the pose of member %d has a non-finite entry in rows 0 - 2", k);
      return QTR_ERR_BAD_ARG;
    }
    N += kfs[k]->info.n_voxels;
    max_n = std::max(max_n, kfs[k]->info.n_voxels);
  }
  if (N > (long long)h->lim.max_points) {
    snprintf(h->err, sizeof(h->err), "keyframe merge: the members hold %lld voxels, which exceeds max_points=%d", N,
             h->lim.max_points);
    return QTR_ERR_CAPACITY;
  }
  QTR_TRY(front_one_check(h, true, (int)N, fp));
  QTR_HIP_TRY(h, hipSetDevice(h->device));
  if (!s.merge_pin) QTR_HIP_TRY(h, hipHostMalloc((void**)&s.merge_pin, sizeof(KfGatherMember) * QTR_SUBMAP_MAX_KEYFRAMES));
  if (!s.merge_dev) QTR_HIP_TRY(h, hipMalloc((void**)&s.merge_dev, sizeof(KfGatherMember) * QTR_SUBMAP_MAX_KEYFRAMES));
  // (the slot's last merge had completed when it returned: nothing reads the pinned table any more)
  static const double ident[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  int prefix = 0;
  for (int k = 0; k < K; ++k) {
    KfGatherMember& m = s.merge_pin[k];
    m.vox = (const float4*)((const char*)kfs[k]->dev + KF_HDR_BYTES);
    m.n = kfs[k]->info.n_voxels;
    m.prefix = prefix;
    memcpy(m.T, poses ? poses + 16 * k : ident, sizeof(m.T));
    prefix += m.n;
  }
  QTR_HIP_TRY(h, hipMemcpyAsync(s.merge_dev, s.merge_pin, sizeof(KfGatherMember) * (size_t)K, hipMemcpyHostToDevice, s.stream));
  QTR_HIP_TRY(h, kf_gather_enqueue(s.merge_dev, K, max_n, s.in_src, s.stream));
  int n = 0, passed = 0;
  QTR_TRY(front_one_chain(h, s, s.in_src, (int)N, fp, &n, &passed));
  return keyframe_pack(h, s, fp, (int)N, n, passed, out);
}

int qtr_keyframe_get_info(const qtr_keyframe* kf, qtr_keyframe_info* info) {
  if (!kf || !info) return QTR_ERR_BAD_ARG;
  *info = kf->info;
  return QTR_OK;
}

long long qtr_keyframe_fetch(qtr_handle* h, const qtr_keyframe* kf, int what, void* dst, size_t bytes) {
  if (!h || !kf || kf->owner != h) return -1;
  if (hipSetDevice(h->device) != hipSuccess) return -1;
  const KfLayout lay = kf_layout(kf->info.n_voxels);
  const size_t n = (size_t)kf->info.n_voxels;
  size_t off = 0, have = 0;
  switch (what) {
    case QTR_KF_VOX: off = lay.vox; have = n * 16; break;
    case QTR_KF_NORMALS: off = lay.normals; have = n * 16; break;
    case QTR_KF_FPFH: off = lay.fpfh; have = n * 132; break;
    case QTR_KF_MEAN: off = 64; have = 16; break;
    default: return -1;
  }
  const size_t m = have < bytes ? have : bytes;
  if (dst && m > 0 && hipMemcpy(dst, (const char*)kf->dev + off, m, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  return (long long)have;
}

void qtr_keyframe_destroy(qtr_handle* h, qtr_keyframe* kf) {
  if (!h || !kf || kf->owner != h) return;
  {
    std::lock_guard<std::mutex> lk(h->kf_mu);
    auto it = std::find(h->keyframes.begin(), h->keyframes.end(), kf);
    if (it == h->keyframes.end()) return;
    h->keyframes.erase(it);
  }
  (void)hipSetDevice(h->device);
  if (kf->dev) (void)hipFree(kf->dev);
  delete kf;
}

// ------------------------------------------------------------------------------------------------
// place index (place.hip): one Scan Context descriptor per keyframe, exhaustive search under all column shifts
void qtr_default_place_params(qtr_place_params* p) {
  if (!p) return;
  p->num_rings = 20;
  p->num_sectors = 60;
  p->max_range = 80.0f;
  p->height_offset = 2.0f;
}

static int check_place_params(qtr_handle* h, const qtr_place_params* p) {
  if (p->num_rings < 4 || p->num_rings > QTR_PLACE_MAX_RINGS || p->num_sectors < 8 || p->num_sectors > QTR_PLACE_MAX_SECTORS ||
      !(p->max_range > 0.0f) || (p->max_range - p->max_range) != 0.0f || (p->height_offset - p->height_offset) != 0.0f) {
    snprintf(h->err, sizeof(h->err), "place params: num_rings %d (4 .. %d), num_sectors %d (8 .. %d), max_range %g (> 0), "
             "height_offset %g (finite)", p->num_rings, QTR_PLACE_MAX_RINGS, p->num_sectors, QTR_PLACE_MAX_SECTORS, p->max_range,
             p->height_offset);
    return QTR_ERR_BAD_ARG;
  }
  return QTR_OK;
}

static int check_place_index(qtr_handle* h, const qtr_place_index* ix) {
  if (!ix) {
    snprintf(h->err, sizeof(h->err), "place index is NULL");
    return QTR_ERR_BAD_ARG;
  }
  if (ix->owner != h) {
    snprintf(h->err, sizeof(h->err), "place index belongs to another handle");
    return QTR_ERR_BAD_ARG;
  }
  return QTR_OK;
}

// the slot's scratch for entries of `stride` floats and searches over up to `cap` entries (it only ever grows; the slot's
// earlier place calls were complete when they returned, so nothing reads the old arena)
static int place_scratch_ensure(qtr_handle* h, Slot& s, int stride, int cap) {
  PlaceScratch& sc = s.place;
  if (!sc.pin) QTR_HIP_TRY(h, hipHostMalloc((void**)&sc.pin, sizeof(qtr_place_match) * QTR_PLACE_MAX_K));
  if (sc.arena && stride <= sc.stride && cap <= sc.cap) return QTR_OK;
  stride = std::max(stride, sc.stride);
  cap = std::max(std::max(cap, sc.cap), 1);
  const size_t o_keys = qtr_up256((size_t)stride * 4), o_shifts = o_keys + qtr_up256((size_t)cap * 8), o_out = o_shifts + qtr_up256((size_t)cap * 4),
               total = o_out + qtr_up256(sizeof(qtr_place_match) * QTR_PLACE_MAX_K);
  if (sc.arena) {
    QTR_HIP_TRY(h, hipStreamSynchronize(s.stream));
    (void)hipFree(sc.arena);
    sc.arena = nullptr;
    sc.stride = sc.cap = 0;
  }
  if (hipMalloc(&sc.arena, total) != hipSuccess) {
    (void)hipGetLastError();
    sc.arena = nullptr;
    snprintf(h->err, sizeof(h->err), "place index: no device memory for %zu bytes of scratch", total);
    return QTR_ERR_HIP;
  }
  char* a = (char*)sc.arena;
  sc.q = (float*)a;
  sc.keys = (u64*)(a + o_keys);
  sc.shifts = (int*)(a + o_shifts);
  sc.out = (qtr_place_match*)(a + o_out);
  sc.stride = stride;
  sc.cap = cap;
  return QTR_OK;
}

int qtr_place_index_create(qtr_handle* h, const qtr_place_params* params, int capacity, qtr_place_index** out) {
  if (out) *out = nullptr;
  if (!h || !out) return QTR_ERR_BAD_ARG;
  qtr_place_params p;
  qtr_default_place_params(&p);
  if (params) p = *params;
  QTR_TRY(check_place_params(h, &p));
  if (capacity < 1) {
    snprintf(h->err, sizeof(h->err), "place index: capacity %d", capacity);
    return QTR_ERR_BAD_ARG;
  }
  QTR_HIP_TRY(h, hipSetDevice(h->device));
  qtr_place_index* ix = new (std::nothrow) qtr_place_index();
  if (!ix) return QTR_ERR_CAPACITY;
  ix->stride = place_stride(p.num_rings, p.num_sectors);
  const size_t bytes = (size_t)capacity * ix->stride * 4;
  if (hipMalloc((void**)&ix->dev, bytes) != hipSuccess) {
    (void)hipGetLastError();
    delete ix;
    snprintf(h->err, sizeof(h->err), "place index: no device memory for %zu bytes", bytes);
    return QTR_ERR_HIP;
  }
  ix->owner = h;
  ix->info.params = p;
  ix->info.size = 0;
  ix->info.capacity = capacity;
  ix->info.device_bytes = (unsigned long long)bytes;
  {
    std::lock_guard<std::mutex> lk(h->kf_mu);
    h->place_indexes.push_back(ix);
  }
  *out = ix;
  return QTR_OK;
}

void qtr_place_index_destroy(qtr_handle* h, qtr_place_index* ix) {
  if (!h || !ix || ix->owner != h) return;
  {
    std::lock_guard<std::mutex> lk(h->kf_mu);
    auto it = std::find(h->place_indexes.begin(), h->place_indexes.end(), ix);
    if (it == h->place_indexes.end()) return;
    h->place_indexes.erase(it);
  }
  (void)hipSetDevice(h->device);
  if (ix->dev) (void)hipFree(ix->dev);
  delete ix;
}

int qtr_place_index_get_info(const qtr_place_index* ix, qtr_place_index_info* info) {
  if (!ix || !info) return QTR_ERR_BAD_ARG;
  *info = ix->info;
  return QTR_OK;
}

int qtr_place_describe(qtr_handle* h, int slot, const qtr_place_params* params, const float* xyz4, int n, float* desc, int mem) {
  Slot* sp = get_slot(h, slot);  // (a host cloud is staged in the slot's input arena)
  if (!sp || !desc || n < 0 || (n > 0 && !xyz4) || (mem != QTR_MEM_HOST && mem != QTR_MEM_DEVICE)) return QTR_ERR_BAD_ARG;
  Slot& s = *sp;
  qtr_place_params p;
  qtr_default_place_params(&p);
  if (params) p = *params;
  QTR_TRY(check_place_params(h, &p));
  if (mem == QTR_MEM_HOST && n > h->lim.max_points) {
    snprintf(h->err, sizeof(h->err), "cloud exceeds max_points=%d", h->lim.max_points);
    return QTR_ERR_CAPACITY;
  }
  QTR_HIP_TRY(h, hipSetDevice(h->device));
  QTR_TRY(place_scratch_ensure(h, s, place_stride(p.num_rings, p.num_sectors), 1));
  const float4* d_pts = (const float4*)xyz4;
  if (mem == QTR_MEM_HOST && n > 0) {
    QTR_HIP_TRY(h, hipMemcpyAsync(s.in_src, xyz4, (size_t)n * 16, hipMemcpyHostToDevice, s.stream));
    d_pts = s.in_src;
  }
  QTR_HIP_TRY(h, place_describe_enqueue(d_pts, n, p, s.place.q, s.stream));
  QTR_HIP_TRY(h, hipMemcpyAsync(desc, s.place.q, (size_t)p.num_rings * p.num_sectors * 4,
                                mem == QTR_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, s.stream));
  QTR_HIP_TRY(h, hipStreamSynchronize(s.stream));
  return QTR_OK;
}

// the checks every add shares; on QTR_OK *entry is where the next entry goes
static int place_add_begin(qtr_handle* h, qtr_place_index* ix, float** entry) {
  QTR_TRY(check_place_index(h, ix));
  if (ix->info.size >= ix->info.capacity) {
    snprintf(h->err, sizeof(h->err), "place index is full (capacity %d)", ix->info.capacity);
    return QTR_ERR_CAPACITY;
  }
  *entry = ix->dev + (size_t)ix->info.size * ix->stride;
  return QTR_OK;
}

int qtr_place_index_add(qtr_handle* h, int slot, qtr_place_index* ix, const qtr_keyframe* kf, int* id_out) {
  Slot* sp = peek_slot(h, slot);  // (nothing of the slot's clouds is touched: a registration on it can still be refined)
  if (!sp || !ix || !kf) return QTR_ERR_BAD_ARG;
  if (kf->owner != h) {
    snprintf(h->err, sizeof(h->err), "keyframe belongs to another handle");
    return QTR_ERR_BAD_ARG;
  }
  float* entry = nullptr;
  QTR_TRY(place_add_begin(h, ix, &entry));
  QTR_HIP_TRY(h, hipSetDevice(h->device));
  QTR_HIP_TRY(h, place_describe_enqueue((const float4*)((const char*)kf->dev + KF_HDR_BYTES), kf->info.n_voxels, ix->info.params,
                                        entry, sp->stream));
  QTR_HIP_TRY(h, hipStreamSynchronize(sp->stream));
  if (id_out) *id_out = ix->info.size;
  ix->info.size += 1;
  return QTR_OK;
}

int qtr_place_index_add_desc(qtr_handle* h, int slot, qtr_place_index* ix, const float* desc, int mem, int* id_out) {
  Slot* sp = peek_slot(h, slot);
  if (!sp || !ix || !desc || (mem != QTR_MEM_HOST && mem != QTR_MEM_DEVICE)) return QTR_ERR_BAD_ARG;
  float* entry = nullptr;
  QTR_TRY(place_add_begin(h, ix, &entry));
  QTR_HIP_TRY(h, hipSetDevice(h->device));
  const qtr_place_params& p = ix->info.params;
  QTR_HIP_TRY(h, hipMemcpyAsync(entry, desc, (size_t)p.num_rings * p.num_sectors * 4,
                                mem == QTR_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, sp->stream));
  QTR_HIP_TRY(h, place_colnorm_enqueue(entry, p, sp->stream));
  QTR_HIP_TRY(h, hipStreamSynchronize(sp->stream));
  if (id_out) *id_out = ix->info.size;
  ix->info.size += 1;
  return QTR_OK;
}

long long qtr_place_index_fetch(qtr_handle* h, const qtr_place_index* ix, int id, int what, void* dst, size_t bytes) {
  if (!h || !ix || ix->owner != h || id < 0 || id >= ix->info.size) return -1;
  if (hipSetDevice(h->device) != hipSuccess) return -1;
  const size_t cells = (size_t)ix->info.params.num_rings * ix->info.params.num_sectors;
  size_t off = 0, have = 0;
  switch (what) {
    case QTR_PLACE_DESC: off = 0; have = cells * 4; break;
    case QTR_PLACE_COLNORM2: off = cells * 4; have = (size_t)ix->info.params.num_sectors * 4; break;
    default: return -1;
  }
  const size_t m = have < bytes ? have : bytes;
  const char* src = (const char*)(ix->dev + (size_t)id * ix->stride) + off;
  if (dst && m > 0 && hipMemcpy(dst, src, m, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  return (long long)have;
}

// the checks both queries share; on QTR_OK [*lo, *lo + *n) is the clamped range (*n may be 0)
static int place_query_begin(qtr_handle* h, const qtr_place_index* ix, int id_lo, int id_hi, int k, int* lo, int* n) {
  QTR_TRY(check_place_index(h, ix));
  if (k < 1 || k > QTR_PLACE_MAX_K) {
    snprintf(h->err, sizeof(h->err), "place query: k = %d (1 .. %d)", k, QTR_PLACE_MAX_K);
    return QTR_ERR_BAD_ARG;
  }
  const int a = std::max(id_lo, 0), b = std::min(id_hi, ix->info.size);
  *lo = a;
  *n = b > a ? b - a : 0;
  return QTR_OK;
}
// the search over [lo, lo + n), n >= 1, with the query's entry in the slot's scratch; the records come back through pinned
// memory behind ONE wait
static int place_query_finish(qtr_handle* h, Slot& s, const qtr_place_index* ix, int lo, int n, int k, qtr_place_match* out,
                              int* n_out) {
  const int kk = std::min(k, n);
  QTR_HIP_TRY(h, place_search_enqueue(ix->dev, ix->info.params, lo, n, kk, s.place, s.stream));
  QTR_HIP_TRY(h, hipMemcpyAsync(s.place.pin, s.place.out, sizeof(qtr_place_match) * kk, hipMemcpyDeviceToHost, s.stream));
  QTR_HIP_TRY(h, hipStreamSynchronize(s.stream));
  memcpy(out, s.place.pin, sizeof(qtr_place_match) * kk);
  *n_out = kk;
  return QTR_OK;
}

int qtr_place_query(qtr_handle* h, int slot, const qtr_place_index* ix, const qtr_keyframe* query, int id_lo, int id_hi, int k,
                    qtr_place_match* out, int* n_out) {
  if (n_out) *n_out = 0;
  Slot* sp = peek_slot(h, slot);
  if (!sp || !ix || !query || !out || !n_out) return QTR_ERR_BAD_ARG;
  if (query->owner != h) {
    snprintf(h->err, sizeof(h->err), "keyframe belongs to another handle");
    return QTR_ERR_BAD_ARG;
  }
  int lo = 0, n = 0;
  QTR_TRY(place_query_begin(h, ix, id_lo, id_hi, k, &lo, &n));
  if (n == 0) return QTR_OK;
  QTR_HIP_TRY(h, hipSetDevice(h->device));
  QTR_TRY(place_scratch_ensure(h, *sp, ix->stride, ix->info.capacity));
  QTR_HIP_TRY(h, place_describe_enqueue((const float4*)((const char*)query->dev + KF_HDR_BYTES), query->info.n_voxels,
                                        ix->info.params, sp->place.q, sp->stream));
  return place_query_finish(h, *sp, ix, lo, n, k, out, n_out);
}

int qtr_place_query_desc(qtr_handle* h, int slot, const qtr_place_index* ix, const float* desc, int mem, int id_lo, int id_hi,
                         int k, qtr_place_match* out, int* n_out) {
  if (n_out) *n_out = 0;
  Slot* sp = peek_slot(h, slot);
  if (!sp || !ix || !desc || !out || !n_out || (mem != QTR_MEM_HOST && mem != QTR_MEM_DEVICE)) return QTR_ERR_BAD_ARG;
  int lo = 0, n = 0;
  QTR_TRY(place_query_begin(h, ix, id_lo, id_hi, k, &lo, &n));
  if (n == 0) return QTR_OK;
  QTR_HIP_TRY(h, hipSetDevice(h->device));
  QTR_TRY(place_scratch_ensure(h, *sp, ix->stride, ix->info.capacity));
  const qtr_place_params& p = ix->info.params;
  QTR_HIP_TRY(h, hipMemcpyAsync(sp->place.q, desc, (size_t)p.num_rings * p.num_sectors * 4,
                                mem == QTR_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, sp->stream));
  QTR_HIP_TRY(h, place_colnorm_enqueue(sp->place.q, p, sp->stream));
  return place_query_finish(h, *sp, ix, lo, n, k, out, n_out);
}

// a pair of keyframes against the handle and the call's front-end knobs
static int check_keyframes(qtr_handle* h, const qtr_keyframe* a, const qtr_keyframe* b, const qtr_frontend_params* fp) {
  if (!a || !b) {
    snprintf(h->err, sizeof(h->err), "keyframe is NULL");
    return QTR_ERR_BAD_ARG;
  }
  if (a->owner != h || b->owner != h) {
    snprintf(h->err, sizeof(h->err), "keyframe belongs to another handle");
    return QTR_ERR_BAD_ARG;
  }
  auto same = [](float x, float y) { return memcmp(&x, &y, 4) == 0; };
  for (const qtr_keyframe* k : {a, b})
    if (!same(k->info.voxel_size, fp->voxel_size) || !same(k->info.normal_radius, fp->normal_radius) ||
        !same(k->info.fpfh_radius, fp->fpfh_radius)) {
      snprintf(h->err, sizeof(h->err), "keyframe was made with voxel_size %g, normal_radius %g, fpfh_radius %g; the call asks "
               "for %g, %g, %g", k->info.voxel_size, k->info.normal_radius, k->info.fpfh_radius, fp->voxel_size,
               fp->normal_radius, fp->fpfh_radius);
      return QTR_ERR_BAD_ARG;
    }
  return QTR_OK;
}

int qtr_register_keyframes(qtr_handle* h, int slot, const qtr_keyframe* kf_src, const qtr_keyframe* kf_tgt,
                           const qtr_frontend_params* fp, const qtr_params* prm, qtr_result* res, int* clique,
                           int* final_inliers, int cap) {
  Slot* sp = get_slot(h, slot);
  if (!sp || !res || !fp) return QTR_ERR_BAD_ARG;
  Slot& s = *sp;
  memset(res, 0, sizeof(*res));
  int rc = check_params(h, prm);
  if (rc != QTR_OK) return res->status = rc;
  if ((rc = check_keyframes(h, kf_src, kf_tgt, fp)) != QTR_OK) return res->status = rc;
  QTR_HIP_TRY(h, hipSetDevice(h->device));
  const int ns = kf_src->info.n_voxels, nt = kf_tgt->info.n_voxels;
  res->n_src = s.last_ns = ns;
  res->n_tgt = s.last_nt = nt;
  if (h->stage_events) QTR_HIP_TRY(h, hipEventRecord(s.ev[EV_BEGIN], s.stream));
  // the matcher's clean slate first — it clears the duplicate tables the load fills, and the solver's state rides in it —
  // then ONE launch for both clouds; the matcher starts at its operand tables (init_done, prep_done)
  QTR_HIP_TRY(h, match_init_enqueue(s.fb, ns, nt, *fp, s.stream, true, (int*)s.sb.st, (int)(sizeof(SolverState) / 4)));
  QTR_HIP_TRY(h, kf_load_enqueue(s.fb, kf_src->dev, ns, kf_tgt->dev, nt, s.stream));
  int L = 0;
  rc = match_device(h, s, ns, nt, fp, &L, true, true);
  res->n_corr = L;
  if (rc != QTR_OK) return res->status = rc;
  s.last_L = L;
  if ((rc = check_max_corr(h, L)) != QTR_OK) return res->status = rc;
  QTR_HIP_TRY(h, gather_matched_enqueue(s.fb, L, s.m_src, s.m_tgt, s.stream));
  if (h->stage_events) QTR_HIP_TRY(h, hipEventRecord(s.ev[EV_MATCH], s.stream));
  rc = solve_device(h, s, s.m_src, s.m_tgt, L, prm, res, true);
  rc = finish_registration(h, s, rc, TIMES_KEYFRAMES, res, clique, nullptr, final_inliers, cap, QTR_MEM_HOST, s.stream);
  mark_registration(s, rc, res);
  return rc;
}

// ------------------------------------------------------------------------------------------------
// batched registration: lanes of slots stepped through the three launch chains in lockstep
static void batch_fail_pair(qtr_handle* h, int pair, int status) {
  qtr_result& r = h->job.results[pair];
  r.status = status;
  r.valid = 0;
  h->job.finished[pair] = 1;
  ++h->job.done;
}

// ICP pieces the refine phase shares with qtr_icp / qtr_refine_pair (defined with them, below)
static int check_icp_params(qtr_handle* h, const qtr_icp_params* p);
static int icp_device(qtr_handle* h, Slot& s, const float4* d_src, int ns, const float4* d_tgt, int nt, const float4* d_nrm,
                      const float4* d_src_nrm, const double* guess, const qtr_icp_params* prm, qtr_icp_result* res);

// The refined records the job has not produced: QTR_ERR_NOT_RUN, valid = 0, T = the registration's T.  After a job
// failure (failed), a pair whose registration did not finish takes its result's status, a pair whose refinement was under
// way QTR_ERR_HIP.
static void refine_fill_rest(qtr_handle* h, bool failed) {
  BatchJob& J = h->job;
  if (!J.refine) return;
  for (int i = 0; i < J.B; ++i) {
    if (J.ref_state[i] == 2) continue;
    qtr_icp_result& q = J.refined[i];
    memset(&q, 0, sizeof(q));
    q.status = QTR_ERR_NOT_RUN;
    if (failed && !J.finished[i]) q.status = J.results[i].status;
    else if (failed && J.ref_state[i] == 1) q.status = QTR_ERR_HIP;
    for (int k = 0; k < 16; ++k) q.T[k] = J.results[i].T[k];
    J.ref_state[i] = 2;
  }
}

// The job failed (HIP error, a lane that never published): drain what is in flight so the handle stays usable, and make
// every record say what happened to its pair — pairs that had been started but did not finish get QTR_ERR_HIP, pairs
// that were never started QTR_ERR_NOT_RUN; finished pairs keep their records.
static void batch_abort(qtr_handle* h) {
  BatchJob& J = h->job;
  for (auto& ln : h->lanes) {
    Slot& lead = h->slots[ln.first_slot];
    (void)hipStreamSynchronize(lead.stream);
    (void)hipStreamSynchronize(lead.stream2);
    ln.phase = LANE_IDLE;
  }
  (void)hipGetLastError();
  for (int i = 0; i < J.B; ++i) {
    if (J.finished[i]) continue;
    memset(&J.results[i], 0, sizeof(qtr_result));
    J.results[i].status = i < J.next ? QTR_ERR_HIP : QTR_ERR_NOT_RUN;
  }
  refine_fill_rest(h, true);
  J.active = false;
}

// What a pair descriptor asks for: scans (front end + back end), pre-matched correspondences (back end only — the
// reference's setInputSource / setInputTarget / computeTransformation on what it is handed,
// examples/run_global_registration.cpp:243-246), or both (front end of the scans, back end on the given correspondences).
static inline bool pair_has_scans(const qtr_pair_desc& pd) { return pd.src_raw4 != nullptr || pd.tgt_raw4 != nullptr; }
static inline bool pair_has_corr(const qtr_pair_desc& pd) {
  return pd.src_corr4 != nullptr || pd.tgt_corr4 != nullptr || pd.n_corr != 0;
}

static int lane_start_chunk(qtr_handle* h, Lane& ln);
static int lane_enqueue_refine(qtr_handle* h, Lane& ln);

// Solver chain of the chunk: the pairs of `from_match` (survivors of the matching chain, ln.L / ln.csrc / ln.ctgt set)
// plus the chunk's correspondence-only pairs.
static int lane_enqueue_solver(qtr_handle* h, Lane& ln, const std::vector<int>& from_match) {
  BatchJob& J = h->job;
  Slot& lead = h->slots[ln.first_slot];
  std::vector<int> all(from_match);
  all.insert(all.end(), ln.corr_only.begin(), ln.corr_only.end());
  ln.corr_only.clear();
  ln.active.swap(all);
  if (ln.active.empty()) return lane_start_chunk(h, ln);
  std::vector<int> Ls;
  std::vector<SolverBufs*> SB;
  std::vector<const float4*> srcs, tgts;
  for (int g : ln.active) {
    Slot& s = h->slots[ln.first_slot + g];
    s.last_L = ln.L[g];
    s.last_Wb = (((ln.L[g] + 63) / 64) + 3) & ~3;
    s.sb.mail_seq = ++s.seq;
    SB.push_back(&s.sb);
    srcs.push_back(ln.csrc[g]);
    tgts.push_back(ln.ctgt[g]);
    Ls.push_back(ln.L[g]);
  }
  solver_set_hca_share((int)h->lanes.size());  // the lanes' solver chains overlap: each keeps to its share of the device
  QTR_HIP_TRY(h, solver_enqueue_group(SB.data(), (int)SB.size(), srcs.data(), tgts.data(), Ls.data(), J.prm, &ln.stage,
                                      lead.stream));
  ln.phase = LANE_SOLVE;
  return QTR_OK;
}

// The demo's STEP 2 and 3 on raw sweeps (reference examples/run_global_registration.cpp:136-160): per scan
// PatchWork::estimate_ground -> non-ground points -> ImageProjection::segmentCloud -> valid segments.  Both stages hand a
// count to the next one through the host, so a scan is a chain of four host-visible steps — run for ALL pairs of the
// chunk side by side, every pair on its own slot's stream and arenas (target first, then source: the two scans of a pair
// share the slot), the host advancing whichever slot's step has finished.  (Rounds 2-3 ran them pair after pair with a
// blocking read-back per step: a chunk of sixteen raw pairs waited 64 times.)  The valid segments land in the slot's
// staging buffers, which are the voxel grid's input; the lane's stream waits for the copies, not the host.
struct PreScan {
  int stage = 0;  // 0 start, 1 ground segmentation of scan c in flight, 2 range-image stage in flight, 3 done
  int c = 1;      // scan being processed: 1 target, then 0 source
  int status = QTR_OK;
  int n[2] = {0, 0};  // valid points of source / target
};
static int lane_preprocess(qtr_handle* h, Lane& ln, std::vector<PreScan>& pre) {
  BatchJob& J = h->job;
  Slot& lead = h->slots[ln.first_slot];
  int open = 0;
  for (int g = 0; g < ln.count; ++g) {
    const qtr_pair_desc& pd = J.pairs[ln.first_pair + g];
    const bool usable = pair_has_scans(pd) && pd.src_raw4 && pd.tgt_raw4 && pd.n_src > 0 && pd.n_tgt > 0 &&
                        pd.n_src <= h->lim.max_points && pd.n_tgt <= h->lim.max_points;
    if (!usable) pre[(size_t)g].stage = 3;  // (refused by the checks below, or a pair without scans)
    else ++open;
  }
  unsigned long spins = 0;
  while (open > 0) {
    bool moved = false;
    for (int g = 0; g < ln.count; ++g) {
      PreScan& q = pre[(size_t)g];
      if (q.stage == 3) continue;
      const qtr_pair_desc& pd = J.pairs[ln.first_pair + g];
      Slot& s = h->slots[ln.first_slot + g];
      int rc = QTR_OK;
      if (q.stage == 0) {
        rc = pw_begin(h, s, q.c ? pd.tgt_raw4 : pd.src_raw4, q.c ? pd.n_tgt : pd.n_src, &h->pre_pw, J.mem);
        q.stage = 1;
        moved = true;
      } else {
        const hipError_t e = hipEventQuery(s.ev[EV_STAGE_END]);
        if (e == hipErrorNotReady) continue;
        if (e != hipSuccess) {
          snprintf(h->err, sizeof(h->err), "batch pre-processing: %s", hipGetErrorString(e));
          return QTR_ERR_HIP;
        }
        moved = true;
        if (q.stage == 1) {  // ground removed: its non-ground points go through the range image
          int ng = 0, nn = 0;
          pw_end(s, &ng, &nn);
          rc = seg_begin(h, s, (const float*)s.pwb.out_n, nn, &h->pre_ip, QTR_MEM_DEVICE);
          q.stage = 2;
        } else {  // valid segments known: into the staging buffer; next scan, or done
          const int nv = s.pinned_i32[0];
          q.n[q.c] = nv;
          if (nv > h->lim.max_points) rc = QTR_ERR_CAPACITY;
          else if (nv > 0)
            // (on the slot's own stream: the next scan's stages, which reuse the buffers this copy reads, queue up behind it)
            QTR_HIP_TRY(h, hipMemcpyAsync(q.c ? s.in_tgt : s.in_src, s.seg.out_valid, (size_t)nv * 16, hipMemcpyDeviceToDevice,
                                          s.stream));
          if (rc == QTR_OK && q.c == 1) {
            q.c = 0;
            q.stage = 0;
          } else {
            if (rc == QTR_OK) {  // the group's chain (lane stream) reads the staging buffers: it waits for this slot
              QTR_HIP_TRY(h, hipEventRecord(s.ev[EV_STAGE_END], s.stream));
              QTR_HIP_TRY(h, hipStreamWaitEvent(lead.stream, s.ev[EV_STAGE_END], 0));
            }
            q.stage = 3;
            --open;
          }
        }
      }
      if (rc == QTR_ERR_HIP) return rc;
      if (rc != QTR_OK && q.stage != 3) {  // this pair's own failure (capacity, a scan the stage refuses)
        q.status = rc;
        q.stage = 3;
        --open;
      } else if (rc != QTR_OK) {
        q.status = rc;
      }
    }
    if (!moved) {
      __builtin_ia32_pause();
      if ((++spins & 0xffffff) == 0) {  // nothing moved for a long while: a lost device must not hang the host
        for (int g = 0; g < ln.count; ++g)
          if (pre[(size_t)g].stage != 3) QTR_HIP_TRY(h, hipStreamSynchronize(h->slots[ln.first_slot + g].stream));
      }
    } else {
      spins = 0;
    }
  }
  return QTR_OK;
}

static int lane_start_chunk(qtr_handle* h, Lane& ln) {
  BatchJob& J = h->job;
  if (J.next >= J.B) {
    ln.phase = LANE_IDLE;
    ln.count = 0;
    return QTR_OK;
  }
  ln.first_pair = J.next;
  ln.count = min(ln.cap, J.B - J.next);
  J.next += ln.count;
  ln.stage.off = 0;
  ln.active.clear();
  ln.corr_only.clear();
  ln.ns.assign((size_t)ln.count, 0);
  ln.nt.assign((size_t)ln.count, 0);
  ln.L.assign((size_t)ln.count, 0);
  ln.csrc.assign((size_t)ln.count, nullptr);
  ln.ctgt.assign((size_t)ln.count, nullptr);
  ln.raw_s.assign((size_t)ln.count, nullptr);
  ln.raw_t.assign((size_t)ln.count, nullptr);
  ln.Ps.assign((size_t)ln.count, 0);
  ln.Pt.assign((size_t)ln.count, 0);
  Slot& lead = h->slots[ln.first_slot];
  std::vector<FrontBufs*> F;
  std::vector<const float4*> raws;
  std::vector<int> Ps;
  std::vector<void*> kf_dev;                  // keyframe job: the device allocations, two per pair (Ps: their voxel counts)
  std::vector<unsigned long long> kf_seeds;
  std::vector<PreScan> pre((size_t)ln.count);
  if (h->pre_on && !J.kf) QTR_TRY(lane_preprocess(h, ln, pre));
  for (int g = 0; g < ln.count; ++g) {
    const qtr_pair_desc& pd = J.pairs[ln.first_pair + g];
    Slot& s = h->slots[ln.first_slot + g];
    qtr_result& r = J.results[ln.first_pair + g];
    memset(&r, 0, sizeof(r));
    const bool scans = pair_has_scans(pd), corr = pair_has_corr(pd);
    if ((!scans && !corr) || (scans && (pd.n_src <= 0 || pd.n_tgt <= 0 || !pd.src_raw4 || !pd.tgt_raw4)) ||
        (corr && (pd.n_corr < 0 || !pd.src_corr4 || !pd.tgt_corr4))) {
      batch_fail_pair(h, ln.first_pair + g, QTR_ERR_BAD_ARG);
      continue;
    }
    if ((scans && (pd.n_src > h->lim.max_points || pd.n_tgt > h->lim.max_points)) || (corr && pd.n_corr > h->lim.max_corr)) {
      batch_fail_pair(h, ln.first_pair + g, QTR_ERR_CAPACITY);
      continue;
    }
    s.times_pending = TIMES_NONE;
    if (J.kf) {  // a keyframe pair (validated at submission): no voxel chain — the load and the matcher follow the loop
      const qtr_keyframe *ks = (const qtr_keyframe*)pd.src_raw4, *kt = (const qtr_keyframe*)pd.tgt_raw4;
      r.n_src = ln.ns[g] = s.last_ns = ks->info.n_voxels;
      r.n_tgt = ln.nt[g] = s.last_nt = kt->info.n_voxels;
      s.fb.mail_seq = ++s.seq;
      ln.active.push_back(g);
      F.push_back(&s.fb);
      kf_dev.push_back(ks->dev);
      kf_dev.push_back(kt->dev);
      Ps.push_back(ks->info.n_voxels);
      Ps.push_back(kt->info.n_voxels);
      kf_seeds.push_back(pd.seed);
      continue;
    }
    if (corr) {
      r.n_corr = pd.n_corr;
      ln.L[g] = pd.n_corr;
    }
    if (!scans) {  // correspondences only: nothing to do before the solver chain
      QTR_TRY(corr_stage(h, s, pd.src_corr4, pd.tgt_corr4, pd.n_corr, J.mem, lead.stream, &ln.csrc[g], &ln.ctgt[g]));
      ln.corr_only.push_back(g);
      continue;
    }
    const float4 *d_s = (const float4*)pd.src_raw4, *d_t = (const float4*)pd.tgt_raw4;
    int P_s = pd.n_src, P_t = pd.n_tgt;
    if (h->pre_on) {
      // (the sweeps were pre-processed above, all slots of the chunk side by side: the valid segments are in the slot's
      // staging buffers, the lane's stream already waits for the copies)
      const PreScan& q = pre[(size_t)g];
      if (q.status == QTR_OK && (q.n[0] <= 0 || q.n[1] <= 0)) {  // nothing but ground: an empty cloud
        batch_fail_pair(h, ln.first_pair + g, QTR_ERR_BAD_ARG);
        continue;
      }
      if (q.status != QTR_OK) {
        batch_fail_pair(h, ln.first_pair + g, q.status);
        continue;
      }
      P_s = q.n[0];
      P_t = q.n[1];
      d_s = s.in_src;
      d_t = s.in_tgt;
    } else if (J.mem == QTR_MEM_HOST) {
      QTR_HIP_TRY(h, hipMemcpyAsync(s.in_src, pd.src_raw4, (size_t)pd.n_src * 16, hipMemcpyHostToDevice, lead.stream));
      QTR_HIP_TRY(h, hipMemcpyAsync(s.in_tgt, pd.tgt_raw4, (size_t)pd.n_tgt * 16, hipMemcpyHostToDevice, lead.stream));
      d_s = s.in_src;
      d_t = s.in_tgt;
    }
    s.fb.mail_seq = ++s.seq;
    ln.raw_s[g] = d_s;  // (device pointers: what the voxel grid of this pair reads)
    ln.raw_t[g] = d_t;
    ln.Ps[g] = P_s;
    ln.Pt[g] = P_t;
    ln.active.push_back(g);
    F.push_back(&s.fb);
    raws.push_back(d_s);
    raws.push_back(d_t);
    Ps.push_back(P_s);
    Ps.push_back(P_t);
  }
  if (ln.active.empty()) return lane_enqueue_solver(h, ln, {});  // no scans in this chunk (or nothing valid at all)
  if (J.kf) {
    // no voxel chain, and the matching chain is a grouped load (blockIdx.z = pair) in front of the matcher, which finds the
    // per-descriptor preparation done as after the whole path's k2_fpfh.  The lists' checks were made when the keyframes
    // were created and the load leaves their counter words clean: the chunk counts as one that ran k2_neighbors_big.
    QTR_HIP_TRY(h, kf_load_enqueue_group(F.data(), (int)F.size(), kf_dev.data(), Ps.data(), &ln.stage, lead.stream));
    ln.long_lists = true;
    QTR_HIP_TRY(h, match_enqueue_group(F.data(), (int)F.size(), Ps.data(), &J.fp, kf_seeds.data(), &ln.stage, lead.stream, true));
    ln.phase = LANE_MATCH;
    return QTR_OK;
  }
  QTR_HIP_TRY(h, voxelize_enqueue_group(F.data(), (int)F.size(), raws.data(), Ps.data(), J.fp.voxel_size, &ln.stage,
                                        lead.stream, J.fp.fpfh_radius * 1.001f));
  QTR_HIP_TRY(h, hipEventRecord(lead.ev_vox, lead.stream));
  ln.phase = LANE_VOXELS;
  return QTR_OK;
}

// Refine phase of the chunk (qtr_submit_batch_refine), while the chunk's slots still hold its clouds: the pairs of the
// solver chain that ran the front end and registered (QTR_OK / QTR_ERR_CLIQUE_TOO_SMALL, mark_registration's rule) go
// through the grouped ICP kernels (icp.hip), blockIdx.y = pair.  Three chains, each ending in the slots' mailboxes:
//   target boxes (LANE_REFINE_BOXES)  ->  host: every pair's cell grid  ->  grid build + iterations + states (LANE_REFINE_ITER)
// With QTR_ICP_BLOCK = n the iterations go n launches per chain, and the lane stops enqueuing once every pair has stopped.
static int lane_enqueue_refine(qtr_handle* h, Lane& ln) {
  BatchJob& J = h->job;
  Slot& lead = h->slots[ln.first_slot];
  std::vector<int> ref;
  for (int g : ln.active) {
    const int pair = ln.first_pair + g;
    const int st = J.results[pair].status;
    if (pair_has_scans(J.pairs[pair]) && (st == QTR_OK || st == QTR_ERR_CLIQUE_TOO_SMALL)) {
      ref.push_back(g);
      J.ref_state[pair] = 1;
    }
  }
  ln.active.swap(ref);
  if (ln.active.empty()) return lane_start_chunk(h, ln);
  ln.iv.clear();
  std::vector<int> seqs;
  int max_nt = 1;
  for (int g : ln.active) {
    Slot& s = h->slots[ln.first_slot + g];
    IcpView v = s.icp.v;  // (the slot's arena; the single-pair calls' own view is left as it is)
    // cloud[0] / cloud[1] hold the caller's source / target (as qtr_refine_pair reads them); the normals are the FPFH
    // stage's, nothing writes them after it
    icp_view_bind(v, &J.icp, s.fb.cloud[0].vox, ln.ns[g], s.fb.cloud[0].normals, s.fb.cloud[1].vox, ln.nt[g],
                  s.fb.cloud[1].normals);
    v.cell_cnt = s.icp.cells;
    v.cell_start = s.icp.cells + s.icp.cap_cells + 1;
    v.mail = s.fb.mail;
    ln.iv.push_back(v);
    seqs.push_back(++s.seq);
    max_nt = std::max(max_nt, v.nt);
  }
  const int G = (int)ln.iv.size();
  const IcpView* dv = (const IcpView*)stage_push(&ln.stage, ln.iv.data(), sizeof(IcpView) * (size_t)G, lead.stream);
  const int* ds = (const int*)stage_push(&ln.stage, seqs.data(), sizeof(int) * (size_t)G, lead.stream);
  if (!dv || !ds) {
    snprintf(h->err, sizeof(h->err), "batch refine: the lane's view stage is full");
    return QTR_ERR_HIP;
  }
  QTR_HIP_TRY(h, icp_box_enqueue_group(dv, G, max_nt, ds, lead.stream));
  ln.phase = LANE_REFINE_BOXES;
  return QTR_OK;
}

// the next block of iterations of the lane's refining pairs, ending in their states' mails
static int lane_enqueue_icp_block(qtr_handle* h, Lane& ln) {
  BatchJob& J = h->job;
  Slot& lead = h->slots[ln.first_slot];
  std::vector<int> seqs;
  for (int g : ln.active) seqs.push_back(++h->slots[ln.first_slot + g].seq);
  const int* ds = (const int*)stage_push(&ln.stage, seqs.data(), sizeof(int) * seqs.size(), lead.stream);
  if (!ds) {
    snprintf(h->err, sizeof(h->err), "batch refine: the lane's view stage is full");
    return QTR_ERR_HIP;
  }
  const int block = h->icp_block > 0 ? h->icp_block : J.icp.max_iterations;
  const int m = std::min(block, J.icp.max_iterations - ln.ref_it);
  QTR_HIP_TRY(h, icp_iter_enqueue_group(ln.ref_views, (int)seqs.size(), ln.ref_nchunk, m, ds, lead.stream,
                                        J.icp.method));
  ln.ref_it += m;
  ln.phase = LANE_REFINE_ITER;
  return QTR_OK;
}

// LANE_REFINE_BOXES: the boxes are in; every pair's grid (a pair without a finite target point is done: icp_device's early return)
static int lane_refine_grids(qtr_handle* h, Lane& ln) {
  BatchJob& J = h->job;
  Slot& lead = h->slots[ln.first_slot];
  std::vector<int> keep;
  std::vector<IcpView> V;
  std::vector<QtrIcpState> init;
  int max_nt = 1, max_ncell = 1, max_nchunk = 1;
  const bool voxels = icp_voxel_grid(J.icp.method);
  for (size_t k = 0; k < ln.active.size(); ++k) {
    const int g = ln.active[k], pair = ln.first_pair + g;
    Slot& s = h->slots[ln.first_slot + g];
    IcpView v = ln.iv[k];
    QtrIcpState st0;
    qtr_icp_init(&st0, J.results[pair].T);
    // (method 3: the grid is part of the result, so it follows the rule and QTR_ICP_CELL_CAP, not this arena's capacity; a
    // grid past the slot's table grows it, as the single-pair call does.  Past the cap only this pair is refused.)
    const int grid = voxels ? icp_voxel_grid_of(v, s.mail + MAIL_ICP_BOX, J.icp.max_correspondence_distance, h->err, sizeof(h->err))
                            : (int)icp_grid_of(v, s.mail + MAIL_ICP_BOX, J.icp.max_correspondence_distance, s.icp.cap_cells);
    if (grid <= 0) {
      icp_result_empty(&J.refined[pair], J.results[pair].T);
      J.refined[pair].status = grid < 0 ? QTR_ERR_CAPACITY : QTR_OK;
      J.ref_state[pair] = 2;
      continue;
    }
    if (voxels && v.ncell > s.icp.cap_cells) {
      QTR_HIP_TRY(h, hipStreamSynchronize(lead.stream));  // (nothing of this lane may still read the table)
      QTR_HIP_TRY(h, icp_reserve_cells(s.icp, v.ncell));
      v.cell_cnt = s.icp.cells;
      v.cell_start = s.icp.cells + s.icp.cap_cells + 1;
    }
    keep.push_back(g);
    V.push_back(v);
    init.push_back(st0);
    max_nt = std::max(max_nt, v.nt);
    max_ncell = std::max(max_ncell, v.ncell);
    max_nchunk = std::max(max_nchunk, qtr_div_up(v.ns, QTR_ICP_CHUNK));
  }
  ln.active.swap(keep);
  ln.iv.swap(V);
  if (ln.active.empty()) return lane_start_chunk(h, ln);
  const int G = (int)ln.iv.size();
  const IcpView* dv = (const IcpView*)stage_push(&ln.stage, ln.iv.data(), sizeof(IcpView) * (size_t)G, lead.stream);
  const QtrIcpState* di = (const QtrIcpState*)stage_push(&ln.stage, init.data(), sizeof(QtrIcpState) * (size_t)G, lead.stream);
  if (!dv || !di) {
    snprintf(h->err, sizeof(h->err), "batch refine: the lane's view stage is full");
    return QTR_ERR_HIP;
  }
  QTR_HIP_TRY(h, icp_grid_enqueue_group(dv, di, G, max_nt, max_ncell, lead.stream, voxels));
  ln.ref_views = dv;
  ln.ref_nchunk = max_nchunk;
  ln.ref_it = 0;
  return lane_enqueue_icp_block(h, ln);
}

// LANE_REFINE_ITER: the states are in; another block, or the refined records and the next chunk
static int lane_refine_done(qtr_handle* h, Lane& ln) {
  BatchJob& J = h->job;
  std::vector<QtrIcpState> st(ln.active.size());
  bool all_stopped = true;
  for (size_t k = 0; k < ln.active.size(); ++k) {
    const Slot& s = h->slots[ln.first_slot + ln.active[k]];
    int w[QTR_ICP_MAIL_WORDS];
    for (int i = 0; i < QTR_ICP_MAIL_WORDS; ++i) w[i] = s.mail[MAIL_ICP + 16 * (i / 15) + i % 15];
    memset(&st[k], 0, sizeof(QtrIcpState));
    memcpy(&st[k], w, sizeof(w));
    all_stopped = all_stopped && st[k].stop;
  }
  if (!all_stopped && ln.ref_it < J.icp.max_iterations) return lane_enqueue_icp_block(h, ln);
  for (size_t k = 0; k < ln.active.size(); ++k) {
    const int g = ln.active[k], pair = ln.first_pair + g;
    Slot& s = h->slots[ln.first_slot + g];
    icp_result_from(&J.refined[pair], st[k]);
    J.refined[pair].status = QTR_OK;
    J.ref_state[pair] = 2;
    s.icp_ns = ln.iv[k].ns;  // (QTR_DBG_ICP_CORR / _TRACE of the slot: its last refinement)
    s.icp_iters = st[k].iterations;
  }
  return lane_start_chunk(h, ln);
}

// LANE_VOXELS: both clouds' voxel counters of every pair are in -> means beside the FPFH chain, the matching chain
static int lane_after_voxels(qtr_handle* h, Lane& ln) {
  BatchJob& J = h->job;
  Slot& lead = h->slots[ln.first_slot];
  bool passed_through = false;
  std::vector<int> keep;
  std::vector<FrontBufs*> F;
  std::vector<int> n2;
  std::vector<unsigned long long> seeds;
  for (int g : ln.active) {
    Slot& s = h->slots[ln.first_slot + g];
    qtr_result& r = J.results[ln.first_pair + g];
    const VoxVerdict vs = vox_verdict(s.mail + MAIL_VOX0, ln.Ps[g], h->lim.max_voxels),
                     vt = vox_verdict(s.mail + MAIL_VOX1, ln.Pt[g], h->lim.max_voxels);
    if (vs.reason == VOX_TIMEOUT || vt.reason == VOX_TIMEOUT) {
      batch_fail_pair(h, ln.first_pair + g, QTR_ERR_HIP);
      continue;
    }
    if (vs.passed && vs.reason == VOX_OK) {
      QTR_HIP_TRY(h, hipMemcpyAsync(s.fb.cloud[0].vox, ln.raw_s[g], (size_t)vs.n * 16, hipMemcpyDeviceToDevice, lead.stream));
      passed_through = true;
    }
    if (vt.passed && vt.reason == VOX_OK) {
      QTR_HIP_TRY(h, hipMemcpyAsync(s.fb.cloud[1].vox, ln.raw_t[g], (size_t)vt.n * 16, hipMemcpyDeviceToDevice, lead.stream));
      passed_through = true;
    }
    const int ns = r.n_src = vs.n, nt = r.n_tgt = vt.n;
    if (vs.reason != VOX_OK || vt.reason != VOX_OK) {  // (too large either way, or empty)
      batch_fail_pair(h, ln.first_pair + g, QTR_ERR_CAPACITY);
      continue;
    }
    ln.ns[g] = ns;
    ln.nt[g] = nt;
    s.last_ns = ns;
    s.last_nt = nt;
    keep.push_back(g);
    F.push_back(&s.fb);
    n2.push_back(ns);
    n2.push_back(nt);
    seeds.push_back(J.pairs[ln.first_pair + g].seed);
  }
  ln.active.swap(keep);
  if (ln.active.empty()) return lane_enqueue_solver(h, ln, {});
  const int G = (int)F.size();
  if (passed_through) QTR_HIP_TRY(h, hipEventRecord(lead.ev_vox, lead.stream));
  QTR_HIP_TRY(h, hipStreamWaitEvent(lead.stream2, lead.ev_vox, 0));
  QTR_HIP_TRY(h, mean_enqueue_group(F.data(), G, n2.data(), &ln.stage, lead.stream2));  // beside the FPFH chain
  QTR_HIP_TRY(h, hipEventRecord(lead.ev[EV_JOIN2], lead.stream2));
  ln.long_lists = h->long_lists;
  if (ln.long_lists)
    for (int g : ln.active) QTR_TRY(ensure_long_arenas(h, h->slots[ln.first_slot + g]));
  int max_ncell = 1;  // the largest neighbour grid of the group (0: some pair's does not fit the dense cell table)
  for (int g : ln.active) {
    const Slot& sg = h->slots[ln.first_slot + g];
    const int nc2 = cell_table_cells(sg.mail[MAIL_VOX0 + CNT_NCELL], sg.mail[MAIL_VOX1 + CNT_NCELL]);
    max_ncell = (max_ncell == 0 || nc2 == 0) ? 0 : std::max(max_ncell, nc2);
  }
  QTR_HIP_TRY(h, fpfh_enqueue_group(F.data(), G, n2.data(), J.fp.normal_radius, J.fp.fpfh_radius, &ln.stage, lead.stream,
                                    ln.long_lists, true, max_ncell));
  QTR_HIP_TRY(h, hipStreamWaitEvent(lead.stream, lead.ev[EV_JOIN2], 0));
  for (int g : ln.active) {
    Slot& s = h->slots[ln.first_slot + g];
    s.fb.mail_seq = ++s.seq;
  }
  QTR_HIP_TRY(h, match_enqueue_group(F.data(), G, n2.data(), &J.fp, seeds.data(), &ln.stage, lead.stream, true));
  ln.phase = LANE_MATCH;
  return QTR_OK;
}

// LANE_MATCH: the matcher's counters and the clouds' counter lines are in -> the solver chain on the survivors
static int lane_after_match(qtr_handle* h, Lane& ln) {
  BatchJob& J = h->job;
  Slot& lead = h->slots[ln.first_slot];
  std::vector<int> keep;
  bool drained = false;  // lead.stream has been synchronised by a fallback below
  for (int g : ln.active) {
    Slot& s = h->slots[ln.first_slot + g];
    qtr_result& r = J.results[ln.first_pair + g];
    const qtr_pair_desc& pd = J.pairs[ln.first_pair + g];
    const bool given = pair_has_corr(pd);  // the back end runs on the caller's correspondences, not the matcher's
    const int Lm = s.mail[MAIL_MATCH + MC_NCORR];
    const ListsVerdict lv = lists_verdict(s.mail + MAIL_CNT0, s.mail + MAIL_CNT1, ln.long_lists);
    if (!given) r.n_corr = Lm;
    if (Lm < 0 && !given) {  // the tail's look-back timed out (match.hip): nothing usable was written for this pair
      r.n_corr = 0;
      batch_fail_pair(h, ln.first_pair + g, QTR_ERR_HIP);
      continue;
    }
    if (lv == LISTS_TILE_ERROR) {
      batch_fail_pair(h, ln.first_pair + g, QTR_ERR_HIP);
      continue;
    }
    // (a pair that brought its correspondences does not read the matcher's list: its length is no reason to fail it)
    if (lv == LISTS_CAPACITY || (!given && Lm > h->lim.max_corr)) {
      batch_fail_pair(h, ln.first_pair + g, QTR_ERR_CAPACITY);
      continue;
    }
    if (lv == LISTS_NEED_LONG) {
      // This pair goes through the per-pair path on its own slot, and the handle's later chains include the launch.  The
      // group's chain (lane stream) may still be writing this slot's lists — the mail is published before the
      // kernel's last workgroup is done — so the lane stream is drained first; the pair is registered on the clouds
      // the group's voxel grid read (the pre-processed sweeps when qtr_set_batch_preprocess is on, the staged copies
      // of host scans: device pointers either way), and on the caller's correspondences when it brought some.
      h->long_lists = true;
      if (!drained) QTR_HIP_TRY(h, hipStreamSynchronize(lead.stream));
      drained = true;
      qtr_frontend_params f1 = J.fp;
      f1.seed = pd.seed;
      const int rc1 = register_pair_impl(h, s, (const float*)ln.raw_s[g], ln.Ps[g], (const float*)ln.raw_t[g], ln.Pt[g], &f1,
                                         &J.prm, &r, pd.clique, pd.final_inliers, pd.cap, QTR_MEM_DEVICE, J.mem, pd.src_corr4,
                                         pd.tgt_corr4, given ? pd.n_corr : -1);
      if (rc1 == QTR_ERR_HIP) return rc1;
      J.finished[ln.first_pair + g] = 1;
      ++J.done;
      if (J.refine && (r.status == QTR_OK || r.status == QTR_ERR_CLIQUE_TOO_SMALL)) {
        // (the slot holds this pair's clouds as after qtr_register_pair: qtr_refine_pair's own path, on the slot's stream)
        J.ref_state[ln.first_pair + g] = 1;
        if (icp_device(h, s, s.fb.cloud[0].vox, s.last_ns, s.fb.cloud[1].vox, s.last_nt, s.fb.cloud[1].normals,
                       s.fb.cloud[0].normals, r.T, &J.icp,
                       &J.refined[ln.first_pair + g]) != QTR_OK)
          return QTR_ERR_HIP;
        J.ref_state[ln.first_pair + g] = 2;
      }
      continue;
    }
    if (given) {  // (host correspondences: behind the matching chain on the lane's stream — the matched clouds are not needed)
      QTR_TRY(corr_stage(h, s, pd.src_corr4, pd.tgt_corr4, pd.n_corr, J.mem, lead.stream, &ln.csrc[g], &ln.ctgt[g]));
      ln.L[g] = pd.n_corr;
    } else {
      QTR_HIP_TRY(h, gather_matched_enqueue(s.fb, Lm, s.m_src, s.m_tgt, lead.stream));  // no-op after the fused tail
      ln.csrc[g] = s.m_src;
      ln.ctgt[g] = s.m_tgt;
      ln.L[g] = Lm;
    }
    keep.push_back(g);
  }
  return lane_enqueue_solver(h, ln, keep);
}

// LANE_SOLVE: every pair's record and solver state are in -> follow-ups, the records, the lists; then refinement or the
// next chunk
static int lane_after_solve(qtr_handle* h, Lane& ln) {
  BatchJob& J = h->job;
  Slot& lead = h->slots[ln.first_slot];
  int copies = 0;
  for (int g : ln.active) {
    Slot& s = h->slots[ln.first_slot + g];
    const int pair = ln.first_pair + g;
    qtr_result& r = J.results[pair];
    const qtr_pair_desc& pd = J.pairs[pair];
    // Follow-up work of ONE pair of the group runs on the lane's stream (the lane's chain owns the slot's arenas) and is
    // waited for there: the slot's own stream is idle.
    QTR_TRY(solve_followup(h, s, ln.csrc[g], ln.ctgt[g], ln.L[g], &J.prm, lead.stream, false));
    result_from_mail(s, &r);
    // (not finish_registration's way: a list that does not fit marks the pair, the lane goes on and synchronises once)
    const int rc_c = list_out_enqueue(h, pd.clique, s.sb.clique, r.n_clique, pd.cap, J.mem, lead.stream, &copies);
    const int rc_f = list_out_enqueue(h, pd.final_inliers, s.sb.final_inl, r.n_final, pd.cap, J.mem, lead.stream, &copies);
    if (rc_c == QTR_ERR_HIP || rc_f == QTR_ERR_HIP) return QTR_ERR_HIP;
    if (rc_c != QTR_OK || rc_f != QTR_OK) r.status = QTR_ERR_CAPACITY;
    J.finished[pair] = 1;
    ++J.done;
  }
  if (copies) QTR_HIP_TRY(h, hipStreamSynchronize(lead.stream));
  if (J.refine) return lane_enqueue_refine(h, ln);
  return lane_start_chunk(h, ln);
}

// the mailbox word that ends a phase's chain (the voxel stage mails one line per cloud: MAIL_SEQ_VOX0 as well)
static int lane_mail_index(LanePhase phase) {
  switch (phase) {
    case LANE_VOXELS: return MAIL_SEQ_VOX1;
    case LANE_MATCH: return MAIL_SEQ_MATCH;
    case LANE_SOLVE: return MAIL_SEQ_SOLVE;
    case LANE_REFINE_BOXES: return MAIL_SEQ_ICP_BOX;
    default: return MAIL_SEQ_ICP;
  }
}

// advances the lane by at most one chain, once every active slot's mail is in; *progress is set when it did
static int lane_poll(qtr_handle* h, Lane& ln, bool* progress) {
  if (ln.phase == LANE_IDLE) return QTR_OK;
  for (int g : ln.active) {
    const Slot& s = h->slots[ln.first_slot + g];
    if (ln.phase == LANE_VOXELS && !mail_ready(s, MAIL_SEQ_VOX0, s.seq)) return QTR_OK;
    if (!mail_ready(s, lane_mail_index(ln.phase), s.seq)) return QTR_OK;
  }
  *progress = true;
  switch (ln.phase) {
    case LANE_VOXELS: return lane_after_voxels(h, ln);
    case LANE_MATCH: return lane_after_match(h, ln);
    case LANE_SOLVE: return lane_after_solve(h, ln);
    case LANE_REFINE_BOXES: return lane_refine_grids(h, ln);
    default: return lane_refine_done(h, ln);
  }
}

int qtr_set_batch_preprocess(qtr_handle* h, const qtr_pw_params* pw, const qtr_ip_params* ip) {
  if (!h || (pw == nullptr) != (ip == nullptr)) return QTR_ERR_BAD_ARG;
  if (h->job.active) {
    snprintf(h->err, sizeof(h->err), "a batch is in flight on this handle (call qtr_wait first)");
    return QTR_ERR_BAD_ARG;
  }
  h->pre_on = pw != nullptr;
  if (pw) {
    h->pre_pw = *pw;
    h->pre_ip = *ip;
  }
  return QTR_OK;
}

// icp = NULL: plain qtr_submit_batch (no refine phase, no ICP arena, no extra launch)
static int submit_batch_impl(qtr_handle* h, const qtr_pair_desc* pairs, int B, const qtr_frontend_params* fp,
                             const qtr_params* prm, const qtr_icp_params* icp, qtr_result* results, qtr_icp_result* refined,
                             int mem, bool kf = false /* pairs: BatchJob::kf_shadow */) {
  if (h->job.active) {
    snprintf(h->err, sizeof(h->err), "a batch is already in flight on this handle (call qtr_wait first)");
    return QTR_ERR_BAD_ARG;
  }
  if (B < 0 || (B > 0 && (!pairs || !results)) || !fp) {
    snprintf(h->err, sizeof(h->err), "bad batch arguments");
    return QTR_ERR_BAD_ARG;
  }
  const int rc = check_params(h, prm);
  if (rc != QTR_OK) return rc;
  for (auto& sl : h->slots) sl.reg_ready = 0;  // (every slot's clouds are the batch's from here on)
  if (fp->normal_radius > fp->fpfh_radius) {
    snprintf(h->err, sizeof(h->err), "[FPFHManager]: Normal should be lower than fpfh_radius!!!!");
    return QTR_ERR_BAD_ARG;
  }
  QTR_HIP_TRY(h, hipSetDevice(h->device));
  if (icp)  // every slot's ICP arena, and a cell table no grid of the search methods outgrows (no allocation in the lanes;
            // method 3's grid is the rule's, so a lane grows the table of a pair that needs more: lane_refine_grids)
    for (auto& sl : h->slots) {
      QTR_HIP_TRY(h, icp_reserve(sl.icp, h->lim.max_voxels, QTR_ICP_MAX_ITERATIONS));
      QTR_HIP_TRY(h, icp_reserve_cells(sl.icp, QTR_ICP_BATCH_CELLS));
      if (icp_voxel_grid(icp->method)) QTR_HIP_TRY(h, icp_reserve_vox(sl.icp, h->lim.max_voxels));
    }
  BatchJob& J = h->job;
  J.pairs = pairs;
  J.B = B;
  J.next = 0;
  J.done = 0;
  J.fp = *fp;
  J.prm = *prm;
  J.results = results;
  J.mem = mem;
  J.kf = kf;
  J.active = true;
  J.finished.assign((size_t)B, 0);
  for (int i = 0; i < B; ++i) {  // until a pair's record is final it says so (a caller that looks only at the
    memset(&results[i], 0, sizeof(qtr_result));  // per-pair status can tell "never ran" from "ran, no solution")
    results[i].status = QTR_ERR_NOT_RUN;
  }
  J.refine = icp != nullptr;
  J.refined = refined;
  J.ref_state.assign(J.refine ? (size_t)B : 0, 0);
  if (J.refine) {
    J.icp = *icp;
    for (int i = 0; i < B; ++i) {
      memset(&refined[i], 0, sizeof(qtr_icp_result));
      refined[i].status = QTR_ERR_NOT_RUN;
    }
  }
  for (auto& ln : h->lanes) {
    const int r = lane_start_chunk(h, ln);
    if (r != QTR_OK) {
      batch_abort(h);  // earlier lanes may already have work in flight
      return r;
    }
  }
  return QTR_OK;
}

int qtr_submit_batch(qtr_handle* h, const qtr_pair_desc* pairs, int B, const qtr_frontend_params* fp,
                     const qtr_params* prm, qtr_result* results, int mem) {
  if (!h) return QTR_ERR_BAD_ARG;
  return submit_batch_impl(h, pairs, B, fp, prm, nullptr, results, nullptr, mem);
}

int qtr_submit_batch_refine(qtr_handle* h, const qtr_pair_desc* pairs, int B, const qtr_frontend_params* fp,
                            const qtr_params* prm, const qtr_icp_params* icp, qtr_result* results, qtr_icp_result* refined,
                            int mem) {
  if (!h) return QTR_ERR_BAD_ARG;
  if (h->job.active) {
    snprintf(h->err, sizeof(h->err), "a batch is already in flight on this handle (call qtr_wait first)");
    return QTR_ERR_BAD_ARG;
  }
  const int rc = check_icp_params(h, icp);
  if (rc != QTR_OK) return rc;
  if (B > 0 && !refined) {
    snprintf(h->err, sizeof(h->err), "bad batch arguments (refined is NULL)");
    return QTR_ERR_BAD_ARG;
  }
  return submit_batch_impl(h, pairs, B, fp, prm, icp, results, refined, mem);
}

int qtr_submit_batch_keyframes(qtr_handle* h, const qtr_kf_pair_desc* pairs, int B, const qtr_frontend_params* fp,
                               const qtr_params* prm, const qtr_icp_params* icp, qtr_result* results,
                               qtr_icp_result* refined) {
  if (!h) return QTR_ERR_BAD_ARG;
  if (h->job.active) {
    snprintf(h->err, sizeof(h->err), "a batch is already in flight on this handle (call qtr_wait first)");
    return QTR_ERR_BAD_ARG;
  }
  if (B < 0 || (B > 0 && (!pairs || !results)) || !fp) {
    snprintf(h->err, sizeof(h->err), "bad batch arguments");
    return QTR_ERR_BAD_ARG;
  }
  if (icp) QTR_TRY(check_icp_params(h, icp));
  if ((icp == nullptr) != (refined == nullptr) && (B > 0 || refined)) {
    snprintf(h->err, sizeof(h->err), "bad batch arguments (refined goes with icp)");
    return QTR_ERR_BAD_ARG;
  }
  for (int i = 0; i < B; ++i) QTR_TRY(check_keyframes(h, pairs[i].src, pairs[i].tgt, fp));
  std::vector<qtr_pair_desc>& sh = h->job.kf_shadow;
  sh.assign((size_t)B, qtr_pair_desc{});
  for (int i = 0; i < B; ++i) {
    sh[(size_t)i].src_raw4 = (const float*)pairs[i].src;  // (the lanes read them back as keyframes: BatchJob::kf)
    sh[(size_t)i].n_src = pairs[i].src->info.n_voxels;
    sh[(size_t)i].tgt_raw4 = (const float*)pairs[i].tgt;
    sh[(size_t)i].n_tgt = pairs[i].tgt->info.n_voxels;
    sh[(size_t)i].seed = pairs[i].seed;
    sh[(size_t)i].clique = pairs[i].clique;
    sh[(size_t)i].final_inliers = pairs[i].final_inliers;
    sh[(size_t)i].cap = pairs[i].cap;
  }
  return submit_batch_impl(h, sh.data(), B, fp, prm, icp, results, refined, QTR_MEM_HOST, true);
}

int qtr_wait(qtr_handle* h) {
  if (!h) return QTR_ERR_BAD_ARG;
  BatchJob& J = h->job;
  if (!J.active) return QTR_OK;
  (void)hipSetDevice(h->device);
  int rc = QTR_OK;
  unsigned long idle = 0;
  while (true) {
    bool any_active = false, progress = false;
    for (auto& ln : h->lanes) {
      if (ln.phase == LANE_IDLE) continue;
      any_active = true;
      rc = lane_poll(h, ln, &progress);
      if (rc != QTR_OK) break;
    }
    if (rc != QTR_OK || !any_active) break;
    if (progress) {
      idle = 0;
      continue;
    }
    __builtin_ia32_pause();
    if ((++idle & 0xfffff) == 0) {  // nothing moved for a long while: has a launch failed, is the device gone?
      for (auto& ln : h->lanes) {
        if (ln.phase == LANE_IDLE) continue;
        Slot& lead = h->slots[ln.first_slot];
        const hipError_t q = hipStreamQuery(lead.stream);
        if (q == hipSuccess) {  // stream drained, yet a mailbox never arrived
          bool all = true;
          for (int g : ln.active) {
            Slot& s = h->slots[ln.first_slot + g];
            all = all && mail_ready(s, lane_mail_index(ln.phase), s.seq);
          }
          if (!all) {
            snprintf(h->err, sizeof(h->err), "batch lane drained its stream without publishing phase %d", (int)ln.phase);
            rc = QTR_ERR_HIP;
          }
        } else if (q != hipErrorNotReady) {
          snprintf(h->err, sizeof(h->err), "batch lane: %s", hipGetErrorString(q));
          rc = QTR_ERR_HIP;
        }
        (void)hipGetLastError();
      }
      if (rc != QTR_OK) break;
    }
  }
  if (rc != QTR_OK) batch_abort(h);  // leave the handle usable, every record says what happened to its pair
  else refine_fill_rest(h, false);
  J.active = false;
  return rc;
}

// ------------------------------------------------------------------------------------------------
// ---- ICP refinement (icp.hip) -----------------------------------------------------------------------------------------
void qtr_default_icp_params(qtr_icp_params* p) {
  memset(p, 0, sizeof(*p));
  p->max_correspondence_distance = 1.0;
  p->transformation_epsilon = 1e-7;
  p->euclidean_fitness_epsilon = 1e-6;
  p->max_iterations = 30;
  p->method = QTR_ICP_POINT_TO_PLANE;
  p->min_correspondences = 0;
  p->normal_radius = 0.5f;
}

static bool icp_finite(double x) { return x - x == 0.0; }

static int check_icp_params(qtr_handle* h, const qtr_icp_params* p) {
  if (!p || !icp_finite(p->max_correspondence_distance) || !(p->max_correspondence_distance > 0) ||
      !icp_finite(p->transformation_epsilon) || p->transformation_epsilon < 0 || !icp_finite(p->euclidean_fitness_epsilon) ||
      p->euclidean_fitness_epsilon < 0 || p->max_iterations < 1 || p->max_iterations > QTR_ICP_MAX_ITERATIONS ||
      !icp_method_known(p->method) || p->min_correspondences < 0 ||
      !icp_finite((double)p->normal_radius) || !(p->normal_radius > 0)) {
    snprintf(h->err, sizeof(h->err), "invalid ICP parameter");
    return QTR_ERR_BAD_ARG;
  }
  return QTR_OK;
}

// The single-call loop on the slot's ICP arena, which icp_device and the voxel map's registration (voxelmap.hip) share: the
// empty result, the slot's debug / timing fields, then - unless `empty`: there is nothing to refine - bind() (the caller's
// checks, reservations and view), before(&go) (what precedes the loop and ends with the initial state on the device, between
// EV_ICP_BEGIN and EV_ICP_GRID; go = false: nothing to refine after all), launch(v) per iteration with no host read-back inside
// a block of QTR_ICP_BLOCK launches (0: all max_iterations of them in one go), the final read-back, the result and the times.
extern "C++" {  // (a template, inside this file's extern "C")
template <class Bind, class Before, class Launch>
static int icp_loop(qtr_handle* h, Slot& s, int ns, bool empty, const double* guess, const qtr_icp_params* prm,
                    qtr_icp_result* res, Bind bind, Before before, Launch launch) {
  icp_result_empty(res, guess);
  res->status = QTR_OK;
  s.icp_ns = 0;
  s.icp_iters = 0;
  s.icp_ms[0] = s.icp_ms[1] = 0.f;
  if (empty) return QTR_OK;
  QTR_TRY(bind());
  IcpBufs& B = s.icp;
  const IcpView& v = B.v;
  const hipStream_t st = s.stream;
  QTR_HIP_TRY(h, hipEventRecord(s.ev[EV_ICP_BEGIN], st));
  bool go = true;
  QTR_TRY(before(&go));
  if (!go) return QTR_OK;
  QTR_HIP_TRY(h, hipEventRecord(s.ev[EV_ICP_GRID], st));
  const int block = h->icp_block > 0 ? h->icp_block : prm->max_iterations;
  for (int it = 0; it < prm->max_iterations;) {
    const int m = std::min(block, prm->max_iterations - it);
    for (int k = 0; k < m; ++k) launch(v);
    QTR_HIP_TRY(h, hipGetLastError());
    it += m;
    if (it >= prm->max_iterations) break;
    QTR_HIP_TRY(h, hipMemcpyAsync(B.h_state, v.st, sizeof(QtrIcpState), hipMemcpyDeviceToHost, st));
    QTR_HIP_TRY(h, hipStreamSynchronize(st));
    if (B.h_state->stop) break;
  }
  QTR_HIP_TRY(h, hipEventRecord(s.ev[EV_ICP_END], st));
  QTR_HIP_TRY(h, hipMemcpyAsync(B.h_state, v.st, sizeof(QtrIcpState), hipMemcpyDeviceToHost, st));
  QTR_HIP_TRY(h, hipStreamSynchronize(st));
  icp_result_from(res, *B.h_state);
  s.icp_ns = ns;
  s.icp_iters = B.h_state->iterations;
  float ms = 0;
  if (hipEventElapsedTime(&ms, s.ev[EV_ICP_BEGIN], s.ev[EV_ICP_GRID]) == hipSuccess) s.icp_ms[0] = ms;
  if (hipEventElapsedTime(&ms, s.ev[EV_ICP_GRID], s.ev[EV_ICP_END]) == hipSuccess) s.icp_ms[1] = ms;
  s.times_pending = TIMES_NONE;
  s.times = qtr_stage_times{};
  s.times.total = s.icp_ms[0] + s.icp_ms[1];
  return QTR_OK;
}
}  // extern "C++"

// icp_loop on two device-resident clouds: before the loop the grid over the target (box, one read-back that sizes the cell
// table, counting sort, method 3's records).
static int icp_device(qtr_handle* h, Slot& s, const float4* d_src, int ns, const float4* d_tgt, int nt, const float4* d_nrm,
                      const float4* d_src_nrm, const double* guess, const qtr_icp_params* prm, qtr_icp_result* res) {
  const bool voxels = icp_voxel_grid(prm->method);
  const hipStream_t st = s.stream;
  IcpBufs& B = s.icp;
  IcpView& v = B.v;
  const auto bind = [&]() -> int {
    if (icp_reads_src_normals(prm->method) && (!d_nrm || !d_src_nrm)) {
      snprintf(h->err, sizeof(h->err), "plane-to-plane needs the normals of both clouds");
      return QTR_ERR_BAD_ARG;
    }
    QTR_HIP_TRY(h, icp_reserve(B, h->lim.max_voxels, QTR_ICP_MAX_ITERATIONS));
    if (voxels) QTR_HIP_TRY(h, icp_reserve_vox(B, h->lim.max_voxels));
    icp_view_bind(v, prm, d_src, ns, d_src_nrm, d_tgt, nt, d_nrm);
    return QTR_OK;
  };
  const auto before = [&](bool* go) -> int {
    QTR_HIP_TRY(h, icp_box_enqueue(v, B.h_bbox, st));
    QTR_HIP_TRY(h, hipMemcpyAsync(B.h_bbox, v.bbox, 24, hipMemcpyDeviceToHost, st));
    QTR_HIP_TRY(h, hipStreamSynchronize(st));
    const int grid = voxels ? icp_voxel_grid_of(v, B.h_bbox, prm->max_correspondence_distance, h->err, sizeof(h->err))
                            : (int)icp_grid_of(v, B.h_bbox, prm->max_correspondence_distance, QTR_ICP_CELL_CAP);
    if (grid < 0) return QTR_ERR_CAPACITY;
    if (grid == 0) {  // no finite target point
      *go = false;
      return QTR_OK;
    }
    QTR_HIP_TRY(h, icp_reserve_cells(B, v.ncell));
    v.cell_cnt = B.cells;
    v.cell_start = B.cells + B.cap_cells + 1;
    QtrIcpState st0;
    qtr_icp_init(&st0, guess);
    QTR_HIP_TRY(h, icp_grid_enqueue(v, st0, st, voxels));
    return QTR_OK;
  };
  const dim3 chunks(qtr_div_up(ns, QTR_ICP_CHUNK));
  return icp_loop(h, s, ns, ns == 0 || nt == 0, guess, prm, res, bind, before,
                  [&](const IcpView& w) { icp_iter_launch(prm->method, chunks, st, w); });
}

static const double kIcpIdentity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};

static bool icp_guess_ok(const double* g) {
  for (int k = 0; k < 16; ++k)
    if (!icp_finite(g[k])) return false;
  return true;
}

// What qtr_icp, qtr_gicp and qtr_evaluate do with their two clouds (0: source, 1: target) before anything runs: the argument
// and the capacity checks (bad_args, cloud: the entry's own words in the messages; guess may be null), then — run: the entry
// has something to launch — host clouds into the raw-scan buffers (max_points >= max_voxels points each) and the host normal
// sets the entry names into cloud[c].normals.  pts / nrm come back as device pointers.
static int clouds_stage(qtr_handle* h, Slot& s, const char* bad_args, const char* cloud, const double* guess, int mem,
                        const int n[2], const float4* pts[2], const float4* nrm[2], bool run) {
  if (n[0] < 0 || n[1] < 0 || (n[0] > 0 && !pts[0]) || (n[1] > 0 && !pts[1]) ||
      (mem != QTR_MEM_HOST && mem != QTR_MEM_DEVICE) || (guess && !icp_guess_ok(guess))) {
    snprintf(h->err, sizeof(h->err), "%s", bad_args);
    return QTR_ERR_BAD_ARG;
  }
  if (n[0] > h->lim.max_voxels || n[1] > h->lim.max_voxels) {
    snprintf(h->err, sizeof(h->err), "%s exceeds max_voxels=%d", cloud, h->lim.max_voxels);
    return QTR_ERR_CAPACITY;
  }
  if (!run) return QTR_OK;
  QTR_HIP_TRY(h, hipSetDevice(h->device));
  if (mem != QTR_MEM_HOST) return QTR_OK;
  float4* const in[2] = {s.in_src, s.in_tgt};
  for (int c = 0; c < 2; ++c) {
    if (n[c] > 0) QTR_HIP_TRY(h, hipMemcpyAsync(in[c], pts[c], (size_t)n[c] * 16, hipMemcpyHostToDevice, s.stream));
    pts[c] = in[c];
  }
  for (int c = 0; c < 2; ++c)
    if (nrm[c] && n[c] > 0) {
      QTR_HIP_TRY(h, hipMemcpyAsync(s.fb.cloud[c].normals, nrm[c], (size_t)n[c] * 16, hipMemcpyHostToDevice, s.stream));
      nrm[c] = s.fb.cloud[c].normals;
    }
  return QTR_OK;
}

// The normals of `count` device clouds at normal_radius, for a caller that did not bring them: the normal stage of the FPFH
// chain (qtr_fpfh's dense mode) on copies of the clouds in the arenas cloud[first ..], all in one chain.  nrm[k] = the
// arena's normals.
static int normals_at_radius(qtr_handle* h, Slot& s, int first, int count, const float4* const* pts, const int* n,
                             float normal_radius, const float4** nrm) {
  for (int k = 0; k < count; ++k) {
    CloudBufs& cb = s.fb.cloud[first + k];
    QTR_HIP_TRY(h, hipMemcpyAsync(cb.vox, pts[k], (size_t)n[k] * 16, hipMemcpyDeviceToDevice, s.stream));
    QTR_HIP_TRY(h, hipMemsetAsync(cb.counts, 0, 16 * sizeof(int), s.stream));
    QTR_HIP_TRY(h, set_count_enqueue(cb, CNT_NVOX, n[k], s.stream));
  }
  QTR_TRY(ensure_long_arenas(h, s));
  QTR_HIP_TRY(h, fpfh_enqueue(s.fb, first, count, n, normal_radius, normal_radius, s.stream, false, false, true));
  for (int c = first; c < first + count; ++c)
    QTR_HIP_TRY(h, hipMemcpyAsync(s.pinned_i32 + 16 * c, s.fb.cloud[c].counts, 16 * sizeof(int), hipMemcpyDeviceToHost,
                                  s.stream));
  QTR_HIP_TRY(h, hipStreamSynchronize(s.stream));
  for (int k = 0; k < count; ++k) {
    if (s.pinned_i32[16 * (first + k) + CNT_NBR_CAPACITY]) {
      snprintf(h->err, sizeof(h->err), "normals at normal_radius: radius-neighbour lists exceed the long-list arena "
               "(qtr_limits.max_long_neighbors is %d)", h->lim.max_long_neighbors);
      return QTR_ERR_CAPACITY;
    }
    nrm[k] = s.fb.cloud[first + k].normals;
  }
  return QTR_OK;
}

int qtr_icp(qtr_handle* h, int slot, const float* src4, int n_s, const float* tgt4, int n_t, const float* tgt_normals4,
            const double guess[16], const qtr_icp_params* prm, qtr_icp_result* res, int mem) {
  Slot* sp = get_slot(h, slot);
  if (!sp || !res) return QTR_ERR_BAD_ARG;
  memset(res, 0, sizeof(*res));
  Slot& s = *sp;
  int rc = check_icp_params(h, prm);
  if (rc != QTR_OK) return res->status = rc;
  if (icp_reads_src_normals(prm->method))  // (at normal_radius)
    return qtr_gicp(h, slot, src4, n_s, nullptr, tgt4, n_t, tgt_normals4, guess, prm, res, mem);
  const bool plane = icp_reads_tgt_normals(prm->method), run = n_s > 0 && n_t > 0;
  const int n[2] = {n_s, n_t};
  const float4* pts[2] = {(const float4*)src4, (const float4*)tgt4};
  const float4* nrm[2] = {nullptr, plane ? (const float4*)tgt_normals4 : nullptr};
  rc = clouds_stage(h, s, "bad ICP arguments", "ICP cloud", guess, mem, n, pts, nrm, run);
  // the target's missing normals: on a copy of the target in the FIRST cloud's arena
  if (rc == QTR_OK && run && plane && !nrm[1]) rc = normals_at_radius(h, s, 0, 1, pts + 1, n + 1, prm->normal_radius, nrm + 1);
  if (rc == QTR_OK) rc = icp_device(h, s, pts[0], n_s, pts[1], n_t, nrm[1], nullptr, guess ? guess : kIcpIdentity, prm, res);
  return res->status = rc;
}

// Plane-to-plane on any two clouds.  The source lives in the first cloud's arena and the target in the second's (as after a
// registration); a normal set the caller does not bring comes from normals_at_radius — both clouds in one chain when both
// are missing.
int qtr_gicp(qtr_handle* h, int slot, const float* src4, int n_s, const float* src_normals4, const float* tgt4, int n_t,
             const float* tgt_normals4, const double guess[16], const qtr_icp_params* prm, qtr_icp_result* res, int mem) {
  Slot* sp = get_slot(h, slot);
  if (!sp || !res) return QTR_ERR_BAD_ARG;
  memset(res, 0, sizeof(*res));
  Slot& s = *sp;
  int rc = check_icp_params(h, prm);
  if (rc != QTR_OK) return res->status = rc;
  if (!icp_reads_src_normals(prm->method)) {
    snprintf(h->err, sizeof(h->err), "qtr_gicp: method must be QTR_ICP_PLANE_TO_PLANE or QTR_ICP_VOXEL_PLANE_TO_PLANE");
    return res->status = QTR_ERR_BAD_ARG;
  }
  const bool run = n_s > 0 && n_t > 0;
  const int n[2] = {n_s, n_t};
  const float4* pts[2] = {(const float4*)src4, (const float4*)tgt4};
  const float4* nrm[2] = {(const float4*)src_normals4, (const float4*)tgt_normals4};
  rc = clouds_stage(h, s, "bad ICP arguments", "ICP cloud", guess, mem, n, pts, nrm, run);
  const int first = nrm[0] ? 1 : 0, last = nrm[1] ? 0 : 1;  // clouds first..last need their normals
  if (rc == QTR_OK && run && first <= last)
    rc = normals_at_radius(h, s, first, last - first + 1, pts + first, n + first, prm->normal_radius, nrm + first);
  if (rc == QTR_OK) rc = icp_device(h, s, pts[0], n_s, pts[1], n_t, nrm[1], nrm[0], guess ? guess : kIcpIdentity, prm, res);
  return res->status = rc;
}

int qtr_refine_pair(qtr_handle* h, int slot, const double guess[16], const qtr_icp_params* prm, qtr_icp_result* res) {
  Slot* sp = peek_slot(h, slot);  // (a refinement leaves the registration's clouds as they are: it may be repeated)
  if (!sp || !res) return QTR_ERR_BAD_ARG;
  memset(res, 0, sizeof(*res));
  Slot& s = *sp;
  int rc = check_icp_params(h, prm);
  if (rc != QTR_OK) return res->status = rc;
  if (!s.reg_ready) {
    snprintf(h->err, sizeof(h->err), "qtr_refine_pair: the slot's last call was not a registration");
    return res->status = QTR_ERR_BAD_ARG;
  }
  if (guess && !icp_guess_ok(guess)) {
    snprintf(h->err, sizeof(h->err), "bad ICP guess");
    return res->status = QTR_ERR_BAD_ARG;
  }
  QTR_HIP_TRY(h, hipSetDevice(h->device));
  // cloud[0] / cloud[1] hold the caller's source / target whatever roles the matcher gave them (it swaps views, not
  // arenas); the normals of both are the FPFH stage's, at the registration's normal_radius (k2_normals is their only
  // writer: the matcher and the solver read them or leave them alone)
  rc = icp_device(h, s, s.fb.cloud[0].vox, s.last_ns, s.fb.cloud[1].vox, s.last_nt, s.fb.cloud[1].normals,
                  s.fb.cloud[0].normals, guess ? guess : s.reg_T, prm, res);
  return res->status = rc;
}

// ------------------------------------------------------------------------------------------------
// ---- registration evaluation (eval.hip) -------------------------------------------------------------------------------
void qtr_default_eval_params(qtr_eval_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->max_correspondence_distance = 1.0;
}

static int check_eval_params(qtr_handle* h, const qtr_eval_params* p) {
  if (!p || !icp_finite(p->max_correspondence_distance) || !(p->max_correspondence_distance > 0)) {
    snprintf(h->err, sizeof(h->err), "evaluation: max_correspondence_distance must be finite and positive");
    return QTR_ERR_BAD_ARG;
  }
  return QTR_OK;
}
static int check_eval_T(qtr_handle* h, const double* T) {
  if (!T || !qtr_submap_pose_finite(T)) {
    snprintf(h->err, sizeof(h->err), "evaluation: T is NULL or has a non-finite entry in rows 0 - 2");
    return QTR_ERR_BAD_ARG;
  }
  return QTR_OK;
}

static_assert(QTR_EVAL_MAX_PAIRS == QTR_EVAL_MAX_BATCH, "the arena's fixed part holds a whole batch");
struct EvalPair {
  const float4 *src, *tgt, *nrm;  // device pointers (nrm may be null)
  int ns, nt;
  const double* T;
};

// B evaluations on device-resident clouds, validated by the caller.  Two host waits whatever B is: the target boxes (they
// size the cell tables) and the records.  grouped = false (B == 1): the single-pair kernels with the view by value.
static int eval_device(qtr_handle* h, Slot& s, const EvalPair* P, int B, double max_d, bool grouped, qtr_eval_result* out) {
  QtrEvalRecord empty;
  {
    double S0[QTR_EVAL_NT] = {};
    qtr_eval_finish(S0, &empty);  // (what a pair without a considered source point reports)
  }
  size_t var = 0;
  int max_nt = 0, max_nchunk = 0;
  for (int b = 0; b < B; ++b) {
    memset(&out[b], 0, sizeof(out[b]));
    out[b].status = QTR_OK;
    for (int k = 0; k < 16; ++k) out[b].T[k] = P[b].T[k];
    eval_result_from(&out[b], empty);
    const int nchunk = qtr_div_up(P[b].ns, QTR_ICP_CHUNK);
    var += qtr_up256((size_t)nchunk * QTR_EVAL_NT * 8) + 2 * qtr_up256((size_t)P[b].nt * 16) + qtr_up256((size_t)P[b].nt * 8) +
           qtr_up256((size_t)P[b].ns * 4);
    max_nt = std::max(max_nt, P[b].nt);
    max_nchunk = std::max(max_nchunk, nchunk);
  }
  if (max_nchunk == 0) return QTR_OK;
  EvalBufs& E = s.eval;
  QTR_HIP_TRY(h, eval_reserve(E, var));
  char* p = E.d_var;
  auto take = [&](size_t n) {
    char* r = p;
    p += qtr_up256(n);
    return r;
  };
  for (int b = 0; b < B; ++b) {
    IcpView& v = E.h_views[b];
    memset((void*)&v, 0, sizeof(v));
    v.src = P[b].src;
    v.tgt = P[b].tgt;
    v.nrm = P[b].nrm;
    v.ns = P[b].ns;
    v.nt = P[b].nt;
    v.partials = (double*)take((size_t)qtr_div_up(v.ns, QTR_ICP_CHUNK) * QTR_EVAL_NT * 8);
    v.spts = (float4*)take((size_t)v.nt * 16);
    v.snrm = (float4*)take((size_t)v.nt * 16);
    v.place = (int*)take((size_t)v.nt * 8);
    v.corr = (int*)take((size_t)v.ns * 4);
    v.bbox = E.d_boxes + 8 * b;
    v.st = E.d_state + b;
    v.ticket = E.d_tickets + 16 * b;
    v.trace = (double*)(E.d_rec + b);
    v.cfg.max_d2 = max_d * max_d;
    qtr_icp_init(&E.h_init[b], P[b].T);
  }
  E.last_corr = E.h_views[0].corr;
  E.last_ns = 0;
  const hipStream_t st = s.stream;
  const size_t view_block = (sizeof(IcpView) + sizeof(QtrIcpState)) * QTR_EVAL_MAX_BATCH;
  const ViewExt<IcpView> x{E.d_views, {0, 0, 0}};
  // first wait: the boxes of the finite target points
  if (!grouped) {
    QTR_HIP_TRY(h, icp_box_enqueue(E.h_views[0], E.h_boxes, st));
  } else {
    QTR_HIP_TRY(h, hipMemcpyAsync(E.d_views, E.h_views, view_block, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_icp_box_init_group, dim3(1, B), dim3(64), 0, st, x);
    if (max_nt > 0) hipLaunchKernelGGL(k_eval_bbox_group, dim3(qtr_div_up(max_nt, 256), B), dim3(256), 0, st, x);
  }
  QTR_HIP_TRY(h, hipGetLastError());
  QTR_HIP_TRY(h, hipMemcpyAsync(E.h_boxes, E.d_boxes, (size_t)B * 32, hipMemcpyDeviceToHost, st));
  QTR_HIP_TRY(h, hipStreamSynchronize(st));
  size_t cell_ints = 0;
  int max_ncell = 0;
  for (int b = 0; b < B; ++b) {
    IcpView& v = E.h_views[b];
    (void)icp_grid_of(v, E.h_boxes + 8 * b, max_d, QTR_EVAL_CELLS);  // (no finite target point: the empty grid)
    cell_ints += 2 * ((size_t)v.ncell + 1);
    max_ncell = std::max(max_ncell, v.ncell);
  }
  QTR_HIP_TRY(h, eval_reserve_cells(E, cell_ints));
  int* c = E.cells;
  for (int b = 0; b < B; ++b) {
    IcpView& v = E.h_views[b];
    v.cell_cnt = c;
    v.cell_start = c + v.ncell + 1;
    c += 2 * ((size_t)v.ncell + 1);
  }
  // second wait: the records
  if (!grouped) {
    QTR_HIP_TRY(h, icp_grid_enqueue(E.h_views[0], E.h_init[0], st));
    hipLaunchKernelGGL(k_eval, dim3(max_nchunk), dim3(256), 0, st, E.h_views[0]);
  } else {
    QTR_HIP_TRY(h, hipMemcpyAsync(E.d_views, E.h_views, view_block, hipMemcpyHostToDevice, st));
    QTR_HIP_TRY(h, icp_grid_enqueue_group(E.d_views, E.d_init, B, std::max(max_nt, 1), max_ncell, st));
    hipLaunchKernelGGL(k_eval_group, dim3(max_nchunk, B), dim3(256), 0, st, x);
  }
  QTR_HIP_TRY(h, hipGetLastError());
  QTR_HIP_TRY(h, hipMemcpyAsync(E.h_rec, E.d_rec, (size_t)B * sizeof(QtrEvalRecord), hipMemcpyDeviceToHost, st));
  QTR_HIP_TRY(h, hipStreamSynchronize(st));
  for (int b = 0; b < B; ++b)
    if (P[b].ns > 0) eval_result_from(&out[b], E.h_rec[b]);
  E.last_ns = P[0].ns;
  return QTR_OK;
}

int qtr_evaluate(qtr_handle* h, int slot, const float* src4, int n_s, const float* tgt4, int n_t, const float* tgt_normals4,
                 const double T[16], const qtr_eval_params* prm, qtr_eval_result* res, int mem) {
  Slot* sp = get_slot(h, slot);
  if (!sp || !res) return QTR_ERR_BAD_ARG;
  memset(res, 0, sizeof(*res));
  Slot& s = *sp;
  int rc = check_eval_params(h, prm);
  if (rc == QTR_OK) rc = check_eval_T(h, T);
  if (rc != QTR_OK) return res->status = rc;
  const int n[2] = {n_s, n_t};
  const float4* pts[2] = {(const float4*)src4, (const float4*)tgt4};
  const float4* nrm[2] = {nullptr, (const float4*)tgt_normals4};
  rc = clouds_stage(h, s, "bad evaluation arguments", "evaluation: cloud", nullptr, mem, n, pts, nrm, true);
  if (rc != QTR_OK) return res->status = rc;
  const EvalPair P{pts[0], pts[1], nrm[1], n_s, n_t, T};
  rc = eval_device(h, s, &P, 1, prm->max_correspondence_distance, false, res);
  return res->status = rc;
}

int qtr_evaluate_pair(qtr_handle* h, int slot, const double T[16], const qtr_eval_params* prm, qtr_eval_result* res) {
  Slot* sp = peek_slot(h, slot);  // (an evaluation leaves the registration's clouds and the ICP arena as they are)
  if (!sp || !res) return QTR_ERR_BAD_ARG;
  memset(res, 0, sizeof(*res));
  Slot& s = *sp;
  int rc = check_eval_params(h, prm);
  if (rc != QTR_OK) return res->status = rc;
  if (!s.reg_ready) {
    snprintf(h->err, sizeof(h->err), "qtr_evaluate_pair: the slot's last call was not a registration");
    return res->status = QTR_ERR_BAD_ARG;
  }
  if (T && (rc = check_eval_T(h, T)) != QTR_OK) return res->status = rc;
  QTR_HIP_TRY(h, hipSetDevice(h->device));
  const EvalPair P{s.fb.cloud[0].vox, s.fb.cloud[1].vox, s.fb.cloud[1].normals, s.last_ns, s.last_nt, T ? T : s.reg_T};
  rc = eval_device(h, s, &P, 1, prm->max_correspondence_distance, false, res);
  return res->status = rc;
}

// the pairs of a keyframe evaluation against the handle, before anything is enqueued
static int eval_kf_pairs(qtr_handle* h, const qtr_eval_kf_pair* pairs, int B, EvalPair* P) {
  for (int b = 0; b < B; ++b) {
    const qtr_keyframe *a = pairs[b].source, *t = pairs[b].target;
    if (!a || !t) {
      snprintf(h->err, sizeof(h->err), "evaluation: keyframe of pair %d is NULL", b);
      return QTR_ERR_BAD_ARG;
    }
    if (a->owner != h || t->owner != h) {
      snprintf(h->err, sizeof(h->err), "keyframe belongs to another handle");
      return QTR_ERR_BAD_ARG;
    }
    QTR_TRY(check_eval_T(h, pairs[b].T));
    if (a->info.n_voxels > h->lim.max_voxels || t->info.n_voxels > h->lim.max_voxels) {
      snprintf(h->err, sizeof(h->err), "evaluation: keyframe of pair %d exceeds max_voxels=%d", b, h->lim.max_voxels);
      return QTR_ERR_CAPACITY;
    }
    const KfLayout lt = kf_layout(t->info.n_voxels);
    P[b].src = (const float4*)((const char*)a->dev + KF_HDR_BYTES);
    P[b].tgt = (const float4*)((const char*)t->dev + lt.vox);
    P[b].nrm = (const float4*)((const char*)t->dev + lt.normals);
    P[b].ns = a->info.n_voxels;
    P[b].nt = t->info.n_voxels;
    P[b].T = pairs[b].T;
  }
  return QTR_OK;
}

int qtr_evaluate_keyframes(qtr_handle* h, int slot, const qtr_keyframe* source, const qtr_keyframe* target, const double T[16],
                           const qtr_eval_params* prm, qtr_eval_result* res) {
  Slot* sp = peek_slot(h, slot);  // (the keyframes are read where they lie: the slot's clouds stay what they were)
  if (!sp || !res) return QTR_ERR_BAD_ARG;
  memset(res, 0, sizeof(*res));
  int rc = check_eval_params(h, prm);
  if (rc == QTR_OK) rc = check_eval_T(h, T);
  if (rc != QTR_OK) return res->status = rc;
  qtr_eval_kf_pair pr;
  pr.source = source;
  pr.target = target;
  memcpy(pr.T, T, sizeof(pr.T));
  EvalPair P;
  if ((rc = eval_kf_pairs(h, &pr, 1, &P)) != QTR_OK) return res->status = rc;
  QTR_HIP_TRY(h, hipSetDevice(h->device));
  rc = eval_device(h, *sp, &P, 1, prm->max_correspondence_distance, false, res);
  return res->status = rc;
}

int qtr_evaluate_keyframes_batch(qtr_handle* h, int slot, const qtr_eval_kf_pair* pairs, int B, const qtr_eval_params* prm,
                                 qtr_eval_result* results) {
  Slot* sp = peek_slot(h, slot);
  if (!sp) return QTR_ERR_BAD_ARG;
  if (B < 1 || B > QTR_EVAL_MAX_PAIRS || !pairs || !results) {
    snprintf(h->err, sizeof(h->err), "evaluation batch: %d pairs (1 .. %d), pairs and results not NULL", B, QTR_EVAL_MAX_PAIRS);
    return QTR_ERR_BAD_ARG;
  }
  memset(results, 0, sizeof(*results) * (size_t)B);
  int rc = check_eval_params(h, prm);
  EvalPair P[QTR_EVAL_MAX_PAIRS];
  if (rc == QTR_OK) rc = eval_kf_pairs(h, pairs, B, P);
  if (rc == QTR_OK) {
    QTR_HIP_TRY(h, hipSetDevice(h->device));
    rc = eval_device(h, *sp, P, B, prm->max_correspondence_distance, true, results);
  }
  if (rc != QTR_OK)
    for (int b = 0; b < B; ++b) results[b].status = rc;
  return rc;
}

// ---- pose-graph optimisation (pgo.hip) ---------------------------------------------------------------------------------
void qtr_default_pgo_params(qtr_pgo_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->max_iterations = 100;
  p->pcg_max_iterations = 500;
  p->rel_tol = 1e-6;
  p->step_tol = 1e-9;
  p->tau = 1e-5;
  p->pcg_tol = 1e-8;
  p->line_process_weight = 0.0;
  p->edge_prune_threshold = 0.25;
}

static bool pgo_finite(double x) { return (x - x) == 0.0; }

// everything qtr_pgo_optimize refuses, before a device is touched
static int check_pgo_args(qtr_handle* h, int N, const double* poses, const unsigned char* fixed, int E, const int* src,
                          const int* dst, const double* Z, const double* info, const qtr_pgo_params* prm,
                          const double* poses_out, const qtr_pgo_result* res) {
  auto bad = [&](const char* fmt, int a, int b) {
    snprintf(h->err, sizeof(h->err), fmt, a, b);
    return QTR_ERR_BAD_ARG;
  };
  if (!res || !prm || !poses || !poses_out) return bad("qtr_pgo_optimize: poses, poses_out, params and result must not be NULL", 0, 0);
  if (N < 1 || E < 0) return bad("qtr_pgo_optimize: %d nodes (>= 1), %d edges (>= 0)", N, E);
  if (E > 0 && (!src || !dst || !Z || !info)) return bad("qtr_pgo_optimize: src, dst, Z and info must not be NULL with %d edges", E, 0);
  const double tol[4] = {prm->rel_tol, prm->step_tol, prm->tau, prm->pcg_tol};
  for (int k = 0; k < 4; ++k)
    if (!pgo_finite(tol[k]) || !(tol[k] > 0.0))
      return bad("qtr_pgo_optimize: tolerance %d (rel_tol, step_tol, tau, pcg_tol) is not finite and positive", k, 0);
  if (prm->max_iterations < 0 || prm->max_iterations > QTR_PGO_MAX_ITERATIONS || prm->pcg_max_iterations < 1)
    return bad("qtr_pgo_optimize: max_iterations %d (0 .. 65536), pcg_max_iterations %d (>= 1)", prm->max_iterations,
               prm->pcg_max_iterations);
  if (!pgo_finite(prm->line_process_weight) || !pgo_finite(prm->edge_prune_threshold))
    return bad("qtr_pgo_optimize: line_process_weight and edge_prune_threshold must be finite", 0, 0);
  if (N > QTR_PGO_MAX_NODES || E > QTR_PGO_MAX_EDGES) {
    snprintf(h->err, sizeof(h->err), "qtr_pgo_optimize: %d nodes / %d edges exceed QTR_PGO_MAX_NODES / QTR_PGO_MAX_EDGES", N, E);
    return QTR_ERR_CAPACITY;
  }
  if (fixed) {
    bool any = false;
    for (int i = 0; i < N; ++i) any = any || fixed[i] != 0;
    if (!any) return bad("qtr_pgo_optimize: no fixed node among %d", N, 0);
  }
  for (int i = 0; i < N; ++i)
    for (int k = 0; k < 12; ++k)
      if (!pgo_finite(poses[(size_t)16 * i + k])) return bad("qtr_pgo_optimize: pose %d has a non-finite entry in rows 0 - 2", i, 0);
  for (int e = 0; e < E; ++e) {
    if (src[e] < 0 || src[e] >= N || dst[e] < 0 || dst[e] >= N) return bad("qtr_pgo_optimize: edge %d names a node outside 0 .. %d", e, N - 1);
    if (src[e] == dst[e]) return bad("qtr_pgo_optimize: edge %d joins node %d to itself", e, src[e]);
    for (int k = 0; k < 12; ++k)
      if (!pgo_finite(Z[(size_t)16 * e + k])) return bad("qtr_pgo_optimize: Z of edge %d has a non-finite entry in rows 0 - 2", e, 0);
    for (int a = 0; a < 6; ++a)
      for (int b = a; b < 6; ++b)
        if (!pgo_finite(info[(size_t)36 * e + 6 * a + b]))
          return bad("qtr_pgo_optimize: info of edge %d has a non-finite entry in its upper triangle", e, 0);
  }
  return QTR_OK;
}

int qtr_pgo_optimize(qtr_handle* h, int slot, int N, const double* poses, const unsigned char* fixed, int E, const int* src,
                     const int* dst, const double* Z, const double* info, const unsigned char* uncertain,
                     const qtr_pgo_params* prm, double* poses_out, double* weight_out, qtr_pgo_result* res) {
  Slot* sp = peek_slot(h, slot);  // (registration, ICP and evaluation state of the slot stay what they were)
  if (!sp) return QTR_ERR_BAD_ARG;
  int rc = check_pgo_args(h, N, poses, fixed, E, src, dst, Z, info, prm, poses_out, res);
  if (rc != QTR_OK) {
    if (res) {
      memset(res, 0, sizeof(*res));
      res->status = rc;
    }
    return rc;
  }
  memset(res, 0, sizeof(*res));
  Slot& s = *sp;
  std::vector<unsigned char> fx((size_t)N, 0), un((size_t)std::max(E, 1), 0);
  int n_free = 0;
  for (int i = 0; i < N; ++i) {
    fx[i] = fixed ? (fixed[i] ? 1 : 0) : (i == 0 ? 1 : 0);
    n_free += fx[i] ? 0 : 1;
  }
  for (int e = 0; e < E; ++e) un[e] = (uncertain && uncertain[e]) ? 1 : 0;
  PgoBufs& P = s.pgo;
  if (E == 0 || n_free == 0) {  // nothing to optimise
    if (poses_out != poses) memmove(poses_out, poses, sizeof(double) * 16 * (size_t)N);
    if (weight_out)
      for (int e = 0; e < E; ++e) weight_out[e] = 1.0;
    res->valid = 1;
    res->stop_reason = QTR_PGO_STOP_NOTHING;
    P.last_rows = 0;
    return res->status = QTR_OK;
  }
  QtrPgoCfg cfg;
  cfg.rel_tol = prm->rel_tol;
  cfg.step_tol = prm->step_tol;
  cfg.tau = prm->tau;
  cfg.pcg_tol = prm->pcg_tol;
  cfg.mu = prm->line_process_weight;
  cfg.max_iterations = prm->max_iterations;
  cfg.pcg_max_iterations = prm->pcg_max_iterations;
  std::vector<int> off((size_t)N + 1), inc((size_t)2 * E);
  qtr_pgo_incidence(N, E, src, dst, off.data(), inc.data());
  rc = [&]() -> int {
    QTR_HIP_TRY(h, hipSetDevice(h->device));
    QTR_HIP_TRY(h, pgo_reserve(P, pgo_arena_bytes(N, E, cfg.max_iterations)));
    PgoView v;
    memset((void*)&v, 0, sizeof(v));
    pgo_carve(P, N, E, cfg.max_iterations, v);
    v.cfg = cfg;
    P.last_trace = v.trace;
    P.last_rows = 0;
    const hipStream_t st = s.stream;
    qtr_pgo_init(&P.pin[0]);
    const size_t n = (size_t)N, e = (size_t)E;
    QTR_HIP_TRY(h, hipMemcpyAsync((void*)v.fixed, fx.data(), n, hipMemcpyHostToDevice, st));
    QTR_HIP_TRY(h, hipMemcpyAsync((void*)v.unc, un.data(), e, hipMemcpyHostToDevice, st));
    QTR_HIP_TRY(h, hipMemcpyAsync((void*)v.src, src, e * 4, hipMemcpyHostToDevice, st));
    QTR_HIP_TRY(h, hipMemcpyAsync((void*)v.dst, dst, e * 4, hipMemcpyHostToDevice, st));
    QTR_HIP_TRY(h, hipMemcpyAsync((void*)v.off, off.data(), (n + 1) * 4, hipMemcpyHostToDevice, st));
    QTR_HIP_TRY(h, hipMemcpyAsync((void*)v.inc, inc.data(), 2 * e * 4, hipMemcpyHostToDevice, st));
    QTR_HIP_TRY(h, hipMemcpyAsync((void*)v.Z, Z, e * 128, hipMemcpyHostToDevice, st));
    QTR_HIP_TRY(h, hipMemcpyAsync((void*)v.info, info, e * 288, hipMemcpyHostToDevice, st));
    for (int k = 0; k < 2; ++k) QTR_HIP_TRY(h, hipMemcpyAsync(v.X[k], poses, n * 128, hipMemcpyHostToDevice, st));
    QTR_HIP_TRY(h, hipMemcpyAsync(v.st, &P.pin[0], sizeof(QtrPgoState), hipMemcpyHostToDevice, st));
    QTR_HIP_TRY(h, hipMemsetAsync(v.ticket, 0, 64, st));
    const QtrPgoState& now = P.pin[1];
    // one (linearize, step) pair and one host wait per LM iteration; the last pair's step returns at once
    for (int it = 0; it <= cfg.max_iterations; ++it) {
      hipLaunchKernelGGL(k_pgo_linearize, dim3(qtr_div_up(E, 256)), dim3(256), 0, st, v);
      hipLaunchKernelGGL(k_pgo_step, dim3(1), dim3(QTR_PGO_THREADS), 0, st, v);
      QTR_HIP_TRY(h, hipGetLastError());
      QTR_HIP_TRY(h, hipMemcpyAsync(&P.pin[1], v.st, sizeof(QtrPgoState), hipMemcpyDeviceToHost, st));
      QTR_HIP_TRY(h, hipStreamSynchronize(st));
      if (now.stop) break;
    }
    if (!now.stop) {
      snprintf(h->err, sizeof(h->err), "qtr_pgo_optimize: the device did not stop after %d iterations", cfg.max_iterations);
      return QTR_ERR_HIP;
    }
    QTR_HIP_TRY(h, hipMemcpyAsync(poses_out, v.X[now.cur], n * 128, hipMemcpyDeviceToHost, st));
    std::vector<double> w(e);
    QTR_HIP_TRY(h, hipMemcpyAsync(w.data(), v.Ew[now.cur], e * 8, hipMemcpyDeviceToHost, st));
    QTR_HIP_TRY(h, hipStreamSynchronize(st));
    P.last_rows = 1 + now.trials;
    res->iterations = now.trials;
    res->accepted = now.accepted;
    res->pcg_iterations_total = now.pcg_total;
    res->stop_reason = now.reason;
    res->objective_initial = now.F0;
    res->objective_final = now.F;
    res->lambda_final = now.lambda;
    res->valid = pgo_finite(now.F) ? 1 : 0;
    for (int k = 0; k < E; ++k) {
      if (un[k] && w[k] < prm->edge_prune_threshold) res->n_pruned += 1;
      if (weight_out) weight_out[k] = w[k];
    }
    return QTR_OK;
  }();
  return res->status = rc;
}

long long qtr_debug_fetch(qtr_handle* h, int slot, int what, void* dst, size_t bytes) {
  Slot* sp = peek_slot(h, slot);
  if (!sp) return -1;
  Slot& s = *sp;
  if (hipSetDevice(h->device) != hipSuccess) return -1;
  const void* src = nullptr;
  size_t have = 0;
  const int L = s.last_L, W = (L + 63) / 64;
  CloudBufs& c0 = s.fb.cloud[0];
  switch (what) {
    case QTR_DBG_GRAPH_BITMAP: src = s.sb.bm; have = (size_t)L * W * 8; break;
    case QTR_DBG_CORE: src = s.sb.core; have = (size_t)L * 4; break;
    case QTR_DBG_PERM: src = s.sb.perm; have = (size_t)L * 4; break;
    case QTR_DBG_NBR_OFFSETS:
      // the CSR view is only built for inspection
      if (exclusive_scan_i32(c0.nbr_cnt, c0.nbr_off, s.last_n, s.stream) != hipSuccess) return -1;
      src = c0.nbr_off;
      have = (size_t)(s.last_n + 1) * 4;
      break;
    case QTR_DBG_NBR_INDEX:
    case QTR_DBG_NBR_DIST2: {
      int tot = 0;
      if (exclusive_scan_i32(c0.nbr_cnt, c0.nbr_off, s.last_n, s.stream) != hipSuccess) return -1;
      if (hipStreamSynchronize(s.stream) != hipSuccess) return -1;
      if (hipMemcpy(&tot, c0.nbr_off + s.last_n, 4, hipMemcpyDeviceToHost) != hipSuccess) return -1;
      src = (what == QTR_DBG_NBR_INDEX) ? (const void*)c0.nbr_idx : (const void*)c0.nbr_d2;
      have = (size_t)tot * 4;
      break;
    }
    case QTR_DBG_SPFH: src = c0.spfh; have = (size_t)s.last_n * 132; break;
    case QTR_DBG_NN_LARGE_OF_SMALL: src = s.fb.nn_of_small; have = (size_t)(s.last_ns < s.last_nt ? s.last_ns : s.last_nt) * 4; break;
    case QTR_DBG_NN_SMALL_OF_LARGE: src = s.fb.nn_of_large; have = (size_t)(s.last_ns < s.last_nt ? s.last_nt : s.last_ns) * 4; break;
    case QTR_DBG_VOX_SRC: src = s.fb.cloud[0].vox; have = (size_t)s.last_ns * 16; break;
    case QTR_DBG_VOX_TGT: src = s.fb.cloud[1].vox; have = (size_t)s.last_nt * 16; break;
    case QTR_DBG_CORR: src = s.fb.corr; have = (size_t)s.last_L * 8; break;
    case QTR_DBG_MATCH_STATS: src = s.fb.mcounts; have = 16 * 4; break;
    case QTR_DBG_SOLVER_STATE: src = s.sb.st; have = sizeof(SolverState); break;
    case QTR_DBG_ICP_CORR: src = s.icp.v.corr; have = s.icp.v.corr ? (size_t)s.icp_ns * 4 : 0; break;
    case QTR_DBG_ICP_TRACE: src = s.icp.v.trace; have = s.icp.v.trace ? (size_t)s.icp_iters * 18 * 8 : 0; break;
    case QTR_DBG_ICP_TIMES: src = s.icp_ms; have = sizeof(s.icp_ms); break;
    case QTR_DBG_EVAL_CORR: src = s.eval.last_corr; have = s.eval.last_corr ? (size_t)s.eval.last_ns * 4 : 0; break;
    case QTR_DBG_PGO_TRACE: src = s.pgo.last_trace; have = s.pgo.last_trace ? (size_t)s.pgo.last_rows * QTR_PGO_TRACE * 8 : 0; break;
    default: return -1;
  }
  const size_t n = have < bytes ? have : bytes;
  if (dst && n > 0) {
    if (hipStreamSynchronize(s.stream) != hipSuccess) return -1;
    if (what == QTR_DBG_GRAPH_BITMAP && s.last_Wb > W) {  // rows start on 32-byte boundaries on the device: pack them
      const size_t rows = n / ((size_t)W * 8);
      if (rows > 0 && hipMemcpy2D(dst, (size_t)W * 8, src, (size_t)s.last_Wb * 8, (size_t)W * 8, rows, hipMemcpyDeviceToHost) !=
                          hipSuccess)
        return -1;
    } else if (what == QTR_DBG_ICP_TIMES) {
      memcpy(dst, src, n);
    } else if (hipMemcpy(dst, src, n, hipMemcpyDeviceToHost) != hipSuccess) {
      return -1;
    }
  }
  return (long long)have;
}

__global__ void k_debug_math(int fn, const float* a, const float* b, float* out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float r = 0.f, s, c;
  switch (fn) {
    case 0: r = qm_atan2f(a[i], b[i]); break;
    case 1: r = qm_acosf(a[i]); break;
    case 2: qm_sincosf(a[i], &s, &c); r = s; break;
    case 3: qm_sincosf(a[i], &s, &c); r = c; break;
    case 4: r = (float)spfh_angle_bin(a[i], b[i]); break;        // the first block's bin as k2_spfh stores it
    case 5: r = spfh_swap_roles(a[i], b[i]) ? 1.f : 0.f; break;  // the SPFH kernel's shortcut (tests compare it with the
                                                                 // plain arithmetic)
    case 6: r = (float)spfh_bin_of_angle(a[i], b[i]); break;     // the bin shortcut alone: -1 where it is not sure
    default: break;
  }
  out[i] = r;
}

int qtr_debug_math(qtr_handle* h, int fn, const float* a, const float* b, float* out, int n) {
  if (!h || !a || !out || n <= 0) return QTR_ERR_BAD_ARG;
  QTR_HIP_TRY(h, hipSetDevice(h->device));
  float *da = nullptr, *db = nullptr, *dout = nullptr;
  QTR_HIP_TRY(h, hipMalloc((void**)&da, (size_t)n * 4));
  QTR_HIP_TRY(h, hipMalloc((void**)&db, (size_t)n * 4));
  QTR_HIP_TRY(h, hipMalloc((void**)&dout, (size_t)n * 4));
  QTR_HIP_TRY(h, hipMemcpy(da, a, (size_t)n * 4, hipMemcpyHostToDevice));
  QTR_HIP_TRY(h, hipMemcpy(db, b ? b : a, (size_t)n * 4, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_debug_math, dim3((n + 255) / 256), dim3(256), 0, 0, fn, da, db, dout, n);
  QTR_HIP_TRY(h, hipGetLastError());
  QTR_HIP_TRY(h, hipMemcpy(out, dout, (size_t)n * 4, hipMemcpyDeviceToHost));
  (void)hipFree(da);
  (void)hipFree(db);
  (void)hipFree(dout);
  return QTR_OK;
}

}  // extern "C"
