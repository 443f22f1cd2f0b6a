// place.hip — the Scan Context place index: one R x S maximum-height image per keyframe in device memory, and the
// exhaustive search "the k entries most similar to this query, under all column shifts".  The arithmetic is
// include/qtr_place_math.h's, called from the kernels as it is written there.
//   describe  points -> image             k_place_describe (LDS image per workgroup, integer atomicMax on the float bits)
//                                         + k_place_colnorm (the S squared column norms behind the image)
//   score     query x entries -> keys     k_place_score: one wave per entry, lane = shift
//   select    keys -> the k best          k_place_select: one workgroup, k rounds of a block-wide minimum
// An entry is `stride` floats: R * S cells, S squared column norms, padded to a multiple of 4 floats so that every entry
// starts on a 16-byte boundary (20 x 60: 1260 floats = 5040 bytes, no padding).
#include "common.h"
#include "../../include/qtr_place_math.h"

static inline int place_stride(int R, int S) { return ((R + 1) * S + 3) & ~3; }

// per-slot scratch of a query (capi.hip grows it on demand): the query's entry, one key and one shift per scored entry,
// the matches
struct PlaceScratch {
  float* q = nullptr;            // stride floats
  u64* keys = nullptr;           // cap entries
  int* shifts = nullptr;         // cap entries
  qtr_place_match* out = nullptr;  // QTR_PLACE_MAX_K records
  qtr_place_match* pin = nullptr;  // pinned host: the records' way back
  void* arena = nullptr;
  int stride = 0, cap = 0;
};

// img: R * S words, zeroed before the launch.  Heights are positive floats: their bit patterns order like unsigned ints.
__global__ __launch_bounds__(256) void k_place_describe(const float4* __restrict__ pts, int n, int R, int S, float max_range,
                                                        float height_offset, u32* __restrict__ img) {
  __shared__ u32 s_img[QTR_PLACE_MAX_RINGS * QTR_PLACE_MAX_SECTORS];
  const int cells = R * S;
  for (int i = threadIdx.x; i < cells; i += 256) s_img[i] = 0u;
  __syncthreads();
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const float4 p = pts[i];
    float zh = 0.0f;
    const int cell = qtr_place_cell(p.x, p.y, p.z, R, S, max_range, height_offset, &zh);
    if (cell >= 0 && cell < cells) atomicMax(&s_img[cell], __float_as_uint(zh));
  }
  __syncthreads();
  for (int i = threadIdx.x; i < cells; i += 256) {
    const u32 v = s_img[i];
    if (v) atomicMax(&img[i], v);
  }
}

// the S column norms of `count` entries: blockIdx.x = entry, thread = column
__global__ __launch_bounds__(64) void k_place_colnorm(float* __restrict__ entries, int stride, int R, int S) {
  float* e = entries + (size_t)blockIdx.x * stride;
  const int j = threadIdx.x;
  if (j < S) e[R * S + j] = qtr_place_colnorm2(e, R, S, j);
}

// One wave per entry and round, lane = shift.  LDS (dynamic): the query's entry, then one entry per wave of the workgroup.
// Every wave of a workgroup runs the same number of rounds (the barriers are uniform); a wave without an entry idles.
__global__ __launch_bounds__(256) void k_place_score(const float* __restrict__ entries, const float* __restrict__ query, int stride,
                                                     int R, int S, int id_lo, int n, u64* __restrict__ keys,
                                                     int* __restrict__ shifts) {
  extern __shared__ uint4 s_place4[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, s4 = stride >> 2;
  for (int i = threadIdx.x; i < s4; i += 256) s_place4[i] = ((const uint4*)query)[i];
  const float* q = (const float*)s_place4;
  uint4* c4 = s_place4 + (size_t)(1 + wave) * s4;
  const float* c = (const float*)c4;
  const int s = lane < S ? lane : 0;  // (lanes beyond S compute shift 0 again and never win)
  for (int base = blockIdx.x * 4; base < n; base += gridDim.x * 4) {
    const int e = base + wave;
    __syncthreads();  // the previous round's reads are done (first round: nothing)
    if (e < n) {
      const uint4* __restrict__ g = (const uint4*)(entries + (size_t)(id_lo + e) * stride);
      for (int i = lane; i < s4; i += 64) c4[i] = g[i];
    }
    __syncthreads();  // the query (first round) and the entries are in LDS
    if (e < n) {
      const float d = qtr_place_shift_distance(q, q + R * S, c, c + R * S, R, S, s);
      u64 key = lane < S ? qtr_place_key(d, (u32)lane) : ~0ULL;
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
        const u64 o = __shfl_xor(key, off, 64);
        key = o < key ? o : key;
      }
      if (lane == 0) {
        keys[e] = (key & 0xffffffff00000000ULL) | (u32)(id_lo + e);
        shifts[e] = (int)(u32)key;
      }
    }
  }
}

// The k smallest of n keys (all different: the low word is the id), ascending, as match records.  One workgroup of 1024:
// thread t owns keys t, t + 1024, ...; a round is the block-wide minimum of the threads' current minima, after which only
// the winner looks for its next one.
__global__ __launch_bounds__(1024) void k_place_select(const u64* __restrict__ keys, const int* __restrict__ shifts, int n, int id_lo,
                                                       int k, int S, qtr_place_match* __restrict__ out) {
  __shared__ u64 s_min[16];
  __shared__ u64 s_win;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  u64 mine = ~0ULL;
  for (int i = tid; i < n; i += 1024) {
    const u64 v = keys[i];
    mine = v < mine ? v : mine;
  }
  for (int round = 0; round < k; ++round) {
    u64 m = mine;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const u64 o = __shfl_xor(m, off, 64);
      m = o < m ? o : m;
    }
    if (lane == 0) s_min[wave] = m;
    __syncthreads();
    if (tid == 0) {
      u64 w = s_min[0];
      for (int i = 1; i < 16; ++i) w = s_min[i] < w ? s_min[i] : w;
      s_win = w;
    }
    __syncthreads();
    const u64 w = s_win;
    if (w == ~0ULL) break;  // (uniform: fewer than k candidates)
    if (mine == w) {        // one thread: the keys are all different
      const int id = (int)(u32)w;
      const int shift = shifts[id - id_lo];
      qtr_place_match r;
      r.id = id;
      r.shift = shift;
      r.distance = __uint_as_float((u32)(w >> 32));
      r.yaw = qtr_place_yaw(shift, S);
      out[round] = r;
      u64 next = ~0ULL;
      for (int i = tid; i < n; i += 1024) {
        const u64 v = keys[i];
        if (v > w && v < next) next = v;
      }
      mine = next;
    }
  }
}

static inline int place_describe_grid(int n) {
  const int g = (n + 1023) / 1024;  // four points per thread before the stride starts
  return g < 1 ? 1 : (g > 1024 ? 1024 : g);
}

// points (device) -> the entry at `entry` (stride floats: image and column norms; the padding is left alone)
hipError_t place_describe_enqueue(const float4* pts, int n, const qtr_place_params& p, float* entry, hipStream_t st) {
  const int R = p.num_rings, S = p.num_sectors;
  hipError_t e = hipMemsetAsync(entry, 0, (size_t)R * S * 4, st);
  if (e != hipSuccess) return e;
  if (n > 0)
    hipLaunchKernelGGL(k_place_describe, dim3(place_describe_grid(n)), dim3(256), 0, st, pts, n, R, S, p.max_range, p.height_offset,
                       (u32*)entry);
  hipLaunchKernelGGL(k_place_colnorm, dim3(1), dim3(64), 0, st, entry, place_stride(R, S), R, S);
  return hipGetLastError();
}
hipError_t place_colnorm_enqueue(float* entry, const qtr_place_params& p, hipStream_t st) {
  hipLaunchKernelGGL(k_place_colnorm, dim3(1), dim3(64), 0, st, entry, place_stride(p.num_rings, p.num_sectors), p.num_rings,
                     p.num_sectors);
  return hipGetLastError();
}
// entries [id_lo, id_lo + n) against the scratch's query, the k best to sc.out; n >= 1, 1 <= k <= QTR_PLACE_MAX_K
hipError_t place_search_enqueue(const float* entries, const qtr_place_params& p, int id_lo, int n, int k, PlaceScratch& sc,
                                hipStream_t st) {
  const int R = p.num_rings, S = p.num_sectors, stride = place_stride(R, S);
  int grid = (n + 3) / 4;
  grid = grid > 2048 ? 2048 : grid;
  hipLaunchKernelGGL(k_place_score, dim3(grid), dim3(256), (size_t)5 * stride * 4, st, entries, sc.q, stride, R, S, id_lo, n, sc.keys,
                     sc.shifts);
  hipLaunchKernelGGL(k_place_select, dim3(1), dim3(1024), 0, st, sc.keys, sc.shifts, n, id_lo, k, S, sc.out);
  return hipGetLastError();
}
