// place_batch.hip — the grouped place query (include/quatro_place_batch.h): Q queries against one index in one chain.
//   describe  keyframe items -> query slots   k_place_describe_group (blockIdx.y = item; k_place_describe's LDS image)
//   gather    device descriptors -> slots     k_place_gather_group (blockIdx.x = item)
//   norms     every slot                      k_place_colnorm, as it is (blockIdx.x = slot)
//   score     queries x union range -> keys   k_place_score_group: a tile of QT queries in LDS, one wave per entry and
//                                             round, the entry filled into LDS once and scored against the whole tile
//   select    keys -> the k best per query    k_place_select_group (blockIdx.x = query; k_place_select on the query's row)
// The arithmetic is include/qtr_place_math.h's, the plan (ranges, tile, table layout) include/qtr_place_batch_math.h's.
// A query slot is an entry of the index's layout: `stride` floats, image then column norms.  Entry items are not copied:
// their query pointer is the entry itself, with the norms the add stored.
#include "../../include/quatro_place_batch.h"
#include "../../include/qtr_place_batch_math.h"

struct PbQuery {  // one per query, in the call's order
  const float* q;  // stride floats: a slot of the arena or an entry of an index
  int lo, hi;      // the clamped range (lo = hi = 0: empty)
};
struct PbKf {  // one per keyframe item
  const float4* pts;
  int n, slot;
};
struct PbGather {  // one per device-descriptor item
  const float* src;  // R * S floats, 4-byte aligned
  int slot, pad;
};

// the slot's batch arena and what qtr_place_batch_fetch needs of the last call
struct PlaceBatch {
  void* dev = nullptr;
  size_t dev_bytes = 0;
  char* pin = nullptr;  // pinned host: the head (tables and host descriptors) on its way up, the records on their way back
  size_t pin_bytes = 0;
  int Q = -1, U = 0, ulo = 0;  // the last call (Q < 0: none)
  const u64* keys = nullptr;
  const int* shifts = nullptr;
  std::vector<int> lo, hi;
};

static void place_batch_free(Slot& s) {
  if (!s.pbatch) return;
  if (s.pbatch->dev) (void)hipFree(s.pbatch->dev);
  if (s.pbatch->pin) (void)hipHostFree(s.pbatch->pin);
  delete s.pbatch;
  s.pbatch = nullptr;
}

// slots: the arena's query slots, the items' images zeroed before the launch
__global__ __launch_bounds__(256) void k_place_describe_group(const PbKf* __restrict__ tab, int R, int S, float max_range,
                                                              float height_offset, float* __restrict__ slots, int stride) {
  __shared__ u32 s_img[QTR_PLACE_MAX_RINGS * QTR_PLACE_MAX_SECTORS];
  const PbKf it = tab[blockIdx.y];
  if ((int)blockIdx.x * 256 >= it.n) return;  // (uniform: this workgroup has no point of the item)
  u32* __restrict__ img = (u32*)(slots + (size_t)it.slot * stride);
  const int cells = R * S;
  for (int i = threadIdx.x; i < cells; i += 256) s_img[i] = 0u;
  __syncthreads();
  for (int i = blockIdx.x * 256 + threadIdx.x; i < it.n; i += gridDim.x * 256) {
    const float4 p = it.pts[i];
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

__global__ __launch_bounds__(256) void k_place_gather_group(const PbGather* __restrict__ tab, int cells, float* __restrict__ slots,
                                                            int stride) {
  const PbGather it = tab[blockIdx.x];
  float* __restrict__ d = slots + (size_t)it.slot * stride;
  for (int i = threadIdx.x; i < cells; i += 256) d[i] = it.src[i];
}

// Grid = (entry tiles over the union range [ulo, ulo + U), query tiles of QT).  LDS (dynamic): the tile's QT queries, then one
// entry per wave: (QT + 4) * stride * 4 bytes.  Every wave of a workgroup runs the same number of rounds (the barriers are
// uniform); a wave without an entry idles.  Slot (q, e) of the table gets the single path's key or, outside q's range, ~0.
__global__ __launch_bounds__(256) void k_place_score_group(const float* __restrict__ entries, const PbQuery* __restrict__ qtab, int Q,
                                                           int QT, int stride, int R, int S, int ulo, int U,
                                                           u64* __restrict__ keys, int* __restrict__ shifts) {
  extern __shared__ uint4 s_pb4[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, s4 = stride >> 2;
  const int q0 = blockIdx.y * QT;
  const int nq = Q - q0 < QT ? Q - q0 : QT;
  for (int t = 0; t < nq; ++t) {
    const uint4* __restrict__ g = (const uint4*)qtab[q0 + t].q;
    for (int i = threadIdx.x; i < s4; i += 256) s_pb4[(size_t)t * s4 + i] = g[i];
  }
  uint4* c4 = s_pb4 + (size_t)(QT + wave) * s4;
  const float* c = (const float*)c4;
  const int s = lane < S ? lane : 0;  // (lanes beyond S compute shift 0 again and never win)
  for (int base = blockIdx.x * 4; base < U; base += gridDim.x * 4) {
    const int e = base + wave;
    __syncthreads();  // the previous round's reads are done (first round: nothing)
    if (e < U) {
      const uint4* __restrict__ g = (const uint4*)(entries + (size_t)(ulo + e) * stride);
      for (int i = lane; i < s4; i += 64) c4[i] = g[i];
    }
    __syncthreads();  // the queries (first round) and the entries are in LDS
    if (e < U) {
      const int id = ulo + e;
      for (int t = 0; t < nq; ++t) {
        const PbQuery qi = qtab[q0 + t];  // (uniform: scalar loads)
        const bool in = id >= qi.lo && id < qi.hi;  // (uniform per wave)
        u64 key = ~0ULL;
        if (in) {
          const float* q = (const float*)(s_pb4 + (size_t)t * s4);
          const float d = qtr_place_shift_distance(q, q + R * S, c, c + R * S, R, S, s);
          key = lane < S ? qtr_place_key(d, (u32)lane) : ~0ULL;
#pragma unroll
          for (int off = 32; off >= 1; off >>= 1) {
            const u64 o = __shfl_xor(key, off, 64);
            key = o < key ? o : key;
          }
        }
        if (lane == 0) {
          const size_t at = qtr_place_batch_slot(q0 + t, id, ulo, U);
          keys[at] = in ? ((key & 0xffffffff00000000ULL) | (u32)id) : ~0ULL;
          shifts[at] = in ? (int)(u32)key : 0;
        }
      }
    }
  }
}

// k_place_select on row blockIdx.x of the table (U keys, all different or ~0): the k smallest, ascending, as match records
// to out[q * k ..], and how many there were to n_out[q].
__global__ __launch_bounds__(1024) void k_place_select_group(const u64* __restrict__ keys, const int* __restrict__ shifts, int U,
                                                             int ulo, int k, int S, qtr_place_match* __restrict__ out,
                                                             int* __restrict__ n_out) {
  __shared__ u64 s_min[16];
  __shared__ u64 s_win;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t row = (size_t)blockIdx.x * (size_t)U;
  keys += row;
  shifts += row;
  out += (size_t)blockIdx.x * k;
  u64 mine = ~0ULL;
  for (int i = tid; i < U; i += 1024) {
    const u64 v = keys[i];
    mine = v < mine ? v : mine;
  }
  int round = 0;
  for (; round < k; ++round) {
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
      const int shift = shifts[id - ulo];
      qtr_place_match r;
      r.id = id;
      r.shift = shift;
      r.distance = __uint_as_float((u32)(w >> 32));
      r.yaw = qtr_place_yaw(shift, S);
      out[round] = r;
      u64 next = ~0ULL;
      for (int i = tid; i < U; i += 1024) {
        const u64 v = keys[i];
        if (v > w && v < next) next = v;
      }
      mine = next;
    }
  }
  if (tid == 0) n_out[blockIdx.x] = round;
}


int qtr_place_query_batch(qtr_handle* h, int slot, const qtr_place_index* ix, const qtr_place_query_item* items, int Q, int k,
                          qtr_place_match* out, int* n_out) {
  if (n_out && Q > 0) memset(n_out, 0, (size_t)Q * sizeof(int));
  Slot* sp = peek_slot(h, slot);  // (nothing of the slot's clouds or of its single-query scratch is written)
  if (!sp) return QTR_ERR_BAD_ARG;
  if (Q == 0) return QTR_OK;
  if (!ix || !items || !out || !n_out) {
    snprintf(h->err, sizeof(h->err), "place query batch: %s is NULL", !ix ? "index" : !items ? "items" : !out ? "out" : "n_out");
    return QTR_ERR_BAD_ARG;
  }
  if (Q < 0 || Q > QTR_PLACE_BATCH_MAX) {
    snprintf(h->err, sizeof(h->err), "place query batch: Q=%d (0 .. %d)", Q, QTR_PLACE_BATCH_MAX);
    return QTR_ERR_BAD_ARG;
  }
  if (ix->owner != h) {
    snprintf(h->err, sizeof(h->err), "place index belongs to another handle");
    return QTR_ERR_BAD_ARG;
  }
  if (k < 1 || k > QTR_PLACE_MAX_K) {
    snprintf(h->err, sizeof(h->err), "place query batch: k = %d (1 .. %d)", k, QTR_PLACE_MAX_K);
    return QTR_ERR_BAD_ARG;
  }
  const qtr_place_params& p = ix->info.params;
  const int R = p.num_rings, S = p.num_sectors, stride = ix->stride, cells = R * S;
  std::vector<int> lo((size_t)Q), hi((size_t)Q);
  int nh = 0, nd = 0, nk = 0, max_n = 0;
  for (int q = 0; q < Q; ++q) {
    const qtr_place_query_item& it = items[q];
    if (it.kf) {
      if (it.kf->owner != h) {
        snprintf(h->err, sizeof(h->err), "place query batch: item %d: keyframe belongs to another handle", q);
        return QTR_ERR_BAD_ARG;
      }
      ++nk;
      max_n = std::max(max_n, it.kf->info.n_voxels);
    } else if (it.desc) {
      if (it.mem != QTR_MEM_HOST && it.mem != QTR_MEM_DEVICE) {
        snprintf(h->err, sizeof(h->err), "place query batch: item %d: mem %d", q, it.mem);
        return QTR_ERR_BAD_ARG;
      }
      ++(it.mem == QTR_MEM_HOST ? nh : nd);
    } else {
      const qtr_place_index* from = it.from ? it.from : ix;
      if (from->owner != h) {
        snprintf(h->err, sizeof(h->err), "place query batch: item %d: its index belongs to another handle", q);
        return QTR_ERR_BAD_ARG;
      }
      if (from->info.params.num_rings != R || from->info.params.num_sectors != S || from->stride != stride) {
        snprintf(h->err, sizeof(h->err), "place query batch: item %d: its index is %d x %d, the searched one %d x %d", q,
                 from->info.params.num_rings, from->info.params.num_sectors, R, S);
        return QTR_ERR_BAD_ARG;
      }
      if (it.entry < 0 || it.entry >= from->info.size) {
        snprintf(h->err, sizeof(h->err), "place query batch: item %d: %s %d (its index holds %d)", q,
                 it.entry < 0 && !it.from ? "no source; entry" : "entry", it.entry, from->info.size);
        return QTR_ERR_BAD_ARG;
      }
    }
    qtr_place_batch_clamp(it.id_lo, it.id_hi, ix->info.size, &lo[q], &hi[q]);
  }
  int ulo = 0, uhi = 0;
  qtr_place_batch_union(lo.data(), hi.data(), Q, &ulo, &uhi);
  const int U = uhi - ulo;
  if (!qtr_place_batch_pairs_ok(Q, U)) {
    snprintf(h->err, sizeof(h->err), "place query batch: %d queries x %d entries of the union range [%d, %d) exceed %d pairs", Q, U,
             ulo, uhi, QTR_PLACE_BATCH_MAX_PAIRS);
    return QTR_ERR_CAPACITY;
  }
  if (!sp->pbatch) {
    PlaceBatch* nb = new (std::nothrow) PlaceBatch();
    if (!nb) return QTR_ERR_CAPACITY;
    sp->pbatch = nb;  // (from here on the handle frees whatever of it exists)
  }
  PlaceBatch& pb = *sp->pbatch;
  if (U == 0) {  // every range is empty: nothing to enqueue, and a batch whose sections are all empty
    pb.lo.swap(lo);
    pb.hi.swap(hi);
    pb.keys = nullptr;
    pb.shifts = nullptr;
    pb.U = pb.ulo = 0;
    pb.Q = Q;
    return QTR_OK;
  }
  QTR_HIP_TRY(h, hipSetDevice(h->device));
  const hipStream_t st = sp->stream;
  pb.Q = -1;  // (the last call's table is gone once this one writes the arena)

  // the arena's layout for this call: the head (one upload: the three tables, then the slots of the host descriptors), the
  // other slots directly behind them, the score table, the records and counts (one copy back)
  const int ns = nh + nd + nk;
  const size_t slot_bytes = (size_t)stride * 4;
  const size_t o_qtab = 0, o_kftab = o_qtab + qtr_up256((size_t)Q * sizeof(PbQuery)), o_gtab = o_kftab + qtr_up256((size_t)nk * sizeof(PbKf)),
               o_slots = o_gtab + qtr_up256((size_t)nd * sizeof(PbGather)), head_bytes = o_slots + (size_t)nh * slot_bytes,
               o_keys = qtr_up256(o_slots + (size_t)ns * slot_bytes), o_shifts = o_keys + qtr_up256((size_t)Q * U * 8),
               o_back = o_shifts + qtr_up256((size_t)Q * U * 4), out_bytes = (size_t)Q * k * sizeof(qtr_place_match),
               back_bytes = out_bytes + (size_t)Q * 4, need = o_back + qtr_up256(back_bytes);
  const size_t o_pin_back = qtr_up256(head_bytes), pin_need = o_pin_back + back_bytes;
  if (need > pb.dev_bytes) {
    QTR_HIP_TRY(h, hipStreamSynchronize(st));
    if (pb.dev) (void)hipFree(pb.dev);
    pb.dev = nullptr;
    pb.dev_bytes = 0;
    if (hipMalloc(&pb.dev, need) != hipSuccess) {
      (void)hipGetLastError();
      pb.dev = nullptr;
      snprintf(h->err, sizeof(h->err), "place query batch: no device memory for %zu bytes", need);
      return QTR_ERR_HIP;
    }
    pb.dev_bytes = need;
  }
  if (pin_need > pb.pin_bytes) {
    QTR_HIP_TRY(h, hipStreamSynchronize(st));
    if (pb.pin) (void)hipHostFree(pb.pin);
    pb.pin = nullptr;
    pb.pin_bytes = 0;
    QTR_HIP_TRY(h, hipHostMalloc((void**)&pb.pin, pin_need));
    pb.pin_bytes = pin_need;
  }
  char* const dev = (char*)pb.dev;
  float* const slots = (float*)(dev + o_slots);
  PbQuery* const hq = (PbQuery*)(pb.pin + o_qtab);
  PbKf* const hk = (PbKf*)(pb.pin + o_kftab);
  PbGather* const hg = (PbGather*)(pb.pin + o_gtab);
  int ih = 0, id = nh, ik = nh + nd;  // the next slot of each kind: host descriptors, device descriptors, keyframes
  for (int q = 0; q < Q; ++q) {
    const qtr_place_query_item& it = items[q];
    PbQuery v;
    v.lo = lo[q];
    v.hi = hi[q];
    if (it.kf) {
      PbKf& e = hk[ik - nh - nd];
      e.pts = (const float4*)((const char*)it.kf->dev + KF_HDR_BYTES);
      e.n = it.kf->info.n_voxels;
      e.slot = ik;
      v.q = slots + (size_t)ik++ * stride;
    } else if (it.desc && it.mem == QTR_MEM_HOST) {
      memcpy(pb.pin + o_slots + (size_t)ih * slot_bytes, it.desc, (size_t)cells * 4);
      v.q = slots + (size_t)ih++ * stride;
    } else if (it.desc) {
      PbGather& e = hg[id - nh];
      e.src = it.desc;
      e.slot = id;
      e.pad = 0;
      v.q = slots + (size_t)id++ * stride;
    } else {
      const qtr_place_index* from = it.from ? it.from : ix;
      v.q = from->dev + (size_t)it.entry * stride;
    }
    hq[q] = v;
  }
  u64* const keys = (u64*)(dev + o_keys);
  int* const shifts = (int*)(dev + o_shifts);
  qtr_place_match* const d_out = (qtr_place_match*)(dev + o_back);
  int* const d_nout = (int*)(dev + o_back + out_bytes);

  QTR_HIP_TRY(h, hipMemcpyAsync(dev, pb.pin, head_bytes, hipMemcpyHostToDevice, st));
  if (nk > 0) {
    QTR_HIP_TRY(h, hipMemsetAsync(slots + (size_t)(nh + nd) * stride, 0, (size_t)nk * slot_bytes, st));
    if (max_n > 0)
      hipLaunchKernelGGL(k_place_describe_group, dim3(place_describe_grid(max_n), nk), dim3(256), 0, st, (const PbKf*)(dev + o_kftab),
                         R, S, p.max_range, p.height_offset, slots, stride);
  }
  if (nd > 0)
    hipLaunchKernelGGL(k_place_gather_group, dim3(nd), dim3(256), 0, st, (const PbGather*)(dev + o_gtab), cells, slots, stride);
  if (ns > 0) hipLaunchKernelGGL(k_place_colnorm, dim3(ns), dim3(64), 0, st, slots, stride, R, S);
  const int QT = qtr_place_batch_qt(stride);
  const int gx = std::min(qtr_div_up(U, 4), QTR_PLACE_BATCH_GRID_X);
  hipLaunchKernelGGL(k_place_score_group, dim3(gx, qtr_div_up(Q, QT)), dim3(256), (size_t)(QT + 4) * slot_bytes, st, ix->dev,
                     (const PbQuery*)(dev + o_qtab), Q, QT, stride, R, S, ulo, U, keys, shifts);
  hipLaunchKernelGGL(k_place_select_group, dim3(Q), dim3(1024), 0, st, keys, shifts, U, ulo, k, S, d_out, d_nout);
  QTR_HIP_TRY(h, hipGetLastError());
  QTR_HIP_TRY(h, hipMemcpyAsync(pb.pin + o_pin_back, d_out, back_bytes, hipMemcpyDeviceToHost, st));
  QTR_HIP_TRY(h, hipStreamSynchronize(st));
  const qtr_place_match* const h_out = (const qtr_place_match*)(pb.pin + o_pin_back);
  const int* const h_nout = (const int*)(pb.pin + o_pin_back + out_bytes);
  for (int q = 0; q < Q; ++q) {
    const int n = h_nout[q];
    if (n > 0) memcpy(out + (size_t)q * k, h_out + (size_t)q * k, (size_t)n * sizeof(qtr_place_match));
    n_out[q] = n;
  }
  pb.lo.swap(lo);
  pb.hi.swap(hi);
  pb.keys = keys;
  pb.shifts = shifts;
  pb.U = U;
  pb.ulo = ulo;
  pb.Q = Q;
  return QTR_OK;
}

long long qtr_place_batch_fetch(qtr_handle* h, int slot, int query, int what, void* dst, size_t bytes) {
  Slot* sp = peek_slot(h, slot);
  if (!sp || !sp->pbatch || sp->pbatch->Q < 0) return -1;
  const PlaceBatch& pb = *sp->pbatch;
  if (query < 0 || query >= pb.Q || (what != QTR_PLACE_BATCH_DIST && what != QTR_PLACE_BATCH_SHIFT)) return -1;
  const int n = pb.hi[query] - pb.lo[query];
  const size_t have = (size_t)n * 4, m = have < bytes ? have : bytes;
  if (dst && m > 0) {
    if (hipSetDevice(h->device) != hipSuccess) return -1;
    const size_t at = qtr_place_batch_slot(query, pb.lo[query], pb.ulo, pb.U);
    if (what == QTR_PLACE_BATCH_SHIFT) {
      if (hipMemcpy(dst, pb.shifts + at, m, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    } else {  // the distance is the high word of the key
      std::vector<u64> row((size_t)n);
      if (hipMemcpy(row.data(), pb.keys + at, (size_t)n * 8, hipMemcpyDeviceToHost) != hipSuccess) return -1;
      std::vector<u32> d((size_t)n);
      for (int i = 0; i < n; ++i) d[i] = (u32)(row[i] >> 32);
      memcpy(dst, d.data(), m);
    }
  }
  return (long long)have;
}
