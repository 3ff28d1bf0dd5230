// SPF kernels, general metrics, distances only: level-synchronous Dijkstra in
// LDS (kDist16 / kDist32) and the HBM frontier kernel (kGlobal).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spf_device.h"
#include "spf_launch.h"

namespace orh {

// ---------------------------------------------------------------------------
// phase 1b: level-synchronous Dijkstra on a u16 / u32 distance per node
// ---------------------------------------------------------------------------
template <class T>
struct DistWord;

template <>
struct DistWord<uint32_t> {
  static constexpr uint32_t kInfT = 0xFFFFFFFFu;
  __device__ static uint32_t get(const uint32_t* d, uint32_t u) { return d[u]; }
  // lower d[u] to nd (> D); returns the previous value if it was lowered, else nd
  __device__ static bool lower(uint32_t* d, uint32_t u, uint32_t du, uint32_t nd, bool& first) {
    if (nd >= du) return false;
    atomicMin(&d[u], nd);
    first = du == kInfT;
    return true;
  }
};

template <>
struct DistWord<uint16_t> {  // two nodes per u32 word; updated by compare-and-swap
  static constexpr uint32_t kInfT = 0xFFFFu;
  __device__ static uint32_t get(const uint32_t* d, uint32_t u) {
    return (d[u >> 1] >> ((u & 1u) * 16u)) & 0xFFFFu;
  }
  __device__ static bool lower(uint32_t* d, uint32_t u, uint32_t du, uint32_t nd, bool& first) {
    if (nd >= du) return false;
    const uint32_t sh = (u & 1u) * 16u;
    uint32_t old = d[u >> 1];
    for (;;) {
      const uint32_t cur = (old >> sh) & 0xFFFFu;
      if (nd >= cur) return false;  // lowered further by another lane
      const uint32_t nw = (old & ~(0xFFFFu << sh)) | (nd << sh);
      const uint32_t prev = atomicCAS(&d[u >> 1], old, nw);
      if (prev == old) {
        first = cur == 0xFFFFu;
        return true;
      }
      old = prev;
    }
  }
};

template <class T, int K>
struct Dij {
  using DW = DistWord<T>;
  const SpfArgs& a;
  const Src& s;
  uint32_t* dist;  // LDS, T per node
  uint32_t* pend;

  __device__ void edge(const uint2& r, uint32_t du, uint32_t D, uint32_t& lowered) const {
    const uint32_t u = r.x & ORH_REC_COL_MASK;
    const uint32_t nd = D + (a.use_link_metric ? r.y : 1u);
    bool first = false;
    if (DW::lower(dist, u, du, nd, first)) {
      lowered = min(lowered, nd);
      if (first) atomicOr(&pend[u >> 5], 1u << (u & 31u));
    }
  }

  // relax v's out-links at distance D; returns the smallest distance it lowered
  __device__ uint32_t expand(uint32_t v, const uint2 (&rec)[K], uint32_t D) const {
    uint32_t lowered = kInf;
    if (v != s.node && (rec[0].x & ORH_REC_ROW_OVL)) return lowered;
    uint32_t du[K];
    bool lv[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
      lv[j] = live(a, s, rec[j], v * K + j);
      du[j] = lv[j] ? DW::get(dist, rec[j].x & ORH_REC_COL_MASK) : 0u;
    }
#pragma unroll
    for (int j = 0; j < K; ++j)
      if (lv[j]) edge(rec[j], du[j], D, lowered);
    const uint2 last = rec[K - 1];
    if (last.x & ORH_REC_CONT) {
      const uint32_t start = last.x & ORH_REC_COL_MASK;
      for (uint32_t base = 0; base < last.y; base += kOvfBatch) {
        const uint32_t cnt = min(last.y - base, static_cast<uint32_t>(kOvfBatch));
        uint2 ov[kOvfBatch];
#pragma unroll
        for (int j = 0; j < kOvfBatch; ++j)
          if (j < static_cast<int>(cnt)) ov[j] = a.recs[start + base + j];
        uint32_t od[kOvfBatch];
        bool ol[kOvfBatch];
#pragma unroll
        for (int j = 0; j < kOvfBatch; ++j) {
          ol[j] = j < static_cast<int>(cnt) && live(a, s, ov[j], start + base + j);
          od[j] = ol[j] ? DW::get(dist, ov[j].x & ORH_REC_COL_MASK) : 0u;
        }
#pragma unroll
        for (int j = 0; j < kOvfBatch; ++j)
          if (ol[j]) edge(ov[j], od[j], D, lowered);
      }
    }
    return lowered;
  }
};

template <class T, int K>
__global__ __launch_bounds__(kMaxBlock) void spf_dist_kernel(SpfArgs a) {
  using DW = DistWord<T>;
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  __shared__ uint32_t s_min[3];
  const uint32_t N = a.n_nodes;
  const uint32_t NB = (N + 31) >> 5;
  const uint32_t tid = threadIdx.x, nthr = blockDim.x;
  // a.row_list (nullable): workgroup b searches row row_list[b] while b <
  // *row_count, else exits (the rows launch_spf_wms_sliced's batches flagged)
  if (a.row_list && blockIdx.x >= *a.row_count) return;
  const uint32_t row = a.row_list ? a.row_list[blockIdx.x] : blockIdx.x;
  uint32_t* dist = lds;
  uint32_t* pend = lds + a.lds_pend_off / 4;
  const Src s(a, row);
  const Dij<T, K> d{a, s, dist, pend};

  const uint32_t dwords = a.lds_pend_off / 4;
  for (uint32_t i = tid; i < dwords; i += nthr) dist[i] = 0xFFFFFFFFu;
  for (uint32_t i = tid; i < NB; i += nthr) pend[i] = 0u;
  if (tid < 3) s_min[tid] = kInf;
  __syncthreads();
  if (tid == 0) {
    bool first;
    DW::lower(dist, s.node, DW::kInfT, 0u, first);
    pend[s.node >> 5] = 1u << (s.node & 31u);
  }
  __syncthreads();

  constexpr int kBatch = 16 / K;
  constexpr int kScan = 8;  // pending distances read together
  uint32_t D = 0;
  for (uint32_t level = 0;; ++level) {
    const uint32_t slot = level % 3u;  // rotation as in spf_bfs_kernel
    uint32_t local_min = kInf;
    for (uint32_t w = tid; w < NB; w += 2 * nthr) {
      const uint32_t w2 = w + nthr;
      uint64_t bits = pend[w] | (static_cast<uint64_t>(w2 < NB ? pend[w2] : 0u) << 32);
      // split the pending nodes into those at D (expand now) and the rest
      // (candidates for the next D)
      uint64_t todo = 0;
      while (bits) {
        uint32_t bs[kScan], dv[kScan];
        int cnt = 0;
#pragma unroll
        for (int i = 0; i < kScan; ++i) {
          if (bits) {
            bs[i] = static_cast<uint32_t>(__builtin_ctzll(bits));
            bits &= bits - 1;
            const uint32_t v = bs[i] < 32 ? w * 32 + bs[i] : w2 * 32 + (bs[i] - 32);
            dv[i] = DW::get(dist, v);
            cnt = i + 1;
          }
        }
#pragma unroll
        for (int i = 0; i < kScan; ++i) {
          if (i < cnt) {
            if (dv[i] == D) todo |= 1ull << bs[i];
            else local_min = min(local_min, dv[i]);
          }
        }
      }
      if (!todo) continue;
      if (static_cast<uint32_t>(todo)) atomicAnd(&pend[w], ~static_cast<uint32_t>(todo));
      if (todo >> 32) atomicAnd(&pend[w2], ~static_cast<uint32_t>(todo >> 32));
      while (todo) {
        uint32_t vs[kBatch];
        uint2 r[kBatch][K];
        int cnt = 0;
#pragma unroll
        for (int i = 0; i < kBatch; ++i) {
          if (todo) {
            const uint32_t bit = static_cast<uint32_t>(__builtin_ctzll(todo));
            todo &= todo - 1;
            vs[i] = bit < 32 ? w * 32 + bit : w2 * 32 + (bit - 32);
            load_recs<K>(a, vs[i], r[i]);
            cnt = i + 1;
          }
        }
#pragma unroll
        for (int i = 0; i < kBatch; ++i)
          if (i < cnt) local_min = min(local_min, d.expand(vs[i], r[i], D));
      }
    }
    const uint32_t wm = wave_min(local_min);
    if ((tid & 63u) == 0 && wm != kInf) atomicMin(&s_min[slot], wm);
    __syncthreads();
    const uint32_t next = s_min[slot];
    if (next == kInf || level >= N) break;
    if (tid == 0) s_min[(level + 2u) % 3u] = kInf;  // read before this barrier by every wave
    D = next;
  }

  uint32_t* out = dist_row(a.out_dist, a.scratch, a.n_out, N, row);
  for (uint32_t i = tid; i < N; i += nthr) {
    const uint32_t dv = DW::get(dist, i);
    __builtin_nontemporal_store(dv == DW::kInfT ? kInf : dv, &out[i]);
  }
}

// ---------------------------------------------------------------------------
// phase 1c: frontier relaxation with the distances in HBM (graphs whose
// per-source state does not fit LDS, e.g. the 50k-node WAN of C4)
// ---------------------------------------------------------------------------
// One workgroup per source row. The row itself (u32, in the output or the
// scratch) holds the tentative distances; LDS holds only frontier bitmaps,
// so any N up to ~400k fits. Label-correcting with a near/far split
// (delta-stepping): a node lowered to d < T joins the next near frontier,
// one lowered to d >= T the far set; when the near frontier empties, T
// advances to (smallest far distance) + delta and the far nodes below it
// become the frontier. Exact for positive integer metrics: every lowering is
// re-expanded, so the fixpoint is the shortest-path distance. Relaxation is
// an atomicMin on the row (L2 atomics); the row is L2-resident while its
// source is searched.
template <int K>
__global__ __launch_bounds__(256) void spf_global_kernel(SpfArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  __shared__ uint32_t s_flag[3];
  __shared__ uint32_t s_min;
  const uint32_t N = a.n_nodes;
  const uint32_t NB = (N + 31) >> 5;
  const uint32_t tid = threadIdx.x, nthr = blockDim.x, row = blockIdx.x;
  uint32_t* near0 = lds;
  uint32_t* near1 = lds + NB;
  uint32_t* far = lds + 2 * NB;
  const Src s(a, row);
  uint32_t* dist = dist_row(a.out_dist, a.scratch, a.n_out, N, row);

  for (uint32_t i = tid; i < 3 * NB; i += nthr) lds[i] = 0u;
  for (uint32_t i = tid; i < N; i += nthr) dist[i] = kInf;
  if (tid < 3) s_flag[tid] = 0u;
  __syncthreads();  // also orders the row initialisation before the search
  if (tid == 0) {
    dist[s.node] = 0u;
    near0[s.node >> 5] = 1u << (s.node & 31u);
  }
  __syncthreads();

  const uint32_t delta = a.delta;
  uint32_t T = delta;  // near/far threshold
  uint32_t* cur = near0;
  uint32_t* nxt = near1;
  for (uint32_t it = 0;; ++it) {
    // expand the near frontier
    bool pushed_near = false;
    for (uint32_t w = tid; w < NB; w += nthr) {
      uint32_t bits = cur[w];
      if (!bits) continue;
      cur[w] = 0u;
      while (bits) {
        const uint32_t v = w * 32 + __builtin_ctz(bits);
        bits &= bits - 1;
        uint2 rec[K];
        load_recs<K>(a, v, rec);
        if (v != s.node && (rec[0].x & ORH_REC_ROW_OVL)) continue;  // no transit
        const uint32_t dv = __hip_atomic_load(&dist[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        auto relax = [&](const uint2& r, uint32_t q) {
          if (!live(a, s, r, q)) return;
          const uint32_t u = r.x & ORH_REC_COL_MASK;
          const uint32_t nd = dv + (a.use_link_metric ? r.y : 1u);
          if (nd >= __hip_atomic_load(&dist[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
          const uint32_t old = atomicMin(&dist[u], nd);
          if (nd >= old) return;
          if (nd < T) {
            atomicOr(&nxt[u >> 5], 1u << (u & 31u));
            pushed_near = true;
          } else {
            atomicOr(&far[u >> 5], 1u << (u & 31u));
          }
        };
#pragma unroll
        for (int j = 0; j < K; ++j) relax(rec[j], v * K + j);
        const uint2 last = rec[K - 1];
        if (last.x & ORH_REC_CONT) {
          const uint32_t start = last.x & ORH_REC_COL_MASK;
          for (uint32_t q = 0; q < last.y; ++q) relax(a.recs[start + q], start + q);
        }
      }
    }
    const uint32_t par = it % 3u;
    if (pushed_near) s_flag[par] = 1u;
    if (tid == 0) s_min = kInf;
    __syncthreads();  // relaxations (global atomics) and bitmaps settled
    const bool more_near = s_flag[par] != 0u;
    if (tid == 0) s_flag[(par + 2u) % 3u] = 0u;  // the previous iteration's flag
    uint32_t* t = cur;
    cur = nxt;
    nxt = t;
    if (more_near) continue;
    // near frontier empty: smallest far distance, then promote far nodes below
    // the new threshold
    uint32_t local_min = kInf;
    for (uint32_t w = tid; w < NB; w += nthr) {
      for (uint32_t bits = far[w]; bits; bits &= bits - 1) {
        const uint32_t v = w * 32 + __builtin_ctz(bits);
        local_min = min(local_min, __hip_atomic_load(&dist[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
      }
    }
    const uint32_t wm = wave_min(local_min);
    if ((tid & 63u) == 0 && wm != kInf) atomicMin(&s_min, wm);
    __syncthreads();
    const uint32_t m = s_min;
    if (m == kInf) break;  // far set empty: done (every wave sees the same value)
    T = m + delta;
    for (uint32_t w = tid; w < NB; w += nthr) {
      uint32_t bits = far[w], promote = 0u;
      for (uint32_t q = bits; q; q &= q - 1) {
        const uint32_t b = __builtin_ctz(q);
        if (__hip_atomic_load(&dist[w * 32 + b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < T)
          promote |= 1u << b;
      }
      if (promote) {
        far[w] = bits & ~promote;
        cur[w] |= promote;
      }
    }
    __syncthreads();
  }
}

hipError_t launch_dist(const SpfPlan& plan, const SpfArgs& a, uint32_t n_rows, hipStream_t s) {
  const bool k8 = plan.ell_k == 8;
  if (plan.variant == SpfVariant::kDist16)
    return k8 ? launch(spf_dist_kernel<uint16_t, 8>, a, n_rows, plan.block, plan.lds_bytes, s)
              : launch(spf_dist_kernel<uint16_t, 4>, a, n_rows, plan.block, plan.lds_bytes, s);
  return k8 ? launch(spf_dist_kernel<uint32_t, 8>, a, n_rows, plan.block, plan.lds_bytes, s)
            : launch(spf_dist_kernel<uint32_t, 4>, a, n_rows, plan.block, plan.lds_bytes, s);
}

hipError_t launch_global(const SpfPlan& plan, const SpfArgs& a, uint32_t n_rows, hipStream_t s) {
  return plan.ell_k == 8 ? launch(spf_global_kernel<8>, a, n_rows, plan.block, plan.lds_bytes, s)
                         : launch(spf_global_kernel<4>, a, n_rows, plan.block, plan.lds_bytes, s);
}

}  // namespace orh
