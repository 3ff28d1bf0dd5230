// SPF kernel in the reference's extraction order (kExact).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spf_device.h"
#include "spf_launch.h"

namespace orh {

// ---------------------------------------------------------------------------
// exact Dijkstra in the reference's extraction order
// ---------------------------------------------------------------------------
// LinkState::runSpf (LinkState.cpp:808-882) step for step: a binary heap on
// (metric, name), `>=` relaxations that union the first-hop sets, reset on a
// strictly better metric, no transit through overloaded nodes. With a
// zero-metric link the closed form of the other kernels does not hold (a node
// at the same metric contributes its first hops only if it is extracted
// first), and path metrics may exceed 32 bits; this kernel covers both. Lane 0
// of one wave per source runs the search (its state is one source's heap),
// the other lanes initialise and copy out.
size_t exact_state_bytes(uint32_t n, uint32_t words) {
  // metric u64 | pos u32 | heap u32 | nh u32 * words, 16-byte aligned
  return ((static_cast<size_t>(n) * (16 + 4 * words)) + 15) & ~static_cast<size_t>(15);
}

template <bool kLds>
__global__ __launch_bounds__(64) void spf_exact_kernel(ExactArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  const uint32_t N = a.n_nodes, W = a.words, row = blockIdx.x, lane = threadIdx.x;
  uint8_t* base = kLds ? reinterpret_cast<uint8_t*>(lds) : a.scratch + row * a.scratch_stride;
  uint64_t* metric = reinterpret_cast<uint64_t*>(base);
  uint32_t* pos = reinterpret_cast<uint32_t*>(metric + N);  // heap index + 1, kRec when extracted
  uint32_t* heap = pos + N;
  uint32_t* nh = heap + N;
  constexpr uint64_t kInf64 = ~0ull;
  constexpr uint32_t kRec = 0xFFFFFFFFu;
  for (uint32_t v = lane; v < N; v += 64) {
    metric[v] = kInf64;
    pos[v] = 0u;
  }
  for (uint32_t i = lane; i < N * W; i += 64) nh[i] = 0u;
  __syncthreads();
  const uint32_t src = a.srcs[row];
  const uint32_t* ign = nullptr;
  uint32_t n_ign = 0;
  if (a.ignore_ptr) {
    ign = a.ignore_links + a.ignore_ptr[row];
    n_ign = a.ignore_ptr[row + 1] - a.ignore_ptr[row];
  }
  uint32_t* rank_out = a.out_rank ? a.out_rank + static_cast<size_t>(row) * N : nullptr;
  if (lane == 0) {
    auto less = [&](uint32_t x, uint32_t y) {
      const uint64_t mx = metric[x], my = metric[y];
      return mx < my || (mx == my && a.name_rank[x] < a.name_rank[y]);
    };
    auto sift_up = [&](uint32_t i) {
      const uint32_t x = heap[i];
      while (i > 0) {
        const uint32_t p = (i - 1) >> 1, y = heap[p];
        if (!less(x, y)) break;
        heap[i] = y;
        pos[y] = i + 1;
        i = p;
      }
      heap[i] = x;
      pos[x] = i + 1;
    };
    auto sift_down = [&](uint32_t i, uint32_t n) {
      const uint32_t x = heap[i];
      for (;;) {
        uint32_t c = 2 * i + 1;
        if (c >= n) break;
        if (c + 1 < n && less(heap[c + 1], heap[c])) ++c;
        const uint32_t y = heap[c];
        if (!less(y, x)) break;
        heap[i] = y;
        pos[y] = i + 1;
        i = c;
      }
      heap[i] = x;
      pos[x] = i + 1;
    };
    uint32_t n_heap = 0, order = 0;
    metric[src] = 0;
    heap[n_heap++] = src;
    pos[src] = 1;
    const uint32_t K = a.ell_k;
    while (n_heap) {
      const uint32_t v = heap[0];
      if (--n_heap) {
        heap[0] = heap[n_heap];
        sift_down(0, n_heap);
      }
      pos[v] = kRec;  // recorded: final (LinkState.cpp:824)
      if (rank_out) rank_out[v] = order;
      ++order;
      const uint2 r0 = a.recs[static_cast<size_t>(v) * K];
      if (v != src && (r0.x & ORH_REC_ROW_OVL)) continue;  // no transit (:831-838)
      const uint64_t dv = metric[v];
      auto relax = [&](uint32_t q) {
        const uint2 r = a.recs[q];
        if (r.x & (ORH_REC_SKIP | ORH_REC_CONT)) return;
        if (n_ign && ignored(ign, n_ign, a.link[q])) return;
        const uint32_t u = r.x & ORH_REC_COL_MASK;
        if (pos[u] == kRec) return;
        const uint64_t nd = dv + (a.use_link_metric ? static_cast<uint64_t>(r.y) : 1ull);
        if (pos[u] == 0u) {  // first seen: queued at nd (:853-856)
          metric[u] = nd;
          heap[n_heap] = u;
          sift_up(n_heap++);
        } else if (metric[u] > nd) {  // strictly better: reset and re-heap (:862-866)
          metric[u] = nd;
          for (uint32_t k = 0; k < W; ++k) nh[static_cast<size_t>(u) * W + k] = 0u;
          sift_up(pos[u] - 1);
        }
        if (metric[u] != nd) return;
        if (v == src) {  // a direct neighbour's own bit (:869-872)
          const uint32_t b = a.rank_out[q];
          nh[static_cast<size_t>(u) * W + (b >> 5)] |= 1u << (b & 31u);
        } else {
          for (uint32_t k = 0; k < W; ++k)
            nh[static_cast<size_t>(u) * W + k] |= nh[static_cast<size_t>(v) * W + k];
        }
      };
      for (uint32_t j = 0; j < K; ++j) relax(v * K + j);
      const uint2 last = a.recs[static_cast<size_t>(v) * K + K - 1];
      if (last.x & ORH_REC_CONT) {
        const uint32_t start = last.x & ORH_REC_COL_MASK;
        for (uint32_t q = 0; q < last.y; ++q) relax(start + q);
      }
    }
  }
  __syncthreads();
  for (uint32_t v = lane; v < N; v += 64) {
    const uint64_t m = metric[v];
    const bool reached = pos[v] == kRec;
    if (a.out_dist64) a.out_dist64[static_cast<size_t>(row) * N + v] = reached ? m : kInf64;
    if (a.out_dist32) a.out_dist32[static_cast<size_t>(row) * N + v] = reached ? static_cast<uint32_t>(m) : kInf;
    if (rank_out && !reached) rank_out[v] = kInf;
  }
  for (uint32_t i = lane; i < N * W; i += 64) {
    const uint32_t v = i / W;
    a.out_nh[static_cast<size_t>(row) * N * W + i] = (pos[v] == kRec && v != src) ? nh[i] : 0u;
  }
}

hipError_t launch_exact(const ExactArgs& a, size_t lds_limit, hipStream_t s) {
  if (a.n_rows == 0) return hipSuccess;
  const size_t bytes = exact_state_bytes(a.n_nodes, a.words);
  if (bytes <= lds_limit) return launch(spf_exact_kernel<true>, a, a.n_rows, 64, bytes, s);
  if (!a.scratch) return hipErrorInvalidValue;
  hipLaunchKernelGGL(spf_exact_kernel<false>, dim3(a.n_rows), dim3(64), 0, s, a);
  return hipGetLastError();
}

}  // namespace orh
