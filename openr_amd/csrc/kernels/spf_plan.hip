// SPF plan choice and dispatch to the kernel families, the launch-side
// knobs, and the graph-mirror scatter kernels.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstdlib>

#include "spf_device.h"
#include "spf_launch.h"

namespace orh {

LaunchKnobs launch_knobs() {
  static const LaunchKnobs once = [] {  // the fields read once per process
    LaunchKnobs o{};
    const char* e = getenv("ORH_LDS16_BLOCK");
    const int b = e ? atoi(e) : 1024;
    o.lds16_block = (b >= 64 && b <= 1024 && b % 64 == 0) ? static_cast<uint32_t>(b) : 1024u;
    e = getenv("ORH_HOP_NARROW");
    o.hop_narrow = e && atoi(e) == 1;
    e = getenv("ORH_HOP_NODES");
    o.hop_nodes = (e && atoi(e) == 16) ? 16u : 8u;
    e = getenv("ORH_HOP_SPLIT");
    o.hop_split = e ? static_cast<uint32_t>(std::max(1, atoi(e))) : 1u;
    e = getenv("ORH_HOP_WG_PER_CU");
    o.hop_wg_per_cu = e ? static_cast<uint32_t>(atoi(e)) : 0u;
    return o;
  }();
  LaunchKnobs k = once;
  const char* e = getenv("ORH_MS_BLOCK");
  const int b = e ? atoi(e) : 0;
  k.ms_block_set = e != nullptr;
  k.ms_block = (b >= 64 && b <= 1024 && b % 64 == 0) ? static_cast<uint32_t>(b) : 0u;
  e = getenv("ORH_MS_LATENCY");
  k.ms_latency = e ? atoi(e) : 1;
  e = getenv("ORH_MS_WIDE");
  k.ms_wide = e && atoi(e) == 1;
  e = getenv("ORH_WMS_SOURCES");
  k.wms_four = e && atoi(e) == 4;
  e = getenv("ORH_WMS_WIDE_SOURCES");
  k.wms_wide_two = e && atoi(e) == 2;
  e = getenv("ORH_HOP_XCD");
  k.hop_xcd = e && e[0] == '1';
  e = getenv("ORH_HOP_LEAN");
  k.hop_lean = !(e && e[0] == '0');
  return k;
}

static SpfPlan plan_global(SpfPlan p, uint32_t n_nodes, uint64_t path_bound, size_t lds_limit) {
  const size_t bytes = 3 * static_cast<size_t>((n_nodes + 31) / 32) * 4;
  if (path_bound >= 0xFFFFFFFFull || bytes > lds_limit) {
    p.variant = SpfVariant::kUnsupported;
    return p;
  }
  p.variant = SpfVariant::kGlobal;
  p.lds_bytes = std::max<size_t>(bytes, 16);
  p.block = 256;
  return p;
}

SpfPlan plan_spf(uint32_t n_nodes, bool uniform, uint64_t path_bound, uint32_t ell_k,
                 size_t lds_limit, bool multi_source, SpfMode mode) {
  SpfPlan p{};
  p.ell_k = ell_k;
  if (ell_k != 4 && ell_k != 8) return p;
  if (mode == SpfMode::kGlobal || mode == SpfMode::kGlobalTwoPhase)
    return plan_global(p, n_nodes, path_bound, lds_limit);
  const size_t nb = (n_nodes + 31) / 32;
  if (mode == SpfMode::kAuto && multi_source && uniform && path_bound < 0xFFFFFFFFull) {
    // a thread owns J <= 32 nodes (registers); the frontier arrays hold
    // N + 1 entries (the last is the always-zero target of dead slots).
    // 8 waves per workgroup (J = 20 on the 10k grid): one sweep alone takes
    // 0.82 ms against 0.73 at 12 waves (J = 16), but sweeps running side by
    // side on 4 streams - the bench step, any batch of what-if topologies -
    // finish 7 % sooner (26.8 vs 28.7 ms per 32 sweeps): two 8-wave
    // workgroups per CU leave wave slots and VGPRs for the other streams'
    // first-hop and finalize kernels (profiles/r03/o_ms_block_ab.txt)
    // (past 16,384 nodes 512 threads would need J > 32: 12 waves)
    uint32_t block = n_nodes <= 4096 ? 256 : n_nodes <= 16384 ? 512 : 768;
    if (const uint32_t b = launch_knobs().ms_block) block = b;
    const uint32_t j = (n_nodes + block - 1) / block;
    const uint32_t pitch = (n_nodes + 1 + 15) & ~15u;
    if (j <= 32) {
      for (uint32_t mb = 4; mb >= 2; mb /= 2) {
        const size_t bytes = 2 * static_cast<size_t>(mb) * pitch;
        // (16-bit byte offsets in the kernel's ELL columns)
        if (bytes <= lds_limit && static_cast<size_t>(mb) * pitch <= 65536) {
          p.variant = SpfVariant::kMsBfs;
          p.mask_bytes = mb;
          p.ms_j = (j + 3) & ~3u;
          p.ms_pitch = pitch;
          p.lds_bytes = bytes;
          p.block = block;
          return p;
        }
      }
    }
  }
  if (uniform && path_bound < 0xFFFFFFFFull) {
    // levels are < N; the level type's all-ones marks "unvisited"
    p.variant = n_nodes < 0xFFu ? SpfVariant::kBfs8
        : n_nodes < 0xFFFFu     ? SpfVariant::kBfs16
                                : SpfVariant::kBfs32;
    const size_t lb = n_nodes < 0xFFu ? 1 : n_nodes < 0xFFFFu ? 2 : 4;
    p.pend_off = align16(static_cast<size_t>(n_nodes) * lb);
    p.lds_bytes = p.pend_off + 2 * nb * 4;
  } else if (path_bound < 0xFFFFull) {
    p.variant = SpfVariant::kDist16;
    p.pend_off = align16(static_cast<size_t>(n_nodes) * 2);
    p.lds_bytes = p.pend_off + align16(nb * 4);
  } else if (path_bound < 0xFFFFFFFFull) {
    p.variant = SpfVariant::kDist32;
    p.pend_off = align16(static_cast<size_t>(n_nodes) * 4);
    p.lds_bytes = p.pend_off + align16(nb * 4);
  } else {
    return p;
  }
  // a thread owns two bitmap words per pass; 256 threads cover N <= 16,384
  // in one pass and leave room for 8 workgroups per CU
  const uint32_t half = static_cast<uint32_t>((nb + 1) / 2);
  p.block = std::min<uint32_t>(kMaxBlock, std::max<uint32_t>(256, (half + 63) / 64 * 64));
  if (p.lds_bytes > lds_limit) return plan_global(p, n_nodes, path_bound, lds_limit);
  return p;
}

// each variant through its family's launch function (spf_launch.h)
static hipError_t launch_k(const SpfPlan& plan, const SpfArgs& a, uint32_t n_rows, hipStream_t s) {
  switch (plan.variant) {
    case SpfVariant::kMsBfs:
      return launch_ms(plan, a, n_rows, s);
    case SpfVariant::kBfs8:
    case SpfVariant::kBfs16:
    case SpfVariant::kBfs32:
      return launch_bfs(plan, a, n_rows, s);
    case SpfVariant::kBfsNh:
      return launch_bfs_nh(plan, a, n_rows, s);
    case SpfVariant::kDist16:
    case SpfVariant::kDist32:
      return launch_dist(plan, a, n_rows, s);
    case SpfVariant::kGlobal:
      return launch_global(plan, a, n_rows, s);
    case SpfVariant::kGlobalNh:
      return launch_global_nh(plan, a, n_rows, s);
    default:
      return hipErrorInvalidValue;
  }
}

hipError_t launch_spf(const SpfPlan& plan, SpfArgs a, uint32_t n_rows, hipStream_t s) {
  if (n_rows == 0) return hipSuccess;
  a.lds_pend_off = static_cast<uint32_t>(plan.pend_off);
  a.n_rows = n_rows;
  a.ms_pitch = plan.ms_pitch;
  a.ms_zero = a.n_nodes;
  return launch_k(plan, a, n_rows, s);
}

// in-place mirror patch: recs[pos[i]] = vals[i] (one launch per delta batch)
__global__ __launch_bounds__(kBlock) void scatter_recs_kernel(uint2* recs, const uint32_t* pos,
                                                             const uint2* vals, uint32_t n) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i < n) recs[pos[i]] = vals[i];
}

__global__ __launch_bounds__(kBlock) void scatter_rows_kernel(uint2* recs, uint32_t* link, uint16_t* rank,
                                                               const uint32_t* pos, const uint2* vals,
                                                               const uint32_t* links,
                                                               const uint16_t* ranks, uint32_t n) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint32_t q = pos[i];
  recs[q] = vals[i];
  link[q] = links[i];
  rank[q] = ranks[i];
}

hipError_t launch_scatter_rows(uint2* recs, uint32_t* link, uint16_t* rank, const uint32_t* pos,
                               const uint2* vals, const uint32_t* links, const uint16_t* ranks,
                               uint32_t n, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(scatter_rows_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, recs,
                     link, rank, pos, vals, links, ranks, n);
  return hipGetLastError();
}

hipError_t launch_scatter_recs(uint2* recs, const uint32_t* pos, const uint2* vals, uint32_t n,
                               hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(scatter_recs_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, recs,
                     pos, vals, n);
  return hipGetLastError();
}

}  // namespace orh
