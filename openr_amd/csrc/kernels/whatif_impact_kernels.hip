// What-if impact summaries (orh_whatif_impact): each request's row against the
// base row of its source, reduced on the device to one orh_whatif_impact_rec
// while the row is still in its buffer.
//
//   whatif_impact_kernel     one workgroup per (request, tile of kImpactTile
//                            nodes): classify, reduce in the wave, then the
//                            workgroup, then atomics into the record - only for
//                            a tile in which some node changed, which most
//                            tiles of most rows are not. A tier-0 request's
//                            workgroups exit before they read anything.
//   whatif_impact_fin_kernel one thread per request: the (stretch, ~node) key
//                            the tiles maximised becomes max_stretch /
//                            worst_node (ORH_NO_NODE without a farther node).
//
// The records are zeroed before the first kernel (launch_whatif_impact), so a
// tier-0 request's record is the zero record with worst_node = ORH_NO_NODE.
// The request rows are read once (non-temporal loads); the base rows are
// shared by every request of a source and stay in cache (plain loads).
#include "../../../include/openr_hip.h"
#include "whatif_kernels.h"

namespace orh {

namespace {

constexpr uint32_t kImpactBlock = 256;
constexpr uint32_t kImpactTile = kImpactBlock * 8;  // nodes of a row per workgroup: two uint4 per lane and array

// a record while its tiles accumulate: the key (stretch << 32 | ~node) lies
// over max_stretch / worst_node
struct ImpactAcc {
  uint32_t lost, farther, rehomed, narrowed;
  unsigned long long key, sum_stretch, lost_weight, moved_weight;
};
static_assert(sizeof(ImpactAcc) == sizeof(orh_whatif_impact_rec), "accumulator and record share their bytes");
static_assert(sizeof(orh_whatif_impact_rec) == 48, "orh_whatif_impact_rec is 48 bytes");

// per-lane partials of one tile; cnt packs the four class counts in 16 bits
// each (a tile has kImpactTile < 65,536 nodes)
struct Lane {
  unsigned long long cnt, key, sum, lw, mw;
};
static_assert(kImpactTile < 65536, "class counts of a tile are packed in 16 bits");

__device__ __forceinline__ void classify(const ImpactArgs& a, uint32_t v, uint32_t src, uint32_t bd, uint32_t bn,
                                         uint32_t rd, uint32_t rn, Lane& l) {
  if (bd == ORH_UNREACHABLE || v == src) return;
  bool moved = false;
  if (rd == ORH_UNREACHABLE) {
    l.cnt += 1ull;
    if (a.weight) l.lw += a.weight[v];
    if (a.node_lost) atomicAdd(a.node_lost + v, 1u);
    moved = true;
  } else {
    if (rd != bd) {
      const uint32_t stretch = rd - bd;
      l.cnt += 1ull << 16;
      l.sum += stretch;
      const unsigned long long k = (static_cast<unsigned long long>(stretch) << 32) | (~v);
      l.key = k > l.key ? k : l.key;
      moved = true;
    } else if (rn != bn) {
      l.cnt += 1ull << 32;
      moved = true;
    }
    if (__popc(rn) < __popc(bn)) l.cnt += 1ull << 48;
  }
  if (moved) {
    if (a.weight) l.mw += a.weight[v];
    if (a.node_moved) atomicAdd(a.node_moved + v, 1u);
  }
}

__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long x, int o) {
  const uint32_t lo = static_cast<uint32_t>(__shfl_xor(static_cast<int>(x), o));
  const uint32_t hi = static_cast<uint32_t>(__shfl_xor(static_cast<int>(x >> 32), o));
  return (static_cast<unsigned long long>(hi) << 32) | lo;
}

__global__ __launch_bounds__(kImpactBlock) void whatif_impact_kernel(ImpactArgs a, uint32_t tiles, uint32_t vec) {
  const uint32_t r = blockIdx.x / tiles;
  const uint32_t t = blockIdx.x % tiles;
  // tier 0: the source's row stands, the zeroed record is the answer, and the
  // row (never written under ORH_WHATIF_SHARE_BASE) is not read
  if (a.info && ORH_WHATIF_TIER(a.info[r]) == 0) return;
  const size_t N = a.n_nodes;
  const size_t b = a.base_row[r];
  const uint32_t src = a.srcs[r];
  const uint32_t* bd = a.base_dist + b * N;
  const uint32_t* bn = a.base_nh + b * N;
  const uint32_t* rd = a.dist + r * N;
  const uint32_t* rn = a.nh + r * N;
  const uint32_t lo = t * kImpactTile;
  const uint32_t hi = static_cast<uint32_t>(min(static_cast<size_t>(lo) + kImpactTile, N));
  Lane l{};
  if (vec) {
    typedef uint32_t v4 __attribute__((ext_vector_type(4)));
#pragma unroll 2
    for (uint32_t i = lo / 4 + threadIdx.x; i < hi / 4; i += kImpactBlock) {
      const v4 qd = __builtin_nontemporal_load(reinterpret_cast<const v4*>(rd) + i);
      const v4 qn = __builtin_nontemporal_load(reinterpret_cast<const v4*>(rn) + i);
      const v4 pd = reinterpret_cast<const v4*>(bd)[i];
      const v4 pn = reinterpret_cast<const v4*>(bn)[i];
      // an unchanged quad (nearly all of them) is done here
      if (((qd.x ^ pd.x) | (qd.y ^ pd.y) | (qd.z ^ pd.z) | (qd.w ^ pd.w) | (qn.x ^ pn.x) | (qn.y ^ pn.y) |
           (qn.z ^ pn.z) | (qn.w ^ pn.w)) == 0)
        continue;
      classify(a, 4 * i + 0, src, pd.x, pn.x, qd.x, qn.x, l);
      classify(a, 4 * i + 1, src, pd.y, pn.y, qd.y, qn.y, l);
      classify(a, 4 * i + 2, src, pd.z, pn.z, qd.z, qn.z, l);
      classify(a, 4 * i + 3, src, pd.w, pn.w, qd.w, qn.w, l);
    }
  } else {
    for (uint32_t i = lo + threadIdx.x; i < hi; i += kImpactBlock) {
      const uint32_t qd = rd[i], qn = rn[i], pd = bd[i], pn = bn[i];
      if (qd != pd || qn != pn) classify(a, i, src, pd, pn, qd, qn, l);
    }
  }
  // a node in any class sets a count (narrowed alone included)
  if (!__syncthreads_or(l.cnt != 0)) return;
  for (int o = 32; o > 0; o >>= 1) {
    l.cnt += shfl_xor_u64(l.cnt, o);
    l.sum += shfl_xor_u64(l.sum, o);
    l.lw += shfl_xor_u64(l.lw, o);
    l.mw += shfl_xor_u64(l.mw, o);
    const unsigned long long k = shfl_xor_u64(l.key, o);
    l.key = k > l.key ? k : l.key;
  }
  constexpr uint32_t kWaves = kImpactBlock / 64;
  __shared__ Lane part[kWaves];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = l;
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (uint32_t w = 1; w < kWaves; ++w) {
    l.cnt += part[w].cnt;
    l.sum += part[w].sum;
    l.lw += part[w].lw;
    l.mw += part[w].mw;
    l.key = part[w].key > l.key ? part[w].key : l.key;
  }
  ImpactAcc* out = reinterpret_cast<ImpactAcc*>(a.out) + r;
  const uint32_t lost = l.cnt & 0xFFFFu, farther = (l.cnt >> 16) & 0xFFFFu, rehomed = (l.cnt >> 32) & 0xFFFFu,
                 narrowed = static_cast<uint32_t>(l.cnt >> 48);
  if (lost) atomicAdd(&out->lost, lost);
  if (farther) {
    atomicAdd(&out->farther, farther);
    atomicMax(&out->key, l.key);
    atomicAdd(&out->sum_stretch, l.sum);
  }
  if (rehomed) atomicAdd(&out->rehomed, rehomed);
  if (narrowed) atomicAdd(&out->narrowed, narrowed);
  if (l.lw) atomicAdd(&out->lost_weight, l.lw);
  if (l.mw) atomicAdd(&out->moved_weight, l.mw);
}

__global__ __launch_bounds__(256) void whatif_impact_fin_kernel(orh_whatif_impact_rec* out, uint32_t n_req) {
  const uint32_t r = blockIdx.x * 256 + threadIdx.x;
  if (r >= n_req) return;
  const ImpactAcc acc = reinterpret_cast<const ImpactAcc*>(out)[r];
  out[r].max_stretch = acc.farther ? static_cast<uint32_t>(acc.key >> 32) : 0u;
  out[r].worst_node = acc.farther ? ~static_cast<uint32_t>(acc.key) : ORH_NO_NODE;
}

}  // namespace

hipError_t launch_whatif_impact(const ImpactArgs& a, hipStream_t s) {
  if (a.n_req == 0) return hipSuccess;
  const uint32_t tiles = (a.n_nodes + kImpactTile - 1) / kImpactTile;
  const uint64_t grid = static_cast<uint64_t>(tiles) * a.n_req;
  if (grid > 0x7FFFFFFFull) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(a.out, 0, sizeof(orh_whatif_impact_rec) * static_cast<size_t>(a.n_req), s);
  if (e != hipSuccess) return e;
  auto al = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };
  const uint32_t vec = (a.n_nodes & 3u) == 0 && al(a.base_dist) && al(a.base_nh) && al(a.dist) && al(a.nh);
  hipLaunchKernelGGL(whatif_impact_kernel, dim3(static_cast<uint32_t>(grid)), dim3(kImpactBlock), 0, s, a, tiles,
                     vec);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(whatif_impact_fin_kernel, dim3((a.n_req + 255) / 256), dim3(256), 0, s, a.out, a.n_req);
  return hipGetLastError();
}

}  // namespace orh
