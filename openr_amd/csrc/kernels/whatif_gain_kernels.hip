// Two-sided what-if summaries (orh_whatif_gain): each request's row against the
// base row of its source, reduced on the device to one orh_whatif_gain_rec
// while the row is still in its buffer. Where orh_whatif_impact assumes that a
// request only lengthens paths, these records also count the nodes that got
// nearer (a metric lower: orh_whatif_run_lowers) and those that gained an
// equal-cost first hop.
//
//   whatif_gain_kernel     one workgroup per (request, tile of kGainTile
//                          nodes), the shape of whatif_impact_kernel: classify,
//                          reduce in the wave, then the workgroup, then atomics
//                          into the record - only for a tile in which some node
//                          is in a class. A tier-0 request's workgroups exit
//                          before they read anything.
//   whatif_gain_fin_kernel one thread per request: the two keys the tiles
//                          maximised, (stretch, ~node) and (gain, ~node), become
//                          max_stretch / worst_node and max_gain / best_node
//                          (ORH_NO_NODE without a farther / nearer node).
//
// The direction of a changed distance is decided with > and < before anything
// is subtracted, so no difference is ever taken the wrong way round. The
// records are zeroed before the first kernel (launch_whatif_gain). The request
// rows are read once (non-temporal loads); the base rows are shared by every
// request of a source and stay in cache (plain loads).
#include "../../../include/openr_hip.h"
#include "whatif_kernels.h"

namespace orh {

namespace {

constexpr uint32_t kGainBlock = 256;
constexpr uint32_t kGainTile = kGainBlock * 8;  // nodes of a row per workgroup: two uint4 per lane and array

// a record while its tiles accumulate: the keys (stretch << 32 | ~node) and
// (gain << 32 | ~node) lie over max_stretch / worst_node and max_gain / best_node
struct GainAcc {
  uint32_t lost, farther, nearer, rehomed, narrowed, widened;
  unsigned long long key_far, key_near, sum_stretch, sum_gain, lost_weight, moved_weight, nearer_weight;
};
static_assert(sizeof(orh_whatif_gain_rec) == 80, "orh_whatif_gain_rec is 80 bytes");
static_assert(sizeof(GainAcc) == sizeof(orh_whatif_gain_rec), "accumulator and record share their bytes");
static_assert(offsetof(GainAcc, key_far) == offsetof(orh_whatif_gain_rec, max_stretch) &&
                  offsetof(GainAcc, key_near) == offsetof(orh_whatif_gain_rec, max_gain) &&
                  offsetof(GainAcc, sum_stretch) == offsetof(orh_whatif_gain_rec, sum_stretch),
              "the keys lie over the (max, node) pairs");

// per-lane partials of one tile. The six class counts take kCntBits bits each
// in two packed words: dist packs lost, farther, nearer and rehomed (the
// classes of `moved`, one per node at most), mask packs narrowed and widened
constexpr uint32_t kCntBits = 16;
constexpr uint32_t kCntMask = (1u << kCntBits) - 1u;
static_assert(kGainTile <= kCntMask, "a class count of a whole tile fits its packed field");
static_assert(4 * kCntBits <= 64 && 2 * kCntBits <= 32, "four fields in the u64 word, two in the u32 word");
constexpr unsigned long long kOneLost = 1ull, kOneFarther = 1ull << kCntBits, kOneNearer = 1ull << (2 * kCntBits),
                             kOneRehomed = 1ull << (3 * kCntBits);
constexpr uint32_t kOneNarrowed = 1u, kOneWidened = 1u << kCntBits;

struct Lane {
  unsigned long long dist;  // packed counts, see above
  uint32_t mask;
  unsigned long long key_far, key_near, sum_far, sum_near, lw, mw, nw;
};

__device__ __forceinline__ void classify(const GainArgs& a, uint32_t v, uint32_t src, uint32_t bd, uint32_t bn,
                                         uint32_t rd, uint32_t rn, Lane& l) {
  if (bd == ORH_UNREACHABLE || v == src) return;
  bool moved = false;
  if (rd == ORH_UNREACHABLE) {
    l.dist += kOneLost;
    if (a.weight) l.lw += a.weight[v];
    if (a.node_lost) atomicAdd(a.node_lost + v, 1u);
    moved = true;
  } else {
    if (rd > bd) {
      const uint32_t stretch = rd - bd;
      l.dist += kOneFarther;
      l.sum_far += stretch;
      const unsigned long long k = (static_cast<unsigned long long>(stretch) << 32) | (~v);
      l.key_far = k > l.key_far ? k : l.key_far;
      moved = true;
    } else if (rd < bd) {
      const uint32_t gain = bd - rd;
      l.dist += kOneNearer;
      l.sum_near += gain;
      const unsigned long long k = (static_cast<unsigned long long>(gain) << 32) | (~v);
      l.key_near = k > l.key_near ? k : l.key_near;
      if (a.weight) l.nw += a.weight[v];
      if (a.node_nearer) atomicAdd(a.node_nearer + v, 1u);
      moved = true;
    } else if (rn != bn) {
      l.dist += kOneRehomed;
      moved = true;
    }
    const int pr = __popc(rn), pb = __popc(bn);
    if (pr < pb) l.mask += kOneNarrowed;
    else if (pr > pb) l.mask += kOneWidened;
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

__global__ __launch_bounds__(kGainBlock) void whatif_gain_kernel(GainArgs a, uint32_t tiles, uint32_t vec) {
  const uint32_t r = blockIdx.x / tiles;
  const uint32_t t = blockIdx.x % tiles;
  // tier 0: the source's row stands (for a run with lowers too), the zeroed
  // record is the answer, and the row (never written under
  // ORH_WHATIF_SHARE_BASE) is not read
  if (a.info && ORH_WHATIF_TIER(a.info[r]) == 0) return;
  const size_t N = a.n_nodes;
  const size_t b = a.base_row[r];
  const uint32_t src = a.srcs[r];
  const uint32_t* bd = a.base_dist + b * N;
  const uint32_t* bn = a.base_nh + b * N;
  const uint32_t* rd = a.dist + r * N;
  const uint32_t* rn = a.nh + r * N;
  const uint32_t lo = t * kGainTile;
  const uint32_t hi = static_cast<uint32_t>(min(static_cast<size_t>(lo) + kGainTile, N));
  Lane l{};
  if (vec) {
    typedef uint32_t v4 __attribute__((ext_vector_type(4)));
#pragma unroll 2
    for (uint32_t i = lo / 4 + threadIdx.x; i < hi / 4; i += kGainBlock) {
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
    for (uint32_t i = lo + threadIdx.x; i < hi; i += kGainBlock) {
      const uint32_t qd = rd[i], qn = rn[i], pd = bd[i], pn = bn[i];
      if (qd != pd || qn != pn) classify(a, i, src, pd, pn, qd, qn, l);
    }
  }
  // a node in any class sets a count (narrowed or widened alone included)
  if (!__syncthreads_or((l.dist | l.mask) != 0)) return;
  for (int o = 32; o > 0; o >>= 1) {
    l.dist += shfl_xor_u64(l.dist, o);
    l.mask += static_cast<uint32_t>(__shfl_xor(static_cast<int>(l.mask), o));
    l.sum_far += shfl_xor_u64(l.sum_far, o);
    l.sum_near += shfl_xor_u64(l.sum_near, o);
    l.lw += shfl_xor_u64(l.lw, o);
    l.mw += shfl_xor_u64(l.mw, o);
    l.nw += shfl_xor_u64(l.nw, o);
    unsigned long long k = shfl_xor_u64(l.key_far, o);
    l.key_far = k > l.key_far ? k : l.key_far;
    k = shfl_xor_u64(l.key_near, o);
    l.key_near = k > l.key_near ? k : l.key_near;
  }
  constexpr uint32_t kWaves = kGainBlock / 64;
  __shared__ Lane part[kWaves];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = l;
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (uint32_t w = 1; w < kWaves; ++w) {
    l.dist += part[w].dist;
    l.mask += part[w].mask;
    l.sum_far += part[w].sum_far;
    l.sum_near += part[w].sum_near;
    l.lw += part[w].lw;
    l.mw += part[w].mw;
    l.nw += part[w].nw;
    l.key_far = part[w].key_far > l.key_far ? part[w].key_far : l.key_far;
    l.key_near = part[w].key_near > l.key_near ? part[w].key_near : l.key_near;
  }
  GainAcc* out = reinterpret_cast<GainAcc*>(a.out) + r;
  const uint32_t lost = static_cast<uint32_t>(l.dist) & kCntMask,
                 farther = static_cast<uint32_t>(l.dist >> kCntBits) & kCntMask,
                 nearer = static_cast<uint32_t>(l.dist >> (2 * kCntBits)) & kCntMask,
                 rehomed = static_cast<uint32_t>(l.dist >> (3 * kCntBits)) & kCntMask,
                 narrowed = l.mask & kCntMask, widened = (l.mask >> kCntBits) & kCntMask;
  if (lost) atomicAdd(&out->lost, lost);
  if (farther) {
    atomicAdd(&out->farther, farther);
    atomicMax(&out->key_far, l.key_far);
    atomicAdd(&out->sum_stretch, l.sum_far);
  }
  if (nearer) {
    atomicAdd(&out->nearer, nearer);
    atomicMax(&out->key_near, l.key_near);
    atomicAdd(&out->sum_gain, l.sum_near);
  }
  if (rehomed) atomicAdd(&out->rehomed, rehomed);
  if (narrowed) atomicAdd(&out->narrowed, narrowed);
  if (widened) atomicAdd(&out->widened, widened);
  if (l.lw) atomicAdd(&out->lost_weight, l.lw);
  if (l.mw) atomicAdd(&out->moved_weight, l.mw);
  if (l.nw) atomicAdd(&out->nearer_weight, l.nw);
}

__global__ __launch_bounds__(256) void whatif_gain_fin_kernel(orh_whatif_gain_rec* out, uint32_t n_req) {
  const uint32_t r = blockIdx.x * 256 + threadIdx.x;
  if (r >= n_req) return;
  const GainAcc acc = reinterpret_cast<const GainAcc*>(out)[r];
  out[r].max_stretch = acc.farther ? static_cast<uint32_t>(acc.key_far >> 32) : 0u;
  out[r].worst_node = acc.farther ? ~static_cast<uint32_t>(acc.key_far) : ORH_NO_NODE;
  out[r].max_gain = acc.nearer ? static_cast<uint32_t>(acc.key_near >> 32) : 0u;
  out[r].best_node = acc.nearer ? ~static_cast<uint32_t>(acc.key_near) : ORH_NO_NODE;
}

}  // namespace

hipError_t launch_whatif_gain(const GainArgs& a, hipStream_t s) {
  if (a.n_req == 0) return hipSuccess;
  const uint32_t tiles = (a.n_nodes + kGainTile - 1) / kGainTile;
  const uint64_t grid = static_cast<uint64_t>(tiles) * a.n_req;
  if (grid > 0x7FFFFFFFull) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(a.out, 0, sizeof(orh_whatif_gain_rec) * static_cast<size_t>(a.n_req), s);
  if (e != hipSuccess) return e;
  auto al = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };
  const uint32_t vec = (a.n_nodes & 3u) == 0 && al(a.base_dist) && al(a.base_nh) && al(a.dist) && al(a.nh);
  hipLaunchKernelGGL(whatif_gain_kernel, dim3(static_cast<uint32_t>(grid)), dim3(kGainBlock), 0, s, a, tiles, vec);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(whatif_gain_fin_kernel, dim3((a.n_req + 255) / 256), dim3(256), 0, s, a.out, a.n_req);
  return hipGetLastError();
}

}  // namespace orh
