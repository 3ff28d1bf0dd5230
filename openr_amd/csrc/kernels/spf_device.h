// Batched SPF and route-selection kernels for gfx950 (MI355X).
//
// Semantics: LinkState::runSpf (openr/decision/LinkState.cpp:808-882) in its
// closed form, valid for link metrics >= 1:
//   d(u)   shortest metric over up, non-ignored links, no transit through an
//          overloaded node other than the source (:831-838)
//   NH(u)  = OR over predecessors (l, v) with d(v) + w_v(l) == d(u) and v a
//          transit node of   (v == src ? {u} : NH(v))          (:857-873)
//
// Two phases, both batched over many sources:
//
// 1. Distance rows (one workgroup per source row). The first-hop masks are
//    NOT carried through the search, so the per-source LDS state is only what
//    the distances need:
//      BFS    (every live link has the same metric w0): a u8/u16/u32 level
//             per node plus two frontier bitmaps; the row (level * w0) is
//             written to HBM once, coalesced, when the search ends. No
//             atomics return, no min-reduction: the next level is the next
//             frontier.
//      Dist16 / Dist32 (general metrics): a u16 or u32 distance per node plus
//             a pending-set bitmap; level-synchronous Dijkstra that expands
//             every node at the minimum pending distance D at once (exact for
//             positive integer metrics), the next D from a DPP wave minimum.
//    Small state buys occupancy: BFS on N = 10,000 needs 22.5 KB, so seven
//    sources are resident per CU.
// 2. First hops (one workgroup per (source, 1024-node tile)). With metrics
//    >= 1 the closed form unrolls to: bit i (the source's i-th distinct
//    neighbour n_i) is in NH(v) iff some up link s->n_i is tight
//    (w == d_s(n_i)) and either v == n_i, or n_i is not overloaded and
//    d_s(n_i) + d_{n_i}(v) == d_s(v), where d_{n_i} is n_i's own SPF with the
//    same ignore set (a tight path leaves s through n_i and continues along
//    a shortest path of n_i whose intermediates are transit nodes; paths of
//    n_i back through s are never tight). Phase 1 therefore also computes
//    the rows of the sources' neighbours (free for an all-sources sweep: they
//    are sources themselves), and phase 2 is a streaming, coalesced pass over
//    1 + deg(s) distance rows per source.
//
// Graph records are 8 bytes (col|flags, w_out), ELL-style K per node with a
// continuation into an overflow area, so expanding a node is ONE dependent
// global round trip (K records issued together, served from L2 where the
// graph stays resident for every workgroup on the XCD).
//
// This header: what every SPF kernel family shares (constants, wave
// reductions, the ignore-set tests, record loads) and the host launch helpers.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>
#include <type_traits>
#include <unordered_map>

#include "spf_kernels.h"

namespace orh {

constexpr int kBlock = 256;     // route selection, first hops
constexpr int kMaxBlock = 1024;  // SPF
constexpr int kOvfBatch = 8;     // overflow records in flight per expanded node
constexpr int kHopPer = 4;       // nodes per thread in the first-hop kernel
constexpr uint32_t kInf = 0xFFFFFFFFu;

__device__ inline bool ignored(const uint32_t* ign, uint32_t n, uint32_t link) {
  uint32_t lo = 0, hi = n;  // sorted ascending; tiny (KSP2 / what-if sets)
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    const uint32_t x = ign[mid];
    if (x == link) return true;
    if (x < link) lo = mid + 1; else hi = mid;
  }
  return false;
}

// is `node` in the request's drain set (what-if jobs: nodes treated as
// overloaded)? sorted ascending, a few entries; callers test n != 0 first
__device__ inline bool drained(const uint32_t* drn, uint32_t n, uint32_t node) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    const uint32_t x = drn[mid];
    if (x == node) return true;
    if (x < node) lo = mid + 1; else hi = mid;
  }
  return false;
}

__device__ inline uint32_t* dist_row(uint32_t* out, uint32_t* scratch, uint32_t n_out, uint32_t N,
                                     uint32_t row) {
  return row < n_out ? out + static_cast<size_t>(row) * N
                     : scratch + static_cast<size_t>(row - n_out) * N;
}

// wave-wide minimum through DPP row shifts and row broadcasts (no LDS)
__device__ inline uint32_t wave_min(uint32_t v) {
#define ORH_DPP_MIN(ctrl, rmask)                                                         \
  v = min(v, static_cast<uint32_t>(__builtin_amdgcn_update_dpp(                           \
                 static_cast<int>(kInf), static_cast<int>(v), ctrl, rmask, 0xF, false)))
  ORH_DPP_MIN(0x111, 0xF);  // row_shr:1
  ORH_DPP_MIN(0x112, 0xF);  // row_shr:2
  ORH_DPP_MIN(0x114, 0xF);  // row_shr:4
  ORH_DPP_MIN(0x118, 0xF);  // row_shr:8  -> lane 15 of each row holds the row minimum
  ORH_DPP_MIN(0x142, 0xA);  // row_bcast:15 into rows 1, 3
  ORH_DPP_MIN(0x143, 0xC);  // row_bcast:31 into rows 2, 3 -> lane 63 holds the minimum
#undef ORH_DPP_MIN
  return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), 63));
}

// wave-wide sum (every lane active), the DPP pattern of wave_min
__device__ inline uint32_t wave_sum(uint32_t v) {
#define ORH_DPP_ADD(ctrl, rmask) \
  v += static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), ctrl, rmask, 0xF, false))
  ORH_DPP_ADD(0x111, 0xF);  // row_shr:1
  ORH_DPP_ADD(0x112, 0xF);  // row_shr:2
  ORH_DPP_ADD(0x114, 0xF);  // row_shr:4
  ORH_DPP_ADD(0x118, 0xF);  // row_shr:8  -> lane 15 of each row holds the row sum
  ORH_DPP_ADD(0x142, 0xA);  // row_bcast:15 into rows 1, 3
  ORH_DPP_ADD(0x143, 0xC);  // row_bcast:31 into rows 2, 3 -> lane 63 holds the sum
#undef ORH_DPP_ADD
  return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), 63));
}

struct Src {
  uint32_t node;
  const uint32_t* ign;
  uint32_t n_ign;
  // optional LDS filter of the ignore set (a bit per hashed link id, no
  // false negatives): a clear bit skips the binary search in global memory
  const uint32_t* filt;
  uint32_t fshift;
  // the row's drained nodes (SpfArgs::drain_ptr); set by the kernel
  // instantiation that honours them (spf_global_nh_async_kernel, kDrain)
  const uint32_t* drn;
  uint32_t n_drn;
  __device__ Src(const SpfArgs& a, uint32_t row)
      : node(a.srcs[row]), ign(nullptr), n_ign(0), filt(nullptr), fshift(0), drn(nullptr), n_drn(0) {
    if (a.ignore_ptr) {
      const uint32_t b = a.ignore_ptr[row];
      ign = a.ignore_links + b;
      n_ign = a.ignore_ptr[row + 1] - b;
    }
  }
};

__device__ inline uint32_t ign_hash(uint32_t link, uint32_t shift) { return (link * 0x9E3779B1u) >> shift; }

// a record the search may relax: up, not a continuation, not ignored
__device__ inline bool live(const SpfArgs& a, const Src& s, const uint2& r, uint32_t q) {
  if (r.x & (ORH_REC_SKIP | ORH_REC_CONT)) return false;
  if (!s.n_ign) return true;
  const uint32_t l = a.link[q];
  if (s.filt) {
    const uint32_t h = ign_hash(l, s.fshift);
    if (!((s.filt[h >> 5] >> (h & 31u)) & 1u)) return true;
  }
  return !ignored(s.ign, s.n_ign, l);
}

// live() with the record's link id already loaded (searches with ignore sets
// fetch the ids together with the records: one round trip, not two)
__device__ inline bool live_link(const Src& s, const uint2& r, uint32_t l) {
  if (r.x & (ORH_REC_SKIP | ORH_REC_CONT)) return false;
  if (!s.n_ign) return true;
  if (s.filt) {
    const uint32_t h = ign_hash(l, s.fshift);
    if (!((s.filt[h >> 5] >> (h & 31u)) & 1u)) return true;
  }
  return !ignored(s.ign, s.n_ign, l);
}

template <int K>
__device__ inline void load_recs(const SpfArgs& a, uint32_t v, uint2 (&rec)[K]) {
  const uint2* slots = a.recs + static_cast<size_t>(v) * K;
#pragma unroll
  for (int j = 0; j < K; ++j) rec[j] = slots[j];
}

// level bytes of the multi-source BFS plans (spf_msbfs_kernel writes them,
// the first-hop kernels read them): 254 = the u32 row holds the distance
// (levels >= 254), 255 = unreached
constexpr uint32_t kLvlDirect = 254u, kLvlNone = 255u;

// The first-hop test over level bytes, four nodes per word op: source s has
// neighbour n as a tight first hop towards v iff L_n(v) + 1 == L_s(v) with v
// reached from s. The callers keep kLvlDirect bytes away (the levels behind
// them are in the u32 rows).
// 0x80 in every byte of z that is zero
__host__ __device__ inline uint32_t lvl_zero_bytes(uint32_t z) {
  return ~(((z & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | z | 0x7F7F7F7Fu);
}
// a source's own level word with byte src_byte (0..3, else none: the source
// itself, which has no next hops) forced to "unreached"
__host__ __device__ inline uint32_t lvl_own_forced(uint32_t ow, uint32_t src_byte) {
  return src_byte < 4u ? ow | (0xFFu << (src_byte * 8u)) : ow;
}
// 0x80 in every byte of a level word that is reached (not kLvlNone)
__host__ __device__ inline uint32_t lvl_reached(uint32_t w) { return ~lvl_zero_bytes(~w) & 0x80808080u; }
// 0x01 in every byte where nw + 1 == ot and ot is reached (`reached` =
// lvl_reached(ot); a kernel whose rows hold no kLvlDirect byte passes
// kLvlAllReached, which folds away: only nw = 254 increments to 255). The increment is bytewise mod 256: the low seven bits
// carry into bit 7, which is then flipped back by the byte's own bit 7, so no
// carry leaves a byte; a neighbour's 255 wraps to 0, a level only the source
// holds, which lvl_own_forced turned into 255
constexpr uint32_t kLvlAllReached = 0x80808080u;
__host__ __device__ inline uint32_t lvl_tight(uint32_t nw, uint32_t ot, uint32_t reached) {
  const uint32_t inc = ((nw & 0x7F7F7F7Fu) + 0x01010101u) ^ (nw & 0x80808080u);
  return (lvl_zero_bytes(inc ^ ot) & reached) >> 7;
}
// the whole test of one neighbour word against one own word
__host__ __device__ inline uint32_t lvl_tight_word(uint32_t nw, uint32_t ow, uint32_t src_byte) {
  const uint32_t ot = lvl_own_forced(ow, src_byte);
  return lvl_tight(nw, ot, lvl_reached(ot));
}

// workgroup barrier that orders LDS only (s_waitcnt lgkmcnt(0) + s_barrier);
// the "memory" clobber keeps the compiler from moving LDS accesses across it
__device__ inline void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// wave-wide OR (same DPP pattern as wave_min)
__device__ inline uint32_t wave_or(uint32_t v) {
#define ORH_DPP_OR(ctrl, rmask)                                                     \
  v |= static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), ctrl, rmask, 0xF, false))
  ORH_DPP_OR(0x111, 0xF);
  ORH_DPP_OR(0x112, 0xF);
  ORH_DPP_OR(0x114, 0xF);
  ORH_DPP_OR(0x118, 0xF);
  ORH_DPP_OR(0x142, 0xA);
  ORH_DPP_OR(0x143, 0xC);
#undef ORH_DPP_OR
  return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), 63));
}

// f(integral_constant<int, i>) for i in [0, J), unrolled at compile time
template <int J, int I = 0, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < J) {
    f(std::integral_constant<int, I>{});
    static_for<J, I + 1>(f);
  }
}

// XCD-aware block order: the dispatcher deals workgroups round-robin over the
// 8 XCDs (block b -> XCD b % 8), each with its own L2. Remapped, XCD x runs a
// contiguous range of logical blocks, so the sources resident on one XCD at a
// time are neighbours in row order and share their neighbours' level rows in
// that XCD's L2 instead of each XCD fetching them from HBM. Bijective for any
// grid size.
__device__ inline uint32_t xcd_block(uint32_t b, uint32_t nb, uint32_t group) {
  constexpr uint32_t kXcd = 8;
  if (group == 0) {  // one contiguous range per XCD
    const uint32_t x = b % kXcd, k = b / kXcd, q = nb / kXcd, r = nb % kXcd;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + k;
  }
  // runs of `group` consecutive blocks per XCD, dealt round-robin; the tail
  // that does not fill a whole round keeps its order
  const uint32_t full = nb / (kXcd * group) * (kXcd * group);
  if (b >= full) return b;
  const uint32_t x = b % kXcd, k = b / kXcd;
  return ((k / group) * kXcd + x) * group + k % group;
}

// dynamic-LDS opt-in, raised once per kernel to the largest size launched
// (hipFuncSetAttribute is a runtime call worth avoiding on every sweep)
template <typename Kern>
static hipError_t lds_opt_in(Kern kernel, size_t lds) {
  static std::mutex mu;
  static std::unordered_map<const void*, size_t> granted;
  const void* f = reinterpret_cast<const void*>(kernel);
  std::lock_guard<std::mutex> lock(mu);
  auto it = granted.find(f);
  if (it != granted.end() && lds <= it->second) return hipSuccess;
  hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     static_cast<int>(lds));
  if (e == hipSuccess) granted[f] = lds;
  return e;
}

template <typename Kern, typename Args>
static hipError_t launch(Kern kernel, const Args& a, uint32_t grid, uint32_t block, size_t lds,
                         hipStream_t s) {
  hipError_t e = lds_opt_in(kernel, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), lds, s, a);
  return hipGetLastError();
}

inline size_t align16(size_t x) { return (x + 15) & ~static_cast<size_t>(15); }

}  // namespace orh
