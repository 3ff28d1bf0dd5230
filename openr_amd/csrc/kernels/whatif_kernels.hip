// What-if repair: batched runSpf(src, useLinkMetric, linksToIgnore) derived
// from the plain SPF rows of the batch's sources (gfx950).
//
// A what-if batch (link-failure SPFs, "1,024 runSpf(src,
// true, {link})" = few sources x many links) repeats its sources. Removing
// links only lengthens paths, and only below a link that is tight on the
// source's shortest-path DAG (LinkState.cpp:857-873 closed form, SURVEY.md
// Appendix A.1):
//
//   A = the heads of the ignored links that are tight (d(x) + w_x = d(y), x
//       a transit node), closed under tight out-edges of transit nodes.
//
// Every node outside A keeps its distance AND its first-hop set: none of its
// tight predecessors is in A and none of its tight in-links is ignored, so by
// induction on d its predecessor set is unchanged. Nodes in A are re-derived
// from the closed form restricted to A: a boundary label per node (the lattice
// meet over its predecessors outside A: smaller distance replaces, equal
// distance ORs the masks) and then chaotic relaxation over the predecessor
// edges inside A until no label changes. Positive metrics make the predecessor
// graph of the final labels acyclic, so the fixpoint is unique and equals what
// a fresh search computes: results are bit-identical to runSpf on the reduced
// graph. A link-failure batch touches few nodes per request (C4: 55 % of the
// requests have an empty A, the mean is 4 nodes, the largest 932), so the
// batch costs its sources' searches plus one streaming copy of the rows.
//
// Kernels:
//   whatif_copy_kernel    base rows -> request rows (dist + one mask word),
//                         16-byte loads/stores, HBM-bound (the output floor)
//   whatif_repair_kernel  one workgroup per request: A in LDS (bitmap over
//                         the nodes, node list, labels, predecessor edges);
//                         a request whose A or edge list outgrows LDS is
//                         flagged, repaired again with its state in a global
//                         slot sized for the whole graph, and only when the
//                         slots run out re-searched by
//                         spf_global_nh_async_kernel with the flags as its
//                         row mask
//
// Drained nodes (orh_whatif_run_drains): a request may also name nodes to be
// treated as overloaded. Draining X (not the source, reached, not already
// overloaded) removes exactly the relaxations out of X, so it is a link cut in
// one direction only: the host stages one cut (X, y, record X -> y) per
// out-record of X and the seeds take them as they are. A then is
//
//   the heads of the tight ignored links and of the tight out-records of the
//   drained nodes, closed under tight out-records of transit nodes that are
//   not drained in this request
//
// (a drained node inside A is re-derived but not expanded: its own tight
// heads are seeds already), and the predecessor rule skips a drained
// predecessor p != s as it skips an overloaded one. The lattice argument is
// unchanged: relaxations are only removed, a node outside A keeps all of its
// tight predecessors (none is in A, none drained with a tight record to it,
// since that record's head would be a seed), and inside A the fixpoint over
// the remaining predecessor edges is unique. The repair kernels are
// instantiated with and without the drain tests (kDrain); a run without
// drains launches the code it always did. Tier 4's full search honours the
// set through SpfArgs::drain_ptr (spf_hbm_kernels.hip, its own kDrain).
//
// Metric raises (orh_whatif_run_metrics): a request may also raise the metric
// one end of a link advertises (Link::setMetricFromNode, LinkState.cpp:640-710:
// costing a link out). An ignored link is a metric raised to infinity, and the
// argument above needs only that relaxations get weaker: with w the record's
// own weight and w' >= w the raised one, the host stages one cut (tail, head,
// record) per raised record next to the ignore and drain cuts, and a sorted
// per-request list (record, w'). Then
//
//   seeds    as before: heads of the cut records that are tight in the base
//            row under the OLD weight w (tail a transit node)
//   closure  unchanged, under the old weights
//   pred     an ignored link is skipped (ignore wins over a raise of the same
//            link); else the edge weighs w' when the request raises that
//            record, w otherwise - inside A and at its boundary alike
//
// A node outside A keeps every tight predecessor at its old weight (a raised
// tight record's head is a seed), no label got smaller anywhere, so its row
// entry stands; inside A the fixpoint over the reweighted predecessor edges is
// unique as before. Templated on kRaise like kDrain: a run without raises
// launches the instantiations it always did. The full search is not taught
// about raises: a run that stages any takes none (the host leaves full_cap 0
// and refuses a graph without slots), so tier 3, whose state is sized for the
// whole graph, ends every such request.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "spf_device.h"  // edge record flags, ignored()
#include "whatif_device.h"  // meet, bar, for_records, cut_tight, relabel
#include "whatif_kernels.h"

namespace orh {
namespace {

constexpr uint32_t kSlotBlock = 1024;  // slot pass: few large affected sets, one per CU
constexpr uint32_t kCopyTile = 256 * 16;  // u32 elements of a row per copy workgroup

// base rows -> request rows; vec: every row is 16-byte aligned (N % 4 == 0
// and aligned buffers), so a thread moves uint4s
__global__ __launch_bounds__(256) void whatif_copy_kernel(RepairArgs a, uint32_t tiles, uint32_t vec) {
  uint32_t r = blockIdx.x / tiles;
  const uint32_t t = blockIdx.x % tiles;
  if (a.share_base) {  // block i copies the i-th queued request's row
    if (r >= a.counters[0]) return;
    r = a.queues[r];
  }
  const size_t N = a.n_nodes;
  const size_t b = a.base_row[r];
  const uint32_t* sd = a.base_dist + b * N;
  const uint32_t* sn = a.base_nh + b * N;
  uint32_t* dd = a.out_dist + r * N;
  uint32_t* dn = a.out_nh + r * N;
  const size_t lo = static_cast<size_t>(t) * kCopyTile, hi = min(lo + kCopyTile, N);
  if (vec) {
    typedef uint32_t v4 __attribute__((ext_vector_type(4)));
    for (size_t i = lo / 4 + threadIdx.x; i < hi / 4; i += 256) {
      __builtin_nontemporal_store(reinterpret_cast<const v4*>(sd)[i], reinterpret_cast<v4*>(dd) + i);
      __builtin_nontemporal_store(reinterpret_cast<const v4*>(sn)[i], reinterpret_cast<v4*>(dn) + i);
    }
  } else {
    for (size_t i = lo + threadIdx.x; i < hi; i += 256) {
      dd[i] = sd[i];
      dn[i] = sn[i];
    }
  }
}

// One request: A (the nodes below a tight ignored link, closed under tight
// out-records of transit nodes), boundary labels from predecessors outside
// A, chaotic relaxation inside A, rows written. State at `base` with the
// caps cap_a / cap_e (LDS, or a global slot with whole-graph caps). Returns
// |A|, or ~0u when A or its edge list outgrows the caps. The membership
// bitmap must be all zero on entry; the caller clears it afterwards.
template <int K, bool kDrain, bool kRaise>
__device__ uint32_t repair_one(const RepairArgs& a, uint32_t r, uint32_t* base, uint32_t cap_a, uint32_t cap_e,
                               uint32_t* s_cnt, uint32_t* s_ecnt, uint32_t* s_ovf, uint32_t* s_flag) {
  const uint32_t N = a.n_nodes;
  const uint32_t tid = threadIdx.x, B = blockDim.x;
  const RepairState st(base, cap_a, cap_e);  // the layout: whatif_device.h
  uint32_t* alist = st.alist;
  uint32_t* bits = st.bits;

  const uint32_t s = a.srcs[r];
  const size_t b = a.base_row[r];
  const uint32_t* bd = a.base_dist + b * N;
  const uint32_t* bn = a.base_nh + b * N;
  const bool metric = a.use_link_metric != 0;
  // the request's drained nodes (sorted; never s): no transit, like ovl
  const uint32_t* drn = nullptr;
  uint32_t n_drn = 0;
  if constexpr (kDrain) {
    drn = a.drn + a.drn_ptr[r];
    n_drn = a.drn_ptr[r + 1] - a.drn_ptr[r];
  }
  // the request's raised records (sorted by record): read-only global memory,
  // in the slot pass too, so no barrier orders it
  const uint2* rse = nullptr;
  uint32_t n_rse = 0;
  if constexpr (kRaise) {
    rse = a.rse + a.rse_ptr[r];
    n_rse = a.rse_ptr[r + 1] - a.rse_ptr[r];
  }

  if (tid == 0) {
    *s_cnt = 0u;
    *s_ecnt = 0u;
    *s_ovf = 0u;
  }
  if (tid < 3) s_flag[tid] = 0u;
  bar();

  auto add = [&](uint32_t u) {
    const uint32_t bit = 1u << (u & 31u);
    if (atomicOr(&bits[u >> 5], bit) & bit) return;
    const uint32_t k = atomicAdd(s_cnt, 1u);
    if (k < cap_a) alist[k] = u;
    else *s_ovf = 1u;
  };
  // seeds: heads of tight ignored records whose tail is a transit node (a
  // drained node's out-records and the raised records are staged as cuts of
  // their own; tight means tight under the record's own, old weight)
  for (uint32_t c = a.cut_ptr[r] + tid; c < a.cut_ptr[r + 1]; c += B) {
    const uint4 cut = a.cuts[c];  // (tail, head, record of tail -> head, 0)
    if (cut_tight(a, bd, s, cut)) add(cut.y);
  }
  bar();
  if (*s_cnt == 0u) return 0u;  // nothing below a tight ignored link: the base row stands

  // A: closure under tight out-records of transit nodes, level by level
  uint32_t lo = 0;
  for (;;) {
    const uint32_t hi = min(*s_cnt, cap_a);
    const bool ovf = *s_ovf != 0u;
    bar();  // everyone has read the range before it grows
    if (ovf || lo == hi) break;
    for (uint32_t k = lo + tid; k < hi; k += B) {
      const uint32_t v = alist[k];
      if (a.ovl[v]) continue;  // reached, but no transit (v != s: s is never in A)
      if constexpr (kDrain)
        if (n_drn && drained(drn, n_drn, v)) continue;  // re-derived, not expanded
      const uint64_t dv = bd[v];
      for_records<K>(a.recs, v, [&](const uint2& rec, uint32_t) {
        const uint32_t u = rec.x & ORH_REC_COL_MASK;
        if (bits[u >> 5] & (1u << (u & 31u))) return;
        if (dv + (metric ? rec.y : 1u) == bd[u]) add(u);
      });
    }
    lo = hi;
    bar();
  }
  const uint32_t n = min(*s_cnt, cap_a);
  if (*s_ovf) return ~0u;
  // boundary labels from the base rows of the predecessors outside A, then
  // the fixpoint inside A, under the request's raised weights
  return relabel<K, kDrain, kRaise>(a, r, st, cap_e, n, bd, bn, rse, n_rse, s_ecnt, s_ovf, s_flag);
}

// seed pass, one thread per request: a request with no tight ignored link
// keeps the copied base row (tier 0); the others join queue 0 (wave-aggregated
// appends: one atomic per wave)
__global__ __launch_bounds__(256) void whatif_seed_kernel(RepairArgs a) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  bool hit = false;
  if (r < a.n_req) {
    const uint32_t N = a.n_nodes;
    const uint32_t s = a.srcs[r];
    const uint32_t* bd = a.base_dist + static_cast<size_t>(a.base_row[r]) * N;
    for (uint32_t c = a.cut_ptr[r]; c < a.cut_ptr[r + 1] && !hit; ++c) hit = cut_tight(a, bd, s, a.cuts[c]);
    if (a.info) a.info[r] = kWhatifTierBase;
  }
  const unsigned long long m = __ballot(hit);
  if (!m) return;
  const uint32_t lane = __lane_id();
  const uint32_t leader = static_cast<uint32_t>(__builtin_ctzll(m));
  uint32_t at = 0;
  if (lane == leader) at = atomicAdd(&a.counters[0], static_cast<uint32_t>(__popcll(m)));
  at = __shfl(at, static_cast<int>(leader));
  if (hit) a.queues[at + static_cast<uint32_t>(__popcll(m & ((1ull << lane) - 1ull)))] = r;
}

// tier kTier drains queue q into queue q + 1: LDS state (tiers 1, 2) or one global
// slot per workgroup (tier 3); a request that outgrows the caps moves on to
// the next queue. Every workgroup leaves once its claim passes the queue's
// length (fixed before this launch by the previous kernel).
template <int K, uint32_t kTier, bool kDrain, bool kRaise>
__global__ __launch_bounds__(kTier == kWhatifTierSmall ? 128 : kTier == kWhatifTierLarge ? 256 : kSlotBlock)
void whatif_repair_kernel(RepairArgs a, uint32_t cap_a, uint32_t cap_e, uint32_t q) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  __shared__ uint32_t s_cnt, s_ecnt, s_ovf, s_req;
  __shared__ uint32_t s_flag[3];
  constexpr bool kSlot = kTier == kWhatifTierSlot;
  const uint32_t N = a.n_nodes, NB = (N + 31) / 32;
  const uint32_t tid = threadIdx.x, B = blockDim.x;
  uint32_t* base = kSlot ? reinterpret_cast<uint32_t*>(a.slot_mem + blockIdx.x * a.slot_bytes) : lds;
  uint32_t* alist = base + 2 * 2 * cap_a + 2 * cap_e + 2 * cap_a;  // see repair_one's layout
  uint32_t* bits = alist + cap_a;
  for (uint32_t i = tid; i < NB; i += B) bits[i] = 0u;
  const uint32_t len = a.counters[2 * q];
  const uint32_t skip = kSlot ? min(len, a.full_cap) : 0u;  // the full search's share
  if (kSlot && a.info)
    for (uint32_t i = blockIdx.x * B + tid; i < skip; i += gridDim.x * B)
      a.info[a.queues[static_cast<size_t>(q) * a.n_req + i]] = kWhatifTierSearch;
  for (;;) {
    if (tid == 0) {
      const uint32_t i = atomicAdd(&a.counters[2 * q + 1], 1u) + skip;
      s_req = i < len ? a.queues[static_cast<size_t>(q) * a.n_req + i] : ~0u;
    }
    bar();
    const uint32_t r = s_req;
    if (r == ~0u) break;
    const uint32_t n = repair_one<K, kDrain, kRaise>(a, r, base, cap_a, cap_e, &s_cnt, &s_ecnt, &s_ovf, s_flag);
    if (tid == 0) {
      if (n != ~0u) {
        if (a.info) a.info[r] = kTier | (n << 3);
        if (kSlot) a.fallback[r] = 0u;
      } else if (!kSlot) {
        const uint32_t j = atomicAdd(&a.counters[2 * (q + 1)], 1u);
        a.queues[static_cast<size_t>(q + 1) * a.n_req + j] = r;
        if (kTier == kWhatifTierLarge) a.fallback[r] = 1u;  // the full search takes it without slots
      }
    }
    // clear the membership bitmap: through the node list when it holds all
    // of A, else whole
    const uint32_t cnt = s_cnt;
    bar();
    if (cnt > cap_a) {
      for (uint32_t i = tid; i < NB; i += B) bits[i] = 0u;
    } else {
      for (uint32_t k = tid; k < cnt; k += B) bits[alist[k] >> 5] = 0u;
    }
    bar();
  }
}

}  // namespace

size_t repair_lds_bytes(uint32_t n_nodes, uint32_t cap_a, uint32_t cap_e) {
  return static_cast<size_t>(cap_a) * (8 + 8 + 8 + 4) + static_cast<size_t>(cap_e) * 8 +
         static_cast<size_t>((n_nodes + 31) / 32) * 4;
}

size_t repair_slot_bytes(uint32_t n_nodes, uint32_t n_recs) {
  return (repair_lds_bytes(n_nodes, n_nodes, n_recs) + 255) & ~static_cast<size_t>(255);
}

namespace {

size_t tier1_lds(const RepairArgs& a, uint32_t* sa, uint32_t* se) {
  *sa = std::min(kSmallA, a.cap_a);
  *se = std::min(kSmallE, a.cap_e);
  return repair_lds_bytes(a.n_nodes, *sa, *se);
}

// queue-draining grids: as many workgroups as the LDS lets share a CU (one
// request each at a time), never more than there are requests
uint32_t tier_grid(const RepairArgs& a, size_t lds_limit, size_t lds, uint32_t per_cu_cap) {
  const uint32_t per_cu = static_cast<uint32_t>(std::min<size_t>(per_cu_cap, std::max<size_t>(1, lds_limit / lds)));
  return std::max<uint32_t>(1u, std::min<uint32_t>(a.n_req, a.n_cu * per_cu));
}

}  // namespace

hipError_t launch_repair_front(const RepairArgs& a, uint32_t ell_k, size_t lds_limit, hipStream_t s) {
  if (a.n_req == 0) return hipSuccess;
  if (ell_k != 4 && ell_k != 8) return hipErrorInvalidValue;
  const uint32_t tiles = (a.n_nodes + kCopyTile - 1) / kCopyTile;
  const uint64_t grid = static_cast<uint64_t>(tiles) * a.n_req;
  if (grid > 0x7FFFFFFFull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(whatif_seed_kernel, dim3((a.n_req + 255) / 256), dim3(256), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  auto al = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };
  const uint32_t vec = (a.n_nodes & 3u) == 0 && al(a.base_dist) && al(a.base_nh) && al(a.out_dist) &&
                       al(a.out_nh);
  hipLaunchKernelGGL(whatif_copy_kernel, dim3(static_cast<uint32_t>(grid)), dim3(256), 0, s, a, tiles, vec);
  return hipGetLastError();
}

hipError_t launch_repair_back(const RepairArgs& a, uint32_t ell_k, size_t lds_limit, hipStream_t s) {
  return launch_repair_back_split(a, ell_k, lds_limit, s, s, nullptr);
}

namespace {

// one tier's launch: the instantiation for the graph's ELL width, with the
// drain tests only when the run stages drained nodes and the raised weights
// only when it stages metric raises
template <uint32_t kTier>
hipError_t launch_tier(const RepairArgs& a, uint32_t ell_k, uint32_t grid, uint32_t block, size_t lds,
                       hipStream_t s, uint32_t cap_a, uint32_t cap_e, uint32_t q) {
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), lds, s, a, cap_a, cap_e, q);
    return hipGetLastError();
  };
  if (a.rse_ptr) {
    if (a.drn_ptr)
      return ell_k == 8 ? go(whatif_repair_kernel<8, kTier, true, true>)
                        : go(whatif_repair_kernel<4, kTier, true, true>);
    return ell_k == 8 ? go(whatif_repair_kernel<8, kTier, false, true>)
                      : go(whatif_repair_kernel<4, kTier, false, true>);
  }
  if (a.drn_ptr)
    return ell_k == 8 ? go(whatif_repair_kernel<8, kTier, true, false>)
                      : go(whatif_repair_kernel<4, kTier, true, false>);
  return ell_k == 8 ? go(whatif_repair_kernel<8, kTier, false, false>)
                    : go(whatif_repair_kernel<4, kTier, false, false>);
}

// Which tiers a run launches and which queue each drains; the one place that
// knows it (the back launch and repair_slot_queue both read it). The seed
// fills queue 0; a tier that runs moves what outgrows it to the next queue.
struct TierPlan {
  bool t1;            // tier 1 exists: its LDS state is smaller than tier 2's
  bool t2;            // tier 2 runs (not with skip_large behind a tier 1)
  uint32_t q2, qs;    // the queues tier 2 and the slot tier drain (tier 1: queue 0)
  uint32_t sa, se;    // tier 1's caps
  size_t lds1, lds2;  // LDS bytes of tiers 1 and 2
};

TierPlan tier_plan(const RepairArgs& a) {
  TierPlan p{};
  p.lds1 = tier1_lds(a, &p.sa, &p.se);
  p.lds2 = repair_lds_bytes(a.n_nodes, a.cap_a, a.cap_e);
  p.t1 = p.lds1 < p.lds2;
  // skip_large: the slot tier (and the full searches) take tier 1's overflow
  p.t2 = !(a.skip_large && p.t1);
  p.q2 = p.t1 ? 1u : 0u;  // without the small tier, tier 2 drains queue 0 itself
  p.qs = p.t2 ? p.q2 + 1u : p.q2;
  return p;
}

}  // namespace

hipError_t launch_repair_back_split(const RepairArgs& a, uint32_t ell_k, size_t lds_limit, hipStream_t s,
                                    hipStream_t s3, hipEvent_t mid) {
  if (a.n_req == 0) return hipSuccess;
  if (ell_k != 4 && ell_k != 8) return hipErrorInvalidValue;
  const TierPlan p = tier_plan(a);
  hipError_t e = hipSuccess;
  if (p.t1) {
    e = launch_tier<kWhatifTierSmall>(a, ell_k, tier_grid(a, lds_limit, p.lds1, 16), 128, p.lds1, s, p.sa, p.se, 0u);
    if (e != hipSuccess) return e;
  }
  if (p.t2) {
    e = launch_tier<kWhatifTierLarge>(a, ell_k, tier_grid(a, lds_limit, p.lds2, 8), 256, p.lds2, s, a.cap_a, a.cap_e,
                                      p.q2);
    if (e != hipSuccess) return e;
  }
  if (a.n_slots == 0) return e;
  if (s3 != s) {
    if ((e = hipEventRecord(mid, s)) != hipSuccess || (e = hipStreamWaitEvent(s3, mid, 0)) != hipSuccess) return e;
  }
  return launch_tier<kWhatifTierSlot>(a, ell_k, a.n_slots, kSlotBlock, 0, s3, a.n_nodes, a.n_recs, p.qs);
}

uint32_t repair_slot_queue(const RepairArgs& a) { return tier_plan(a).qs; }

namespace {

// ---- row digests (verification of whole batches) ---------------------------
// digest(row) = sum over v of mix(v, dist[v], nh[v][0..words)) mod 2^64: an
// order-free sum of a strong per-node hash, so equal rows give equal digests
// however they were produced, and one digest per row checks a batch whose rows
// do not fit the host (C4: 262,144 rows of 50,000 nodes). tests/helpers.py
// row_digest restates it in numpy.
__device__ inline uint64_t fmix64(uint64_t z) {
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__global__ void __launch_bounds__(256) row_digest_kernel(const uint32_t* __restrict__ dist,
                                                         const uint32_t* __restrict__ nh, uint32_t words,
                                                         uint32_t n, unsigned long long* __restrict__ out) {
  const size_t row = blockIdx.x;
  const uint32_t* d = dist + row * n;
  const uint32_t* m = nh + row * static_cast<size_t>(n) * words;
  uint64_t acc = 0;
  for (uint32_t v = threadIdx.x; v < n; v += blockDim.x) {
    uint64_t h = fmix64(static_cast<uint64_t>(v) * 0x9E3779B97F4A7C15ull + d[v]);
    for (uint32_t k = 0; k < words; ++k)
      h = fmix64(h ^ (static_cast<uint64_t>(m[static_cast<size_t>(v) * words + k]) +
                      static_cast<uint64_t>(k) * 0xC2B2AE3D27D4EB4Full));
    acc += h;
  }
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t lo = static_cast<uint32_t>(__shfl_xor(static_cast<int>(acc), o));
    const uint32_t hi = static_cast<uint32_t>(__shfl_xor(static_cast<int>(acc >> 32), o));
    acc += (static_cast<uint64_t>(hi) << 32) | lo;
  }
  __shared__ uint64_t part[4];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) out[row] = part[0] + part[1] + part[2] + part[3];
}

}  // namespace

hipError_t launch_row_digest(const uint32_t* dist, const uint32_t* nh, uint32_t words, uint32_t n,
                             uint32_t rows, uint64_t* out, hipStream_t s) {
  if (rows == 0) return hipSuccess;
  hipLaunchKernelGGL(row_digest_kernel, dim3(rows), dim3(256), 0, s, dist, nh, words, n,
                     reinterpret_cast<unsigned long long*>(out));
  return hipGetLastError();
}

}  // namespace orh
