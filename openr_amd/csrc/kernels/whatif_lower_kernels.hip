// What-if metric lowers: stage 2 of a request that lowers link metrics (costs
// a link back in, Link::setMetricFromNode, LinkState.cpp:640-710) (gfx950).
//
// Stage 1 is the repair of whatif_kernels.hip, unchanged: it leaves the row R1
// of the request's ignored links, drained nodes and raised metrics, exact for
// that graph G1. Every change stage 1 knows only weakens relaxations. A lowered
// metric strengthens one: distances fall, which nodes change depends on the
// new distances, and a new equal-cost path widens first-hop masks down the
// DAG without moving a distance. whatif_lower_kernel turns R1, in place, into
// the exact row of G2 = G1 with the lowered records, one workgroup per request
// that stages an effective lower.
//
// "Transit" below: the node is the request's source, or neither overloaded nor
// drained in this request. An ignored link is skipped everywhere (ignore wins
// over a lower, as over a raise). A record weighs what the request's sorted
// (record, weight) list says - its lowered value, else its raised one - and
// its own weight otherwise.
//
//   1 distances  seeds: heads v of lowered records p -> v with p reached and
//                transit and d(p) + w' < d(v). A label-correcting wave: a node
//                whose distance fell relaxes its live out-records if it is
//                transit; a smaller candidate replaces the head's distance
//                (atomicMin on the row) and queues the head again. C = the
//                nodes whose distance fell.
//   2 mask set   M = C plus the heads of lowered records that are now tight
//                (d(p) + w' == d(v), p reached and transit), closed under the
//                records tight in the NEW distances and weights out of
//                transit nodes.
//   3 labels     relabel (whatif_device.h), the meet-fixpoint the repair runs
//                over its A: the mask of v in M is the OR over its tight
//                predecessors under G2; the source offers v's own bit, a
//                predecessor outside M its R1 mask, one inside M its current
//                label. Distances come out as step 1 left them.
//
// Why this is exact. A node y outside M kept its distance (C is in M). No
// tight predecessor of y is in M, or the closure had added y. No lowered
// record into y is tight, or y were a seed of M. A predecessor that was tight
// and whose distance fell would have pulled y into C. A predecessor that was
// not tight cannot have become tight without its distance falling or its
// record being lowered, both excluded. So y has the same tight predecessors
// with the same labels (by induction on d), and its entry of R1 stands.
// Inside M, positive metrics make the tight-predecessor graph acyclic, so the
// mask fixpoint is unique and equals the fresh search's. Step 1 is
// Bellman-Ford from a valid upper bound: R1 is exact for G1 and G1 -> G2 only
// lowers weights, so every d is the length of a real G2 path throughout, and
// at the fixpoint no record can relax, which makes it the G2 distance.
//
// State. The row lives in global memory and belongs to the workgroup alone;
// waves hand it to each other through bar() (vector stores drained, then the
// barrier), and an agent-scope acquire after each wave round refreshes the
// CU's L1 behind the atomics. The frontiers of steps 1 and 2 are bitmaps over
// the nodes, which cannot overflow; M's node list and step 3's labels and
// edges take the repair's LDS layout up to the caps. A request whose M or
// edge list outgrows them leaves M marked in the row itself - a zero mask on
// a reached node that is not the source, which no finished row has - and
// joins a queue; the second launch (kSlot) reads M back from the marks and
// runs step 3 with its state in one of the run's global slots, which are
// sized for the whole graph and free once the run's slot tier has ended.
//
// SHARE_BASE: a request with an effective lower owns its row. Where stage 1
// left it at tier 0 the copy kernel skipped it, so this kernel copies the base
// row first (the seed test tells: cut_tight over the request's cuts).

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "spf_device.h"
#include "whatif_device.h"
#include "whatif_kernels.h"

namespace orh {
namespace {

constexpr uint32_t kLowerBlock = 256, kLowerSlotBlock = 1024;
// counters of the lower pass (RepairArgs::counters): the slot queue's length
// and its next index to claim
constexpr uint32_t kLowQueueLen = 6, kLowQueueNext = 7;

// what a request of the lower pass reads besides the row
template <bool kDrain>
struct LowerReq {
  uint32_t r, s;
  uint32_t *od, *on;
  const uint32_t* ign;
  uint32_t n_ign;
  const uint32_t* drn;
  uint32_t n_drn;
  const uint2* wl;
  uint32_t n_wl;
  __device__ LowerReq(const RepairArgs& a, const LowerArgs& l, uint32_t j) {
    r = l.req[j];
    s = a.srcs[r];
    od = a.out_dist + static_cast<size_t>(r) * a.n_nodes;
    on = a.out_nh + static_cast<size_t>(r) * a.n_nodes;
    ign = a.ign + a.ign_ptr[r];
    n_ign = a.ign_ptr[r + 1] - a.ign_ptr[r];
    drn = nullptr;
    n_drn = 0;
    if constexpr (kDrain) {
      drn = a.drn + a.drn_ptr[r];
      n_drn = a.drn_ptr[r + 1] - a.drn_ptr[r];
    }
    wl = l.wl + l.wl_ptr[j];
    n_wl = l.wl_ptr[j + 1] - l.wl_ptr[j];
  }
  __device__ bool transit(const RepairArgs& a, uint32_t v) const {
    if (v == s) return true;
    if (a.ovl[v]) return false;
    if constexpr (kDrain)
      if (n_drn && drained(drn, n_drn, v)) return false;
    return true;
  }
  __device__ bool skipped(const RepairArgs& a, uint32_t q) const { return n_ign && ignored(ign, n_ign, a.link[q]); }
};

// every set bit of the bitmap word w at index i: f(node)
template <class F>
__device__ inline void for_bits(uint32_t w, uint32_t i, F&& f) {
  while (w) {
    const uint32_t b = static_cast<uint32_t>(__builtin_ctz(w));
    w &= w - 1u;
    f(i * 32u + b);
  }
}

// Steps 1 and 2 and, when M fits the caps, step 3 of request l.req[j], state
// in LDS. Returns |M|, or ~0u with M marked in the row (zero masks).
// st.bits, cur and nxt are all zero on entry; cur and nxt on return too.
template <int K, bool kDrain>
__device__ uint32_t lower_one(const RepairArgs& a, const LowerArgs& l, uint32_t j, const RepairState& st,
                              uint32_t* cur, uint32_t* nxt, uint32_t* s_cnt, uint32_t* s_ecnt, uint32_t* s_ovf,
                              uint32_t* s_more, uint32_t* s_flag) {
  const uint32_t N = a.n_nodes, NB = (N + 31) / 32;
  const uint32_t tid = threadIdx.x, B = blockDim.x;
  const LowerReq<kDrain> q(a, l, j);
  uint32_t* od = q.od;
  uint32_t* on = q.on;
  uint32_t* bits = st.bits;
  uint32_t* alist = st.alist;

  if (tid == 0) {
    *s_cnt = 0u;
    *s_ecnt = 0u;
    *s_ovf = 0u;
    *s_more = 0u;
  }
  if (tid < 3) s_flag[tid] = 0u;
  bar();
  if (a.share_base) {  // a row stage 1 left to the base row was never copied
    const uint32_t* bd = a.base_dist + static_cast<size_t>(a.base_row[q.r]) * N;
    const uint32_t* bn = a.base_nh + static_cast<size_t>(a.base_row[q.r]) * N;
    for (uint32_t c = a.cut_ptr[q.r] + tid; c < a.cut_ptr[q.r + 1]; c += B)
      if (cut_tight(a, bd, q.s, a.cuts[c])) *s_more = 1u;
    bar();
    const bool copied = *s_more != 0u;
    bar();
    if (tid == 0) *s_more = 0u;
    if (!copied)
      for (uint32_t v = tid; v < N; v += B) {
        od[v] = bd[v];
        on[v] = bn[v];
      }
    bar();
  }

  // M membership: bitmap (complete whatever the list holds) and node list
  auto add = [&](uint32_t u) {
    const uint32_t bit = 1u << (u & 31u);
    if (atomicOr(&bits[u >> 5], bit) & bit) return false;
    const uint32_t k = atomicAdd(s_cnt, 1u);
    if (k < l.cap_a) alist[k] = u;
    else *s_ovf = 1u;
    return true;
  };
  auto queue = [&](uint32_t u) {
    atomicOr(&nxt[u >> 5], 1u << (u & 31u));
    *s_more = 1u;
  };
  // a candidate distance for u: the row's entry falls, u joins C and the wave
  auto relax = [&](uint32_t u, uint64_t cand) {
    if (cand >= od[u]) return;  // a stale entry is an older, larger one: a filter only
    if (static_cast<uint32_t>(cand) < atomicMin(&od[u], static_cast<uint32_t>(cand))) {
      add(u);
      queue(u);
    }
  };
  // next round of a frontier loop: did anyone queue a node? then cur <- nxt
  auto advance = [&]() {
    bar();
    const bool more = *s_more != 0u;
    bar();
    if (!more) return false;
    if (tid == 0) *s_more = 0u;
    for (uint32_t i = tid; i < NB; i += B) {
      cur[i] = nxt[i];
      nxt[i] = 0u;
    }
    bar();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // the row's entries behind the atomics
    return true;
  };

  // 1: distances. Seeds, then the label-correcting wave
  const uint32_t c0 = l.rec_ptr[j], c1 = l.rec_ptr[j + 1];
  for (uint32_t c = c0 + tid; c < c1; c += B) {
    const uint4 x = l.recs[c];  // (tail, head, record tail -> head, lowered weight)
    if ((a.recs[x.z].x & ORH_REC_SKIP) || q.skipped(a, x.z)) continue;
    const uint32_t dp = od[x.x];
    if (dp == kInfD || !q.transit(a, x.x)) continue;
    relax(x.y, static_cast<uint64_t>(dp) + x.w);
  }
  while (advance()) {
    for (uint32_t i = tid; i < NB; i += B)
      for_bits(cur[i], i, [&](uint32_t v) {
        if (!q.transit(a, v)) return;  // nearer, but nothing below it moves
        const uint64_t dv = __hip_atomic_load(&od[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for_records<K>(a.recs, v, [&](const uint2& rec, uint32_t e) {
          if (q.skipped(a, e)) return;
          relax(rec.x & ORH_REC_COL_MASK, dv + raised(q.wl, q.n_wl, e, rec.y));
        });
      });
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");

  // 2: M = C, the lowered heads now tight, and the closure under records
  // tight in the new distances out of transit nodes
  for (uint32_t c = c0 + tid; c < c1; c += B) {
    const uint4 x = l.recs[c];
    if ((a.recs[x.z].x & ORH_REC_SKIP) || q.skipped(a, x.z)) continue;
    const uint32_t dp = od[x.x];
    if (dp == kInfD || !q.transit(a, x.x)) continue;
    if (static_cast<uint64_t>(dp) + x.w == od[x.y]) add(x.y);
  }
  bar();
  if (*s_cnt == 0u) return 0u;  // no lower takes effect: R1 stands
  for (uint32_t i = tid; i < NB; i += B) nxt[i] = bits[i];  // the first frontier is M itself
  if (tid == 0) *s_more = 1u;
  while (advance()) {
    for (uint32_t i = tid; i < NB; i += B)
      for_bits(cur[i], i, [&](uint32_t v) {
        if (!q.transit(a, v)) return;  // re-derived, not expanded
        const uint64_t dv = od[v];
        for_records<K>(a.recs, v, [&](const uint2& rec, uint32_t e) {
          const uint32_t u = rec.x & ORH_REC_COL_MASK;
          if ((bits[u >> 5] & (1u << (u & 31u))) || q.skipped(a, e)) return;
          if (dv + raised(q.wl, q.n_wl, e, rec.y) == od[u] && add(u)) queue(u);
        });
      });
  }
  for (uint32_t i = tid; i < NB; i += B) cur[i] = 0u;  // the last frontier (nxt is zero)
  bar();

  // 3: labels, here when M and its edges fit
  uint32_t n = ~0u;
  if (*s_ovf == 0u)
    n = relabel<K, kDrain, true>(a, q.r, st, l.cap_e, *s_cnt, od, on, q.wl, q.n_wl, s_ecnt, s_ovf, s_flag);
  if (n != ~0u) return n;
  // M outgrew the caps: left as zero masks for the slot pass
  for (uint32_t i = tid; i < NB; i += B) for_bits(bits[i], i, [&](uint32_t v) { on[v] = 0u; });
  return ~0u;
}

// Step 3 of a queued request, state in a global slot with whole-graph caps: M
// read back from the row's marks. Returns |M|.
template <int K, bool kDrain>
__device__ uint32_t lower_marked(const RepairArgs& a, const LowerArgs& l, uint32_t j, const RepairState& st,
                                 uint32_t* s_cnt, uint32_t* s_ecnt, uint32_t* s_ovf, uint32_t* s_flag) {
  const uint32_t N = a.n_nodes;
  const uint32_t tid = threadIdx.x, B = blockDim.x;
  const LowerReq<kDrain> q(a, l, j);
  if (tid == 0) {
    *s_cnt = 0u;
    *s_ecnt = 0u;
    *s_ovf = 0u;
  }
  if (tid < 3) s_flag[tid] = 0u;
  bar();
  for (uint32_t v = tid; v < N; v += B)
    if (v != q.s && q.od[v] != kInfD && q.on[v] == 0u) {
      atomicOr(&st.bits[v >> 5], 1u << (v & 31u));
      st.alist[atomicAdd(s_cnt, 1u)] = v;  // at most N entries: the slot holds them
    }
  bar();
  return relabel<K, kDrain, true>(a, q.r, st, a.n_recs, *s_cnt, q.od, q.on, q.wl, q.n_wl, s_ecnt, s_ovf, s_flag);
}

// kSlot false: workgroup b takes the requests b, b + grid, ... of the run's
// lower list, state in LDS; what outgrows it joins l.queue. kSlot true: one
// global slot per workgroup drains that queue (its length is fixed before this
// launch by the first).
template <int K, bool kDrain, bool kSlot>
__global__ __launch_bounds__(kSlot ? kLowerSlotBlock : kLowerBlock)
void whatif_lower_kernel(RepairArgs a, LowerArgs l) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  __shared__ uint32_t s_cnt, s_ecnt, s_ovf, s_more, s_req;
  __shared__ uint32_t s_flag[3];
  const uint32_t N = a.n_nodes, NB = (N + 31) / 32;
  const uint32_t tid = threadIdx.x, B = blockDim.x;
  const uint32_t cap_a = kSlot ? N : l.cap_a, cap_e = kSlot ? a.n_recs : l.cap_e;
  uint32_t* base = kSlot ? reinterpret_cast<uint32_t*>(a.slot_mem + blockIdx.x * a.slot_bytes) : lds;
  const RepairState st(base, cap_a, cap_e);
  uint32_t* cur = st.bits + NB;  // LDS pass only: the frontier bitmaps behind the repair state
  uint32_t* nxt = cur + NB;
  for (uint32_t i = tid; i < (kSlot ? NB : 3u * NB); i += B) st.bits[i] = 0u;
  bar();
  // after a request: its info word, and the membership bitmap cleared (through
  // the node list when it holds all of M, else whole)
  auto finish = [&](uint32_t j, uint32_t n) {
    const uint32_t r = l.req[j];
    if (tid == 0) {
      if (n == ~0u) l.queue[atomicAdd(&a.counters[kLowQueueLen], 1u)] = j;
      else if (n && a.info) a.info[r] = kWhatifTierLowered | (((a.info[r] >> 3) + n) << 3);
    }
    const uint32_t cnt = s_cnt;
    bar();
    if (cnt > cap_a) {
      for (uint32_t i = tid; i < NB; i += B) st.bits[i] = 0u;
    } else {
      for (uint32_t k = tid; k < cnt; k += B) st.bits[st.alist[k] >> 5] = 0u;
    }
    bar();
  };
  if constexpr (kSlot) {
    const uint32_t len = a.counters[kLowQueueLen];
    for (;;) {
      if (tid == 0) {
        const uint32_t i = atomicAdd(&a.counters[kLowQueueNext], 1u);
        s_req = i < len ? l.queue[i] : ~0u;
      }
      bar();
      const uint32_t j = s_req;
      if (j == ~0u) break;
      finish(j, lower_marked<K, kDrain>(a, l, j, st, &s_cnt, &s_ecnt, &s_ovf, s_flag));
    }
  } else {
    for (uint32_t j = blockIdx.x; j < l.n_low; j += gridDim.x)
      finish(j, lower_one<K, kDrain>(a, l, j, st, cur, nxt, &s_cnt, &s_ecnt, &s_ovf, &s_more, s_flag));
  }
}

template <bool kSlot>
hipError_t launch_pass(const RepairArgs& a, const LowerArgs& l, uint32_t ell_k, uint32_t grid, size_t lds,
                       hipStream_t s) {
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kSlot ? kLowerSlotBlock : kLowerBlock), lds, s, a, l);
    return hipGetLastError();
  };
  if (a.drn_ptr)
    return ell_k == 8 ? go(whatif_lower_kernel<8, true, kSlot>) : go(whatif_lower_kernel<4, true, kSlot>);
  return ell_k == 8 ? go(whatif_lower_kernel<8, false, kSlot>) : go(whatif_lower_kernel<4, false, kSlot>);
}

}  // namespace

size_t lower_lds_bytes(uint32_t n_nodes, uint32_t cap_a, uint32_t cap_e) {
  return repair_lds_bytes(n_nodes, cap_a, cap_e) + 2 * static_cast<size_t>((n_nodes + 31) / 32) * 4;
}

hipError_t launch_lower(const RepairArgs& a, const LowerArgs& l, uint32_t ell_k, size_t lds_limit, hipStream_t s) {
  if (l.n_low == 0) return hipSuccess;
  if ((ell_k != 4 && ell_k != 8) || a.n_slots == 0) return hipErrorInvalidValue;
  const size_t lds = lower_lds_bytes(a.n_nodes, l.cap_a, l.cap_e);
  if (lds > lds_limit) return hipErrorInvalidValue;
  const uint32_t per_cu = static_cast<uint32_t>(std::min<size_t>(8, lds_limit / lds));
  const uint32_t grid = std::max<uint32_t>(1u, std::min<uint32_t>(l.n_low, a.n_cu * per_cu));
  const hipError_t e = launch_pass<false>(a, l, ell_k, grid, lds, s);
  if (e != hipSuccess) return e;
  return launch_pass<true>(a, l, ell_k, std::min(a.n_slots, l.n_low), 0, s);
}

}  // namespace orh
