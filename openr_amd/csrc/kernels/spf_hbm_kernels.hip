// SPF kernel, general metrics: HBM frontier relaxation with fused first hops
// (kGlobalNh).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spf_device.h"
#include "spf_launch.h"

namespace orh {

// ---------------------------------------------------------------------------
// phase 1c': HBM frontier relaxation with fused first hops
// ---------------------------------------------------------------------------
// The two-phase scheme derives NH(v) from the rows of the source's
// neighbours; for a batch whose neighbour rows are not sources themselves
// (what-if SPFs, KSP2 k=2 re-runs, a subset of sources) that multiplies the
// searches by 1 + deg(s). Here the search carries the closed form directly:
// each node has a 64-bit label {dist (hi), first-hop mask (lo)} in HBM, and a
// relaxation from v offers u the candidate {d(v) + w, v == src ? bit(u) :
// nh(v)}. Labels merge in a lattice: a smaller distance replaces, an equal
// one ORs the masks; any change re-queues u (near if below the threshold,
// else far). A candidate whose distance equals d*(u) comes from a predecessor
// whose distance is already final, so stale bits never survive: the fixpoint
// is exactly (d*, NH) of SURVEY.md Appendix A.1. Used when every source has
// at most 32 distinct neighbours (one mask word).
//
// The far set also tracks a lower bound of its distances (LDS atomicMin on
// every far push, recomputed exactly while promoting), so advancing the
// threshold costs one pass over the far nodes instead of two.

// Expand frontier nodes vs[0..c) of one row: the group's record, label and
// neighbour-label loads are in flight together (one round trip per stage for
// the group instead of per node), then merge(u, nd, cnh, cl) runs per live
// out-edge with u's label cl as loaded.
// label access: {dist (hi), first-hop mask (lo)} in a u64, or the distance
// alone in a u32 (dist-only searches: KSP2 rows feed traces, not first hops)
__device__ inline uint32_t lab_dist(unsigned long long l) { return static_cast<uint32_t>(l >> 32); }
__device__ inline uint32_t lab_dist(uint32_t l) { return l; }
__device__ inline uint32_t lab_nh(unsigned long long l) { return static_cast<uint32_t>(l); }
__device__ inline uint32_t lab_nh(uint32_t) { return 0u; }

struct NoPre {
  __device__ void operator()(uint32_t) const {}
};
// pre(bound): called once the group's records are in, before any merge, with
// the most pushes the group can make (its records, continuation lists
// included); a caller that passes one calls expand_group from every lane
// (c = 0 included), so pre runs with the whole wave active
// kDrain: the row's drained nodes (s.drn, what-if jobs) are no transit either
template <int K, int G, typename L, bool kDrain, typename Merge, typename Pre = NoPre>
__device__ __forceinline__ void expand_group(const SpfArgs& a, const Src& s, L* lab,
                                             const uint32_t (&vs)[G], int c, Merge& merge,
                                             Pre&& pre = Pre{}) {
  constexpr bool kNh = sizeof(L) == 8;
  uint2 rec[G][K];
  L lv[G];
  uint32_t lk[G][K];  // link ids (ignore sets), loaded with the records
#pragma unroll
  for (int g = 0; g < G; ++g) {
    if (g >= c) break;
    load_recs<K>(a, vs[g], rec[g]);
#pragma unroll
    for (int j = 0; j < K; ++j) lk[g][j] = s.n_ign ? a.link[vs[g] * K + j] : 0u;
    lv[g] = __hip_atomic_load(&lab[vs[g]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  {
    uint32_t bound = 0;
#pragma unroll
    for (int g = 0; g < G; ++g)
      if (g < c) bound += K + ((rec[g][K - 1].x & ORH_REC_CONT) ? rec[g][K - 1].y : 0u);
    pre(bound);
  }
  L cl[G][K];
  bool ok[G][K];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    bool transit = g < c && (vs[g] == s.node || !(rec[g][0].x & ORH_REC_ROW_OVL));
    if constexpr (kDrain) transit = transit && !(s.n_drn && vs[g] != s.node && drained(s.drn, s.n_drn, vs[g]));
#pragma unroll
    for (int j = 0; j < K; ++j) {
      ok[g][j] = transit && live_link(s, rec[g][j], lk[g][j]);
      if (ok[g][j])
        cl[g][j] = __hip_atomic_load(&lab[rec[g][j].x & ORH_REC_COL_MASK], __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_AGENT);
    }
  }
#pragma unroll
  for (int g = 0; g < G; ++g) {
    if (g >= c) break;
    const uint32_t v = vs[g];
    if (v != s.node && (rec[g][0].x & ORH_REC_ROW_OVL)) continue;  // no transit
    if constexpr (kDrain)
      if (s.n_drn && v != s.node && drained(s.drn, s.n_drn, v)) continue;  // drained: no transit
    const uint32_t dv = lab_dist(lv[g]);
    const uint32_t nhv = lab_nh(lv[g]);
    const bool from_src = kNh && v == s.node;
#pragma unroll
    for (int j = 0; j < K; ++j) {
      if (!ok[g][j]) continue;
      const uint2 r = rec[g][j];
      merge(r.x & ORH_REC_COL_MASK, dv + (a.use_link_metric ? r.y : 1u),
            from_src ? (1u << a.rank_out[v * K + j]) : nhv, cl[g][j]);
    }
    const uint2 last = rec[g][K - 1];
    if (last.x & ORH_REC_CONT) {
      const uint32_t start = last.x & ORH_REC_COL_MASK;
      for (uint32_t q = 0; q < last.y; ++q) {
        const uint2 r = a.recs[start + q];
        if (!live(a, s, r, start + q)) continue;
        const uint32_t u = r.x & ORH_REC_COL_MASK;
        merge(u, dv + (a.use_link_metric ? r.y : 1u), from_src ? (1u << a.rank_out[start + q]) : nhv,
              __hip_atomic_load(&lab[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
      }
    }
  }
}

// The search is asynchronous: within a bucket no barrier separates relaxation
// rounds. A thread claims the near nodes of its own words (atomicExch of the
// word; others only set bits) as soon as they appear and expands them; the
// bucket ends when s_work, the count of queued plus claimed-but-unexpanded
// near nodes, reaches zero. A push counts itself
// before its bit becomes visible and an expansion uncounts its nodes after
// its pushes, so the count never undercounts: zero means no near work exists
// or can appear, and every wave leaves the loop on the same condition. The
// lattice fixpoint does not depend on the order relaxations run in, so the
// result is bit for bit that of a round-synchronous search (a barrier between
// rounds); what goes away is the per-round barrier that held every wave to
// the slowest one (the C4 WAN runs about a hundred near rounds per search:
// the C4 what-if 2.39 -> 2.05 ms, profiles/r02/p_hbm_async_ab.txt).
// kDrain (what-if jobs with drained nodes, a.drain_ptr set): the row's drain
// set counts as overloaded; the other launches run the instantiation without
template <int K, bool kNh, bool kDrain>
__global__ __launch_bounds__(1024) void spf_global_nh_async_kernel(SpfArgs a) {
  typedef typename std::conditional<kNh, unsigned long long, uint32_t>::type L;
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  __shared__ uint32_t s_work;
  __shared__ uint32_t s_min[2];
  const uint32_t N = a.n_nodes;
  const uint32_t NB = (N + 31) >> 5;
  const uint32_t tid = threadIdx.x, nthr = blockDim.x;
  if (a.row_list && blockIdx.x >= *a.row_count) return;
  const uint32_t row = a.row_list ? a.row_list[blockIdx.x] : blockIdx.x;
  constexpr L kInfLabel = kNh ? static_cast<L>(0xFFFFFFFF00000000ull) : static_cast<L>(kInf);
  constexpr int G = K <= 4 ? 4 : 2;
  __shared__ uint32_t s_nign;
  uint32_t* near = lds;
  uint32_t* far = lds + NB;
  if (a.row_mask && !a.row_mask[row]) return;  // repaired elsewhere (whole workgroup)
  Src s(a, row);
  if constexpr (kDrain) {
    s.drn = a.drain_nodes + a.drain_ptr[row];
    s.n_drn = a.drain_ptr[row + 1] - a.drain_ptr[row];
  }
  L* lab = reinterpret_cast<L*>(a.labels) + static_cast<size_t>(a.row_list ? blockIdx.x : row) * N;
  // the plan's third bitmap holds the ignore filter: FW words, a power of two
  // <= 256, and the set's real length (fixed-stride lists end in ~0u padding,
  // e.g. KSP2's k = 2 rows)
  uint32_t* filt = lds + 2 * NB;
  uint32_t FW = 1;
  while (2 * FW <= min(NB, 256u)) FW *= 2;
  const uint32_t fshift = 32u - (5u + static_cast<uint32_t>(__builtin_ctz(FW)));

  for (uint32_t i = tid; i < 2 * NB; i += nthr) lds[i] = 0u;
  if (s.n_ign)
    for (uint32_t i = tid; i < FW; i += nthr) filt[i] = 0u;
  for (uint32_t i = tid; i < N; i += nthr) lab[i] = kInfLabel;
  if (tid < 2) s_min[tid] = kInf;
  if (tid == 0) s_nign = 0u;
  __syncthreads();
  if (s.n_ign) {
    for (uint32_t i = tid; i < s.n_ign; i += nthr) {
      const uint32_t l = s.ign[i];
      if (l == 0xFFFFFFFFu) continue;
      atomicAdd(&s_nign, 1u);
      const uint32_t h = ign_hash(l, fshift);
      atomicOr(&filt[h >> 5], 1u << (h & 31u));
    }
    __syncthreads();
    s.n_ign = s_nign;  // sorted: the real entries come first
    s.filt = filt;
    s.fshift = fshift;
  }
  if (tid == 0) {
    lab[s.node] = static_cast<L>(0);
    near[s.node >> 5] = 1u << (s.node & 31u);
    s_work = 1u;
  }
  __syncthreads();

  const uint32_t delta = a.delta;
  uint32_t T = delta;
  uint32_t mpar = 0;
  for (;;) {
    uint32_t far_min = kInf;
    uint32_t newq = 0;  // pushes of the current group that queued a node
    auto merge = [&](uint32_t u, uint32_t nd, uint32_t cnh, L cl) {
      if constexpr (kNh) {
        for (;;) {
          const uint32_t cd = static_cast<uint32_t>(cl >> 32);
          if (nd > cd) return;
          const unsigned long long nl = nd < cd
              ? ((static_cast<unsigned long long>(nd) << 32) | cnh)
              : (cl | cnh);
          if (nl == cl) return;
          const unsigned long long old = atomicCAS(&lab[u], cl, nl);
          if (old == cl) break;
          cl = old;
        }
      } else {  // distance alone: a strict decrease re-queues
        (void)cnh;
        if (nd >= cl) return;
        if (nd >= atomicMin(&lab[u], nd)) return;
      }
      const uint32_t bit = 1u << (u & 31u);
      if (nd < T) {
        const uint32_t old = atomicOr(&near[u >> 5], bit);
        atomicAnd(&far[u >> 5], ~bit);
        newq += (old & bit) ? 0u : 1u;  // reserved by the wave
      } else {
        atomicOr(&far[u >> 5], bit);
        far_min = min(far_min, nd);
      }
    };
    uint32_t w = tid, bits = 0, wbase = 0;
    for (;;) {
      uint32_t vs[G];
      int c = 0;
      while (c < G) {
        while (!bits && w < NB) {
          bits = __hip_atomic_load(&near[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          if (bits) bits = atomicExch(&near[w], 0u);  // at least the bits seen: only we clear
          wbase = w * 32;
          w += nthr;
        }
        if (!bits) break;
        vs[c++] = wbase + __builtin_ctz(bits);
        bits &= bits - 1;
      }
      if (!bits && w >= NB) w = tid;  // words exhausted: rescan them next time
      if (__builtin_amdgcn_ballot_w64(c > 0) == 0ull) {
        // the whole wave found nothing: done once nothing is queued or claimed
        const uint32_t pending = __builtin_amdgcn_readfirstlane(
            __hip_atomic_load(&s_work, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
        if (pending == 0u) break;
        __builtin_amdgcn_s_sleep(1);
        continue;
      }
      // the work count per wave, as in spf_lds16_kernel: the group's
      // possible pushes reserved before its merges, the unused ones and
      // the expanded nodes returned after them
      uint32_t bound = 0;
      newq = 0;
      expand_group<K, G, L, kDrain>(a, s, lab, vs, c, merge, [&](uint32_t b) {
        bound = b;
        const uint32_t r = wave_sum(b);
        if ((tid & 63u) == 0u && r) atomicAdd(&s_work, r);
      });
      const uint32_t back = wave_sum(c > 0 ? bound - newq + static_cast<uint32_t>(c) : 0u);
      if ((tid & 63u) == 0u && back) atomicSub(&s_work, back);
    }
    {
      const uint32_t fm = wave_min(far_min);
      if ((tid & 63u) == 0 && fm != kInf) atomicMin(&s_min[mpar], fm);
    }
    __syncthreads();  // bucket drained everywhere; far bound folded
    const uint32_t m = s_min[mpar];
    if (m == kInf) break;  // far set empty: done (every thread read the same value)
    T = m + delta;
    const uint32_t npar = mpar ^ 1u;
    if (tid == 0) s_min[npar] = kInf;
    __syncthreads();
    uint32_t local_min = kInf, promoted = 0;
    for (uint32_t w2 = tid; w2 < NB; w2 += nthr) {
      uint32_t fb = far[w2], promote = 0u;
      for (uint32_t q = fb; q; q &= q - 1) {
        const uint32_t b = __builtin_ctz(q);
        const uint32_t d = lab_dist(__hip_atomic_load(&lab[w2 * 32 + b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        if (d < T) promote |= 1u << b;
        else local_min = min(local_min, d);
      }
      if (promote) {
        far[w2] = fb & ~promote;
        near[w2] = promote;  // the near set is empty between buckets
        promoted += __builtin_popcount(promote);
      }
    }
    const uint32_t pr = wave_sum(promoted);
    if ((tid & 63u) == 0u && pr) atomicAdd(&s_work, pr);
    const uint32_t wm = wave_min(local_min);
    if ((tid & 63u) == 0 && wm != kInf) atomicMin(&s_min[npar], wm);
    mpar = npar;
    __syncthreads();
  }
  __syncthreads();
  uint32_t* od = a.out_dist + static_cast<size_t>(row) * N;
  uint32_t* on = kNh ? a.out_nh + static_cast<size_t>(row) * N * a.words : nullptr;
  for (uint32_t i = tid; i < N; i += nthr) {
    const L l = __hip_atomic_load(&lab[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_nontemporal_store(lab_dist(l), &od[i]);
    if constexpr (kNh) {
      if (a.words == 1) {
        __builtin_nontemporal_store(lab_nh(l), &on[i]);
      } else {
        on[static_cast<size_t>(i) * a.words] = lab_nh(l);
        for (uint32_t k = 1; k < a.words; ++k) on[static_cast<size_t>(i) * a.words + k] = 0u;
      }
    }
  }
}

template <int K>
static hipError_t launch_global_nh_k(const SpfPlan& plan, const SpfArgs& a, uint32_t n_rows, hipStream_t s) {
  if (a.dist_only) {  // distances alone (u32 labels), no first-hop rows
    if (a.drain_ptr) return hipErrorInvalidValue;  // drains come with first hops (what-if jobs)
    return launch(spf_global_nh_async_kernel<K, false, false>, a, n_rows, plan.block, plan.lds_bytes, s);
  }
  if (a.drain_ptr)
    return launch(spf_global_nh_async_kernel<K, true, true>, a, n_rows, plan.block, plan.lds_bytes, s);
  return launch(spf_global_nh_async_kernel<K, true, false>, a, n_rows, plan.block, plan.lds_bytes, s);
}

hipError_t launch_global_nh(const SpfPlan& plan, const SpfArgs& a, uint32_t n_rows, hipStream_t s) {
  return plan.ell_k == 8 ? launch_global_nh_k<8>(plan, a, n_rows, s) : launch_global_nh_k<4>(plan, a, n_rows, s);
}

}  // namespace orh
