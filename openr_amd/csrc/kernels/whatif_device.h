// Device helpers shared by the what-if repair kernels (whatif_kernels.hip) and
// the metric-lower pass behind them (whatif_lower_kernels.hip): the label
// lattice, the barrier discipline of state kept in global memory, the
// per-request weight list, the record walk, and the meet-fixpoint over a node
// set (relabel) that both passes end with.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spf_device.h"  // edge record flags, ignored(), drained()
#include "whatif_kernels.h"

namespace orh {
namespace {

constexpr uint32_t kInfD = 0xFFFFFFFFu;
constexpr unsigned long long kInfLab = 0xFFFFFFFF00000000ull;  // {dist = inf, mask = 0}

// lattice meet of a label and the candidate {d, nh}: a smaller distance
// replaces, an equal one ORs the mask
__device__ inline unsigned long long meet(unsigned long long l, uint64_t d, uint32_t nh) {
  if (d >= kInfD) return l;
  const uint32_t ld = static_cast<uint32_t>(l >> 32);
  if (d < ld) return (d << 32) | nh;
  if (d == ld) return l | nh;
  return l;
}

// workgroup barrier that first drains this wave's global stores: the repair
// state (and the mask row used as index map) lives in global memory in the
// slot pass, and other waves read it with plain loads after the barrier
__device__ inline void bar() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}

// the request's replaced weight of record `rec`, else w: (record, new weight)
// pairs sorted by record, a few entries; callers test n != 0 first
__device__ inline uint32_t raised(const uint2* rse, uint32_t n, uint32_t rec, uint32_t w) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    const uint2 x = rse[mid];
    if (x.x == rec) return x.y;
    if (x.x < rec) lo = mid + 1; else hi = mid;
  }
  return w;
}

// visit the live records of node v: ELL slots then the overflow list
template <int K, class F>
__device__ inline void for_records(const uint2* recs, uint32_t v, F&& f) {
  const uint2* slots = recs + static_cast<size_t>(v) * K;
  uint2 r[K];
#pragma unroll
  for (int j = 0; j < K; ++j) r[j] = slots[j];
#pragma unroll
  for (int j = 0; j < K; ++j)
    if (!(r[j].x & (ORH_REC_SKIP | ORH_REC_CONT))) f(r[j], static_cast<uint32_t>(v * K + j));
  if (r[K - 1].x & ORH_REC_CONT) {
    const uint32_t start = r[K - 1].x & ORH_REC_COL_MASK;
    for (uint32_t q = 0; q < r[K - 1].y; ++q) {
      const uint2 o = recs[start + q];
      if (!(o.x & ORH_REC_SKIP)) f(o, start + q);
    }
  }
}

// is the staged cut (tail, head, record tail -> head, 0) tight in the row bd
// of source s under the record's own weight, its tail a transit node?
__device__ inline bool cut_tight(const RepairArgs& a, const uint32_t* bd, uint32_t s, const uint4& cut) {
  const uint2 rec = a.recs[cut.z];
  if (rec.x & ORH_REC_SKIP) return false;  // link down: never on a path
  const uint32_t dx = bd[cut.x];
  if (dx == kInfD || (cut.x != s && a.ovl[cut.x])) return false;
  return static_cast<uint64_t>(dx) + (a.use_link_metric ? rec.y : 1u) == bd[cut.y];
}

// The repair state at `base` for the caps cap_a / cap_e (LDS, or a global
// slot with whole-graph caps):
//   labels u64[cap_a] | boundary labels u64[cap_a] | edges uint2[cap_e] |
//   edge ranges uint2[cap_a] | node list u32[cap_a] | membership bitmap u32[NB]
struct RepairState {
  unsigned long long* lab;
  unsigned long long* blab;
  uint2* edges;
  uint2* erange;
  uint32_t* alist;
  uint32_t* bits;
  __device__ RepairState(uint32_t* base, uint32_t cap_a, uint32_t cap_e) {
    lab = reinterpret_cast<unsigned long long*>(base);
    blab = lab + cap_a;
    edges = reinterpret_cast<uint2*>(blab + cap_a);
    erange = edges + cap_e;
    alist = reinterpret_cast<uint32_t*>(erange + cap_a);
    bits = alist + cap_a;
  }
};

// The labels of the n nodes of st.alist (their bits set in st.bits)
// re-derived and written into the request's row: a boundary label per node
// (the lattice meet over its predecessors outside the set, which offer their
// entries of the rows D / NH), then chaotic relaxation over the predecessor
// edges inside the set until no label changes. A predecessor that is the
// source offers the head's own bit (rank_out). An ignored link is skipped;
// a record weighs what the request's list wl says (kRaise), else its own
// weight. D / NH are the base rows in the repair, and the request's own row
// (whose entries outside the set stand) in the lower pass. Returns n, or ~0u
// when the edges outgrow cap_e (*s_ecnt and *s_ovf zero on entry; the mask row
// then holds list indices on the set).
template <int K, bool kDrain, bool kRaise>
__device__ inline uint32_t relabel(const RepairArgs& a, uint32_t r, const RepairState& st, uint32_t cap_e, uint32_t n,
                                   const uint32_t* D, const uint32_t* NH, const uint2* wl, uint32_t n_wl,
                                   uint32_t* s_ecnt, uint32_t* s_ovf, uint32_t* s_flag) {
  const uint32_t N = a.n_nodes;
  const uint32_t tid = threadIdx.x, B = blockDim.x;
  unsigned long long* lab = st.lab;
  unsigned long long* blab = st.blab;
  uint2* edges = st.edges;
  uint2* erange = st.erange;
  const uint32_t* alist = st.alist;
  const uint32_t* bits = st.bits;
  const uint32_t s = a.srcs[r];
  uint32_t* od = a.out_dist + static_cast<size_t>(r) * N;
  uint32_t* on = a.out_nh + static_cast<size_t>(r) * N;
  const uint32_t* ign = a.ign + a.ign_ptr[r];
  const uint32_t n_ign = a.ign_ptr[r + 1] - a.ign_ptr[r];
  const bool metric = a.use_link_metric != 0;
  const uint32_t* drn = nullptr;
  uint32_t n_drn = 0;
  if constexpr (kDrain) {
    drn = a.drn + a.drn_ptr[r];
    n_drn = a.drn_ptr[r + 1] - a.drn_ptr[r];
  }
  // the request's mask row doubles as the node -> list index map (rewritten below)
  for (uint32_t k = tid; k < n; k += B) on[alist[k]] = k;
  bar();

  // boundary labels from predecessors outside the set; edges from those inside
  auto pred = [&](const uint2& rec, uint32_t q, auto&& inside, auto&& outside) {
    if (n_ign && ignored(ign, n_ign, a.link[q])) return;
    const uint32_t p = rec.x & ORH_REC_COL_MASK;
    const uint32_t q2 = a.rev[q];
    const uint2 back = a.recs[q2];  // p -> v: p's metric and p's overload bit
    if (p != s && (back.x & ORH_REC_ROW_OVL)) return;
    if constexpr (kDrain)
      if (n_drn && p != s && drained(drn, n_drn, p)) return;
    uint32_t w = metric ? back.y : 1u;
    if constexpr (kRaise)
      if (n_wl) w = raised(wl, n_wl, q2, w);  // staged for metric jobs only
    if (bits[p >> 5] & (1u << (p & 31u))) inside(p, w);
    else outside(p, q2, w);
  };
  for (uint32_t k = tid; k < n; k += B) {
    const uint32_t v = alist[k];
    uint32_t cnt = 0;
    unsigned long long bl = kInfLab;
    for_records<K>(a.recs, v, [&](const uint2& rec, uint32_t q) {
      pred(rec, q, [&](uint32_t, uint32_t) { ++cnt; },
           [&](uint32_t p, uint32_t q2, uint32_t w) {
             const uint32_t dp = D[p];
             if (dp == kInfD) return;
             bl = meet(bl, static_cast<uint64_t>(dp) + w, p == s ? (1u << a.rank_out[q2]) : NH[p]);
           });
    });
    const uint32_t e0 = cnt ? atomicAdd(s_ecnt, cnt) : 0u;
    if (e0 + cnt > cap_e) {
      *s_ovf = 1u;
      cnt = 0;
    }
    uint32_t e = e0;
    if (cnt)
      for_records<K>(a.recs, v, [&](const uint2& rec, uint32_t q) {
        pred(rec, q, [&](uint32_t p, uint32_t w) { edges[e++] = make_uint2(on[p], w); },
             [](uint32_t, uint32_t, uint32_t) {});
      });
    erange[k] = make_uint2(e0, e0 + cnt);
    blab[k] = bl;
    lab[k] = kInfLab;
  }
  bar();
  if (*s_ovf) return ~0u;

  // chaotic relaxation inside the set until no label changes (labels only
  // descend in the lattice; a sweep that writes nothing proves the fixpoint)
  for (uint32_t it = 0;; ++it) {
    bool changed = false;
    for (uint32_t k = tid; k < n; k += B) {
      unsigned long long nl = blab[k];
      const uint2 er = erange[k];
      uint32_t e = er.x;
      for (; e + 4 <= er.y; e += 4) {  // four predecessor labels in flight
        uint2 ed[4];
        unsigned long long lj[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) ed[q] = edges[e + q];
#pragma unroll
        for (int q = 0; q < 4; ++q) lj[q] = lab[ed[q].x];
#pragma unroll
        for (int q = 0; q < 4; ++q) nl = meet(nl, (lj[q] >> 32) + ed[q].y, static_cast<uint32_t>(lj[q]));
      }
      for (; e < er.y; ++e) {
        const uint2 ed = edges[e];
        const unsigned long long lj = lab[ed.x];
        nl = meet(nl, (lj >> 32) + ed.y, static_cast<uint32_t>(lj));
      }
      if (nl != lab[k]) {
        lab[k] = nl;
        changed = true;
      }
    }
    const uint32_t par = it % 3u;
    if (changed) s_flag[par] = 1u;
    bar();
    const bool more = s_flag[par] != 0u;
    if (tid == 0) s_flag[(par + 2u) % 3u] = 0u;  // the previous sweep's flag, read before this barrier
    if (!more) break;
  }
  for (uint32_t k = tid; k < n; k += B) {
    const uint32_t v = alist[k];
    const unsigned long long l = lab[k];
    od[v] = static_cast<uint32_t>(l >> 32);
    on[v] = static_cast<uint32_t>(l);
  }
  return n;
}

}  // namespace
}  // namespace orh
