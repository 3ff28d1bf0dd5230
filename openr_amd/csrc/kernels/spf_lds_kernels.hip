// SPF kernels, general metrics, one search per CU with its labels in LDS: u16
// distances (spf_lds16_kernel) and {dist, first hops} labels (kLdsNh).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "spf_device.h"
#include "spf_launch.h"

namespace orh {

// ---------------------------------------------------------------------------
// phase 1c'': the asynchronous delta-stepping search with u16 distances in LDS
// ---------------------------------------------------------------------------
// Distances only (KSP2 searches): the async kernel above with its labels moved
// from HBM into LDS as u16 pairs (two nodes per word, lowered by
// compare-and-swap), so the 50k-node WAN of C4 (100 KB of distances + 12.5 KB
// of near / far bitmaps + a 16 KB spill table) keeps a whole search on one
// CU. Relaxation chains then pay LDS latency instead of a global atomic per
// hop; only the edge records (read-only, shared by every search,
// L2-resident) come from memory.
// A u16 entry holds distances 0..0xFFFD inline; 0xFFFF is unreached and
// 0xFFFE "spilled": the node's distance (>= 0xFFFE, the heavy-tailed metrics
// of C4 leave a few such nodes per row) sits in an LDS hash table keyed by
// node id. A spilled node that later gets an inline distance simply drops its
// table entry from use (inline < any spilled value). Only when the table is
// full is a candidate dropped; the row is then exact unless a node ends
// unreached (a dropped candidate exceeds every finite distance its node ends
// with, and a node whose distance needed the table stays unreached), so such
// a row is queued in ovf_rows for the HBM kernel (launch_spf_lds16).
constexpr uint32_t kSpillSlots = 2048, kSpillProbe = 64;
constexpr uint32_t kIgnLds = 1024;  // ignore sets up to this size are searched in LDS
constexpr uint32_t kD16Spill = 0xFFFEu, kD16None = 0xFFFFu;

// The bucket's work count s_work is one LDS word every thread updates: per
// lane, an add per push and a subtract per duplicate and per expanded group
// serialise on that one address. Here a wave reserves, before its group's
// merges, every push the group could make (its nodes' records) with one
// atomic, counts locally the pushes that queued a new node, and returns the
// rest together with its expanded nodes with one more (wave sums over DPP).
// The count still never undercounts: the reservation precedes the wave's
// near-bit updates in its LDS order, and the release follows them.
// A/B of the round-6 search knobs on the C4 batch (profiles/r06/j_ksp2_ab.txt,
// k_ksp2_ab.txt): a thread expanding the nodes it lowered itself instead of
// publishing them (3.0 -> 3.8 ms), a longer s_sleep (no change), 512 threads
// (3.0 -> 4.2 ms), 2 or 8 nodes per group instead of 4 (no change).
constexpr int kLds16Group = 4;  // nodes a thread expands together (K <= 4)
constexpr int kLds16Sleep = 1;  // s_sleep argument of a wave that found no work
template <int K>
__global__ __launch_bounds__(1024) void spf_lds16_kernel(SpfArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  __shared__ uint32_t s_work, s_min[2], s_nign, s_ovf, s_inf, s_stop;
  const uint32_t N = a.n_nodes;
  const uint32_t NB = (N + 31) >> 5;
  const uint32_t tid = threadIdx.x, nthr = blockDim.x;
  const uint32_t row = a.row_order ? a.row_order[blockIdx.x] : blockIdx.x;
  if (a.row_mask && !a.row_mask[row]) return;
  constexpr int G = K <= 4 ? kLds16Group : 2;  // nodes a thread expands together
  const uint32_t DWp = ((N + 1) / 2 + 3) & ~3u;
  uint32_t stop_lo = 0, stop_hi = 0;  // this row's target nodes (early stop)
  if (a.stop_ptr) {
    stop_lo = a.stop_ptr[row];
    stop_hi = a.stop_ptr[row + 1];
  }
  uint32_t* dist = lds;  // node u: bits 16 (u & 1) .. of word u / 2
  uint32_t* near = lds + DWp;
  uint32_t* far = near + NB;
  uint32_t* filt = far + NB;
  uint32_t FW = 1;
  while (2 * FW <= min(NB, 256u)) FW *= 2;
  uint32_t* sp_key = filt + FW;  // spill table: node id (~0u empty) | distance
  uint32_t* sp_val = sp_key + kSpillSlots;
  const uint32_t fshift = 32u - (5u + static_cast<uint32_t>(__builtin_ctz(FW)));
  Src s(a, row);
  for (uint32_t i = tid; i < DWp; i += nthr) dist[i] = 0xFFFFFFFFu;
  for (uint32_t i = tid; i < 2 * NB; i += nthr) near[i] = 0u;
  for (uint32_t i = tid; i < 2 * kSpillSlots; i += nthr) sp_key[i] = ~0u;
  if (s.n_ign)
    for (uint32_t i = tid; i < FW; i += nthr) filt[i] = 0u;
  if (tid < 2) s_min[tid] = kInf;
  if (tid == 0) {
    s_nign = 0u;
    s_ovf = 0u;
    s_inf = 0u;
    s_stop = 0u;
  }
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
    // the set itself into LDS too: a filter hit (every relaxation of an
    // ignored link - KSP2's k = 2 searches start on the k = 1 path) then
    // binary-searches LDS instead of a chain of dependent global loads
    if (s.n_ign <= kIgnLds) {
      uint32_t* ign_lds = sp_key + 2 * kSpillSlots;
      for (uint32_t i = tid; i < s.n_ign; i += nthr) ign_lds[i] = s.ign[i];
      __syncthreads();
      s.ign = ign_lds;
    }
  }
  if (tid == 0) {
    dist[s.node >> 1] &= ~(0xFFFFu << ((s.node & 1u) * 16u));
    near[s.node >> 5] = 1u << (s.node & 31u);
    s_work = 1u;
  }
  __syncthreads();
  // spill slot of u (inserted when `insert`), or -1: absent / table full
  auto sp_slot = [&](uint32_t u, bool insert) -> int {
    uint32_t h = (u * 0x9E3779B1u) >> (32u - 11u);  // 2048 slots
    for (uint32_t p = 0; p < kSpillProbe; ++p, h = (h + 1u) & (kSpillSlots - 1u)) {
      const uint32_t k = sp_key[h];
      if (k == u) return static_cast<int>(h);
      if (k != ~0u) continue;
      if (!insert) return -1;
      const uint32_t prev = atomicCAS(&sp_key[h], ~0u, u);
      if (prev == ~0u || prev == u) return static_cast<int>(h);
    }
    return -1;
  };
  // distance of u from its u16 entry e (kInf: unreached)
  auto eff = [&](uint32_t u, uint32_t e) -> uint32_t {
    if (e < kD16Spill) return e;
    if (e == kD16None) return kInf;
    const int sl = sp_slot(u, false);
    return sl < 0 ? kInf : sp_val[sl];
  };
  auto get = [&](uint32_t u) { return eff(u, (dist[u >> 1] >> ((u & 1u) * 16u)) & 0xFFFFu); };

  const uint32_t delta = a.delta;
  uint32_t T = delta;
  uint32_t mpar = 0;
  uint32_t stop_m = 0;  // > 0: stopped with every node at distance <= stop_m final
  bool ovf = false;
  const bool lane0 = (tid & 63u) == 0u;
  for (;;) {
    uint32_t far_min = kInf;
    uint32_t newq = 0;  // pushes of the current group that queued a node
    // lower u to nd, starting from the word w as read; queue it if lowered
    auto merge = [&](uint32_t u, uint32_t nd, uint32_t w) {
      const uint32_t sh = (u & 1u) * 16u;
      uint32_t e = (w >> sh) & 0xFFFFu;
      if (nd < kD16Spill) {  // inline: below any spilled distance
        for (;;) {
          if (e < kD16Spill && nd >= e) return;
          const uint32_t nw = (w & ~(0xFFFFu << sh)) | (nd << sh);
          const uint32_t prev = atomicCAS(&dist[u >> 1], w, nw);
          if (prev == w) break;
          w = prev;
          e = (w >> sh) & 0xFFFFu;
        }
      } else {
        if (e < kD16Spill) return;  // an inline distance is smaller
        const int sl = sp_slot(u, true);
        if (sl < 0) {  // table full: dropped
          ovf = true;
          return;
        }
        if (nd >= atomicMin(&sp_val[sl], nd)) return;
        while (e == kD16None) {  // mark the entry spilled (unless it went inline meanwhile)
          const uint32_t nw = w & ~(0x1u << sh);  // 0xFFFF -> 0xFFFE
          const uint32_t prev = atomicCAS(&dist[u >> 1], w, nw);
          if (prev == w) break;
          w = prev;
          e = (w >> sh) & 0xFFFFu;
        }
        if (e < kD16Spill) return;
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
    uint32_t wi = tid, bits = 0, wbase = 0;
    for (;;) {
      uint32_t vs[G];
      int c = 0;
      while (c < G) {
        while (!bits && wi < NB) {
          bits = __hip_atomic_load(&near[wi], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          if (bits) bits = atomicExch(&near[wi], 0u);  // at least the bits seen: only we clear
          wbase = wi * 32;
          wi += nthr;
        }
        if (!bits) break;
        vs[c++] = wbase + __builtin_ctz(bits);
        bits &= bits - 1;
      }
      if (!bits && wi >= NB) wi = tid;  // words exhausted: rescan them next time
      if (__builtin_amdgcn_ballot_w64(c > 0) == 0ull) {
        const uint32_t pending = __builtin_amdgcn_readfirstlane(
            __hip_atomic_load(&s_work, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
        if (pending == 0u) break;
        __builtin_amdgcn_s_sleep(kLds16Sleep);
        continue;
      }
      // the group's records in flight together, then the neighbours' words
      uint2 rec[G][K];
      uint32_t lk[G][K];  // link ids (ignore sets), loaded with the records
#pragma unroll
      for (int g = 0; g < G; ++g) {
        if (g < c) load_recs<K>(a, vs[g], rec[g]);
#pragma unroll
        for (int j = 0; j < K; ++j) lk[g][j] = (g < c && s.n_ign) ? a.link[vs[g] * K + j] : 0u;
      }
      // every push the group can make (its records, continuation lists
      // included), reserved in s_work by the wave before any of its merges
      uint32_t bound = 0;
#pragma unroll
      for (int g = 0; g < G; ++g)
        if (g < c) bound += K + ((rec[g][K - 1].x & ORH_REC_CONT) ? rec[g][K - 1].y : 0u);
      const uint32_t resv = wave_sum(bound);
      if (lane0 && resv) atomicAdd(&s_work, resv);
      newq = 0;
      if (c > 0) {
        uint32_t dv[G], nw[G][K];
        bool ok[G][K];
#pragma unroll
        for (int g = 0; g < G; ++g) {
          dv[g] = g < c ? get(vs[g]) : 0u;
          const bool transit = g < c && (vs[g] == s.node || !(rec[g][0].x & ORH_REC_ROW_OVL));
#pragma unroll
          for (int j = 0; j < K; ++j) {
            ok[g][j] = transit && live_link(s, rec[g][j], lk[g][j]);
            nw[g][j] = ok[g][j] ? dist[(rec[g][j].x & ORH_REC_COL_MASK) >> 1] : 0u;
          }
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
          if (g >= c) break;
#pragma unroll
          for (int j = 0; j < K; ++j)
            if (ok[g][j])
              merge(rec[g][j].x & ORH_REC_COL_MASK, dv[g] + (a.use_link_metric ? rec[g][j].y : 1u), nw[g][j]);
          const uint2 last = rec[g][K - 1];
          const bool transit = vs[g] == s.node || !(rec[g][0].x & ORH_REC_ROW_OVL);
          if (transit && (last.x & ORH_REC_CONT)) {
            const uint32_t start = last.x & ORH_REC_COL_MASK;
            for (uint32_t q = 0; q < last.y; ++q) {
              const uint2 r = a.recs[start + q];
              if (!live(a, s, r, start + q)) continue;
              const uint32_t u = r.x & ORH_REC_COL_MASK;
              merge(u, dv[g] + (a.use_link_metric ? r.y : 1u), dist[u >> 1]);
            }
          }
        }
      }
      // the unused reservation and the expanded nodes, after the merges
      const uint32_t back = wave_sum(c > 0 ? bound - newq + static_cast<uint32_t>(c) : 0u);
      if (lane0 && back) atomicSub(&s_work, back);
    }
    {
      const uint32_t fm = wave_min(far_min);
      if ((tid & 63u) == 0 && fm != kInf) atomicMin(&s_min[mpar], fm);
    }
    __syncthreads();  // bucket drained everywhere; far bound folded
    const uint32_t m = s_min[mpar];
    if (m == kInf) break;  // far set empty: done
    T = m + delta;
    const uint32_t npar = mpar ^ 1u;
    if (tid == 0) {
      s_min[npar] = kInf;
      // every node at distance <= m is final (m: the least unsettled one);
      // once the targets are among them, no trace to them reads further
      if (stop_hi > stop_lo) {
        bool done = true;
        for (uint32_t q = stop_lo; q < stop_hi && done; ++q) done = get(a.stop_nodes[q]) <= m;
        if (done) s_stop = m;
      }
    }
    __syncthreads();
    if (s_stop) {
      stop_m = s_stop;
      break;
    }
    uint32_t local_min = kInf, promoted = 0;
    for (uint32_t w2 = tid; w2 < NB; w2 += nthr) {
      const uint32_t fb = far[w2];
      uint32_t promote = 0u;
      for (uint32_t q = fb; q; q &= q - 1) {
        const uint32_t b = __builtin_ctz(q);
        const uint32_t d = get(w2 * 32 + b);
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
    if (lane0 && pr) atomicAdd(&s_work, pr);
    const uint32_t wm = wave_min(local_min);
    if ((tid & 63u) == 0 && wm != kInf) atomicMin(&s_min[npar], wm);
    mpar = npar;
    __syncthreads();
  }
  if (ovf) s_ovf = 1u;
  __syncthreads();
  uint32_t* od = dist_row(a.out_dist, a.scratch, a.n_out, N, row);
  bool inf = false;
  for (uint32_t i = tid; i < N; i += nthr) {
    const uint32_t d = get(i);
    inf |= d == kInf;
    __builtin_nontemporal_store(d, &od[i]);
  }
  // exact unless a node ended unreached; stopped early, exact up to stop_m
  // unless the spill table overflowed below it (dropped candidates are all
  // >= 0xFFFE): otherwise the HBM kernel redoes the row
  if (s_ovf && !(stop_m && stop_m < kD16Spill)) {
    if (inf || stop_m) s_inf = 1u;
    __syncthreads();
    if (tid == 0 && s_inf) {
      const uint32_t k = atomicAdd(&a.ovf_rows[0], 1u);
      a.ovf_rows[1 + k] = row;
    }
  }
}

// ---------------------------------------------------------------------------
// phase 1c''': general metrics, first hops fused, labels in LDS (kLdsNh)
// ---------------------------------------------------------------------------
// The asynchronous delta-stepping of spf_global_nh_async_kernel with its
// {dist, first-hop mask} labels in LDS instead of HBM: a weighted graph that
// fits (N = 10,000: 40 KB packed) is searched by one workgroup per source
// with no global atomics and no second phase - the first hops ride along the
// search as in runSpf itself (LinkState.cpp:857-873): a smaller candidate
// replaces a label, an equal one ORs its mask in (and re-queues the node so
// the new bits reach its successors). The fixpoint is order-independent, so
// the rows are the HBM kernel's bit for bit.
// kPacked: a u32 label {dist (16 bits, hi) | mask (16 bits, lo)}, for sources
// with <= 16 distinct neighbours; a candidate distance >= 0xFFFF cannot be
// held, so the row is appended to a.ovf_rows and written by the u64 form
// (launch_spf_lds_nh runs it over that list). Else a u64 label {dist (32) |
// mask (32)} as in the HBM kernel.
template <int K, bool kPacked>
__global__ __launch_bounds__(1024) void spf_lds_nh_kernel(SpfArgs a) {
  typedef typename std::conditional<kPacked, uint32_t, unsigned long long>::type L;
  constexpr uint32_t kSh = kPacked ? 16u : 32u;
  constexpr uint32_t kDInf = kPacked ? 0xFFFFu : 0xFFFFFFFFu;  // the unreached distance
  constexpr L kInfLabel = static_cast<L>(static_cast<L>(kDInf) << kSh);
  constexpr L kMaskBits = static_cast<L>((static_cast<L>(1) << kSh) - 1u);
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  __shared__ uint32_t s_work, s_min[2], s_nign, s_ovf;
  const uint32_t N = a.n_nodes;
  const uint32_t NB = (N + 31) >> 5;
  const uint32_t tid = threadIdx.x, nthr = blockDim.x;
  if (a.row_list && blockIdx.x >= *a.row_count) return;
  const uint32_t row = a.row_list ? a.row_list[blockIdx.x] : blockIdx.x;
  constexpr int G = K <= 4 ? 4 : 2;
  L* lab = reinterpret_cast<L*>(lds);
  const uint32_t lab_words = kPacked ? ((N + 1u) & ~1u) : 2u * N;  // keeps near 8-byte aligned
  uint32_t* near = lds + lab_words;
  uint32_t* far = near + NB;
  uint32_t* filt = far + NB;
  uint32_t FW = 1;
  while (2 * FW <= min(NB, 256u)) FW *= 2;
  const uint32_t fshift = 32u - (5u + static_cast<uint32_t>(__builtin_ctz(FW)));
  Src s(a, row);
  for (uint32_t i = tid; i < N; i += nthr) lab[i] = kInfLabel;
  for (uint32_t i = tid; i < 2 * NB; i += nthr) near[i] = 0u;
  if (s.n_ign)
    for (uint32_t i = tid; i < FW; i += nthr) filt[i] = 0u;
  if (tid < 2) s_min[tid] = kInf;
  if (tid == 0) {
    s_nign = 0u;
    s_ovf = 0u;
  }
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
  bool ovf = false;
  for (;;) {
    uint32_t far_min = kInf;
    // merge the candidate {nd, cnh} into u's label (cl: as loaded); re-queue
    // u if the label changed
    auto merge = [&](uint32_t u, uint32_t nd, uint32_t cnh, L cl) {
      if (kPacked && nd >= kDInf) {  // not representable: the u64 form redoes the row
        ovf = true;
        return;
      }
      for (;;) {
        const uint32_t cd = static_cast<uint32_t>(cl >> kSh);
        if (nd > cd) return;
        const L nl = nd < cd ? static_cast<L>((static_cast<L>(nd) << kSh) | cnh) : static_cast<L>(cl | cnh);
        if (nl == cl) return;
        const L old = atomicCAS(&lab[u], cl, nl);
        if (old == cl) break;
        cl = old;
      }
      const uint32_t bit = 1u << (u & 31u);
      if (nd < T) {
        atomicAdd(&s_work, 1u);  // counted before the bit is visible
        const uint32_t old = atomicOr(&near[u >> 5], bit);
        atomicAnd(&far[u >> 5], ~bit);
        if (old & bit) atomicSub(&s_work, 1u);  // already queued
      } else {
        atomicOr(&far[u >> 5], bit);
        far_min = min(far_min, nd);
      }
    };
    uint32_t wi = tid, bits = 0, wbase = 0;
    for (;;) {
      uint32_t vs[G];
      int c = 0;
      while (c < G) {
        while (!bits && wi < NB) {
          bits = __hip_atomic_load(&near[wi], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          if (bits) bits = atomicExch(&near[wi], 0u);  // at least the bits seen: only we clear
          wbase = wi * 32;
          wi += nthr;
        }
        if (!bits) break;
        vs[c++] = wbase + __builtin_ctz(bits);
        bits &= bits - 1;
      }
      if (!bits && wi >= NB) wi = tid;  // words exhausted: rescan them next time
      if (__builtin_amdgcn_ballot_w64(c > 0) == 0ull) {
        const uint32_t pending = __builtin_amdgcn_readfirstlane(
            __hip_atomic_load(&s_work, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
        if (pending == 0u) break;
        __builtin_amdgcn_s_sleep(1);
        continue;
      }
      if (c > 0) {
        // the group's records in flight together, then the labels
        uint2 rec[G][K];
        uint32_t lk[G][K];
#pragma unroll
        for (int g = 0; g < G; ++g) {
          if (g < c) load_recs<K>(a, vs[g], rec[g]);
#pragma unroll
          for (int j = 0; j < K; ++j) lk[g][j] = (g < c && s.n_ign) ? a.link[vs[g] * K + j] : 0u;
        }
        L lv[G], cl[G][K];
        bool ok[G][K];
#pragma unroll
        for (int g = 0; g < G; ++g) {
          lv[g] = g < c ? lab[vs[g]] : static_cast<L>(0);
          const bool transit = g < c && (vs[g] == s.node || !(rec[g][0].x & ORH_REC_ROW_OVL));
#pragma unroll
          for (int j = 0; j < K; ++j) {
            ok[g][j] = transit && live_link(s, rec[g][j], lk[g][j]);
            cl[g][j] = ok[g][j] ? lab[rec[g][j].x & ORH_REC_COL_MASK] : static_cast<L>(0);
          }
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
          if (g >= c) break;
          const uint32_t v = vs[g];
          const uint32_t dv = static_cast<uint32_t>(lv[g] >> kSh);
          const uint32_t nhv = static_cast<uint32_t>(lv[g] & kMaskBits);
          const bool from_src = v == s.node;
#pragma unroll
          for (int j = 0; j < K; ++j)
            if (ok[g][j])
              merge(rec[g][j].x & ORH_REC_COL_MASK, dv + (a.use_link_metric ? rec[g][j].y : 1u),
                    from_src ? (1u << a.rank_out[v * K + j]) : nhv, cl[g][j]);
          const uint2 last = rec[g][K - 1];
          const bool transit = from_src || !(rec[g][0].x & ORH_REC_ROW_OVL);
          if (transit && (last.x & ORH_REC_CONT)) {
            const uint32_t start = last.x & ORH_REC_COL_MASK;
            for (uint32_t q = 0; q < last.y; ++q) {
              const uint2 r = a.recs[start + q];
              if (!live(a, s, r, start + q)) continue;
              const uint32_t u = r.x & ORH_REC_COL_MASK;
              merge(u, dv + (a.use_link_metric ? r.y : 1u), from_src ? (1u << a.rank_out[start + q]) : nhv,
                    lab[u]);
            }
          }
        }
        atomicSub(&s_work, static_cast<uint32_t>(c));
      }
    }
    {
      const uint32_t fm = wave_min(far_min);
      if ((tid & 63u) == 0 && fm != kInf) atomicMin(&s_min[mpar], fm);
    }
    __syncthreads();  // bucket drained everywhere; far bound folded
    const uint32_t m = s_min[mpar];
    if (m == kInf) break;  // far set empty: done
    T = m + delta;
    const uint32_t npar = mpar ^ 1u;
    if (tid == 0) s_min[npar] = kInf;
    __syncthreads();
    uint32_t local_min = kInf, promoted = 0;
    for (uint32_t w2 = tid; w2 < NB; w2 += nthr) {
      const uint32_t fb = far[w2];
      uint32_t promote = 0u;
      for (uint32_t q = fb; q; q &= q - 1) {
        const uint32_t b = __builtin_ctz(q);
        const uint32_t d = static_cast<uint32_t>(lab[w2 * 32 + b] >> kSh);
        if (d < T) promote |= 1u << b;
        else local_min = min(local_min, d);
      }
      if (promote) {
        far[w2] = fb & ~promote;
        near[w2] = promote;  // the near set is empty between buckets
        promoted += __builtin_popcount(promote);
      }
    }
    if (promoted) atomicAdd(&s_work, promoted);
    const uint32_t wm = wave_min(local_min);
    if ((tid & 63u) == 0 && wm != kInf) atomicMin(&s_min[npar], wm);
    mpar = npar;
    __syncthreads();
  }
  if (kPacked && ovf) s_ovf = 1u;
  __syncthreads();
  if (kPacked && s_ovf) {  // the u64 form writes this row
    if (tid == 0) {
      const uint32_t k = atomicAdd(&a.ovf_rows[0], 1u);
      a.ovf_rows[1 + k] = row;
    }
    return;
  }
  // labels -> dist row (kInf = unreachable) and first-hop row, coalesced (a
  // neighbour row of a two-phase plan, row >= n_out: the distances alone)
  uint32_t* od = dist_row(a.out_dist, a.scratch, a.n_out, N, row);
  uint32_t* on = row < a.n_out ? a.out_nh + static_cast<size_t>(row) * N * a.words : nullptr;
  for (uint32_t i = tid; i < N; i += nthr) {
    const L l = lab[i];
    const uint32_t d = static_cast<uint32_t>(l >> kSh);
    __builtin_nontemporal_store(d == kDInf ? kInf : d, &od[i]);
    const uint32_t m = static_cast<uint32_t>(l & kMaskBits);
    if (!on) continue;
    if (a.words == 1) {
      __builtin_nontemporal_store(m, &on[i]);
    } else {
      on[static_cast<size_t>(i) * a.words] = m;
      for (uint32_t k = 1; k < a.words; ++k) on[static_cast<size_t>(i) * a.words + k] = 0u;
    }
  }
}

size_t lds_nh_bytes(uint32_t n_nodes, bool packed) {
  const size_t nb = (n_nodes + 31) / 32;
  size_t fw = 1;
  while (2 * fw <= std::min<size_t>(nb, 256)) fw *= 2;
  const size_t lab = packed ? ((n_nodes + 1) & ~size_t{1}) : 2 * static_cast<size_t>(n_nodes);
  return 4 * (lab + 2 * nb + fw);
}

size_t lds16_bytes(uint32_t n_nodes) {
  const size_t nb = (n_nodes + 31) / 32;
  size_t fw = 1;
  while (2 * fw <= std::min<size_t>(nb, 256)) fw *= 2;
  return 4 * ((((n_nodes + 1) / 2 + 3) & ~size_t{3}) + 2 * nb + fw + 2 * kSpillSlots + kIgnLds);
}

hipError_t launch_spf_lds16(const SpfPlan& fallback, SpfArgs a, uint32_t n_rows, uint32_t ell_k,
                            hipStream_t s) {
  if (n_rows == 0) return hipSuccess;
  if (!a.ovf_rows || !a.dist_only || fallback.variant != SpfVariant::kGlobalNh) return hipErrorInvalidValue;
  a.n_rows = n_rows;
  const size_t lds = lds16_bytes(a.n_nodes);
  hipError_t e = hipMemsetAsync(a.ovf_rows, 0, 4, s);
  if (e != hipSuccess) return e;
  static const uint32_t block = launch_knobs().lds16_block;
  e = ell_k == 8 ? launch(spf_lds16_kernel<8>, a, n_rows, block, lds, s)
                 : launch(spf_lds16_kernel<4>, a, n_rows, block, lds, s);
  if (e != hipSuccess) return e;
  // rows the u16 search could not finish: the HBM kernel over that list
  // (workgroups past the list's length exit at once)
  SpfArgs b = a;
  b.row_list = a.ovf_rows + 1;
  b.row_count = a.ovf_rows;
  b.row_order = nullptr;
  return launch_spf(fallback, b, n_rows, s);
}

hipError_t launch_spf_lds_nh(SpfArgs a, uint32_t n_rows, uint32_t ell_k, bool packed, uint32_t block,
                             hipStream_t s) {
  if (n_rows == 0) return hipSuccess;
  if (packed && !a.ovf_rows) return hipErrorInvalidValue;
  a.n_rows = n_rows;
  a.row_list = nullptr;
  a.row_count = nullptr;
  hipError_t e = hipSuccess;
  if (packed) {
    e = hipMemsetAsync(a.ovf_rows, 0, 4, s);
    if (e != hipSuccess) return e;
    const size_t lds = lds_nh_bytes(a.n_nodes, true);
    e = ell_k == 8 ? launch(spf_lds_nh_kernel<8, true>, a, n_rows, block, lds, s)
                   : launch(spf_lds_nh_kernel<4, true>, a, n_rows, block, lds, s);
    if (e != hipSuccess) return e;
    // rows with a distance past 16 bits: the u64 form over that list
    // (workgroups past the list's length exit at once)
    a.row_list = a.ovf_rows + 1;
    a.row_count = a.ovf_rows;
  }
  const size_t lds = lds_nh_bytes(a.n_nodes, false);
  return ell_k == 8 ? launch(spf_lds_nh_kernel<8, false>, a, n_rows, block, lds, s)
                    : launch(spf_lds_nh_kernel<4, false>, a, n_rows, block, lds, s);
}

hipError_t launch_lds_nh_rows(const SpfArgs& a, uint32_t n_rows, hipStream_t s) {
  const size_t lds = lds_nh_bytes(a.n_nodes, false);
  return a.recs_k == 8 ? launch(spf_lds_nh_kernel<8, false>, a, n_rows, 256, lds, s)
                       : launch(spf_lds_nh_kernel<4, false>, a, n_rows, 256, lds, s);
}

}  // namespace orh
