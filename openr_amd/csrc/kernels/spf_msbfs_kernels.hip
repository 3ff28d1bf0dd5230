// SPF kernels, uniform metric, many sources: bit-parallel multi-source BFS
// (kMsBfs) and the pass that turns its level blocks into rows.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "spf_device.h"
#include "spf_launch.h"

namespace orh {

// ---------------------------------------------------------------------------
// phase 1a': bit-parallel multi-source BFS (uniform metric, no ignore sets)
// ---------------------------------------------------------------------------
// One workgroup runs S = 32 (u32 masks) or 16 (u16) source rows at once, one
// bit per source (multi-source BFS, Then et al., VLDB 2015), as a pull over
// the nodes:
//   nx(v) = (OR over live records v -> u of F(u)) & ~visited(v)
// Thread t owns the nodes t, t + B, ..., t + (J-1)B of the layout's order
// (cluster order on deep graphs, else Cuthill-McKee: host/ms_order.h) and keeps
// their ELL columns (packed 16-bit; a dead or down slot points at an
// always-zero LDS entry) and their visited masks in registers, so LDS holds
// only the two frontier arrays (this level's and the next): 8 bytes per node
// at S = 32, two workgroups per CU at N = 10,000. Groups of owned nodes whose
// masks are full on every lane are skipped (a full node's stale frontier
// entry only repeats bits every neighbour already holds). A node's bits
// reach its neighbours only if it is a transit node (not overloaded; a
// source always transits its own bit at level 0).
//
// Levels leave the CU as they are found, as bytes in a node-major scratch
// lvl[(batch * N + v) * S + b] (one S-byte block per node, written only by
// the node's owner thread, so a store instruction's 64 lanes land in one
// 2 KB span), and ms_finalize_kernel turns the scratch into host-order rows
// with coalesced stores (u8 level rows; the u32 distance rows too, unless
// the first-hop pass writes those, HopArgs::write_dist). (Measured alternatives: a row-major scratch
// written per source bit issues ~5x more store instructions on the grid, where
// a node's bits arrive a few at a time but different lanes get different bits;
// dword stores for whole nibbles cost more than the stores they save.) Levels
// >= 254 are written to the output row directly (marker 254), so any depth is
// exact; 255 = unreached.
//
// Interval skip (kMsSkipInterval): every live record v -> u has |u - v| <= bw, the
// bandwidth of the layout's order (small in Cuthill-McKee order, which is
// where the skip can pay; most of N in cluster order). If the nodes
// that gained a bit at level L-1 span the ids [lo, hi], only nodes in
// [lo - bw, hi + bw] can gain one at level L; a 64-node slice (one wave's
// nodes of one j) outside it is skipped without reading its neighbours'
// frontier entries. The interval is two LDS words per level (wave min / max
// reductions); the per-slice test is scalar, so the variant costs no VGPRs
// beyond the two running bounds (a slice-bitmap form of the same skip needed
// 117 VGPRs, one workgroup per CU, and ran 1.4x slower).
//
// Adjacency skip (kMsSkipAdj, a.ms_adj): cluster order makes the id bandwidth
// most of N but keeps the slices a slice touches few (ms_slice_adjacency,
// host/ms_order.h: 6.6 on the 10k grid), so the key is which slices gained a
// bit, not an id interval. s_act holds one bit per slice in three phases,
// like s_lo / s_hin: during level L a wave whose slice has any arrival
// (nx != 0 before the overloaded-node mask: conservative) ORs the slice's bit
// into phase L % 3 and phase (L + 1) % 3 is cleared; the sources' slices are
// marked where the sources are planted. Right after level L - 1's barrier,
// with the progress flag (one LDS round trip), lane 8 q + k reads word k of
// phase (L - 1) % 3; at the top of level L it ANDs it with word k of the
// adjacency mask of the wave's slice 8 r + q, which it keeps in adjm[r], and
// one ballot per r gives the wave-uniform todo bits: slice j is todo iff a
// slice adjacent to it, or itself, was marked. A group runs only if it is open and one of its slices
// is todo, so it keeps the group of 2 and its back-to-back gathers. The
// adjacency is built from every record a node has, down ones included, so
// link flips cannot invalidate it. Measured: the 2-lane C2 step 19.41 ->
// 18.83 ms; slower where a batch has its CU to itself, so the latency and
// lone-sweep plans leave it off (ms_set_width; profiles/ms_adj/).
//
// Why a skipped slice is harmless under either skip: it keeps stale f_nxt
// entries, but a stale entry's bits reached every neighbour one level after
// they were new - that neighbour's slice ran on that level, because the
// node's own slice had just gained them (it was within reach / marked) - so
// a stale entry only repeats bits its readers have visited (see below). And a
// slice none of whose adjacent slices was marked reads stale or zero entries
// alone: nothing can arrive.
//
// The search is latency-bound, not LDS-bound: on the 10k grid one workgroup
// takes ~0.7 ms whether 32 or 313 of them run (two fit per CU), ~165 levels
// of ~9k cycles, of which ~25 % are the level-byte stores and ~23 % the
// barrier. A top-down form (a node reads only its own word, new frontier
// nodes OR their bits into their neighbours' words with ds_or) issues ~4x
// fewer LDS operations and measured slower: 0.79 vs 0.74 ms (grid), 0.21 vs
// 0.18 ms (C3 Clos).
template <class M>
struct MsMask;
// V: the register type of a node's visited / new bits
template <>
struct MsMask<uint64_t> {
  static constexpr uint32_t kS = 64;
  typedef uint64_t V;
  __device__ static uint32_t ctz(uint64_t x) { return static_cast<uint32_t>(__builtin_ctzll(x)); }
};
template <>
struct MsMask<uint32_t> {
  static constexpr uint32_t kS = 32;
  typedef uint32_t V;
  __device__ static uint32_t ctz(uint32_t x) { return static_cast<uint32_t>(__builtin_ctz(x)); }
};
template <>
struct MsMask<uint16_t> {
  static constexpr uint32_t kS = 16;
  typedef uint32_t V;
  __device__ static uint32_t ctz(uint32_t x) { return static_cast<uint32_t>(__builtin_ctz(x)); }
};

__device__ inline uint32_t ms_col(const uint2& r, uint32_t zero) {
  return (r.x & (ORH_REC_SKIP | ORH_REC_CONT)) ? zero : (r.x & ORH_REC_COL_MASK);
}

constexpr int kMsSkipNone = 0, kMsSkipInterval = 1, kMsSkipAdj = 2;
constexpr uint32_t kMsAdjWords = 8;  // host/ms_order.h: words of a slice's adjacency mask

template <int K, class M, int J, int kMode>
__global__ __launch_bounds__(1024) void spf_msbfs_kernel(SpfArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  constexpr uint32_t kS = MsMask<M>::kS;
  typedef typename MsMask<M>::V V;
  constexpr int KH = (K + 1) / 2;
  const uint32_t N = a.n_nodes;
  const uint32_t NZ = a.ms_zero;  // index of the always-zero frontier entry
  const uint32_t tid = threadIdx.x, B = blockDim.x;
  const uint32_t b0 = blockIdx.x * a.ms_width;  // a batch: ms_width <= kS sources
  const uint32_t S = min(a.ms_width, a.n_rows - b0);
  const V full = S >= 8 * sizeof(V) ? ~V(0) : (V(1) << S) - V(1);
  __shared__ uint32_t s_prog[3];
  __shared__ uint32_t s_lo[3], s_hin[3];  // per level: min / ~max id with a new frontier bit
  constexpr bool kSkip = kMode == kMsSkipInterval, kAdj = kMode == kMsSkipAdj;
  __shared__ uint32_t s_act[kAdj ? 3 : 1][kMsAdjWords];  // per level: the slices with an arrival, a bit each
  M* f_cur = reinterpret_cast<M*>(lds);
  M* f_nxt = f_cur + a.ms_pitch;
  // the ELL columns hold byte offsets into a frontier array (16 bits each:
  // the planner keeps pitch * sizeof(M) <= 64 KiB), so a gather address is
  // one add of the array's offset that also picks the half-word (3 VALU ->
  // 1 per gather, ~3 % of the step: profiles/r05/l_msbfs_offsets_ab.txt); u64
  // masks (opt-in) store dword offsets, doubled at the read
  constexpr uint32_t kE = sizeof(M);
  constexpr uint32_t kC = kE <= 4 ? kE : 4;  // bytes per stored column unit
  const char* const lbase = reinterpret_cast<const char*>(lds);
  uint32_t cur_off = 0u, nxt_off = a.ms_pitch * kE;  // f_cur / f_nxt in bytes
  uint8_t* lvl = a.ms_direct ? nullptr : a.ms_lvl + static_cast<size_t>(blockIdx.x) * N * kS;  // [N][kS]
  // arrival log (u16 / u32 masks, kLog): each wave appends its nodes' level
  // events {new bits (hi), slice j << 14 | lane << 8 | level (lo)} to a log
  // of its own - one scalar count, one coalesced store per (j, level) with
  // arrivals - and the node-major level blocks are assembled from the logs
  // once the search ends. Capacity: a node gains >= 1 bit per event, so
  // J * 64 * kS events per wave
  constexpr bool kLog = sizeof(M) <= 4;
  const uint32_t lane = tid & 63u, wave = tid >> 6, waves = B >> 6;
  uint64_t* wlog = kLog ? a.ms_log + (static_cast<size_t>(blockIdx.x) * waves + wave) * J * 64u * kS : nullptr;
  uint32_t wcnt = 0;  // events in this wave's log (wave-uniform)
  __shared__ uint32_t s_wcnt[16];
  auto log_events = [&](int j, V nx, uint32_t lv) -> bool {  // true: the slice has an arrival
    const uint64_t m = __builtin_amdgcn_ballot_w64(nx != 0u);
    if (!m) return false;
    if (nx) {
      const uint32_t pos = wcnt + __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(m >> 32),
                                                            __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(m), 0u));
      wlog[pos] = (static_cast<uint64_t>(nx) << 32) | (static_cast<uint32_t>(j) << 14) | (lane << 8) |
                  min(lv, kLvlDirect);
    }
    wcnt += static_cast<uint32_t>(__builtin_popcountll(m));
    return true;
  };
#ifdef ORH_DIAG_STAMPS
  const uint64_t t_entry = __builtin_amdgcn_s_memtime();
#endif

  for (uint32_t i = tid; i < 2 * a.ms_pitch; i += B) f_cur[i] = 0;
  if (tid < 3) {
    s_prog[tid] = 0u;
    s_lo[tid] = ~0u;
    s_hin[tid] = ~0u;
  }
  if (kAdj && tid < 3 * kMsAdjWords) (&s_act[0][0])[tid] = 0u;
  if (!kLog) {  // every level byte starts as "unreached"
    uint4* l4 = reinterpret_cast<uint4*>(lvl);
    for (uint32_t i = tid; i < N * kS / 16; i += B) l4[i] = make_uint4(~0u, ~0u, ~0u, ~0u);
  }
  __syncthreads();
  if (tid < S) {  // sources may repeat: OR the bits in
    const uint32_t src = a.dev_of[a.srcs[a.order[b0 + tid]]];
    const uintptr_t byte = reinterpret_cast<uintptr_t>(f_cur + src) + tid / 8u;
    atomicOr(reinterpret_cast<uint32_t*>(byte & ~uintptr_t(3)), 1u << ((byte & 3u) * 8u + (tid & 7u)));
    if (!kLog) lvl[static_cast<size_t>(src) * kS + tid] = 0;
  }
  if (kSkip && tid < S) {  // level 0's frontier: the sources
    const uint32_t src = a.dev_of[a.srcs[a.order[b0 + tid]]];
    atomicMin(&s_lo[0], src);
    atomicMin(&s_hin[0], ~src);
  }
  if (kAdj && tid < S) {  // level 0's marks: the sources' slices, wherever they are
    const uint32_t sl = a.dev_of[a.srcs[a.order[b0 + tid]]] >> 6;
    atomicOr(&s_act[0][sl >> 5], 1u << (sl & 31u));
  }
  // adjacency masks of this wave's slices: lane 8 q + k holds word k of
  // slice j = 8 r + q (id slice j * waves + wave) in adjm[r]
  constexpr int kAdjR = kAdj ? (J + 7) / 8 : 1;
  uint32_t adjm[kAdjR];
  if constexpr (kAdj) {
    const uint32_t n_slices = (N + 63u) >> 6;
#pragma unroll
    for (int r = 0; r < kAdjR; ++r) {
      const uint32_t j = 8u * r + (lane >> 3), sl = j * waves + wave;
      adjm[r] = j < static_cast<uint32_t>(J) && sl < n_slices ? a.ms_adj[sl * kMsAdjWords + (lane & 7u)] : 0u;
      // the load lands here, not in the level loop: a use the compiler cannot
      // see through, or it waits for vmcnt(0) - and with it for every log
      // store of the level before - at the top of each level
      asm volatile("" : "+v"(adjm[r]));
    }
  }

  uint32_t col[J][KH];
  V vis[J];
  uint32_t ovlm = 0u, ovfm = 0u;  // bit j: owned node j overloaded / has an overflow list
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const uint32_t v = j * B + tid;
#pragma unroll
    for (int h = 0; h < KH; ++h) col[j][h] = (NZ * kC) | ((NZ * kC) << 16);
    vis[j] = full;
    if (v < N) {
      const uint2* slots = a.recs + static_cast<size_t>(v) * K;
      uint2 r[K];
#pragma unroll
      for (int k = 0; k < K; ++k) r[k] = slots[k];
#pragma unroll
      for (int h = 0; h < KH; ++h)
        col[j][h] = ms_col(r[2 * h], NZ) * kC | ((2 * h + 1 < K ? ms_col(r[2 * h + 1], NZ) : NZ) * kC << 16);
      if (r[0].x & ORH_REC_ROW_OVL) ovlm |= 1u << j;
      if (r[K - 1].x & ORH_REC_CONT) ovfm |= 1u << j;
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const uint32_t v = j * B + tid;
    if (v < N) vis[j] = f_cur[v];  // level 0: the sources
    if (kLog) log_events(j, v < N ? vis[j] : V(0), 0u);
  }
  // (a wave-uniform bit j - some lane of this wave owns, in slice j, a node
  // with an overflow list / an overloaded node - tested before the per-lane
  // tests measured slower: the kernel grew from 89 to 107 VGPRs and the 2-lane
  // step from 23.0 to 26.5 ms (profiles/r06/g_ms_ab.txt), so the per-lane
  // tests stay alone)

  const uint32_t w0 = a.w0;
#ifdef ORH_DIAG_STAMPS
  const uint64_t t_begin = __builtin_amdgcn_s_memtime();
  uint64_t t_bar = 0, t_store = 0;
  uint32_t n_levels = 0;
#endif
  const uint32_t bw = a.ms_bw;
  const uint32_t wave_base = __builtin_amdgcn_readfirstlane(tid & ~63u);
  // adjacency skip: word lane & 7 of the previous level's marks, read right
  // after the level barrier together with the progress flag (one LDS round
  // trip a level, not two)
  uint32_t act = 0u;
  if constexpr (kAdj) act = s_act[0][lane & 7u];
  uint32_t level = 1;
  for (;; ++level) {
    int prog = 0;
    // opaque per level: keeps the compiler from hoisting J * K unpacked LDS
    // addresses and J per-node pointers out of the level loop (VGPR budget:
    // a 768-thread workgroup per CU at J = 16 uses ~74)
    uint32_t me = tid;
    asm volatile("" : "+v"(me));
    // ids that can gain a bit at this level: within bw of the previous
    // level's new frontier (scalar; empty when the frontier was)
    uint32_t reach_lo = 0u, reach_hi = ~0u, jm = 0u;  // jm: this wave's slices with a new frontier bit
    // first id of this wave's slice j0 (advanced by B per slice; opaque per
    // level so the 16 slice bases are not hoisted into SGPRs that spill)
    uint32_t slice = wave_base;
    if constexpr (kSkip) asm volatile("" : "+s"(slice));
    // adjacency skip: bit 8 q.. of todo[r] set iff slice 8 r + q can gain a bit
    uint64_t todo[kAdjR];
    if constexpr (kAdj) {
#pragma unroll
      for (int r = 0; r < kAdjR; ++r) {
        asm volatile("" : "+v"(adjm[r]));
        todo[r] = __builtin_amdgcn_ballot_w64((act & adjm[r]) != 0u);
      }
      if (tid < kMsAdjWords) s_act[(level + 1u) % 3u][tid] = 0u;  // read at level - 1, written at level + 1
    }
    if constexpr (kSkip) {
      const uint32_t lo = __builtin_amdgcn_readfirstlane(s_lo[(level + 2u) % 3u]);
      const uint32_t hi = ~__builtin_amdgcn_readfirstlane(s_hin[(level + 2u) % 3u]);
      reach_lo = lo > bw ? lo - bw : 0u;
      reach_hi = hi + bw;
      if (tid < 1) {  // read at level - 1, written at level + 1
        s_lo[(level + 1u) % 3u] = ~0u;
        s_hin[(level + 1u) % 3u] = ~0u;
      }
    }
    // groups of G owned nodes: a group is skipped when every lane holds all
    // bits for all G nodes (wave-uniform branch); otherwise all G * K
    // frontier reads go out back to back before any is consumed. The skip
    // variant tests single slices (G = 1): its active band is a slice or two
    // per wave, and a group of 4 would do 2-4x the reads the band needs
    // owned nodes whose frontier reads go out together: 2 (round 4: one C2
    // sweep 0.859 -> 0.823 ms and the 4-lane step 25.6 -> 25.0 ms against 4;
    // 5: no change; 10: slower - profiles/r04/v_ms_group_ab.txt)
    constexpr int kMsGroup = 2;
    constexpr int G = kSkip ? 1 : (J % kMsGroup == 0 ? kMsGroup : 2);
#pragma unroll
    for (int j0 = 0; j0 < J; j0 += G) {
      const uint32_t sl = slice;
      if constexpr (kSkip) slice += B;
      if constexpr (kAdj) {  // j0 and G are even: the group's slices sit in one todo word
        static_assert(G == 2, "the adjacency skip tests groups of 2 slices");
        if (!((todo[j0 / 8] >> (8 * (j0 % 8))) & 0xFFFFull)) continue;
      }
      bool open = false;
#pragma unroll
      for (int g = 0; g < G; ++g) open |= vis[j0 + g] != full;
      if (!__builtin_amdgcn_ballot_w64(open)) continue;
      // no new frontier within reach of the slice: nothing can arrive, and
      // its f_nxt entries stay stale (harmless, see above)
      if (kSkip && (sl > reach_hi || sl + 63u < reach_lo)) continue;
      V acc[G];
#pragma unroll
      for (int g = 0; g < G; ++g)
#pragma unroll
        for (int h = 0; h < KH; ++h) asm volatile("" : "+v"(col[j0 + g][h]));
#pragma unroll
      for (int g = 0; g < G; ++g) {
        acc[g] = 0u;
#pragma unroll
        for (int h = 0; h < KH; ++h) {
          acc[g] |= *reinterpret_cast<const M*>(lbase + cur_off + (col[j0 + g][h] & 0xFFFFu) * (kE / kC));
          if (2 * h + 1 < K)
            acc[g] |= *reinterpret_cast<const M*>(lbase + cur_off + (col[j0 + g][h] >> 16) * (kE / kC));
        }
      }
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const int j = j0 + g;
        const uint32_t v = j * B + me;
        V nx = 0u;
        if (vis[j] != full) {  // also every v >= N
          if ((ovfm >> j) & 1u) {
            const uint2 last = a.recs[static_cast<size_t>(v) * K + K - 1];
            const uint2* ov = a.recs + (last.x & ORH_REC_COL_MASK);
            for (uint32_t q = 0; q < last.y; ++q) {
              const uint32_t r = ov[q].x;
              if (!(r & ORH_REC_SKIP)) acc[g] |= f_cur[r & ORH_REC_COL_MASK];
            }
          }
          nx = acc[g] & ~vis[j];
          vis[j] |= nx;
        }
#ifdef ORH_DIAG_STAMPS
        const uint64_t t_s0 = __builtin_amdgcn_s_memtime();
#endif
        bool any = false;  // wave-uniform: the slice has an arrival
#ifndef ORH_EXP_NO_LVL_STORE  // timing experiment only: drops the level bytes
        if (kLog) any = log_events(j, nx, level);
#endif
        if (kAdj && !kLog) any = __builtin_amdgcn_ballot_w64(nx != 0u) != 0u;
        if constexpr (kAdj) jm |= (any ? 1u : 0u) << j;
        if (nx) {
          prog = 1;
#ifndef ORH_EXP_NO_LVL_STORE
          {
          uint8_t* lb = lvl + static_cast<size_t>(v) * kS;
          if (level < kLvlDirect) {
            if (!kLog)
              for (V q = nx; q; q &= q - 1) lb[MsMask<M>::ctz(q)] = static_cast<uint8_t>(level);
          } else {  // deep levels: the distance row directly (the level byte says so)
            const uint32_t vh = a.host_of[v];
            for (V q = nx; q; q &= q - 1) {
              const uint32_t b = MsMask<M>::ctz(q);
              if (!kLog) lb[b] = kLvlDirect;
              dist_row(a.out_dist, a.scratch, a.n_out, N, a.order[b0 + b])[vh] = level * w0;
            }
          }
          }
#endif
        }
#ifdef ORH_DIAG_STAMPS
        t_store += __builtin_amdgcn_s_memtime() - t_s0;
#endif
        if ((ovlm >> j) & 1u) nx = 0u;  // reached, but no transit through an overloaded node
        // only a node with new bits writes its entry: whatever an entry still
        // holds from an older level (bits that reached it at level L - 2k)
        // reached every neighbour by level L - 2k + 1, so the pull masks it
        // with the neighbour's visited bits. Writing the zeros (every open
        // node, every level) was ~1/3 of the loop's LDS cycles
        if (nx) f_nxt[v] = static_cast<M>(nx);
        if constexpr (kSkip) jm |= (__builtin_amdgcn_ballot_w64(nx != 0u) != 0u ? 1u : 0u) << j;
      }
    }
    if constexpr (kAdj) {  // this wave's slices with an arrival into the level's marks: lane j, slice j
      const uint32_t ln = me & 63u;
      if (ln < static_cast<uint32_t>(J) && ((jm >> ln) & 1u)) {
        const uint32_t sl = ln * (B >> 6) + (me >> 6);
        atomicOr(&s_act[level % 3u][sl >> 5], 1u << (sl & 31u));
      }
    }
    if constexpr (kSkip) {  // this wave's new-frontier slices into the level's interval
      if (jm && (tid & 63u) == 0) {
        const uint32_t jl = static_cast<uint32_t>(__builtin_ctz(jm));
        const uint32_t jh = 31u - static_cast<uint32_t>(__builtin_clz(jm));
        atomicMin(&s_lo[level % 3u], jl * B + wave_base);
        atomicMin(&s_hin[level % 3u], ~(jh * B + wave_base + 63u));
      }
    }
    // every level that makes progress adds >= 1 visited bit: at most S * N
    // levels. The barrier waits for LDS traffic only: the level bytes on
    // their way to memory are read by the next kernel, and waiting for their
    // write acknowledgements every level (what __syncthreads does) is wasted.
    if (prog) s_prog[level % 3u] = 1u;
#ifdef ORH_DIAG_STAMPS
    const uint64_t t_b0 = __builtin_amdgcn_s_memtime();
#endif
    lds_barrier();
#ifdef ORH_DIAG_STAMPS
    t_bar += __builtin_amdgcn_s_memtime() - t_b0;
    ++n_levels;
#endif
    const uint32_t progressed = s_prog[level % 3u];
    if constexpr (kAdj) act = s_act[level % 3u][me & 7u];
    if (!progressed) break;
    if (tid == 0) s_prog[(level + 2u) % 3u] = 0u;  // the previous level's flag, read before this barrier
    M* t = f_cur;
    f_cur = f_nxt;
    f_nxt = t;
    const uint32_t to = cur_off;
    cur_off = nxt_off;
    nxt_off = to;
  }
  // for the lean first-hop kernel: the rows of this batch may hold kLvlDirect
  // bytes iff its last level with an arrival (level - 1) got that far; every
  // output path below shares this one store. Workgroup 0 also empties that
  // kernel's redo list
  if (a.row_deep && tid < S) a.row_deep[a.order[b0 + tid]] = level > kLvlDirect ? 1u : 0u;
  if (a.hop_redo_count && blockIdx.x == 0 && tid == 0) *a.hop_redo_count = 0u;
  if constexpr (kLog) {
    // the logs -> node-major level blocks, one wave's nodes at a time: the
    // workgroup zeroes their J * 64 blocks in LDS (the frontier arrays are
    // free once every wave has left the level loop), scatters the wave's
    // events into them (loads in flight eight at a time) and writes the
    // blocks out whole, 16 bytes a thread
    if (lane == 0) s_wcnt[wave] = wcnt;
    __shared__ uint32_t s_row[kS];
    if (tid < S) s_row[tid] = a.order[b0 + tid];
    __syncthreads();
    // node blocks padded to kS + 4 bytes: consecutive blocks start 9 (kS =
    // 32) or 5 (kS = 16) banks apart, so the scattered byte writes of a wave
    // spread over the banks instead of 8 blocks sharing one
    constexpr uint32_t kP = kS + 4, kQ = kS / 16;
    uint8_t* blk = reinterpret_cast<uint8_t*>(lds);
    const uint32_t nw32 = J * 64u * kP / 4u;
    for (uint32_t w = 0; w < waves; ++w) {
      for (uint32_t i = tid; i < nw32; i += B) lds[i] = ~0u;
      __syncthreads();
      const uint32_t n_ev = s_wcnt[w];
      const uint64_t* wl = a.ms_log + (static_cast<size_t>(blockIdx.x) * waves + w) * J * 64u * kS;
      for (uint32_t e0 = tid; e0 < n_ev; e0 += 8u * B) {
        uint64_t x[8];
#pragma unroll
        for (uint32_t u = 0; u < 8; ++u) x[u] = e0 + u * B < n_ev ? wl[e0 + u * B] : 0ull;
#pragma unroll
        for (uint32_t u = 0; u < 8; ++u) {
          uint8_t* nb = blk + ((static_cast<uint32_t>(x[u]) >> 8) & 0x7FFu) * kP;  // (j * 64 + lane) * kP
          const uint8_t lv = static_cast<uint8_t>(x[u] & 0xFFu);
          // (the first two bits of an event decoded straight-line ahead of this
          // loop: 19.49 against 19.56 ms per step in cluster order, inside the
          // run-to-run range - profiles/ms_cluster/step_ab.txt)
          for (V q = static_cast<V>(x[u] >> 32); q; q &= q - 1) nb[MsMask<M>::ctz(q)] = lv;
        }
      }
      __syncthreads();
      if (a.ms_direct) {
        // host-order layout: the wave's slice j is the host ids j * B + w * 64
        // + [0, 64), so each source's row gets 64 consecutive levels - the
        // u8 level row and the u32 distance row written here, coalesced (a
        // thread: 4 nodes of one source; 16 threads: one 64-node run). The
        // padding [N, lvl_pitch) of the level rows is "unreached" (no event
        // lands there). Deep levels (marker 254) were written during the search
        const uint32_t P = a.lvl_pitch, w0 = a.w0, nq = J * 16u;
        for (uint32_t i = tid; i < S * nq; i += B) {
          const uint32_t b = i / nq, jq = i % nq;
          const uint32_t j = jq >> 4, n0 = j * 64u + (jq & 15u) * 4u;
          const uint32_t v0 = j * B + w * 64u + (jq & 15u) * 4u;
          if (v0 >= P) continue;
          const uint8_t* nb = blk + n0 * kP + b;
          const uint32_t l[4] = {nb[0], nb[kP], nb[2 * kP], nb[3 * kP]};
          const uint32_t r = s_row[b];
          *reinterpret_cast<uint32_t*>(a.lvl_rows + static_cast<size_t>(r) * P + v0) =
              l[0] | (l[1] << 8) | (l[2] << 16) | (l[3] << 24);
          if (r >= a.n_out || v0 >= N) continue;  // a neighbour row is read through its level row
          uint32_t d[4];
          bool deep = false;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            d[k] = l[k] == kLvlNone ? kInf : l[k] * w0;
            deep |= l[k] == kLvlDirect;
          }
          uint32_t* od = a.out_dist + static_cast<size_t>(r) * N + v0;
          if (!deep && v0 + 4u <= N && (reinterpret_cast<uintptr_t>(od) & 15u) == 0u) {
            typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
            const u32x4 q = {d[0], d[1], d[2], d[3]};
            __builtin_nontemporal_store(q, reinterpret_cast<u32x4*>(od));
          } else {
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k)
              if (v0 + k < N && l[k] != kLvlDirect) __builtin_nontemporal_store(d[k], od + k);
          }
        }
      } else {
        for (uint32_t i = tid; i < J * 64u * kQ; i += B) {
          const uint32_t node = i / kQ, q = i % kQ;  // node = j * 64 + lane
          const uint32_t v = (node >> 6) * B + w * 64u + (node & 63u);
          const uint32_t* src = lds + node * (kP / 4u) + q * 4u;
          if (v < N)
            reinterpret_cast<uint4*>(lvl + static_cast<size_t>(v) * kS)[q] = make_uint4(src[0], src[1], src[2], src[3]);
        }
      }
      __syncthreads();
    }
  }
#ifdef ORH_DIAG_STAMPS
  if (tid == 0 && blockIdx.x < 4096) {  // per workgroup: entry, exit, hardware id, levels
    uint64_t* w = a.diag + 16 + 4 * static_cast<size_t>(blockIdx.x);
    w[0] = t_entry;
    w[1] = __builtin_amdgcn_s_memtime();
    w[2] = static_cast<uint64_t>(__builtin_amdgcn_s_getreg(0xF804)) |
           (static_cast<uint64_t>(__builtin_amdgcn_s_getreg(0xF814)) << 32);
    w[3] = n_levels;
  }
  if ((tid & 63u) == 0) {  // per wave: total, barrier and store-block cycles, levels
    const uint64_t tot = __builtin_amdgcn_s_memtime() - t_begin;
    atomicAdd(reinterpret_cast<unsigned long long*>(&a.diag[0]), tot);
    atomicAdd(reinterpret_cast<unsigned long long*>(&a.diag[1]), t_bar);
    atomicAdd(reinterpret_cast<unsigned long long*>(&a.diag[3]), static_cast<unsigned long long>(n_levels));
    atomicAdd(reinterpret_cast<unsigned long long*>(&a.diag[4]), 1ull);
    atomicMax(reinterpret_cast<unsigned long long*>(&a.diag[5]), tot);
    atomicMax(reinterpret_cast<unsigned long long*>(&a.diag[6]), static_cast<unsigned long long>(n_levels));
    atomicAdd(reinterpret_cast<unsigned long long*>(&a.diag[8]), t_store);
  }
#endif
}

// node-major level bytes -> host-order u32 distance rows, one workgroup per
// (batch, 256-node host tile); per source bit b the 256 stores of a row are
// contiguous. kDist = false: the u8 level rows alone (an 8-bit transpose);
// the first-hop pass, which loads each source's level bytes anyway, writes
// the u32 rows from them (HopArgs::write_dist)
template <class M, bool kDist>
__global__ __launch_bounds__(256) void ms_finalize_kernel(SpfArgs a, uint32_t tiles) {
  constexpr uint32_t kS = MsMask<M>::kS;
  __shared__ uint32_t* s_out[kS];
  __shared__ uint32_t s_row[kS];
  const uint32_t N = a.n_nodes;
  const uint32_t batch = blockIdx.x / tiles, tile = blockIdx.x % tiles;
  const uint32_t i = tile * 256 + threadIdx.x;
  const uint32_t b0 = batch * a.ms_width;
  const uint32_t S = min(a.ms_width, a.n_rows - b0);
  if (threadIdx.x < S) {
    s_row[threadIdx.x] = a.order[b0 + threadIdx.x];
    if (kDist) s_out[threadIdx.x] = dist_row(a.out_dist, a.scratch, a.n_out, N, s_row[threadIdx.x]);
  }
  __syncthreads();
  if (i >= N) {  // level-row padding [N, pitch): "unreached" for the 16-byte reads
    if (i < a.lvl_pitch)
      for (uint32_t b = 0; b < S; ++b)
        a.lvl_rows[static_cast<size_t>(s_row[b]) * a.lvl_pitch + i] = static_cast<uint8_t>(kLvlNone);
    return;
  }
  const uint32_t v = a.dev_of[i];
  const uint4* blk = reinterpret_cast<const uint4*>(a.ms_lvl + (static_cast<size_t>(batch) * N + v) * kS);
  uint32_t w[kS / 4];
#pragma unroll
  for (int q = 0; q < static_cast<int>(kS / 16); ++q) {
    const uint4 x = blk[q];
    w[4 * q] = x.x;
    w[4 * q + 1] = x.y;
    w[4 * q + 2] = x.z;
    w[4 * q + 3] = x.w;
  }
  const uint32_t w0 = a.w0;
#pragma unroll
  for (uint32_t b = 0; b < kS; ++b) {
    if (b >= S) break;
    const uint32_t l = (w[b / 4] >> ((b & 3u) * 8u)) & 0xFFu;
    const uint32_t r = s_row[b];
    a.lvl_rows[static_cast<size_t>(r) * a.lvl_pitch + i] = static_cast<uint8_t>(l);
    // neighbour-only rows are read through their level row
    if (!kDist || l == kLvlDirect || r >= a.n_out) continue;
    __builtin_nontemporal_store(l == kLvlNone ? kInf : l * w0, &s_out[b][i]);
  }
}

template <int K, class M, int J>
static hipError_t launch_ms_j(const SpfPlan& plan, const SpfArgs& a, uint32_t n_rows, hipStream_t s) {
  if (a.ms_width == 0 || a.ms_width > MsMask<M>::kS) return hipErrorInvalidValue;
  const uint32_t batches = (n_rows + a.ms_width - 1) / a.ms_width;
  // the log's block assembly reuses the frontier arrays' LDS: one wave's
  // J * 64 node blocks at a time
  size_t lds = plan.lds_bytes;
  if (sizeof(M) <= 4) {
    if (!a.ms_log) return hipErrorInvalidValue;
    lds = std::max<size_t>(lds, size_t{J} * 64 * (MsMask<M>::kS + 4));
  }
  const SpfArgs& b = a;
  if (a.ms_bw)
    return launch(spf_msbfs_kernel<K, M, J, kMsSkipInterval>, b, batches, plan.block, lds, s);
  if (a.ms_adj)
    return launch(spf_msbfs_kernel<K, M, J, kMsSkipAdj>, b, batches, plan.block, lds, s);
  return launch(spf_msbfs_kernel<K, M, J, kMsSkipNone>, b, batches, plan.block, lds, s);
}

template <int K, class M>
static hipError_t launch_ms_m(const SpfPlan& plan, const SpfArgs& a, uint32_t n_rows, hipStream_t s) {
  switch (plan.ms_j) {
    case 4: return launch_ms_j<K, M, 4>(plan, a, n_rows, s);
    case 8: return launch_ms_j<K, M, 8>(plan, a, n_rows, s);
    case 12: return launch_ms_j<K, M, 12>(plan, a, n_rows, s);
    case 16: return launch_ms_j<K, M, 16>(plan, a, n_rows, s);
    case 20: return launch_ms_j<K, M, 20>(plan, a, n_rows, s);
    case 24: return launch_ms_j<K, M, 24>(plan, a, n_rows, s);
    case 28: return launch_ms_j<K, M, 28>(plan, a, n_rows, s);
    case 32: return launch_ms_j<K, M, 32>(plan, a, n_rows, s);
    default: return hipErrorInvalidValue;
  }
}

template <int K>
static hipError_t launch_ms_k(const SpfPlan& plan, const SpfArgs& a, uint32_t n_rows, hipStream_t s) {
  switch (plan.mask_bytes) {
    case 2: return launch_ms_m<K, uint16_t>(plan, a, n_rows, s);
    case 4: return launch_ms_m<K, uint32_t>(plan, a, n_rows, s);
    case 8: return launch_ms_m<K, uint64_t>(plan, a, n_rows, s);
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_ms(const SpfPlan& plan, const SpfArgs& a, uint32_t n_rows, hipStream_t s) {
  return plan.ell_k == 8 ? launch_ms_k<8>(plan, a, n_rows, s) : launch_ms_k<4>(plan, a, n_rows, s);
}

size_t ms_log_bytes(const SpfPlan& plan, uint32_t n_rows) {
  if (plan.variant != SpfVariant::kMsBfs || plan.ms_width == 0 || plan.mask_bytes > 4) return 0;
  const size_t batches = (n_rows + plan.ms_width - 1) / plan.ms_width;
  return batches * plan.ms_j * plan.block * (plan.mask_bytes * 8) * sizeof(uint64_t);
}

size_t ms_scratch_bytes(const SpfPlan& plan, uint32_t n_nodes, uint32_t n_rows) {
  if (plan.variant != SpfVariant::kMsBfs || plan.ms_width == 0) return 0;
  const uint32_t w = plan.ms_width;
  return static_cast<size_t>((n_rows + w - 1) / w) * n_nodes * (plan.mask_bytes * 8);
}

void ms_set_width(SpfPlan& plan, uint32_t n_nodes, uint32_t n_rows, uint32_t n_cu, size_t lds_limit,
                  bool alone) {
  if (plan.variant != SpfVariant::kMsBfs) return;
  plan.ms_width = plan.mask_bytes * 8;
  // ORH_MS_WIDE=1 (opt-in): when u32 masks need more than one batch per CU
  // and u64 frontier arrays fit in LDS, widen the masks and spread the rows
  // over at most n_cu batches of ceil(n_rows / n_cu) sources. On C2 (250
  // batches of 40) this swept in 0.86-0.92 ms against 0.75 for 313 u32
  // batches: the batches that share a CU are not the slow ones
  // (per-workgroup stamps, profiles/r02/msbfs_ab.md), and u64 masks cost more
  // per level than they save
  // latency plan: when every batch has a CU to itself (a sweep over a shard
  // of the sources, N GPUs sharing one topology), the per-level time of one
  // workgroup is the sweep time, so the batch gets 1024 threads (fewer nodes
  // per thread: J = 12 instead of 20 on the 10k grid). ORH_MS_LATENCY=0: off;
  // ORH_MS_LATENCY=2: with the interval skip as well (it cuts a lone C2
  // corner batch 0.48 -> 0.32 ms, profiles/r02/msbfs_ab.md, but a C2 shard of
  // 1,254 sources measured 0.785 vs 0.748 ms with it, profiles/r04/
  // f_strong_rehearsal_skip.txt vs e_strong_rehearsal.txt)
  plan.ms_skip = 0;
  plan.ms_own_cu = 0;
  const LaunchKnobs knobs = launch_knobs();
  {
    const bool plans = knobs.ms_latency != 0 && !knobs.ms_block_set;
    const uint32_t batches = (n_rows + plan.mask_bytes * 8 - 1) / (plan.mask_bytes * 8);
    const uint32_t j = (n_nodes + 1023) / 1024;
    if (plans && n_cu && batches <= n_cu && plan.block < 1024 && j <= 32) {
      plan.block = 1024;
      plan.ms_j = (j + 3) & ~3u;
      plan.ms_skip = knobs.ms_latency == 2;
      // a batch alone on its CU is bound by the per-level latency chain, which
      // the adjacency skip lengthens (its marks are read after the barrier)
      // and skipped gathers do not shorten: the C5 area graph swept in 0.122
      // against 0.111 ms with it, the 70 x 70 grid in 0.227 against 0.215
      // (profiles/ms_adj/order_ab.txt), so this plan leaves it off
      plan.ms_own_cu = 1;
    } else if (plans && alone && plan.block == 512) {
      // lone-sweep plan: no other sweep in flight on the device, so the
      // batches do not share CUs with other streams' kernels and 12 waves
      // per batch cut the per-level time (one C2 sweep 0.82 -> 0.68 ms of
      // MS-BFS); under concurrent sweeps 8 waves stay (the 4-lane step
      // 24.8 vs 26.3 ms at 12, profiles/r04/ai_ms_block_ab.txt). The plan
      // needs two 12-wave batches on a CU, 6 waves per SIMD, 80 VGPRs: the
      // adjacency variant's J = 16 takes 81, one batch per CU, and the lone
      // C2 sweep ran 1.08 against 0.95 ms with it (profiles/ms_adj/
      // lone_ab.txt), so this plan leaves the adjacency skip off too
      const uint32_t j12 = (n_nodes + 767) / 768;
      if (j12 <= 32) {
        plan.ms_own_cu = 1;
        plan.block = 768;
        plan.ms_j = (j12 + 3) & ~3u;
      }
    }
  }
  const size_t bytes64 = 2 * 8 * static_cast<size_t>(plan.ms_pitch);
  if (knobs.ms_wide && plan.mask_bytes == 4 && n_cu && n_rows > 32ull * n_cu && bytes64 <= lds_limit &&
      4ull * plan.ms_pitch <= 65536) {
    plan.mask_bytes = 8;
    plan.lds_bytes = bytes64;
    plan.ms_width = std::min<uint32_t>(64, (n_rows + n_cu - 1) / n_cu);
  }
}

template <bool kDist>
static void launch_ms_finalize_as(const SpfPlan& plan, const SpfArgs& a, uint32_t grid, uint32_t tiles,
                                  hipStream_t s) {
  if (plan.mask_bytes == 2)
    hipLaunchKernelGGL((ms_finalize_kernel<uint16_t, kDist>), dim3(grid), dim3(256), 0, s, a, tiles);
  else if (plan.mask_bytes == 4)
    hipLaunchKernelGGL((ms_finalize_kernel<uint32_t, kDist>), dim3(grid), dim3(256), 0, s, a, tiles);
  else
    hipLaunchKernelGGL((ms_finalize_kernel<uint64_t, kDist>), dim3(grid), dim3(256), 0, s, a, tiles);
}

hipError_t launch_ms_finalize(const SpfPlan& plan, SpfArgs a, uint32_t n_rows, hipStream_t s,
                              bool write_dist) {
  if (plan.variant != SpfVariant::kMsBfs || n_rows == 0) return hipErrorInvalidValue;
  a.n_rows = n_rows;
  if (a.ms_width == 0 || a.ms_width > plan.mask_bytes * 8) return hipErrorInvalidValue;
  const uint32_t batches = (n_rows + a.ms_width - 1) / a.ms_width;
  const uint32_t tiles = (a.n_nodes + 255) / 256;
  if (write_dist)
    launch_ms_finalize_as<true>(plan, a, batches * tiles, tiles, s);
  else
    launch_ms_finalize_as<false>(plan, a, batches * tiles, tiles, s);
  return hipGetLastError();
}

}  // namespace orh
