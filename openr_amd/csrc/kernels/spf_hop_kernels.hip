// Phase 2 of the two-phase SPF plans: first-hop masks from distance rows or
// (multi-source BFS plans) u8 level rows.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "spf_device.h"
#include "spf_launch.h"

namespace orh {

// ---------------------------------------------------------------------------
// phase 2: first-hop masks
// ---------------------------------------------------------------------------
// distance of node x in row `row`: the u32 distance row, or (multi-source
// plans) the u8 level row scaled by w0
template <bool kLvl>
__device__ inline uint32_t hop_dist(const HopArgs& a, uint32_t row, uint32_t x) {
  const uint32_t* dr = dist_row(const_cast<uint32_t*>(a.dist), const_cast<uint32_t*>(a.scratch),
                                a.n_out, a.n_nodes, row);
  if (!kLvl) return dr[x];
  const uint32_t l = a.lvl_rows[static_cast<size_t>(row) * a.lvl_pitch + x];
  return l == kLvlNone ? kInf : l == kLvlDirect ? dr[x] : l * a.w0;
}

// the source's tight first links into LDS: ent[k] = {n, d_s(n), n's row,
// rank | 0x80000000 if n is overloaded}; returns the count. LDS layout:
// minw[nb] | node[nb] | ent[nb] (hop_lds_bytes)
template <bool kLvl>
__device__ inline uint32_t hop_entries(const HopArgs& a, uint32_t i, uint32_t* lds, uint32_t* s_cnt) {
  const uint32_t tid = threadIdx.x;
  const uint32_t src = a.srcs[i];
  const uint32_t nb0 = a.nbr_ptr[i], nb = a.nbr_ptr[i + 1] - nb0;
  uint32_t* minw = lds;
  uint32_t* node = lds + nb;
  uint4* ent = reinterpret_cast<uint4*>(lds + ((2 * nb + 3) & ~3u));
  const uint32_t* ign = nullptr;
  uint32_t n_ign = 0;
  if (a.ignore_ptr) {
    ign = a.ignore_links + a.ignore_ptr[i];
    n_ign = a.ignore_ptr[i + 1] - a.ignore_ptr[i];
  }

  for (uint32_t r = tid; r < nb; r += kBlock) minw[r] = kInf;
  if (tid == 0) *s_cnt = 0;
  __syncthreads();
  // the source's links: smallest live metric per distinct neighbour
  const uint32_t K = a.ell_k;
  auto consider = [&](uint32_t q) {
    const uint2 r = a.recs[q];
    if (r.x & (ORH_REC_SKIP | ORH_REC_CONT)) return;
    if (n_ign && ignored(ign, n_ign, a.link[q])) return;
    const uint32_t rk = a.rank_out[q];
    atomicMin(&minw[rk], a.use_link_metric ? r.y : 1u);
    node[rk] = r.x & ORH_REC_COL_MASK;
  };
  for (uint32_t j = tid; j < K; j += kBlock) consider(src * K + j);
  const uint2 last = a.recs[static_cast<size_t>(src) * K + K - 1];
  if (last.x & ORH_REC_CONT)
    for (uint32_t j = tid; j < last.y; j += kBlock) consider((last.x & ORH_REC_COL_MASK) + j);
  __syncthreads();
  // tight first links: d_s(n) equals the cheapest live link to n
  for (uint32_t r = tid; r < nb; r += kBlock) {
    if (minw[r] == kInf) continue;
    const uint32_t u = node[r];
    const uint32_t du = hop_dist<kLvl>(a, i, u);
    if (du != minw[r]) continue;
    const uint32_t k = atomicAdd(s_cnt, 1u);
    ent[k] = make_uint4(u, du, a.nbr_row[nb0 + r], r | (a.overloaded[u] ? 0x80000000u : 0u));
  }
  __syncthreads();
  return *s_cnt;
}

__global__ __launch_bounds__(kBlock) void first_hop_kernel(HopArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  __shared__ uint32_t s_cnt;
  const uint32_t N = a.n_nodes;
  const uint32_t tid = threadIdx.x;
  // XCD-aware order (opt-in, ORH_HOP_XCD=1): an XCD runs a contiguous range
  // of sources, so the neighbour rows its sources share would be read
  // through its own L2; measured slower on the C2w sweep (0.395 vs 0.372 ms,
  // profiles/r06/ah_hop_xcd_ab.txt): a source's tiles spread over the XCDs
  // balance better than the L2 reuse pays
  const uint32_t lb = a.xcd_hop ? xcd_block(blockIdx.x, gridDim.x, a.xcd_group) : blockIdx.x;
  const uint32_t i = lb / a.tiles, tile = lb % a.tiles;
  const uint32_t src = a.srcs[i];
  const uint32_t nb = a.nbr_ptr[i + 1] - a.nbr_ptr[i];
  const uint4* ent = reinterpret_cast<const uint4*>(lds + ((2 * nb + 3) & ~3u));
  const uint32_t ne = hop_entries<false>(a, i, lds, &s_cnt);
  const uint32_t* ds = dist_row(const_cast<uint32_t*>(a.dist), const_cast<uint32_t*>(a.scratch),
                                a.n_out, N, i);


  uint32_t v[kHopPer], dv[kHopPer];
#pragma unroll
  for (int k = 0; k < kHopPer; ++k) {
    v[k] = tile * (kBlock * kHopPer) + k * kBlock + tid;
    dv[k] = v[k] < N ? ds[v[k]] : kInf;
    if (v[k] == src) dv[k] = kInf;  // the source has no next hops
  }
  const uint32_t W = a.words;
  uint32_t* nh = a.out_nh + static_cast<size_t>(i) * N * W;
  for (uint32_t word = 0; word < W; ++word) {
    uint32_t acc[kHopPer] = {};
    for (uint32_t e = 0; e < ne; ++e) {
      const uint4 en = ent[e];
      const uint32_t r = en.w & 0x7FFFFFFFu;
      if ((r >> 5) != word) continue;
      const uint32_t bit = 1u << (r & 31u);
      const bool transit = !(en.w & 0x80000000u);
      const uint32_t* dr = dist_row(const_cast<uint32_t*>(a.dist),
                                    const_cast<uint32_t*>(a.scratch), a.n_out, N, en.z);
      uint32_t x[kHopPer];
#pragma unroll
      for (int k = 0; k < kHopPer; ++k) x[k] = (transit && dv[k] != kInf) ? dr[v[k]] : kInf;
#pragma unroll
      for (int k = 0; k < kHopPer; ++k) {
        if (dv[k] == kInf) continue;
        if (v[k] == en.x ||
            (x[k] != kInf && static_cast<uint64_t>(en.y) + x[k] == dv[k]))
          acc[k] |= bit;
      }
    }
#pragma unroll
    for (int k = 0; k < kHopPer; ++k)
      if (v[k] < N) __builtin_nontemporal_store(acc[k], &nh[static_cast<size_t>(v[k]) * W + word]);
  }
}

// first hops of multi-source BFS rows: the same closed form over u8 level
// rows (pitch a multiple of 16), P consecutive nodes per thread so every row
// access is one P-byte load (P = 16 for large batches; 4 keeps small ones
// spread over more workgroups)
template <uint32_t P>
struct LvlVec;
template <>
struct LvlVec<16> {
  typedef uint4 T;
  __device__ static uint32_t byte(const uint4& x, uint32_t k) {
    const uint32_t w = k < 4 ? x.x : k < 8 ? x.y : k < 12 ? x.z : x.w;
    return (w >> ((k & 3u) * 8u)) & 0xFFu;
  }
};
template <>
struct LvlVec<8> {
  typedef uint2 T;
  __device__ static uint32_t byte(const uint2& x, uint32_t k) { return ((k < 4 ? x.x : x.y) >> ((k & 3u) * 8u)) & 0xFFu; }
};
template <>
struct LvlVec<4> {
  typedef uint32_t T;
  __device__ static uint32_t byte(const uint32_t& x, uint32_t k) { return (x >> (k * 8u)) & 0xFFu; }
};

__device__ inline bool has_byte_fe(uint32_t x) {  // some byte == kLvlDirect
  const uint32_t z = x ^ 0xFEFEFEFEu;
  return ((z - 0x01010101u) & ~z & 0x80808080u) != 0u;
}

// One workgroup per (source, tile phase): the source's tight first links are
// gathered once, then the workgroup walks tiles phase, phase + split, ...
// kList: the sources a.redo_list[0, *a.redo_count) instead of all (the ones
// first_hop_lean_kernel left), any grid striding over them
template <uint32_t kLvlPer, bool kList = false>
__global__ __launch_bounds__(kBlock) void first_hop_lvl_kernel(HopArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  __shared__ uint32_t s_cnt;
  typedef typename LvlVec<kLvlPer>::T Vec;
  constexpr uint32_t kWords = kLvlPer / 4;
  const uint32_t N = a.n_nodes, P = a.lvl_pitch, w0 = a.w0;
  const uint32_t tid = threadIdx.x;
  const uint32_t split = a.tile_split;
  // one logical block per workgroup, or (persistent grid, a multiple of the
  // 8 XCDs; ORH_HOP_WG_PER_CU) XCD x = b % 8 owns a contiguous logical range
  // its workgroups stride through
  uint32_t lb, lb_end, lb_step;
  if constexpr (kList) {
    lb = blockIdx.x;
    lb_end = *a.redo_count * split;
    lb_step = gridDim.x;
  } else if (gridDim.x >= a.n_logical) {
    lb = xcd_block(blockIdx.x, gridDim.x, a.xcd_group);
    lb_end = lb + 1;
    lb_step = 1;
  } else {
    constexpr uint32_t kXcd = 8;
    const uint32_t x = blockIdx.x % kXcd, k = blockIdx.x / kXcd;
    const uint32_t q = a.n_logical / kXcd, r = a.n_logical % kXcd;
    const uint32_t lo = x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q;
    lb = lo + k;
    lb_end = lo + q + (x < r ? 1u : 0u);
    lb_step = gridDim.x / kXcd;
  }
  for (; lb < lb_end; lb += lb_step) {
  const uint32_t i = kList ? a.redo_list[lb / split] : lb / split, phase = lb % split;
  const uint32_t src = a.srcs[i];
  const uint32_t nb = a.nbr_ptr[i + 1] - a.nbr_ptr[i];
  const uint4* ent = reinterpret_cast<const uint4*>(lds + ((2 * nb + 3) & ~3u));
  const uint32_t ne = hop_entries<true>(a, i, lds, &s_cnt);
  const uint32_t W = a.words;
  uint32_t* nh = a.out_nh + static_cast<size_t>(i) * N * W;
  for (uint32_t tile = phase; tile < a.tiles; tile += split) {
    const uint32_t v0 = (tile * kBlock + tid) * kLvlPer;
    if (v0 >= N) break;
    auto dist_at = [&](uint32_t row, const Vec& x, uint32_t k) -> uint32_t {
      const uint32_t l = LvlVec<kLvlPer>::byte(x, k);
      if (l == kLvlNone) return kInf;
      if (l == kLvlDirect)
        return dist_row(const_cast<uint32_t*>(a.dist), const_cast<uint32_t*>(a.scratch), a.n_out,
                        N, row)[v0 + k];
      return l * w0;
    };
    auto words_of = [](const Vec& x, uint32_t (&w)[kWords]) {
      if constexpr (kLvlPer == 16) {
        w[0] = x.x; w[1] = x.y; w[2] = x.z; w[3] = x.w;
      } else if constexpr (kLvlPer == 8) {
        w[0] = x.x; w[1] = x.y;
      } else {
        w[0] = x;
      }
    };
    const Vec own = *reinterpret_cast<const Vec*>(a.lvl_rows + static_cast<size_t>(i) * P + v0);
    uint32_t ow[kWords];
    words_of(own, ow);
    bool own_direct = false;
#pragma unroll
    for (uint32_t q = 0; q < kWords; ++q) own_direct |= has_byte_fe(ow[q]);
    if (a.write_dist) {
      // the source's own distance row from the level bytes just loaded (the
      // level-only ms_finalize_kernel left it unwritten): once per tile, the
      // source's own entry included (level 0). kLvlDirect entries are skipped:
      // the search kernel wrote them, and dist_at / hop_entries read exactly
      // those entries of this row back - no other, so a thread never reads an
      // entry this kernel writes
      uint32_t* od = dist_row(const_cast<uint32_t*>(a.dist), const_cast<uint32_t*>(a.scratch), a.n_out,
                              N, i) + v0;
      auto dist_of = [&](uint32_t k) -> uint32_t {
        const uint32_t l = (ow[k / 4] >> ((k & 3u) * 8u)) & 0xFFu;
        return l == kLvlNone ? kInf : l * w0;
      };
      if (!own_direct && v0 + kLvlPer <= N && (reinterpret_cast<uintptr_t>(od) & 15u) == 0u) {
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
#pragma unroll
        for (uint32_t q = 0; q < kWords; ++q) {
          const u32x4 x = {dist_of(4 * q), dist_of(4 * q + 1), dist_of(4 * q + 2), dist_of(4 * q + 3)};
          __builtin_nontemporal_store(x, reinterpret_cast<u32x4*>(od) + q);
        }
      } else {
#pragma unroll
        for (uint32_t k = 0; k < kLvlPer; ++k)
          if (v0 + k < N && ((ow[k / 4] >> ((k & 3u) * 8u)) & 0xFFu) != kLvlDirect)
            __builtin_nontemporal_store(dist_of(k), od + k);
      }
    }
    // d_s(v0 + k) where needed (the direct path; kInf: the source, which has
    // no next hops, and the padding past N) - not held for all k (VGPRs)
    auto own_dist = [&](uint32_t k) -> uint32_t {
      return (v0 + k == src || v0 + k >= N) ? kInf : dist_at(i, own, k);
    };
    // own level bytes with the source's byte forced to "unreached" (no next
    // hops; bytes past N are the row padding, unreached already)
    uint32_t ot[kWords];
#pragma unroll
    for (uint32_t q = 0; q < kWords; ++q) ot[q] = ow[q];
    if (src >= v0 && src < v0 + kLvlPer) {
#pragma unroll
      for (uint32_t q = 0; q < kWords; ++q)
        if ((src - v0) / 4u == q) ot[q] |= 0xFFu << (((src - v0) & 3u) * 8u);
    }
    for (uint32_t word = 0; word < W; ++word) {
      uint32_t acc[kLvlPer] = {};
      uint32_t pk[kWords] = {};  // byte k of word q: mask bits 0..7 of node 4q + k (packed path)
      // the neighbour rows of kGroup entries are loaded back to back before
      // any is used: one memory round trip per group, not per entry (the
      // loads of a dynamic-length loop are otherwise issued one at a time)
      constexpr uint32_t kGroup = 4;  // (1: one entry per round trip, the round-3 loop)
      for (uint32_t e0 = 0; e0 < ne; e0 += kGroup) {
      uint4 ens[kGroup];
      Vec nxs[kGroup];
      uint32_t use = 0;  // bit g: entry e0 + g belongs to this word
#pragma unroll
      for (uint32_t g = 0; g < kGroup; ++g) {
        if (e0 + g >= ne) break;
        ens[g] = ent[e0 + g];
        if (((ens[g].w & 0x7FFFFFFFu) >> 5) != word) continue;
        use |= 1u << g;
        if (!(ens[g].w & 0x80000000u))
          nxs[g] = *reinterpret_cast<const Vec*>(a.lvl_rows + static_cast<size_t>(ens[g].z) * P + v0);
      }
#pragma unroll
      for (uint32_t g = 0; g < kGroup; ++g) {
        if (!((use >> g) & 1u)) continue;
        const uint4 en = ens[g];
        const uint32_t r = en.w & 0x7FFFFFFFu;
        const uint32_t bit = 1u << (r & 31u);
        if (en.x >= v0 && en.x < v0 + kLvlPer) {
#pragma unroll
          for (uint32_t k = 0; k < kLvlPer; ++k)
            if (v0 + k == en.x && ((ot[k / 4] >> ((k & 3u) * 8u)) & 0xFFu) != kLvlNone) acc[k] |= bit;
        }
        if (en.w & 0x80000000u) continue;  // overloaded neighbour: no transit
        const Vec nx = nxs[g];
        uint32_t nw[kWords];
        words_of(nx, nw);
        bool direct = own_direct || en.y != w0;
#pragma unroll
        for (uint32_t q = 0; q < kWords; ++q) direct |= has_byte_fe(nw[q]);
        if (!direct && bit < 256u) {
          // plain levels, four nodes per word op: tight iff L_n(v) + 1 ==
          // L_s(v), bytewise mod 256 (an unreached 255 wraps to 0, a level
          // only the source holds, forced to 255 in ot)
#pragma unroll
          for (uint32_t q = 0; q < kWords; ++q) pk[q] |= lvl_tight(nw[q], ot[q], kLvlAllReached) * bit;  // !direct: no kLvlDirect byte
        } else if (!direct) {  // plain levels, a rank past 7
#pragma unroll
          for (uint32_t k = 0; k < kLvlPer; ++k)
            if (((nw[k / 4] >> ((k & 3u) * 8u)) & 0xFFu) + 1u == ((ot[k / 4] >> ((k & 3u) * 8u)) & 0xFFu))
              acc[k] |= bit;
        } else {
#pragma unroll
          for (uint32_t k = 0; k < kLvlPer; ++k) {
            const uint32_t dk = own_dist(k);
            if (dk == kInf) continue;
            const uint32_t x = dist_at(en.z, nx, k);
            if (x != kInf && static_cast<uint64_t>(en.y) + x == dk) acc[k] |= bit;
          }
        }
      }
      }  // entry group
#pragma unroll
      for (uint32_t k = 0; k < kLvlPer; ++k) acc[k] |= (pk[k / 4] >> ((k & 3u) * 8u)) & 0xFFu;
      if (kLvlPer >= 8 && W == 1 && v0 + kLvlPer <= N && (N & 3u) == 0) {
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
        u32x4* o = reinterpret_cast<u32x4*>(nh + v0);
#pragma unroll
        for (uint32_t q = 0; q < kLvlPer / 4; ++q) {
          const u32x4 x = {acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]};
          __builtin_nontemporal_store(x, &o[q]);
        }
      } else {
#pragma unroll
        for (uint32_t k = 0; k < kLvlPer; ++k)
          if (v0 + k < N) nh[static_cast<size_t>(v0 + k) * W + word] = acc[k];
      }
    }
  }
  __syncthreads();  // every thread is done with this source's entries
  }
}

// The lean form of first_hop_lvl_kernel for what a large plain sweep is made
// of (launch_first_hop checks it): one mask word, ranks below 8 (a node's
// mask is one byte), no ignore sets, N a multiple of 4 with 16-byte aligned
// output rows, and no kLvlDirect byte in the rows a source reads - a source
// whose own row or a neighbour's row is flagged in a.row_deep goes to
// a.redo_list and first_hop_lvl_kernel<.., true> redoes it. Same results.
//
// A tile is Q strips of 1,024 nodes; in strip q wave w covers the 256 nodes
// from q * 1024 + w * 256, lane l the four from 4 l: every row access is one
// coalesced dword per lane and every store instruction writes 16 B per lane
// to 1 KB of contiguous memory. A strip's masks are one packed dword (a byte
// per node); mask and distance dwords are byte extracts at the store. The
// rows of the first kLeanGroup entries are loaded for the next tile before
// this tile's compute (entries past those, sources of 5..8 tight first
// links, are loaded in the tile), and the first tile's own bytes before the
// entries are gathered.
constexpr uint32_t kLeanGroup = 4;

template <uint32_t Q>
__global__ __launch_bounds__(kBlock) void first_hop_lean_kernel(HopArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  __shared__ uint32_t s_cnt;
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  constexpr uint32_t kTile = kBlock * 4u * Q;
  const uint32_t N = a.n_nodes, P = a.lvl_pitch, w0 = a.w0;
  const uint32_t tid = threadIdx.x;
  const uint32_t split = a.tile_split;
  const uint32_t lb = xcd_block(blockIdx.x, gridDim.x, a.xcd_group);
  const uint32_t i = lb / split, phase = lb % split;
  const uint32_t wave_at = __builtin_amdgcn_readfirstlane(tid & ~63u);  // 64 x the wave's index (its lanes' nodes: from 4 x this in a strip)
  const uint32_t lane4 = (tid & 63u) * 4u;
  const uint8_t* own_row = a.lvl_rows + static_cast<size_t>(i) * P;
  // strip q of tile t starts at node t * kTile + q * 1024; this wave's part at + wave_at * 4
  auto strip_at = [&](uint32_t tile, uint32_t q) { return tile * kTile + q * (kBlock * 4u) + wave_at * 4u; };
  auto load_own = [&](uint32_t tile, uint32_t (&ow)[Q]) {
#pragma unroll
    for (uint32_t q = 0; q < Q; ++q) {
      const uint32_t v = strip_at(tile, q) + lane4;
      ow[q] = v < N ? *reinterpret_cast<const uint32_t*>(own_row + v) : ~0u;
    }
  };
  uint32_t ow_c[Q];
  load_own(phase, ow_c);  // in flight while the entries are gathered

  // neighbour rows that may hold kLvlDirect bytes (tight or not), and the own row
  const uint32_t nb0 = a.nbr_ptr[i], nb = a.nbr_ptr[i + 1] - nb0;
  uint32_t redo = 0;
  if (tid < nb) redo = a.row_deep[a.nbr_row[nb0 + tid]];
  if (tid == kBlock - 1) redo = a.row_deep[i];
  const uint32_t src = a.srcs[i];
  const uint4* ent = reinterpret_cast<const uint4*>(lds + ((2 * nb + 3) & ~3u));
  const uint32_t ne = hop_entries<true>(a, i, lds, &s_cnt);
  // a tight link is one of metric w0 in a uniform sweep; anything else is the generic kernel's
  if (tid < ne && ent[tid].y != w0) redo = 1;
  if (__syncthreads_or(static_cast<int>(redo))) {
    if (phase == 0 && tid == 0) a.redo_list[atomicAdd(a.redo_count, 1u)] = i;
    return;
  }

  // the first kLeanGroup entries, wave-uniform: node, level row, mask bit, transit
  uint32_t en_n[kLeanGroup], en_bit[kLeanGroup];
  const uint8_t* en_row[kLeanGroup];
  bool en_transit[kLeanGroup];
#pragma unroll
  for (uint32_t g = 0; g < kLeanGroup; ++g) {
    en_n[g] = ~0u;
    en_bit[g] = 0u;
    en_row[g] = own_row;
    en_transit[g] = false;
    if (g < ne) {
      const uint4 e = ent[g];
      const uint32_t w = __builtin_amdgcn_readfirstlane(e.w);
      en_n[g] = __builtin_amdgcn_readfirstlane(e.x);
      en_bit[g] = 1u << (w & 7u);
      en_row[g] = a.lvl_rows + static_cast<size_t>(__builtin_amdgcn_readfirstlane(e.z)) * P;
      en_transit[g] = !(w >> 31);
    }
  }
  auto load_nbrs = [&](uint32_t tile, uint32_t (&nx)[kLeanGroup][Q]) {
#pragma unroll
    for (uint32_t g = 0; g < kLeanGroup; ++g) {
      if (!en_transit[g]) continue;
#pragma unroll
      for (uint32_t q = 0; q < Q; ++q) {
        const uint32_t v = strip_at(tile, q) + lane4;
        nx[g][q] = v < N ? *reinterpret_cast<const uint32_t*>(en_row[g] + v) : 0u;
      }
    }
  };
  // entry {node n, bit} as the first hop towards n itself: the byte of n in
  // its strip's packed word, if n is reached (one scalar test per strip)
  auto direct = [&](uint32_t n, uint32_t bit, uint32_t at, uint32_t reached, uint32_t& pk) {
    if (n - at >= 256u) return;
    const uint32_t d = n - at - lane4;
    if (d < 4u) pk |= ((reached >> (d * 8u + 7u)) & 1u) * (bit << (d * 8u));
  };

  uint32_t nx_c[kLeanGroup][Q];
  load_nbrs(phase, nx_c);
  uint32_t* const nh = a.out_nh + static_cast<size_t>(i) * N;
  uint32_t* const od = const_cast<uint32_t*>(a.dist) + static_cast<size_t>(i) * N;
  for (uint32_t tile = phase;;) {
    const uint32_t next = tile + split;
    const bool more = next < a.tiles;
    uint32_t ow_n[Q], nx_n[kLeanGroup][Q];
#ifndef ORH_EXP_LEAN_NO_PREFETCH  // timing experiment only: the next tile's loads after this tile's stores
    if (more) {  // the next tile's rows, before this tile's compute
      load_own(next, ow_n);
      load_nbrs(next, nx_n);
    }
#endif
#pragma unroll
    for (uint32_t q = 0; q < Q; ++q) {
      const uint32_t at = strip_at(tile, q), v = at + lane4;
      const uint32_t ow = ow_c[q];
      const uint32_t live = lvl_reached(ow);  // 0x80 per reached node (the padding lanes: none)
      uint32_t ot = ow, reached = live;
      if (src - at < 256u) {  // the source's strip: its own byte counts as unreached
        ot = lvl_own_forced(ow, src - at - lane4);
        reached = lvl_reached(ot);
      }
      uint32_t pk = 0u;
#pragma unroll
      for (uint32_t g = 0; g < kLeanGroup; ++g) {
        if (en_transit[g]) pk |= lvl_tight(nx_c[g][q], ot, kLvlAllReached) * en_bit[g];
        direct(en_n[g], en_bit[g], at, reached, pk);
      }
      for (uint32_t e = kLeanGroup; e < ne; ++e) {  // sources of more tight links: one round trip each
        const uint4 en = ent[e];
        const uint32_t w = __builtin_amdgcn_readfirstlane(en.w), bit = 1u << (w & 7u);
        if (!(w >> 31)) {
          const uint8_t* row = a.lvl_rows + static_cast<size_t>(__builtin_amdgcn_readfirstlane(en.z)) * P;
          const uint32_t nx = v < N ? *reinterpret_cast<const uint32_t*>(row + v) : 0u;
          pk |= lvl_tight(nx, ot, kLvlAllReached) * bit;
        }
        direct(__builtin_amdgcn_readfirstlane(en.x), bit, at, reached, pk);
      }
      if (v >= N) continue;  // N % 4 == 0: a lane's four nodes are all inside or all outside
      if (a.write_dist) {
        // the source's own distance row from the level bytes (its own entry is
        // level 0); no byte is kLvlDirect here
        u32x4 d = {(ow & 0xFFu) * w0, ((ow >> 8) & 0xFFu) * w0, ((ow >> 16) & 0xFFu) * w0, (ow >> 24) * w0};
        if (live != 0x80808080u) {
          if (!(live & 0x80u)) d.x = kInf;
          if (!(live & 0x8000u)) d.y = kInf;
          if (!(live & 0x800000u)) d.z = kInf;
          if (!(live & 0x80000000u)) d.w = kInf;
        }
        __builtin_nontemporal_store(d, reinterpret_cast<u32x4*>(od + v));
      }
      const u32x4 m = {pk & 0xFFu, (pk >> 8) & 0xFFu, (pk >> 16) & 0xFFu, pk >> 24};
      __builtin_nontemporal_store(m, reinterpret_cast<u32x4*>(nh + v));
    }
    if (!more) break;
#ifdef ORH_EXP_LEAN_NO_PREFETCH
    load_own(next, ow_n);
    load_nbrs(next, nx_n);
#endif
    tile = next;
#pragma unroll
    for (uint32_t q = 0; q < Q; ++q) {
      ow_c[q] = ow_n[q];
#pragma unroll
      for (uint32_t g = 0; g < kLeanGroup; ++g) nx_c[g][q] = nx_n[g][q];
    }
  }
}

size_t hop_aux_bytes(uint32_t n_rows) { return (hop_aux_deep_off(n_rows) + n_rows + 255) & ~size_t{255}; }

size_t hop_lds_bytes(uint32_t max_nbr) {
  return static_cast<size_t>((2 * max_nbr + 3) & ~3u) * 4 + static_cast<size_t>(max_nbr) * 16;
}

hipError_t launch_first_hop(HopArgs a, uint32_t max_nbr, hipStream_t s, uint32_t* nodes_per_thread,
                            uint32_t* split, uint32_t* lean_ran) {
  if (lean_ran) *lean_ran = 0;
  if (a.n_out == 0) return hipSuccess;
  a.tiles = (a.n_nodes + kBlock * kHopPer - 1) / (kBlock * kHopPer);
  const uint64_t grid = static_cast<uint64_t>(a.tiles) * a.n_out;
  if (grid > 0x7FFFFFFFull) return hipErrorInvalidValue;
  const size_t lds = std::max<size_t>(hop_lds_bytes(max_nbr), 16);
  static const LaunchKnobs knobs = launch_knobs();  // the hop_* fields: once per process
  if (a.lvl_rows) {
    // 16 nodes per thread unless that leaves fewer than ~32 workgroups per CU
    // a workgroup per source walks the tiles (one gather of the source's
    // first links), split over phases while that leaves < 8192 workgroups
    const uint32_t t16 = (a.n_nodes + kBlock * 16 - 1) / (kBlock * 16);
    const bool wide = !knobs.hop_narrow && static_cast<uint64_t>(t16) * a.n_out >= 8192;
    // 8 nodes per thread for large batches (104 VGPRs, 8-byte row loads):
    // one C2 sweep's first hops 0.323 -> 0.292 ms against 16 per thread (158
    // VGPRs), the 4-lane step the same (profiles/r04/r_hop_nodes_ab.txt)
    const uint32_t per = wide ? knobs.hop_nodes : 4u;
    a.tiles = (a.n_nodes + kBlock * per - 1) / (kBlock * per);
    a.tile_split = 1;
    while (a.tile_split < a.tiles && static_cast<uint64_t>(a.tile_split) * a.n_out < 8192) ++a.tile_split;
    a.tile_split = std::max(a.tile_split, std::min(knobs.hop_split, a.tiles));
    uint64_t g2 = static_cast<uint64_t>(a.tile_split) * a.n_out;
    if (g2 > 0x7FFFFFFFull) return hipErrorInvalidValue;
    a.n_logical = static_cast<uint32_t>(g2);
    // hop_wg_per_cu: persistent workgroups, that many per CU, for even
    // per-source work. C2 sweep, first hops: 0.362 ms one per block, 0.389 ms
    // at 8 per CU, 0.439 at 4 (profiles/r03/n_ms_variants_ab.txt): more
    // workgroups in flight beat fewer, longer-lived ones
    const uint32_t per_cu = knobs.hop_wg_per_cu;
    static const uint32_t n_cu = [] {
      int d = 0, c = 0;
      if (hipGetDevice(&d) != hipSuccess || hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, d) != hipSuccess)
        return 0u;
      return static_cast<uint32_t>(c);
    }();
    if (a.xcd_group == 0 && per_cu && n_cu) {
      const uint64_t cap = (static_cast<uint64_t>(n_cu) * per_cu) & ~uint64_t{7};
      if (cap >= 8 && cap < g2) g2 = cap;
    }
    if (nodes_per_thread) *nodes_per_thread = per;
    if (split) *split = a.tile_split;
    // The lean kernel where its preconditions hold (ORH_HOP_LEAN=0, read per
    // launch: never). Its tile is the 8-node kernel's (256 x 4 x Q nodes, Q =
    // 2), so tiles, tile_split, n_logical and the XCD-aware block order above
    // are kept as they are; one workgroup per logical block. N % 4 != 0 or an
    // unaligned output is declined (the rows of odd sources would start off a
    // 16-byte boundary). The generic kernel follows over the sources the lean
    // one listed - none, in a sweep of fewer than kLvlDirect levels - with at
    // most a workgroup per CU; the search kernel emptied the list.
    constexpr uint32_t kLeanQ = 2;
    const bool lean = launch_knobs().hop_lean && wide && per == 4 * kLeanQ && a.words == 1 && max_nbr <= 8 &&
                      !a.ignore_ptr && a.row_deep && a.redo_list && a.redo_count && (a.n_nodes & 3u) == 0 &&
                      ((reinterpret_cast<uintptr_t>(a.out_nh) | reinterpret_cast<uintptr_t>(a.dist)) & 15u) == 0 &&
                      g2 == a.n_logical;
    if (lean_ran) *lean_ran = lean ? 1u : 0u;
    if (lean) {
      const hipError_t e = launch(first_hop_lean_kernel<kLeanQ>, a, a.n_logical, kBlock, lds, s);
      if (e != hipSuccess) return e;
      const uint32_t redo_grid = std::min(a.n_logical, n_cu ? n_cu : 256u);
      return launch(first_hop_lvl_kernel<4 * kLeanQ, true>, a, redo_grid, kBlock, lds, s);
    }
    return per == 16 ? launch(first_hop_lvl_kernel<16>, a, static_cast<uint32_t>(g2), kBlock, lds, s)
         : per == 8  ? launch(first_hop_lvl_kernel<8>, a, static_cast<uint32_t>(g2), kBlock, lds, s)
                     : launch(first_hop_lvl_kernel<4>, a, static_cast<uint32_t>(g2), kBlock, lds, s);
  }
  if (nodes_per_thread) *nodes_per_thread = 1;
  if (split) *split = a.tiles;
  a.xcd_hop = launch_knobs().hop_xcd ? 1u : 0u;  // read per launch (A/B)
  return launch(first_hop_kernel, a, static_cast<uint32_t>(grid), kBlock, lds, s);
}

}  // namespace orh

// openr_hip.h: the host build of the kernels' bytewise first-hop test
extern "C" uint32_t orh_lvl_tight_word(uint32_t nbr_word, uint32_t own_word, uint32_t src_byte) {
  return orh::lvl_tight_word(nbr_word, own_word, src_byte);
}
