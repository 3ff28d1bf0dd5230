// SPF kernels, general metrics, many sources: multi-source Bellman-Ford in
// LDS (kWms), its sliced-ELL form for any node degree (kWmsSliced) and that
// form with u32 labels for metrics past 15 bits (kWmsWide).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spf_device.h"
#include "spf_launch.h"

namespace orh {

// ---------------------------------------------------------------------------
// phase 1d: general metrics, many sources: multi-source Bellman-Ford in LDS
// ---------------------------------------------------------------------------
// The weighted counterpart of spf_msbfs_kernel. A workgroup holds the u16
// distances of 4 sources for every node in LDS (8 bytes per node, two packed
// u16 pairs) and relaxes them in pull form: per round each thread recomputes
// its own nodes, d(v) = min(d(v), min over in-links (u, w) of d(u) + w), for
// the 4 sources at once with packed 16-bit adds (saturating: 0xFFFF stays
// "unreached") and packed minima. The in-links of a thread's nodes sit in
// its registers ({u, w(u -> v)} per slot, a_wms layout, Cuthill-McKee ids),
// so a round touches no global memory. Writes go in place (any value read
// is a path length, so the fixpoint is the same in any order) and a round
// without a change anywhere ends the search: the labels are then the
// shortest distances of runSpf (LinkState.cpp:808-882) for positive metrics.
// No transit through an overloaded node: a slot whose u is overloaded is dead,
// except that an overloaded source still reaches its own neighbours (applied
// once before the rounds). First hops: phase 2 over the u32 rows.
// A label past 0xFFFF - 1 - max metric could hide a distance that does not fit
// 16 bits: such a batch lists its rows in a.ovf_rows and the caller redoes
// them: spf_wms_wide_kernel's row-list entry in batches where the graph has
// its wide layout, else spf_lds_nh_kernel (u64 labels, fused first hops -
// phase 2 then recomputes the same first hops).
constexpr uint32_t kWmsOvl = 0x80000000u;  // slot flag: u is overloaded

// packed u16 pairs: saturating add (v_pk_add_u16 clamp: 0xFFFF stays
// "unreached") and minimum (v_pk_min_u16)
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
__device__ inline uint32_t pk_add_sat_u16(uint32_t a, uint32_t b) {
  const u16x2 r = __builtin_elementwise_add_sat(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b));
  return __builtin_bit_cast(uint32_t, r);
}
__device__ inline uint32_t pk_min_u16(uint32_t a, uint32_t b) {
  const u16x2 r = __builtin_elementwise_min(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b));
  return __builtin_bit_cast(uint32_t, r);
}

// J <= 10 capped at 64 VGPRs, so that two 1,024-thread batches share a CU
// (their LDS, 2 x 80 KB, fits), measured slower on C2w
// (profiles/r06/g_c2w_*), so one batch per CU
// S = 4 or 8 sources per batch: a node's labels are S u16 in S / 2 dwords
// (8: 16 B per node, so N <= ~10,200 fits one batch per CU)
template <int K, int J, int S>
__global__ __launch_bounds__(1024) void spf_wms_kernel(SpfArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  constexpr uint32_t W = S / 2;  // dwords per node
  typedef uint32_t DV __attribute__((ext_vector_type(W)));
  const uint32_t N = a.n_nodes;
  const uint32_t tid = threadIdx.x, B = blockDim.x;
  const uint32_t b0 = blockIdx.x * S;
  const uint32_t nsrc = min(static_cast<uint32_t>(S), a.n_rows - b0);
  __shared__ uint32_t s_prog[3], s_ovf;
  DV* D = reinterpret_cast<DV*>(lds);  // [N + 1]; D[N] stays unreached
  auto ld = [&](uint32_t u) -> DV { return D[u]; };
  auto st = [&](uint32_t u, const DV& v) { D[u] = v; };
  {
    DV none;
#pragma unroll
    for (uint32_t q = 0; q < W; ++q) none[q] = ~0u;
    for (uint32_t i = tid; i <= N; i += B) st(i, none);
  }
  if (tid < 3) s_prog[tid] = 0u;
  if (tid == 0) s_ovf = 0u;
  __syncthreads();
  if (tid < nsrc) {  // sources may repeat: clear each lane's half alone
    const uint32_t src = a.dev_of[a.srcs[a.order[b0 + tid]]];
    uint32_t* w = reinterpret_cast<uint32_t*>(D + src) + (tid >> 1);
    atomicAnd(w, (tid & 1u) ? 0x0000FFFFu : 0xFFFF0000u);
  }
  __syncthreads();
  // the in-link slots of the owned nodes: {u (16 bits) | w (15 bits) << 16 |
  // kWmsOvl}; an unused slot (no link, link down) reads u = N, the entry that
  // stays unreached
  // node of (this thread, j): band schedule - wave w owns chunks [w J, (w +
  // 1) J) - or interleaved - chunk j * waves + w
  const bool band = a.wms_band != 0u;
  const uint32_t wave = tid >> 6;
  const uint32_t lane = tid & 63u;
  auto node_of = [&](uint32_t j) { return band ? (wave * J + j) * 64u + lane : j * B + tid; };
  uint32_t slot[J][K];
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const uint32_t v = node_of(j);
#pragma unroll
    for (int k = 0; k < K; ++k) slot[j][k] = v < N ? a.wms_slots[static_cast<size_t>(v) * K + k] : N;
  }
  // an overloaded source reaches its neighbours and no further: a slot whose
  // u is overloaded contributes w to the lanes where u is the source (label
  // 0: only a source holds it, and this pass writes nothing below 1), once,
  // and is dead from then on like every other slot of an overloaded node
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const uint32_t v = node_of(j);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (!(slot[j][k] & kWmsOvl)) continue;
      const uint32_t u = slot[j][k] & 0xFFFFu, w = (slot[j][k] >> 16) & 0x7FFFu;
      slot[j][k] = N;
      const DV du = ld(u);
      DV d = ld(v);  // v < N: a slot of a padding node is never flagged
#pragma unroll
      for (uint32_t q = 0; q < W; ++q) {
        const uint32_t lo = (du[q] & 0xFFFFu) == 0u ? w : 0xFFFFu, hi = (du[q] >> 16) == 0u ? w : 0xFFFFu;
        d[q] = pk_min_u16(d[q], lo | (hi << 16));
      }
      st(v, d);
    }
  }
  __syncthreads();
  // activity: a wave's slice j is the 64-node chunk c = v / 64 (Cuthill-McKee
  // ids). A chunk whose nodes changed in round r sets its bit in chg[r % 3];
  // in round r + 1 a slice is recomputed only if a chunk within the layout
  // bandwidth of it (where all its in-links come from) changed in round r -
  // a node whose in-neighbours all kept their labels since it was last
  // recomputed cannot change. (A change later in the same round is seen in
  // the next one.) Three rotating bitmaps: one read, one written, one cleared.
  // a.ms_bw = 0: every slice every round (ORH_WMS_SKIP, orh_spf_run)
  const uint32_t nchunk = (N + 63) / 64, cw = (nchunk + 31) / 32;
  uint32_t* chg = reinterpret_cast<uint32_t*>(D + N + 1);  // [3][cw]
  for (uint32_t i = tid; i < 3 * cw; i += B) chg[i] = 0u;
  const uint32_t bw = a.ms_bw;
  __syncthreads();
  // (the owner keeping its J labels in registers instead of reading its own
  // back from LDS measured slower: C2w distances 3.65 vs 3.55 ms,
  // profiles/r06/x_wms_ab.txt; two forward/backward passes per round 3.72)
  for (uint32_t round = 1;; ++round) {
    int prog = 0;
    const uint32_t* prev = chg + ((round + 2u) % 3u) * cw;
    uint32_t* cur = chg + (round % 3u) * cw;
    if (tid < cw) chg[((round + 1u) % 3u) * cw + tid] = 0u;  // read in round - 1, written in round + 1
    // back: the band schedule's backward sweep, which also sees the chunks
    // this round's forward sweep changed
    auto relax = [&](auto jc, bool back) {
      constexpr int j = decltype(jc)::value;
      const uint32_t v = node_of(j);
      const uint32_t c = __builtin_amdgcn_readfirstlane(band ? wave * J + j : j * (B >> 6) + wave);  // this slice's chunk
      if ((round > 1 || back) && bw) {
        const uint32_t lo = c * 64u > bw ? (c * 64u - bw) >> 6 : 0u;
        const uint32_t hi = min(nchunk - 1u, (c * 64u + 63u + bw) >> 6);
        bool act = false;
        for (uint32_t w = lo >> 5; w <= (hi >> 5) && !act; ++w) {
          uint32_t m = (round > 1 ? prev[w] : 0u) | (back ? cur[w] : 0u);
          if (w == (lo >> 5)) m &= ~0u << (lo & 31u);
          if (w == (hi >> 5) && (hi & 31u) != 31u) m &= (2u << (hi & 31u)) - 1u;
          act = m != 0u;
        }
        if (!act) return;
      }
      if (v >= N) return;
      // opaque per round: the addresses and replicated weights are derived
      // again each time instead of held in J * K more registers
#pragma unroll
      for (int k = 0; k < K; ++k) asm volatile("" : "+v"(slot[j][k]));
      DV du[K];
#pragma unroll
      for (int k = 0; k < K; ++k) du[k] = ld(slot[j][k] & 0xFFFFu);
      const DV own = ld(v);
      DV acc = own;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        // {w, w}: the high half twice (an unused slot: w = 0 on the unreached entry)
        const uint32_t wr = __builtin_amdgcn_perm(slot[j][k], slot[j][k], 0x03020302u);
#pragma unroll
        for (uint32_t q = 0; q < W; ++q) acc[q] = pk_min_u16(acc[q], pk_add_sat_u16(du[k][q], wr));
      }
      bool changed = false;
#pragma unroll
      for (uint32_t q = 0; q < W; ++q) changed |= acc[q] != own[q];
      if (changed) {
        st(v, acc);
        prog = 1;
      }
      if (__builtin_amdgcn_ballot_w64(changed) && (tid & 63u) == 0u) atomicOr(&cur[c >> 5], 1u << (c & 31u));
    };
    // (walking the slices backwards in odd rounds, for paths against the
    // slice order, measured no faster: profiles/r06/h_c2w_variants.txt)
    constexpr int kWmsPasses = 1;  // forward + backward sweeps of a band per round
    for (int pass = 0; pass < (band ? kWmsPasses : 1); ++pass) {
      static_for<J>([&](auto jc) { relax(jc, pass > 0); });
      if (band)  // and back: a band passes its changes both ways in one round
        static_for<J>([&](auto jc) { relax(std::integral_constant<int, J - 1 - decltype(jc)::value>{}, true); });
    }
    if (prog) s_prog[round % 3u] = 1u;
    lds_barrier();
    if (!s_prog[round % 3u]) break;
    if (tid == 0) s_prog[(round + 2u) % 3u] = 0u;
  }
  // rows out in host order (coalesced), a u16 label widened to u32; a label
  // within max metric of 0xFFFF may stand for a distance that did not fit
  const uint32_t lim = a.wms_limit;
  uint32_t* out[S];
#pragma unroll
  for (uint32_t k = 0; k < S; ++k)
    out[k] = k < nsrc ? dist_row(a.out_dist, a.scratch, a.n_out, N, a.order[b0 + k]) : nullptr;
  bool ovf = false;
  for (uint32_t i = tid; i < N; i += B) {
    const DV d = ld(a.dev_of[i]);
#pragma unroll
    for (uint32_t k = 0; k < S; ++k) {
      if (k >= nsrc) break;
      const uint32_t l = (d[k / 2] >> ((k & 1u) * 16u)) & 0xFFFFu;
      ovf |= l != 0xFFFFu && l > lim;
      __builtin_nontemporal_store(l == 0xFFFFu ? kInf : l, &out[k][i]);
    }
  }
  if (ovf) s_ovf = 1u;
  __syncthreads();
  if (s_ovf && tid < nsrc) {
    const uint32_t k = atomicAdd(&a.ovf_rows[0], 1u);
    a.ovf_rows[1 + k] = a.order[b0 + tid];
  }
}

// The same search with the in-links in global memory instead of registers,
// for graphs with nodes of any degree (kWmsSliced). Sliced ELL over the
// Cuthill-McKee ids: slice s is the 64 nodes [64 s, 64 s + 64), one lane per
// node, and as wide as its largest in-degree (rounded up to 4 columns);
// column k of slice s is the 64 words a.wsl_slots[a.wsl_off[s] + 64 k ..], one
// coalesced 256-byte load per wave. A slot is the spf_wms_kernel word {u | w(u
// -> v) << 16 | overloaded(u) << 31}, u = N for padding and down links. A node
// is owned by one lane, so no two lanes ever write the same label. Wave w
// owns the slices [a.wsl_band[w], a.wsl_band[w + 1]) (cut by the host so the
// waves carry like column counts) and sweeps them forward, then backward,
// each round. The slots are shared by every batch and read-only, so a slot
// whose u is overloaded is masked to u = N as it is read in the rounds.
template <int S>
__global__ __launch_bounds__(1024) void spf_wms_sliced_kernel(SpfArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  constexpr uint32_t W = S / 2;  // dwords per node
  typedef uint32_t DV __attribute__((ext_vector_type(W)));
  const uint32_t N = a.n_nodes;
  const uint32_t tid = threadIdx.x, B = blockDim.x;
  const uint32_t b0 = blockIdx.x * S;
  const uint32_t nsrc = min(static_cast<uint32_t>(S), a.n_rows - b0);
  __shared__ uint32_t s_prog[3], s_ovf;
  DV* D = reinterpret_cast<DV*>(lds);  // [N + 1]; D[N] stays unreached
  {
    DV none;
#pragma unroll
    for (uint32_t q = 0; q < W; ++q) none[q] = ~0u;
    for (uint32_t i = tid; i <= N; i += B) D[i] = none;
  }
  if (tid < 3) s_prog[tid] = 0u;
  if (tid == 0) s_ovf = 0u;
  __syncthreads();
  if (tid < nsrc) {  // sources may repeat: clear each lane's half alone
    const uint32_t src = a.dev_of[a.srcs[a.order[b0 + tid]]];
    atomicAnd(reinterpret_cast<uint32_t*>(D + src) + (tid >> 1), (tid & 1u) ? 0x0000FFFFu : 0xFFFF0000u);
  }
  __syncthreads();
  const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t lane = tid & 63u;
  const uint32_t sb = a.wsl_band[wave], se = a.wsl_band[wave + 1];
  const uint32_t* slots = a.wsl_slots + lane;
  // an overloaded source reaches its neighbours and no further (as in
  // spf_wms_kernel): a flagged slot contributes w to the lanes where u is the
  // source (label 0: only a source holds it, and this pass writes nothing
  // below 1), once, here. a.wsl_ovl = 0: the layout has no flagged slot
  if (a.wsl_ovl) {
    for (uint32_t s = sb; s < se; ++s) {
      const uint32_t o1 = a.wsl_off[s + 1];
      const uint32_t v = min(s * 64u + lane, N);
      for (uint32_t o = a.wsl_off[s]; o < o1; o += 64u) {
        const uint32_t sl = slots[o];
        if (!(sl & kWmsOvl)) continue;
        const uint32_t u = sl & 0xFFFFu, w = (sl >> 16) & 0x7FFFu;
        const DV du = D[u];
        DV d = D[v];  // v < N: a slot of a padding node is never flagged
#pragma unroll
        for (uint32_t q = 0; q < W; ++q) {
          const uint32_t lo = (du[q] & 0xFFFFu) == 0u ? w : 0xFFFFu, hi = (du[q] >> 16) == 0u ? w : 0xFFFFu;
          d[q] = pk_min_u16(d[q], lo | (hi << 16));
        }
        D[v] = d;
      }
    }
    __syncthreads();
  }
  for (uint32_t round = 1;; ++round) {
    int prog = 0;
    auto relax = [&](uint32_t s) {
      const uint32_t o1 = a.wsl_off[s + 1];
      const uint32_t v = min(s * 64u + lane, N);  // a lane past N: every slot N, never changes
      const DV own = D[v];
      DV acc = own;
      // 4 columns at a time (a slice's width is a multiple of 4): the slot
      // loads, then the label reads, in flight together
#pragma unroll 2
      for (uint32_t o = a.wsl_off[s]; o < o1; o += 256u) {
        uint32_t sl[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) sl[k] = slots[o + 64u * k];
#pragma unroll
        for (int k = 0; k < 4; ++k) sl[k] = (sl[k] & kWmsOvl) ? N : sl[k];  // dead after the pass above
        DV du[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) du[k] = D[sl[k] & 0xFFFFu];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          // {w, w}: the high half twice (padding: w = 0 on the unreached entry)
          const uint32_t wr = __builtin_amdgcn_perm(sl[k], sl[k], 0x03020302u);
#pragma unroll
          for (uint32_t q = 0; q < W; ++q) acc[q] = pk_min_u16(acc[q], pk_add_sat_u16(du[k][q], wr));
        }
      }
      bool changed = false;
#pragma unroll
      for (uint32_t q = 0; q < W; ++q) changed |= acc[q] != own[q];
      if (changed) {
        D[v] = acc;
        prog = 1;
      }
    };
    // forward, then back (the last slice was relaxed just now): a band passes
    // its changes both ways in one round
    for (uint32_t s = sb; s < se; ++s) relax(s);
    if (se > sb)
      for (uint32_t s = se - 1; s-- > sb;) relax(s);
    if (prog) s_prog[round % 3u] = 1u;
    lds_barrier();
    if (!s_prog[round % 3u]) break;
    if (tid == 0) s_prog[(round + 2u) % 3u] = 0u;
  }
  // rows out in host order, as spf_wms_kernel writes them
  const uint32_t lim = a.wms_limit;
  uint32_t* out[S];
#pragma unroll
  for (uint32_t k = 0; k < S; ++k)
    out[k] = k < nsrc ? dist_row(a.out_dist, a.scratch, a.n_out, N, a.order[b0 + k]) : nullptr;
  bool ovf = false;
  for (uint32_t i = tid; i < N; i += B) {
    const DV d = D[a.dev_of[i]];
#pragma unroll
    for (uint32_t k = 0; k < S; ++k) {
      if (k >= nsrc) break;
      const uint32_t l = (d[k / 2] >> ((k & 1u) * 16u)) & 0xFFFFu;
      ovf |= l != 0xFFFFu && l > lim;
      __builtin_nontemporal_store(l == 0xFFFFu ? kInf : l, &out[k][i]);
    }
  }
  if (ovf) s_ovf = 1u;
  __syncthreads();
  if (s_ovf && tid < nsrc) {
    const uint32_t k = atomicAdd(&a.ovf_rows[0], 1u);
    a.ovf_rows[1 + k] = a.order[b0 + tid];
  }
}

// The sliced search with u32 labels (kWmsWide): for graphs whose metrics do
// not fit the 15 bits of a slot word, and for the rows the two u16 kernels
// flag. Same geometry (slices, columns, the bands of a.wsl_off / a.wsl_band),
// same rounds. A node's labels are S u32 (S = 4: 16 B, one ds_read_b128 per
// in-link, the footprint of the u16 form at 8 sources; S = 2: 8 B, where 16 B
// per node no longer fit LDS), 0xFFFFFFFF unreached. A slot is 8 bytes, {u |
// overloaded(u) << 31, w(u -> v)} with the full u32 metric, padding and down
// links {N, 0}; a wave's column is one coalesced 512-byte load. The add
// saturates for "unreached + w" alone: the plan is chosen only when
// wide_metrics(g) is false (orh_api.hip), i.e. the sum of all live metrics
// plus the largest stays below 0xFFFFFFFF, so no path sum reaches the
// unreached value and every row this kernel writes is final: no overflow
// list, no a.wms_limit.
// Rows: batch b takes rows a.order[b S .. b S + S) of a.n_rows, or, with
// a.row_list (the flagged rows of a u16 sweep), a.row_list[b S .. b S + S) of
// *a.row_count; a batch past the count returns before it touches LDS.
constexpr uint32_t kWmsWideStatic = 16;  // the kernel's static LDS (s_prog), for wms_wide_lds_bytes
template <int S>
__global__ __launch_bounds__(1024) void spf_wms_wide_kernel(SpfArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  typedef uint32_t DV __attribute__((ext_vector_type(S)));
  const uint32_t N = a.n_nodes;
  const uint32_t tid = threadIdx.x, B = blockDim.x;
  const uint32_t b0 = blockIdx.x * S;
  const uint32_t* rows = a.row_list ? a.row_list : a.order;
  const uint32_t n_rows = a.row_list ? min(*a.row_count, a.n_rows) : a.n_rows;
  if (b0 >= n_rows) return;
  const uint32_t nsrc = min(static_cast<uint32_t>(S), n_rows - b0);
  __shared__ uint32_t s_prog[4];
  static_assert(sizeof(s_prog) == kWmsWideStatic, "wms_wide_lds_bytes counts the static LDS");
  DV* D = reinterpret_cast<DV*>(lds);  // [N + 1]; D[N] stays unreached
  {
    DV none;
#pragma unroll
    for (int q = 0; q < S; ++q) none[q] = kInf;
    for (uint32_t i = tid; i <= N; i += B) D[i] = none;
  }
  if (tid < 3) s_prog[tid] = 0u;
  __syncthreads();
  // sources may repeat: each lane of the batch has its own dword
  if (tid < nsrc) lds[a.dev_of[a.srcs[rows[b0 + tid]]] * S + tid] = 0u;
  __syncthreads();
  const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t lane = tid & 63u;
  const uint32_t sb = a.wsl_band[wave], se = a.wsl_band[wave + 1];
  const uint2* slots = a.wsw_slots + lane;
  // an overloaded source reaches its neighbours and no further (as in
  // spf_wms_kernel): a flagged slot contributes w to the lanes where u is the
  // source (label 0: only a source holds it, and this pass writes nothing
  // below 1), once, here. a.wsl_ovl = 0: the layout has no flagged slot
  if (a.wsl_ovl) {
    for (uint32_t s = sb; s < se; ++s) {
      const uint32_t o1 = a.wsl_off[s + 1];
      const uint32_t v = min(s * 64u + lane, N);
      for (uint32_t o = a.wsl_off[s]; o < o1; o += 64u) {
        const uint2 sl = slots[o];
        if (!(sl.x & kWmsOvl)) continue;
        const DV du = D[sl.x & ~kWmsOvl];
        DV d = D[v];  // v < N: a slot of a padding node is never flagged
#pragma unroll
        for (int q = 0; q < S; ++q) d[q] = min(d[q], du[q] == 0u ? sl.y : kInf);
        D[v] = d;
      }
    }
    __syncthreads();
  }
  for (uint32_t round = 1;; ++round) {
    int prog = 0;
    auto relax = [&](uint32_t s) {
      const uint32_t o1 = a.wsl_off[s + 1];
      const uint32_t v = min(s * 64u + lane, N);  // a lane past N: every slot N, never changes
      const DV own = D[v];
      DV acc = own;
      // 4 columns at a time (a slice's width is a multiple of 4): the slot
      // loads, then the label reads, in flight together
#pragma unroll 2
      for (uint32_t o = a.wsl_off[s]; o < o1; o += 256u) {
        uint2 sl[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) sl[k] = slots[o + 64u * k];
        DV du[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) du[k] = D[(sl[k].x & kWmsOvl) ? N : sl[k].x];  // dead after the pass above
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          DV w;  // padding: w = 0 on the unreached entry
#pragma unroll
          for (int q = 0; q < S; ++q) w[q] = sl[k].y;
          acc = __builtin_elementwise_min(acc, __builtin_elementwise_add_sat(du[k], w));
        }
      }
      bool changed = false;
#pragma unroll
      for (int q = 0; q < S; ++q) changed |= acc[q] != own[q];
      if (changed) {
        D[v] = acc;
        prog = 1;
      }
    };
    // forward, then back (the last slice was relaxed just now): a band passes
    // its changes both ways in one round
    for (uint32_t s = sb; s < se; ++s) relax(s);
    if (se > sb)
      for (uint32_t s = se - 1; s-- > sb;) relax(s);
    if (prog) s_prog[round % 3u] = 1u;
    lds_barrier();
    if (!s_prog[round % 3u]) break;
    if (tid == 0) s_prog[(round + 2u) % 3u] = 0u;
  }
  // rows out in host order; the unreached label is the rows' kInf already
  uint32_t* out[S];
#pragma unroll
  for (int k = 0; k < S; ++k)
    out[k] = static_cast<uint32_t>(k) < nsrc ? dist_row(a.out_dist, a.scratch, a.n_out, N, rows[b0 + k]) : nullptr;
  for (uint32_t i = tid; i < N; i += B) {
    const DV d = D[a.dev_of[i]];
#pragma unroll
    for (int k = 0; k < S; ++k) {
      if (static_cast<uint32_t>(k) >= nsrc) break;
      __builtin_nontemporal_store(d[k], &out[k][i]);
    }
  }
}

size_t wms_lds_bytes(uint32_t n_nodes, uint32_t sources) {
  const size_t cw = (static_cast<size_t>(n_nodes) + 63) / 64 / 32 + 1;
  return (static_cast<size_t>(n_nodes) + 1) * 2 * sources + 3 * cw * 4;  // labels, then the chunk-change bitmaps
}

template <int K, int S>
static hipError_t launch_wms_k(const SpfArgs& a, uint32_t batches, size_t lds, hipStream_t s) {
  const uint32_t j = (a.n_nodes + 1023) / 1024;
  if constexpr (S == 8) {  // 16 B a node: N <= ~10,200, J <= 10
    switch (j <= 2 ? 2 : j <= 4 ? 4 : j <= 6 ? 6 : j <= 8 ? 8 : 10) {
      case 2: return launch(spf_wms_kernel<K, 2, 8>, a, batches, 1024, lds, s);
      case 4: return launch(spf_wms_kernel<K, 4, 8>, a, batches, 1024, lds, s);
      case 6: return launch(spf_wms_kernel<K, 6, 8>, a, batches, 1024, lds, s);
      case 8: return launch(spf_wms_kernel<K, 8, 8>, a, batches, 1024, lds, s);
      default: return launch(spf_wms_kernel<K, 10, 8>, a, batches, 1024, lds, s);
    }
  } else {
    switch (j <= 2 ? 2 : j <= 4 ? 4 : j <= 6 ? 6 : j <= 8 ? 8 : j <= 10 ? 10 : j <= 12 ? 12 : j <= 16 ? 16 : 20) {
      case 2: return launch(spf_wms_kernel<K, 2, 4>, a, batches, 1024, lds, s);
      case 4: return launch(spf_wms_kernel<K, 4, 4>, a, batches, 1024, lds, s);
      case 6: return launch(spf_wms_kernel<K, 6, 4>, a, batches, 1024, lds, s);
      case 8: return launch(spf_wms_kernel<K, 8, 4>, a, batches, 1024, lds, s);
      case 10: return launch(spf_wms_kernel<K, 10, 4>, a, batches, 1024, lds, s);
      case 12: return launch(spf_wms_kernel<K, 12, 4>, a, batches, 1024, lds, s);
      case 16: return launch(spf_wms_kernel<K, 16, 4>, a, batches, 1024, lds, s);
      default: return launch(spf_wms_kernel<K, 20, 4>, a, batches, 1024, lds, s);
    }
  }
}

uint32_t wms_sources(uint32_t n_nodes, size_t lds_limit) {
  return !launch_knobs().wms_four && n_nodes <= 10240 && wms_lds_bytes(n_nodes, 8) <= lds_limit ? 8u : 4u;
}

size_t wms_wide_lds_bytes(uint32_t n_nodes, uint32_t sources) {
  return (static_cast<size_t>(n_nodes) + 1) * 4 * sources + kWmsWideStatic;
}

uint32_t wms_wide_sources(uint32_t n_nodes, size_t lds_limit) {
  if (n_nodes == 0 || n_nodes > 20480) return 0u;
  if (!launch_knobs().wms_wide_two && wms_wide_lds_bytes(n_nodes, 4) <= lds_limit) return 4u;
  return wms_wide_lds_bytes(n_nodes, 2) <= lds_limit ? 2u : 0u;
}

hipError_t launch_spf_wms_wide(SpfArgs a, uint32_t n_rows, uint32_t block, size_t lds_limit, hipStream_t s) {
  if (n_rows == 0) return hipSuccess;
  const uint32_t S = wms_wide_sources(a.n_nodes, lds_limit);
  if (!S || !a.wsw_slots || !a.wsl_off || !a.wsl_band || !a.dev_of || (!a.row_list != !a.row_count) ||
      (block != 256 && block != 512 && block != 1024))
    return hipErrorInvalidValue;
  a.n_rows = n_rows;
  const uint32_t batches = (n_rows + S - 1) / S;
  const size_t lds = wms_wide_lds_bytes(a.n_nodes, S) - kWmsWideStatic;
  return S == 4 ? launch(spf_wms_wide_kernel<4>, a, batches, block, lds, s)
                : launch(spf_wms_wide_kernel<2>, a, batches, block, lds, s);
}

// the rows a u16 sweep flagged (a.ovf_rows: count, then rows), redone in wide
// batches: a grid for every row, the batches past the count exit at once
static hipError_t redo_wide(SpfArgs a, uint32_t n_rows, uint32_t block, size_t lds_limit, hipStream_t s) {
  a.row_list = a.ovf_rows + 1;
  a.row_count = a.ovf_rows;
  return launch_spf_wms_wide(a, n_rows, block, lds_limit, s);
}

hipError_t launch_spf_wms(SpfArgs a, uint32_t n_rows, uint32_t wms_k, uint32_t wide_block, size_t lds_limit,
                          hipStream_t s) {
  if (n_rows == 0) return hipSuccess;
  if (!a.ovf_rows || !a.wms_slots || a.n_nodes > 20480 || a.n_nodes >= 0xFFFFu) return hipErrorInvalidValue;
  a.n_rows = n_rows;
  a.row_list = nullptr;
  a.row_count = nullptr;
  hipError_t e = hipMemsetAsync(a.ovf_rows, 0, 4, s);
  if (e != hipSuccess) return e;
  // 8 sources per batch where their labels fit one CU's LDS (the rounds, the
  // barriers and the slot registers then serve twice the sources)
  const uint32_t S = wms_sources(a.n_nodes, lds_limit);
  const uint32_t batches = (n_rows + S - 1) / S;
  const size_t lds = wms_lds_bytes(a.n_nodes, S);
  if (S == 8)
    e = wms_k == 8 ? launch_wms_k<8, 8>(a, batches, lds, s) : launch_wms_k<4, 8>(a, batches, lds, s);
  else
    e = wms_k == 8 ? launch_wms_k<8, 4>(a, batches, lds, s) : launch_wms_k<4, 4>(a, batches, lds, s);
  if (e != hipSuccess) return e;
  // rows whose distances may not fit 16 bits: wide batches over the list
  // (wide_block: the graph has its wide layout), or the u64 LDS search
  // (workgroups past its length exit at once); its first-hop rows are
  // rewritten, identically, by phase 2
  if (wide_block) return redo_wide(a, n_rows, wide_block, lds_limit, s);
  a.row_list = a.ovf_rows + 1;
  a.row_count = a.ovf_rows;
  return launch_lds_nh_rows(a, n_rows, s);
}

hipError_t launch_spf_wms_sliced(const SpfPlan& redo, SpfArgs a, uint32_t n_rows, uint32_t block, bool wide_redo,
                                 size_t lds_limit, hipStream_t s) {
  if (n_rows == 0) return hipSuccess;
  if (!a.ovf_rows || !a.wsl_slots || !a.wsl_off || !a.wsl_band || a.n_nodes > 20480 ||
      (block != 256 && block != 512 && block != 1024) ||
      (redo.variant != SpfVariant::kDist16 && redo.variant != SpfVariant::kDist32))
    return hipErrorInvalidValue;
  a.n_rows = n_rows;
  a.row_list = nullptr;
  a.row_count = nullptr;
  hipError_t e = hipMemsetAsync(a.ovf_rows, 0, 4, s);
  if (e != hipSuccess) return e;
  const uint32_t S = wms_sources(a.n_nodes, lds_limit);
  const uint32_t batches = (n_rows + S - 1) / S;
  const size_t lds = wms_lds_bytes(a.n_nodes, S);
  e = S == 8 ? launch(spf_wms_sliced_kernel<8>, a, batches, block, lds, s)
             : launch(spf_wms_sliced_kernel<4>, a, batches, block, lds, s);
  if (e != hipSuccess) return e;
  // rows whose distances may not fit 16 bits: wide batches over the list
  // (wide_redo: the layout carries its 8-byte slots too), or the two-phase
  // plan's own search (distances only, any neighbour count); workgroups past
  // the list's length exit at once
  if (wide_redo) return redo_wide(a, n_rows, block, lds_limit, s);
  a.row_list = a.ovf_rows + 1;
  a.row_count = a.ovf_rows;
  return launch_spf(redo, a, n_rows, s);
}

}  // namespace orh
