// libopenr_hip: C ABI (include/openr_hip.h) over the gfx950 SPF kernels, in
// units: orh_api.hip (per-device contexts, per-area graph mirrors) and, under
// api/, spf.hip, whatif.hip, ksp.hip and routes.hip. This header holds the
// context and graph types and what else crosses the units' lines.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <mutex>
#include <string>
#include <vector>

#include "../../../include/openr_hip.h"
#include "../kernels/spf_kernels.h"

struct orh_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, evm = nullptr, ev1 = nullptr;  // around phase 1 | phase 2
  size_t lds_limit = 160 * 1024;
  uint32_t n_cu = 256;  // compute units (multi-source batch sizing)
  orh::SpfMode spf_mode = orh::SpfMode::kAuto;  // orh_set_spf_mode
  // ORH_DELTA_PCT: HBM-kernel near/far width in % of the mean live metric;
  // 50 measured best on the C4 WAN what-if batch (25: 12.4, 50: 11.9,
  // 100: 13.1, 200: 17.0, 400: 23.6 ms; log-normal metrics, mean ~3x median)
  uint32_t delta_pct = 50;
  orh_spf_info last_info{};    // orh_last_spf_info
  std::string err;
  orh_counters counters{};
  // reusable device staging for the exact kernel's request arrays
  uint32_t* d_req = nullptr;
  size_t d_req_cap = 0;
  // distance rows of neighbours that are not themselves requested sources
  uint32_t* d_scratch = nullptr;
  size_t d_scratch_cap = 0;  // in u32
  // HBM kernel with fused first hops: {dist, nh} labels per row
  unsigned long long* d_labels = nullptr;
  size_t d_labels_cap = 0;  // in labels
  // multi-source BFS: u8 level row per row (first-hop input)
  uint8_t* d_lvl_rows = nullptr;
  size_t d_lvl_rows_cap = 0;  // in bytes
  // lean first-hop kernel: per half (p2_half) redo count, redo list and
  // row_deep flags (orh::hop_aux_bytes)
  uint8_t* d_hop_aux = nullptr;
  size_t d_hop_aux_cap = 0;  // in bytes, both halves
  // multi-source BFS: node-major level bytes
  uint8_t* d_ms_lvl = nullptr;
  size_t d_ms_lvl_cap = 0;
  // deferred second phase (ORH_SPF_DEFER_HOPS): finalize + first hops of a
  // sweep on stream2 while the context stream takes the next sweep's search.
  // The level bytes alternate between two halves of d_ms_lvl; a search into
  // half b first waits for the phase 2 still reading it (ev_p2[b])
  hipStream_t stream2 = nullptr;
  hipEvent_t ev_ms2 = nullptr;                // end of the search phase 2 follows
  hipEvent_t ev_p2[2] = {nullptr, nullptr};   // end of the phase 2 reading half b
  bool p2_pending[2] = {false, false};        // ev_p2[b] not yet joined
  uint32_t p2_half = 0;                       // half of the next deferred sweep
  // orh_spf_batch's device rows (reused: a hipMalloc/hipFree pair per call
  // costs more than a single-source SPF)
  uint32_t* d_batch = nullptr;
  size_t d_batch_cap = 0;  // in u32
  // mirror-patch staging (positions + records of one delta batch)
  uint32_t* d_patch = nullptr;
  size_t d_patch_cap = 0;  // in u32
  // exact kernel: per-row heap state when it does not fit in LDS, and
  // orh_spf_batch_exact's device rows
  uint8_t* d_exact = nullptr;
  size_t d_exact_cap = 0;  // in bytes
  uint8_t* d_batch_x = nullptr;
  size_t d_batch_x_cap = 0;  // in bytes
  uint8_t* d_ksp = nullptr;  // orh_ksp2_batch: rows, traces' scratch and output
  size_t d_ksp_cap = 0;
  uint32_t* h_ksp = nullptr;  // orh_ksp2_batch's pinned output blocks
  size_t h_ksp_cap = 0;       // in u32
  uint8_t* d_rep_slots = nullptr;  // global repair slots (requests that outgrow LDS)
  size_t d_rep_slots_cap = 0;
  const orh_whatif* slots_owner = nullptr;  // the what-if job using them (one at a time)
  uint32_t* h_pinned = nullptr;  // orh_spf_batch_pinned's host rows (hipHostMalloc)
  size_t h_pinned_cap = 0;       // in u32
  // ORH_WHATIF_REPAIR: 0 off, 1 automatic (sources repeat, small ignore
  // sets), 2 every ignore-set batch the repair can take
  int repair_mode = 1;
  uint32_t rep_cap_a = 0, rep_cap_e = 0;  // LDS repair caps; 0 = by graph size (ORH_REPAIR_CAPS=A,E)
};

// orh_spf_run's request as staged in orh_graph::d_req (stage_request):
// n_rows | srcs[n_rows] | ign_ptr[n_rows + 1] ign[..] | nbr_ptr[n_src + 1]
// nbr_row[..] | order[n_rows], the offsets in words
struct StagedRequest {
  std::vector<uint32_t> key;  // graph generation + sources + ignore sets; empty: nothing staged
  uint32_t n_rows = 0;        // sources + neighbour rows
  uint32_t off_ign_ptr = 0, off_ign = 0, off_nbr_ptr = 0, off_nbr_row = 0, off_order = 0, off_order_ms = 0;
  uint32_t xcd_group = 0;  // HopArgs::xcd_group
};

struct orh_graph {
  orh_ctx* ctx = nullptr;
  // process-wide unique id of the uploaded structure (new on every load), so
  // a context's staged request can never match a different or reloaded graph
  // even when a new orh_graph reuses a freed one's address
  uint64_t gen = 0;
  uint32_t n_nodes = 0, n_edges = 0, n_links = 0;
  // host CSR (ABI semantics) kept for deltas, neighbour tables and bounds
  std::vector<uint32_t> row_ptr, col, w_out, w_in, meta;
  std::vector<uint32_t> ent_row;  // entry -> row (entry_rows), valid for ent_row_gen
  uint64_t ent_row_gen = ~0ull;
  std::vector<uint8_t> overloaded;
  std::vector<uint32_t> dn_ptr, dn;  // distinct neighbours per node, ascending id
  std::vector<uint16_t> rank_out;    // per CSR entry: col's rank among row's distinct neighbours
  uint64_t sum_max_metric = 0;       // sum over up CSR entries of max(w_out, w_in)
  uint32_t max_metric = 0;
  uint32_t min_out = 0, max_out = 0;  // w_out range over up CSR entries
  uint32_t mean_out = 1;               // mean w_out over up CSR entries
  bool has_zero = false;               // an up CSR entry has w_out == 0
  std::vector<uint32_t> name_rank;     // orh_csr::name_rank (identity when not given)
  uint32_t* d_name_rank = nullptr;
  // device layout: ELL slots v*K .. v*K+K-1, the last one a continuation
  // record into the overflow area when deg(v) > K
  uint32_t ell_k = 4;
  uint32_t n_recs = 0;
  std::vector<uint32_t> pos;  // CSR entry -> device record index
  uint2* d_recs = nullptr;
  uint32_t* d_link = nullptr;
  uint16_t* d_rank_out = nullptr;
  uint8_t* d_ovl = nullptr;
  // multi-source layouts: the same ELL records in a Cuthill-McKee node
  // order (neighbours get nearby ids, so a batch of consecutive sources is a
  // compact region and a wave's 64 nodes progress together); the BFS of a
  // deep graph has an order of its own (msb_*, below). Rebuilt lazily
  // after attribute patches. Rows in HBM are always indexed by host id.
  std::vector<uint32_t> ms_dev_of, ms_host_of;  // host -> CM id, CM id -> host
  bool ms_identity = false;  // the layout kept the host order (order_nodes)
  bool ms_dirty = true;
  uint32_t ms_bw = 0;  // CM bandwidth over live records when the interval skip is on, else 0
  uint32_t ms_bw_layout = 1;  // the same bandwidth whatever the opt-in (latency-plan skip)
  uint2* d_ms_recs = nullptr;
  uint32_t* d_ms_dev_of = nullptr;
  uint32_t* d_ms_host_of = nullptr;
  // the multi-source BFS's own node order (ms_cluster_order, host/ms_order.h):
  // runs of 64 ids that are compact clusters. ms_cluster: the graph has one
  // (order_nodes decides); then ms_recs, the BFS batches and the BFS kernels'
  // id maps use msb_*, while the multi-source Bellman-Ford layouts, whose
  // band cuts lean on Cuthill-McKee's band structure, keep ms_dev_of /
  // ms_host_of. Without it the BFS shares those
  std::vector<uint32_t> msb_dev_of, msb_host_of;
  bool ms_cluster = false;
  uint32_t ms_cm_depth = 0;  // deepest level of Cuthill-McKee's own BFS (order_nodes)
  uint32_t wms_bw = 1;       // bandwidth of the Cuthill-McKee ids over live records (kWms's skip)
  uint32_t* d_msb_dev_of = nullptr;
  uint32_t* d_msb_host_of = nullptr;
  // slice adjacency of the multi-source BFS layout (ms_slice_adjacency,
  // host/ms_order.h) as the kernel's bitmasks [slices][kMsAdjWords], rebuilt
  // with the layout; empty past kMsAdjSlices slices. ms_adj_on: the sweeps
  // take the adjacency skip (cluster order by default, ORH_MS_ADJ)
  std::vector<uint32_t> ms_adj_words;
  bool ms_adj_on = false, ms_adj_forced = false;
  uint32_t* d_ms_adj = nullptr;
  // multi-source Bellman-Ford (kWms): in-link slots per Cuthill-McKee node,
  // rebuilt with the multi-source layout; wms_ok: the graph qualifies (every
  // degree <= 8, metrics < 2^15, N < 20,481); wms_k slots per node (4 or 8)
  uint32_t* d_wms = nullptr;
  bool wms_dirty = true, wms_ok = false;
  uint32_t wms_maxw = 0, wms_k = 4;
  uint32_t wms_maxdeg = 0;  // largest CSR row, as of the last sync_wms_layout
  // sliced multi-source Bellman-Ford (kWmsSliced): the same slot words for
  // any degree, column-major per 64-node slice (sync_wms_sliced_layout).
  // d_wsl: slots | slice offsets [slices + 1] | band starts for 4, 8 and 16
  // waves (5 + 9 + 17 words) | the 8-byte slots of the wide kernel
  // (kWmsWide), when asked for; wsl_ok: N <= 20,480 and live metrics
  // 1..0x7FFF; wsl_wide: the 8-byte slots are there (N <= 20,480, live
  // metrics >= 1); wsl_maxw: the largest live metric
  uint32_t* d_wsl = nullptr;
  size_t d_wsl_cap = 0;  // in u32
  bool wsl_dirty = true, wsl_ok = false, wsl_ovl = false, wsl_wide = false;
  uint32_t wsl_maxw = 0, wsl_block = 1024;
  size_t wsl_off_at = 0, wsl_band_at = 0, wsl_wide_at = 0;  // word offsets into d_wsl
  uint32_t wsl_real = 0, wsl_padded = 0;   // live in-links, slots (padding included)
  std::vector<int32_t> row_of;  // scratch for orh_spf_run (all -1 between calls)
  // orh_spf_run's staged request on this graph (sources, ignore sets,
  // neighbour rows, batch order), keyed by the request: a repeated sweep
  // neither rebuilds nor uploads it, even when several graphs share a context
  uint32_t* d_req = nullptr;
  size_t d_req_cap = 0;
  StagedRequest staged;
  // what-if repair: per record, the record of the same link from the other
  // end; per link, its two CSR entries (~0 when absent); valid for rev_gen
  uint32_t* d_rev = nullptr;
  uint64_t rev_gen = 0;
  std::vector<uint32_t> link_ent;  // [2 * n_links]
};

// What more than one unit calls. Hidden: none of it is part of the library's
// dynamic symbol table (tests/test_abi.py)
#pragma GCC visibility push(hidden)
namespace orh::api {

inline int fail(orh_ctx* ctx, int code, const std::string& msg) {
  if (ctx) ctx->err = msg;
  return code;
}

inline int hip_fail(orh_ctx* ctx, hipError_t e, const char* what) {
  return fail(ctx, ORH_E_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
}

#define ORH_HIP(ctx, call)                                 \
  do {                                                     \
    hipError_t e_ = (call);                                \
    if (e_ != hipSuccess) return hip_fail(ctx, e_, #call); \
  } while (0)

// ---- orh_api.hip: contexts
void join_deferred(orh_ctx* ctx);
void drain_deferred(orh_ctx* ctx);
bool device_busy_elsewhere(const orh_ctx* ctx);
int grow_device(orh_ctx* ctx, void** p, size_t* cap, size_t need, size_t elem, bool drain);
template <class T>  // *p holds *cap elements of T
int grow_device(orh_ctx* ctx, T** p, size_t* cap, size_t need, bool drain) {
  return grow_device(ctx, reinterpret_cast<void**>(p), cap, need, sizeof(T), drain);
}
inline int ensure_labels(orh_ctx* ctx, size_t n) { return grow_device(ctx, &ctx->d_labels, &ctx->d_labels_cap, n, false); }
inline int ensure_bytes(orh_ctx* ctx, uint8_t** p, size_t* cap, size_t bytes) { return grow_device(ctx, p, cap, bytes, false); }

// ---- orh_api.hip: graph mirrors
inline uint32_t n_distinct(const orh_graph* g, uint32_t v) { return g->dn_ptr[v + 1] - g->dn_ptr[v]; }
bool wide_metrics(const orh_graph* g);
const std::vector<uint32_t>& entry_rows(orh_graph* g);
int sync_ms_layout(orh_graph* g);
int sync_wms_layout(orh_graph* g);
int sync_wms_sliced_layout(orh_graph* g, bool wide);

// ---- spf.hip
int run_exact(orh_graph* g, const orh_spf_request* req, uint32_t words, uint32_t* d_dist32, uint64_t* d_dist64,
              uint32_t* d_nh, uint32_t* d_rank);

// ---- whatif.hip
int ensure_rev(orh_graph* g);
bool repair_eligible(orh_graph* g, const orh_spf_request* req, uint32_t words);
int run_repair(orh_graph* g, const orh_spf_request* req, uint32_t* d_dist, uint32_t* d_nh);

}  // namespace orh::api
#pragma GCC visibility pop
