// libopenr_hip: C ABI (include/openr_hip.h) over the gfx950 SPF kernels.
//
// Owns per-device contexts (stream, events, counters, request staging,
// scratch distance rows) and per-area graph mirrors (ELL edge records, link
// ids, node flags and the neighbour-rank table that numbers first-hop bits).
#include "api/orh_internal.h"
#include "host/ms_order.h"
#include "kernels/whatif_kernels.h"

using namespace orh::api;

namespace {

void free_graph_device(orh_graph* g) {
  (void)hipFree(g->d_recs);
  (void)hipFree(g->d_link);
  (void)hipFree(g->d_rank_out);
  (void)hipFree(g->d_ovl);
  (void)hipFree(g->d_ms_recs);
  (void)hipFree(g->d_ms_dev_of);
  (void)hipFree(g->d_ms_host_of);
  (void)hipFree(g->d_msb_dev_of);
  (void)hipFree(g->d_msb_host_of);
  g->d_msb_dev_of = nullptr;
  g->d_msb_host_of = nullptr;
  (void)hipFree(g->d_ms_adj);
  g->d_ms_adj = nullptr;
  (void)hipFree(g->d_name_rank);
  (void)hipFree(g->d_rev);
  g->d_rev = nullptr;
  (void)hipFree(g->d_req);
  g->d_req = nullptr;
  g->d_req_cap = 0;
  g->staged.key.clear();
  g->rev_gen = 0;
  g->d_name_rank = nullptr;
  g->d_ms_recs = nullptr;
  g->d_ms_dev_of = nullptr;
  g->d_ms_host_of = nullptr;
  g->ms_dirty = true;
  (void)hipFree(g->d_wms);
  g->d_wms = nullptr;
  g->wms_dirty = true;
  (void)hipFree(g->d_wsl);
  g->d_wsl = nullptr;
  g->d_wsl_cap = 0;
  g->wsl_dirty = true;
  g->d_recs = nullptr;
  g->d_link = nullptr;
  g->d_rank_out = nullptr;
  g->d_ovl = nullptr;
}

// distinct neighbour lists and, per CSR entry, the neighbour's rank in its
// row's list (= the first-hop bit of that neighbour)
void build_neighbours(orh_graph* g) {
  const uint32_t N = g->n_nodes;
  g->dn_ptr.assign(N + 1, 0);
  g->dn.clear();
  g->rank_out.assign(g->n_edges, 0);
  std::vector<uint32_t> l;
  for (uint32_t v = 0; v < N; ++v) {
    l.clear();
    for (uint32_t e = g->row_ptr[v]; e < g->row_ptr[v + 1]; ++e)
      if (g->meta[e] != ORH_META_EMPTY) l.push_back(g->col[e]);
    std::sort(l.begin(), l.end());
    l.erase(std::unique(l.begin(), l.end()), l.end());
    for (uint32_t e = g->row_ptr[v]; e < g->row_ptr[v + 1]; ++e)
      g->rank_out[e] = g->meta[e] == ORH_META_EMPTY
          ? 0
          : static_cast<uint16_t>(std::lower_bound(l.begin(), l.end(), g->col[e]) - l.begin());
    g->dn.insert(g->dn.end(), l.begin(), l.end());
    g->dn_ptr[v + 1] = static_cast<uint32_t>(g->dn.size());
  }
}

// ELL width: smallest power of two covering 90% of the node degrees, in [4, 8]
uint32_t choose_ell_k(const orh_graph* g) {
  std::vector<uint32_t> deg(g->n_nodes);
  for (uint32_t v = 0; v < g->n_nodes; ++v) deg[v] = g->row_ptr[v + 1] - g->row_ptr[v];
  if (deg.empty()) return 4;
  std::nth_element(deg.begin(), deg.begin() + deg.size() * 9 / 10, deg.end());
  return deg[deg.size() * 9 / 10] > 4 ? 8 : 4;
}

// The node orders of the multi-source layouts (host/ms_order.h): Cuthill-McKee
// for all of them, the cluster order for the multi-source BFS of deep graphs
void order_nodes(orh_graph* g) {
  const uint32_t N = g->n_nodes;
  auto& host_of = g->ms_host_of;
  auto& dev_of = g->ms_dev_of;
  const uint32_t depth = orh::ms_cm_order(N, g->dn_ptr.data(), g->dn.data(), host_of, dev_of);
  g->ms_cm_depth = depth;
  // ORH_MS_ORDER=host (A/B): the host order itself. Its slices are runs of
  // host ids, so the multi-source BFS writes the u32 distance rows straight
  // from its level assembly (no ms_finalize pass) and a wave's gathers read
  // neighbours at the same offsets (v +- 1, v +- n on a grid numbered row by
  // row) instead of across anti-diagonal boundaries. Measured slower on the
  // C2 grid, so Cuthill-McKee stays the default: the 32-sweep step 24.2-24.6
  // ms against 22.9, one sweep 1.10 against 0.93 ms (the host-order BFS 0.75
  // against 0.64 ms, the direct rows another 0.13 ms in it for 0.06 ms of
  // phase 2; profiles/r06/j_ms_ab.txt). ORH_MS_ORDER=cm forces the default
  const char* fe = getenv("ORH_MS_ORDER");  // read per layout (tests set it per graph)
  g->ms_identity = fe && strcmp(fe, "host") == 0;
  if (g->ms_identity)
    for (uint32_t v = 0; v < N; ++v) dev_of[v] = host_of[v] = v;
  // The multi-source BFS's order. Cuthill-McKee's 64-node slices are pieces of
  // a BFS level (on the C2 grid: of an anti-diagonal, 126 hops end to end), so
  // every slice stays short of some bit for ~100 levels and its arrivals come
  // a few lanes at a time; the search pays per (slice, level), not per node.
  // The cluster order makes the slices compact (ms_cluster_order;
  // tools/ms_order_model.py: 0.40x the log store instructions and 0.64x the
  // open slice-levels on C2). That only pays where arrivals spread over many
  // levels: by default a graph takes it when Cuthill-McKee's own BFS is at
  // least kMsClusterDepth levels deep (a Clos is 4-6 deep and keeps
  // Cuthill-McKee; DESIGN.md section 5 has the measurements).
  // ORH_MS_ORDER=cluster / cm force either
  constexpr uint32_t kMsClusterDepth = 32;
  g->ms_cluster = !g->ms_identity && N > 0 &&
                  (fe && strcmp(fe, "cluster") == 0 ? true
                   : fe && strcmp(fe, "cm") == 0    ? false
                                                    : depth >= kMsClusterDepth);
  g->msb_dev_of.clear();
  g->msb_host_of.clear();
  if (g->ms_cluster)
    orh::ms_cluster_order(N, g->dn_ptr.data(), g->dn.data(), host_of.data(), dev_of.data(), g->msb_host_of,
                          g->msb_dev_of);
}

// the id maps of the multi-source BFS layout (ms_recs, its batches, its kernels)
const std::vector<uint32_t>& msb_dev_of(const orh_graph* g) { return g->ms_cluster ? g->msb_dev_of : g->ms_dev_of; }
const std::vector<uint32_t>& msb_host_of(const orh_graph* g) {
  return g->ms_cluster ? g->msb_host_of : g->ms_host_of;
}

uint2 device_record(const orh_graph* g, uint32_t v, uint32_t e, const uint32_t* dev_of = nullptr) {
  uint32_t x = dev_of ? dev_of[g->col[e]] : g->col[e];
  if (g->meta[e] & ORH_META_DOWN) x |= ORH_REC_SKIP;
  if (g->overloaded[v]) x |= ORH_REC_ROW_OVL;
  return make_uint2(x, g->w_out[e]);
}

void build_layout(orh_graph* g, std::vector<uint2>& recs, std::vector<uint32_t>& link,
                  std::vector<uint16_t>& rank) {
  const uint32_t K = g->ell_k, N = g->n_nodes;
  size_t n = static_cast<size_t>(N) * K;
  for (uint32_t v = 0; v < N; ++v) {
    const uint32_t d = g->row_ptr[v + 1] - g->row_ptr[v];
    if (d > K) n += d - (K - 1);
  }
  recs.assign(std::max<size_t>(n, 1), make_uint2(ORH_REC_SKIP, 1));
  link.assign(recs.size(), 0);
  rank.assign(recs.size(), 0);
  g->pos.assign(g->n_edges, 0);
  uint32_t ovf = N * K;
  for (uint32_t v = 0; v < N; ++v) {
    const uint32_t e0 = g->row_ptr[v], d = g->row_ptr[v + 1] - e0, base = v * K;
    const uint32_t inl = d <= K ? d : K - 1;
    for (uint32_t j = 0; j < inl; ++j) g->pos[e0 + j] = base + j;
    if (d > K) {
      recs[base + K - 1] = make_uint2(ovf | ORH_REC_CONT, d - inl);
      for (uint32_t j = inl; j < d; ++j) g->pos[e0 + j] = ovf++;
    }
    for (uint32_t j = 0; j < d; ++j) {
      const uint32_t q = g->pos[e0 + j];
      recs[q] = device_record(g, v, e0 + j);
      link[q] = g->meta[e0 + j] & ORH_META_LINK_MASK;
      rank[q] = g->rank_out[e0 + j];
    }
  }
  g->n_recs = static_cast<uint32_t>(recs.size());
}

// the ELL records again, rows and columns in the multi-source BFS's ids
// (cluster order, else Cuthill-McKee)
void build_ms_layout(orh_graph* g, std::vector<uint2>& recs) {
  const uint32_t K = g->ell_k, N = g->n_nodes;
  const std::vector<uint32_t>& dev_of = msb_dev_of(g);
  const std::vector<uint32_t>& host_of = msb_host_of(g);
  recs.assign(g->n_recs, make_uint2(ORH_REC_SKIP, 1));
  uint32_t ovf = N * K, bw = 0, bw_cm = 0;
  auto put = [&](uint32_t q, uint32_t dv, uint32_t v, uint32_t e) {
    recs[q] = device_record(g, v, e, dev_of.data());
    if (!(recs[q].x & ORH_REC_SKIP)) {
      const uint32_t u = recs[q].x & ORH_REC_COL_MASK;
      bw = std::max(bw, u > dv ? u - dv : dv - u);
      const uint32_t cu = g->ms_dev_of[g->col[e]], cv = g->ms_dev_of[v];
      bw_cm = std::max(bw_cm, cu > cv ? cu - cv : cv - cu);
    }
  };
  for (uint32_t dv = 0; dv < N; ++dv) {
    const uint32_t v = host_of[dv];
    const uint32_t e0 = g->row_ptr[v], d = g->row_ptr[v + 1] - e0, base = dv * K;
    const uint32_t inl = d <= K ? d : K - 1;
    for (uint32_t j = 0; j < inl; ++j) put(base + j, dv, v, e0 + j);
    if (d > K) {
      recs[base + K - 1] = make_uint2(ovf | ORH_REC_CONT, d - inl);
      for (uint32_t j = inl; j < d; ++j) put(ovf++, dv, v, e0 + j);
    }
  }
  // the pull OR is order-free, so each node's inline slots are sorted by
  // neighbour id: a slot then reads the same relative neighbour (e.g. "lower
  // anti-diagonal, left") across a wave's consecutive Cuthill-McKee nodes,
  // consecutive frontier words instead of a mix of directions at the border
  // rows (bank conflicts of the ds_read_b32 gathers). ORH_MS_SORT=0: CSR order.
  // (In cluster order, sorting by the neighbour's id minus the owner's - so
  // that a cluster's border lanes keep each direction in one slot - measured
  // the same: 19.54 against 19.56 ms per step, profiles/ms_cluster/step_ab.txt.)
  const char* es = getenv("ORH_MS_SORT");
  if (!(es && atoi(es) == 0)) {
    for (uint32_t dv = 0; dv < N; ++dv) {
      uint2* r = recs.data() + static_cast<size_t>(dv) * K;
      const uint32_t n_inl = (r[K - 1].x & ORH_REC_CONT) ? K - 1 : K;
      std::stable_sort(r, r + n_inl, [](const uint2& a, const uint2& b) {
        const uint32_t ka = (a.x & ORH_REC_SKIP) ? ~0u : (a.x & ORH_REC_COL_MASK);
        const uint32_t kb = (b.x & ORH_REC_SKIP) ? ~0u : (b.x & ORH_REC_COL_MASK);
        return ka < kb;
      });
    }
  }
  // interval skip (spf_msbfs_kernel<..., true>), opt-in with ORH_MS_SKIP=1:
  // it cuts a lone corner batch of the C2 grid from 0.48 to 0.32 ms, but the
  // all-sources sweep stays at 0.75-0.77 ms either way (profiles/r02/
  // msbfs_ab.md: with every CU busy the level-byte stores, not the skipped
  // slices, set the time)
  const char* e = getenv("ORH_MS_SKIP");
  const bool on = e && atoi(e) == 1;
  g->ms_bw = on ? std::max(bw, 1u) : 0u;
  g->ms_bw_layout = std::max(bw, 1u);
  g->wms_bw = std::max(bw_cm, 1u);
  // adjacency skip (spf_msbfs_kernel's kMsSkipAdj): the slices a slice can
  // receive from, over every CSR entry of its nodes - down and drained ones
  // too, and a free slot (its col is the node itself) - so only a change of
  // the rows' neighbours, which rebuilds this layout, can change it. On where
  // the cluster order is (it is what makes the sets small) and the slices fit
  // the kernel's bitmasks; ORH_MS_ADJ=0: off, ORH_MS_ADJ=1: under any order
  std::vector<uint32_t> adj_ptr, adj;
  orh::ms_slice_adjacency(N, g->row_ptr.data(), g->col.data(), dev_of.data(), adj_ptr, adj);
  g->ms_adj_words = orh::ms_adjacency_masks(adj_ptr, adj);
  const char* ea = getenv("ORH_MS_ADJ");
  const bool adj_on = ea && atoi(ea) == 0 ? false : ea && atoi(ea) == 1 ? true : g->ms_cluster;
  g->ms_adj_on = adj_on && !g->ms_adj_words.empty();
  g->ms_adj_forced = g->ms_adj_on && ea && atoi(ea) == 1;
}

uint64_t next_graph_gen() {
  static std::atomic<uint64_t> gen{0};
  return ++gen;
}

// re-upload the device records of CSR entries `edges` (row node, entry) with
// one staging copy and one scatter launch
int upload_records(orh_graph* g, const std::vector<std::pair<uint32_t, uint32_t>>& edges) {
  if (edges.empty()) return ORH_OK;
  orh_ctx* ctx = g->ctx;
  const uint32_t n = static_cast<uint32_t>(edges.size());
  // staging: pos[n] (u32, padded to 8 bytes) | vals[n] (uint2)
  const size_t pos_words = (n + 1) & ~1u;
  std::vector<uint32_t> staging(pos_words + 2 * static_cast<size_t>(n));
  uint2* vals = reinterpret_cast<uint2*>(staging.data() + pos_words);
  for (uint32_t i = 0; i < n; ++i) {
    staging[i] = g->pos[edges[i].second];
    vals[i] = device_record(g, edges[i].first, edges[i].second);
  }
  if (int rc = grow_device(ctx, &ctx->d_patch, &ctx->d_patch_cap, staging.size(), false)) return rc;
  ORH_HIP(ctx, hipMemcpyAsync(ctx->d_patch, staging.data(), staging.size() * sizeof(uint32_t),
                              hipMemcpyHostToDevice, ctx->stream));
  ORH_HIP(ctx, orh::launch_scatter_recs(g->d_recs, ctx->d_patch,
                                        reinterpret_cast<const uint2*>(ctx->d_patch + pos_words), n,
                                        ctx->stream));
  ORH_HIP(ctx, hipStreamSynchronize(ctx->stream));  // staging is a local
  g->ms_dirty = true;
  g->wms_dirty = true;
  g->wsl_dirty = true;
  return ORH_OK;
}

uint32_t row_of(const orh_graph* g, uint32_t e) {
  return static_cast<uint32_t>(std::upper_bound(g->row_ptr.begin(), g->row_ptr.end(), e) -
                               g->row_ptr.begin()) - 1;
}

void recompute_bounds(orh_graph* g) {
  g->sum_max_metric = 0;
  g->max_metric = 0;
  g->min_out = 0xFFFFFFFFu;
  g->max_out = 0;
  g->has_zero = false;
  for (uint32_t e = 0; e < g->n_edges; ++e) {
    if (g->meta[e] & ORH_META_DOWN) continue;
    g->has_zero |= g->w_out[e] == 0;
    const uint32_t m = std::max(g->w_out[e], g->w_in[e]);
    g->max_metric = std::max(g->max_metric, m);
    g->sum_max_metric += m;  // each link is counted twice (both CSR entries)
    g->min_out = std::min(g->min_out, g->w_out[e]);
    g->max_out = std::max(g->max_out, g->w_out[e]);
  }
  if (g->max_out == 0) g->min_out = g->max_out = 1;  // no up link
  uint64_t sum_out = 0, n_up = 0;
  for (uint32_t e = 0; e < g->n_edges; ++e)
    if (!(g->meta[e] & ORH_META_DOWN)) {
      sum_out += g->w_out[e];
      ++n_up;
    }
  g->mean_out = n_up ? static_cast<uint32_t>(sum_out / n_up) : 1u;
}

}  // namespace

// every live context, by device: a sweep planned while no other context of
// its device has a sweep in flight (its end event not reached) takes the
// lone-sweep plan (orh::ms_set_width)
static std::mutex g_ctx_mu;
static std::vector<orh_ctx*> g_ctxs;

namespace orh::api {

bool device_busy_elsewhere(const orh_ctx* ctx) {
  std::lock_guard<std::mutex> lock(g_ctx_mu);
  for (const orh_ctx* o : g_ctxs)
    if (o != ctx && o->device == ctx->device && hipEventQuery(o->ev1) == hipErrorNotReady) return true;
  return false;
}

int sync_ms_layout(orh_graph* g) {
  if (!g->ms_dirty) return ORH_OK;
  orh_ctx* ctx = g->ctx;
  std::vector<uint2> recs;
  build_ms_layout(g, recs);
  if (!g->d_ms_recs) {
    const size_t nn = std::max<uint32_t>(g->n_nodes, 1);
    if (hipMalloc(&g->d_ms_recs, recs.size() * sizeof(uint2)) != hipSuccess ||
        hipMalloc(&g->d_ms_dev_of, nn * sizeof(uint32_t)) != hipSuccess ||
        hipMalloc(&g->d_ms_host_of, nn * sizeof(uint32_t)) != hipSuccess ||
        (g->ms_cluster && (hipMalloc(&g->d_msb_dev_of, nn * sizeof(uint32_t)) != hipSuccess ||
                           hipMalloc(&g->d_msb_host_of, nn * sizeof(uint32_t)) != hipSuccess)) ||
        (!g->ms_adj_words.empty() &&
         hipMalloc(&g->d_ms_adj, g->ms_adj_words.size() * sizeof(uint32_t)) != hipSuccess))
      return fail(ctx, ORH_E_NOMEM, "multi-source layout: device allocation failed");
    if (g->ms_cluster) {
      ORH_HIP(ctx, hipMemcpyAsync(g->d_msb_dev_of, g->msb_dev_of.data(), g->n_nodes * sizeof(uint32_t),
                                  hipMemcpyHostToDevice, ctx->stream));
      ORH_HIP(ctx, hipMemcpyAsync(g->d_msb_host_of, g->msb_host_of.data(), g->n_nodes * sizeof(uint32_t),
                                  hipMemcpyHostToDevice, ctx->stream));
    }
    ORH_HIP(ctx, hipMemcpyAsync(g->d_ms_dev_of, g->ms_dev_of.data(), g->n_nodes * sizeof(uint32_t),
                                hipMemcpyHostToDevice, ctx->stream));
    ORH_HIP(ctx, hipMemcpyAsync(g->d_ms_host_of, g->ms_host_of.data(), g->n_nodes * sizeof(uint32_t),
                                hipMemcpyHostToDevice, ctx->stream));
  }
  ORH_HIP(ctx, hipMemcpyAsync(g->d_ms_recs, recs.data(), recs.size() * sizeof(uint2),
                              hipMemcpyHostToDevice, ctx->stream));
  if (g->d_ms_adj)  // the slice count is the graph's: the size never changes
    ORH_HIP(ctx, hipMemcpyAsync(g->d_ms_adj, g->ms_adj_words.data(), g->ms_adj_words.size() * sizeof(uint32_t),
                                hipMemcpyHostToDevice, ctx->stream));
  ORH_HIP(ctx, hipStreamSynchronize(ctx->stream));  // recs is a local
  g->ms_dirty = false;
  return ORH_OK;
}

// kWms in-link slots: per Cuthill-McKee node dv, ell_k slots {u | w(u -> v)
// << 16 | overloaded(u) << 31}, u the Cuthill-McKee id of the neighbour and
// w the metric of the link from u's side (LinkState.cpp:851-852: the search
// relaxes getMetricFromNode(u)); a down link or an unused slot is u = N
int sync_wms_layout(orh_graph* g) {
  if (!g->wms_dirty) return ORH_OK;
  int rc = sync_ms_layout(g);
  if (rc) return rc;
  const uint32_t N = g->n_nodes;
  uint32_t maxdeg = 0;
  for (uint32_t v = 0; v < N; ++v) maxdeg = std::max(maxdeg, g->row_ptr[v + 1] - g->row_ptr[v]);
  const uint32_t K = maxdeg <= 4 ? 4u : 8u;  // slots per node (its own width, not the ELL's)
  g->wms_k = K;
  g->wms_maxdeg = maxdeg;
  g->wms_ok = N > 0 && N <= 20480 && maxdeg <= 8;
  g->wms_maxw = 0;
  std::vector<uint32_t> slots;
  if (g->wms_ok) {
    slots.assign(static_cast<size_t>(N) * K, N);
    for (uint32_t dv = 0; dv < N && g->wms_ok; ++dv) {
      const uint32_t v = g->ms_host_of[dv];
      uint32_t k = 0;
      for (uint32_t e = g->row_ptr[v]; e < g->row_ptr[v + 1]; ++e, ++k) {
        if (g->meta[e] & ORH_META_DOWN) continue;
        const uint32_t w = g->w_in[e], u = g->col[e];
        if (w == 0 || w > 0x7FFFu) {
          g->wms_ok = false;
          break;
        }
        g->wms_maxw = std::max(g->wms_maxw, w);
        slots[static_cast<size_t>(dv) * K + k] = g->ms_dev_of[u] | (w << 16) | (g->overloaded[u] ? 0x80000000u : 0u);
      }
    }
  }
  if (g->wms_ok) {
    orh_ctx* ctx = g->ctx;
    if (!g->d_wms) ORH_HIP(ctx, hipMalloc(&g->d_wms, static_cast<size_t>(N) * 8 * sizeof(uint32_t)));
    ORH_HIP(ctx, hipMemcpyAsync(g->d_wms, slots.data(), slots.size() * sizeof(uint32_t), hipMemcpyHostToDevice,
                                ctx->stream));
    ORH_HIP(ctx, hipStreamSynchronize(ctx->stream));  // slots is a local
  }
  g->wms_dirty = false;
  return ORH_OK;
}

// kWmsSliced in-link slots: the sync_wms_layout words for a graph of any
// degree, as a sliced ELL over the Cuthill-McKee ids. Slice s is the nodes
// [64 s, 64 s + 64); its width is its largest live in-degree rounded up to 4
// columns (the kernel reads 4 at a time); column k is the 64 words at
// off[s] + 64 k, padding u = N. The waves of a batch own contiguous bands of
// slices: band starts for 4, 8 and 16 waves, cut where the running column
// count (+ 1 per slice, its own label) passes w / waves of the total.
// wsl_block: the widest workgroup that still cuts the heaviest band by a
// tenth against half as many waves (one indivisible wide slice bounds it).
// wide: the 8-byte slots of spf_wms_wide_kernel too, {u | overloaded(u) << 31,
// w} with the full metric, padding {N, 0}, in the same slices, columns and
// bands (one set of offsets serves both slot arrays); a graph whose metrics
// pass 15 bits has these alone (wsl_ok false, wsl_wide true)
int sync_wms_sliced_layout(orh_graph* g, bool wide) {
  if (!g->wsl_dirty && (!wide || g->wsl_wide)) return ORH_OK;
  int rc = sync_ms_layout(g);
  if (rc) return rc;
  const uint32_t N = g->n_nodes;
  bool shape_ok = N > 0 && N <= 20480;  // and no zero metric: what both slot formats need
  g->wsl_maxw = 0;
  g->wsl_ovl = false;
  g->wsl_wide = false;
  g->wsl_real = g->wsl_padded = 0;
  const uint32_t n_slice = (N + 63) / 64;
  std::vector<uint32_t> off(n_slice + 1, 0), deg(N, 0);
  for (uint32_t dv = 0; dv < N && shape_ok; ++dv) {
    const uint32_t v = g->ms_host_of[dv];
    for (uint32_t e = g->row_ptr[v]; e < g->row_ptr[v + 1]; ++e) {
      if (g->meta[e] & ORH_META_DOWN) continue;
      const uint32_t w = g->w_in[e];
      if (w == 0) {
        shape_ok = false;
        break;
      }
      g->wsl_maxw = std::max(g->wsl_maxw, w);
      ++deg[dv];
    }
  }
  g->wsl_ok = shape_ok && g->wsl_maxw <= 0x7FFFu;
  wide = wide && shape_ok;
  if (g->wsl_ok || wide) {
    for (uint32_t s = 0; s < n_slice; ++s) {
      uint32_t width = 0;
      for (uint32_t dv = s * 64; dv < std::min(N, s * 64 + 64); ++dv) width = std::max(width, deg[dv]);
      off[s + 1] = off[s] + ((width + 3u) & ~3u) * 64u;
    }
    const size_t n_slots = off[n_slice];
    const size_t off_at = n_slots, band_at = off_at + n_slice + 1;
    const size_t wide_at = (band_at + 5 + 9 + 17 + 1) & ~size_t{1};  // 8-byte aligned
    const size_t total = wide_at + (wide ? 2 * n_slots : 0);
    std::vector<uint32_t> st(total, N);
    if (wide)  // padding {N, 0}
      for (size_t i = 0; i < n_slots; ++i) st[wide_at + 2 * i + 1] = 0u;
    for (uint32_t dv = 0; dv < N; ++dv) {
      const uint32_t v = g->ms_host_of[dv];
      uint32_t k = 0;
      for (uint32_t e = g->row_ptr[v]; e < g->row_ptr[v + 1]; ++e) {
        if (g->meta[e] & ORH_META_DOWN) continue;
        const uint32_t u = g->col[e];
        if (g->overloaded[u]) g->wsl_ovl = true;
        const size_t at = off[dv / 64] + 64u * k++ + (dv & 63u);
        const uint32_t uw = g->ms_dev_of[u] | (g->overloaded[u] ? 0x80000000u : 0u);
        if (g->wsl_ok) st[at] = uw | (g->w_in[e] << 16);
        if (wide) {
          st[wide_at + 2 * at] = uw;
          st[wide_at + 2 * at + 1] = g->w_in[e];
        }
        ++g->wsl_real;
      }
    }
    g->wsl_padded = static_cast<uint32_t>(n_slots);
    g->wsl_wide = wide;
    g->wsl_wide_at = wide_at;
    std::copy(off.begin(), off.end(), st.begin() + off_at);
    uint64_t all = 0;
    for (uint32_t s = 0; s < n_slice; ++s) all += (off[s + 1] - off[s]) / 64 + 1;
    uint64_t heaviest[3] = {0, 0, 0};
    uint32_t* band = st.data() + band_at;
    for (uint32_t i = 0, waves = 4; i < 3; ++i, band += waves + 1, waves *= 2) {
      uint64_t run = 0;
      uint32_t s = 0;
      for (uint32_t w = 0; w <= waves; ++w) {
        // band w starts at the first slice whose running count reaches w / waves of the total
        while (s < n_slice && w < waves && run * waves < all * w) run += (off[s + 1] - off[s]) / 64 + 1, ++s;
        band[w] = w == waves ? n_slice : s;
      }
      for (uint32_t w = 0; w < waves; ++w) {
        uint64_t c = 0;
        for (uint32_t q = band[w]; q < band[w + 1]; ++q) c += (off[q + 1] - off[q]) / 64 + 1;
        heaviest[i] = std::max(heaviest[i], c);
      }
    }
    g->wsl_block = 256;
    if (heaviest[1] * 10 <= heaviest[0] * 9) {
      g->wsl_block = 512;
      if (heaviest[2] * 10 <= heaviest[1] * 9) g->wsl_block = 1024;
    }
    orh_ctx* ctx = g->ctx;
    if ((rc = grow_device(ctx, &g->d_wsl, &g->d_wsl_cap, st.size(), false))) return rc;
    ORH_HIP(ctx, hipMemcpyAsync(g->d_wsl, st.data(), st.size() * sizeof(uint32_t), hipMemcpyHostToDevice,
                                ctx->stream));
    ORH_HIP(ctx, hipStreamSynchronize(ctx->stream));  // st is a local
    g->wsl_off_at = off_at;
    g->wsl_band_at = band_at;
  }
  g->wsl_dirty = false;
  return ORH_OK;
}

// row of every CSR entry, rebuilt when the structure generation moves (a
// what-if run stages two cuts per ignored link: 131k binary searches over
// row_ptr per 65,536-request C4 chunk otherwise)
const std::vector<uint32_t>& entry_rows(orh_graph* g) {
  if (g->ent_row_gen != g->gen || g->ent_row.size() != g->n_edges) {
    g->ent_row.assign(g->n_edges, 0u);
    for (uint32_t v = 0; v < g->n_nodes; ++v)
      for (uint32_t e = g->row_ptr[v]; e < g->row_ptr[v + 1]; ++e) g->ent_row[e] = v;
    g->ent_row_gen = g->gen;
  }
  return g->ent_row;
}

// deferred second phases: the context stream waits for them (device side)
void join_deferred(orh_ctx* ctx) {
  for (int b = 0; b < 2; ++b)
    if (ctx->p2_pending[b]) {
      hipStreamWaitEvent(ctx->stream, ctx->ev_p2[b], 0);
      ctx->p2_pending[b] = false;
    }
}

// ... or the host waits for them (before a buffer they read is freed or
// rewritten outside the context stream's order)
void drain_deferred(orh_ctx* ctx) {
  if (!ctx->stream2) return;
  hipStreamSynchronize(ctx->stream2);
  ctx->p2_pending[0] = ctx->p2_pending[1] = false;
}

// The one allocate-and-replace behind the reusable device buffers: *p holds
// *cap elements of `elem` bytes. A need that fits returns at once; else the old
// block is freed, after the deferred second phases that may still read it when
// `drain`, and exactly `need` elements take its place (on failure: null, cap 0)
int grow_device(orh_ctx* ctx, void** p, size_t* cap, size_t need, size_t elem, bool drain) {
  if (need <= *cap) return ORH_OK;
  if (drain) drain_deferred(ctx);
  hipFree(*p);
  *p = nullptr;
  *cap = 0;
  ORH_HIP(ctx, hipMalloc(p, need * elem));
  *cap = need;
  return ORH_OK;
}

// path metrics of the graph can reach the 32-bit sentinel (link metrics are
// summed in 64 bits by the reference, LinkState.h:22)
bool wide_metrics(const orh_graph* g) {
  return g->sum_max_metric / 2 + g->max_metric >= 0xFFFFFFFFull;
}

}  // namespace orh::api

extern "C" {

int orh_device_count(int* out) {
  if (!out) return ORH_E_INVALID;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
  *out = n;
  return ORH_OK;
}

int orh_create(int device, uint32_t flags, orh_ctx** out) {
  (void)flags;
  if (!out) return ORH_E_INVALID;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return ORH_E_DEVICE;
  if (device < 0 || device >= n) return ORH_E_INVALID;
  auto* ctx = new (std::nothrow) orh_ctx();
  if (!ctx) return ORH_E_NOMEM;
  ctx->device = device;
  if (hipSetDevice(device) != hipSuccess ||
      hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreate(&ctx->ev0) != hipSuccess || hipEventCreate(&ctx->evm) != hipSuccess ||
      hipEventCreate(&ctx->ev1) != hipSuccess) {
    delete ctx;
    return ORH_E_DEVICE;
  }
  if (const char* e = getenv("ORH_SPF_MODE")) ctx->spf_mode = static_cast<orh::SpfMode>(atoi(e) % orh::kSpfModes);
  if (const char* e = getenv("ORH_DELTA_PCT")) ctx->delta_pct = std::max(1, atoi(e));
  if (const char* e = getenv("ORH_WHATIF_REPAIR")) ctx->repair_mode = atoi(e);
  if (const char* e = getenv("ORH_REPAIR_CAPS")) {
    unsigned ca = 0, ce = 0;
    if (sscanf(e, "%u,%u", &ca, &ce) == 2 && ca >= 64 && ce >= 256) {
      ctx->rep_cap_a = ca;
      ctx->rep_cap_e = ce;
    }
  }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.sharedMemPerBlock > 0) {
    ctx->lds_limit = std::max<size_t>(prop.sharedMemPerBlock, 64 * 1024);
    if (prop.multiProcessorCount > 0) ctx->n_cu = static_cast<uint32_t>(prop.multiProcessorCount);
  }
  {
    std::lock_guard<std::mutex> lock(g_ctx_mu);
    g_ctxs.push_back(ctx);
  }
  *out = ctx;
  return ORH_OK;
}

int orh_set_spf_mode(orh_ctx* ctx, int mode) {
  if (!ctx || mode < 0 || mode >= orh::kSpfModes) return ORH_E_INVALID;
  ctx->spf_mode = static_cast<orh::SpfMode>(mode);
  return ORH_OK;
}

int orh_set_repair_mode(orh_ctx* ctx, int mode) {
  if (!ctx || mode < ORH_REPAIR_OFF || mode > ORH_REPAIR_ALWAYS) return ORH_E_INVALID;
  ctx->repair_mode = mode;
  return ORH_OK;
}

int orh_destroy(orh_ctx* ctx) {
  if (!ctx) return ORH_E_INVALID;
  {
    std::lock_guard<std::mutex> lock(g_ctx_mu);
    g_ctxs.erase(std::remove(g_ctxs.begin(), g_ctxs.end(), ctx), g_ctxs.end());
  }
  hipSetDevice(ctx->device);
  drain_deferred(ctx);
  hipStreamSynchronize(ctx->stream);
  hipFree(ctx->d_req);
  hipFree(ctx->d_scratch);
  hipFree(ctx->d_labels);
  hipFree(ctx->d_lvl_rows);
  hipFree(ctx->d_hop_aux);
  hipFree(ctx->d_ms_lvl);
  hipFree(ctx->d_batch);
  hipFree(ctx->d_patch);
  hipFree(ctx->d_exact);
  hipFree(ctx->d_batch_x);
  hipFree(ctx->d_rep_slots);
  hipFree(ctx->d_ksp);
  if (ctx->h_ksp) hipHostFree(ctx->h_ksp);
  if (ctx->h_pinned) hipHostFree(ctx->h_pinned);
  hipEventDestroy(ctx->ev0);
  hipEventDestroy(ctx->evm);
  hipEventDestroy(ctx->ev1);
  if (ctx->stream2) {
    hipEventDestroy(ctx->ev_ms2);
    hipEventDestroy(ctx->ev_p2[0]);
    hipEventDestroy(ctx->ev_p2[1]);
    hipStreamDestroy(ctx->stream2);
  }
  hipStreamDestroy(ctx->stream);
  delete ctx;
  return ORH_OK;
}

const char* orh_last_error(const orh_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int orh_sync(orh_ctx* ctx) {
  if (!ctx) return ORH_E_INVALID;
  join_deferred(ctx);
  ORH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ORH_OK;
}

int orh_get_counters(const orh_ctx* ctx, orh_counters* out) {
  if (!ctx || !out) return ORH_E_INVALID;
  *out = ctx->counters;
  return ORH_OK;
}

int orh_reset_counters(orh_ctx* ctx) {
  if (!ctx) return ORH_E_INVALID;
  ctx->counters = orh_counters{};
  return ORH_OK;
}

int orh_device_alloc(orh_ctx* ctx, size_t bytes, void** d_out) {
  if (!ctx || !d_out) return ORH_E_INVALID;
  hipSetDevice(ctx->device);
  if (hipMalloc(d_out, std::max<size_t>(bytes, 16)) != hipSuccess)
    return fail(ctx, ORH_E_NOMEM, "device allocation failed");
  return ORH_OK;
}

int orh_device_free(orh_ctx* ctx, void* d_ptr) {
  if (!ctx) return ORH_E_INVALID;
  hipFree(d_ptr);
  return ORH_OK;
}

int orh_memcpy_d2h(orh_ctx* ctx, void* h_dst, const void* d_src, size_t bytes) {
  if (!ctx || (!h_dst && bytes) || (!d_src && bytes)) return ORH_E_INVALID;
  if (!bytes) return ORH_OK;
  join_deferred(ctx);
  ORH_HIP(ctx, hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
  ORH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ORH_OK;
}

int orh_memcpy_h2d(orh_ctx* ctx, void* d_dst, const void* h_src, size_t bytes) {
  if (!ctx || (!d_dst && bytes) || (!h_src && bytes)) return ORH_E_INVALID;
  if (!bytes) return ORH_OK;
  join_deferred(ctx);
  ORH_HIP(ctx, hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, ctx->stream));
  ORH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ORH_OK;
}

int orh_memcpy_d2d(orh_ctx* ctx, void* d_dst, const void* d_src, size_t bytes) {
  if (!ctx || (!d_dst && bytes) || (!d_src && bytes)) return ORH_E_INVALID;
  join_deferred(ctx);
  ORH_HIP(ctx, hipMemcpyAsync(d_dst, d_src, bytes, hipMemcpyDeviceToDevice, ctx->stream));
  ORH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ORH_OK;
}

int orh_row_digest(orh_ctx* ctx, const uint32_t* d_dist, const uint32_t* d_nh, uint32_t words, uint32_t n,
                   uint32_t n_rows, uint64_t* d_out) {
  if (!ctx || words == 0 || (n_rows && (!d_dist || !d_nh || !d_out))) return ORH_E_INVALID;
  if (n_rows == 0) return ORH_OK;
  join_deferred(ctx);
  ORH_HIP(ctx, hipSetDevice(ctx->device));
  ORH_HIP(ctx, orh::launch_row_digest(d_dist, d_nh, words, n, n_rows, d_out, ctx->stream));
  return ORH_OK;
}

int orh_graph_create(orh_ctx* ctx, orh_graph** out) {
  if (!ctx || !out) return ORH_E_INVALID;
  auto* g = new (std::nothrow) orh_graph();
  if (!g) return ORH_E_NOMEM;
  g->ctx = ctx;
  *out = g;
  return ORH_OK;
}

int orh_graph_destroy(orh_graph* g) {
  if (!g) return ORH_E_INVALID;
  hipSetDevice(g->ctx->device);
  drain_deferred(g->ctx);
  hipStreamSynchronize(g->ctx->stream);
  free_graph_device(g);
  delete g;
  return ORH_OK;
}

int orh_graph_load(orh_graph* g, const orh_csr* c) {
  if (!g || !c) return ORH_E_INVALID;
  orh_ctx* ctx = g->ctx;
  drain_deferred(ctx);  // the deferred phase 2 reads the graph
  if (!c->row_ptr || (c->n_edges && (!c->col || !c->w_out || !c->w_in || !c->meta)) ||
      (c->n_nodes && !c->node_overloaded))
    return fail(ctx, ORH_E_INVALID, "orh_graph_load: null array");
  if (c->row_ptr[0] != 0 || c->row_ptr[c->n_nodes] != c->n_edges)
    return fail(ctx, ORH_E_INVALID, "orh_graph_load: row_ptr does not span n_edges");
  if (c->n_nodes > ORH_REC_COL_MASK)
    return fail(ctx, ORH_E_UNSUPPORTED, "orh_graph_load: more than 2^27 nodes");
  for (uint32_t v = 0; v < c->n_nodes; ++v)
    if (c->row_ptr[v] > c->row_ptr[v + 1])
      return fail(ctx, ORH_E_INVALID, "orh_graph_load: row_ptr not monotone");
  for (uint32_t e = 0; e < c->n_edges; ++e)
    if (c->meta[e] != ORH_META_EMPTY && c->col[e] >= c->n_nodes)
      return fail(ctx, ORH_E_INVALID, "orh_graph_load: col out of range");
  if (c->name_rank)
    for (uint32_t v = 0; v < c->n_nodes; ++v)
      if (c->name_rank[v] >= c->n_nodes)
        return fail(ctx, ORH_E_INVALID, "orh_graph_load: name_rank out of range");
  // ORH_LOAD_PROF=1: phase times on stderr
  static const bool prof_on = getenv("ORH_LOAD_PROF") != nullptr;
  auto t_prev = std::chrono::steady_clock::now();
  auto mark = [&](const char* what) {
    if (!prof_on) return;
    const auto now = std::chrono::steady_clock::now();
    fprintf(stderr, "load-prof %-14s %8.3f ms\n", what,
            std::chrono::duration<double, std::milli>(now - t_prev).count());
    t_prev = now;
  };
  ORH_HIP(ctx, hipSetDevice(ctx->device));
  ORH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  free_graph_device(g);
  mark("free");
  g->n_nodes = c->n_nodes;
  g->n_edges = c->n_edges;
  g->n_links = c->n_links;
  g->row_ptr.assign(c->row_ptr, c->row_ptr + c->n_nodes + 1);
  g->col.assign(c->col, c->col + c->n_edges);
  g->w_out.assign(c->w_out, c->w_out + c->n_edges);
  g->w_in.assign(c->w_in, c->w_in + c->n_edges);
  g->meta.assign(c->meta, c->meta + c->n_edges);
  for (uint32_t v = 0; v < c->n_nodes; ++v)  // free slots point at their own row
    for (uint32_t e = c->row_ptr[v]; e < c->row_ptr[v + 1]; ++e)
      if (g->meta[e] == ORH_META_EMPTY) g->col[e] = v;
  g->overloaded.assign(c->node_overloaded, c->node_overloaded + c->n_nodes);
  for (auto& o : g->overloaded) o = o ? 1 : 0;
  g->name_rank.resize(c->n_nodes);
  for (uint32_t v = 0; v < c->n_nodes; ++v) g->name_rank[v] = c->name_rank ? c->name_rank[v] : v;
  g->gen = next_graph_gen();
  g->row_of.assign(g->n_nodes, -1);
  mark("copy-in");
  recompute_bounds(g);
  mark("bounds");
  build_neighbours(g);
  mark("neighbours");
  for (uint32_t v = 0; v < g->n_nodes; ++v)
    if (n_distinct(g, v) > 0xFFFFu)
      return fail(ctx, ORH_E_UNSUPPORTED, "orh_graph_load: more than 65535 neighbours");
  g->ell_k = choose_ell_k(g);
  order_nodes(g);
  mark("order");
  std::vector<uint2> recs;
  std::vector<uint32_t> link;
  std::vector<uint16_t> rank;
  build_layout(g, recs, link, rank);
  mark("layout");
  const size_t nn = std::max<uint32_t>(g->n_nodes, 1);
  if (hipMalloc(&g->d_recs, recs.size() * sizeof(uint2)) != hipSuccess ||
      hipMalloc(&g->d_link, link.size() * sizeof(uint32_t)) != hipSuccess ||
      hipMalloc(&g->d_rank_out, rank.size() * sizeof(uint16_t)) != hipSuccess ||
      hipMalloc(&g->d_ovl, nn) != hipSuccess ||
      hipMalloc(&g->d_name_rank, nn * sizeof(uint32_t)) != hipSuccess) {
    free_graph_device(g);
    return fail(ctx, ORH_E_NOMEM, "orh_graph_load: device allocation failed");
  }
  ORH_HIP(ctx, hipMemcpyAsync(g->d_recs, recs.data(), recs.size() * sizeof(uint2),
                              hipMemcpyHostToDevice, ctx->stream));
  ORH_HIP(ctx, hipMemcpyAsync(g->d_link, link.data(), link.size() * sizeof(uint32_t),
                              hipMemcpyHostToDevice, ctx->stream));
  ORH_HIP(ctx, hipMemcpyAsync(g->d_rank_out, rank.data(), rank.size() * sizeof(uint16_t),
                              hipMemcpyHostToDevice, ctx->stream));
  if (g->n_nodes) {
    ORH_HIP(ctx, hipMemcpyAsync(g->d_ovl, g->overloaded.data(), g->n_nodes, hipMemcpyHostToDevice,
                                ctx->stream));
    ORH_HIP(ctx, hipMemcpyAsync(g->d_name_rank, g->name_rank.data(), g->n_nodes * sizeof(uint32_t),
                                hipMemcpyHostToDevice, ctx->stream));
  }
  ORH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  mark("upload");
  return ORH_OK;
}

int orh_graph_patch_edges(orh_graph* g, uint32_t n, const uint32_t* idx, const uint32_t* w_out,
                          const uint32_t* w_in, const uint32_t* meta) {
  if (!g || (n && (!idx || !w_out || !w_in || !meta))) return ORH_E_INVALID;
  orh_ctx* ctx = g->ctx;
  drain_deferred(ctx);  // the deferred phase 2 reads the graph
  if (!g->d_recs && n) return fail(ctx, ORH_E_STATE, "orh_graph_patch_edges: no graph loaded");
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t e = idx[i];
    if (e >= g->n_edges) return fail(ctx, ORH_E_INVALID, "orh_graph_patch_edges: bad edge index");
    if ((meta[i] & ORH_META_LINK_MASK) != (g->meta[e] & ORH_META_LINK_MASK))
      return fail(ctx, ORH_E_INVALID, "orh_graph_patch_edges: link id changed (use orh_graph_apply_delta)");
    if (g->meta[e] == ORH_META_EMPTY && meta[i] != ORH_META_EMPTY)
      return fail(ctx, ORH_E_INVALID, "orh_graph_patch_edges: free slot (use orh_graph_apply_delta)");
  }
  ORH_HIP(ctx, hipSetDevice(ctx->device));
  std::vector<std::pair<uint32_t, uint32_t>> edges;
  edges.reserve(n);
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t e = idx[i];
    g->w_out[e] = w_out[i];
    g->w_in[e] = w_in[i];
    g->meta[e] = meta[i] & ~ORH_META_COL_OVERLOADED;
    edges.emplace_back(row_of(g, e), e);
  }
  std::sort(edges.begin(), edges.end());
  edges.erase(std::unique(edges.begin(), edges.end()), edges.end());
  int rc = upload_records(g, edges);
  if (rc) return rc;
  recompute_bounds(g);
  return ORH_OK;
}

int orh_graph_apply_delta(orh_graph* g, uint32_t n_rows, const uint32_t* rows, const uint32_t* ptr,
                          const uint32_t* col, const uint32_t* w_out, const uint32_t* w_in,
                          const uint32_t* meta, uint32_t n_links) {
  if (!g || (n_rows && (!rows || !ptr))) return ORH_E_INVALID;
  orh_ctx* ctx = g->ctx;
  drain_deferred(ctx);  // the deferred phase 2 reads the graph
  if (!g->d_recs) return fail(ctx, ORH_E_STATE, "orh_graph_apply_delta: no graph loaded");
  const uint32_t N = g->n_nodes;
  if (n_rows && ptr[0] != 0) return fail(ctx, ORH_E_INVALID, "orh_graph_apply_delta: ptr[0] != 0");
  std::vector<uint8_t> seen(N, 0);
  for (uint32_t i = 0; i < n_rows; ++i) {
    const uint32_t v = rows[i];
    if (v >= N || seen[v]) return fail(ctx, ORH_E_INVALID, "orh_graph_apply_delta: bad or repeated row");
    seen[v] = 1;
    if (ptr[i + 1] < ptr[i]) return fail(ctx, ORH_E_INVALID, "orh_graph_apply_delta: ptr not monotone");
    if (ptr[i + 1] - ptr[i] > g->row_ptr[v + 1] - g->row_ptr[v])
      return fail(ctx, ORH_E_UNSUPPORTED, "orh_graph_apply_delta: row " + std::to_string(v) +
                                              " outgrows its capacity (reload)");
  }
  const uint32_t n_ent = n_rows ? ptr[n_rows] : 0u;
  if (n_ent && (!col || !w_out || !w_in || !meta)) return fail(ctx, ORH_E_INVALID, "orh_graph_apply_delta: null array");
  for (uint32_t k = 0; k < n_ent; ++k) {
    if (col[k] >= N) return fail(ctx, ORH_E_INVALID, "orh_graph_apply_delta: col out of range");
    if (meta[k] != ORH_META_EMPTY && (meta[k] & ORH_META_LINK_MASK) >= std::max<uint32_t>(n_links, 1))
      return fail(ctx, ORH_E_INVALID, "orh_graph_apply_delta: link id >= n_links");
  }
  ORH_HIP(ctx, hipSetDevice(ctx->device));
  for (uint32_t i = 0; i < n_rows; ++i) {
    const uint32_t v = rows[i], e0 = g->row_ptr[v], cap = g->row_ptr[v + 1] - e0;
    const uint32_t d = ptr[i + 1] - ptr[i];
    for (uint32_t j = 0; j < cap; ++j) {
      const uint32_t e = e0 + j;
      if (j < d) {
        const uint32_t k = ptr[i] + j;
        g->col[e] = meta[k] == ORH_META_EMPTY ? v : col[k];
        g->w_out[e] = w_out[k];
        g->w_in[e] = w_in[k];
        g->meta[e] = meta[k] == ORH_META_EMPTY ? meta[k] : meta[k] & ~ORH_META_COL_OVERLOADED;
      } else {
        g->col[e] = v;
        g->w_out[e] = g->w_in[e] = 1;
        g->meta[e] = ORH_META_EMPTY;
      }
    }
  }
  g->n_links = n_links;
  build_neighbours(g);
  for (uint32_t i = 0; i < n_rows; ++i)
    if (n_distinct(g, rows[i]) > 0xFFFFu)
      return fail(ctx, ORH_E_UNSUPPORTED, "orh_graph_apply_delta: more than 65535 neighbours (reload)");
  recompute_bounds(g);
  // the changed rows' device records, link ids and neighbour ranks
  std::vector<uint32_t> pos;
  std::vector<uint2> vals;
  std::vector<uint32_t> links;
  std::vector<uint16_t> ranks;
  for (uint32_t i = 0; i < n_rows; ++i) {
    const uint32_t v = rows[i];
    for (uint32_t e = g->row_ptr[v]; e < g->row_ptr[v + 1]; ++e) {
      pos.push_back(g->pos[e]);
      vals.push_back(device_record(g, v, e));
      links.push_back(g->meta[e] & ORH_META_LINK_MASK);
      ranks.push_back(g->rank_out[e]);
    }
  }
  const uint32_t n = static_cast<uint32_t>(pos.size());
  if (n) {
    // staging: pos u32[n] | links u32[n] | vals uint2[n] | ranks u16[n]
    const size_t words = 2 * size_t{n} + 2 * size_t{n} + (size_t{n} + 1) / 2;
    std::vector<uint32_t> st(words, 0);
    std::memcpy(st.data(), pos.data(), 4 * size_t{n});
    std::memcpy(st.data() + n, links.data(), 4 * size_t{n});
    std::memcpy(st.data() + 2 * size_t{n}, vals.data(), 8 * size_t{n});
    std::memcpy(st.data() + 4 * size_t{n}, ranks.data(), 2 * size_t{n});
    if (int rc = grow_device(ctx, &ctx->d_patch, &ctx->d_patch_cap, st.size(), false)) return rc;
    ORH_HIP(ctx, hipMemcpyAsync(ctx->d_patch, st.data(), st.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    ORH_HIP(ctx, orh::launch_scatter_rows(
                     g->d_recs, g->d_link, g->d_rank_out, ctx->d_patch,
                     reinterpret_cast<const uint2*>(ctx->d_patch + 2 * size_t{n}), ctx->d_patch + n,
                     reinterpret_cast<const uint16_t*>(ctx->d_patch + 4 * size_t{n}), n, ctx->stream));
    ORH_HIP(ctx, hipStreamSynchronize(ctx->stream));  // staging is a local
  }
  g->ms_dirty = true;
  g->wms_dirty = true;
  g->wsl_dirty = true;
  g->gen = next_graph_gen();  // staged requests hold neighbour lists of the old rows
  return ORH_OK;
}

int orh_graph_patch_nodes(orh_graph* g, uint32_t n, const uint32_t* idx, const uint8_t* ovl) {
  if (!g || (n && (!idx || !ovl))) return ORH_E_INVALID;
  orh_ctx* ctx = g->ctx;
  drain_deferred(ctx);  // the deferred phase 2 reads the graph
  if (!g->d_recs && n) return fail(ctx, ORH_E_STATE, "orh_graph_patch_nodes: no graph loaded");
  for (uint32_t i = 0; i < n; ++i)
    if (idx[i] >= g->n_nodes) return fail(ctx, ORH_E_INVALID, "orh_graph_patch_nodes: bad node");
  ORH_HIP(ctx, hipSetDevice(ctx->device));
  std::vector<std::pair<uint32_t, uint32_t>> edges;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t v = idx[i];
    g->overloaded[v] = ovl[i] ? 1 : 0;
    // v's own records carry its row bit
    for (uint32_t e = g->row_ptr[v]; e < g->row_ptr[v + 1]; ++e) edges.emplace_back(v, e);
  }
  std::sort(edges.begin(), edges.end());
  edges.erase(std::unique(edges.begin(), edges.end()), edges.end());
  if (n && g->n_nodes)  // the whole flag array: one copy instead of one per node
    ORH_HIP(ctx, hipMemcpyAsync(g->d_ovl, g->overloaded.data(), g->n_nodes, hipMemcpyHostToDevice,
                                ctx->stream));
  int rc = upload_records(g, edges);  // synchronizes the stream
  if (rc) return rc;
  ORH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ORH_OK;
}

int orh_graph_device_flags(const orh_graph* g, const uint8_t** d_overloaded) {
  if (!g || !d_overloaded) return ORH_E_INVALID;
  if (!g->d_ovl) return fail(g->ctx, ORH_E_STATE, "orh_graph_device_flags: no graph loaded");
  *d_overloaded = g->d_ovl;
  return ORH_OK;
}

int orh_graph_flags(const orh_graph* g, uint32_t* flags) {
  if (!g || !flags) return ORH_E_INVALID;
  *flags = (g->has_zero ? ORH_GRAPH_ZERO_METRIC : 0u) | (wide_metrics(g) ? ORH_GRAPH_WIDE_METRIC : 0u);
  return ORH_OK;
}

int orh_graph_info(const orh_graph* g, uint32_t* n_nodes, uint32_t* n_edges) {
  if (!g) return ORH_E_INVALID;
  if (n_nodes) *n_nodes = g->n_nodes;
  if (n_edges) *n_edges = g->n_edges;
  return ORH_OK;
}

int orh_graph_ms_order(const orh_graph* g, uint32_t* out, uint32_t cap, uint32_t* kind) {
  if (!g || (cap && !out)) return ORH_E_INVALID;
  const std::vector<uint32_t>& host_of = msb_host_of(g);
  for (uint32_t i = 0; i < g->n_nodes && i < cap; ++i) out[i] = host_of[i];
  if (kind) *kind = g->ms_cluster ? ORH_MS_ORDER_CLUSTER : g->ms_identity ? ORH_MS_ORDER_HOST : ORH_MS_ORDER_CM;
  return ORH_OK;
}

int orh_graph_neighbors(const orh_graph* g, uint32_t src, uint32_t* out, uint32_t cap,
                        uint32_t* n_out) {
  if (!g || !n_out) return ORH_E_INVALID;
  if (src >= g->n_nodes) return ORH_E_INVALID;
  const uint32_t n = n_distinct(g, src);
  *n_out = n;
  for (uint32_t i = 0; i < n && i < cap; ++i) out[i] = g->dn[g->dn_ptr[src] + i];
  return ORH_OK;
}

int orh_spf_words(const orh_graph* g, const uint32_t* srcs, uint32_t n, uint32_t* out) {
  if (!g || !out || (n && !srcs)) return ORH_E_INVALID;
  uint32_t mx = 1;
  for (uint32_t i = 0; i < n; ++i) {
    if (srcs[i] >= g->n_nodes) return ORH_E_INVALID;
    mx = std::max(mx, n_distinct(g, srcs[i]));
  }
  *out = (mx + 31) / 32;
  return ORH_OK;
}

}  // extern "C"

// timing helper used by bench/tests through the ABI: elapsed ms of the last
// SPF launch (waits for it)
extern "C" int orh_last_spf_ms(orh_ctx* ctx, double* ms_out) {
  if (!ctx || !ms_out) return ORH_E_INVALID;
  ORH_HIP(ctx, hipEventSynchronize(ctx->ev1));
  float ms = 0.f;
  ORH_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
  *ms_out = ms;
  ctx->counters.last_kernel_ms = ms;
  ctx->counters.total_kernel_ms += ms;
  return ORH_OK;
}

extern "C" int orh_last_spf_info(const orh_ctx* ctx, orh_spf_info* out) {
  if (!ctx || !out) return ORH_E_INVALID;
  *out = ctx->last_info;
  return ORH_OK;
}

extern "C" int orh_last_spf_phase_ms(orh_ctx* ctx, double* dist_ms, double* hop_ms) {
  if (!ctx || !dist_ms || !hop_ms) return ORH_E_INVALID;
  ORH_HIP(ctx, hipEventSynchronize(ctx->ev1));
  float a = 0.f, b = 0.f;
  ORH_HIP(ctx, hipEventElapsedTime(&a, ctx->ev0, ctx->evm));
  ORH_HIP(ctx, hipEventElapsedTime(&b, ctx->evm, ctx->ev1));
  *dist_ms = a;
  *hop_ms = b;
  return ORH_OK;
}
