// KSP2: the sources' rows, the host traces (orh_ksp2) and the device batch
// (orh_ksp2_batch).
#include "orh_internal.h"
#include "../kernels/ksp_kernels.h"

using namespace orh::api;

namespace {

// one source's SPF row as the KSP2 traces read it: u64 distances (~0 =
// unreachable) and, from the exact kernel, the extraction rank (else empty:
// extraction order is (distance, name rank))
struct KspRow {
  std::vector<uint64_t> dist;
  std::vector<uint32_t> rank;
};

// rows for `n` searches from src (ignore sets ign_ptr / ign, or none), in
// chunks that bound the device and host buffers
int ksp_rows(orh_graph* g, uint32_t src, uint32_t n, const uint32_t* ign_ptr, const uint32_t* ign,
             std::vector<KspRow>& rows) {
  orh_ctx* ctx = g->ctx;
  const uint32_t N = g->n_nodes;
  uint32_t words = 1;
  int rc = orh_spf_words(g, &src, 1, &words);
  if (rc) return rc;
  const bool exact = g->has_zero || wide_metrics(g);
  const uint32_t chunk = static_cast<uint32_t>(std::max<size_t>(1, (size_t{256} << 20) / (size_t{N} * (12 + 4 * words))));
  rows.resize(n);
  std::vector<uint32_t> srcs, ptr;
  std::vector<uint32_t> d32;
  for (uint32_t r0 = 0; r0 < n; r0 += chunk) {
    const uint32_t m = std::min(chunk, n - r0);
    srcs.assign(m, src);
    orh_spf_request req{};
    req.h_srcs = srcs.data();
    req.n_src = m;
    req.use_link_metric = 1;
    if (ign_ptr) {
      ptr.assign(m + 1, 0);
      for (uint32_t i = 0; i <= m; ++i) ptr[i] = ign_ptr[r0 + i] - ign_ptr[r0];
      req.h_ignore_ptr = ptr.data();
      req.h_ignore_links = ign + ign_ptr[r0];
      if (ptr[m] == 0) req.h_ignore_links = ptr.data();  // non-null, nothing read
    }
    const size_t nd = static_cast<size_t>(m) * N;
    const size_t bytes = nd * 8 + nd * 4 + nd * 4 * words;
    rc = ensure_bytes(ctx, &ctx->d_batch_x, &ctx->d_batch_x_cap, bytes);
    if (rc) return rc;
    uint64_t* dd64 = reinterpret_cast<uint64_t*>(ctx->d_batch_x);
    uint32_t* drank = reinterpret_cast<uint32_t*>(dd64 + nd);
    uint32_t* dnh = drank + nd;
    if (exact) {
      rc = run_exact(g, &req, words, nullptr, dd64, dnh, drank);
    } else {
      rc = orh_spf_run(g, &req, words, reinterpret_cast<uint32_t*>(dd64), dnh);
    }
    if (rc) return rc;
    if (exact) {
      std::vector<uint64_t> h(nd);
      std::vector<uint32_t> hr(nd);
      ORH_HIP(ctx, hipMemcpyAsync(h.data(), dd64, nd * 8, hipMemcpyDeviceToHost, ctx->stream));
      ORH_HIP(ctx, hipMemcpyAsync(hr.data(), drank, nd * 4, hipMemcpyDeviceToHost, ctx->stream));
      ORH_HIP(ctx, hipStreamSynchronize(ctx->stream));
      for (uint32_t i = 0; i < m; ++i) {
        rows[r0 + i].dist.assign(h.begin() + size_t{i} * N, h.begin() + size_t{i + 1} * N);
        rows[r0 + i].rank.assign(hr.begin() + size_t{i} * N, hr.begin() + size_t{i + 1} * N);
      }
    } else {
      d32.resize(nd);
      ORH_HIP(ctx, hipMemcpyAsync(d32.data(), dd64, nd * 4, hipMemcpyDeviceToHost, ctx->stream));
      ORH_HIP(ctx, hipStreamSynchronize(ctx->stream));
      for (uint32_t i = 0; i < m; ++i) {
        auto& d = rows[r0 + i].dist;
        d.resize(N);
        for (uint32_t v = 0; v < N; ++v) {
          const uint32_t x = d32[size_t{i} * N + v];
          d[v] = x == ORH_UNREACHABLE ? ~0ull : x;
        }
        rows[r0 + i].rank.clear();
      }
    }
  }
  return ORH_OK;
}

// NodeSpfResult::pathLinks of v (LinkState.cpp:857-873 insertion order):
// (link id, prev) over live, non-ignored CSR entries v <- u with
// dist[u] + metric(u -> v) == dist[v], u extracted before v and transit
// (u == src or not overloaded); by u's extraction order, then the link's
// position in u's row
void ksp_path_links(const orh_graph* g, uint32_t src, const KspRow& row, uint32_t v,
                    const std::vector<uint32_t>& ign, std::vector<std::pair<uint32_t, uint32_t>>& out) {
  out.clear();
  const uint64_t dv = row.dist[v];
  if (dv == ~0ull || v == src) return;
  struct Cand {
    uint64_t k1;
    uint32_t k2, pos, link, prev;
  };
  std::vector<Cand> c;
  for (uint32_t e = g->row_ptr[v]; e < g->row_ptr[v + 1]; ++e) {
    if (g->meta[e] & ORH_META_DOWN) continue;
    const uint32_t link = g->meta[e] & ORH_META_LINK_MASK;
    if (!ign.empty() && std::binary_search(ign.begin(), ign.end(), link)) continue;
    const uint32_t u = g->col[e];
    const uint64_t du = row.dist[u];
    if (du == ~0ull) continue;
    if (u != src && g->overloaded[u]) continue;
    if (du + g->w_in[e] != dv) continue;
    if (!row.rank.empty() && row.rank[u] > row.rank[v]) continue;
    uint32_t pos = 0;
    for (uint32_t f = g->row_ptr[u]; f < g->row_ptr[u + 1]; ++f, ++pos)
      if ((g->meta[f] & ORH_META_LINK_MASK) == link && g->col[f] == v) break;
    if (row.rank.empty()) c.push_back({du, g->name_rank[u], pos, link, u});
    else c.push_back({row.rank[u], 0u, pos, link, u});
  }
  std::sort(c.begin(), c.end(), [](const Cand& a, const Cand& b) {
    if (a.k1 != b.k1) return a.k1 < b.k1;
    if (a.k2 != b.k2) return a.k2 < b.k2;
    return a.pos < b.pos;
  });
  for (const auto& x : c) out.emplace_back(x.link, x.prev);
}

// traceOnePath (LinkState.cpp:398-419): greedy DFS dst -> src; a link is
// consumed on first touch even when its branch fails. false = no path.
bool ksp_trace(const orh_graph* g, uint32_t src, uint32_t dst, const KspRow& row,
               const std::vector<uint32_t>& ign, std::vector<uint8_t>& visited,
               std::vector<uint32_t>& path) {
  if (src == dst) return true;
  std::vector<std::pair<uint32_t, uint32_t>> links;
  ksp_path_links(g, src, row, dst, ign, links);
  for (const auto& [link, prev] : links) {
    if (visited[link]) continue;
    visited[link] = 1;
    if (ksp_trace(g, src, prev, row, ign, visited, path)) {
      path.push_back(link);
      return true;
    }
  }
  return false;
}

// successive traces sharing one visited-link set (LinkState.cpp:778-787)
std::vector<std::vector<uint32_t>> ksp_paths(const orh_graph* g, uint32_t src, uint32_t dst,
                                             const KspRow& row, const std::vector<uint32_t>& ign) {
  std::vector<std::vector<uint32_t>> paths;
  if (src != dst && row.dist[dst] == ~0ull) return paths;
  std::vector<uint8_t> visited(std::max<uint32_t>(g->n_links, 1), 0);
  for (;;) {
    std::vector<uint32_t> p;
    if (!ksp_trace(g, src, dst, row, ign, visited, p) || p.empty()) break;
    paths.push_back(std::move(p));
  }
  return paths;
}

}  // namespace

extern "C" {

int orh_ksp2(orh_graph* g, uint32_t src, const uint32_t* dsts, uint32_t n_dst, uint32_t* out,
             size_t cap, size_t* n_words) {
  if (!g || !n_words || (n_dst && !dsts) || (cap && !out)) return ORH_E_INVALID;
  orh_ctx* ctx = g->ctx;
  join_deferred(ctx);
  if (!g->d_recs || g->n_nodes == 0) return fail(ctx, ORH_E_STATE, "orh_ksp2: no graph loaded");
  if (src >= g->n_nodes) return fail(ctx, ORH_E_INVALID, "orh_ksp2: source out of range");
  for (uint32_t i = 0; i < n_dst; ++i)
    if (dsts[i] >= g->n_nodes) return fail(ctx, ORH_E_INVALID, "orh_ksp2: destination out of range");
  for (uint32_t e = 0; e < g->n_edges; ++e)
    if (g->meta[e] != ORH_META_EMPTY && (g->meta[e] & ORH_META_LINK_MASK) >= std::max<uint32_t>(g->n_links, 1))
      return fail(ctx, ORH_E_INVALID, "orh_ksp2: link id >= n_links");
  // k = 1: src's own SPF
  std::vector<KspRow> base;
  int rc = ksp_rows(g, src, 1, nullptr, nullptr, base);
  if (rc) return rc;
  const std::vector<uint32_t> none;
  std::vector<std::vector<std::vector<uint32_t>>> k1(n_dst), k2(n_dst);
  std::vector<uint32_t> ptr(1, 0), ign;
  std::vector<std::vector<uint32_t>> sets(n_dst);
  for (uint32_t i = 0; i < n_dst; ++i) {
    k1[i] = ksp_paths(g, src, dsts[i], base[0], none);
    for (const auto& p : k1[i]) sets[i].insert(sets[i].end(), p.begin(), p.end());
    std::sort(sets[i].begin(), sets[i].end());
    sets[i].erase(std::unique(sets[i].begin(), sets[i].end()), sets[i].end());
  }
  // k = 2: one fresh SPF per destination whose k = 1 paths exist; without
  // k = 1 links the memoized row serves (LinkState.cpp:775-776)
  std::vector<uint32_t> fresh;
  for (uint32_t i = 0; i < n_dst; ++i) {
    if (sets[i].empty()) continue;
    fresh.push_back(i);
    ign.insert(ign.end(), sets[i].begin(), sets[i].end());
    ptr.push_back(static_cast<uint32_t>(ign.size()));
  }
  std::vector<KspRow> rows;
  if (!fresh.empty()) {
    rc = ksp_rows(g, src, static_cast<uint32_t>(fresh.size()), ptr.data(), ign.data(), rows);
    if (rc) return rc;
  }
  for (uint32_t i = 0, f = 0; i < n_dst; ++i) {
    if (sets[i].empty()) {
      k2[i] = ksp_paths(g, src, dsts[i], base[0], none);
    } else {
      k2[i] = ksp_paths(g, src, dsts[i], rows[f++], sets[i]);
    }
  }
  size_t need = 0;
  for (uint32_t i = 0; i < n_dst; ++i)
    for (const auto* ks : {&k1[i], &k2[i]}) {
      need += 1;
      for (const auto& p : *ks) need += 1 + p.size();
    }
  *n_words = need;
  if (need > cap) return cap ? fail(ctx, ORH_E_INVALID, "orh_ksp2: output buffer too small") : ORH_OK;
  size_t w = 0;
  for (uint32_t i = 0; i < n_dst; ++i)
    for (const auto* ks : {&k1[i], &k2[i]}) {
      out[w++] = static_cast<uint32_t>(ks->size());
      for (const auto& p : *ks) {
        out[w++] = static_cast<uint32_t>(p.size());
        for (uint32_t l : p) out[w++] = l;
      }
    }
  return ORH_OK;
}

// KSP2 for a batch of (src, dst) pairs on the device: the sources' plain
// rows, the k = 1 traces (ksp_trace_kernel), the k = 2 searches with each
// pair's k = 1 links ignored (spf_global_nh kernel over the pairs that have
// k = 1 paths), the k = 2 traces; only the paths leave the device
constexpr uint32_t kKspOutCap = 1024, kKspIgnCap = 512, kKspHashCap = 2048, kKspStackCap = 1024;
constexpr uint32_t kKspChunk = 2048;

int orh_ksp2_batch(orh_graph* g, uint32_t n_pairs, const uint32_t* h_src, const uint32_t* h_dst,
                   const uint32_t** out_blocks, uint32_t* block_words) {
  if (!g || !out_blocks || !block_words || (n_pairs && (!h_src || !h_dst))) return ORH_E_INVALID;
  orh_ctx* ctx = g->ctx;
  join_deferred(ctx);
  if (!g->d_recs || g->n_nodes == 0) return fail(ctx, ORH_E_STATE, "orh_ksp2_batch: no graph loaded");
  if (g->has_zero || wide_metrics(g))
    return fail(ctx, ORH_E_UNSUPPORTED, "orh_ksp2_batch: zero / 64-bit path metrics need the exact kernel's order");
  const uint32_t N = g->n_nodes;
  for (uint32_t i = 0; i < n_pairs; ++i)
    if (h_src[i] >= N || h_dst[i] >= N) return fail(ctx, ORH_E_INVALID, "orh_ksp2_batch: node out of range");
  *block_words = kKspOutCap;
  const size_t out_words = static_cast<size_t>(n_pairs) * kKspOutCap;
  if (out_words > ctx->h_ksp_cap) {
    if (ctx->h_ksp) hipHostFree(ctx->h_ksp);
    ctx->h_ksp = nullptr;
    ctx->h_ksp_cap = 0;
    ORH_HIP(ctx, hipHostMalloc(reinterpret_cast<void**>(&ctx->h_ksp), std::max<size_t>(out_words, 1) * 4,
                               hipHostMallocDefault));
    ctx->h_ksp_cap = std::max<size_t>(out_words, 1);
  }
  *out_blocks = ctx->h_ksp;
  if (n_pairs == 0) return ORH_OK;
  hipSetDevice(ctx->device);
  int rc = ensure_rev(g);
  if (rc) return rc;
  const uint64_t bound = g->sum_max_metric / 2 + g->max_metric;
  const bool uniform = g->min_out == g->max_out;
  uint32_t chunk = kKspChunk;  // ORH_KSP_CHUNK: pairs per device pass (A/B)
  if (const char* e = getenv("ORH_KSP_CHUNK")) chunk = std::max(1, atoi(e));
  // ORH_KSP_PROF=1: host and device (events) time of each stage on stderr
  const bool prof = getenv("ORH_KSP_PROF") != nullptr;
  constexpr int kStages = 7;
  static const char* const kStageName[kStages] = {"stage", "k1 search", "k1 trace", "k2 search", "k2 trace",
                                                  "copy-out", ""};
  hipEvent_t ev[kStages] = {};
  double host_ms[kStages] = {};
  auto h_now = [] { return std::chrono::steady_clock::now(); };
  auto t_host = h_now();
  auto mark = [&](int k) {
    if (!prof) return;
    if (!ev[k]) hipEventCreate(&ev[k]);
    hipEventRecord(ev[k], ctx->stream);
    const auto t = h_now();
    host_ms[k] += std::chrono::duration<double, std::milli>(t - t_host).count();
    t_host = t;
  };
  for (uint32_t c0 = 0; c0 < n_pairs; c0 += chunk) {
    mark(0);
    const uint32_t P = std::min(chunk, n_pairs - c0);
    // distinct sources of the chunk, and each pair's row among them
    std::vector<uint32_t> srcs, row1(P), rowp(P);
    auto& ro = g->row_of;
    for (uint32_t i = 0; i < P; ++i) {
      const uint32_t x = h_src[c0 + i];
      if (ro[x] < 0) {
        ro[x] = static_cast<int32_t>(srcs.size());
        srcs.push_back(x);
      }
      row1[i] = static_cast<uint32_t>(ro[x]);
      rowp[i] = i;
    }
    for (uint32_t x : srcs) ro[x] = -1;
    const uint32_t S = static_cast<uint32_t>(srcs.size());
    // device layout (u32 words): the staged request first - src | dst | row1 |
    // rowp | ign_ptr [P+1] | sources [S] | stop targets - then dist1 [S][N] |
    // dist2 [P][N] | ign [P][cap] | need2 | out | visited | stack
    // (the traces read distances only: both searches run dist-only)
    const size_t nd1 = static_cast<size_t>(S) * N, nd2 = static_cast<size_t>(P) * N;
    size_t off = 0;
    auto take = [&](size_t words_) {
      const size_t o = off;
      off += (words_ + 63) & ~size_t{63};  // 256-byte aligned pieces
      return o;
    };
    const size_t o_src = take(P), o_dst = take(P), o_r1 = take(P), o_rp = take(P), o_ip = take(P + 1);
    const size_t o_s1 = take(S);
    // early-stop targets of the searches: the k = 1 row of a source stops once
    // all its pairs' destinations are final, a k = 2 row once its pair's is
    const size_t o_sp1 = take(S + 1), o_sn1 = take(P), o_sp2 = take(P + 1);
    const size_t staged = off;  // words uploaded in one copy
    const size_t o_d1 = take(nd1), o_d2 = take(nd2);
    const size_t o_ign = take(size_t{P} * kKspIgnCap), o_need = take(P), o_out = take(size_t{P} * kKspOutCap);
    const size_t o_vis = take(size_t{P} * kKspHashCap);
    const size_t o_st = take(size_t{P} * kKspStackCap * (sizeof(orh::KspFrame) / 4));
    const size_t o_ovf = take(size_t{std::max(S, P)} + 1);
    const size_t o_ord = take(P);  // k = 2 search order (longest first)
    rc = ensure_bytes(ctx, &ctx->d_ksp, &ctx->d_ksp_cap, off * 4);
    if (rc) return rc;
    uint32_t* D = reinterpret_cast<uint32_t*>(ctx->d_ksp);
    // the staged request is assembled in this chunk's pinned output block
    // (its copy-out comes later on the same stream) and goes up in one copy
    uint32_t* H = ctx->h_ksp + size_t{c0} * kKspOutCap;
    if (staged > size_t{P} * kKspOutCap) return fail(ctx, ORH_E_INVALID, "orh_ksp2_batch: staging block too small");
    std::memcpy(H + o_src, h_src + c0, P * 4ull);
    std::memcpy(H + o_dst, h_dst + c0, P * 4ull);
    std::memcpy(H + o_r1, row1.data(), P * 4ull);
    std::memcpy(H + o_rp, rowp.data(), P * 4ull);
    for (uint32_t i = 0; i <= P; ++i) H[o_ip + i] = i * kKspIgnCap;  // fixed-stride ignore lists
    std::memcpy(H + o_s1, srcs.data(), S * 4ull);
    const char* stop_e = getenv("ORH_KSP_STOP");  // 0: full searches (A/B)
    const bool stop = !(stop_e && stop_e[0] == '0');
    if (stop) {
      uint32_t* sp1 = H + o_sp1;
      std::fill(sp1, sp1 + S + 1, 0u);
      for (uint32_t i = 0; i < P; ++i) ++sp1[row1[i] + 1];
      for (uint32_t r = 0; r < S; ++r) sp1[r + 1] += sp1[r];
      std::vector<uint32_t> fill(sp1, sp1 + S);
      for (uint32_t i = 0; i < P; ++i) H[o_sn1 + fill[row1[i]]++] = h_dst[c0 + i];
      for (uint32_t i = 0; i <= P; ++i) H[o_sp2 + i] = i;
    }
    ORH_HIP(ctx, hipMemcpyAsync(D, H, staged * 4ull, hipMemcpyHostToDevice, ctx->stream));
    ORH_HIP(ctx, hipMemsetAsync(D + o_vis, 0, size_t{P} * kKspHashCap * 4, ctx->stream));
    // both searches: the HBM frontier kernel, distances only (u32 labels)
    orh::SpfPlan fp = orh::plan_spf(N, uniform, bound, g->ell_k, ctx->lds_limit, false, orh::SpfMode::kGlobal);
    if (fp.variant == orh::SpfVariant::kUnsupported)
      return fail(ctx, ORH_E_UNSUPPORTED, "orh_ksp2_batch: no search plan for this graph");
    fp.variant = orh::SpfVariant::kGlobalNh;
    auto block_for = [&](uint32_t rows) { return rows <= ctx->n_cu ? 1024u : rows <= 2 * ctx->n_cu ? 512u : 256u; };
    // one search per CU with u16 distances in LDS when they fit (the HBM
    // kernel finishes any row that needs wider distances); ORH_KSP_LDS=0: the
    // HBM kernel for every row (A/B)
    const char* lds_e = getenv("ORH_KSP_LDS");
    const bool lds_env = !(lds_e && lds_e[0] == '0');
    const bool use_lds16 = lds_env && orh::lds16_bytes(N) <= ctx->lds_limit;
    auto search = [&](const orh::SpfArgs& sa, uint32_t rows) {
      return use_lds16 ? orh::launch_spf_lds16(fp, sa, rows, g->ell_k, ctx->stream)
                       : orh::launch_spf(fp, sa, rows, ctx->stream);
    };
    rc = ensure_labels(ctx, (std::max(nd1, nd2) + 1) / 2);  // u64 units, u32 labels
    if (rc) return rc;
    orh::SpfArgs a{};
    a.n_nodes = N;
    a.recs = g->d_recs;
    a.link = g->d_link;
    a.use_link_metric = 1;
    a.w0 = g->max_out;
    a.delta = uniform ? a.w0
                      : std::max<uint32_t>(1u, static_cast<uint32_t>(
                                                   static_cast<uint64_t>(g->mean_out) * ctx->delta_pct / 100u));
    a.scratch = ctx->d_scratch;
    a.labels = ctx->d_labels;
    a.words = 1;
    a.rank_out = g->d_rank_out;
    a.dist_only = 1;
    a.ovf_rows = D + o_ovf;
    // k = 1 rows: the sources' plain SPFs (LinkState::getSpfResult), as far
    // as their pairs' destinations (the rows feed the k = 1 traces only)
    a.n_out = S;
    a.srcs = D + o_s1;
    a.out_dist = D + o_d1;
    a.stop_ptr = stop ? D + o_sp1 : nullptr;
    a.stop_nodes = stop ? D + o_sn1 : nullptr;
    fp.block = block_for(S);
    const orh_counters c_before = ctx->counters;
    mark(1);
    hipError_t e = search(a, S);
    if (e != hipSuccess) return hip_fail(ctx, e, "ksp2 k=1 search launch");
    mark(2);
    orh::KspArgs ka{};
    ka.n_nodes = N;
    ka.n_pairs = P;
    ka.recs = g->d_recs;
    ka.link = g->d_link;
    ka.rev = g->d_rev;
    ka.name_rank = g->d_name_rank;
    ka.src = D + o_src;
    ka.dst = D + o_dst;
    ka.ign = D + o_ign;
    ka.ign_cap = kKspIgnCap;
    ka.need2 = D + o_need;
    ka.out = D + o_out;
    ka.out_cap = kKspOutCap;
    ka.visited = D + o_vis;
    ka.hash_cap = kKspHashCap;
    ka.stack = reinterpret_cast<orh::KspFrame*>(D + o_st);
    ka.stack_cap = kKspStackCap;
    ka.k = 1;
    ka.row = D + o_r1;
    ka.dist = D + o_d1;
    e = orh::launch_ksp_trace(ka, g->ell_k, ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "ksp2 k=1 trace launch");
    mark(3);
    // k = 2 searches: every pair with k = 1 paths, its k = 1 links ignored
    // (row mask = need2)
    a.n_out = P;
    a.srcs = D + o_src;
    a.ignore_ptr = D + o_ip;
    a.ignore_links = D + o_ign;
    a.out_dist = D + o_d2;
    a.row_mask = D + o_need;
    a.stop_ptr = stop ? D + o_sp2 : nullptr;
    a.stop_nodes = stop ? D + o_dst : nullptr;
    // the LDS searches start with the pairs whose k = 1 destination is
    // farthest (ORH_KSP_ORDER=0: pair order, A/B)
    static const bool by_dist = [] {
      const char* oe = getenv("ORH_KSP_ORDER");
      return !(oe && oe[0] == '0');
    }();
    if (use_lds16 && by_dist && P <= 4096) {
      e = orh::launch_ksp_order(D + o_d1, D + o_r1, D + o_dst, D + o_need, N, P, D + o_ord, ctx->stream);
      if (e != hipSuccess) return hip_fail(ctx, e, "ksp2 order launch");
      a.row_order = D + o_ord;
    }
    fp.block = block_for(P);
    e = search(a, P);
    a.row_order = nullptr;
    if (e != hipSuccess) return hip_fail(ctx, e, "ksp2 k=2 search launch");
    mark(4);
    ORH_HIP(ctx, hipMemsetAsync(D + o_vis, 0, size_t{P} * kKspHashCap * 4, ctx->stream));
    ka.k = 2;
    ka.row = D + o_rp;
    ka.dist = D + o_d2;
    e = orh::launch_ksp_trace(ka, g->ell_k, ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "ksp2 k=2 trace launch");
    mark(5);
    ORH_HIP(ctx, hipMemcpyAsync(ctx->h_ksp + size_t{c0} * kKspOutCap, D + o_out, size_t{P} * kKspOutCap * 4,
                                hipMemcpyDeviceToHost, ctx->stream));
    mark(6);
    ORH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->counters = c_before;  // the caller counts runs the reference's way (memo)
    ctx->counters.spf_launches += 3;
    if (prof) {  // stage k: host time to issue it, device time between its events
      for (int k = 0; k + 1 < kStages; ++k) {
        float d = 0.f;
        hipEventElapsedTime(&d, ev[k], ev[k + 1]);
        std::fprintf(stderr, "ksp-batch %-10s host %8.3f ms  device %8.3f ms\n", kStageName[k], host_ms[k + 1], d);
      }
      std::fprintf(stderr, "ksp-batch after copy-out sync host %8.3f ms\n",
                   std::chrono::duration<double, std::milli>(h_now() - t_host).count());
      if (use_lds16) {
        uint32_t n_ovf = 0;
        ORH_HIP(ctx, hipMemcpy(&n_ovf, D + o_ovf, 4, hipMemcpyDeviceToHost));
        std::fprintf(stderr, "ksp-batch lds16: %u of %u k=2 rows re-run by the HBM kernel\n", n_ovf, P);
      }
      for (double& h : host_ms) h = 0;
    }
  }
  if (prof)
    for (auto& e : ev)
      if (e) hipEventDestroy(e);
  return ORH_OK;
}

}  // extern "C"
