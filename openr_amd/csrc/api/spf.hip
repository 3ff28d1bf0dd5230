// SPF sweeps: the exact kernel's runs, orh_spf_run and its steps (staging, plan
// choice, phases 1 and 2), the batch forms and the _exact forms.
#include "orh_internal.h"

using namespace orh::api;

// ---- orh_spf_run's steps ----------------------------------------------------
namespace {

// The sweep's buffers over grow_device (orh_api.hip); `true`: a deferred
// second phase may read the buffer, so it is drained first. The request
// staging grows to at least 4,096 words. (Unlike its old copy, ensure_req now
// leaves a zero cap, not the stale one, behind a failed allocation.)
int ensure_req(orh_ctx* ctx, size_t words) {
  if (words <= ctx->d_req_cap) return ORH_OK;
  return grow_device(ctx, &ctx->d_req, &ctx->d_req_cap, std::max<size_t>(words, 4096), false);
}
int ensure_graph_req(orh_graph* g, size_t words) {
  if (words <= g->d_req_cap) return ORH_OK;
  g->staged.key.clear();
  return grow_device(g->ctx, &g->d_req, &g->d_req_cap, std::max<size_t>(words, 4096), false);
}
int ensure_lvl_rows(orh_ctx* ctx, size_t n) { return grow_device(ctx, &ctx->d_lvl_rows, &ctx->d_lvl_rows_cap, n, true); }
int ensure_hop_aux(orh_ctx* ctx, size_t n) { return grow_device(ctx, &ctx->d_hop_aux, &ctx->d_hop_aux_cap, n, true); }
int ensure_scratch(orh_ctx* ctx, size_t n) { return grow_device(ctx, &ctx->d_scratch, &ctx->d_scratch_cap, n, true); }
int ensure_ms_lvl(orh_ctx* ctx, size_t n) { return grow_device(ctx, &ctx->d_ms_lvl, &ctx->d_ms_lvl_cap, n, true); }

// what the steps know of a request
struct SweepFacts {
  uint32_t n_src, n_rows;  // requested sources; staged rows (sources + neighbour rows)
  uint32_t max_nbr, words;  // most distinct neighbours of a source; first-hop words per node
  bool uniform, has_ign;
  uint32_t w0;  // the metric of every link when uniform
  uint32_t flags;
  int32_t use_link_metric;
};

// Stages the request in g->d_req, unless the request staged there already is
// this one (g->staged.key). Phase 1 computes a distance row for every
// requested source and for every distinct neighbour of one (the first-hop
// phase reads them). Without ignore sets rows are shared by node: a neighbour
// that is itself requested reuses its output row, the others get scratch
// rows. With per-source ignore sets a source's neighbour rows are its own
// (same ignore set).
int stage_request(orh_graph* g, const orh_spf_request* req, bool has_ign) {
  orh_ctx* ctx = g->ctx;
  const uint32_t n_src = req->n_src;
  const uint32_t n_ign = has_ign ? req->h_ignore_ptr[n_src] : 0u;
  StagedRequest st;
  // request key: graph generation + sources + ignore sets
  std::vector<uint32_t>& key = st.key;
  key.reserve(6 + n_src + (has_ign ? n_src + 1 + n_ign : 0));
  const uint64_t gp = reinterpret_cast<uintptr_t>(g);
  key.insert(key.end(), {static_cast<uint32_t>(gp), static_cast<uint32_t>(gp >> 32),
                         static_cast<uint32_t>(g->gen), static_cast<uint32_t>(g->gen >> 32),
                         n_src, has_ign ? 1u : 0u});
  key.insert(key.end(), req->h_srcs, req->h_srcs + n_src);
  if (has_ign) {
    key.insert(key.end(), req->h_ignore_ptr, req->h_ignore_ptr + n_src + 1);
    key.insert(key.end(), req->h_ignore_links, req->h_ignore_links + n_ign);
  }
  if (g->staged.key == key) return ORH_OK;
  std::vector<uint32_t> srcs(req->h_srcs, req->h_srcs + n_src), nbr_ptr(n_src + 1, 0), nbr_row;
  std::vector<uint32_t> ign_ptr, ign;
  if (!has_ign) {
    auto& ro = g->row_of;
    for (uint32_t i = 0; i < n_src; ++i)
      if (ro[req->h_srcs[i]] < 0) ro[req->h_srcs[i]] = static_cast<int32_t>(i);
    for (uint32_t i = 0; i < n_src; ++i) {
      const uint32_t s = req->h_srcs[i];
      for (uint32_t k = g->dn_ptr[s]; k < g->dn_ptr[s + 1]; ++k) {
        const uint32_t u = g->dn[k];
        if (ro[u] < 0) {
          ro[u] = static_cast<int32_t>(srcs.size());
          srcs.push_back(u);
        }
        nbr_row.push_back(static_cast<uint32_t>(ro[u]));
      }
      nbr_ptr[i + 1] = static_cast<uint32_t>(nbr_row.size());
    }
    for (uint32_t u : srcs) ro[u] = -1;
  } else {
    ign_ptr.assign(1, 0);
    auto add_set = [&](uint32_t i) {
      std::vector<uint32_t> s(req->h_ignore_links + req->h_ignore_ptr[i],
                              req->h_ignore_links + req->h_ignore_ptr[i + 1]);
      std::sort(s.begin(), s.end());  // bsearch on device
      ign.insert(ign.end(), s.begin(), s.end());
      ign_ptr.push_back(static_cast<uint32_t>(ign.size()));
    };
    for (uint32_t i = 0; i < n_src; ++i) add_set(i);
    for (uint32_t i = 0; i < n_src; ++i) {
      const uint32_t s = req->h_srcs[i];
      for (uint32_t k = g->dn_ptr[s]; k < g->dn_ptr[s + 1]; ++k) {
        nbr_row.push_back(static_cast<uint32_t>(srcs.size()));
        srcs.push_back(g->dn[k]);
        add_set(i);
      }
      nbr_ptr[i + 1] = static_cast<uint32_t>(nbr_row.size());
    }
  }
  st.n_rows = static_cast<uint32_t>(srcs.size());
  {  // first-hop block order: one contiguous source range per XCD when the
     // per-source work (neighbour rows) is even, else runs of 16 so heavy
     // sources (Clos spines) still spread over the XCDs (A/B: C2 0.342 vs
     // 0.350 ms, C3 0.231 vs 0.107 ms for contiguous vs runs of 16/64)
    uint64_t sum = 0;
    uint32_t mx = 0;
    for (uint32_t i = 0; i < n_src; ++i) {
      const uint32_t d = nbr_ptr[i + 1] - nbr_ptr[i];
      sum += d;
      mx = std::max(mx, d);
    }
    st.xcd_group = static_cast<uint64_t>(mx) * n_src <= 2 * sum ? 0u : 16u;
  }
  std::vector<uint32_t> staging;
  staging.reserve(2 * srcs.size() + ign_ptr.size() + ign.size() + nbr_ptr.size() + nbr_row.size() + 1);
  auto append = [&](const std::vector<uint32_t>& part) {
    const uint32_t at = static_cast<uint32_t>(staging.size());
    staging.insert(staging.end(), part.begin(), part.end());
    return at;
  };
  staging.push_back(st.n_rows);
  append(srcs);
  st.off_ign_ptr = append(ign_ptr);
  st.off_ign = append(ign);
  st.off_nbr_ptr = append(nbr_ptr);
  st.off_nbr_row = append(nbr_row);
  // multi-source batches (consecutive runs of ms_width rows): rows in
  // ascending device id of their source (Cuthill-McKee here, the cluster
  // order below), so a batch's sources are neighbours. (Measured alternatives on C2: BFS balls of 32 rows - 10.6
  // arrival levels per node and batch against 16.4 - swept in 0.92 ms
  // against 0.77; dispatching the batches middle-out changed nothing.)
  std::vector<uint32_t> order(st.n_rows);
  for (uint32_t r = 0; r < st.n_rows; ++r) order[r] = r;
  std::stable_sort(order.begin(), order.end(),
                   [&](uint32_t x, uint32_t y) { return g->ms_dev_of[srcs[x]] < g->ms_dev_of[srcs[y]]; });
  st.off_order = append(order);
  // a graph in cluster order: the BFS batches in that order too (the
  // Bellman-Ford plans keep the Cuthill-McKee batches above)
  st.off_order_ms = st.off_order;
  if (g->ms_cluster) {
    std::stable_sort(order.begin(), order.end(),
                     [&](uint32_t x, uint32_t y) { return g->msb_dev_of[srcs[x]] < g->msb_dev_of[srcs[y]]; });
    st.off_order_ms = append(order);
  }
  drain_deferred(ctx);  // a deferred phase 2 may still read the staged request
  int rc = ensure_graph_req(g, staging.size());
  if (rc) return rc;
  g->staged.key.clear();  // d_req no longer holds the request it names
  ORH_HIP(ctx, hipMemcpyAsync(g->d_req, staging.data(), staging.size() * 4, hipMemcpyHostToDevice,
                              ctx->stream));
  ORH_HIP(ctx, hipStreamSynchronize(ctx->stream));  // staging is a local
  g->staged = std::move(st);
  return ORH_OK;
}

bool env_is(const char* name, char c) {
  const char* e = getenv(name);
  return e && e[0] == c;
}

int env_int(const char* name, int unset) {
  const char* e = getenv(name);
  return e ? atoi(e) : unset;
}

// The environment knobs of orh_spf_run, all read by spf_knobs (the planners
// and launchers of the kernel units read theirs through LaunchKnobs,
// kernels/spf_launch.h). The first group is read
// once, at the first sweep of the process; the second at every sweep, because
// tests flip those in-process. ORH_MS_DEFER_PRIO alone is read elsewhere: once
// per context, when ensure_stream2 creates the second stream.
struct SpfKnobs {
  // ---- read once per process
  // ORH_WMS=0: no kWms plan (A/B)
  bool wms;
  // ORH_WMS_MIN (256): the fewest requested sources that take kWms or
  // kWmsSliced; below, the fused per-source search, which needs no neighbour
  // rows, is the better plan
  uint32_t wms_min;
  // ORH_LDS_NH=0: no kLdsNh plan, the two-phase LDS plan instead (A/B)
  bool lds_nh;
  // ORH_LDS_NH_MIN (32): fewer sources without ignore sets keep the two-phase
  // LDS plan: a lone search pays the fused kernel's per-bucket barriers with
  // nothing beside it (C2's buildRouteDb after a metric change: spf(me)
  // 1.15 ms fused against ~0.6 two-phase, profiles/r06/e_bench_phases.json)
  uint32_t lds_nh_min;
  // ORH_LDS_NH_BLOCK=64..1024 in steps of 64: threads per kLdsNh workgroup
  // instead of the choice by source count (0)
  uint32_t lds_nh_block;
  // ORH_LDS_NH_DELTA_PCT (200): bucket width of the LDS searches (kLdsNh,
  // kWms) in % of the mean live metric. Their relaxations cost LDS latency,
  // not a global atomic, so wider buckets (fewer bucket barriers) pay: C2w
  // sweep 45.5 / 30.8 / 28.9 / 29.0 / 31.4 ms at 25 / 100 / 200 / 400 / 800
  // (profiles/r06/b_c2w_delta_block.txt)
  uint32_t lds_nh_delta_pct;
  // ORH_MS_DEFER=1: an ORH_SPF_DEFER_HOPS sweep's phase 2 goes to stream2, its
  // level bytes in half p2_half of two. Off by default: the 32-sweep C2 step
  // measured 23.1-23.2 ms deferred against 23.05 (2 lanes; 36.2 ms at 1
  // lane), i.e. the GPU is already busy while a sweep's phase 2 runs - the
  // searches and the phase-2 streams share the CUs, so starting the next
  // search earlier only reorders the same work (profiles/r06/n_defer_ab.txt)
  bool ms_defer;
  // ---- read on every run
  // ORH_BFS_NH_MAX (one per CU): the most sources that take kBfsNh; 0: off
  uint32_t bfs_nh_max;
  // ORH_WMS_SLICED=0: no kWmsSliced plan (A/B)
  bool wms_sliced;
  // ORH_WMS_SLICED_ALL=1: kWmsSliced also for sources of <= 32 neighbours
  // (A/B against kLdsNh)
  bool wms_sliced_all;
  // ORH_WMS_SLICED_BLOCK=256|512|1024: threads per kWmsSliced batch instead of
  // the layout's choice (0) (A/B)
  uint32_t wms_sliced_block;
  // ORH_WMS_WIDE=0: no kWmsWide plan (A/B): sweeps whose metrics pass 15 bits
  // keep the per-source plans
  bool wms_wide;
  // ORH_WMS_WIDE_REDO=0: the rows kWms / kWmsSliced flag are redone per source
  // instead of in wide batches (A/B)
  bool wms_wide_redo;
  // ORH_MS_DIRECT=0: the rows of a host-order multi-source BFS through ms_lvl
  // and ms_finalize instead of out of the search kernel (A/B)
  bool ms_direct;
  // ORH_WMS_SKIP=1: kWms's activity skip over the in-links' reach in layout
  // ids. Its per-slice bitmap test costs more than the slices it skips once
  // a round sweeps each band both ways: C2w distances 5.07 ms with it,
  // 3.58 ms without (profiles/r06/v_wms_skip_ab.txt)
  bool wms_skip;
  // ORH_WMS_BAND=0: kWms over interleaved chunks, one sweep per round,
  // instead of the band schedule (A/B)
  bool wms_band;
  // ORH_HOP_DIST=0: the distance rows of a finalize sweep from
  // ms_finalize_kernel instead of the first-hop pass (A/B)
  bool hop_dist;
};

SpfKnobs spf_knobs(const orh_ctx* ctx) {
  static const SpfKnobs once = [] {
    SpfKnobs k{};
    k.wms = !env_is("ORH_WMS", '0');
    k.wms_min = static_cast<uint32_t>(env_int("ORH_WMS_MIN", 256));
    k.lds_nh = !env_is("ORH_LDS_NH", '0');
    k.lds_nh_min = static_cast<uint32_t>(env_int("ORH_LDS_NH_MIN", 32));
    const int b = env_int("ORH_LDS_NH_BLOCK", 0);
    k.lds_nh_block = (b >= 64 && b <= 1024 && b % 64 == 0) ? static_cast<uint32_t>(b) : 0u;
    const int pct = env_int("ORH_LDS_NH_DELTA_PCT", 200);
    k.lds_nh_delta_pct = pct > 0 ? static_cast<uint32_t>(pct) : 200u;
    k.ms_defer = env_is("ORH_MS_DEFER", '1');
    return k;
  }();
  SpfKnobs k = once;
  k.bfs_nh_max = static_cast<uint32_t>(env_int("ORH_BFS_NH_MAX", static_cast<int>(ctx->n_cu)));
  k.wms_sliced = !env_is("ORH_WMS_SLICED", '0');
  k.wms_sliced_all = env_is("ORH_WMS_SLICED_ALL", '1');
  const int b = env_int("ORH_WMS_SLICED_BLOCK", 0);
  k.wms_sliced_block = (b == 256 || b == 512 || b == 1024) ? static_cast<uint32_t>(b) : 0u;
  k.wms_wide = !env_is("ORH_WMS_WIDE", '0');
  k.wms_wide_redo = !env_is("ORH_WMS_WIDE_REDO", '0');
  k.ms_direct = !env_is("ORH_MS_DIRECT", '0');
  k.wms_skip = env_is("ORH_WMS_SKIP", '1');
  k.wms_band = !env_is("ORH_WMS_BAND", '0');
  k.hop_dist = !env_is("ORH_HOP_DIST", '0');
  return k;
}

// what phase 1 launches
struct SweepPlan {
  orh::SpfPlan run;    // the search
  uint32_t n_rows;     // rows it searches: the staged ones, or one per source when the first hops are fused
  bool wms, wsl;       // kWms; kWmsSliced (whose flagged rows the base plan's search redoes)
  bool wide;           // kWmsWide
  uint32_t wide_redo;  // kWms / kWmsSliced: sources per wide batch that redoes the flagged rows (0: per source)
  bool lds_nh_packed;  // kLdsNh with u32 labels first
  bool fused;          // the search writes the first hops too: no phase 2
  size_t label_words;  // d_labels entries to reserve (0: none)
  uint32_t wsl_block;  // threads per kWmsSliced batch
};

// few rows: wide workgroups (a big frontier phase is split over more threads;
// the rows do not fill the CUs anyway); many: narrow ones, several per CU
uint32_t block_by_sources(const orh_ctx* ctx, uint32_t n_src) {
  return n_src <= ctx->n_cu ? 1024u : n_src <= 2 * ctx->n_cu ? 512u : 256u;
}

// The plan of a sweep from the base plan (plan_spf) of its graph. The rules
// in their order of precedence (a base plan is a BFS, a two-phase LDS or an
// HBM plan, so rules of different bases never meet):
//   kBfsNh      BFS base, at most bfs_nh_max sources
//   kWms        many sources on a graph whose in-links fit 8 slots per node
//   kWmsSliced  the same sweep where kWms declined
//   kWmsWide    the same sweep where those two declined for a metric past 15 bits alone
//   kLdsNh      general metrics otherwise, sources of at most 32 neighbours
//   kGlobalNh   HBM base
int choose_plan(orh_graph* g, const orh::SpfPlan& base, const SweepFacts& f, const SpfKnobs& k,
                SweepPlan* out) {
  using V = orh::SpfVariant;
  const orh_ctx* ctx = g->ctx;
  const uint32_t N = g->n_nodes;
  const bool automatic = ctx->spf_mode == orh::SpfMode::kAuto;
  SweepPlan p{};
  p.run = base;
  p.n_rows = f.n_rows;
  orh::ms_set_width(p.run, N, f.n_rows, ctx->n_cu, ctx->lds_limit,
                    base.variant == V::kMsBfs && !device_busy_elsewhere(ctx));
  // uniform metric, few sources: one fused BFS + first-hop workgroup per
  // source instead of searching every neighbour row too
  const bool bfs_base = base.variant == V::kMsBfs || base.variant == V::kBfs8 ||
                        base.variant == V::kBfs16 || base.variant == V::kBfs32;
  uint32_t blk = 0, jj = 0;
  size_t lds = 0;
  if (bfs_base && automatic && f.n_src <= k.bfs_nh_max &&
      orh::bfs_nh_shape(N, f.words, ctx->lds_limit, &blk, &jj, &lds)) {
    p.run.variant = V::kBfsNh;
    p.run.block = blk;
    p.run.lds_bytes = lds;
    p.n_rows = f.n_src;
  }
  // the three plans for general metrics whose labels fit LDS start from the
  // two-phase LDS plan; orh_set_spf_mode(1) (per-source) keeps that one
  const bool weighted = automatic && !f.uniform && (base.variant == V::kDist16 || base.variant == V::kDist32);
  const bool lds_nh_fits = orh::lds_nh_bytes(N, false) <= ctx->lds_limit;
  // many sources: multi-source Bellman-Ford batches in LDS, then the first
  // hops over the u32 rows (phase 2)
  const bool many = weighted && !f.has_ign && f.n_src >= k.wms_min && orh::wms_lds_bytes(N) <= ctx->lds_limit;
  // u32 labels: sources per wide batch that fit LDS (0: none); big: some live
  // metric is past the 15 bits of a u16 plan's slot word; may_flag: a u16
  // label can pass 0xFFFE - max metric, so a u16 sweep may flag rows
  const uint32_t wide_s = many ? orh::wms_wide_sources(N, ctx->lds_limit) : 0u;
  const bool big = g->max_metric > 0x7FFFu;
  const bool may_flag = g->sum_max_metric / 2 + 2 * static_cast<uint64_t>(g->max_metric) > 0xFFFEull;
  const bool redo_wide = k.wms_wide_redo && wide_s && !big && may_flag;
  bool wms_shape = false;  // kWms's graph but for the metric range: every degree <= 8
  if (many && k.wms && lds_nh_fits) {  // spf_wms_kernel; flagged rows redone by the u64 LDS search
    int rc = sync_wms_layout(g);
    if (rc) return rc;
    p.wms = g->wms_ok;
    wms_shape = g->wms_maxdeg <= 8;
  }
  // a graph kWms declined, with sources of more than 32 distinct neighbours
  // (where kLdsNh does not apply and the sweep would run the two-phase plan):
  // spf_wms_sliced_kernel, flagged rows redone by that plan's own search
  const bool wsl_shape = many && !p.wms && k.wms_sliced && base.lds_bytes <= ctx->lds_limit &&
                         (f.max_nbr > 32 || k.wms_sliced_all);
  const bool wide_rule = many && !p.wms && k.wms_wide && wide_s && big && (wms_shape || wsl_shape);
  if (wsl_shape) {
    int rc = sync_wms_sliced_layout(g, redo_wide || wide_rule);
    if (rc) return rc;
    p.wsl = g->wsl_ok;
  }
  // a sweep the two u16 plans declined for their metric range alone:
  // spf_wms_wide_kernel, u32 labels and full metrics, every row final
  if (wide_rule && !p.wsl) {
    int rc = sync_wms_sliced_layout(g, true);
    if (rc) return rc;
    p.wide = g->wsl_wide && g->wsl_maxw > 0x7FFFu;
  }
  // the rows a u16 sweep flags: redone in wide batches where the graph has
  // its wide layout, else per source
  if ((p.wms || p.wsl) && redo_wide) {
    int rc = sync_wms_sliced_layout(g, true);
    if (rc) return rc;
    if (g->wsl_wide) p.wide_redo = wide_s;
  }
  if (p.wide) {
    p.run.variant = V::kWmsWide;
    p.wsl_block = k.wms_sliced_block ? k.wms_sliced_block : g->wsl_block;
  } else if (p.wms || p.wsl) {
    p.run.variant = p.wms ? V::kWms : V::kWmsSliced;
    p.label_words = (static_cast<size_t>(p.n_rows) + 2) / 2 + 1;  // the overflow row list
    if (p.wsl || p.wide_redo) p.wsl_block = k.wms_sliced_block ? k.wms_sliced_block : g->wsl_block;
  } else if (weighted && k.lds_nh && (f.has_ign || f.n_src >= k.lds_nh_min) && f.max_nbr <= 32 && lds_nh_fits) {
    // one search per source with the first hops fused (spf_lds_nh_kernel)
    // instead of the two-phase LDS kernels, which also search every neighbour
    // row and then stream 1 + deg rows per source
    p.run.variant = V::kLdsNh;
    p.lds_nh_packed = f.max_nbr <= 16;
    p.n_rows = f.n_src;
    p.run.block = k.lds_nh_block ? k.lds_nh_block : block_by_sources(ctx, f.n_src);
    p.label_words = (static_cast<size_t>(f.n_src) + 2) / 2 + 1;  // the overflow row list
  }
  // HBM kernel: fuse the first hops into the search (one row per source)
  // when the two-phase scheme would need extra neighbour rows (or the HBM
  // kernel is forced)
  if (base.variant == V::kGlobal && f.max_nbr <= 32 && ctx->spf_mode != orh::SpfMode::kGlobalTwoPhase &&
      (ctx->spf_mode == orh::SpfMode::kGlobal || p.n_rows > f.n_src)) {
    p.run.variant = V::kGlobalNh;
    p.n_rows = f.n_src;
    p.run.block = block_by_sources(ctx, f.n_src);
    p.label_words = static_cast<size_t>(f.n_src) * N;
  }
  p.fused = p.run.variant == V::kGlobalNh || p.run.variant == V::kBfsNh || p.run.variant == V::kLdsNh;
  *out = p;
  return ORH_OK;
}

// SpfArgs of the search. A multi-source BFS gets its buffers here (layout,
// level bytes and arrival log, level rows); *defer: its phase 2 goes to stream2
int fill_spf_args(orh_graph* g, const SweepFacts& f, const SweepPlan& sp, const SpfKnobs& k, uint32_t* d_dist,
                  uint32_t* d_nh, orh::SpfArgs* out, bool* defer) {
  using V = orh::SpfVariant;
  orh_ctx* ctx = g->ctx;
  const uint32_t N = g->n_nodes;
  const StagedRequest& st = g->staged;
  orh::SpfArgs a{};
  a.n_nodes = N;
  a.n_out = f.n_src;
  a.recs = g->d_recs;
  a.link = g->d_link;
  *defer = false;
  if (sp.run.variant == V::kMsBfs) {
    int rc = sync_ms_layout(g);
    if (rc) return rc;
    // the interval skip: opt-in for every sweep (ORH_MS_SKIP=1) or for the
    // latency plan alone (ORH_MS_LATENCY=2)
    a.ms_bw = g->ms_bw ? g->ms_bw : sp.run.ms_skip ? g->ms_bw_layout : 0u;
    // the adjacency skip, unless the interval skip is on (the two never run
    // together) or the plan is the latency or the lone-sweep one, where it
    // measured slower (ms_set_width); ORH_MS_ADJ=1 takes it even there
    a.ms_adj = !a.ms_bw && g->ms_adj_on && (!sp.run.ms_own_cu || g->ms_adj_forced) ? g->d_ms_adj : nullptr;
    a.ms_width = sp.run.ms_width;
    // host-order layout, u16 / u32 masks: the rows come out of the search
    // kernel itself
    a.ms_direct = k.ms_direct && g->ms_identity && sp.run.mask_bytes <= 4 ? 1u : 0u;
    const size_t scratch =
        a.ms_direct ? 0 : (orh::ms_scratch_bytes(sp.run, N, sp.n_rows) + 255) & ~size_t{255};
    const size_t log_bytes = orh::ms_log_bytes(sp.run, sp.n_rows);
    *defer = k.ms_defer && (f.flags & ORH_SPF_DEFER_HOPS) && !a.ms_direct && sp.n_rows == f.n_src;
    const size_t halves = *defer ? 2 : 1;
    rc = ensure_ms_lvl(ctx, halves * scratch + log_bytes);
    if (rc) return rc;
    a.ms_log = log_bytes ? reinterpret_cast<uint64_t*>(ctx->d_ms_lvl + halves * scratch) : nullptr;
    a.recs = g->d_ms_recs;
    a.dev_of = g->ms_cluster ? g->d_msb_dev_of : g->d_ms_dev_of;
    a.host_of = g->ms_cluster ? g->d_msb_host_of : g->d_ms_host_of;
    a.ms_lvl = ctx->d_ms_lvl + (*defer ? ctx->p2_half * scratch : 0);
    a.lvl_pitch = (N + 15u) & ~15u;
    rc = ensure_lvl_rows(ctx, static_cast<size_t>(sp.n_rows) * a.lvl_pitch);
    if (rc) return rc;
    a.lvl_rows = ctx->d_lvl_rows;
    // the lean first-hop kernel's state: a deferred phase 2 reads its half
    // while the next sweep's search writes the other
    const size_t aux = orh::hop_aux_bytes(sp.n_rows);
    rc = ensure_hop_aux(ctx, 2 * aux);
    if (rc) return rc;
    uint8_t* half = ctx->d_hop_aux + (*defer ? ctx->p2_half * aux : 0);
    a.hop_redo_count = reinterpret_cast<uint32_t*>(half);
    a.row_deep = half + orh::hop_aux_deep_off(sp.n_rows);
  }
  a.order = g->d_req + (sp.run.variant == V::kMsBfs ? st.off_order_ms : st.off_order);
  a.srcs = g->d_req + 1;
  a.ignore_ptr = f.has_ign ? g->d_req + st.off_ign_ptr : nullptr;
  a.ignore_links = f.has_ign ? g->d_req + st.off_ign : nullptr;
  a.use_link_metric = f.use_link_metric;
  a.w0 = f.w0;
  // near/far width of the HBM kernel: the mean live metric (one BFS level
  // when metrics are uniform); bucket width of the LDS searches
  const uint32_t pct = sp.run.variant == V::kLdsNh || sp.wms ? k.lds_nh_delta_pct : ctx->delta_pct;
  a.delta = f.uniform ? f.w0
                      : std::max<uint32_t>(1u, static_cast<uint32_t>(static_cast<uint64_t>(g->mean_out) * pct / 100u));
  a.out_dist = d_dist;
  a.scratch = ctx->d_scratch;
  a.labels = ctx->d_labels;
  a.out_nh = d_nh;
  a.words = f.words;
  a.rank_out = g->d_rank_out;
  if (sp.run.variant == V::kLdsNh || sp.wms || sp.wsl) a.ovf_rows = reinterpret_cast<uint32_t*>(ctx->d_labels);
  if (sp.wsl) {
    a.dev_of = g->d_ms_dev_of;
    a.wms_limit = 0xFFFEu - g->wsl_maxw;
    a.wsl_slots = g->d_wsl;
    a.wsl_off = g->d_wsl + g->wsl_off_at;
    a.wsl_ovl = g->wsl_ovl ? 1u : 0u;
    a.wsl_band = g->d_wsl + g->wsl_band_at + (sp.wsl_block == 256 ? 0u : sp.wsl_block == 512 ? 5u : 14u);
  }
  if (sp.wide || sp.wide_redo) {  // the wide kernel's slots in the sliced geometry
    a.dev_of = g->d_ms_dev_of;
    a.wsw_slots = reinterpret_cast<const uint2*>(g->d_wsl + g->wsl_wide_at);
    a.wsl_off = g->d_wsl + g->wsl_off_at;
    a.wsl_ovl = g->wsl_ovl ? 1u : 0u;
    a.wsl_band = g->d_wsl + g->wsl_band_at + (sp.wsl_block == 256 ? 0u : sp.wsl_block == 512 ? 5u : 14u);
  }
  if (sp.wms) {
    a.dev_of = g->d_ms_dev_of;
    a.wms_slots = g->d_wms;
    a.wms_limit = 0xFFFEu - g->wms_maxw;
    a.ms_bw = k.wms_skip ? g->wms_bw : 0u;
    a.recs_k = g->ell_k;
    a.wms_band = k.wms_band ? 1u : 0u;
  }
  *out = a;
  return ORH_OK;
}

// HopArgs of the first-hop phase over the rows of search `a`
orh::HopArgs fill_hop_args(const orh_graph* g, const SweepFacts& f, const SweepPlan& sp, const orh::SpfArgs& a) {
  const orh_ctx* ctx = g->ctx;
  const StagedRequest& st = g->staged;
  orh::HopArgs h{};
  h.n_nodes = g->n_nodes;
  h.n_out = f.n_src;
  h.words = f.words;
  h.ell_k = g->ell_k;
  h.recs = g->d_recs;
  h.link = g->d_link;
  h.rank_out = g->d_rank_out;
  h.overloaded = g->d_ovl;
  h.srcs = a.srcs;
  h.ignore_ptr = a.ignore_ptr;
  h.ignore_links = a.ignore_links;
  h.use_link_metric = f.use_link_metric;
  h.nbr_ptr = g->d_req + st.off_nbr_ptr;
  h.xcd_group = st.xcd_group;
  h.nbr_row = g->d_req + st.off_nbr_row;
  h.dist = a.out_dist;
  h.scratch = ctx->d_scratch;
  h.out_nh = a.out_nh;
  h.lvl_rows = sp.run.variant == orh::SpfVariant::kMsBfs ? a.lvl_rows : nullptr;
  h.lvl_pitch = a.lvl_pitch;
  h.w0 = f.w0;
  if (h.lvl_rows && a.row_deep) {
    h.row_deep = a.row_deep;
    h.redo_count = a.hop_redo_count;
    h.redo_list = a.hop_redo_count + orh::hop_aux_list_off() / 4;
  }
  return h;
}

// Orders the context stream behind the deferred second phases this sweep's
// buffers are shared with, then starts the sweep's clock
int begin_sweep(orh_ctx* ctx, bool defer) {
  if (!defer) {
    join_deferred(ctx);  // earlier deferred sweeps share the scratch
  } else if (ctx->p2_pending[ctx->p2_half]) {
    // the search rewrites the half the phase 2 two sweeps back reads
    ORH_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_p2[ctx->p2_half], 0));
    ctx->p2_pending[ctx->p2_half] = false;
  }
  ORH_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  return ORH_OK;
}

std::string plan_text(const SweepPlan& sp, bool shape) {
  std::string m = "variant " + std::to_string(int(sp.run.variant)) + " rows " + std::to_string(sp.n_rows);
  if (shape)
    m += " lds " + std::to_string(sp.run.lds_bytes) + " block " + std::to_string(sp.run.block) + " j " +
         std::to_string(sp.run.ms_j);
  return m;
}

// the search; kWmsSliced redoes its flagged rows with the base plan's search,
// or, like kWms, in wide batches (sp.wide_redo)
int launch_phase1(orh_graph* g, const orh::SpfPlan& base, const SweepPlan& sp, const orh::SpfArgs& a) {
  using V = orh::SpfVariant;
  orh_ctx* ctx = g->ctx;
  const hipError_t pre = hipGetLastError();
  if (pre != hipSuccess)
    return hip_fail(ctx, pre, ("pending HIP error before spf launch (" + plan_text(sp, false) + ")").c_str());
  const hipError_t e =
      sp.run.variant == V::kLdsNh
          ? orh::launch_spf_lds_nh(a, sp.n_rows, g->ell_k, sp.lds_nh_packed, sp.run.block, ctx->stream)
      : sp.wide ? orh::launch_spf_wms_wide(a, sp.n_rows, sp.wsl_block, ctx->lds_limit, ctx->stream)
      : sp.wms  ? orh::launch_spf_wms(a, sp.n_rows, g->wms_k, sp.wide_redo ? sp.wsl_block : 0u, ctx->lds_limit,
                                      ctx->stream)
      : sp.wsl  ? orh::launch_spf_wms_sliced(base, a, sp.n_rows, sp.wsl_block, sp.wide_redo != 0, ctx->lds_limit,
                                             ctx->stream)
               : orh::launch_spf(sp.run, a, sp.n_rows, ctx->stream);
  if (e != hipSuccess) return hip_fail(ctx, e, ("spf kernel launch " + plan_text(sp, true)).c_str());
  return ORH_OK;
}

#ifdef ORH_DIAG_STAMPS
constexpr size_t kDiagWords = 16 + 4 * 4096;
uint64_t* d_diag = nullptr;

void diag_begin(orh_ctx* ctx, orh::SpfArgs* a) {
  if (!d_diag) hipMalloc(&d_diag, kDiagWords * 8);
  hipMemsetAsync(d_diag, 0, kDiagWords * 8, ctx->stream);
  a->diag = d_diag;
}

void diag_report(orh_ctx* ctx) {
  std::vector<uint64_t> h(kDiagWords);
  hipMemcpyAsync(h.data(), d_diag, kDiagWords * 8, hipMemcpyDeviceToHost, ctx->stream);
  hipStreamSynchronize(ctx->stream);
  if (h[4])
    fprintf(stderr, "diag: waves %llu avg cycles %.0f barrier %.0f groups/wave %.1f levels %.1f max cycles %llu max levels %llu read %.0f proc %.0f\n",
            (unsigned long long)h[4], double(h[0]) / h[4], double(h[1]) / h[4],
            double(h[2]) / h[4], double(h[3]) / h[4], (unsigned long long)h[5], (unsigned long long)h[6], double(h[7]) / h[4], double(h[8]) / h[4]);
  // per workgroup: duration, and how many workgroups shared its CU at any time
  struct Wg { uint64_t t0, t1, cu; uint32_t lv, b; };
  std::vector<Wg> wg;
  for (uint32_t b = 0; b < 4096; ++b) {
    const uint64_t* w = &h[16 + 4 * b];
    if (!w[1]) continue;
    const uint64_t hw = w[2];
    // HW_ID: CU_ID [11:8], SH_ID [12], SE_ID [15:13]; XCC_ID in the high word
    const uint64_t cu = ((hw >> 8) & 0xF) | (((hw >> 12) & 1) << 4) | (((hw >> 13) & 7) << 5) | ((hw >> 32) & 0xF) << 8;
    wg.push_back({w[0], w[1], cu, static_cast<uint32_t>(w[3]), b});
  }
  if (wg.empty()) return;
  uint64_t t_min = ~0ull, t_max = 0;
  for (auto& x : wg) { t_min = std::min(t_min, x.t0); t_max = std::max(t_max, x.t1); }
  std::vector<uint64_t> dur_solo, dur_shared;
  uint64_t worst = 0; uint32_t worst_b = 0, worst_lv = 0; int worst_share = 0;
  for (auto& x : wg) {
    int share = 0;
    for (auto& y : wg) if (&y != &x && y.cu == x.cu && y.t0 < x.t1 && x.t0 < y.t1) ++share;
    (share ? dur_shared : dur_solo).push_back(x.t1 - x.t0);
    if (x.t1 - x.t0 > worst) { worst = x.t1 - x.t0; worst_b = x.b; worst_lv = x.lv; worst_share = share; }
  }
  auto med = [](std::vector<uint64_t> v) { if (v.empty()) return 0.0; std::sort(v.begin(), v.end()); return double(v[v.size() / 2]); };
  auto mx = [](const std::vector<uint64_t>& v) { uint64_t m = 0; for (auto x : v) m = std::max(m, x); return double(m); };
  uint64_t last_start = 0;
  for (auto& x : wg) last_start = std::max(last_start, x.t0 - t_min);
  fprintf(stderr, "diag-wg: %zu wgs span %llu; solo %zu med %.0f max %.0f; shared %zu med %.0f max %.0f; worst wg %u (%u levels, %d partners) %llu; last start %llu\n",
          wg.size(), (unsigned long long)(t_max - t_min), dur_solo.size(), med(dur_solo), mx(dur_solo),
          dur_shared.size(), med(dur_shared), mx(dur_shared), worst_b, worst_lv, worst_share,
          (unsigned long long)worst, (unsigned long long)last_start);
}
#endif

// what orh_last_spf_info reports of the search (phase 2 adds its own shape)
orh_spf_info search_info(const orh_graph* g, const SweepPlan& sp, const orh::SpfArgs& a) {
  const bool ms = sp.run.variant == orh::SpfVariant::kMsBfs;
  orh_spf_info info{};
  info.variant = static_cast<int32_t>(sp.run.variant);
  info.rows = sp.n_rows;
  info.mask_bits = ms ? sp.run.mask_bytes * 8 : 0;
  info.batch_sources = ms ? sp.run.ms_width : 0;
  info.ms_threads = ms ? sp.run.block : 0;
  info.ms_skip = ms && a.ms_bw ? 1u : 0u;
  info.ms_adj = ms && a.ms_adj ? 1u : 0u;
  info.ms_direct = ms ? a.ms_direct : (sp.wms || sp.wsl || sp.wide) && g->ms_identity ? 1u : 0u;
  if (sp.wsl) {
    info.batch_sources = orh::wms_sources(g->n_nodes, g->ctx->lds_limit);
    info.ms_threads = sp.wsl_block;
    info.wsl_links = g->wsl_real;
    info.wsl_slots = g->wsl_padded;
  }
  if (sp.wide) {
    info.batch_sources = orh::wms_wide_sources(g->n_nodes, g->ctx->lds_limit);
    info.ms_threads = sp.wsl_block;
    info.wsl_links = g->wsl_real;
    info.wsl_slots = g->wsl_padded;
  }
  info.wide_redo = sp.wide_redo;
  return info;
}

// the second stream of deferred second phases and its events, at first use
int ensure_stream2(orh_ctx* ctx) {
  if (ctx->stream2) return ORH_OK;
  // ORH_MS_DEFER_PRIO (A/B): stream2's priority, -1 high / 1 low / 0 (default) normal
  int lo = 0, hi = 0;
  const int want = env_int("ORH_MS_DEFER_PRIO", 0);
  if (want != 0 && hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess) {
    ORH_HIP(ctx, hipStreamCreateWithPriority(&ctx->stream2, hipStreamNonBlocking, want < 0 ? hi : lo));
  } else {
    ORH_HIP(ctx, hipStreamCreateWithFlags(&ctx->stream2, hipStreamNonBlocking));
  }
  ORH_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_ms2, hipEventDisableTiming));
  ORH_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_p2[0], hipEventDisableTiming));
  ORH_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_p2[1], hipEventDisableTiming));
  return ORH_OK;
}

// Phase 2 of a sweep whose search leaves the first hops to it: the first-hop
// pass, after ms_finalize_kernel when a multi-source BFS left level bytes.
// *end: the stream the sweep ends on (stream2 when deferred)
int launch_phase2(orh_graph* g, const SweepPlan& sp, const SpfKnobs& k, const orh::SpfArgs& a, orh::HopArgs h,
                  uint32_t max_nbr, bool defer, orh_spf_info* info, hipStream_t* end) {
  orh_ctx* ctx = g->ctx;
  *end = ctx->stream;
  ORH_HIP(ctx, hipEventRecord(ctx->evm, ctx->stream));
  if (sp.fused) return ORH_OK;
  if (sp.run.variant == orh::SpfVariant::kMsBfs) {
#ifdef ORH_EXP_MSBFS_ONLY  // timing experiment only (tools/diag_build.sh): no phase 2
    return ORH_OK;
#endif
    if (defer) {
      // phase 2 on stream2 after this search; the context stream is free for
      // the next sweep's search
      int rc = ensure_stream2(ctx);
      if (rc) return rc;
      ORH_HIP(ctx, hipEventRecord(ctx->ev_ms2, ctx->stream));
      ORH_HIP(ctx, hipStreamWaitEvent(ctx->stream2, ctx->ev_ms2, 0));
      *end = ctx->stream2;
    }
    // The u32 distance rows of a finalize sweep (u16 / u32 masks): written by
    // the first-hop pass from the level bytes each of its threads loads
    // anyway, so ms_finalize_kernel writes the u8 level rows alone. That pass
    // covers every output row 0..n_src-1 (one source each; neighbour-only rows
    // r >= n_src have no distance row either way), and nothing reads d_dist
    // between the two launches: on the deferred path both go to stream2 and
    // ev_p2, which every reader of the rows joins, is recorded after the
    // first-hop kernel
    const bool hop_dist = k.hop_dist && !a.ms_direct && sp.run.mask_bytes <= 4;
    h.write_dist = hop_dist ? 1u : 0u;
    info->hop_dist = h.write_dist;
    if (!a.ms_direct) {
      const hipError_t e = orh::launch_ms_finalize(sp.run, a, sp.n_rows, *end, !hop_dist);
      if (e != hipSuccess) return hip_fail(ctx, e, "multi-source finalize launch");
    }
  }
  const hipError_t e = orh::launch_first_hop(h, max_nbr, *end, &info->hop_nodes, &info->hop_split, &info->hop_lean);
  if (e != hipSuccess) return hip_fail(ctx, e, "first-hop kernel launch");
  info->hop_redo = info->hop_lean ? h.n_out : 0u;
  if (defer) {
    ORH_HIP(ctx, hipEventRecord(ctx->ev_p2[ctx->p2_half], *end));
    ctx->p2_pending[ctx->p2_half] = true;
    ctx->p2_half ^= 1u;
  }
  return ORH_OK;
}

// the sweep's end on stream `end`; last_kernel_ms is resolved lazily by
// orh_spf_batch / orh_sync users
int finish_sweep(orh_ctx* ctx, const orh_spf_info& info, uint32_t n_src, hipStream_t end) {
  ctx->last_info = info;
  ORH_HIP(ctx, hipEventRecord(ctx->ev1, end));
  ctx->counters.spf_runs += n_src;
  ctx->counters.spf_launches += 1;
  ctx->counters.last_kernel_ms = -1.0;
  return ORH_OK;
}

// orh_spf_batch's device rows, grown to n_u32 words
bool ensure_batch(orh_ctx* ctx, size_t n_u32) {
  return grow_device(ctx, &ctx->d_batch, &ctx->d_batch_cap, n_u32, false) == ORH_OK;
}

}  // namespace

namespace orh::api {

// The exact kernel (LinkState::runSpf's own extraction order): one wave per
// requested row, nothing shared between rows. Rows run in chunks whose heap
// state fits a bounded scratch when it is too large for LDS.
int run_exact(orh_graph* g, const orh_spf_request* req, uint32_t words, uint32_t* d_dist32, uint64_t* d_dist64,
              uint32_t* d_nh, uint32_t* d_rank) {
  orh_ctx* ctx = g->ctx;
  const uint32_t n_src = req->n_src, N = g->n_nodes;
  uint32_t max_nbr = 1;
  for (uint32_t i = 0; i < n_src; ++i) {
    if (req->h_srcs[i] >= N) return fail(ctx, ORH_E_INVALID, "exact SPF: source out of range");
    max_nbr = std::max(max_nbr, n_distinct(g, req->h_srcs[i]));
  }
  if (words < (max_nbr + 31) / 32) return fail(ctx, ORH_E_INVALID, "exact SPF: words too small");
  hipSetDevice(ctx->device);
  // staging: srcs[n_src] | ign_ptr[n_src + 1] ign[..] (ignore sets sorted for
  // the device binary search)
  const bool has_ign = req->h_ignore_ptr != nullptr;
  std::vector<uint32_t> staging(req->h_srcs, req->h_srcs + n_src);
  const size_t off_ign_ptr = staging.size();
  if (has_ign) {
    const size_t off_ign = off_ign_ptr + n_src + 1;
    staging.resize(off_ign);
    staging[off_ign_ptr] = 0;
    for (uint32_t i = 0; i < n_src; ++i) {
      std::vector<uint32_t> set(req->h_ignore_links + req->h_ignore_ptr[i],
                                req->h_ignore_links + req->h_ignore_ptr[i + 1]);
      std::sort(set.begin(), set.end());
      staging.insert(staging.end(), set.begin(), set.end());
      staging[off_ign_ptr + i + 1] = static_cast<uint32_t>(staging.size() - off_ign);
    }
  }
  int rc = ensure_req(ctx, staging.size());
  if (rc) return rc;
  ORH_HIP(ctx, hipMemcpyAsync(ctx->d_req, staging.data(), staging.size() * 4, hipMemcpyHostToDevice,
                              ctx->stream));
  ORH_HIP(ctx, hipStreamSynchronize(ctx->stream));  // staging is a local
  orh::ExactArgs a{};
  a.n_nodes = N;
  a.words = words;
  a.use_link_metric = req->use_link_metric;
  a.ell_k = g->ell_k;
  a.recs = g->d_recs;
  a.link = g->d_link;
  a.rank_out = g->d_rank_out;
  a.name_rank = g->d_name_rank;
  a.ignore_links = has_ign ? ctx->d_req + off_ign_ptr + n_src + 1 : nullptr;
  const size_t state = orh::exact_state_bytes(N, words);
  uint32_t chunk = n_src;
  if (state > ctx->lds_limit) {  // per-row global heap state, at most 1 GiB at a time
    chunk = static_cast<uint32_t>(std::max<size_t>(1, std::min<size_t>(n_src, (size_t{1} << 30) / state)));
    rc = ensure_bytes(ctx, &ctx->d_exact, &ctx->d_exact_cap, state * chunk);
    if (rc) return rc;
    a.scratch = ctx->d_exact;
    a.scratch_stride = state;
  }
  ORH_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  for (uint32_t r0 = 0; r0 < n_src; r0 += chunk) {
    const size_t base = static_cast<size_t>(r0) * N;
    a.n_rows = std::min(chunk, n_src - r0);
    a.srcs = ctx->d_req + r0;
    a.ignore_ptr = has_ign ? ctx->d_req + off_ign_ptr + r0 : nullptr;
    a.out_dist32 = d_dist32 ? d_dist32 + base : nullptr;
    a.out_dist64 = d_dist64 ? d_dist64 + base : nullptr;
    a.out_nh = d_nh + base * words;
    a.out_rank = d_rank ? d_rank + base : nullptr;
    hipError_t e = orh::launch_exact(a, ctx->lds_limit, ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "exact SPF kernel launch");
  }
  ORH_HIP(ctx, hipEventRecord(ctx->evm, ctx->stream));
  ORH_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  orh_spf_info info{};
  info.variant = static_cast<int32_t>(orh::SpfVariant::kExact);
  info.rows = n_src;
  ctx->last_info = info;
  ctx->counters.spf_runs += n_src;
  ctx->counters.spf_launches += 1;
  ctx->counters.last_kernel_ms = -1.0;
  return ORH_OK;
}

}  // namespace orh::api

extern "C" {

// One sweep: a dist row and the first-hop masks of every requested source.
// Validate; the exact kernel or the what-if repair where they apply; else the
// base plan of the graph, the staged request, the sweep's plan, the kernels'
// arguments, the search (phase 1), the first hops (phase 2), the bookkeeping.
int orh_spf_run(orh_graph* g, const orh_spf_request* req, uint32_t words, uint32_t* d_dist,
                uint32_t* d_nh) {
  if (!g || !req || (req->n_src && (!req->h_srcs || !d_dist || !d_nh)))
    return g ? fail(g->ctx, ORH_E_INVALID, "orh_spf_run: null argument") : ORH_E_INVALID;
  orh_ctx* ctx = g->ctx;
  if (req->n_src == 0) return ORH_OK;
  if (!g->d_recs || g->n_nodes == 0) return fail(ctx, ORH_E_STATE, "orh_spf_run: no graph loaded");
  const uint32_t n_src = req->n_src, N = g->n_nodes;
  uint32_t max_nbr = 1;
  for (uint32_t i = 0; i < n_src; ++i) {
    if (req->h_srcs[i] >= N) return fail(ctx, ORH_E_INVALID, "orh_spf_run: source out of range");
    max_nbr = std::max(max_nbr, n_distinct(g, req->h_srcs[i]));
  }
  if (words < (max_nbr + 31) / 32) return fail(ctx, ORH_E_INVALID, "orh_spf_run: words too small");
  // zero link metrics: the first hops depend on the extraction order among
  // equal-metric nodes, which only the exact kernel follows
  if (ctx->spf_mode == orh::SpfMode::kExact || (req->use_link_metric && g->has_zero)) {
    if (req->use_link_metric && wide_metrics(g))
      return fail(ctx, ORH_E_UNSUPPORTED,
                  "orh_spf_run: path metrics may reach 2^32 - 1 (use orh_spf_run_exact)");
    return run_exact(g, req, words, d_dist, nullptr, d_nh, nullptr);
  }
  SweepFacts f{};
  f.n_src = n_src;
  f.max_nbr = max_nbr;
  f.words = words;
  f.uniform = !req->use_link_metric || g->min_out == g->max_out;
  f.has_ign = req->h_ignore_ptr != nullptr;
  f.w0 = req->use_link_metric ? g->max_out : 1u;
  f.flags = req->flags;
  f.use_link_metric = req->use_link_metric;
  // any tentative value is at most (sum of link metrics) + max metric; BFS
  // levels at most (N - 1) * w0
  const uint64_t bound = f.uniform ? static_cast<uint64_t>(N) * f.w0
      : req->use_link_metric ? g->sum_max_metric / 2 + g->max_metric
                             : static_cast<uint64_t>(g->n_links) + 1;
  if (f.has_ign && ctx->spf_mode == orh::SpfMode::kAuto && max_nbr <= 32 && repair_eligible(g, req, words)) {
    hipSetDevice(ctx->device);
    return run_repair(g, req, d_dist, d_nh);
  }
  const orh::SpfPlan base =
      orh::plan_spf(N, f.uniform, bound, g->ell_k, ctx->lds_limit, !f.has_ign, ctx->spf_mode);
  if (base.variant == orh::SpfVariant::kUnsupported)
    return fail(ctx, ORH_E_UNSUPPORTED, "orh_spf_run: no distance kernel for this graph (N=" +
                                            std::to_string(N) + ", path bound " +
                                            std::to_string(bound) + "; orh_spf_run_exact covers it)");
  if (orh::hop_lds_bytes(max_nbr) > ctx->lds_limit)
    return fail(ctx, ORH_E_UNSUPPORTED, "orh_spf_run: too many neighbours for the first-hop phase");
  hipSetDevice(ctx->device);

  int rc = stage_request(g, req, f.has_ign);
  if (rc) return rc;
  f.n_rows = g->staged.n_rows;
  const SpfKnobs knobs = spf_knobs(ctx);
  SweepPlan sp{};
  rc = choose_plan(g, base, f, knobs, &sp);
  if (rc) return rc;
  if (sp.label_words) rc = ensure_labels(ctx, sp.label_words);
  if (rc) return rc;
  if (sp.n_rows > n_src) rc = ensure_scratch(ctx, static_cast<size_t>(sp.n_rows - n_src) * N);
  if (rc) return rc;

  orh::SpfArgs a{};
  bool defer = false;  // this sweep's phase 2 goes to stream2
  rc = fill_spf_args(g, f, sp, knobs, d_dist, d_nh, &a, &defer);
  if (rc) return rc;
  const orh::HopArgs h = fill_hop_args(g, f, sp, a);

  rc = begin_sweep(ctx, defer);
  if (rc) return rc;
#ifdef ORH_DIAG_STAMPS
  diag_begin(ctx, &a);
#endif
  rc = launch_phase1(g, base, sp, a);
  if (rc) return rc;
#ifdef ORH_DIAG_STAMPS
  diag_report(ctx);
#endif
  orh_spf_info info = search_info(g, sp, a);
  hipStream_t end = ctx->stream;
  rc = launch_phase2(g, sp, knobs, a, h, max_nbr, defer, &info, &end);
  if (rc) return rc;
  return finish_sweep(ctx, info, n_src, end);
}

int orh_spf_batch(orh_graph* g, const orh_spf_request* req, uint32_t words, uint32_t* h_dist,
                  uint32_t* h_nh) {
  if (!g || !req) return ORH_E_INVALID;
  orh_ctx* ctx = g->ctx;
  if (req->n_src == 0) return ORH_OK;
  if (!h_dist || !h_nh) return fail(ctx, ORH_E_INVALID, "orh_spf_batch: null output");
  const size_t nd = static_cast<size_t>(req->n_src) * g->n_nodes;
  hipSetDevice(ctx->device);
  if (!ensure_batch(ctx, nd * (1 + words)))
    return fail(ctx, ORH_E_NOMEM, "orh_spf_batch: device allocation failed");
  uint32_t* d_dist = ctx->d_batch;
  uint32_t* d_nh = ctx->d_batch + nd;
  int rc = orh_spf_run(g, req, words, d_dist, d_nh);
  if (rc == ORH_OK) {
    join_deferred(ctx);
    hipError_t e = hipMemcpyAsync(h_dist, d_dist, nd * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess)
      e = hipMemcpyAsync(h_nh, d_nh, nd * words * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) rc = hip_fail(ctx, e, "orh_spf_batch: copy-out");
    float ms = 0.f;
    if (rc == ORH_OK && hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1) == hipSuccess) {
      ctx->counters.last_kernel_ms = ms;
      ctx->counters.total_kernel_ms += ms;
    }
  }
  return rc;
}

int orh_spf_batch_pinned(orh_graph* g, const orh_spf_request* req, uint32_t words,
                         const uint32_t** h_dist, const uint32_t** h_nh) {
  if (!g || !req || !h_dist || !h_nh) return ORH_E_INVALID;
  orh_ctx* ctx = g->ctx;
  *h_dist = *h_nh = nullptr;
  if (req->n_src == 0) return ORH_OK;
  const size_t nd = static_cast<size_t>(req->n_src) * g->n_nodes;
  hipSetDevice(ctx->device);
  if (!ensure_batch(ctx, nd * (1 + words)))
    return fail(ctx, ORH_E_NOMEM, "orh_spf_batch_pinned: device allocation failed");
  if (nd * (1 + words) > ctx->h_pinned_cap) {
    if (ctx->h_pinned) hipHostFree(ctx->h_pinned);
    ctx->h_pinned = nullptr;
    ctx->h_pinned_cap = 0;
    if (hipHostMalloc(reinterpret_cast<void**>(&ctx->h_pinned), nd * (1 + words) * 4, hipHostMallocDefault) !=
        hipSuccess)
      return fail(ctx, ORH_E_NOMEM, "orh_spf_batch_pinned: pinned host allocation failed");
    ctx->h_pinned_cap = nd * (1 + words);
  }
  int rc = orh_spf_run(g, req, words, ctx->d_batch, ctx->d_batch + nd);
  if (rc != ORH_OK) return rc;
  join_deferred(ctx);
  hipError_t e = hipMemcpyAsync(ctx->h_pinned, ctx->d_batch, nd * (1 + words) * 4, hipMemcpyDeviceToHost,
                                ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return hip_fail(ctx, e, "orh_spf_batch_pinned: copy-out");
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1) == hipSuccess) {
    ctx->counters.last_kernel_ms = ms;
    ctx->counters.total_kernel_ms += ms;
  }
  *h_dist = ctx->h_pinned;
  *h_nh = ctx->h_pinned + nd;
  return ORH_OK;
}

int orh_spf_run_exact(orh_graph* g, const orh_spf_request* req, uint32_t words, uint64_t* d_dist,
                      uint32_t* d_nh, uint32_t* d_rank) {
  if (!g || !req || (req->n_src && (!req->h_srcs || !d_dist || !d_nh)))
    return g ? fail(g->ctx, ORH_E_INVALID, "orh_spf_run_exact: null argument") : ORH_E_INVALID;
  if (req->n_src == 0) return ORH_OK;
  join_deferred(g->ctx);
  if (!g->d_recs || g->n_nodes == 0)
    return fail(g->ctx, ORH_E_STATE, "orh_spf_run_exact: no graph loaded");
  return run_exact(g, req, words, nullptr, d_dist, d_nh, d_rank);
}

int orh_spf_batch_exact(orh_graph* g, const orh_spf_request* req, uint32_t words, uint64_t* h_dist,
                        uint32_t* h_nh, uint32_t* h_rank) {
  if (!g || !req) return ORH_E_INVALID;
  orh_ctx* ctx = g->ctx;
  join_deferred(ctx);
  if (req->n_src == 0) return ORH_OK;
  if (!h_dist || !h_nh) return fail(ctx, ORH_E_INVALID, "orh_spf_batch_exact: null output");
  const size_t nd = static_cast<size_t>(req->n_src) * g->n_nodes;
  const size_t bytes = nd * 8 + nd * words * 4 + nd * 4;
  hipSetDevice(ctx->device);
  int rc = ensure_bytes(ctx, &ctx->d_batch_x, &ctx->d_batch_x_cap, bytes);
  if (rc) return fail(ctx, ORH_E_NOMEM, "orh_spf_batch_exact: device allocation failed");
  uint64_t* d_dist = reinterpret_cast<uint64_t*>(ctx->d_batch_x);
  uint32_t* d_nh = reinterpret_cast<uint32_t*>(d_dist + nd);
  uint32_t* d_rank = d_nh + nd * words;
  rc = orh_spf_run_exact(g, req, words, d_dist, d_nh, h_rank ? d_rank : nullptr);
  if (rc == ORH_OK) {
    hipError_t e = hipMemcpyAsync(h_dist, d_dist, nd * 8, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess)
      e = hipMemcpyAsync(h_nh, d_nh, nd * words * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && h_rank)
      e = hipMemcpyAsync(h_rank, d_rank, nd * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) rc = hip_fail(ctx, e, "orh_spf_batch_exact: copy-out");
    float ms = 0.f;
    if (rc == ORH_OK && hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1) == hipSuccess) {
      ctx->counters.last_kernel_ms = ms;
      ctx->counters.total_kernel_ms += ms;
    }
  }
  return rc;
}

}  // extern "C"
