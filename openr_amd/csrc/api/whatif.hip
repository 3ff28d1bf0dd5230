// What-if jobs: repair caps and eligibility, orh_whatif, a run's resolve, stage,
// provision and launch steps, the summaries and orh_whatif_*.
#include "orh_internal.h"
#include "../kernels/whatif_kernels.h"

using namespace orh::api;

namespace orh::api {

// ---- what-if repair (whatif_kernels.hip) ----------------------------------
// per-record reverse records and per-link CSR entries of the current structure
int ensure_rev(orh_graph* g) {
  if (g->d_rev && g->rev_gen == g->gen) return ORH_OK;
  orh_ctx* ctx = g->ctx;
  const uint32_t L = g->n_links;
  g->link_ent.assign(2 * static_cast<size_t>(L), ~0u);
  for (uint32_t e = 0; e < g->n_edges; ++e) {
    if (g->meta[e] == ORH_META_EMPTY) continue;
    const uint32_t l = g->meta[e] & ORH_META_LINK_MASK;
    if (l >= L) continue;
    uint32_t* ent = &g->link_ent[2 * static_cast<size_t>(l)];
    (ent[0] == ~0u ? ent[0] : ent[1]) = e;
  }
  std::vector<uint32_t> rev(std::max<uint32_t>(g->n_recs, 1), 0u);
  for (uint32_t e = 0; e < g->n_recs && e < rev.size(); ++e) rev[e] = e;
  for (uint32_t l = 0; l < L; ++l) {
    const uint32_t a = g->link_ent[2 * l], b = g->link_ent[2 * l + 1];
    if (a == ~0u || b == ~0u) continue;
    rev[g->pos[a]] = g->pos[b];
    rev[g->pos[b]] = g->pos[a];
  }
  if (!g->d_rev) ORH_HIP(ctx, hipMalloc(&g->d_rev, rev.size() * sizeof(uint32_t)));
  ORH_HIP(ctx, hipMemcpyAsync(g->d_rev, rev.data(), rev.size() * sizeof(uint32_t), hipMemcpyHostToDevice,
                              ctx->stream));
  ORH_HIP(ctx, hipStreamSynchronize(ctx->stream));  // rev is a local
  g->rev_gen = g->gen;
  return ORH_OK;
}

// LDS caps of the repair pass: 2,048 nodes / 8,192 edges when that state fits
// the LDS (C4 what-if 2.05 -> 1.93 ms against 1,024 / 4,096: fewer requests
// fall through to the global-slot pass), else 1,024 / 4,096
static void repair_caps(const orh_ctx* ctx, uint32_t n_nodes, uint32_t* cap_a, uint32_t* cap_e) {
  if (ctx->rep_cap_a) {
    *cap_a = ctx->rep_cap_a;
    *cap_e = ctx->rep_cap_e;
  } else if (orh::repair_lds_bytes(n_nodes, 2048, 8192) <= ctx->lds_limit) {
    *cap_a = 2048;
    *cap_e = 8192;
  } else {
    *cap_a = 1024;
    *cap_e = 4096;
  }
}

constexpr uint32_t kRepairSlots = 64;       // tier 3: whole-graph state in global memory
constexpr size_t kRepairSlotBudget = 1ull << 30;  // bytes for all slots
constexpr uint32_t kRepairMaxIgnore = 8;  // link-failure sets; KSP2 k = 2 sets are whole paths

// Slot-tier workgroups of a run of n_req >= 1 requests: one slot each, as many
// as the budget holds. 0: no slot fits this graph, and what outgrows tier 2 is
// searched in full (tier 4); runs and impact summaries must agree on that
static uint32_t repair_slots_for(uint32_t n_nodes, uint32_t n_recs, uint32_t n_req) {
  const size_t slot_bytes = orh::repair_slot_bytes(n_nodes, n_recs);
  return static_cast<uint32_t>(
      std::min<size_t>(std::min<size_t>(kRepairSlots, n_req), kRepairSlotBudget / std::max<size_t>(slot_bytes, 1)));
}

// What-if search plan for the graph: the repair needs one mask word per
// source, no zero metrics (the exact kernel's extraction order decides those
// first hops) and a full-search plan for the no-slot fallback
static int whatif_plan(orh_graph* g, bool use_link_metric, uint64_t* bound, bool* uniform) {
  orh_ctx* ctx = g->ctx;
  if (!g->d_recs || g->n_nodes == 0) return fail(ctx, ORH_E_STATE, "what-if: no graph loaded");
  if (use_link_metric && g->has_zero)
    return fail(ctx, ORH_E_UNSUPPORTED, "what-if: zero link metrics need the exact kernel");
  const uint32_t N = g->n_nodes;
  *uniform = !use_link_metric || g->min_out == g->max_out;
  const uint32_t w0 = use_link_metric ? g->max_out : 1u;
  *bound = *uniform ? static_cast<uint64_t>(N) * w0
           : use_link_metric ? g->sum_max_metric / 2 + g->max_metric
                             : static_cast<uint64_t>(g->n_links) + 1;
  uint32_t cap_a = 0, cap_e = 0;
  repair_caps(ctx, N, &cap_a, &cap_e);
  if (orh::repair_lds_bytes(N, cap_a, cap_e) > ctx->lds_limit)
    return fail(ctx, ORH_E_UNSUPPORTED, "what-if: repair state exceeds LDS");
  const orh::SpfPlan fp = orh::plan_spf(N, *uniform, *bound, g->ell_k, ctx->lds_limit, false, orh::SpfMode::kGlobal);
  if (fp.variant == orh::SpfVariant::kUnsupported)
    return fail(ctx, ORH_E_UNSUPPORTED, "what-if: no search plan for this graph");
  return ORH_OK;
}

// Can run_repair take this ignore-set batch? (sources repeat, small sets,
// one mask word, the LDS state fits, and the fallback search has a plan)
bool repair_eligible(orh_graph* g, const orh_spf_request* req, uint32_t words) {
  const orh_ctx* ctx = g->ctx;
  if (ctx->repair_mode == 0 || words != 1 || !req->h_ignore_ptr) return false;
  uint64_t bound = 0;
  bool uniform = false;
  const std::string err = g->ctx->err;
  const int rc = whatif_plan(g, req->use_link_metric != 0, &bound, &uniform);
  g->ctx->err = err;  // not eligible is not an error of this call
  if (rc) return false;
  if (ctx->repair_mode >= 2) return true;
  for (uint32_t i = 0; i < req->n_src; ++i)
    if (req->h_ignore_ptr[i + 1] - req->h_ignore_ptr[i] > kRepairMaxIgnore) return false;
  std::vector<uint32_t> s(req->h_srcs, req->h_srcs + req->n_src);
  std::sort(s.begin(), s.end());
  const size_t m = static_cast<size_t>(std::unique(s.begin(), s.end()) - s.begin());
  return 2 * m <= req->n_src;
}

}  // namespace orh::api

// A what-if job (include/openr_hip.h): the plain rows of its sources, then
// any number of request batches repaired from them
// run slots a job cycles through: run r + kRunSlots reuses run r's queues,
// staging and slot memory (and waits for its side part)
constexpr int kRunSlots = 3;

// request staging: pinned host words and their device copy (stage_acquire)
struct StageBuf {
  uint32_t* h = nullptr;
  uint32_t* d = nullptr;
  size_t cap = 0;           // u32, both sides
  hipEvent_t ev = nullptr;  // upload done (and, on the context stream, what was queued before it)
};

// what one run slot owns, and the side-stream part of its last run
struct RunSlot {
  StageBuf stage;
  uint32_t* d_work = nullptr;  // queues [3][n] | counters | fallback flags [n]
  size_t work_cap = 0;            // bytes
  hipEvent_t front_ev = nullptr;  // context-stream part done
  hipEvent_t mid_ev = nullptr;    // tiers 1 and 2 done on `side` (split runs)
  hipEvent_t side_ev = nullptr;   // side-stream part done
  bool pending = false;           // side part not yet joined into the context stream
  uintptr_t out_lo = 0, out_hi = 0;  // output span of that run (hazard checks)
  uint8_t* t3_slots = nullptr;       // the slot memory of its split slot tier
  size_t t3_slots_cap = 0;
};

struct orh_whatif {
  orh_graph* g = nullptr;
  uint64_t gen = 0;  // graph structure the base rows belong to
  int32_t use_link_metric = 1;
  bool uniform = false;
  uint64_t bound = 0;
  std::vector<uint32_t> srcs;
  uint32_t* d_base = nullptr;  // dist rows [m][N], then mask rows [m][N]
  size_t base_cap = 0;         // bytes
  // runs cycle through kRunSlots slots: the repair tiers of run r run on
  // `side` (and t3[r % kT3]) while run r + 1's seed / copy run on the context
  // stream
  hipStream_t side = nullptr;
  RunSlot run[kRunSlots];
  int cur = 0;
  hipEvent_t ev_begin = nullptr, ev_end = nullptr;  // create .. last flush
  uint64_t requests = 0;
  // tier-3 slots: the context's (when no other job holds them) or the job's own
  uint8_t* own_slots = nullptr;
  size_t own_slots_cap = 0;
  // labels of the full searches that take the slot tier's largest repairs
  // (side stream only, so one buffer serves every run slot)
  void* d_full_lab = nullptr;
  size_t full_lab_cap = 0;
  uint32_t flags = 0;  // ORH_WHATIF_* job flags
  // the slot tier of a run on a stream of its own (t3[run % kT3]), with its
  // slot's memory, after event mid_ev (tiers 1 and 2 done on `side`):
  // the next run's small tiers start without waiting for its largest repairs
  // two streams, by run parity: with the context stream and `side` that is
  // HIP's 4 hardware queues (GPU_MAX_HW_QUEUES); a fifth stream would share
  // a queue with `side` and hold its next tiers behind a slot tier
  static constexpr int kT3 = 2;
  hipStream_t t3[kT3] = {};
  uint64_t runs = 0;
  // orh_whatif_impact's request staging (base row | source node per request),
  // cycled like the run slots' but its own: an impact call is queued between
  // runs whose staging is still in flight
  StageBuf imp[kRunSlots];
  int imp_cur = 0;
};

namespace {

// The environment switches of the what-if runs, all read by whatif_knobs, once
// per process. (ORH_REPAIR_CAPS is per context: orh_create reads it.)
struct WhatifKnobs {
  // ORH_WHATIF_FULL=n (A/B, default 0): the slot tier's queue goes to full
  // searches first, up to n rows (labels within 1 GB). C4: 79 requests per
  // job searched in full 30.7-31.2 ms against 29.6 ms in slots
  // (profiles/r03/r_c4_full_search_ab.txt): the slots stay the default
  uint32_t full;
  // ORH_WHATIF_T3_SPLIT=0: the slot tier stays on `side` (A/B)
  bool t3_split;
  // ORH_WHATIF_SEARCH_CAP (256, A/B): the full searches per run of a job
  // with ORH_WHATIF_SEARCH_LARGE. 256: tier 1's whole overflow of a C4 block
  // (profiles/r06/an_skip_t2_ab/); 8 / 16 / 32 behind tier 2:
  // profiles/r06/ab_search_cap.txt
  uint32_t search_cap;
  // ORH_WHATIF_SKIP_T2=0 keeps tier 2 (A/B). By default, with full searches,
  // tier 1's overflow goes to them directly: tier 2 between them put its
  // 0.4 ms on a short job's critical path (C4 block of 8: 5.34 -> 4.73 ms,
  // profiles/r06/an_skip_t2_ab/)
  bool skip_t2;
};

const WhatifKnobs& whatif_knobs() {
  static const WhatifKnobs once = [] {
    auto num = [](const char* name, int unset) {
      const char* e = getenv(name);
      return e ? atoi(e) : unset;
    };
    WhatifKnobs k{};
    k.full = static_cast<uint32_t>(num("ORH_WHATIF_FULL", 0));
    k.t3_split = num("ORH_WHATIF_T3_SPLIT", 1) != 0;
    const int cap = num("ORH_WHATIF_SEARCH_CAP", 0);
    k.search_cap = cap > 0 ? static_cast<uint32_t>(cap) : 256u;
    k.skip_t2 = num("ORH_WHATIF_SKIP_T2", 1) != 0;
    return k;
  }();
  return once;
}

// One batch of requests of a job, as the orh_whatif_run* entry points
// pass it on
struct WhatifRequests {
  uint32_t n_req;
  const uint32_t* src_idx;
  const uint32_t *ign_ptr, *ign_links;
  // nullable (none): per request the nodes it drains, i.e. treats as
  // overloaded (orh_whatif_run_drains)
  const uint32_t *drn_ptr, *drn_nodes;
  // nullable (none): per request the metrics it raises (orh_whatif_run_metrics)
  const uint32_t* met_ptr;
  const orh_whatif_metric* mets;
  // nullable (none): per request the metrics it lowers (orh_whatif_run_lowers)
  const uint32_t* low_ptr;
  const orh_whatif_metric* lows;
  uint32_t *d_dist, *d_nh, *d_info;
};

// a raise resolved to a record: a cut and an entry of the request's sorted
// (record, raised weight) list
struct StagedRaise {
  uint32_t rec, w, tail, head, old;  // record, raised weight, its ends, its own weight
};
struct StagedRaises {
  std::vector<uint32_t> ptr;  // [n_req + 1] when the batch has a metric list
  std::vector<StagedRaise> list;
  bool any() const { return !list.empty(); }  // else: exactly the run without the lists
};

// the requests of a batch with at least one effective lower, as the lower pass
// reads them (orh::LowerArgs): per such request its lowered records and its
// sorted (record, weight) list of lowers and raises together
struct StagedLowers {
  std::vector<uint32_t> req, rec_ptr{0u}, wl_ptr{0u};
  std::vector<uint4> recs;
  std::vector<uint2> wl;
  uint32_t cap_a = 0, cap_e = 0;  // LDS caps of the pass
  bool any() const { return !req.empty(); }  // else: exactly the run without the list
};

// the staging's pinned host words and device copy for `words` words, after
// the slot's last upload: need + 25 %, at least 4,096 words
int stage_acquire(orh_ctx* ctx, StageBuf* b, size_t words) {
  if (b->ev) ORH_HIP(ctx, hipEventSynchronize(b->ev));  // its last upload is done
  if (words > b->cap) {
    if (b->h) hipHostFree(b->h);
    hipFree(b->d);
    b->h = nullptr;
    b->d = nullptr;
    b->cap = 0;
    const size_t cap = std::max<size_t>(words + words / 4, 4096);
    ORH_HIP(ctx, hipHostMalloc(reinterpret_cast<void**>(&b->h), cap * 4, hipHostMallocDefault));
    ORH_HIP(ctx, hipMalloc(&b->d, cap * 4));
    b->cap = cap;
  }
  if (!b->ev) ORH_HIP(ctx, hipEventCreateWithFlags(&b->ev, hipEventDisableTiming));
  return ORH_OK;
}

// the bytes [lo, hi) that the rows of n_req requests cover
struct Span {
  uintptr_t lo, hi;
};
Span out_span(const uint32_t* d_dist, const uint32_t* d_nh, uint32_t n_req, uint32_t N) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(d_dist), b = reinterpret_cast<uintptr_t>(d_nh);
  return {std::min(a, b), std::max(a, b) + size_t{n_req} * N * 4};
}

// every pending run whose rows overlap the span, and slot also_slot's (-1:
// none) whatever it wrote, joins the context stream
int join_overlapping(orh_whatif* job, Span s, int also_slot) {
  orh_ctx* ctx = job->g->ctx;
  for (int k = 0; k < kRunSlots; ++k) {
    RunSlot& r = job->run[k];
    if (r.pending && (k == also_slot || (s.lo < r.out_hi && r.out_lo < s.hi))) {
      ORH_HIP(ctx, hipStreamWaitEvent(ctx->stream, r.side_ev, 0));
      r.pending = false;
    }
  }
  return ORH_OK;
}
int join_all(orh_whatif* job) { return join_overlapping(job, Span{0, ~uintptr_t{0}}, -1); }

// Source indices and metric raises, validated and resolved before anything is
// queued: per request its effective raises sorted by record, the largest of a
// repeated (link, end) kept. A hop-count job checks them and stages none
int resolve_raises(orh_whatif* job, const WhatifRequests& rq, StagedRaises* out) {
  orh_graph* g = job->g;
  orh_ctx* ctx = g->ctx;
  const uint32_t n_req = rq.n_req, m = static_cast<uint32_t>(job->srcs.size());
  for (uint32_t i = 0; i < n_req; ++i)
    if (rq.src_idx[i] >= m) return fail(ctx, ORH_E_INVALID, "orh_whatif_run: source index out of range");
  if (!rq.met_ptr) return ORH_OK;
  std::vector<StagedRaise>& rse = out->list;
  const std::vector<uint32_t>& erow = entry_rows(g);
  out->ptr.assign(size_t{n_req} + 1, 0u);
  for (uint32_t i = 0; i < n_req; ++i) {
    const size_t r0 = rse.size();
    for (uint32_t k = rq.met_ptr[i]; k < rq.met_ptr[i + 1]; ++k) {
      const orh_whatif_metric& mr = rq.mets[k];
      if (mr.link >= g->n_links) continue;  // as ignore sets do
      const uint32_t ent[2] = {g->link_ent[2 * static_cast<size_t>(mr.link)],
                               g->link_ent[2 * static_cast<size_t>(mr.link) + 1]};
      if (ent[0] == ~0u && ent[1] == ~0u) continue;  // a free slot
      bool end_ok = mr.from_node == ORH_NO_NODE, down = false;
      for (uint32_t e : ent)
        if (e != ~0u) {
          end_ok |= erow[e] == mr.from_node;
          down |= (g->meta[e] & ORH_META_DOWN) != 0;
        }
      if (!end_ok)
        return fail(ctx, ORH_E_INVALID, "orh_whatif_run_metrics: from_node is not an end of the link");
      if (down) continue;  // never on a path, whatever it costs
      for (uint32_t e : ent) {
        if (e == ~0u || (mr.from_node != ORH_NO_NODE && erow[e] != mr.from_node)) continue;
        if (mr.metric < g->w_out[e])
          return fail(ctx, ORH_E_INVALID,
                      "orh_whatif_run_metrics: metric below the current one (a decrease is a topology change)");
        if (mr.metric == g->w_out[e] || !job->use_link_metric) continue;
        rse.push_back({g->pos[e], mr.metric, erow[e], g->col[e], g->w_out[e]});
      }
    }
    std::sort(rse.begin() + static_cast<ptrdiff_t>(r0), rse.end(), [](const StagedRaise& x, const StagedRaise& y) {
      return x.rec != y.rec ? x.rec < y.rec : x.w > y.w;
    });
    rse.erase(std::unique(rse.begin() + static_cast<ptrdiff_t>(r0), rse.end(),
                          [](const StagedRaise& x, const StagedRaise& y) { return x.rec == y.rec; }),
              rse.end());
    out->ptr[i + 1] = static_cast<uint32_t>(rse.size());
  }
  if (rse.empty()) return ORH_OK;
  // rows are u32: the job's distance bound (whatif_plan) plus what one
  // request adds to a path must stay below the unreached mark
  for (uint32_t i = 0; i < n_req; ++i) {
    uint64_t add = 0;
    for (uint32_t k = out->ptr[i]; k < out->ptr[i + 1]; ++k) add += rse[k].w - rse[k].old;
    if (job->bound + add >= 0xFFFFFFFFull)
      return fail(ctx, ORH_E_UNSUPPORTED, "orh_whatif_run_metrics: raised distances may exceed 32 bits");
  }
  if (repair_slots_for(g->n_nodes, g->n_recs, n_req) == 0)
    return fail(ctx, ORH_E_UNSUPPORTED,
                "orh_whatif_run_metrics: no repair slot fits this graph, and the full search takes no raises");
  return ORH_OK;
}

// LDS caps of the lower pass: sized as repair_caps sizes tier 2, with the two
// frontier bitmaps on top; false when no state fits the LDS
static bool lower_caps(const orh_ctx* ctx, uint32_t n_nodes, uint32_t* cap_a, uint32_t* cap_e) {
  const uint32_t ladder[4][2] = {{ctx->rep_cap_a, ctx->rep_cap_e}, {2048, 8192}, {1024, 4096}, {256, 1024}};
  for (const auto& c : ladder)
    if (c[0] && orh::lower_lds_bytes(n_nodes, c[0], c[1]) <= ctx->lds_limit) {
      *cap_a = c[0];
      *cap_e = c[1];
      return true;
    }
  return false;
}

// Metric lowers, validated and resolved before anything is queued: per request
// its effective lowers by record, the smallest of a repeated (link, end) kept,
// merged with its staged raises into the weight list of the lower pass. A
// hop-count job checks them and stages none
int resolve_lowers(orh_whatif* job, const WhatifRequests& rq, const StagedRaises& rs, StagedLowers* out) {
  if (!rq.low_ptr) return ORH_OK;
  orh_graph* g = job->g;
  orh_ctx* ctx = g->ctx;
  const std::vector<uint32_t>& erow = entry_rows(g);
  std::vector<uint4> cur;
  for (uint32_t i = 0; i < rq.n_req; ++i) {
    cur.clear();
    for (uint32_t k = rq.low_ptr[i]; k < rq.low_ptr[i + 1]; ++k) {
      const orh_whatif_metric& ml = rq.lows[k];
      if (ml.link >= g->n_links) continue;  // as ignore sets do
      const uint32_t ent[2] = {g->link_ent[2 * static_cast<size_t>(ml.link)],
                               g->link_ent[2 * static_cast<size_t>(ml.link) + 1]};
      if (ent[0] == ~0u && ent[1] == ~0u) continue;  // a free slot
      bool end_ok = ml.from_node == ORH_NO_NODE, down = false;
      for (uint32_t e : ent)
        if (e != ~0u) {
          end_ok |= erow[e] == ml.from_node;
          down |= (g->meta[e] & ORH_META_DOWN) != 0;
        }
      if (!end_ok) return fail(ctx, ORH_E_INVALID, "orh_whatif_run_lowers: from_node is not an end of the link");
      if (down) continue;  // restoring a down link is a topology change
      if (ml.metric == 0)
        return fail(ctx, ORH_E_UNSUPPORTED, "orh_whatif_run_lowers: what-if jobs have no zero-metric links");
      auto named = [&](uint32_t e) { return e != ~0u && (ml.from_node == ORH_NO_NODE || erow[e] == ml.from_node); };
      for (uint32_t e : ent)
        if (named(e) && ml.metric > g->w_out[e])
          return fail(ctx, ORH_E_INVALID, "orh_whatif_run_lowers: metric above the current one (a raise goes in h_metrics)");
      for (uint32_t e : ent) {
        if (!named(e)) continue;
        if (rq.met_ptr)
          for (uint32_t k2 = rq.met_ptr[i]; k2 < rq.met_ptr[i + 1]; ++k2)
            if (rq.mets[k2].link == ml.link &&
                (rq.mets[k2].from_node == ORH_NO_NODE || rq.mets[k2].from_node == erow[e]))
              return fail(ctx, ORH_E_INVALID, "orh_whatif_run_lowers: a (link, end) both raised and lowered in one request");
        if (ml.metric == g->w_out[e] || !job->use_link_metric) continue;
        cur.push_back(make_uint4(erow[e], g->col[e], g->pos[e], ml.metric));
      }
    }
    if (cur.empty()) continue;
    std::sort(cur.begin(), cur.end(), [](const uint4& x, const uint4& y) { return x.z != y.z ? x.z < y.z : x.w < y.w; });
    cur.erase(std::unique(cur.begin(), cur.end(), [](const uint4& x, const uint4& y) { return x.z == y.z; }), cur.end());
    out->req.push_back(i);
    const size_t w0 = out->wl.size();
    for (const uint4& x : cur) {
      out->recs.push_back(x);
      out->wl.push_back(make_uint2(x.z, x.w));
    }
    if (rs.any())
      for (uint32_t k = rs.ptr[i]; k < rs.ptr[i + 1]; ++k) out->wl.push_back(make_uint2(rs.list[k].rec, rs.list[k].w));
    std::sort(out->wl.begin() + static_cast<ptrdiff_t>(w0), out->wl.end(),
              [](const uint2& x, const uint2& y) { return x.x < y.x; });
    out->rec_ptr.push_back(static_cast<uint32_t>(out->recs.size()));
    out->wl_ptr.push_back(static_cast<uint32_t>(out->wl.size()));
  }
  if (!out->any()) return ORH_OK;
  if (repair_slots_for(g->n_nodes, g->n_recs, rq.n_req) == 0)
    return fail(ctx, ORH_E_UNSUPPORTED,
                "orh_whatif_run_lowers: no repair slot fits this graph, and the full search takes no lowers");
  if (!lower_caps(ctx, g->n_nodes, &out->cap_a, &out->cap_e))
    return fail(ctx, ORH_E_UNSUPPORTED, "orh_whatif_run_lowers: the lower pass's state exceeds LDS");
  return ORH_OK;
}

// The most cuts the batch stages: two per ignored link, one per out-record of
// a drained node (an upper bound: the sets are deduplicated, and lose the
// request's source, while they are staged) and one per raised record
int count_cuts(orh_whatif* job, const WhatifRequests& rq, const StagedRaises& rs, size_t* n_cuts) {
  const orh_graph* g = job->g;
  size_t n = rs.list.size();
  for (uint32_t k = 0; k < rq.ign_ptr[rq.n_req]; ++k) {
    const size_t l = rq.ign_links[k];
    if (l < g->n_links) n += (g->link_ent[2 * l] != ~0u) + (g->link_ent[2 * l + 1] != ~0u);
  }
  const uint32_t n_drn = rq.drn_ptr ? rq.drn_ptr[rq.n_req] : 0u;
  for (uint32_t k = 0; k < n_drn; ++k) {
    const uint32_t x = rq.drn_nodes[k];
    if (x >= g->n_nodes) return fail(g->ctx, ORH_E_INVALID, "orh_whatif_run_drains: drained node out of range");
    n += g->row_ptr[x + 1] - g->row_ptr[x];
  }
  *n_cuts = n;
  return ORH_OK;
}

// The staged words of a run, as u32 offsets; the only place that knows them:
//   base_row[n] | srcs[n] | ign_ptr[n+1] | ign[n_ign] |
//   with drains: drn_ptr[n+1] | drn[n_drn] |
//   cut_ptr[n+1] | (pad to 16 B) cuts uint4[n_cuts] |
//   with raises: rse_ptr[n+1] | (pad to 8 B) rse uint2[n_rse] |
//   with lowers (m requests have some): req[m] | rec_ptr[m+1] | wl_ptr[m+1] |
//     (pad to 16 B) recs uint4[n_lrec] | wl uint2[n_lwl] |
//   4 spare words
struct WhatifLayout {
  size_t off_src, off_ip, off_ign, off_dp, off_drn, off_cp, off_cuts, off_rp, off_rse, words;
  size_t off_lreq, off_lrp, off_lwp, off_lrec, off_lwl;
};
WhatifLayout whatif_layout(size_t n, size_t n_ign, bool drains, size_t n_drn, size_t n_cuts, size_t n_rse,
                           const StagedLowers& sl) {
  WhatifLayout l{};
  l.off_src = n;
  l.off_ip = 2 * n;
  l.off_ign = l.off_ip + n + 1;
  l.off_dp = l.off_ign + n_ign;
  l.off_drn = l.off_dp + n + 1;
  l.off_cp = drains ? l.off_drn + n_drn : l.off_ign + n_ign;
  l.off_cuts = (l.off_cp + n + 1 + 3) & ~size_t{3};
  l.off_rp = l.off_cuts + 4 * n_cuts;
  l.off_rse = (l.off_rp + n + 1 + 1) & ~size_t{1};
  size_t end = n_rse ? l.off_rse + 2 * n_rse : l.off_rp;
  if (sl.any()) {
    const size_t m = sl.req.size();
    l.off_lreq = end;
    l.off_lrp = l.off_lreq + m;
    l.off_lwp = l.off_lrp + m + 1;
    l.off_lrec = (l.off_lwp + m + 1 + 3) & ~size_t{3};
    l.off_lwl = l.off_lrec + 4 * sl.recs.size();
    end = l.off_lwl + 2 * sl.wl.size();
  }
  l.words = end + 4;
  return l;
}

// The pinned words of a run: per request its ignore set sorted and unique, its
// drain set likewise and without its own source, and its cuts: ignored link
// ends, then drained nodes' out-records, then raised records
void fill_stage(const orh_whatif* job, const WhatifRequests& rq, const StagedRaises& rs, const StagedLowers& sl,
                const WhatifLayout& l, uint32_t* h) {
  orh_graph* g = job->g;
  const uint32_t n_req = rq.n_req;
  std::memcpy(h, rq.src_idx, n_req * 4ull);
  for (uint32_t i = 0; i < n_req; ++i) h[l.off_src + i] = job->srcs[rq.src_idx[i]];
  uint32_t* hp = h + l.off_ip;
  uint32_t* hc = h + l.off_cp;
  uint4* cuts = reinterpret_cast<uint4*>(h + l.off_cuts);
  uint2* hr = rs.any() ? reinterpret_cast<uint2*>(h + l.off_rse) : nullptr;
  const std::vector<uint32_t>& erow = entry_rows(g);
  size_t ni = 0, nc = 0, nd = 0;
  hp[0] = 0;
  hc[0] = 0;
  if (rq.drn_ptr) h[l.off_dp] = 0;
  for (uint32_t i = 0; i < n_req; ++i) {
    uint32_t* set = h + l.off_ign + ni;
    size_t len = 0;
    for (uint32_t k = rq.ign_ptr[i]; k < rq.ign_ptr[i + 1]; ++k) set[len++] = rq.ign_links[k];
    std::sort(set, set + len);  // bsearch on device
    len = static_cast<size_t>(std::unique(set, set + len) - set);
    for (size_t k = 0; k < len; ++k) {
      const uint32_t ln = set[k];
      if (ln >= g->n_links) continue;
      for (int e2 = 0; e2 < 2; ++e2) {
        const uint32_t e = g->link_ent[2 * static_cast<size_t>(ln) + e2];
        if (e == ~0u) continue;
        cuts[nc++] = make_uint4(erow[e], g->col[e], g->pos[e], 0u);
      }
    }
    ni += len;
    hp[i + 1] = static_cast<uint32_t>(ni);
    if (rq.drn_ptr) {
      // the request's drain set, sorted (bsearch on device), without its own
      // source (an overloaded source still relaxes, LinkState.cpp:831-838);
      // one cut per out-record of each node: the seeds test their tightness
      // and skip a tail that is overloaded already or unreached
      uint32_t* dset = h + l.off_drn + nd;
      size_t dl = 0;
      for (uint32_t k = rq.drn_ptr[i]; k < rq.drn_ptr[i + 1]; ++k)
        if (rq.drn_nodes[k] != job->srcs[rq.src_idx[i]]) dset[dl++] = rq.drn_nodes[k];
      std::sort(dset, dset + dl);
      dl = static_cast<size_t>(std::unique(dset, dset + dl) - dset);
      for (size_t k = 0; k < dl; ++k) {
        const uint32_t x = dset[k];
        for (uint32_t e = g->row_ptr[x]; e < g->row_ptr[x + 1]; ++e)
          if (g->meta[e] != ORH_META_EMPTY) cuts[nc++] = make_uint4(x, g->col[e], g->pos[e], 0u);
      }
      nd += dl;
      h[l.off_dp + i + 1] = static_cast<uint32_t>(nd);
    }
    if (rs.any())
      for (uint32_t k = rs.ptr[i]; k < rs.ptr[i + 1]; ++k) {
        cuts[nc++] = make_uint4(rs.list[k].tail, rs.list[k].head, rs.list[k].rec, 0u);
        hr[k] = make_uint2(rs.list[k].rec, rs.list[k].w);
      }
    hc[i + 1] = static_cast<uint32_t>(nc);
  }
  if (rs.any()) std::memcpy(h + l.off_rp, rs.ptr.data(), (size_t{n_req} + 1) * 4);
  if (sl.any()) {  // the lower pass's lists, as resolve_lowers made them
    std::memcpy(h + l.off_lreq, sl.req.data(), sl.req.size() * 4);
    std::memcpy(h + l.off_lrp, sl.rec_ptr.data(), sl.rec_ptr.size() * 4);
    std::memcpy(h + l.off_lwp, sl.wl_ptr.data(), sl.wl_ptr.size() * 4);
    std::memcpy(h + l.off_lrec, sl.recs.data(), sl.recs.size() * sizeof(uint4));
    std::memcpy(h + l.off_lwl, sl.wl.data(), sl.wl.size() * sizeof(uint2));
  }
}

// what provision_run decided for a run
struct RunPlan {
  uint32_t n_slots;  // workgroups of the slot tier; 0: no slot fits the budget
  size_t slot_bytes;
  uint8_t* slot_mem;
  // full searches wanted for the slot tier's queue: ORH_WHATIF_FULL=n (A/B),
  // or the job's ORH_WHATIF_SEARCH_LARGE (ORH_WHATIF_SEARCH_CAP per run). A
  // run with raises takes none (the search knows no raised weights): its slot
  // tier ends every request
  // run with lowers neither (a lower leaves the metric range the search's
  // bucket widths are planned from)
  uint32_t full_n;
  bool split;           // the slot tier on its own stream, over the run slot's memory
  uint32_t full_cap;    // of full_n, what the labels' 1 GB and the batch allow
  uint32_t skip_large;  // no tier 2 in front of the full searches
  // rows the full search may take, i.e. the labels it needs: full_cap of the
  // slot tier's queue, or without slots any of the batch (the flagged ones)
  uint32_t search_rows;
};

// *p freed and exactly `bytes` (never 0) allocated in its place, whatever *cap
// was; the caller has waited for whatever may still use the old memory
int regrow(orh_ctx* ctx, void** p, size_t* cap, size_t bytes) {
  *cap = 0;  // nothing fits: grow_device frees *p and allocates anew
  return grow_device(ctx, p, cap, bytes, 1, false);
}

// Work queues, slot memory and full-search labels of the run in slot c, each
// grown to the exact need, after the wait that makes freeing the old one safe
int provision_run(orh_whatif* job, int c, uint32_t n_req, bool raises, uint32_t n_low, RunPlan* out) {
  orh_graph* g = job->g;
  orh_ctx* ctx = g->ctx;
  RunSlot& slot = job->run[c];
  const uint32_t N = g->n_nodes;
  const WhatifKnobs& knobs = whatif_knobs();
  // the lower pass's slot queue (one word per request that lowers) at the end
  const size_t work = 3 * size_t{n_req} + orh::kWhatifCounters + n_req + n_low;
  if (work * 4 > slot.work_cap) {
    if (slot.pending) ORH_HIP(ctx, hipStreamSynchronize(job->side));  // its old buffer may be in use
    const int rc = regrow(ctx, reinterpret_cast<void**>(&slot.d_work), &slot.work_cap, work * 4);
    if (rc) return rc;
  }
  ORH_HIP(ctx, hipMemsetAsync(slot.d_work + 3 * size_t{n_req}, 0, (orh::kWhatifCounters + n_req) * 4ull,
                              ctx->stream));
  RunPlan p{};
  p.slot_bytes = orh::repair_slot_bytes(N, g->n_recs);
  p.n_slots = repair_slots_for(N, g->n_recs, n_req);
  p.full_n = raises ? 0u : knobs.full ? knobs.full : (job->flags & ORH_WHATIF_SEARCH_LARGE) ? knobs.search_cap : 0u;
  p.split = p.n_slots && p.full_n == 0 && knobs.t3_split;
  const size_t slots_bytes = p.n_slots * p.slot_bytes;
  if (p.split) {
    // run slot c's own slot memory, grown only with its streams idle
    if (slots_bytes > slot.t3_slots_cap) {
      for (hipStream_t t : job->t3) ORH_HIP(ctx, hipStreamSynchronize(t));
      const int rc = regrow(ctx, reinterpret_cast<void**>(&slot.t3_slots), &slot.t3_slots_cap, slots_bytes);
      if (rc) return rc;
    }
    p.slot_mem = slot.t3_slots;
  } else if (p.n_slots) {
    // the context's slots while no other job's side stream may use them,
    // else the job's own; grown only with the side stream idle
    if (!ctx->slots_owner) ctx->slots_owner = job;
    const bool borrowed = ctx->slots_owner == job;
    uint8_t** mem = borrowed ? &ctx->d_rep_slots : &job->own_slots;
    size_t* cap = borrowed ? &ctx->d_rep_slots_cap : &job->own_slots_cap;
    if (slots_bytes > *cap) ORH_HIP(ctx, hipStreamSynchronize(job->side));
    const int rc = ensure_bytes(ctx, mem, cap, slots_bytes);
    if (rc) return rc;
    p.slot_mem = *mem;
  }
  if (p.n_slots) {
    const size_t by_mem = (size_t{1} << 30) / (static_cast<size_t>(N) * 8);
    p.full_cap = static_cast<uint32_t>(std::min<size_t>({p.full_n, by_mem, n_req}));
    p.skip_large = (knobs.skip_t2 && p.full_cap) ? 1u : 0u;
  }
  // job-owned labels: the searches run on the job's side stream, which later
  // work on the context stream (searches over ctx->d_labels) does not wait for
  p.search_rows = p.n_slots ? p.full_cap : n_req;
  const size_t need = static_cast<size_t>(p.search_rows) * N * 8;
  if (need > job->full_lab_cap) {
    ORH_HIP(ctx, hipStreamSynchronize(job->side));  // the old buffer may be in use
    const int rc = regrow(ctx, &job->d_full_lab, &job->full_lab_cap, need);
    if (rc) return rc;
  }
  *out = p;
  return ORH_OK;
}

orh::RepairArgs fill_repair_args(const orh_whatif* job, int c, const WhatifLayout& l, const RunPlan& p,
                                 const WhatifRequests& rq, bool raises) {
  const orh_graph* g = job->g;
  const orh_ctx* ctx = g->ctx;
  const RunSlot& slot = job->run[c];
  const uint32_t* d = slot.stage.d;
  orh::RepairArgs ra{};
  ra.n_nodes = g->n_nodes;
  ra.n_req = rq.n_req;
  ra.use_link_metric = job->use_link_metric;
  repair_caps(ctx, g->n_nodes, &ra.cap_a, &ra.cap_e);
  ra.recs = g->d_recs;
  ra.link = g->d_link;
  ra.rank_out = g->d_rank_out;
  ra.rev = g->d_rev;
  ra.ovl = g->d_ovl;
  ra.base_dist = job->d_base;
  ra.base_nh = job->d_base + job->srcs.size() * static_cast<size_t>(g->n_nodes);
  ra.base_row = d;
  ra.srcs = d + l.off_src;
  ra.ign_ptr = d + l.off_ip;
  ra.ign = d + l.off_ign;
  if (rq.drn_ptr) {
    ra.drn_ptr = d + l.off_dp;
    ra.drn = d + l.off_drn;
  }
  if (raises) {
    ra.rse_ptr = d + l.off_rp;
    ra.rse = reinterpret_cast<const uint2*>(d + l.off_rse);
  }
  ra.cut_ptr = d + l.off_cp;
  ra.cuts = reinterpret_cast<const uint4*>(d + l.off_cuts);
  ra.out_dist = rq.d_dist;
  ra.out_nh = rq.d_nh;
  ra.queues = slot.d_work;
  ra.counters = slot.d_work + 3 * size_t{rq.n_req};
  ra.fallback = ra.counters + orh::kWhatifCounters;
  ra.info = rq.d_info;
  ra.slot_mem = p.slot_mem;
  ra.slot_bytes = p.slot_bytes;
  ra.n_slots = p.n_slots;
  ra.n_recs = g->n_recs;
  ra.n_cu = ctx->n_cu;
  ra.share_base = (job->flags & ORH_WHATIF_SHARE_BASE) ? 1u : 0u;
  ra.full_cap = p.full_cap;
  ra.skip_large = p.skip_large;
  return ra;
}

// the lower pass over the run's staged requests (n_low 0: the run has none)
orh::LowerArgs fill_lower_args(const orh_whatif* job, int c, const WhatifLayout& l, const StagedLowers& sl,
                               uint32_t n_req) {
  orh::LowerArgs la{};
  if (!sl.any()) return la;
  const RunSlot& slot = job->run[c];
  const uint32_t* d = slot.stage.d;
  la.n_low = static_cast<uint32_t>(sl.req.size());
  la.req = d + l.off_lreq;
  la.rec_ptr = d + l.off_lrp;
  la.recs = reinterpret_cast<const uint4*>(d + l.off_lrec);
  la.wl_ptr = d + l.off_lwp;
  la.wl = reinterpret_cast<const uint2*>(d + l.off_lwl);
  la.queue = slot.d_work + 3 * size_t{n_req} + orh::kWhatifCounters + n_req;
  la.cap_a = sl.cap_a;
  la.cap_e = sl.cap_e;
  return la;
}

// The full search (spf_global_nh_async_kernel) over the run's staged requests.
// With slots it takes the first entries of the slot tier's queue: workgroup b
// searches request queue[b] while b < the queue's length. Without, the
// requests that outgrew tier 2, through the fallback flags as its row mask
// (the others exit at once; scratch is unused, every row is < n_out)
orh::SpfArgs full_search_args(const orh_whatif* job, const orh::RepairArgs& ra) {
  const orh_graph* g = job->g;
  orh::SpfArgs a{};
  a.n_nodes = ra.n_nodes;
  a.n_out = ra.n_req;
  a.recs = g->d_recs;
  a.link = g->d_link;
  a.srcs = ra.srcs;
  a.ignore_ptr = ra.ign_ptr;
  a.ignore_links = ra.ign;
  a.use_link_metric = job->use_link_metric;
  a.w0 = job->use_link_metric ? g->max_out : 1u;
  a.delta = job->uniform ? a.w0
                         : std::max<uint32_t>(1u, static_cast<uint32_t>(static_cast<uint64_t>(g->mean_out) *
                                                                        g->ctx->delta_pct / 100u));
  a.out_dist = ra.out_dist;
  a.scratch = g->ctx->d_scratch;
  a.labels = static_cast<unsigned long long*>(job->d_full_lab);
  a.out_nh = ra.out_nh;
  a.words = 1;
  a.rank_out = g->d_rank_out;
  a.drain_ptr = ra.drn_ptr;
  a.drain_nodes = ra.drn;
  if (ra.n_slots) {
    const uint32_t q = orh::repair_slot_queue(ra);
    a.row_list = ra.queues + static_cast<size_t>(q) * ra.n_req;
    a.row_count = ra.counters + 2 * q;
  } else {
    a.row_mask = ra.fallback;
  }
  return a;
}

// Seed and copy on the context stream; the repair tiers on `side` behind
// them, the slot tier of a split run on its t3 stream; then the full search
// on `side`; then the lower pass (stage 2 of the requests that lower metrics)
// behind the run's last tier, on that tier's stream. side_ev marks the end of
// the run's side part
int launch_run(orh_whatif* job, int c, const orh::RepairArgs& ra, const orh::LowerArgs& la, const RunPlan& p) {
  orh_graph* g = job->g;
  orh_ctx* ctx = g->ctx;
  RunSlot& slot = job->run[c];
  hipError_t e = orh::launch_repair_front(ra, g->ell_k, ctx->lds_limit, ctx->stream);
  if (e != hipSuccess) return hip_fail(ctx, e, "what-if repair launch");
  ORH_HIP(ctx, hipEventRecord(slot.front_ev, ctx->stream));
  // the large repairs on the side stream, after this run's front part; the
  // previous side part is ordered before them on that stream
  ORH_HIP(ctx, hipStreamWaitEvent(job->side, slot.front_ev, 0));
  hipStream_t t3s = job->t3[job->runs % orh_whatif::kT3];
  ++job->runs;
  e = p.split ? orh::launch_repair_back_split(ra, g->ell_k, ctx->lds_limit, job->side, t3s, slot.mid_ev)
              : orh::launch_repair_back(ra, g->ell_k, ctx->lds_limit, job->side);
  if (e != hipSuccess) return hip_fail(ctx, e, "what-if repair launch (large tiers)");
  if (p.search_rows) {
    orh::SpfPlan fp = orh::plan_spf(ra.n_nodes, job->uniform, job->bound, g->ell_k, ctx->lds_limit, false,
                                    orh::SpfMode::kGlobal);
    if (fp.variant == orh::SpfVariant::kUnsupported)
      return fail(ctx, ORH_E_UNSUPPORTED, "what-if: no search plan for this graph");
    fp.variant = orh::SpfVariant::kGlobalNh;
    fp.block = 1024;
    e = orh::launch_spf(fp, full_search_args(job, ra), p.search_rows, job->side);
    if (e != hipSuccess)
      return hip_fail(ctx, e, p.n_slots ? "what-if full-search launch" : "what-if fallback launch");
  }
  if (la.n_low) {
    e = orh::launch_lower(ra, la, g->ell_k, ctx->lds_limit, p.split ? t3s : job->side);
    if (e != hipSuccess) return hip_fail(ctx, e, "what-if lower launch");
  }
  // the run's side part ends with its slot tier (its t3 stream, ordered after
  // tiers 1 and 2 through mid_ev) or on `side`
  ORH_HIP(ctx, hipEventRecord(slot.side_ev, p.split ? t3s : job->side));
  return ORH_OK;
}

// one batch of requests of a job: seed and copy and the small repair tiers
// on the context stream; the large tiers, the slot tier (t3 streams) and,
// without slots, the full search for what outgrew tier 2 on the job's side
// streams, over job-owned memory (slots, labels), joined back into the
// context stream through side_ev
int whatif_run(orh_whatif* job, const WhatifRequests& rq) {
  orh_graph* g = job->g;
  orh_ctx* ctx = g->ctx;
  const uint32_t n_req = rq.n_req;
  StagedRaises rs;
  StagedLowers sl;
  size_t n_cuts = 0;
  int rc = resolve_raises(job, rq, &rs);
  if (!rc) rc = resolve_lowers(job, rq, rs, &sl);
  if (!rc) rc = count_cuts(job, rq, rs, &n_cuts);
  if (rc) return rc;
  const WhatifLayout lay = whatif_layout(n_req, rq.ign_ptr[n_req], rq.drn_ptr != nullptr,
                                         rq.drn_ptr ? rq.drn_ptr[n_req] : 0u, n_cuts, rs.list.size(), sl);
  // slot `cur` is reused: its previous run's side part must be done (the
  // context stream waits); so must the other slots' when they write rows this
  // run overwrites
  const int c = job->cur;
  RunSlot& slot = job->run[c];
  const Span out = out_span(rq.d_dist, rq.d_nh, n_req, g->n_nodes);
  rc = join_overlapping(job, out, c);
  if (!rc) rc = stage_acquire(ctx, &slot.stage, lay.words);
  if (rc) return rc;
  fill_stage(job, rq, rs, sl, lay, slot.stage.h);
  job->cur = (c + 1) % kRunSlots;
  ORH_HIP(ctx, hipMemcpyAsync(slot.stage.d, slot.stage.h, lay.words * 4, hipMemcpyHostToDevice, ctx->stream));
  ORH_HIP(ctx, hipEventRecord(slot.stage.ev, ctx->stream));
  RunPlan plan{};
  // neither raises nor lowers go to a full search
  rc = provision_run(job, c, n_req, rs.any() || sl.any(), static_cast<uint32_t>(sl.req.size()), &plan);
  if (rc) return rc;
  const orh::RepairArgs ra = fill_repair_args(job, c, lay, plan, rq, rs.any());
  rc = launch_run(job, c, ra, fill_lower_args(job, c, lay, sl, n_req), plan);
  if (rc) return rc;
  slot.pending = true;
  slot.out_lo = out.lo;
  slot.out_hi = out.hi;
  job->requests += n_req;
  ctx->counters.spf_runs += n_req;  // one runSpf per request (LinkState.cpp:815)
  ctx->counters.spf_launches += 1;
  ctx->counters.last_kernel_ms = -1.0;
  return ORH_OK;
}

// the side-stream parts of every run so far join the context stream: work
// queued on it afterwards sees all of the job's rows
int whatif_flush(orh_whatif* job) {
  orh_ctx* ctx = job->g->ctx;
  const int rc = join_all(job);
  if (rc) return rc;
  ORH_HIP(ctx, hipEventRecord(job->ev_end, ctx->stream));
  return ORH_OK;
}

// What orh_whatif_impact and orh_whatif_gain share: validation, the joins of
// the runs that wrote the rows, and the staged (base row | source node) words
// of the requests. `what` names the entry point in error messages.
struct SummaryStage {
  const uint32_t* base_dist;
  const uint32_t* base_nh;
  const uint32_t* base_row;  // device [n_req]
  const uint32_t* srcs;      // device [n_req]
  const uint32_t* info;      // the caller's d_info, or null where tier 0 proves nothing
};
int whatif_summary_stage(orh_whatif* job, const char* what, uint32_t n_req, const uint32_t* src_idx,
                         const uint32_t* d_dist, const uint32_t* d_nh, const uint32_t* d_info, SummaryStage* out) {
  orh_graph* g = job->g;
  orh_ctx* ctx = g->ctx;
  const std::string name(what);
  const uint32_t N = g->n_nodes, m = static_cast<uint32_t>(job->srcs.size());
  for (uint32_t i = 0; i < n_req; ++i)
    if (src_idx[i] >= m) return fail(ctx, ORH_E_INVALID, name + ": source index out of range");
  const bool share = (job->flags & ORH_WHATIF_SHARE_BASE) != 0;
  if (share && !d_info)
    return fail(ctx, ORH_E_INVALID, name + ": a SHARE_BASE job's tier-0 rows were never written, d_info is needed");
  // a graph whose runs have no tier-3 slots leaves tier 0 in d_info for the
  // requests its full search re-derived: tier 0 does not prove there that the
  // row stands, so every row is scanned
  if (repair_slots_for(N, g->n_recs, n_req) == 0) {
    if (share) return fail(ctx, ORH_E_UNSUPPORTED, name + ": SHARE_BASE on a graph without repair slots");
    d_info = nullptr;
  }
  // every pending run whose rows overlap the given ones joins the context stream
  int rc = join_overlapping(job, out_span(d_dist, d_nh, n_req, N), -1);
  if (rc) return rc;
  StageBuf& st = job->imp[job->imp_cur];
  const size_t words = 2 * size_t{n_req};
  rc = stage_acquire(ctx, &st, words);
  if (rc) return rc;
  std::memcpy(st.h, src_idx, n_req * 4ull);
  for (uint32_t i = 0; i < n_req; ++i) st.h[n_req + i] = job->srcs[src_idx[i]];
  job->imp_cur = (job->imp_cur + 1) % kRunSlots;
  ORH_HIP(ctx, hipMemcpyAsync(st.d, st.h, words * 4, hipMemcpyHostToDevice, ctx->stream));
  ORH_HIP(ctx, hipEventRecord(st.ev, ctx->stream));
  out->base_dist = job->d_base;
  out->base_nh = job->d_base + static_cast<size_t>(m) * N;
  out->base_row = st.d;
  out->srcs = st.d + n_req;
  out->info = d_info;
  return ORH_OK;
}

// the public entry points' checks before anything is staged
int whatif_summary_check(orh_whatif* job, const char* what, const uint32_t* h_src_idx, const uint32_t* d_dist,
                         const uint32_t* d_nh, const void* d_out) {
  orh_ctx* ctx = job->g->ctx;
  if (!h_src_idx || !d_dist || !d_nh || !d_out) return fail(ctx, ORH_E_INVALID, std::string(what) + ": null argument");
  if (job->gen != job->g->gen)
    return fail(ctx, ORH_E_STATE, std::string(what) + ": the graph changed since the job was created");
  return ORH_OK;
}

// orh_whatif_impact: the requests' rows against their sources' base rows,
// one record each, on the context stream behind the runs that wrote the rows
int whatif_impact(orh_whatif* job, uint32_t n_req, const uint32_t* src_idx, const uint32_t* d_dist,
                  const uint32_t* d_nh, const uint32_t* d_info, const orh_whatif_impact_opts* opts,
                  orh_whatif_impact_rec* d_out) {
  orh_ctx* ctx = job->g->ctx;
  SummaryStage st{};
  const int rc = whatif_summary_stage(job, "orh_whatif_impact", n_req, src_idx, d_dist, d_nh, d_info, &st);
  if (rc) return rc;
  orh::ImpactArgs a{};
  a.n_nodes = job->g->n_nodes;
  a.n_req = n_req;
  a.base_dist = st.base_dist;
  a.base_nh = st.base_nh;
  a.base_row = st.base_row;
  a.srcs = st.srcs;
  a.dist = d_dist;
  a.nh = d_nh;
  a.info = st.info;
  if (opts) {
    a.weight = opts->d_weight;
    a.node_lost = opts->d_node_lost;
    a.node_moved = opts->d_node_moved;
  }
  a.out = d_out;
  const hipError_t e = orh::launch_whatif_impact(a, ctx->stream);
  if (e != hipSuccess) return hip_fail(ctx, e, "what-if impact launch");
  return ORH_OK;
}

// orh_whatif_gain: the same with the two-sided classes
int whatif_gain(orh_whatif* job, uint32_t n_req, const uint32_t* src_idx, const uint32_t* d_dist,
                const uint32_t* d_nh, const uint32_t* d_info, const orh_whatif_gain_opts* opts,
                orh_whatif_gain_rec* d_out) {
  orh_ctx* ctx = job->g->ctx;
  SummaryStage st{};
  const int rc = whatif_summary_stage(job, "orh_whatif_gain", n_req, src_idx, d_dist, d_nh, d_info, &st);
  if (rc) return rc;
  orh::GainArgs a{};
  a.n_nodes = job->g->n_nodes;
  a.n_req = n_req;
  a.base_dist = st.base_dist;
  a.base_nh = st.base_nh;
  a.base_row = st.base_row;
  a.srcs = st.srcs;
  a.dist = d_dist;
  a.nh = d_nh;
  a.info = st.info;
  if (opts) {
    a.weight = opts->d_weight;
    a.node_lost = opts->d_node_lost;
    a.node_moved = opts->d_node_moved;
    a.node_nearer = opts->d_node_nearer;
  }
  a.out = d_out;
  const hipError_t e = orh::launch_whatif_gain(a, ctx->stream);
  if (e != hipSuccess) return hip_fail(ctx, e, "what-if gain launch");
  return ORH_OK;
}

// the plain SPFs of the job's sources into its base rows, on the graph as it
// is now (create, and orh_whatif_refresh after topology changes); the side
// parts of earlier runs, which read the old rows, are joined first
int whatif_base(orh_whatif* job) {
  orh_graph* g = job->g;
  orh_ctx* ctx = g->ctx;
  uint64_t bound = 0;
  bool uniform = false;
  int rc = whatif_plan(g, job->use_link_metric != 0, &bound, &uniform);
  if (rc) return rc;
  for (uint32_t s : job->srcs) {
    if (s >= g->n_nodes) return fail(ctx, ORH_E_INVALID, "what-if: source out of range");
    if (n_distinct(g, s) > 32) return fail(ctx, ORH_E_UNSUPPORTED, "what-if: a source has more than 32 neighbours");
  }
  job->uniform = uniform;
  job->bound = bound;
  rc = ensure_rev(g);
  if (!rc) rc = join_all(job);
  if (rc) return rc;
  const uint32_t m = static_cast<uint32_t>(job->srcs.size());
  const size_t nd = static_cast<size_t>(std::max<uint32_t>(m, 1)) * g->n_nodes;
  if (nd * 8 > job->base_cap) {
    ORH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    hipFree(job->d_base);
    job->d_base = nullptr;
    job->base_cap = 0;
    if (hipMalloc(&job->d_base, nd * 8) != hipSuccess) return fail(ctx, ORH_E_NOMEM, "what-if: base rows");
    job->base_cap = nd * 8;
  }
  ORH_HIP(ctx, hipEventRecord(job->ev_begin, ctx->stream));
  if (m) {
    // internal searches: spf_runs counts the requests
    orh_spf_request br{};
    br.h_srcs = job->srcs.data();
    br.n_src = m;
    br.use_link_metric = job->use_link_metric;
    const orh_counters c0 = ctx->counters;
    rc = orh_spf_run(g, &br, 1, job->d_base, job->d_base + static_cast<size_t>(m) * g->n_nodes);
    ctx->counters = c0;
    if (rc) return rc;
  }
  ORH_HIP(ctx, hipEventRecord(job->ev_end, ctx->stream));
  job->gen = g->gen;
  return ORH_OK;
}

int whatif_create(orh_graph* g, const uint32_t* h_srcs, uint32_t n_srcs, int32_t use_link_metric,
                  orh_whatif** out) {
  orh_ctx* ctx = g->ctx;
  uint64_t bound = 0;
  bool uniform = false;
  int rc = whatif_plan(g, use_link_metric != 0, &bound, &uniform);
  if (rc) return rc;
  for (uint32_t i = 0; i < n_srcs; ++i) {
    if (h_srcs[i] >= g->n_nodes) return fail(ctx, ORH_E_INVALID, "orh_whatif_create: source out of range");
    if (n_distinct(g, h_srcs[i]) > 32)
      return fail(ctx, ORH_E_UNSUPPORTED, "orh_whatif_create: a source has more than 32 neighbours");
  }
  hipSetDevice(ctx->device);
  auto* job = new (std::nothrow) orh_whatif();
  if (!job) return fail(ctx, ORH_E_NOMEM, "orh_whatif_create");
  job->g = g;
  job->gen = g->gen;
  job->use_link_metric = use_link_metric ? 1 : 0;
  job->uniform = uniform;
  job->bound = bound;
  job->srcs.assign(h_srcs, h_srcs + n_srcs);
  auto bail = [&](int code) {
    orh_whatif_destroy(job);
    return code;
  };
  if (hipEventCreate(&job->ev_begin) != hipSuccess || hipEventCreate(&job->ev_end) != hipSuccess ||
      hipStreamCreateWithFlags(&job->side, hipStreamNonBlocking) != hipSuccess)
    return bail(fail(ctx, ORH_E_DEVICE, "orh_whatif_create: events / stream"));
  for (RunSlot& r : job->run)
    if (hipEventCreateWithFlags(&r.front_ev, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&r.side_ev, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&r.mid_ev, hipEventDisableTiming) != hipSuccess)
      return bail(fail(ctx, ORH_E_DEVICE, "orh_whatif_create: events"));
  for (hipStream_t& t : job->t3)
    if (hipStreamCreateWithFlags(&t, hipStreamNonBlocking) != hipSuccess)
      return bail(fail(ctx, ORH_E_DEVICE, "orh_whatif_create: streams"));
  rc = whatif_base(job);
  if (rc) return bail(rc);
  *out = job;
  return ORH_OK;
}

}  // namespace

namespace orh::api {

// runSpf(src, useLinkMetric, ignore) for every request of an ignore-set batch
// from the plain rows of its distinct sources: a what-if job over those
// sources, one run, destroyed after its kernels are queued (stream order)
int run_repair(orh_graph* g, const orh_spf_request* req, uint32_t* d_dist, uint32_t* d_nh) {
  orh_ctx* ctx = g->ctx;
  const uint32_t n_src = req->n_src;
  std::vector<uint32_t> base_srcs, base_row(n_src);
  auto& ro = g->row_of;
  for (uint32_t i = 0; i < n_src; ++i) {
    const uint32_t s = req->h_srcs[i];
    if (ro[s] < 0) {
      ro[s] = static_cast<int32_t>(base_srcs.size());
      base_srcs.push_back(s);
    }
    base_row[i] = static_cast<uint32_t>(ro[s]);
  }
  for (uint32_t s : base_srcs) ro[s] = -1;
  orh_whatif* job = nullptr;
  ORH_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  int rc = whatif_create(g, base_srcs.data(), static_cast<uint32_t>(base_srcs.size()), req->use_link_metric, &job);
  if (rc) return rc;
  ORH_HIP(ctx, hipEventRecord(ctx->evm, ctx->stream));
  rc = whatif_run(job, WhatifRequests{n_src, base_row.data(), req->h_ignore_ptr, req->h_ignore_links, nullptr, nullptr,
                                      nullptr, nullptr, nullptr, nullptr, d_dist, d_nh, nullptr});
  if (!rc) rc = whatif_flush(job);
  if (rc) {
    orh_whatif_destroy(job);
    return rc;
  }
  ORH_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  orh_whatif_destroy(job);
  orh_spf_info info{};
  info.variant = static_cast<int32_t>(orh::SpfVariant::kRepair);
  info.rows = n_src;
  info.batch_sources = static_cast<uint32_t>(base_srcs.size());
  ctx->last_info = info;
  return ORH_OK;
}

}  // namespace orh::api

extern "C" {

int orh_whatif_create(orh_graph* g, const uint32_t* h_srcs, uint32_t n_srcs, int32_t use_link_metric,
                      orh_whatif** out) {
  if (!g || !out || (n_srcs && !h_srcs)) return g ? fail(g->ctx, ORH_E_INVALID, "orh_whatif_create: null argument")
                                                  : ORH_E_INVALID;
  *out = nullptr;
  join_deferred(g->ctx);
  return whatif_create(g, h_srcs, n_srcs, use_link_metric, out);
}

// the checks the orh_whatif_run* entry points share, under `fn`'s name, then
// the run; a list that an entry point does not take is null here
static int checked_run(orh_whatif* job, const WhatifRequests& rq, const char* fn) {
  if (!job) return ORH_E_INVALID;
  orh_ctx* ctx = job->g->ctx;
  join_deferred(ctx);
  const uint32_t n = rq.n_req;
  if (n == 0) return ORH_OK;
  if (!rq.src_idx || !rq.ign_ptr || (rq.ign_ptr[n] && !rq.ign_links) ||
      (rq.drn_ptr && rq.drn_ptr[n] && !rq.drn_nodes) || (rq.met_ptr && rq.met_ptr[n] && !rq.mets) ||
      (rq.low_ptr && rq.low_ptr[n] && !rq.lows) || !rq.d_dist || !rq.d_nh)
    return fail(ctx, ORH_E_INVALID, std::string(fn) + ": null argument");
  if (job->gen != job->g->gen)
    return fail(ctx, ORH_E_STATE, std::string(fn) + ": the graph changed since the job was created");
  hipSetDevice(ctx->device);
  return whatif_run(job, rq);
}

int orh_whatif_run(orh_whatif* job, uint32_t n_req, const uint32_t* h_src_idx, const uint32_t* h_ignore_ptr,
                   const uint32_t* h_ignore_links, uint32_t* d_dist, uint32_t* d_nh, uint32_t* d_info) {
  return checked_run(job, WhatifRequests{n_req, h_src_idx, h_ignore_ptr, h_ignore_links, nullptr, nullptr, nullptr,
                                         nullptr, nullptr, nullptr, d_dist, d_nh, d_info},
                     "orh_whatif_run");
}

int orh_whatif_run_drains(orh_whatif* job, uint32_t n_req, const uint32_t* h_src_idx, const uint32_t* h_ignore_ptr,
                          const uint32_t* h_ignore_links, const uint32_t* h_drain_ptr, const uint32_t* h_drain_nodes,
                          uint32_t* d_dist, uint32_t* d_nh, uint32_t* d_info) {
  return checked_run(job, WhatifRequests{n_req, h_src_idx, h_ignore_ptr, h_ignore_links, h_drain_ptr, h_drain_nodes,
                                         nullptr, nullptr, nullptr, nullptr, d_dist, d_nh, d_info},
                     "orh_whatif_run_drains");
}

int orh_whatif_run_metrics(orh_whatif* job, uint32_t n_req, const uint32_t* h_src_idx, const uint32_t* h_ignore_ptr,
                           const uint32_t* h_ignore_links, const uint32_t* h_drain_ptr, const uint32_t* h_drain_nodes,
                           const uint32_t* h_metric_ptr, const orh_whatif_metric* h_metrics, uint32_t* d_dist,
                           uint32_t* d_nh, uint32_t* d_info) {
  return checked_run(job, WhatifRequests{n_req, h_src_idx, h_ignore_ptr, h_ignore_links, h_drain_ptr, h_drain_nodes,
                                         h_metric_ptr, h_metrics, nullptr, nullptr, d_dist, d_nh, d_info},
                     "orh_whatif_run_metrics");
}

int orh_whatif_run_lowers(orh_whatif* job, uint32_t n_req, const uint32_t* h_src_idx, const uint32_t* h_ignore_ptr,
                          const uint32_t* h_ignore_links, const uint32_t* h_drain_ptr, const uint32_t* h_drain_nodes,
                          const uint32_t* h_metric_ptr, const orh_whatif_metric* h_metrics,
                          const uint32_t* h_lower_ptr, const orh_whatif_metric* h_lowers, uint32_t* d_dist,
                          uint32_t* d_nh, uint32_t* d_info) {
  return checked_run(job, WhatifRequests{n_req, h_src_idx, h_ignore_ptr, h_ignore_links, h_drain_ptr, h_drain_nodes,
                                         h_metric_ptr, h_metrics, h_lower_ptr, h_lowers, d_dist, d_nh, d_info},
                     "orh_whatif_run_lowers");
}

int orh_whatif_impact(orh_whatif* job, uint32_t n_req, const uint32_t* h_src_idx, const uint32_t* d_dist,
                      const uint32_t* d_nh, const uint32_t* d_info, const orh_whatif_impact_opts* opts,
                      orh_whatif_impact_rec* d_out) {
  if (!job) return ORH_E_INVALID;
  orh_ctx* ctx = job->g->ctx;
  join_deferred(ctx);
  if (n_req == 0) return ORH_OK;
  const int rc = whatif_summary_check(job, "orh_whatif_impact", h_src_idx, d_dist, d_nh, d_out);
  if (rc) return rc;
  hipSetDevice(ctx->device);
  return whatif_impact(job, n_req, h_src_idx, d_dist, d_nh, d_info, opts, d_out);
}

int orh_whatif_gain(orh_whatif* job, uint32_t n_req, const uint32_t* h_src_idx, const uint32_t* d_dist,
                    const uint32_t* d_nh, const uint32_t* d_info, const orh_whatif_gain_opts* opts,
                    orh_whatif_gain_rec* d_out) {
  if (!job) return ORH_E_INVALID;
  orh_ctx* ctx = job->g->ctx;
  join_deferred(ctx);
  if (n_req == 0) return ORH_OK;
  const int rc = whatif_summary_check(job, "orh_whatif_gain", h_src_idx, d_dist, d_nh, d_out);
  if (rc) return rc;
  hipSetDevice(ctx->device);
  return whatif_gain(job, n_req, h_src_idx, d_dist, d_nh, d_info, opts, d_out);
}

int orh_whatif_refresh(orh_whatif* job) {
  if (!job) return ORH_E_INVALID;
  hipSetDevice(job->g->ctx->device);
  return whatif_base(job);
}

int orh_whatif_flush(orh_whatif* job) {
  if (!job) return ORH_E_INVALID;
  hipSetDevice(job->g->ctx->device);
  return whatif_flush(job);
}

int orh_whatif_elapsed_ms(orh_whatif* job, double* ms_out) {
  if (!job || !ms_out) return ORH_E_INVALID;
  orh_ctx* ctx = job->g->ctx;
  int rc = whatif_flush(job);
  if (rc) return rc;
  ORH_HIP(ctx, hipEventSynchronize(job->ev_end));
  float ms = 0.f;
  ORH_HIP(ctx, hipEventElapsedTime(&ms, job->ev_begin, job->ev_end));
  *ms_out = ms;
  return ORH_OK;
}

int orh_whatif_set_flags(orh_whatif* job, uint32_t flags) {
  if (!job) return ORH_E_INVALID;
  if (flags & ~(ORH_WHATIF_SHARE_BASE | ORH_WHATIF_SEARCH_LARGE))
    return fail(job->g->ctx, ORH_E_INVALID, "orh_whatif_set_flags: unknown flag");
  job->flags = flags;
  return ORH_OK;
}

int orh_whatif_base_rows(orh_whatif* job, const uint32_t** d_dist, const uint32_t** d_nh) {
  if (!job || !d_dist || !d_nh) return ORH_E_INVALID;
  const size_t nd = job->srcs.size() * static_cast<size_t>(job->g->n_nodes);
  *d_dist = job->d_base;
  *d_nh = job->d_base + nd;
  return ORH_OK;
}

int orh_whatif_destroy(orh_whatif* job) {
  if (!job) return ORH_E_INVALID;
  // queued kernels may still read the job's buffers: drain both streams
  if (job->side) {
    whatif_flush(job);
    hipStreamSynchronize(job->side);
  }
  for (hipStream_t t : job->t3)
    if (t) hipStreamSynchronize(t);
  hipStreamSynchronize(job->g->ctx->stream);
  for (hipStream_t t : job->t3)
    if (t) hipStreamDestroy(t);
  auto release = [](StageBuf& b) {
    if (b.ev) {
      hipEventSynchronize(b.ev);
      hipEventDestroy(b.ev);
    }
    if (b.h) hipHostFree(b.h);
    hipFree(b.d);
  };
  for (int c = 0; c < kRunSlots; ++c) {
    RunSlot& r = job->run[c];
    hipFree(r.t3_slots);
    if (r.mid_ev) hipEventDestroy(r.mid_ev);
    hipFree(r.d_work);
    if (r.front_ev) hipEventDestroy(r.front_ev);
    if (r.side_ev) hipEventDestroy(r.side_ev);
    release(r.stage);
    release(job->imp[c]);
  }
  hipFree(job->d_base);
  hipFree(job->own_slots);
  hipFree(job->d_full_lab);
  if (job->g->ctx->slots_owner == job) job->g->ctx->slots_owner = nullptr;
  if (job->side) hipStreamDestroy(job->side);
  if (job->ev_begin) hipEventDestroy(job->ev_begin);
  if (job->ev_end) hipEventDestroy(job->ev_end);
  delete job;
  return ORH_OK;
}

}  // extern "C"
