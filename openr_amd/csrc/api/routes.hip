// The device prefix mirror and route selection, diff and policy.
#include "orh_internal.h"
#include "../kernels/route_kernels.h"

using namespace orh::api;

struct orh_prefix_set {
  orh_ctx* ctx = nullptr;
  // host mirror of the device arrays (compaction and growth)
  std::vector<uint2> hdr;     // {pool offset, count | prefix flags << 16}
  std::vector<orh_adv> pool;  // advertisement runs, appended on update
  uint32_t live = 0;          // records referenced by a header
  uint2* d_hdr = nullptr;
  size_t hdr_cap = 0;
  orh_adv* d_pool = nullptr;
  size_t pool_cap = 0;
  uint32_t* d_rank = nullptr;  // name ranks then area ranks
  size_t rank_cap = 0;
  uint32_t n_names = 0, n_areas = 0;
  orh::SelArea* d_areas = nullptr;
  std::vector<orh::SelArea> h_areas;
  uint32_t* d_stage = nullptr;
  size_t stage_cap = 0;  // in u32
  uint32_t* d_pol = nullptr;  // policy tables (orh_route_policy)
  size_t pol_cap = 0;         // in u32
  std::vector<uint32_t> h_pol;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;  // around the last route_select launch
};

namespace {

int grow(orh_ctx* ctx, void** d, size_t* cap, size_t need, size_t elem, size_t keep) {
  if (need <= *cap) return ORH_OK;
  const size_t ncap = std::max(need, *cap * 2);
  void* nd = nullptr;
  ORH_HIP(ctx, hipMalloc(&nd, ncap * elem));
  if (*d && keep)
    ORH_HIP(ctx, hipMemcpyAsync(nd, *d, keep * elem, hipMemcpyDeviceToDevice, ctx->stream));
  ORH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  (void)hipFree(*d);
  *d = nd;
  *cap = ncap;
  return ORH_OK;
}

int stage(orh_prefix_set* ps, size_t words) {
  return grow(ps->ctx, reinterpret_cast<void**>(&ps->d_stage), &ps->stage_cap, words, 4, 0);
}

// room for a quarter more: the deltas that follow a full load append
// without reallocating (C5: 10k changed prefixes after a 1M-prefix load took
// 30 ms in the host and device pool growth alone)
size_t with_headroom(size_t n) { return n + n / 4 + 1024; }

int upload_all(orh_prefix_set* ps) {
  orh_ctx* ctx = ps->ctx;
  int rc = grow(ctx, reinterpret_cast<void**>(&ps->d_hdr), &ps->hdr_cap, with_headroom(ps->hdr.size()),
                sizeof(uint2), 0);
  if (rc) return rc;
  rc = grow(ctx, reinterpret_cast<void**>(&ps->d_pool), &ps->pool_cap, with_headroom(ps->pool.size()),
            sizeof(orh_adv), 0);
  if (rc) return rc;
  if (!ps->hdr.empty())
    ORH_HIP(ctx, hipMemcpyAsync(ps->d_hdr, ps->hdr.data(), ps->hdr.size() * sizeof(uint2),
                                hipMemcpyHostToDevice, ctx->stream));
  if (!ps->pool.empty())
    ORH_HIP(ctx, hipMemcpyAsync(ps->d_pool, ps->pool.data(), ps->pool.size() * sizeof(orh_adv),
                                hipMemcpyHostToDevice, ctx->stream));
  ORH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ORH_OK;
}

}  // namespace

extern "C" {

int orh_prefix_create(orh_ctx* ctx, orh_prefix_set** out) {
  if (!ctx || !out) return ORH_E_INVALID;
  auto* ps = new (std::nothrow) orh_prefix_set();
  if (!ps) return ORH_E_NOMEM;
  ps->ctx = ctx;
  *out = ps;
  return ORH_OK;
}

int orh_prefix_destroy(orh_prefix_set* ps) {
  if (!ps) return ORH_E_INVALID;
  hipSetDevice(ps->ctx->device);
  hipStreamSynchronize(ps->ctx->stream);
  hipFree(ps->d_hdr);
  hipFree(ps->d_pool);
  hipFree(ps->d_rank);
  hipFree(ps->d_areas);
  hipFree(ps->d_stage);
  hipFree(ps->d_pol);
  if (ps->ev0) hipEventDestroy(ps->ev0);
  if (ps->ev1) hipEventDestroy(ps->ev1);
  delete ps;
  return ORH_OK;
}

int orh_prefix_load(orh_prefix_set* ps, uint32_t n_prefix, const uint32_t* adv_ptr,
                    const orh_adv* advs, const uint8_t* pflags) {
  if (!ps || (n_prefix && (!adv_ptr || !pflags))) return ORH_E_INVALID;
  orh_ctx* ctx = ps->ctx;
  const uint32_t n_adv = n_prefix ? adv_ptr[n_prefix] : 0;
  if (n_adv && !advs) return fail(ctx, ORH_E_INVALID, "orh_prefix_load: null advertisements");
  for (uint32_t p = 0; p < n_prefix; ++p)
    if (adv_ptr[p + 1] < adv_ptr[p] || adv_ptr[p + 1] - adv_ptr[p] > 0xFFFFu)
      return fail(ctx, ORH_E_INVALID, "orh_prefix_load: bad adv_ptr / > 65535 advertisements");
  ORH_HIP(ctx, hipSetDevice(ctx->device));
  ps->hdr.reserve(with_headroom(n_prefix));
  ps->hdr.resize(n_prefix);
  for (uint32_t p = 0; p < n_prefix; ++p)
    ps->hdr[p] = make_uint2(adv_ptr[p], (adv_ptr[p + 1] - adv_ptr[p]) | (uint32_t(pflags[p]) << 16));
  ps->pool.reserve(with_headroom(n_adv));
  ps->pool.assign(advs, advs + n_adv);
  ps->live = n_adv;
  return upload_all(ps);
}

int orh_prefix_apply_delta(orh_prefix_set* ps, uint32_t n, const uint32_t* ids,
                           const uint32_t* adv_ptr, const orh_adv* advs, const uint8_t* pflags) {
  if (!ps || (n && (!ids || !adv_ptr || !pflags))) return ORH_E_INVALID;
  if (n == 0) return ORH_OK;
  orh_ctx* ctx = ps->ctx;
  const uint32_t n_adv = adv_ptr[n];
  if (n_adv && !advs) return fail(ctx, ORH_E_INVALID, "orh_prefix_apply_delta: null advertisements");
  ORH_HIP(ctx, hipSetDevice(ctx->device));
  uint32_t max_id = 0;
  for (uint32_t i = 0; i < n; ++i) {
    if (adv_ptr[i + 1] < adv_ptr[i] || adv_ptr[i + 1] - adv_ptr[i] > 0xFFFFu)
      return fail(ctx, ORH_E_INVALID, "orh_prefix_apply_delta: bad adv_ptr");
    max_id = std::max(max_id, ids[i]);
  }
  const size_t old_n = ps->hdr.size();
  if (max_id >= old_n) ps->hdr.resize(static_cast<size_t>(max_id) + 1, make_uint2(0u, 0u));
  const uint32_t base = static_cast<uint32_t>(ps->pool.size());
  bool ascending = true;
  for (uint32_t i = 0; i < n; ++i) {
    uint2& h = ps->hdr[ids[i]];
    ps->live -= h.y & 0xFFFFu;
    const uint32_t c = adv_ptr[i + 1] - adv_ptr[i];
    h = make_uint2(base + adv_ptr[i], c | (uint32_t(pflags[i]) << 16));
    ps->live += c;
    ascending &= i == 0 || ids[i - 1] < ids[i];
  }
  // an id given more than once keeps its last list (the mirror above already
  // does): the scatter writes each id once, so no two threads race on a header
  std::vector<uint32_t> uniq(ids, ids + n);
  if (!ascending) {
    std::sort(uniq.begin(), uniq.end());
    uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
  }
  const uint32_t n_set = static_cast<uint32_t>(uniq.size());
  std::vector<uint2> vals(n_set);
  for (uint32_t i = 0; i < n_set; ++i) vals[i] = ps->hdr[uniq[i]];
  ps->pool.insert(ps->pool.end(), advs, advs + n_adv);
  // mostly garbage: rebuild the pool from the live runs and re-upload
  if (ps->pool.size() > 4096 && ps->pool.size() > 2 * static_cast<size_t>(ps->live)) {
    std::vector<orh_adv> packed;
    packed.reserve(with_headroom(ps->live));
    for (auto& h : ps->hdr) {
      const uint32_t c = h.y & 0xFFFFu;
      const uint32_t off = static_cast<uint32_t>(packed.size());
      packed.insert(packed.end(), ps->pool.begin() + h.x, ps->pool.begin() + h.x + c);
      h.x = off;
    }
    ps->pool.swap(packed);
    return upload_all(ps);
  }
  int rc = grow(ctx, reinterpret_cast<void**>(&ps->d_hdr), &ps->hdr_cap, ps->hdr.size(),
                sizeof(uint2), old_n);
  if (rc) return rc;
  if (ps->hdr.size() > old_n)  // new ids start withdrawn
    ORH_HIP(ctx, hipMemsetAsync(ps->d_hdr + old_n, 0, (ps->hdr.size() - old_n) * sizeof(uint2),
                                ctx->stream));
  rc = grow(ctx, reinterpret_cast<void**>(&ps->d_pool), &ps->pool_cap, std::max<size_t>(ps->pool.size(), 1),
            sizeof(orh_adv), base);
  if (rc) return rc;
  if (n_adv)
    ORH_HIP(ctx, hipMemcpyAsync(ps->d_pool + base, advs, static_cast<size_t>(n_adv) * sizeof(orh_adv),
                                hipMemcpyHostToDevice, ctx->stream));
  // staging: ids[n] (padded to 8 bytes) | headers[n]
  const size_t id_words = (n_set + 1) & ~1u;
  std::vector<uint32_t> st(id_words + 2 * static_cast<size_t>(n_set));
  std::copy(uniq.begin(), uniq.end(), st.begin());
  std::memcpy(st.data() + id_words, vals.data(), n_set * sizeof(uint2));
  rc = stage(ps, st.size());
  if (rc) return rc;
  ORH_HIP(ctx, hipMemcpyAsync(ps->d_stage, st.data(), st.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  ORH_HIP(ctx, orh::launch_scatter_hdr(ps->d_hdr, ps->d_stage,
                                       reinterpret_cast<const uint2*>(ps->d_stage + id_words), n_set,
                                       ctx->stream));
  ORH_HIP(ctx, hipStreamSynchronize(ctx->stream));  // st is a local
  return ORH_OK;
}

int orh_prefix_set_order(orh_prefix_set* ps, uint32_t n_names, const uint32_t* name_rank,
                         uint32_t n_areas, const uint32_t* area_rank) {
  if (!ps || (n_names && !name_rank) || (n_areas && !area_rank)) return ORH_E_INVALID;
  orh_ctx* ctx = ps->ctx;
  if (n_areas > 256) return fail(ctx, ORH_E_UNSUPPORTED, "orh_prefix_set_order: more than 256 areas");
  ORH_HIP(ctx, hipSetDevice(ctx->device));
  const size_t words = static_cast<size_t>(n_names) + 256;
  int rc = grow(ctx, reinterpret_cast<void**>(&ps->d_rank), &ps->rank_cap, words, 4, 0);
  if (rc) return rc;
  std::vector<uint32_t> r(words, 0xFFFFFFFFu);
  std::copy(name_rank, name_rank + n_names, r.begin());
  std::copy(area_rank, area_rank + n_areas, r.begin() + n_names);
  ORH_HIP(ctx, hipMemcpyAsync(ps->d_rank, r.data(), words * 4, hipMemcpyHostToDevice, ctx->stream));
  ORH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ps->n_names = n_names;
  ps->n_areas = n_areas;
  return ORH_OK;
}

int orh_prefix_info(const orh_prefix_set* ps, uint32_t* n_prefix, uint32_t* n_live, uint32_t* n_pool) {
  if (!ps) return ORH_E_INVALID;
  if (n_prefix) *n_prefix = static_cast<uint32_t>(ps->hdr.size());
  if (n_live) *n_live = ps->live;
  if (n_pool) *n_pool = static_cast<uint32_t>(ps->pool.size());
  return ORH_OK;
}

int orh_route_select(orh_prefix_set* ps, uint32_t me_name, uint32_t flags, uint32_t n_areas,
                     const orh_select_area* areas, const orh_select_out* out) {
  if (!ps) return ORH_E_INVALID;
  return orh_route_select_range(ps, me_name, flags, n_areas, areas, 0, static_cast<uint32_t>(ps->hdr.size()), out);
}

int orh_route_select_range(orh_prefix_set* ps, uint32_t me_name, uint32_t flags, uint32_t n_areas,
                           const orh_select_area* areas, uint32_t pid_lo, uint32_t pid_hi,
                           const orh_select_out* out) {
  if (!ps || !out || (n_areas && !areas)) return ORH_E_INVALID;
  orh_ctx* ctx = ps->ctx;
  join_deferred(ctx);
  if (pid_lo > pid_hi || pid_hi > ps->hdr.size())
    return fail(ctx, ORH_E_INVALID, "orh_route_select_range: range beyond the prefix set");
  const uint32_t n_prefix = pid_hi;
  if (pid_lo == pid_hi) return ORH_OK;
  if (n_areas > orh::kMaxSelectAreas)
    return fail(ctx, ORH_E_UNSUPPORTED, "orh_route_select: more than 32 areas");
  if (!out->d_status || !out->d_metric || !out->d_best || (out->total_words && !out->d_mask))
    return fail(ctx, ORH_E_INVALID, "orh_route_select: null output");
  if (!ps->d_rank) return fail(ctx, ORH_E_STATE, "orh_route_select: orh_prefix_set_order not called");
  uint32_t words = 0;
  for (uint32_t b = 0; b < n_areas; ++b) {
    const orh_select_area& A = areas[b];
    if (A.d_dist && (!A.d_nh || !A.d_overloaded || !A.d_name_node || A.words == 0))
      return fail(ctx, ORH_E_INVALID, "orh_route_select: incomplete area");
    if (A.word_off + A.words > out->total_words)
      return fail(ctx, ORH_E_INVALID, "orh_route_select: area words exceed total_words");
    words += A.words;
  }
  ORH_HIP(ctx, hipSetDevice(ctx->device));
  if (!ps->d_areas) ORH_HIP(ctx, hipMalloc(&ps->d_areas, orh::kMaxSelectAreas * sizeof(orh::SelArea)));
  ps->h_areas.assign(orh::kMaxSelectAreas, orh::SelArea{});
  for (uint32_t b = 0; b < n_areas; ++b)
    ps->h_areas[b] = orh::SelArea{areas[b].present, areas[b].d_dist, areas[b].d_nh, areas[b].d_overloaded,
                                  areas[b].d_name_node, areas[b].words, areas[b].word_off};
  ORH_HIP(ctx, hipMemcpyAsync(ps->d_areas, ps->h_areas.data(), n_areas * sizeof(orh::SelArea),
                              hipMemcpyHostToDevice, ctx->stream));
  orh::RouteSelectArgs a{};
  a.pid_lo = pid_lo;
  a.n_prefix = n_prefix;
  a.hdr = ps->d_hdr;
  a.adv = ps->d_pool;
  a.name_rank = ps->d_rank;
  a.area_rank = ps->d_rank + ps->n_names;
  a.n_names = ps->n_names;
  a.me_name = me_name;
  a.flags = flags;
  a.n_areas = n_areas;
  a.areas = ps->d_areas;
  a.status = out->d_status;
  a.metric = out->d_metric;
  a.best = out->d_best;
  a.mask = out->d_mask;
  a.total_words = out->total_words;
  if (!ps->ev0) {
    ORH_HIP(ctx, hipEventCreate(&ps->ev0));
    ORH_HIP(ctx, hipEventCreate(&ps->ev1));
  }
  ORH_HIP(ctx, hipEventRecord(ps->ev0, ctx->stream));
  hipError_t e = orh::launch_route_select(a, ctx->stream);
  if (e != hipSuccess) return hip_fail(ctx, e, "route_select launch");
  ORH_HIP(ctx, hipEventRecord(ps->ev1, ctx->stream));
  (void)words;
  return ORH_OK;
}

int orh_route_diff(orh_prefix_set* ps, uint32_t n_prefix, uint32_t prev_n, const orh_select_out* cur,
                   const orh_select_out* prev, uint32_t* d_changed, uint32_t* d_count) {
  if (!ps || !cur || !prev || !d_changed || !d_count) return ORH_E_INVALID;
  orh_ctx* ctx = ps->ctx;
  if (cur->total_words != prev->total_words)
    return fail(ctx, ORH_E_INVALID, "orh_route_diff: different mask widths");
  if (!cur->d_status || !cur->d_metric || !cur->d_best || !prev->d_status || !prev->d_metric || !prev->d_best ||
      (cur->total_words && (!cur->d_mask || !prev->d_mask)))
    return fail(ctx, ORH_E_INVALID, "orh_route_diff: null selection output");
  ORH_HIP(ctx, hipSetDevice(ctx->device));
  ORH_HIP(ctx, hipMemsetAsync(d_count, 0, sizeof(uint32_t), ctx->stream));
  orh::RouteDiffArgs a{};
  a.n_prefix = n_prefix;
  a.prev_n = std::min(prev_n, n_prefix);
  a.words = cur->total_words;
  a.status = cur->d_status;
  a.metric = cur->d_metric;
  a.best = cur->d_best;
  a.mask = cur->d_mask;
  a.p_status = prev->d_status;
  a.p_metric = prev->d_metric;
  a.p_best = prev->d_best;
  a.p_mask = prev->d_mask;
  a.out = d_changed;
  a.count = d_count;
  hipError_t e = orh::launch_route_diff(a, ctx->stream);
  if (e != hipSuccess) return hip_fail(ctx, e, "route_diff launch");
  return ORH_OK;
}

int orh_route_policy(orh_prefix_set* ps, uint32_t n_prefix, const orh_select_out* sel,
                     const orh_policy* pol, uint8_t* d_out, uint32_t* d_invalidated) {
  return orh_route_policy_range(ps, 0, n_prefix, sel, pol, d_out, d_invalidated);
}

int orh_route_policy_range(orh_prefix_set* ps, uint32_t pid_lo, uint32_t n_prefix, const orh_select_out* sel,
                           const orh_policy* pol, uint8_t* d_out, uint32_t* d_invalidated) {
  if (!ps || !sel || !pol || !d_out || !d_invalidated) return ORH_E_INVALID;
  orh_ctx* ctx = ps->ctx;
  if (pol->n_stmts > ORH_POL_MAX_STMTS)
    return fail(ctx, ORH_E_UNSUPPORTED, "orh_route_policy: more than 32 statements");
  if (n_prefix > ps->hdr.size() || pid_lo > n_prefix)
    return fail(ctx, ORH_E_INVALID, "orh_route_policy: prefix range beyond the set");
  if (pol->total_words != sel->total_words)
    return fail(ctx, ORH_E_INVALID, "orh_route_policy: mask widths differ");
  if (!sel->d_status || !sel->d_best || (sel->total_words && !sel->d_mask) ||
      (pol->n_tagsets && !pol->h_tagset_stmts) || (pol->n_pfx && (!pol->h_pfx_id || !pol->h_pfx_stmts)) ||
      (pol->n_stmts && pol->total_words && !pol->h_keep))
    return fail(ctx, ORH_E_INVALID, "orh_route_policy: null table");
  for (uint32_t i = 1; i < pol->n_pfx; ++i)
    if (pol->h_pfx_id[i] <= pol->h_pfx_id[i - 1])
      return fail(ctx, ORH_E_INVALID, "orh_route_policy: prefix ids not ascending");
  ORH_HIP(ctx, hipSetDevice(ctx->device));
  // a previous launch may still read the device tables, and its upload the
  // host staging: the context stream drains before either is reused
  ORH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  // one upload: tag-set table | prefix ids | prefix statements | keep masks
  const size_t nk = static_cast<size_t>(pol->n_stmts) * pol->total_words;
  auto& h = ps->h_pol;
  h.clear();
  h.reserve(pol->n_tagsets + 2ull * pol->n_pfx + nk + 1);
  h.insert(h.end(), pol->h_tagset_stmts, pol->h_tagset_stmts + pol->n_tagsets);
  h.insert(h.end(), pol->h_pfx_id, pol->h_pfx_id + pol->n_pfx);
  h.insert(h.end(), pol->h_pfx_stmts, pol->h_pfx_stmts + pol->n_pfx);
  if (nk) h.insert(h.end(), pol->h_keep, pol->h_keep + nk);
  h.push_back(0u);
  int rc = grow(ctx, reinterpret_cast<void**>(&ps->d_pol), &ps->pol_cap, h.size(), 4, 0);
  if (rc) return rc;
  ORH_HIP(ctx, hipMemcpyAsync(ps->d_pol, h.data(), h.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  ORH_HIP(ctx, hipMemsetAsync(d_invalidated, 0, sizeof(uint32_t), ctx->stream));
  orh::RoutePolicyArgs a{};
  a.pid_lo = pid_lo;
  a.n_prefix = n_prefix;
  a.words = sel->total_words;
  a.hdr = ps->d_hdr;
  a.adv = ps->d_pool;
  a.status = sel->d_status;
  a.best = sel->d_best;
  a.mask = sel->d_mask;
  a.n_stmts = pol->n_stmts;
  a.stmt_tags = pol->stmt_tags;
  a.stmt_pfx = pol->stmt_prefixes;
  a.n_tagsets = pol->n_tagsets;
  a.tagset_stmts = ps->d_pol;
  a.n_pfx = pol->n_pfx;
  a.pfx_id = ps->d_pol + pol->n_tagsets;
  a.pfx_stmts = a.pfx_id + pol->n_pfx;
  a.keep = a.pfx_stmts + pol->n_pfx;
  a.out = d_out;
  a.invalidated = d_invalidated;
  hipError_t e = orh::launch_route_policy(a, ctx->stream);
  if (e != hipSuccess) return hip_fail(ctx, e, "route_policy launch");
  return ORH_OK;
}

int orh_last_select_ms(orh_prefix_set* ps, double* ms_out) {
  if (!ps || !ms_out) return ORH_E_INVALID;
  if (!ps->ev1) return fail(ps->ctx, ORH_E_STATE, "orh_last_select_ms: no route_select yet");
  ORH_HIP(ps->ctx, hipEventSynchronize(ps->ev1));
  float ms = 0.f;
  ORH_HIP(ps->ctx, hipEventElapsedTime(&ms, ps->ev0, ps->ev1));
  *ms_out = ms;
  return ORH_OK;
}

}  // extern "C"
