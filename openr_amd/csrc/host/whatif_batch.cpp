// WhatIfBatch: see whatif_batch.h.
#include "whatif_batch.h"

#include <algorithm>
#include <stdexcept>

namespace openr_amd {

namespace {

void check(orh_ctx* ctx, int rc, const char* what) {
  if (rc != ORH_OK)
    throw std::runtime_error(std::string("WhatIfBatch: ") + what + " failed (" + std::to_string(rc) +
                             "): " + (ctx ? orh_last_error(ctx) : ""));
}

}  // namespace

WhatIfBatch::WhatIfBatch(const LinkState& ls, const std::vector<std::string>& srcs,
                         const std::vector<uint32_t>& srcIdx, const std::vector<std::vector<uint32_t>>& ignore,
                         uint32_t chunk, bool useLinkMetric, bool shareBase, bool searchLarge,
                         const std::vector<std::vector<std::string>>& drain,
                         const std::vector<std::vector<WhatIfMetricRaise>>& metric,
                         const std::vector<std::vector<WhatIfMetricLower>>& lower)
    : ls_(ls), useLinkMetric_(useLinkMetric), shareBase_(shareBase), searchLarge_(searchLarge) {
  if (srcIdx.size() != ignore.size()) throw std::invalid_argument("WhatIfBatch: one ignore set per request");
  if (!drain.empty() && drain.size() != srcIdx.size())
    throw std::invalid_argument("WhatIfBatch: one drain set per request (or none at all)");
  std::vector<std::vector<uint32_t>> drainIds(drain.size());
  for (size_t i = 0; i < drain.size(); ++i)
    for (const auto& name : drain[i]) {
      auto id = ls.nodeId(name);
      if (!id) throw std::invalid_argument("WhatIfBatch: unknown drained node " + name);
      drainIds[i].push_back(*id);
      drains_ = true;
    }
  if (!metric.empty() && metric.size() != srcIdx.size())
    throw std::invalid_argument("WhatIfBatch: one list of metric raises per request (or none at all)");
  if (!lower.empty() && lower.size() != srcIdx.size())
    throw std::invalid_argument("WhatIfBatch: one list of metric lowers per request (or none at all)");
  // a list of metric changes by node id; *any: some request has one
  auto resolve = [&](const std::vector<std::vector<WhatIfMetricRaise>>& in, const char* what, bool* any) {
    std::vector<std::vector<orh_whatif_metric>> ids(in.size());
    for (size_t i = 0; i < in.size(); ++i)
      for (const auto& mr : in[i]) {
        uint32_t from = ORH_NO_NODE;
        if (!mr.from.empty()) {
          auto id = ls.nodeId(mr.from);
          if (!id) throw std::invalid_argument("WhatIfBatch: unknown node " + mr.from + " in a metric " + what);
          from = *id;
        }
        ids[i].push_back({mr.link, from, mr.metric});
        *any = true;
      }
    return ids;
  };
  const auto raiseIds = resolve(metric, "raise", &raises_);
  const auto lowerIds = resolve(lower, "lower", &lowers_);
  if (chunk == 0) throw std::invalid_argument("WhatIfBatch: chunk must be positive");
  for (const auto& s : srcs) {
    auto id = ls.nodeId(s);
    if (!id) throw std::invalid_argument("WhatIfBatch: unknown source " + s);
    srcs_.push_back(*id);
  }
  for (uint32_t i : srcIdx)
    if (i >= srcs_.size()) throw std::invalid_argument("WhatIfBatch: source index out of range");
  srcIdx_ = srcIdx;
  // per chunk: the ignore CSR rebased to the chunk
  const size_t n = srcIdx.size();
  chunk_ = static_cast<uint32_t>(std::min<size_t>(chunk, std::max<size_t>(n, 1)));
  for (size_t c0 = 0; c0 < n; c0 += chunk_) {
    const size_t c1 = std::min(n, c0 + chunk_);
    std::vector<uint32_t> ptr{0}, links, dptr, dnodes, mptr, lptr;
    std::vector<orh_whatif_metric> mets, lows;
    for (size_t i = c0; i < c1; ++i) {
      links.insert(links.end(), ignore[i].begin(), ignore[i].end());
      ptr.push_back(static_cast<uint32_t>(links.size()));
    }
    if (links.empty()) links.push_back(0);  // non-null pointer
    if (drains_) {
      dptr.push_back(0);
      for (size_t i = c0; i < c1; ++i) {
        dnodes.insert(dnodes.end(), drainIds[i].begin(), drainIds[i].end());
        dptr.push_back(static_cast<uint32_t>(dnodes.size()));
      }
      if (dnodes.empty()) dnodes.push_back(0);
    }
    if (raises_) {
      mptr.push_back(0);
      for (size_t i = c0; i < c1; ++i) {
        mets.insert(mets.end(), raiseIds[i].begin(), raiseIds[i].end());
        mptr.push_back(static_cast<uint32_t>(mets.size()));
      }
      if (mets.empty()) mets.push_back({0u, ORH_NO_NODE, 0u});
    }
    if (lowers_) {
      lptr.push_back(0);
      for (size_t i = c0; i < c1; ++i) {
        lows.insert(lows.end(), lowerIds[i].begin(), lowerIds[i].end());
        lptr.push_back(static_cast<uint32_t>(lows.size()));
      }
      if (lows.empty()) lows.push_back({0u, ORH_NO_NODE, 0u});
    }
    chunks_.push_back({c0, c1, std::move(ptr), std::move(links), std::move(dptr), std::move(dnodes),
                       std::move(mptr), std::move(mets), std::move(lptr), std::move(lows)});
  }
  graph_ = ls.deviceGraph();
  ctx_ = ls.context();
  check(ctx_, orh_graph_info(graph_, &n_, &edges_), "orh_graph_info");
  check(ctx_, orh_device_alloc(ctx_, std::max<size_t>(n, 1) * 4, reinterpret_cast<void**>(&dInfo_)),
        "orh_device_alloc");
  allocate();
}

void WhatIfBatch::allocate() {
  if (nBuf_) return;
  const size_t rows = static_cast<size_t>(chunk_) * n_;
  const int want = static_cast<int>(std::max<size_t>(1, std::min<size_t>(chunks_.size(), kBufs)));
  for (int b = 0; b < want; ++b) {
    if (orh_device_alloc(ctx_, rows * 4, reinterpret_cast<void**>(&dDist_[b])) != ORH_OK ||
        orh_device_alloc(ctx_, rows * 4, reinterpret_cast<void**>(&dNh_[b])) != ORH_OK) {
      nBuf_ = b + 1;
      release();
      throw std::runtime_error("WhatIfBatch: device allocation failed (" + std::to_string(rows * 8) +
                               " bytes of rows per buffer)");
    }
    nBuf_ = b + 1;
  }
}

void WhatIfBatch::freeImpact() {
  if (dImpact_) orh_device_free(ctx_, dImpact_);
  if (dWeight_) orh_device_free(ctx_, dWeight_);
  if (dNodeLost_) orh_device_free(ctx_, dNodeLost_);
  if (dNodeMoved_) orh_device_free(ctx_, dNodeMoved_);
  if (dGain_) orh_device_free(ctx_, dGain_);
  if (dNodeNearer_) orh_device_free(ctx_, dNodeNearer_);
  dImpact_ = nullptr;
  dGain_ = nullptr;
  dWeight_ = dNodeLost_ = dNodeMoved_ = dNodeNearer_ = nullptr;
}

void WhatIfBatch::release() {
  if (impactRan_ && dImpact_) {  // the last run's summaries outlive the buffers
    hImpact_.resize(srcIdx_.size());
    impact(hImpact_.data());
    if (nodeCounts_ && dNodeLost_) {
      hNodeLost_.resize(n_);
      hNodeMoved_.resize(n_);
      nodeImpact(hNodeLost_.data(), hNodeMoved_.data());
    }
  }
  if (gainRan_ && dGain_) {
    hGain_.resize(srcIdx_.size());
    gain(hGain_.data());
    if (nodeCounts_ && dNodeNearer_) {
      hNodeLost_.resize(n_);
      hNodeMoved_.resize(n_);
      hNodeNearer_.resize(n_);
      nodeGain(hNodeLost_.data(), hNodeMoved_.data(), hNodeNearer_.data());
    }
  }
  freeImpact();
  if (job_) {
    orh_whatif_destroy(job_);
    job_ = nullptr;
  }
  for (int b = 0; b < nBuf_; ++b) {
    if (dDist_[b]) orh_device_free(ctx_, dDist_[b]);
    if (dNh_[b]) orh_device_free(ctx_, dNh_[b]);
    dDist_[b] = dNh_[b] = nullptr;
  }
  nBuf_ = 0;
}

WhatIfBatch::~WhatIfBatch() {
  impactRan_ = gainRan_ = false;  // nothing to keep
  release();
  if (dInfo_) orh_device_free(ctx_, dInfo_);
  if (dDigest_) orh_device_free(ctx_, dDigest_);
  if (dBaseDigest_) orh_device_free(ctx_, dBaseDigest_);
}

void WhatIfBatch::setDigests(bool on) {
  digests_ = on;
  if (!on || dDigest_) return;
  check(ctx_, orh_device_alloc(ctx_, std::max<size_t>(srcIdx_.size(), 1) * 8, reinterpret_cast<void**>(&dDigest_)),
        "orh_device_alloc");
  check(ctx_, orh_device_alloc(ctx_, std::max<size_t>(srcs_.size(), 1) * 8, reinterpret_cast<void**>(&dBaseDigest_)),
        "orh_device_alloc");
}

void WhatIfBatch::setImpact(bool on, const std::vector<std::pair<std::string, uint32_t>>& weights,
                            bool nodeCounts) {
  setSummary(&impact_, gain_, on, weights, nodeCounts);
}

void WhatIfBatch::setGain(bool on, const std::vector<std::pair<std::string, uint32_t>>& weights, bool nodeCounts) {
  setSummary(&gain_, impact_, on, weights, nodeCounts);
}

// one summary mode switched on or off; the weights and the node-count flag
// belong to whichever mode is on, so switching one off leaves them alone while
// the other is on
void WhatIfBatch::setSummary(bool* mode, bool other, bool on,
                             const std::vector<std::pair<std::string, uint32_t>>& weights, bool nodeCounts) {
  if (!on && other) {
    *mode = false;
    return;
  }
  std::vector<uint32_t> w;
  if (on && !weights.empty()) {
    w.assign(n_, 0u);
    for (const auto& [name, x] : weights) {
      auto id = ls_.nodeId(name);
      if (!id || *id >= n_) throw std::invalid_argument("WhatIfBatch: unknown weighted node " + name);
      w[*id] = x;
    }
  }
  *mode = on;
  nodeCounts_ = on && nodeCounts;
  weights_ = std::move(w);
  if (dWeight_) {  // the next run uploads the new ones
    orh_device_free(ctx_, dWeight_);
    dWeight_ = nullptr;
  }
}

// chunk c's rows, still in buffer c % nBuf_, into its requests' records
void WhatIfBatch::queueImpact(size_t c) {
  const Chunk& ch = chunks_[c];
  const int b = static_cast<int>(c % nBuf_);
  if (gain_) {
    orh_whatif_gain_opts opts{};
    opts.d_weight = weights_.empty() ? nullptr : dWeight_;
    opts.d_node_lost = nodeCounts_ ? dNodeLost_ : nullptr;
    opts.d_node_moved = nodeCounts_ ? dNodeMoved_ : nullptr;
    opts.d_node_nearer = nodeCounts_ ? dNodeNearer_ : nullptr;
    check(ctx_,
          orh_whatif_gain(job_, static_cast<uint32_t>(ch.hi - ch.lo), srcIdx_.data() + ch.lo, dDist_[b], dNh_[b],
                          dInfo_ + ch.lo, &opts, dGain_ + ch.lo),
          "orh_whatif_gain");
    return;
  }
  orh_whatif_impact_opts opts{};
  opts.d_weight = weights_.empty() ? nullptr : dWeight_;
  opts.d_node_lost = nodeCounts_ ? dNodeLost_ : nullptr;
  opts.d_node_moved = nodeCounts_ ? dNodeMoved_ : nullptr;
  check(ctx_,
        orh_whatif_impact(job_, static_cast<uint32_t>(ch.hi - ch.lo), srcIdx_.data() + ch.lo, dDist_[b], dNh_[b],
                          dInfo_ + ch.lo, &opts, dImpact_ + ch.lo),
        "orh_whatif_impact");
}

void WhatIfBatch::impact(orh_whatif_impact_rec* out) const {
  if (!impactRan_) throw std::logic_error("WhatIfBatch: impact was not enabled for the last run");
  if (dImpact_)
    check(ctx_, orh_memcpy_d2h(ctx_, out, dImpact_, srcIdx_.size() * sizeof(orh_whatif_impact_rec)),
          "orh_memcpy_d2h");
  else
    std::copy(hImpact_.begin(), hImpact_.end(), out);
}

void WhatIfBatch::nodeImpact(uint32_t* lost, uint32_t* moved) const {
  if (!impactRan_ || !nodeCounts_)
    throw std::logic_error("WhatIfBatch: node counts were not enabled for the last run");
  if (dNodeLost_) {
    check(ctx_, orh_memcpy_d2h(ctx_, lost, dNodeLost_, n_ * 4ull), "orh_memcpy_d2h");
    check(ctx_, orh_memcpy_d2h(ctx_, moved, dNodeMoved_, n_ * 4ull), "orh_memcpy_d2h");
  } else {
    std::copy(hNodeLost_.begin(), hNodeLost_.end(), lost);
    std::copy(hNodeMoved_.begin(), hNodeMoved_.end(), moved);
  }
}

void WhatIfBatch::gain(orh_whatif_gain_rec* out) const {
  if (!gainRan_) throw std::logic_error("WhatIfBatch: gain was not enabled for the last run");
  if (dGain_)
    check(ctx_, orh_memcpy_d2h(ctx_, out, dGain_, srcIdx_.size() * sizeof(orh_whatif_gain_rec)), "orh_memcpy_d2h");
  else
    std::copy(hGain_.begin(), hGain_.end(), out);
}

void WhatIfBatch::nodeGain(uint32_t* lost, uint32_t* moved, uint32_t* nearer) const {
  if (!gainRan_ || !nodeCounts_)
    throw std::logic_error("WhatIfBatch: node counts were not enabled for the last run");
  if (dNodeNearer_) {
    check(ctx_, orh_memcpy_d2h(ctx_, lost, dNodeLost_, n_ * 4ull), "orh_memcpy_d2h");
    check(ctx_, orh_memcpy_d2h(ctx_, moved, dNodeMoved_, n_ * 4ull), "orh_memcpy_d2h");
    check(ctx_, orh_memcpy_d2h(ctx_, nearer, dNodeNearer_, n_ * 4ull), "orh_memcpy_d2h");
  } else {
    std::copy(hNodeLost_.begin(), hNodeLost_.end(), lost);
    std::copy(hNodeMoved_.begin(), hNodeMoved_.end(), moved);
    std::copy(hNodeNearer_.begin(), hNodeNearer_.end(), nearer);
  }
}

void WhatIfBatch::run() {
  impactRan_ = gainRan_ = false;
  if (impact_ && gain_)
    throw std::invalid_argument("WhatIfBatch: impact and gain summaries are two modes of one pass, enable one");
  if (impact_ && lowers_)  // the summary's classes assume that no node gets nearer
    throw std::invalid_argument(
        "WhatIfBatch: impact summaries do not cover requests that lower metrics (gain summaries do: setGain)");
  if (impact_ || gain_) {  // buffers of the mode; the node counters start at zero (before the job's clock)
    auto alloc = [&](auto** p, size_t bytes) {
      if (!*p) check(ctx_, orh_device_alloc(ctx_, std::max<size_t>(bytes, 8), reinterpret_cast<void**>(p)),
                     "orh_device_alloc");
    };
    if (impact_) alloc(&dImpact_, srcIdx_.size() * sizeof(orh_whatif_impact_rec));
    else alloc(&dGain_, srcIdx_.size() * sizeof(orh_whatif_gain_rec));
    if (!weights_.empty() && !dWeight_) {
      alloc(&dWeight_, n_ * 4ull);
      check(ctx_, orh_memcpy_h2d(ctx_, dWeight_, weights_.data(), n_ * 4ull), "orh_memcpy_h2d");
    }
    if (nodeCounts_) {
      alloc(&dNodeLost_, n_ * 4ull);
      alloc(&dNodeMoved_, n_ * 4ull);
      const std::vector<uint32_t> zero(n_, 0u);
      check(ctx_, orh_memcpy_h2d(ctx_, dNodeLost_, zero.data(), n_ * 4ull), "orh_memcpy_h2d");
      check(ctx_, orh_memcpy_h2d(ctx_, dNodeMoved_, zero.data(), n_ * 4ull), "orh_memcpy_h2d");
      if (gain_) {
        alloc(&dNodeNearer_, n_ * 4ull);
        check(ctx_, orh_memcpy_h2d(ctx_, dNodeNearer_, zero.data(), n_ * 4ull), "orh_memcpy_h2d");
      }
    }
  }
  // the graph as it is now: a what-if job is bound to its graph's structure
  // (orh_whatif_run fails with ORH_E_STATE after a delta or reload)
  {
    uint32_t n = 0, e = 0;
    check(ctx_, orh_graph_info(ls_.deviceGraph(), &n, &e), "orh_graph_info");  // flushes pending deltas
    if (n != n_)
      throw std::runtime_error("WhatIfBatch: the topology's node count changed (" + std::to_string(n_) + " -> " +
                               std::to_string(n) + "): rows are sized for the old one, make a new batch");
    edges_ = e;
  }
  allocate();
  if (job_ && ls_.stateStamp() != stamp_) {  // the LinkState changed: a job on the graph as it is now
    orh_whatif_destroy(job_);
    job_ = nullptr;
  }
  if (!job_) {
    stamp_ = ls_.stateStamp();
    check(ctx_, orh_whatif_create(graph_, srcs_.data(), static_cast<uint32_t>(srcs_.size()), useLinkMetric_ ? 1 : 0,
                                  &job_),
          "orh_whatif_create");
    const uint32_t fl = (shareBase_ ? ORH_WHATIF_SHARE_BASE : 0u) | (searchLarge_ ? ORH_WHATIF_SEARCH_LARGE : 0u);
    if (fl) check(ctx_, orh_whatif_set_flags(job_, fl), "orh_whatif_set_flags");
  } else {
    check(ctx_, orh_whatif_refresh(job_), "orh_whatif_refresh");
  }
  if (digests_) {
    const uint32_t *bd = nullptr, *bn = nullptr;
    check(ctx_, orh_whatif_base_rows(job_, &bd, &bn), "orh_whatif_base_rows");
    check(ctx_, orh_row_digest(ctx_, bd, bn, 1, n_, static_cast<uint32_t>(srcs_.size()), dBaseDigest_),
          "orh_row_digest");
  }
  for (size_t c = 0; c < chunks_.size(); ++c) {
    const Chunk& ch = chunks_[c];
    const uint32_t nr = static_cast<uint32_t>(ch.hi - ch.lo);
    const int b = static_cast<int>(c % nBuf_);  // cycle the row buffers
    // this run overwrites the rows of chunk c - nBuf_, and waits for them by
    // itself: their summary goes right before it
    if ((impact_ || gain_) && c >= static_cast<size_t>(nBuf_)) queueImpact(c - nBuf_);
    if (lowers_)
      check(ctx_,
            orh_whatif_run_lowers(job_, nr, srcIdx_.data() + ch.lo, ch.ptr.data(), ch.links.data(),
                                  drains_ ? ch.drnPtr.data() : nullptr, drains_ ? ch.drnNodes.data() : nullptr,
                                  raises_ ? ch.metPtr.data() : nullptr, raises_ ? ch.mets.data() : nullptr,
                                  ch.lowPtr.data(), ch.lows.data(), dDist_[b], dNh_[b], dInfo_ + ch.lo),
            "orh_whatif_run_lowers");
    else if (raises_)
      check(ctx_,
            orh_whatif_run_metrics(job_, nr, srcIdx_.data() + ch.lo, ch.ptr.data(), ch.links.data(),
                                   drains_ ? ch.drnPtr.data() : nullptr, drains_ ? ch.drnNodes.data() : nullptr,
                                   ch.metPtr.data(), ch.mets.data(), dDist_[b], dNh_[b], dInfo_ + ch.lo),
            "orh_whatif_run_metrics");
    else if (drains_)
      check(ctx_,
            orh_whatif_run_drains(job_, nr, srcIdx_.data() + ch.lo, ch.ptr.data(), ch.links.data(),
                                  ch.drnPtr.data(), ch.drnNodes.data(), dDist_[b], dNh_[b], dInfo_ + ch.lo),
            "orh_whatif_run_drains");
    else
      check(ctx_,
            orh_whatif_run(job_, nr, srcIdx_.data() + ch.lo, ch.ptr.data(), ch.links.data(), dDist_[b], dNh_[b],
                           dInfo_ + ch.lo),
            "orh_whatif_run");
    if (digests_) {  // the chunk's rows complete in stream order, then digested
      check(ctx_, orh_whatif_flush(job_), "orh_whatif_flush");
      check(ctx_, orh_row_digest(ctx_, dDist_[b], dNh_[b], 1, n_, nr, dDigest_ + ch.lo), "orh_row_digest");
    }
  }
  if (impact_ || gain_) {  // the chunks still in the buffers
    const size_t nc = chunks_.size();
    for (size_t c = nc > static_cast<size_t>(nBuf_) ? nc - nBuf_ : 0; c < nc; ++c) queueImpact(c);
    (gain_ ? gainRan_ : impactRan_) = true;
  }
  check(ctx_, orh_whatif_flush(job_), "orh_whatif_flush");
}

double WhatIfBatch::lastMs() const {
  double ms = 0;
  if (!job_) throw std::logic_error("WhatIfBatch: no run");
  check(ctx_, orh_whatif_elapsed_ms(job_, &ms), "orh_whatif_elapsed_ms");
  return ms;
}

void WhatIfBatch::sync() const { check(ctx_, orh_sync(ctx_), "orh_sync"); }

void WhatIfBatch::info(uint32_t* out) const {
  check(ctx_, orh_memcpy_d2h(ctx_, out, dInfo_, srcIdx_.size() * 4), "orh_memcpy_d2h");
}

void WhatIfBatch::digests(uint64_t* out) const {
  if (!digests_) throw std::logic_error("WhatIfBatch: digests were not enabled for the last run");
  check(ctx_, orh_memcpy_d2h(ctx_, out, dDigest_, srcIdx_.size() * 8), "orh_memcpy_d2h");
  if (!shareBase_) return;
  // a request whose source row stands was not copied: its row is the base row
  std::vector<uint32_t> inf(srcIdx_.size());
  std::vector<uint64_t> base(srcs_.size());
  info(inf.data());
  check(ctx_, orh_memcpy_d2h(ctx_, base.data(), dBaseDigest_, base.size() * 8), "orh_memcpy_d2h");
  for (size_t i = 0; i < inf.size(); ++i)
    if (ORH_WHATIF_TIER(inf[i]) == 0) out[i] = base[srcIdx_[i]];
}

void WhatIfBatch::fetch(size_t i, uint32_t* dist, uint32_t* nh) const {
  const Chunk& last = chunks_.back();
  if (i < last.lo || i >= last.hi) throw std::out_of_range("WhatIfBatch.fetch: not in the last chunk");
  if (!job_ || !nBuf_) throw std::logic_error("WhatIfBatch.fetch: no rows (not run, or released)");
  const size_t r = i - last.lo;
  const int b = static_cast<int>((chunks_.size() - 1) % nBuf_);
  const uint32_t* d = dDist_[b] + r * n_;
  const uint32_t* m = dNh_[b] + r * n_;
  if (shareBase_) {  // a request whose source row stands reads the job's base row
    uint32_t inf = 0;
    check(ctx_, orh_memcpy_d2h(ctx_, &inf, dInfo_ + i, 4), "orh_memcpy_d2h");
    if (ORH_WHATIF_TIER(inf) == 0) {
      const uint32_t *bd = nullptr, *bn = nullptr;
      check(ctx_, orh_whatif_base_rows(job_, &bd, &bn), "orh_whatif_base_rows");
      d = bd + static_cast<size_t>(srcIdx_[i]) * n_;
      m = bn + static_cast<size_t>(srcIdx_[i]) * n_;
    }
  }
  check(ctx_, orh_memcpy_d2h(ctx_, dist, d, n_ * 4ull), "orh_memcpy_d2h");
  check(ctx_, orh_memcpy_d2h(ctx_, nh, m, n_ * 4ull), "orh_memcpy_d2h");
}

}  // namespace openr_amd
