// Batched link-failure and node-drain what-if SPFs ("4,096
// links x 64 sources" of runSpf(src, true, {link}), LinkState.cpp:808-882;
// a drain is the same SPF with the node's overload bit set, :480-493) through one
// what-if job of libopenr_hip (orh_whatif_*): the sources' plain rows are
// searched once, then the requests run in chunks into device row buffers; a
// request's row is its source's row except below a tight ignored link or a
// tight out-link of a drained node, where the job re-derives it (bit-identical
// to a fresh runSpf). A request may also raise link metrics (cost a link out,
// Link::setMetricFromNode, :640-710): the same repair below the raised records
// that were tight, with the raised weights. And it may lower them (cost a
// link back in): a second pass behind the repair lets distances fall and
// first-hop masks widen below the lowered records.
//
// This is the library form a caller outside Python drives (the bench, the
// multi-device split in multi_device.h); the Python binding wraps it.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "link_state.h"

namespace openr_amd {

// One metric raise of a what-if request (costing a link out): the metric
// that `from` advertises for LinkState link `link` becomes `metric` (>= the
// current one). An empty `from` raises it from both ends.
struct WhatIfMetricRaise {
  uint32_t link;
  std::string from;
  uint32_t metric;
};

// One metric lower (costing a link back in): the same triple, `metric` <= the
// current one.
using WhatIfMetricLower = WhatIfMetricRaise;

class WhatIfBatch {
 public:
  // request i = (srcs[srcIdx[i]], ignore[i]) with ignore sets of LinkState link
  // ids; chunk = requests per orh_whatif_run. shareBase: ORH_WHATIF_SHARE_BASE
  // (a request whose source row stands references the job's base row);
  // searchLarge: ORH_WHATIF_SEARCH_LARGE (the largest repairs searched in
  // full: for a device's block of a split job). drain: per request the names
  // of the nodes it treats as overloaded (empty: no request drains any; else
  // one list per request, each possibly empty); an unknown name is
  // std::invalid_argument. metric: per request its metric raises, with the
  // same conventions (empty: none at all; an unknown end name is
  // std::invalid_argument; a decrease fails the run, see
  // orh_whatif_run_metrics). lower: per request its metric lowers, same
  // conventions (an increase fails the run, see orh_whatif_run_lowers); a
  // batch with lowers takes no impact summaries (run() throws
  // std::invalid_argument with setImpact(true)): setGain summarises it
  WhatIfBatch(const LinkState& ls, const std::vector<std::string>& srcs, const std::vector<uint32_t>& srcIdx,
              const std::vector<std::vector<uint32_t>>& ignore, uint32_t chunk, bool useLinkMetric = true,
              bool shareBase = false, bool searchLarge = false,
              const std::vector<std::vector<std::string>>& drain = {},
              const std::vector<std::vector<WhatIfMetricRaise>>& metric = {},
              const std::vector<std::vector<WhatIfMetricLower>>& lower = {});
  ~WhatIfBatch();
  WhatIfBatch(const WhatIfBatch&) = delete;
  WhatIfBatch& operator=(const WhatIfBatch&) = delete;

  // the sources' plain searches (the first run; later runs refresh them on
  // the graph as it is now), then every chunk; asynchronous on the context
  // stream
  void run();
  void sync() const;
  // device time of the last run (base searches to the last chunk, HIP events)
  double lastMs() const;
  // per request (caller's order): ORH_WHATIF_TIER | ORH_WHATIF_AFFECTED << 3
  void info(uint32_t* out) const;
  // verification mode: every chunk's rows are digested (orh_row_digest) before
  // their buffer is reused, and a shared-base request gets its source row's
  // digest; each chunk is flushed first, so runs in this mode are slower
  void setDigests(bool on);
  void digests(uint64_t* out) const;
  // impact mode: every chunk's rows are summarised on the device
  // (orh_whatif_impact: lost / farther / rehomed / narrowed nodes, stretch,
  // weights) while they are still in their buffer. A chunk's summary is queued
  // where the pipeline waits for the chunk anyway - before the run that
  // reuses its row buffer, or before the final flush - so the mode adds one
  // streaming pass over the repaired rows and no stall. weights: (node name,
  // weight) pairs, absent nodes weigh 0, an unknown name is
  // std::invalid_argument; nodeCounts: per node, in how many requests it is
  // lost / moved (nodeImpact)
  void setImpact(bool on, const std::vector<std::pair<std::string, uint32_t>>& weights = {},
                 bool nodeCounts = false);
  // [requests()] records of the last run, in the caller's request order
  void impact(orh_whatif_impact_rec* out) const;
  // [nodes()] each (graph node ids), summed over the last run's requests
  void nodeImpact(uint32_t* lost, uint32_t* moved) const;
  // gain mode: impact mode with the two-sided records of orh_whatif_gain
  // (nearer and widened nodes, gain next to stretch), for batches with or
  // without lowers; queued at the same points, same arguments. One mode per
  // run: with setImpact on as well run() throws std::invalid_argument
  void setGain(bool on, const std::vector<std::pair<std::string, uint32_t>>& weights = {},
               bool nodeCounts = false);
  // [requests()] records of the last run, in the caller's request order
  void gain(orh_whatif_gain_rec* out) const;
  // [nodes()] each (graph node ids), summed over the last run's requests
  void nodeGain(uint32_t* lost, uint32_t* moved, uint32_t* nearer) const;
  // rows of request i; only the last chunk's rows are still in the buffers
  // (std::out_of_range otherwise)
  void fetch(size_t i, uint32_t* dist, uint32_t* nh) const;
  // free the row buffers and the job (the next run allocates them again)
  void release();

  size_t requests() const { return srcIdx_.size(); }
  size_t sources() const { return srcs_.size(); }
  uint32_t chunk() const { return chunk_; }
  uint32_t nodes() const { return n_; }
  uint32_t edges() const { return edges_; }
  orh_ctx* context() const { return ctx_; }

 private:
  struct Chunk {
    size_t lo, hi;
    std::vector<uint32_t> ptr, links;
    std::vector<uint32_t> drnPtr, drnNodes;  // drained node ids, rebased like the ignore CSR
    std::vector<uint32_t> metPtr;            // metric raises, rebased the same way
    std::vector<orh_whatif_metric> mets;
    std::vector<uint32_t> lowPtr;            // metric lowers, likewise
    std::vector<orh_whatif_metric> lows;
  };
  void allocate();
  const LinkState& ls_;
  bool useLinkMetric_;
  bool shareBase_;
  bool searchLarge_;
  bool digests_{false};
  bool drains_{false};  // some request drains a node: runs go through orh_whatif_run_drains
  bool raises_{false};  // some request raises a metric: runs go through orh_whatif_run_metrics
  bool lowers_{false};  // some request lowers a metric: runs go through orh_whatif_run_lowers
  std::vector<uint32_t> srcs_, srcIdx_;
  std::vector<Chunk> chunks_;
  uint32_t chunk_{1};
  orh_graph* graph_{nullptr};
  orh_ctx* ctx_{nullptr};
  orh_whatif* job_{nullptr};
  uint64_t stamp_{0};  // LinkState::stateStamp the job was created at
  uint32_t n_{0}, edges_{0};
  // up to three row buffers, cycled between chunks, so a chunk's repairs
  // (which write into its rows) overlap the next two chunks' copies
  static constexpr size_t kBufs = 3;
  int nBuf_{0};
  uint32_t* dDist_[kBufs] = {};
  uint32_t* dNh_[kBufs] = {};
  uint32_t* dInfo_{nullptr};
  uint64_t* dDigest_{nullptr};      // [requests] (verification mode)
  uint64_t* dBaseDigest_{nullptr};  // [sources]
  // impact and gain mode (they share the weights and the node counters)
  void queueImpact(size_t c);  // chunk c's summary in the mode that is on
  void freeImpact();
  void setSummary(bool* mode, bool other, bool on, const std::vector<std::pair<std::string, uint32_t>>& weights,
                  bool nodeCounts);
  bool impact_{false};
  bool gain_{false};
  bool nodeCounts_{false};
  bool impactRan_{false};  // the last run filled dImpact_ (and the node arrays)
  bool gainRan_{false};    // the last run filled dGain_ (and the node arrays)
  std::vector<uint32_t> weights_;            // [n_] (empty: none)
  orh_whatif_impact_rec* dImpact_{nullptr};  // [requests]
  uint32_t* dWeight_{nullptr};               // [n_]
  uint32_t* dNodeLost_{nullptr};             // [n_]
  uint32_t* dNodeMoved_{nullptr};            // [n_]
  orh_whatif_gain_rec* dGain_{nullptr};      // [requests] (gain mode)
  uint32_t* dNodeNearer_{nullptr};           // [n_] (gain mode)
  // the last run's results, kept on the host when release() frees the above
  std::vector<orh_whatif_impact_rec> hImpact_;
  std::vector<orh_whatif_gain_rec> hGain_;
  std::vector<uint32_t> hNodeLost_, hNodeMoved_, hNodeNearer_;
};

}  // namespace openr_amd
