// Node orders for the multi-source BFS layout: pure functions of the
// distinct-neighbour lists (no HIP, no graph state).
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace orh {

constexpr uint32_t kMsOrderNone = 0xFFFFFFFFu;

// Cuthill-McKee: BFS from a low-degree node of each component, neighbours
// visited in ascending degree (then node id) order. dn_ptr / dn: distinct
// neighbours per node. Fills host_of (id -> node) and dev_of (node -> id);
// returns the deepest BFS level of any component.
inline uint32_t ms_cm_order(uint32_t n, const uint32_t* dn_ptr, const uint32_t* dn, std::vector<uint32_t>& host_of,
                            std::vector<uint32_t>& dev_of) {
  host_of.clear();
  host_of.reserve(n);
  dev_of.assign(n, kMsOrderNone);
  std::vector<uint32_t> deg(n), by_deg(n), nb, lvl(n, 0);
  uint32_t depth = 0;
  for (uint32_t v = 0; v < n; ++v) {
    deg[v] = dn_ptr[v + 1] - dn_ptr[v];
    by_deg[v] = v;
  }
  std::stable_sort(by_deg.begin(), by_deg.end(), [&](uint32_t a, uint32_t b) { return deg[a] < deg[b]; });
  for (uint32_t root : by_deg) {
    if (dev_of[root] != kMsOrderNone) continue;
    size_t head = host_of.size();
    dev_of[root] = static_cast<uint32_t>(host_of.size());
    host_of.push_back(root);
    while (head < host_of.size()) {
      const uint32_t v = host_of[head++];
      nb.clear();
      for (uint32_t k = dn_ptr[v]; k < dn_ptr[v + 1]; ++k)
        if (dev_of[dn[k]] == kMsOrderNone) nb.push_back(dn[k]);
      std::stable_sort(nb.begin(), nb.end(), [&](uint32_t a, uint32_t b) { return deg[a] < deg[b]; });
      for (uint32_t u : nb) {
        dev_of[u] = static_cast<uint32_t>(host_of.size());
        host_of.push_back(u);
        lvl[u] = lvl[v] + 1;
        depth = std::max(depth, lvl[u]);
      }
    }
  }
  return depth;
}

// Cluster order: device ids in runs of 64 - one wave's slice in
// spf_msbfs_kernel - that are compact BFS clusters, where Cuthill-McKee's
// runs are long thin pieces of a BFS level. The search pays per slice, not
// per node: its gathers run for every slice that still misses a bit, and one
// log store is issued per (slice, level) with an arrival, so a compact slice
// is open for fewer levels and its arrivals share fewer, fuller stores
// (tools/ms_order_model.py counts both).
//
// A cluster is seeded from the queue of unassigned nodes next to finished
// clusters, else (a new component) from the lowest unassigned Cuthill-McKee
// id, and grown by BFS over unassigned nodes, neighbours in Cuthill-McKee
// order, until its run of 64 ids is full; ids inside it are in growth order,
// so its first 32 ids (a batch of sources) are compact too. A growth that
// runs dry inside a component (a pocket between finished clusters) takes the
// next seed into the same run, so the clusters stay aligned with the runs; a
// component ends wherever its last node falls, and the next component's
// first cluster fills that run up. The queue only ever holds nodes of the
// component being numbered, so components get contiguous ids. O(E log deg).
//
// dn_ptr / dn: distinct neighbours per node; cm_host_of / cm_dev_of: the
// Cuthill-McKee order (id -> node, node -> id). Fills host_of (id -> node)
// and dev_of (node -> id).
inline void ms_cluster_order(uint32_t n, const uint32_t* dn_ptr, const uint32_t* dn, const uint32_t* cm_host_of,
                             const uint32_t* cm_dev_of, std::vector<uint32_t>& host_of,
                             std::vector<uint32_t>& dev_of) {
  constexpr uint32_t kRun = 64;
  host_of.clear();
  host_of.reserve(n);
  dev_of.assign(n, kMsOrderNone);
  if (n == 0) return;
  std::vector<uint32_t> nb(dn, dn + dn_ptr[n]);  // neighbour lists in Cuthill-McKee order
  for (uint32_t v = 0; v < n; ++v)
    std::stable_sort(nb.begin() + dn_ptr[v], nb.begin() + dn_ptr[v + 1],
                     [&](uint32_t a, uint32_t b) { return cm_dev_of[a] < cm_dev_of[b]; });
  std::vector<uint32_t> seeds;  // FIFO
  size_t seed_head = 0;
  uint32_t next_cm = 0;
  while (host_of.size() < n) {
    uint32_t seed = kMsOrderNone;
    while (seed_head < seeds.size() && seed == kMsOrderNone) {
      const uint32_t s = seeds[seed_head++];
      if (dev_of[s] == kMsOrderNone) seed = s;
    }
    if (seed == kMsOrderNone) {
      while (dev_of[cm_host_of[next_cm]] != kMsOrderNone) ++next_cm;
      seed = cm_host_of[next_cm];
    }
    const size_t first = host_of.size();
    const size_t end = std::min<size_t>(n, first + (kRun - first % kRun));
    dev_of[seed] = static_cast<uint32_t>(first);
    host_of.push_back(seed);
    for (size_t head = first; head < host_of.size() && host_of.size() < end;) {
      const uint32_t v = host_of[head++];
      for (uint32_t k = dn_ptr[v]; k < dn_ptr[v + 1] && host_of.size() < end; ++k) {
        const uint32_t u = nb[k];
        if (dev_of[u] != kMsOrderNone) continue;
        dev_of[u] = static_cast<uint32_t>(host_of.size());
        host_of.push_back(u);
      }
    }
    const size_t last = host_of.size();
    for (size_t i = first; i < last; ++i) {
      const uint32_t v = host_of[i];
      for (uint32_t k = dn_ptr[v]; k < dn_ptr[v + 1]; ++k)
        if (dev_of[nb[k]] == kMsOrderNone) seeds.push_back(nb[k]);
    }
  }
}

// Slice adjacency of an order: for each 64-id slice (ids [64 s, 64 s + 64):
// one wave's nodes of one j in spf_msbfs_kernel) the slices that hold a
// neighbour of any of its nodes, the slice itself included, ascending. A node
// can gain a frontier bit only from a neighbour, so a slice can gain one at
// level L only if one of these slices gained one at level L - 1: the key of
// the kernel's adjacency skip. Cluster order keeps the sets small (5.6 slices
// on the 100 x 100 grid, 9 at most) where the id bandwidth is most of N.
//
// nb_ptr / nb: per node, every neighbour the layout can ever read - all CSR
// records of the node, continuation ones and down or drained ones included,
// repeats allowed - so the sets are a superset that up / down and metric
// flips cannot invalidate; dev_of: node -> id. Fills adj_ptr [slices + 1]
// and adj.
inline void ms_slice_adjacency(uint32_t n, const uint32_t* nb_ptr, const uint32_t* nb, const uint32_t* dev_of,
                               std::vector<uint32_t>& adj_ptr, std::vector<uint32_t>& adj) {
  constexpr uint32_t kRun = 64;
  const uint32_t slices = (n + kRun - 1) / kRun;
  std::vector<std::vector<uint32_t>> sets(slices);
  for (uint32_t s = 0; s < slices; ++s) sets[s].push_back(s);
  for (uint32_t v = 0; v < n; ++v) {
    std::vector<uint32_t>& set = sets[dev_of[v] / kRun];
    for (uint32_t k = nb_ptr[v]; k < nb_ptr[v + 1]; ++k) set.push_back(dev_of[nb[k]] / kRun);
  }
  adj_ptr.assign(slices + 1, 0);
  adj.clear();
  for (uint32_t s = 0; s < slices; ++s) {
    std::sort(sets[s].begin(), sets[s].end());
    sets[s].erase(std::unique(sets[s].begin(), sets[s].end()), sets[s].end());
    adj.insert(adj.end(), sets[s].begin(), sets[s].end());
    adj_ptr[s + 1] = static_cast<uint32_t>(adj.size());
  }
}

// The form spf_msbfs_kernel reads: per slice a bitmask over the slices,
// kMsAdjWords words (bit t of word k: slice 32 k + t is adjacent), so the
// kernel's envelope is kMsAdjSlices slices (16,384 nodes: every u32- and
// u64-mask shape). Empty when the graph has more slices.
constexpr uint32_t kMsAdjWords = 8;
constexpr uint32_t kMsAdjSlices = 32 * kMsAdjWords;
inline std::vector<uint32_t> ms_adjacency_masks(const std::vector<uint32_t>& adj_ptr,
                                                const std::vector<uint32_t>& adj) {
  const size_t slices = adj_ptr.empty() ? 0 : adj_ptr.size() - 1;
  std::vector<uint32_t> words;
  if (slices == 0 || slices > kMsAdjSlices) return words;
  words.assign(slices * kMsAdjWords, 0u);
  for (size_t s = 0; s < slices; ++s)
    for (uint32_t k = adj_ptr[s]; k < adj_ptr[s + 1]; ++k) words[s * kMsAdjWords + adj[k] / 32] |= 1u << (adj[k] % 32);
  return words;
}

}  // namespace orh
