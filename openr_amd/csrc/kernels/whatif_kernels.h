// Internal interface of the what-if repair kernels (whatif_kernels.hip), the
// metric-lower pass behind them (whatif_lower_kernels.hip), the impact
// summaries over their rows (whatif_impact_kernels.hip) and the two-sided
// summaries (whatif_gain_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

struct orh_whatif_impact_rec;  // include/openr_hip.h
struct orh_whatif_gain_rec;

namespace orh {

// ---- what-if repair (whatif_kernels.hip) ----------------------------------
// runSpf(src, useLinkMetric, ignore) for many (src, ignore set) requests from
// the plain SPF rows of their sources: a request's row is the base row except
// on the nodes downstream of a tight ignored link, which are re-derived.
//
// Requests move through tiers; each tier is a work queue drained by a fixed
// grid of workgroups (every workgroup exits once the queue is empty):
//   seed   one thread per request: no tight ignored link -> the base row
//          stands (tier 0); else the request joins queue 1
//   tier 1 small LDS state (kSmallA nodes / kSmallE edges): most repairs
//   tier 2 large LDS state (cap_a / cap_e)
//   tier 3 global slots sized for the whole graph (cannot overflow)
//   tier 4 only without slots: the full HBM search (fallback flags)
// A request may also drain nodes (treat them as overloaded): their
// out-records are staged as cuts, drn_ptr / drn carry the sets. A request may
// raise link metrics too: the raised records are staged as cuts, rse_ptr /
// rse carry (record, new weight); a run with raises takes no full search.
constexpr uint32_t kWhatifTierBase = 0, kWhatifTierSmall = 1, kWhatifTierLarge = 2, kWhatifTierSlot = 3,
                   kWhatifTierSearch = 4;
// a row that the lower pass re-derived behind the tiers (whatif_lower_kernels.hip)
constexpr uint32_t kWhatifTierLowered = 5;
constexpr uint32_t kSmallA = 256, kSmallE = 1024;
// counters (u32, zeroed before a run): per queue q = 0..2 its length and the
// next index to claim; the last two are the lower pass's slot queue
constexpr uint32_t kWhatifCounters = 8;

struct RepairArgs {
  uint32_t n_nodes;
  uint32_t n_req;
  int32_t use_link_metric;
  uint32_t cap_a;  // tier 2: affected nodes a workgroup repairs in LDS
  uint32_t cap_e;  // tier 2: predecessor edges among them
  const uint2* recs;
  const uint32_t* link;
  const uint16_t* rank_out;
  const uint32_t* rev;  // per record: the record of the same link from the other end
  const uint8_t* ovl;   // [N] node overloaded
  const uint32_t* base_dist;  // [m][N]
  const uint32_t* base_nh;    // [m][N], one mask word
  const uint32_t* base_row;   // [n_req] base row of the request's source
  const uint32_t* srcs;       // [n_req]
  const uint32_t* ign_ptr;    // [n_req + 1]
  const uint32_t* ign;        // sorted per request
  const uint32_t* cut_ptr;    // [n_req + 1]
  const uint4* cuts;          // (tail, head, record tail -> head, 0) per ignored link end, and per
                              // out-record of a drained node, and per raised record
  // drained nodes (nullable: none, and the kernels without the drain tests
  // run): per request the nodes treated as overloaded, sorted, without the
  // request's source
  const uint32_t* drn_ptr;    // [n_req + 1]
  const uint32_t* drn;
  // metric raises (nullable: none, and the kernels without the raise lookup
  // run): per request (record index, raised weight) pairs sorted by record;
  // each raised record is staged as a cut as well
  const uint32_t* rse_ptr;    // [n_req + 1]
  const uint2* rse;
  uint32_t* out_dist;         // [n_req][N]
  uint32_t* out_nh;           // [n_req][N], one mask word
  uint32_t* fallback;         // [n_req] set when a request needs the full search (no slots)
  uint32_t* info;             // [n_req] tier | affected nodes << 3 (nullable)
  uint32_t* queues;           // [3][n_req] request ids of queues 0..2 (tiers 1..3)
  uint32_t* counters;         // [kWhatifCounters]
  // tier 3: n_slots global slots of slot_bytes each, one per workgroup
  uint8_t* slot_mem;
  size_t slot_bytes;
  uint32_t n_slots;
  uint32_t n_recs;  // device records (slot edge capacity)
  uint32_t n_cu;    // grid sizing of the queue-draining tiers
  // the first full_cap entries of the slot tier's queue are searched in full
  // instead (a separate launch over that list, repair_slot_queue): a large
  // subtree repairs slower in a slot than the whole search runs; the slot
  // tier takes the rest and marks those requests kWhatifTierSearch
  uint32_t full_cap;
  // copy only the requests the seed queued for repair (queue 0): the others'
  // rows are their sources' base rows, which the caller reads from the job
  uint32_t share_base;
  // no tier 2 (host-side launch plan only): the requests that outgrow tier 1
  // go straight to the full searches / slot tier, which then start as soon
  // as tier 1 ends (a short job's largest repairs are its critical path)
  uint32_t skip_large;
};
// queue index the slot tier drains (the full search's list)
uint32_t repair_slot_queue(const RepairArgs& a);
// LDS bytes of the repair kernel for the given caps
size_t repair_lds_bytes(uint32_t n_nodes, uint32_t cap_a, uint32_t cap_e);
// bytes of one global repair slot (whole-graph caps)
size_t repair_slot_bytes(uint32_t n_nodes, uint32_t n_recs);
// seed, copy each request's base rows, then the repair tiers; with no slots
// the requests that outgrow tier 2 get fallback[r] = 1 (zeroed beforehand).
// In two parts: seed and copy (HBM-bound, the whole GPU), then the
// repair tiers (latency-bound, a few thousand workgroups), which may run on a
// second stream, overlapping the next batch's copy
hipError_t launch_repair_front(const RepairArgs& a, uint32_t ell_k, size_t lds_limit, hipStream_t s);
hipError_t launch_repair_back(const RepairArgs& a, uint32_t ell_k, size_t lds_limit, hipStream_t s);
// the same with the slot tier on its own stream s3, after event `mid`
// (recorded on s behind tiers 1 and 2): the next run's small tiers on s do
// not wait for this run's largest repairs
hipError_t launch_repair_back_split(const RepairArgs& a, uint32_t ell_k, size_t lds_limit, hipStream_t s,
                                    hipStream_t s3, hipEvent_t mid);

// ---- metric lowers (whatif_lower_kernels.hip) -----------------------------
// Stage 2 of the requests of a run that lower link metrics: each one's row,
// as the repair tiers left it, becomes the exact row of the graph with the
// lowered records as well (the kernel file has the rule and why it is exact).
struct LowerArgs {
  uint32_t n_low;           // requests with at least one effective lower
  const uint32_t* req;      // [n_low] their request ids, ascending
  const uint32_t* rec_ptr;  // [n_low + 1]
  const uint4* recs;        // lowered records: (tail, head, record tail -> head, lowered weight)
  const uint32_t* wl_ptr;   // [n_low + 1]
  const uint2* wl;          // per request (record, weight) sorted by record: its lowers and its raises
  uint32_t* queue;          // [n_low] list positions whose sets outgrew the LDS caps (slot pass)
  uint32_t cap_a, cap_e;    // LDS caps of the first pass: nodes of M, predecessor edges among them
};
// LDS bytes of the first pass for the given caps
size_t lower_lds_bytes(uint32_t n_nodes, uint32_t cap_a, uint32_t cap_e);
// both passes on stream s, behind the run's last tier: the LDS pass, then the
// slot pass over a.slot_mem (a.n_slots > 0) for what outgrew it
hipError_t launch_lower(const RepairArgs& a, const LowerArgs& l, uint32_t ell_k, size_t lds_limit, hipStream_t s);

// per row r < rows: the digest of (dist[r][v], nh[r][v][0..words)) over v < n
// (row_digest_kernel), into out[r]
hipError_t launch_row_digest(const uint32_t* dist, const uint32_t* nh, uint32_t words, uint32_t n,
                             uint32_t rows, uint64_t* out, hipStream_t s);

// ---- what-if impact (whatif_impact_kernels.hip) ---------------------------
// request r's row (dist / nh + r * N) against base row base_row[r], reduced to
// out[r] (orh_whatif_impact in include/openr_hip.h has the classes)
struct ImpactArgs {
  uint32_t n_nodes;
  uint32_t n_req;
  const uint32_t* base_dist;  // [m][N]
  const uint32_t* base_nh;    // [m][N], one mask word
  const uint32_t* base_row;   // [n_req] base row of the request's source
  const uint32_t* srcs;       // [n_req] its source node (in no class)
  const uint32_t* dist;       // [n_req][N]
  const uint32_t* nh;         // [n_req][N]
  const uint32_t* info;       // [n_req] (nullable: every row is scanned); tier 0: the row is not read
  const uint32_t* weight;     // [N] (nullable)
  uint32_t* node_lost;        // [N] (nullable), accumulated
  uint32_t* node_moved;       // [N] (nullable), accumulated
  ::orh_whatif_impact_rec* out;  // [n_req]
};
// zeroes the records, scans, then finishes max_stretch / worst_node
hipError_t launch_whatif_impact(const ImpactArgs& a, hipStream_t s);

// ---- two-sided what-if summaries (whatif_gain_kernels.hip) ----------------
// the same comparison with the nodes that got nearer and those whose first-hop
// set grew counted too (orh_whatif_gain in include/openr_hip.h has the classes)
struct GainArgs {
  uint32_t n_nodes;
  uint32_t n_req;
  const uint32_t* base_dist;  // [m][N]
  const uint32_t* base_nh;    // [m][N], one mask word
  const uint32_t* base_row;   // [n_req] base row of the request's source
  const uint32_t* srcs;       // [n_req] its source node (in no class)
  const uint32_t* dist;       // [n_req][N]
  const uint32_t* nh;         // [n_req][N]
  const uint32_t* info;       // [n_req] (nullable: every row is scanned); tier 0: the row is not read
  const uint32_t* weight;     // [N] (nullable)
  uint32_t* node_lost;        // [N] (nullable), accumulated
  uint32_t* node_moved;       // [N] (nullable), accumulated
  uint32_t* node_nearer;      // [N] (nullable), accumulated
  ::orh_whatif_gain_rec* out;  // [n_req]
};
// zeroes the records, scans, then finishes max_stretch / worst_node and
// max_gain / best_node
hipError_t launch_whatif_gain(const GainArgs& a, hipStream_t s);

}  // namespace orh
