// Internal to the SPF units (spf_*.hip): the launch function of each kernel
// family, which launch_spf (spf_plan.hip) dispatches to, and the launch-side
// knobs. orh_api.hip sees spf_kernels.h only.
#pragma once

#include "spf_kernels.h"

namespace orh {

// Environment knobs of the planners and launchers, read in launch_knobs()
// (spf_plan.hip) and nowhere else; orh_spf_run's own are SpfKnobs (orh_api.hip).
struct LaunchKnobs {
  // read at every call (tests and A/B runs flip them in-process)
  uint32_t ms_block;    // ORH_MS_BLOCK (A/B): threads per multi-source workgroup, a multiple of 64
                        // in [64, 1024]; 0 = unset or invalid
  bool ms_block_set;    // ORH_MS_BLOCK present at all: no latency / lone-sweep plan (ms_set_width)
  int ms_latency;       // ORH_MS_LATENCY (default 1): 0 = no latency / lone-sweep plan, 2 = the
                        // latency plan with the interval skip as well (see ms_set_width)
  bool ms_wide;         // ORH_MS_WIDE=1 (opt-in): u64 masks when u32 ones need more than one batch
                        // per CU (see ms_set_width)
  bool wms_four;        // ORH_WMS_SOURCES=4 (A/B): 4-source batches even where 8 fit
  bool wms_wide_two;    // ORH_WMS_WIDE_SOURCES=2 (A/B): 2-source wide batches even where 4 fit
  bool hop_xcd;         // ORH_HOP_XCD=1 (A/B): first_hop_kernel's XCD-aware source order
  bool hop_lean;        // ORH_HOP_LEAN=0 (A/B): the generic level-row first-hop kernel even where the
                        // lean one applies
  // read once per process
  uint32_t lds16_block;  // ORH_LDS16_BLOCK (A/B): threads per u16 LDS search (one search per CU
                         // either way); a multiple of 64 in [64, 1024], else 1024
  bool hop_narrow;       // ORH_HOP_NARROW=1 (A/B): 4 nodes per thread even for large batches (65
                         // instead of 158 VGPRs: waves that fit beside the MS-BFS workgroups of
                         // other streams)
  uint32_t hop_nodes;    // ORH_HOP_NODES=16 (A/B): the 16-node form for large batches, else 8
  uint32_t hop_split;    // ORH_HOP_SPLIT=n (A/B): at least n workgroups per source (tile phases)
  uint32_t hop_wg_per_cu;  // ORH_HOP_WG_PER_CU (A/B, default 0 = one workgroup per logical
                           // block): persistent workgroups, that many per CU (launch_first_hop)
};
LaunchKnobs launch_knobs();

// one per family; each picks its instantiation from plan.ell_k (4 or 8)
hipError_t launch_ms(const SpfPlan& plan, const SpfArgs& a, uint32_t n_rows, hipStream_t s);
hipError_t launch_bfs(const SpfPlan& plan, const SpfArgs& a, uint32_t n_rows, hipStream_t s);
hipError_t launch_bfs_nh(const SpfPlan& plan, const SpfArgs& a, uint32_t n_rows, hipStream_t s);
hipError_t launch_dist(const SpfPlan& plan, const SpfArgs& a, uint32_t n_rows, hipStream_t s);
hipError_t launch_global(const SpfPlan& plan, const SpfArgs& a, uint32_t n_rows, hipStream_t s);
hipError_t launch_global_nh(const SpfPlan& plan, const SpfArgs& a, uint32_t n_rows, hipStream_t s);
// spf_lds_nh_kernel<K, false> (K = a.recs_k) over the rows a.row_list lists,
// 256 threads each: the rows the WMS batches flagged
hipError_t launch_lds_nh_rows(const SpfArgs& a, uint32_t n_rows, hipStream_t s);

}  // namespace orh
