// How a registration becomes launches, decided ONCE per registration and on the host alone: the tunables (Options, one table
// for set and get), what the context looks like to the decision (PlanEnv), the launch shape + kernel sequence (Plan, make_plan)
// and the key a captured launch sequence is cached under (GraphKey).  No HIP in here: plain C++17, checked on the CPU by
// tests/cpp/launch_plan_check.cpp; madicp_capi.hip switches on Plan::route and evaluates nothing of this again.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <tuple>

#include "madicp_hip.h"

namespace madicp {

// ---- constants shared with the kernels (kernels.hip.h includes this header) ---------------------------------------------------
constexpr int kBlock = 768;          // threads per icp_round workgroup = 12 wave64 = 3 per SIMD: ONE workgroup per CU
constexpr int kWaves = kBlock / 64;
constexpr int kAcc = 30;             // 21 (lower triangle of H, column by column) + 6 (b) + accepted pairs + nodes visited
                                     // (the reference's count: cached depths included) + nodes actually walked this round;
                                     // 30 doubles = 240 B: partial rows are 16-byte aligned
constexpr int kTopMax = 2048;  // LDS-staged top levels (kernels.hip.h): entries per tree, and the dynamic LDS of a launch that stages them
constexpr int kTopLdsBytes = kTopMax * (16 + 16);
// DEEP launches (a batch shares the chip) and their leaf-major rounds (icp_leaf_major.inc.h): ranges of at least
// kQueueMinPasses passes; at most kDeepTrees trees per workgroup
constexpr int kQueueMinPasses = 2;
constexpr int kDeepTreesLog2 = 4, kDeepTrees = 1 << kDeepTreesLog2;
constexpr int kJoinGroups = 4 * kWaves;  // 48 (kernels.hip.h, "Join of the per-workgroup partials")
constexpr int kJoinRows = 6;             // rows per lane held in registers (nblocks <= 288); longer ones stream
constexpr int join_rows(int nblocks) {
  return (nblocks <= kJoinGroups * kJoinRows) ? kJoinGroups * kJoinRows : (nblocks + kJoinGroups - 1) / kJoinGroups * kJoinGroups;
}
constexpr int kFoldGroups = 8;           // row & 7
// exchange granules (icp_persist, and icp_round's FOLD variant): see icp_persist for the protocol
constexpr int kRowGranules = 2 * kAcc;  // 480 bytes per row
constexpr size_t xch_level1(int n_scans, int grid) { return (size_t)2 * n_scans * grid * kRowGranules; }
constexpr size_t xch_granules(int n_scans, int grid) {
  return xch_level1(n_scans, grid) + (size_t)2 * n_scans * kFoldGroups * kRowGranules;
}
constexpr size_t kXchRowsMax = 1024 + 8 * MADICP_MAX_BATCH;  // level-1 rows + level-2 rows of the largest admissible launch
constexpr int kP2pFlagLeaves = 131072;  // moving sets beyond this OR their flags through the communicator, as before

// ---- options: every tunable of a context (madicp_ctx_set_option / madicp_ctx_get_option), with its default ----------------------
struct Options {
  int blocks_per_cu = 1;  // icp_round workgroups (768 threads) per CU
  int deal_trees = 2;     // a Job lists the caller's trees dealt over the eight XCD pieces, rows of eight in alternating direction (fill_job)
  int units_per_wg = 1;   // when a scan has more trees than workgroups: cut every tree's leaves into enough ranges for at least
                          // this many (tree, range) units per workgroup (see make_plan)
  int use_graph = 1;
  int comm_graph = 0;     // capture the RCCL calls too (off: rounds are launched eagerly with a communicator)
  int qpt_override = 0;
  int cache_corr = 1;  // reuse correspondences across GN rounds when provably unchanged
  int deep_min_leaves = 512;  // option "deep_min_leaves": with 24 keyframes or more and two scans in flight (48 or more and one), a launch with
                         // more trees than workgroups per XCD piece is DEEP (one range x all the piece's trees per workgroup) when a range
                         // holds at least this many leaves (make_plan)
  int interleave = 2;    // option "interleave_ranges": a range is every RPT-th group of 64 leaves instead of a contiguous stretch of the
                         // scan (kernels.hip.h, "Ranges"): 0 never, 1 DEEP launches (a batch shares the chip), 2 every launch
  int cache_gate = 1;   // option "cache_gate": a pair that keeps its leaf and was rejected with more slack than it has moved since is
                        // not evaluated again (kernels.hip.h, "Gate reuse")
  int queue_walks = 8192; // option "leaf_major": a DEEP launch (a batch shares the chip) runs a round leaf-major — moving leaf once per
                        // pass for all the workgroup's trees, walkers queued and walked densely — when the workgroup walked fewer
                        // than this many nodes per pass in the previous round (0: never; icp_leaf_major.inc.h)
  int nn_lds_top = 0;  // option "nn_lds_top": nn_search batches of >= 16 k queries walk the tree's top levels from LDS (nn_descend_top).
                       // Off: measured SLOWER for one 120 k-query launch (8.7 vs 6.6 us against a 20 k-leaf tree, 10.7 vs 9.2 us against a
                       // 120 k-leaf tree) — staging 48 KiB per workgroup costs more than the ~11 LDS levels save in a kernel this short
  int eager_when_busy = 1; // a registration queued behind another is launched kernel by kernel, not as a graph (graph_ok)
  int seq_completion = 1;  // streamed registrations publish completion through HostResult::seq instead of an event
  int host_feed_wait = 1;  // ... and the host, not the stream, waits for their feed while another one is in flight
  int publish_side = 1;    // streamed registrations: icp_publish carries results to the host beside the next registration
  int match_all = 0;       // option "match_all_rounds": the matched flags a registration returns are the OR over all its rounds
  int persistent = 0;      // all rounds of a registration as ONE launch (icp_persist) where the geometry admits it
  int xcd_fold = 0;        // per-round launches whose group leaders fold their XCD's rows at the end of the launch (experiment)
  int debug_collective_us = 0;  // development: a delay kernel of this length behind every collective (tools/shard_probe.py)
  int shard_tail = 0;      // sharded rounds leave the rank's adders themselves (icp_round's TAIL variant) instead of an icp_reduce launch.
                           // Off: built, bit-identical, measured SLOWER (profiles/r4_c_shard_probe.md: the 256 tickets on one address and the
                           // cross-XCD read of the rows cost ~8 us at the end of every round; the separate icp_reduce launch costs 4.5 us and no gap)
  int build_after_registration = 0;  // option (experiment, default off): a look-ahead construction's kernels wait for the registration in
                                     // flight (frontend_capi.inc.h; measured: does not remove the look-ahead cliff, profiles/r5_lookahead_matrix.md)
  int shard_p2p = 0;       // sharded rounds join over peer-mapped mailboxes inside the round kernel (madicp_p2p_attach) instead
                           // of icp_reduce + a collective between two rounds
  int upload_f32 = 1;        // option "upload_f32": a cloud of float-exact coordinates crosses PCIe as floats (frontend_capi.inc.h)
  int p2p_allow_coarse = 0;  // option "p2p_allow_coarse": accept a coarse-grained mailbox (ranks that share ONE device only)
  int shard_split = 1;     // a sharded batch of >= 4 scans runs as two halves on two streams: one half's all-reduce under the
                           // other half's round (profiles/r4_c_shard_probe.md: -14 % per registration at 8 scans with a 15 us
                           // collective; a loss without one, and with halves of one scan)
  int stage_min_leaves = 1024;  // LDS staging threshold (leaves per unit); 0 = always, huge = never (measured break-even ~1000)
  int comm_timeout_ms = 60000;  // bounded host wait behind a registration's collectives
  // how the host waits for a sequence number the device publishes (seq_wait.h: stream_collect, icp_publish_collect, tree_build)
  int wait_mode = 0;        // 0 spin, 1 sched_yield, 2 sleep ~50 us
  int wait_timeout_ms = 0;  // 0: unbounded; the two collects only — a tree build has no ticket to collect again and waits unbounded
};

// One row per settable key.  Bool: any non-zero value is 1.  Range: a value outside lo..hi is refused with `err`.
// Clamp: a value outside lo..hi becomes the nearer end.  Floor: a value below lo is refused with `err`, one above hi becomes hi.
struct OptionRow {
  enum Kind { Bool, Range, Clamp, Floor };
  const char* name;
  int Options::*member;
  Kind kind;
  int64_t lo, hi;
  const char* err;
};
inline constexpr OptionRow kOptionTable[] = {
    {"grid_blocks_per_cu", &Options::blocks_per_cu, OptionRow::Range, 1, 4, "grid_blocks_per_cu must be in 1..4"},
    {"publish_side", &Options::publish_side, OptionRow::Bool, 0, 1, ""},
    {"deal_trees", &Options::deal_trees, OptionRow::Range, 0, 2, "deal_trees is 0 (as listed), 1 (round-robin over the XCD pieces) or 2 (alternating rows)"},
    {"units_per_workgroup", &Options::units_per_wg, OptionRow::Range, 1, 64, "units_per_workgroup must be in 1..64"},
    {"use_graph", &Options::use_graph, OptionRow::Bool, 0, 1, ""},
    {"comm_graph", &Options::comm_graph, OptionRow::Bool, 0, 1, ""},
    {"cache_correspondences", &Options::cache_corr, OptionRow::Bool, 0, 1, ""},
    {"cache_gate", &Options::cache_gate, OptionRow::Bool, 0, 1, ""},
    {"deep_min_leaves", &Options::deep_min_leaves, OptionRow::Range, 64, 1 << 24, "deep_min_leaves must be in 64 .. 2^24"},
    {"interleave_ranges", &Options::interleave, OptionRow::Range, 0, 2, "interleave_ranges is 0 (never), 1 (batches that share the chip) or 2 (always)"},
    {"leaf_major", &Options::queue_walks, OptionRow::Range, 0, 1 << 20, "leaf_major must be 0 (never) or a node count per pass"},
    {"lds_stage_min_leaves", &Options::stage_min_leaves, OptionRow::Floor, 0, 1 << 30, "lds_stage_min_leaves must be >= 0"},
    {"eager_when_busy", &Options::eager_when_busy, OptionRow::Bool, 0, 1, ""},
    {"seq_completion", &Options::seq_completion, OptionRow::Bool, 0, 1, ""},
    {"host_feed_wait", &Options::host_feed_wait, OptionRow::Bool, 0, 1, ""},
    {"xcd_fold", &Options::xcd_fold, OptionRow::Bool, 0, 1, ""},
    {"debug_collective_us", &Options::debug_collective_us, OptionRow::Clamp, 0, 1000, ""},
    {"shard_tail", &Options::shard_tail, OptionRow::Bool, 0, 1, ""},
    {"build_after_registration", &Options::build_after_registration, OptionRow::Bool, 0, 1, ""},
    {"shard_p2p", &Options::shard_p2p, OptionRow::Bool, 0, 1, ""},
    {"shard_split", &Options::shard_split, OptionRow::Clamp, 0, 2, ""},
    {"match_all_rounds", &Options::match_all, OptionRow::Bool, 0, 1, ""},
    {"persistent", &Options::persistent, OptionRow::Bool, 0, 1, ""},
    {"wait_mode", &Options::wait_mode, OptionRow::Range, 0, 2, "wait_mode must be 0 (spin), 1 (yield) or 2 (sleep)"},
    {"wait_timeout_ms", &Options::wait_timeout_ms, OptionRow::Floor, 0, 1 << 30, "wait_timeout_ms must be >= 0"},
    {"comm_timeout_ms", &Options::comm_timeout_ms, OptionRow::Floor, 1, 1 << 30, "comm_timeout_ms must be >= 1"},
    {"p2p_allow_coarse", &Options::p2p_allow_coarse, OptionRow::Bool, 0, 1, ""},
    {"upload_f32", &Options::upload_f32, OptionRow::Bool, 0, 1, ""},
    {"nn_lds_top", &Options::nn_lds_top, OptionRow::Bool, 0, 1, ""},
    {"queries_per_lane", &Options::qpt_override, OptionRow::Range, 0, 2, "queries_per_lane must be 0 (default), 1 or 2"},
};

inline const OptionRow* option_row(const std::string& key) {
  for (const OptionRow& r : kOptionTable)
    if (key == r.name) return &r;
  return nullptr;
}

// false: unknown key or refused value — *err says which, the option is unchanged
inline bool option_set(Options& o, const std::string& key, int64_t value, std::string* err) {
  const OptionRow* r = option_row(key);
  const bool refused = r && ((value < r->lo && (r->kind == OptionRow::Range || r->kind == OptionRow::Floor)) ||
                             (value > r->hi && r->kind == OptionRow::Range));
  if (!r || refused) {
    *err = r ? std::string(r->err) : "unknown option: " + key;
    return false;
  }
  if (r->kind == OptionRow::Bool) value = value ? 1 : 0;
  o.*(r->member) = (int)std::max(r->lo, std::min(value, r->hi));
  return true;
}

inline bool option_get(const Options& o, const std::string& key, int64_t* out) {
  const OptionRow* r = option_row(key);
  if (r) *out = o.*(r->member);
  return r != nullptr;
}

// what the decision sees of a context
struct PlanEnv {
  int n_cus = 256;
  bool rccl = false;            // a communicator is installed
  bool host_transport = false;  // ... or a host-staged transport supplied by the caller
  bool p2p_attached = false;    // the peer mailboxes are mapped (madicp_p2p_attach)
  int n_ranks = 1;
  bool sharded() const { return rccl || host_transport; }
};

// ---- the plan: the kernel sequence of a registration (Route) and its launch shape -------------------------------------------
enum class Route {
  Rounds,   // one icp_round launch per round (sharded: + icp_reduce + an all-reduce behind each), icp_final
  Persist,  // all rounds as ONE launch (icp_persist), icp_final
  Fold,     // per-round launches with the XCD-hierarchical join (option "xcd_fold")
  Tail,     // sharded rounds that leave the rank's adders themselves: the TAIL variant publishes rows as exchange granules
  P2p,      // sharded rounds that join over the peer-mapped mailboxes inside the round kernel
};

struct Plan {  // one registration's launch shape and route
  int batch = 1, iters = 1, K = 0, trace = 0;  // as asked for
  int grid = 8;   // workgroups per scan (multiple of 8)
  int qpt = 1;    // leaves a lane walks at once: 1 or 2
  int lds = 0;    // dynamic LDS of the launch: kTopLdsBytes when units are big enough to stage a tree's top, else 0
  int rpt = 1;    // ranges per tree = units per tree
  int queue = 0;  // 1: units are long enough for queued walks (the QUEUE instantiation of icp_round, where the route has one)
  Route route = Route::Rounds;
  bool flags_in_box = false;  // P2p and every scan's matched flags fit a mailbox row: icp_final ORs them over the mailboxes itself,
                              // the whole registration is free of collectives — the single-GPU launch sequence, capturable
  bool interleave = false;    // the Jobs carry kFlagInterleave (option "interleave_ranges")
  // every member, for comparing plans (GraphKey): a member added above is added here
  auto tie() const { return std::tie(batch, iters, K, trace, grid, qpt, lds, rpt, queue, route, flags_in_box, interleave); }
};

// launch geometry: 8 XCDs x slots workgroups per scan, about blocks_per_cu * n_cus in total over the batch, and
// one (tree, range) unit per workgroup so that every workgroup gets the same number of leaves; then the route.
// flags_fit: every scan's leaves fit a mailbox flag row (L <= kP2pFlagLeaves; every rank holds the same moving sets, so
// every rank decides the same way)
inline Plan make_plan(const Options& o, const PlanEnv& e, int max_L, int K, int batch, int iters, bool trace, bool flags_fit) {
  Plan p;
  p.batch = batch; p.iters = iters; p.K = K; p.trace = trace ? 1 : 0;
  // One 768-thread workgroup per CU (3 waves per SIMD is what the kernel's registers allow), one (tree, range) unit
  // per workgroup; a batch shares the CUs between its scans.  One leaf per lane and pass by default (two leaves per
  // lane share their loads but were not measured faster).
  p.qpt = o.qpt_override == 2 ? 2 : 1;
  long long grid = std::max<long long>(8, (long long)o.blocks_per_cu * e.n_cus / std::max(1, batch));
  const long long max_useful = (long long)std::max(1, K) * ((max_L + 63) / 64);  // never below one wave of leaves per unit
  grid = std::max<long long>(8, std::min(grid, max_useful) / 8 * 8);
  p.grid = static_cast<int>(grid);
  p.rpt = static_cast<int>(std::max<long long>(1, grid / std::max(1, K)));
  if (o.units_per_wg > 1 && K > 0) {
    // More trees than workgroups (a batch shares the chip): with one range per tree a workgroup owns whole trees, and trees
    // differ in cost (how many of the scan's leaves still have to walk them, how many match) — the launch waits for the
    // workgroup with the expensive ones.  Finer ranges give every workgroup of an XCD piece a slice of ALL the piece's trees.
    const long long want = ((long long)o.units_per_wg * grid + K - 1) / K;
    const long long cap = std::max<long long>(1, max_L / 256);  // (a range of fewer than 256 leaves is not worth a descriptor)
    p.rpt = static_cast<int>(std::max<long long>(p.rpt, std::min(want, cap)));
  }
  // DEEP launches: more trees than workgroups per XCD piece (a batch shares the chip).  Every workgroup then gets ONE range
  // of the scan and ALL the trees of its piece — ranges per tree = workgroups per piece, so that its units u_first, u_first +
  // nslots, ... are the same range of consecutive trees — which is what the leaf-major rounds need (icp_leaf_major.inc.h)
  const int nslots = p.grid / 8;
  // (how many leaves a range must hold for that: two passes of a workgroup — below, the leaf-major queue has nothing to compact —
  // unless the piece holds three trees or more: then one unit per workgroup means the launch waits for the workgroups that drew
  // the newest keyframes, and one range of ALL the piece's trees per workgroup pays from 512 leaves on; measured,
  // profiles/r6_deep_threshold.md: 24-64 keyframes x 1-2 scans in flight + 3 .. + 40 %, 16 keyframes - 9 %)
  // (one scan in flight against 24-47 keyframes stays as it was: - 2 .. - 4 % that way at 32 keyframes, + 3 % at 24)
  const bool small_ranges_pay = K >= 24 && (batch >= 2 || K >= 48);
  const int deep_min = small_ranges_pay ? o.deep_min_leaves : std::max(o.deep_min_leaves, kQueueMinPasses * kBlock);
  if (K >= 8 && o.queue_walks > 0 && p.qpt == 1 && p.rpt < nslots && max_L / nslots >= deep_min && (K + 7) / 8 + 1 <= kDeepTrees)
    p.rpt = nslots;
  const int per_range = (max_L + p.rpt - 1) / p.rpt;
  p.lds = (K > 0 && per_range >= o.stage_min_leaves) ? kTopLdsBytes : 0;
  p.queue = (K >= 8 && o.queue_walks > 0 && p.qpt == 1 && p.rpt == nslots && per_range >= deep_min) ? 1 : 0;
  p.interleave = o.interleave == 2 || (o.interleave == 1 && p.queue);

  // The route.  Persist and Fold wait INSIDE a launch for workgroups of the same launch and tag their granules with 8 bits of
  // round: no collective between rounds (not sharded), 2..250 rounds, a scan's rows within the join and the exchange rows.
  const bool rows_fit = (p.grid >> 3) <= kJoinGroups && K >= 1 && xch_granules(batch, p.grid) <= kXchRowsMax * 2 * kRowGranules;
  const bool one_launch_join = !e.sharded() && !trace && iters >= 2 && iters <= 250 && rows_fit;
  const bool sharded_in_kernel = e.sharded() && !trace && p.qpt == 1 && iters <= 250;
  if (o.persistent && one_launch_join && o.blocks_per_cu == 1 && (long long)p.grid * batch <= e.n_cus)
    p.route = Route::Persist;  // icp_persist needs every workgroup resident at once: one 768-thread workgroup per CU is all a CU holds
  else if (sharded_in_kernel && o.shard_p2p && e.p2p_attached)
    p.route = Route::P2p;
  else if (sharded_in_kernel && o.shard_tail && xch_level1(batch, p.grid) <= kXchRowsMax * 2 * kRowGranules)
    p.route = Route::Tail;
  else if (o.xcd_fold && !o.persistent && one_launch_join && p.qpt == 1)
    p.route = Route::Fold;  // (as icp_persist except residency: the leaders only wait for workgroups of their own launch, which all run to completion)
  p.flags_in_box = p.route == Route::P2p && flags_fit;
  return p;
}

// May the launch sequence go as a captured graph?  With a communicator the RCCL calls are captured only on request (option
// "comm_graph"); a host-staged transport makes a host round trip per round: never capturable; over the peer mailboxes with
// the flags in them nothing of the registration is a collective or a host step: it is captured like a single-GPU one (the
// tags come from Job::p2p_epoch, not from a kernel argument).
// queued_behind: the stream is known to be busy with an earlier registration.  A graph launch costs the QUEUE ~8 us more
// than the same kernels launched one by one (markers around the graph: 234 vs 229 us per streamed registration) but costs
// the HOST less, so a registration that would start at once goes as a graph (its first kernel starts sooner: 300 vs 307 us
// submit-to-result) and one that has to wait for its predecessor anyway goes kernel by kernel.
// allow_graph: the caller's veto (pointers in the Jobs that differ per call, buffers a capture would bake)
inline bool graph_ok(const Plan& p, const Options& o, const PlanEnv& e, bool queued_behind, bool allow_graph) {
  const bool capturable = p.flags_in_box || (!e.host_transport && (!e.rccl || o.comm_graph) && p.route != Route::P2p);
  return allow_graph && o.use_graph && capturable && !(queued_behind && o.eager_when_busy && (!e.rccl || p.flags_in_box));
}

// Do a streamed registration's results go out through the device-resident outbox and icp_publish on the side stream?  Not
// when the completion is an event on the compute stream or the loop is sharded (its matched flags are reduced behind
// icp_final) — or the rounds need the whole chip to themselves: icp_persist / the xcd_fold variant wait INSIDE a launch for
// workgroups that must all be resident, at 3 x 168 registers per SIMD lane nothing fits beside them, and an icp_publish
// workgroup that got its CU first (the compute stream is still waiting for the feed) would keep one of them out until their
// bounded waits expire
inline bool side_publish(const Plan& p, const Options& o, const PlanEnv& e) {
  return o.publish_side && o.seq_completion && (!e.sharded() || p.flags_in_box) && p.route != Route::Persist && p.route != Route::Fold;
}

// ---- what a captured launch sequence bakes in: the whole plan, the Job array it works on, the communicator ------------------
struct GraphKey {
  Plan plan;
  int slot;   // which device Job array: -1 the batch's, >= 0 that stream slot's
  bool comm;  // a communicator is installed (its calls, or none, are in the sequence)
  bool operator<(const GraphKey& o) const { return std::make_tuple(plan.tie(), slot, comm) < std::make_tuple(o.plan.tie(), o.slot, o.comm); }
};

}  // namespace madicp
