/* madicp_hip.h — C ABI of libmadicp_hip.so: the MI355X (gfx950) implementation of MAD-ICP's
 * data-association + registration hot path.
 *
 * This is the boundary the host C++ classes (mad_icp_amd/csrc/host: MADtree, MADicp, Pipeline) bind to,
 * and what a reference maintainer would bind to from mad_icp/src.  Plain pointers
 * and sizes only; no C++/torch types; no exceptions cross it.
 *
 * Conventions
 *   - every call returns 0 on success, <0 on error; madicp_last_error() gives the message of the last
 *     failing call on the calling thread.
 *   - host buffers are owned by the caller, device buffers by the library (referred to by integer ids).
 *   - 3x3 rotations / 6x6 matrices cross the ABI ROW-major; a pose is 12 doubles: R (9, row-major), t (3).
 *     (The reference holds them as column-major Eigen objects; the host classes convert.)
 *   - clouds are (N,3) float64, C-contiguous — the memory layout of std::vector<Eigen::Vector3d>
 *     (mad_icp/src/tools/mad_tree.h:42, mad_icp/src/pybind/eigen_stl_bindings.h:73-81).
 *   - all arithmetic on the path is IEEE fp64 with the reference's operation order and no FMA contraction,
 *     so descent/gate decisions are bit-identical to the CPU path.
 *   - a context is bound to one device and owns two streams: the compute stream (the caller's, or its own) carries the
 *     registrations, an internal copy stream feeds them (tree uploads, the next scan's leaves).  Calls on one context
 *     are not re-entrant and must come from one host thread at a time.
 *   - "synchronous on return" below means: the caller's HOST buffers are no longer referenced and every output
 *     argument is filled.  Uploads, transforms and releases return as soon as the host buffer has been staged; the
 *     device work behind them is ordered by events, never by a device-wide synchronisation, and nothing on the
 *     registration path allocates or frees device memory (pooled buffers, grow-only staging).
 */
#ifndef MADICP_HIP_H
#define MADICP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MADICP_OK 0
#define MADICP_ERR_INVALID (-1)   /* bad argument / unknown id            */
#define MADICP_ERR_DEVICE (-2)    /* HIP runtime error (no device, OOM …) */
#define MADICP_ERR_COMM (-3)      /* collective error: RCCL failure, a host transport's error, or a collective that did
                                     not complete within "comm_timeout_ms" (the communicator is then aborted)      */
#define MADICP_ERR_CAPACITY (-4)  /* more trees / scans than the ABI caps */
#define MADICP_ERR_TIMEOUT (-5)   /* a bounded host wait ("wait_timeout_ms") ran out; the work is still in flight */

#define MADICP_MAX_TREES 128 /* keyframe trees one registration may reference (reference README suggests 16) */
#define MADICP_MAX_BATCH 64  /* scans in flight in one batched registration                                  */

/* One MAD-tree node, 64 bytes, nodes stored in DFS preorder (left child = this + 1).
 * Replaces the heap-allocated `struct MADtree` (mad_icp/src/tools/mad_tree.h:47-102): only the fields the
 * hot path reads are kept — mean_ (:96), the split axis eigenvectors_.col(2) for internal nodes
 * (mad_tree.cpp:147-148) or the normal eigenvectors_.col(0) for leaves (mad_icp.cpp:65), bbox_(0)
 * (mad_icp.cpp:97) and the child links. */
typedef struct madicp_node {
  double mean[3]; /* internal: centroid; leaf: the surface point nearest to it (mad_tree.cpp:76-86) */
  double dir[3];  /* internal: split-plane normal (col 2); leaf: surface normal (col 0)             */
  int32_t right;  /* internal: index of the right child minus own index (>= 2); leaf: 0            */
  int32_t leaf_id;/* leaf: ordinal in getLeafs() order (mad_tree.cpp:154-163); internal: -1         */
  double bbox0;   /* bbox_(0): extent along the normal                                              */
} madicp_node;

/* MADicp constructor arguments (mad_icp/src/odometry/mad_icp.cpp:31-32).  rho_ker is passed as the user
 * gives it; the library takes the square root exactly where the reference constructor does. */
typedef struct madicp_icp_params {
  double min_ball; /* = b_max of the fixed trees (pipeline.cpp:52, mad_icp_wrapper.h:59) */
  double rho_ker;
  double b_ratio;
} madicp_icp_params;

typedef struct madicp_ctx madicp_ctx;

const char* madicp_last_error(void);
/* ABI version: bumped on any incompatible change. */
int madicp_abi_version(void);

/* ---- context ------------------------------------------------------------------------------------ */
/* stream: a hipStream_t created by the caller (e.g. torch's current stream) or NULL to let the library
 * create its own non-blocking stream on `device_id`. */
int madicp_ctx_create(int device_id, void* stream, madicp_ctx** out);
int madicp_ctx_destroy(madicp_ctx* ctx);
int madicp_ctx_synchronize(madicp_ctx* ctx);
/* Tuning knobs (all optional): key in {"grid_blocks_per_cu" (1..4), "use_graph" (0/1), "queries_per_lane" (1,2),
 * "cache_correspondences" (0/1: reuse a correspondence in later GN rounds when it is provably unchanged),
 * "cache_gate" (0/1, default 1: a pair that keeps its leaf and was rejected by the gate of mad_icp.cpp:81-83 with more slack than it
 * has moved since is not evaluated again — its leaf record is not fetched; the same decisions either way, and the same bits
 * wherever the pairs are added in scan order (every launch but the leaf-major rounds of a batch, which add their walkers last)),
 * "leaf_major" (0: never; n > 0, default 8192: when a batch shares the chip — more keyframe trees than workgroups per XCD piece —
 * every workgroup gets one range of the scan's leaves and all the trees of its piece, and a round that follows one in which the
 * workgroup walked fewer than n nodes per pass runs LEAF-MAJOR: the moving leaf is read and transformed once per pass for all
 * those trees, and the pairs that still have to walk are queued per wavefront and walked densely.  H and b come out in another
 * summation order (~1e-16 relative), so the poses of later rounds differ by as much: the decisions — leaf, depth, gate, matched
 * flags, visit count — are the same except where a pair sits exactly on a split plane or on the gate's radius (equal on every
 * data set of the test suite, asserted there; not a structural guarantee)),
 * "publish_side" (0/1, default 1: a streamed registration leaves its results in a device-resident outbox and a one-workgroup
 * kernel on a side stream carries them, and the matched flags, to the caller's pinned block while the compute stream is already
 * running the next registration — the two PCIe round trips of that hand-over were 5 us of every registration; off: the
 * closing kernel writes them itself),
 * "deal_trees" (0/1/2, default 2: a registration lists the caller's trees dealt over the eight XCD pieces of the round kernel —
 * neighbours in the caller's list, e.g. keyframes along a trajectory, cost a given scan about the same, and with them in one
 * piece one XCD worked while seven waited; 1 = round-robin, 2 = rows of eight in alternating direction, so that the piece that
 * drew the newest (dearest) keyframe of one row draws the oldest of the next; results keep the caller's indices),
 * "interleave_ranges" (0/1/2, default 2: the ranges a scan's leaves are cut into for the workgroups are every n-th group of 64
 * leaves instead of contiguous stretches — a stretch of the leaf order is a stretch of space, and stretches differ several-fold
 * in how many of their pairs pass the gate: the launch waited for the workgroups that drew the busy stretch; 1 = only in batches
 * that share the chip, 2 = every launch.  Another summation order for H and b (~1e-16), the same decisions),
 * "deep_min_leaves" (default 512: from 24 keyframes on with two or more scans in flight — from 48 on with one — a launch with more
 * trees than workgroups per XCD piece gives every workgroup one range of the scan and all the trees of its piece as soon as a range
 * holds this many leaves; otherwise the rule stays two passes of a workgroup, 1536 leaves — measured, profiles/r6_deep_threshold.md),
 * "units_per_workgroup" (1..64, default 1: with more trees than workgroups per scan, cut the leaves into enough ranges for at
 * least this many (tree, range) units per workgroup; measured: no gain),
 * "lds_stage_min_leaves" (a workgroup copies a tree's top levels into LDS when its unit holds at least this many leaves),
 * "nn_lds_top" (0/1: madicp_nn_search batches of >= 16 k queries stage the tree's top levels in LDS; default 0, measured
 * slower for single launches), "comm_graph" (0/1: with a communicator, capture the per-round RCCL all-reduces into the registration's hipGraph
 * instead of launching the rounds eagerly), "eager_when_busy" (0/1, default 1: a registration queued behind another one is
 * launched kernel by kernel instead of as a hipGraph — measured 5 us per registration cheaper on the queue),
 * "seq_completion" (0/1, default 1: a streamed registration publishes its completion through a sequence number in the
 * pinned result block that madicp_stream_collect polls, instead of an event on the stream), "host_feed_wait" (0/1,
 * default 1: while another registration is in flight the HOST waits for a streamed scan's upload before it launches the
 * rounds, so no barrier packet sits between two registrations), "wait_mode" (how madicp_stream_collect and
 * madicp_tree_build wait for the device's sequence number: 0 = spin on the calling core (default: lowest latency), 1 =
 * sched_yield between polls, 2 = sleep ~50 us between polls (a drop-in odometry process that has other threads to run)),
 * "wait_timeout_ms" (0 = unbounded, default; otherwise such a wait returns MADICP_ERR_TIMEOUT when it runs out — the
 * ticket stays collectable), "match_all_rounds" (0/1, default 0: the matched flags of a registration are
 * the OR over ALL its rounds instead of the last round's — what the reference's Pipeline leaves behind when its realtime
 * check ends the loop before iteration MAX_ICP_ITS - 1, the only one that resets them: pipeline.cpp:167-176),
 * "persistent" (0/1, default 0: all rounds of a single-GPU registration as ONE launch; bit-identical, measured slower —
 * profiles/r3_b_persist_negative.md), "shard_split" (0/1/2, default 1: with a communicator, a batch of >= 4 scans (2: of >= 2
 * scans) runs as two halves on two streams, so that one half's per-round all-reduce is in flight under the other half's round
 * kernel; collectives are enqueued in one order on every rank — the option decides how many collectives a round makes, so it MUST
 * have the same value on every rank of the communicator, as must the batch sizes the ranks submit), "shard_tail" (0/1, default 0: the sharded round kernel leaves
 * the rank's adders itself instead of a separate icp_reduce launch; bit-identical, measured slower —
 * profiles/r4_c_shard_probe.md), "xcd_fold" (0/1, default 0: per-round launches with the XCD-hierarchical join at the
 * end of each launch; bit-identical, measured slower — profiles/r3_j_xcd_fold_negative.md), "upload_f32" (0/1, default 1: a cloud
 * handed to madicp_cloud_upload / madicp_tree_build_begin whose coordinates are ALL exactly floats — what a sensor driver, a KITTI
 * .bin or a PointCloud2 delivers — crosses PCIe as floats and is widened on the device: the same doubles bit for bit, half the
 * transfer in front of the builder's first kernel; any other cloud goes as doubles), "comm_timeout_ms" (default 60000: with a communicator, how long the host waits for a
 * registration's collectives before it aborts the communicator and returns MADICP_ERR_COMM)}. */
int madicp_ctx_set_option(madicp_ctx* ctx, const char* key, int64_t value);
/* the current value of one of the keys above (a caller that changes an option of a context it shares puts it back) */
int madicp_ctx_get_option(madicp_ctx* ctx, const char* key, int64_t* out_value);

/* ---- MAD-tree (fixed side) ---------------------------------------------------------------------- */
/* Upload a linearised tree.  Replaces keeping `MADtree*` alive in Frame::tree_ (frame.h:47).  The node array is
 * validated first (DFS-preorder structure, child links inside their parent's extent, leaf ordinals unique and in
 * range): a malformed array is MADICP_ERR_INVALID, never an out-of-bounds access.  Returns once `nodes` has been
 * staged; the copy and the build of the screening records run on the context's copy stream. */
int madicp_tree_upload(madicp_ctx* ctx, const madicp_node* nodes, int32_t n_nodes, int32_t n_leaves, int* out_tree_id);
/* The same for an array whose structure the PRODUCER guarantees — madicp_host_tree_build's output (csrc/host/
 * tree_builder.cpp), which is what the host MADtree / Pipeline classes upload once per scan — so that the O(n) host
 * validation pass (0.25 ms of a 2.9 ms drop-in frame at 45 k nodes) is not paid per frame.  rho2 = max |mean_i - mean_0|_2
 * over the internal nodes with finite means (madicp_tree_upload computes it while validating; the builder while
 * numbering the leaves).  No check beyond n_nodes == 2 n_leaves - 1: a malformed array here is undefined behaviour
 * on the device.  Arrays from anywhere else go through madicp_tree_upload. */
int madicp_tree_upload_trusted(madicp_ctx* ctx, const madicp_node* nodes, int32_t n_nodes, int32_t n_leaves, double rho2,
                               int* out_tree_id);
int madicp_tree_release(madicp_ctx* ctx, int tree_id);
int madicp_tree_download(madicp_ctx* ctx, int tree_id, madicp_node* out_nodes, int32_t n_nodes);
/* MADtree::applyTransform (mad_tree.cpp:165-172): mean <- R mean + t, dir <- R dir on every node.  Stream-ordered
 * behind every registration enqueued so far; no host synchronisation. */
int madicp_tree_transform(madicp_ctx* ctx, int tree_id, const double R[9], const double t[3]);
/* Batched MADtree::bestMatchingLeafFast (mad_tree.cpp:144-152) as used by MADtreeWrapper::search /
 * searchCloud / searchCloudDist (mad_tree_wrapper.h:42-67).  queries: host (n,3).  Any output may be NULL.
 * out_leaf_id = getLeafs() ordinal, out_node = index into the node array, out_dist = |q - leaf.mean|,
 * out_depth = internal nodes visited. */
int madicp_nn_search(madicp_ctx* ctx, int tree_id, const double* queries, int64_t n, uint32_t* out_leaf_id,
                     uint32_t* out_node, double* out_dist, int32_t* out_depth);
/* Same with queries / outputs already resident on the device (device pointers), asynchronous. */
int madicp_nn_search_device_enqueue(madicp_ctx* ctx, int tree_id, const double* d_queries, int64_t n,
                                    uint32_t* d_out_leaf_id, uint32_t* d_out_node, double* d_out_dist,
                                    int32_t* d_out_depth);

/* ---- moving side -------------------------------------------------------------------------------- */
/* MADicp::setMoving (mad_icp.cpp:53-55): the sensor-frame means of the current scan's leaves, (L,3). */
int madicp_moving_upload(madicp_ctx* ctx, const double* leaf_means, int32_t L, int* out_moving_id);
/* The next scan into the SAME buffers (grow-only: no allocation, free or synchronisation in steady state).  A set's buffers
 * hold (L + L / 8) leaves rounded up to a multiple of 256: a scan more than one eighth larger than the largest before it
 * re-allocates them (and the correspondence cache with them), a smaller one uses their head.  Either way a registration's
 * outputs — X, H, b, matched flags, X_iters, visits, counts — are a function of its arguments and the resident trees alone,
 * bit for bit, whatever the set, the stream slot or the context held before (tests/test_gpu_registration_history.py). */
int madicp_moving_update(madicp_ctx* ctx, int moving_id, const double* leaf_means, int32_t L);
/* The same on the library's COPY stream: the transfer runs beside the batch the compute stream is working on — one that reads
 * OTHER moving sets — instead of behind it.  Ordered by the library: the transfer waits for the last registration that read
 * this set, the next registration that reads it waits for the transfer.  (Two sets of moving ids used alternately: the upload
 * of batch i + 1 hides under batch i.) */
int madicp_moving_update_async(madicp_ctx* ctx, int moving_id, const double* leaf_means, int32_t L);
int madicp_moving_release(madicp_ctx* ctx, int moving_id);

/* ---- registration ------------------------------------------------------------------------------- */
/* One linearisation at a given pose, no state update: resetAdders + update() over K trees
 * (mad_icp.cpp:43-51,74-103 under pipeline.cpp:178-183).  out_H (36, row-major) and out_b (6) are the
 * summed adders; out_corr (K*L, optional) gets for tree k / moving leaf i the NN leaf ordinal, with bit 31
 * set when the gate at mad_icp.cpp:81-83 rejected the pair; out_matched (L, optional) the OR over trees of
 * the accepted pairs; out_visits (optional) the total number of internal nodes visited. */
int madicp_icp_linearize(madicp_ctx* ctx, int moving_id, const int* tree_ids, int K, const double X[12],
                         const madicp_icp_params* params, double out_H[36], double out_b[6], uint32_t* out_corr,
                         uint8_t* out_matched, uint64_t* out_visits);

/* The whole GN loop on the device, no host round trip between iterations: n_iters rounds of
 * {resetAdders; update() over the K trees; updateState()} — pipeline.cpp:166-193 and
 * mad_icp_wrapper.h:72-81.  X is MADicp::X_ (in: initial guess, out: estimate); out_H/out_b are
 * MADicp::H_adder_/b_adder_ of the LAST round (pipeline.cpp:223 reads H_adder_); out_matched (L, optional)
 * are the matched_ flags of the last round (cleared before it, pipeline.cpp:172-176);
 * out_X_iters (n_iters*12, optional) the pose BEFORE each round. */
int madicp_icp_register(madicp_ctx* ctx, int moving_id, const int* tree_ids, int K, double X[12],
                        const madicp_icp_params* params, int n_iters, double out_H[36], double out_b[6],
                        uint8_t* out_matched, double* out_X_iters, uint64_t* out_visits);

/* n_scans independent registrations against the same K trees, advanced in lock-step by the same
 * launches (BASELINE config 5: scans batched in flight).  X: n_scans*12, out_H: n_scans*36,
 * out_b: n_scans*6, out_n_matched: n_scans (count of matched leaves of the last round). */
int madicp_icp_register_batch(madicp_ctx* ctx, int n_scans, const int* moving_ids, const int* tree_ids, int K,
                              double* X, const madicp_icp_params* params, int n_iters, double* out_H,
                              double* out_b, int32_t* out_n_matched, uint64_t* out_visits);

/* Asynchronous form for throughput measurement: everything stays on the device; results are fetched
 * later with madicp_icp_fetch (which synchronises).  X0: n_scans*12 initial guesses (copied on call). */
int madicp_icp_register_batch_enqueue(madicp_ctx* ctx, int n_scans, const int* moving_ids, const int* tree_ids,
                                      int K, const double* X0, const madicp_icp_params* params, int n_iters);
int madicp_icp_fetch(madicp_ctx* ctx, int n_scans, double* out_X, double* out_H, double* out_b,
                     int32_t* out_n_matched, uint64_t* out_visits);
/* matched_ flags of scan `scan` of the last batch (L bytes). */
int madicp_icp_fetch_matched(madicp_ctx* ctx, int scan, uint8_t* out_matched, int32_t L);
/* Batches in flight, results out without a stream synchronisation: madicp_icp_publish_enqueue puts ONE small kernel behind the
 * batch that was enqueued last; it carries the batch's X / H / b / counts to a pinned host block and releases a sequence
 * number.  madicp_icp_publish_collect(ticket) waits for that number (bounded like madicp_stream_collect: "wait_mode",
 * "wait_timeout_ms", "comm_timeout_ms") and copies the results out — whenever the caller likes, typically after it has uploaded
 * (madicp_moving_update_async) and enqueued the NEXT batch.  A ring of four result blocks: a ticket must be collected before
 * the fourth batch after it is published.  Only MADICP_ERR_TIMEOUT keeps the ticket (the batch is still in flight: collect it
 * again); every other error of madicp_icp_publish_collect is terminal and releases the ticket and its block, like a success. */
int madicp_icp_publish_enqueue(madicp_ctx* ctx, int n_scans, int* out_ticket);
int madicp_icp_publish_collect(madicp_ctx* ctx, int ticket, int n_scans, double* out_X, double* out_H, double* out_b,
                               int32_t* out_n_matched, uint64_t* out_visits);

/* ---- streamed registrations: new scan in -> X / H / b / matched flags out --------------------------- */
/* What Pipeline::compute does per frame (pipeline.cpp:154-204), as one asynchronous submission: setMoving(leaf_means),
 * init(X0), n_iters rounds against K resident trees, and the read-out of X_, H_adder_, b_adder_, the matched_ flags and
 * their count.  The leaves and the job description are fed on the copy stream (they overlap the registration in
 * flight), the results are written by the registration's last kernel straight into pinned host memory, a sequence
 * number last, and madicp_stream_collect polls that number (spinning on the calling thread until the registration has
 * finished; an event instead with option "seq_completion" = 0).  Up to 4 tickets may be outstanding; collect them in any order before
 * their slot is needed again (MADICP_ERR_CAPACITY otherwise).  Bit-identical to madicp_icp_register on the same inputs.
 * A submission sizes its own slot AND every idle slot of the ring for its L and K (the capacity rule of
 * madicp_moving_update): the first submission sizes the whole ring, a later one re-allocates only where a scan outgrew a
 * slot — a slot with a ticket pending is left alone and is sized by the next submission that finds it idle. */
int madicp_stream_submit(madicp_ctx* ctx, const double* leaf_means, int32_t L, const int* tree_ids, int K,
                         const double X0[12], const madicp_icp_params* params, int n_iters, int* out_ticket);
/* The same with the moving set taken from a tree that is already resident: the scan's own MAD-tree, uploaded for the
 * frame window (pipeline.cpp:140-144: current_leaves_ ARE its leaves, in getLeafs() order, sensor frame). */
int madicp_stream_submit_tree(madicp_ctx* ctx, int moving_tree_id, const int* tree_ids, int K, const double X0[12],
                              const madicp_icp_params* params, int n_iters, int* out_ticket);
/* Any output may be NULL; out_matched holds L bytes. */
int madicp_stream_collect(madicp_ctx* ctx, int ticket, double out_X[12], double out_H[36], double out_b[6],
                          uint8_t* out_matched, int32_t* out_n_matched, uint64_t* out_visits);

/* (Measurement and test aids — madicp_icp_time_*, madicp_nn_time_descend, madicp_debug_* — are declared in
 * include/madicp_hip_measure.h: exported by the same library for bench.py and tests/, not part of the drop-in boundary.) */

/* ---- device front-end: scans resident in HBM, ingest + deskew, MAD-tree build (row f-1) -- */
/* Additive (the reference has no such interface: its Pipeline takes a host vector and builds on the CPU).  A "cloud" is
 * an (n,3) float64 scan in device memory, referred to by id.  Everything here runs on the context's copy stream, i.e.
 * concurrently with a registration in flight; results are handed to the compute stream by events. */
int madicp_cloud_upload(madicp_ctx* ctx, const double* xyz, int64_t n, int* out_cloud_id);
int madicp_cloud_release(madicp_ctx* ctx, int cloud_id);
int madicp_cloud_size(madicp_ctx* ctx, int cloud_id, int64_t* out_n);
int madicp_cloud_download(madicp_ctx* ctx, int cloud_id, double* out_xyz, int64_t n);
/* apps/cpp_runners/bin_runner.cpp:126-166: float32 records (x, y, z, intensity ...; `stride_floats` floats apart) ->
 * fp64 points in input order, dropping |p| < min_range, |p| > max_range (|p| in float, as there) and NaN coordinates;
 * kitti_correction != 0 applies the VERTICAL_ANGLE_OFFSET rotation of :153-158.  Synchronises once (the number of
 * surviving points sizes the cloud). */
int madicp_cloud_ingest_f32(madicp_ctx* ctx, const float* records, int64_t n_records, int stride_floats, double min_range,
                            double max_range, int kitti_correction, int* out_cloud_id, int64_t* out_n);
/* Pipeline::deskew (mad_icp/src/odometry/pipeline.cpp:79-123) in place: azimuth sort, then every point moved by the pose
 * of its time chunk.  velocity = naive_vel of :82-86 ([translation; logMapSO3(rotation)] of T_prev^-1 T_now, divided by
 * the scan period), which the caller computes (six numbers, host libm like the reference); the thresholds, times and
 * chunk poses are tabulated on the host with the reference's own running arithmetic.  The cloud ends up in azimuth
 * order, like the reference's.  Points whose azimuths tie exactly may come out in a different order than std::sort
 * leaves them (it is not stable), and the device atan2 may differ from libm's in the last bit: the result is the
 * reference's up to the order of such ties.  out_chunks (n, optional): the time chunk of every point in walk order
 * (largest azimuth first) — synchronises when given.  A cloud that carries stamps (madicp_cloud_ingest_records) LOSES them
 * here: the points are sorted, the stamps would no longer line up.  An attribute column (madicp_cloud_set_attr, below) is KEPT:
 * it is re-ordered with the points. */
int madicp_cloud_deskew(madicp_ctx* ctx, int cloud_id, const double velocity[6], double sensor_hz, int32_t* out_chunks);
/* Motion compensation from PER-POINT TIMESTAMPS, for callers whose driver delivers them (a PointCloud2 `t` / `timestamp` /
 * `time` field): additive, the reference has no such path — its azimuth guess above fits a single 360-degree head that starts
 * at +pi and turns clockwise, and nothing else.  stamps01[i] is the acquisition time of point i normalised over the scan, 0 =
 * start, 1 = end.  Same time model as madicp_cloud_deskew: 1024 chunk times t_0 = -1/hz, t_{k+1} = t_k + (1/hz)/1023, one pose
 * [expMapSO3(omega t_k), v t_k] per chunk from the same host table.  Chunk of a point, in fp64 without contraction: NaN -> 1023
 * (time unknown: taken as the scan's end, the frame the pose refers to); else q = floor(s * 1023 + 0.5), q <= 0 -> 0,
 * q >= 1023 -> 1023 (covers +-inf and out-of-range stamps), otherwise (int)q.  out[i] = pose[k_i] * p[i]: the cloud KEEPS ITS
 * INPUT ORDER (nothing is sorted), written to a fresh buffer like the azimuth path's.  One streaming kernel on the copy
 * stream; the stamps cross PCIe through the context's pinned staging.  MADICP_ERR_INVALID — before anything is launched or
 * allocated — for a null argument, an unknown cloud, n != the cloud's size, sensor_hz <= 0; MADICP_ERR_CAPACITY while a
 * look-ahead build is in flight; the cloud is unchanged after either.  out_chunks (n, optional): the chunk of every point in
 * input order — synchronises when given.  Bit-equal to madicp_host_deskew_stamped (madicp_host.h) for the same velocity. */
int madicp_cloud_deskew_stamped(madicp_ctx* ctx, int cloud_id, const double* stamps01, int64_t n, const double velocity[6],
                                double sensor_hz, int32_t* out_chunks);
/* RAW POINT RECORDS WITH A TIME FIELD — what a LiDAR driver actually delivers: a PointCloud2-style byte buffer of records
 * `point_step` bytes apart, little-endian float32 x / y / z at byte offsets, and a `t` / `time` / `timestamp` field of uint32,
 * float32 or float64.  Additive.  madicp_cloud_ingest_records takes such a buffer to a resident, range-filtered cloud that
 * CARRIES ITS OWN normalised stamps (a device buffer owned by the cloud, pooled like the points, released with it), and
 * madicp_cloud_deskew_own_stamps motion-compensates by them: the stamps never cross PCIe as doubles.  Everything in fp64
 * without contraction:
 *   survivors     madicp_cloud_ingest_f32's rule on the three floats read from off_x / off_y / off_z: float norm
 *                 sqrtf(x*x + (y*y + z*z)) compared in double, ON a bound stays, NaN coordinates dropped, the same KITTI
 *                 rotation, input order kept — the same points, bit for bit, as madicp_cloud_ingest_f32 gives for the (n,3)
 *                 float32 view of the same coordinates.
 *   time          t64 = (double)field, exact for all three types.
 *   range         t_range == NULL: t0 / t1 = min / max of t64 over ALL records with a FINITE time, dropped ones included (the
 *                 reference's apps/utils/point_cloud2.py:90-93 takes the whole message; ignoring non-finite values is an
 *                 addition — one NaN would poison its np.min), each canonicalised as t + 0.0 (a -0.0 extreme becomes +0.0);
 *                 +inf / -inf when no record has a finite time.  Else {t_begin, t_end}, both finite with t_end > t_begin.
 *   stamp         s = (t64 - t0) / (t1 - t0); every stamp NaN unless t1 - t0 > 0 (all times equal, no finite time): the
 *                 chunk rule below sends NaN to chunk 1023, the scan's end.  +-inf and values outside [0, 1] are left as
 *                 IEEE produces them; the chunk rule clamps them.
 * out_n: the survivors; out_t_range (optional): the t0, t1 used — it travels with the one device-to-host copy of the survivor
 * count (one synchronisation, like madicp_cloud_ingest_f32).  With t_type == MADICP_T_NONE the cloud has no stamps, off_t is
 * ignored and out_t_range is +inf, -inf.  MADICP_ERR_INVALID — before anything is launched or allocated, no cloud created —
 * for a null argument, n_records outside 1 .. 2^30 - 1, point_step outside 12 .. 256, a field that does not lie inside
 * [0, point_step), an unknown t_type, a t_range that is not finite and increasing; MADICP_ERR_INVALID as well when no record
 * survives; MADICP_ERR_CAPACITY while a look-ahead build is in flight.  Bit-equal to madicp_host_ingest_records
 * (madicp_host.h).  (The call IS madicp_cloud_ingest_sources, below, for one plain source — R the identity, t zero, t_scale 1,
 * t_offset 0 — behind the refusals above: the same kernels, the same chain.) */
#define MADICP_T_NONE 0 /* time field types: sensor_msgs/PointField's own codes */
#define MADICP_T_U32 6
#define MADICP_T_F32 7
#define MADICP_T_F64 8
typedef struct madicp_record_layout {
  int32_t point_step;          /* bytes from one record to the next, 12 .. 256, ANY value (13, 22, 26 ... are legal) */
  int32_t off_x, off_y, off_z; /* byte offsets of the little-endian float32 coordinates, any alignment */
  int32_t off_t;               /* byte offset of the time field (ignored when t_type == MADICP_T_NONE) */
  int32_t t_type;
} madicp_record_layout;
int madicp_cloud_ingest_records(madicp_ctx* ctx, const void* data, int64_t n_records, const madicp_record_layout* layout,
                                double min_range, double max_range, int kitti_correction,
                                const double* t_range /* NULL: min / max over the records; else {t_begin, t_end} */,
                                int* out_cloud_id, int64_t* out_n, double out_t_range[2] /* optional */);
/* the stamps a cloud carries (n = the cloud's size), in the cloud's order; MADICP_ERR_INVALID when it has none: only clouds of
 * madicp_cloud_ingest_records with a time field do, and madicp_cloud_deskew — which SORTS the points — drops them */
int madicp_cloud_stamps(madicp_ctx* ctx, int cloud_id, double* out_stamps01, int64_t n);
/* madicp_cloud_deskew_stamped with the stamps read from the cloud's own device buffer: the same kernel, the same pose table, the
 * same refusals and out_chunks; MADICP_ERR_INVALID for a cloud without stamps.  The cloud keeps its stamps (input order is
 * kept). */
int madicp_cloud_deskew_own_stamps(madicp_ctx* ctx, int cloud_id, const double velocity[6], double sensor_hz, int32_t* out_chunks);
/* SEVERAL SENSORS' RECORDS INTO ONE CLOUD — a multi-head rig (two Ousters on one vehicle, each with its lidar_to_base) delivers
 * S buffers per frame: each in its own sensor frame, often with its own point_step and time type, each time field counting
 * from its own message header.  Additive.  madicp_cloud_ingest_sources takes the S buffers to ONE resident cloud in the base
 * frame with ONE set of normalised stamps, in one chain of launches and one host synchronisation whatever S is (all sources
 * cross PCIe in one copy).  The survivors of source 0 come first in input order, then source 1's, and so on; the cloud carries
 * stamps exactly when the sources have a time field, and madicp_cloud_stamps / madicp_cloud_deskew_own_stamps work on it
 * unchanged.  Per record, madicp_cloud_ingest_records' rules with two additions, everything in fp64 without contraction:
 *   survivors     the range filter on the raw floats IN THE SENSOR'S OWN FRAME, with that source's own min_range / max_range:
 *                 that is where self-hits and the maximum range are defined.
 *   common clock  tc = t64 * t_scale + t_offset (two roundings, no fma); a source with t_scale == 1.0 and t_offset == 0.0
 *                 exactly takes t64 as it is.  Finiteness is judged on tc.  t_range == NULL: t0 / t1 = min / max of tc over ALL
 *                 records of ALL sources with a finite tc, dropped ones included, each canonicalised as t + 0.0; else the
 *                 caller's {t_begin, t_end} ON THE COMMON CLOCK.  stamp = (tc - t0) / (t1 - t0), NaN unless t1 - t0 > 0.
 *                 PRECISION: pass t_offset relative to the frame's start, not an absolute epoch — an offset of 1.7e9 s leaves
 *                 tc a resolution of 2.4e-7 s and eats the nanoseconds of a uint32 field.
 *   sensor->base  after the optional KITTI rotation (which belongs to the sensor frame): base[i] = t[i] + (R[3i] * o0 +
 *                 (R[3i+1] * o1 + R[3i+2] * o2)) — the evaluation order of pose * point in madicp_cloud_deskew_stamped; a
 *                 source whose R is exactly the identity and whose t is exactly zero skips it.  R is used AS GIVEN: that it is
 *                 orthonormal is the caller's business (a scaled or sheared R scales or shears the points).
 * One source with the identity, t_scale 1 and t_offset 0 is what madicp_cloud_ingest_records passes on: the same bits.
 * out_n: all survivors; out_n_per_source (n_sources values, optional): those of every source (they ride in the same one
 * device-to-host copy); out_t_range (optional): the t0, t1 used, +inf, -inf without a time field or a finite time.
 * MADICP_ERR_INVALID — before anything is staged, launched or allocated, no cloud created — for a null argument (a source's
 * data included), n_sources outside 1 .. MADICP_MAX_SOURCES, an n_records < 1 or a total above 2^30, a layout
 * madicp_cloud_ingest_records refuses, a non-finite entry of R or t, a t_scale that is not finite and > 0, a non-finite t_offset,
 * sources with AND without a time field (all or none), a t_range that is not finite and increasing; MADICP_ERR_INVALID as well
 * when no record of any source survives; MADICP_ERR_CAPACITY while a look-ahead build is in flight.  The caller's buffers are
 * read up to data[n_records * point_step) and no further.  Bit-equal to madicp_host_ingest_sources (madicp_host.h). */
#define MADICP_MAX_SOURCES 8
typedef struct madicp_record_source {
  const void* data;
  int64_t n_records;             /* >= 1 */
  madicp_record_layout layout;
  double R[9], t[3];             /* sensor -> base, R row-major */
  double min_range, max_range;   /* in the sensor's frame */
  double t_scale, t_offset;      /* field units -> the common clock */
  int32_t kitti_correction, reserved;
} madicp_record_source;
int madicp_cloud_ingest_sources(madicp_ctx* ctx, const madicp_record_source* sources, int n_sources,
                                const double* t_range /* NULL: min / max over all records; else {t_begin, t_end} */,
                                int* out_cloud_id, int64_t* out_n, int64_t* out_n_per_source /* n_sources, optional */,
                                double out_t_range[2] /* optional */);
/* A PER-POINT ATTRIBUTE — every real record carries more than x y z t (intensity, reflectivity, ring, a label), and a consumer of
 * the exported scan or of the map wants it on the points it gets back.  Additive and default off.  The attribute is ONE 32-bit word
 * per point: the bytes of one named record field, little-endian, zero-extended to 32 bits.  Nothing converts, scales or interprets
 * it: a FLOAT32 keeps its bits (NaN payloads and -0.0 included), an INT16 of -1 is the word 0x0000ffff.  It belongs to the point
 * and travels with it: through the range filter and the compaction of the ingest, the merge of several sources, the re-ordering
 * of madicp_cloud_deskew (the column is replaced by its gather in the sorted order — unlike the stamps it is NOT dropped; the
 * stamped deskews keep input order and leave it alone), the voxel thinning of the export and the folds of a map.  A row's word is
 * its OWNING point's, the lowest index of its voxel: nothing is averaged.
 *   madicp_cloud_ingest_sources_attr  madicp_cloud_ingest_sources with `fields`, one per source: the cloud carries the column, filled
 *                                     by the same launches.  fields == NULL: no attribute — that IS madicp_cloud_ingest_sources.
 *                                     Further refusals (MADICP_ERR_INVALID, nothing staged): a field that does not lie inside
 *                                     [0, point_step) or whose type is none of MADICP_A_INT8 .. MADICP_A_FLOAT32, sources with
 *                                     AND without an attribute (type MADICP_A_NONE: all or none), differing types over the sources.
 *   madicp_cloud_set_attr             gives ANY resident cloud (madicp_cloud_upload ...) a column, or its column new words; n = the
 *                                     cloud's size.  Returns once `attr` has been staged.
 *   madicp_cloud_attr                 the column, in the cloud's order; MADICP_ERR_INVALID when the cloud carries none.
 *   madicp_cloud_export_f32_attr      madicp_cloud_export_f32 — the same rule, refusals and synchronisation count, the same rows —
 *                                     with out_attr[r] the word of row r (capacity_rows words).  MADICP_ERR_INVALID, nothing
 *                                     written, when the cloud carries no column.
 * Bit-equal to madicp_host_ingest_sources_attr / madicp_host_cloud_export_f32_attr (madicp_host.h). */
#define MADICP_A_NONE 0 /* attribute field types: sensor_msgs/PointField's own codes */
#define MADICP_A_INT8 1
#define MADICP_A_UINT8 2
#define MADICP_A_INT16 3
#define MADICP_A_UINT16 4
#define MADICP_A_INT32 5
#define MADICP_A_UINT32 6
#define MADICP_A_FLOAT32 7
typedef struct madicp_attr_field {
  int32_t offset; /* byte offset of the field in the record, any alignment */
  int32_t type;   /* MADICP_A_* */
} madicp_attr_field;
int madicp_cloud_ingest_sources_attr(madicp_ctx* ctx, const madicp_record_source* sources, int n_sources,
                                     const madicp_attr_field* fields /* n_sources, or NULL: no attribute */,
                                     const double* t_range, int* out_cloud_id, int64_t* out_n,
                                     int64_t* out_n_per_source /* n_sources, optional */, double out_t_range[2] /* optional */);
int madicp_cloud_set_attr(madicp_ctx* ctx, int cloud_id, const uint32_t* attr, int64_t n);
int madicp_cloud_attr(madicp_ctx* ctx, int cloud_id, uint32_t* out_attr, int64_t n);
/* A RESIDENT CLOUD OUT — what a mapping, loop-closure or visualisation consumer wants of a registered scan: the points in
 * another frame (the map's), as float32, thinned to one point per voxel.  Additive.  The rule, everything in fp64 without
 * contraction (one source for the device and the host twin: mad_icp_amd/csrc/common/export_point.h):
 *   position      q[i] = t[i] + (R[3i] * p0 + (R[3i+1] * p1 + R[3i+2] * p2)), R row-major — the evaluation order of pose * point in
 *                 madicp_cloud_deskew_stamped and of sensor->base above.  R is used AS GIVEN.
 *   output        (float)q[i], round to nearest even; overflow to +-inf as IEEE gives it.
 *   voxel == 0    every point goes out, in cloud order; nothing is dropped, NaN rows included: *out_n = the cloud's size.
 *   voxel > 0     cell per axis f = floor(q[i] / voxel), a true division.  A point is a CANDIDATE only if all three cells satisfy
 *                 -1048576.0 <= f < 1048576.0 — NaN and +-inf fail and the point is dropped.  Key = (kx + 2^20) | (ky + 2^20) << 21
 *                 | (kz + 2^20) << 42.  Of the candidates that share a key the one with the LOWEST INDEX in cloud order is kept;
 *                 kept points go out in ascending index order.  No candidate at all is MADICP_OK with *out_n = 0.
 * The result is a function of the input alone: no scheduling order shows in it, two calls give the same bytes.  The cloud — and
 * the stamps it may carry — is only read.  Runs on the copy stream in idle parts of the builder's scratch; at most two host
 * synchronisations (the row count, then the rows; voxel == 0: one).  MADICP_ERR_INVALID — before anything is launched or
 * allocated, nothing written — for a null argument, an unknown cloud, a non-finite entry of R or t, a voxel that is negative or
 * not finite.  MADICP_ERR_CAPACITY while a look-ahead build is in flight (nothing written), and when capacity_rows is smaller
 * than the rows needed: *out_n is that number and out_xyz is not written — call again with room for *out_n rows (the cloud's
 * size always suffices).  Bit-equal to madicp_host_cloud_export_f32 (madicp_host.h). */
int madicp_cloud_export_f32(madicp_ctx* ctx, int cloud_id, const double R[9], const double t[3], double voxel, float* out_xyz,
                            int64_t capacity_rows, int64_t* out_n);
int madicp_cloud_export_f32_attr(madicp_ctx* ctx, int cloud_id, const double R[9], const double t[3], double voxel, float* out_xyz,
                                 uint32_t* out_attr, int64_t capacity_rows, int64_t* out_n);
/* THE VOXEL MAP — what a mapping consumer wants of a drive, not of one scan: registered scans accumulated on the device into an
 * append-only set of float32 rows, one per voxel, of which the consumer fetches only what was added since it last looked.
 * Additive.  Per point the export's rule above, everything in fp64 without contraction (one source:
 * mad_icp_amd/csrc/common/export_point.h); the KEY of a point comes from its fp64 position, never from the float that is stored.
 * A map has a voxel size (finite, > 0: no "every point" mode), M rows and the set K of their M keys.  Folding a cloud of n points
 * through (R, t): point i is a CANDIDATE if all three cells are in range (as for the export), NEW if it is a candidate and its
 * key is not in K; of the new points that share a key the one with the LOWEST index is kept; kept points are appended as
 * (float)q[i] in ascending index order and their keys join K.  Rows are never changed or removed by a fold, so rows [0, M) after
 * any fold stay a prefix of the map until a prune or a clearing (madicp_map_prune, madicp_map_clear_rays, below), and the map is a function of the sequence of (cloud, pose) alone: launch
 * geometry, timing, initial_rows and the number of growths do not show.
 *   madicp_map_create        initial_rows >= 1 sizes the first block (44 bytes per row: float row, key, two table slots); blocks
 *                            grow geometrically up to 1 <= max_rows <= 2^30.  MADICP_ERR_INVALID for a null argument, a voxel
 *                            that is not finite or not > 0, rows out of those ranges.
 *   madicp_map_create_attr   the same map with a fifth column, the ATTRIBUTE word of every row (above: a per-point attribute): 48
 *                            bytes per row of capacity instead of 44.  madicp_map_insert_cloud appends the owning point's word
 *                            with its row, or the word 0 when the cloud carries no column; a growth moves the column with the
 *                            rows.  The rows are those of a map of madicp_map_create on the same folds, bit for bit.
 *   madicp_map_insert_cloud  folds a resident cloud, which is only read: *out_added rows were appended, the map holds *out_rows.
 *                            MADICP_ERR_CAPACITY, map unchanged, when rows + n > max_rows (conservative on purpose: decided
 *                            before any launch), and while a look-ahead build is in flight (the fold's scratch is the builder's).
 *                            MADICP_ERR_INVALID, nothing changed or written, for a null argument, an unknown id, a non-finite
 *                            entry of R or t.  One host synchronisation, for the count.
 *   madicp_map_size          the rows the map holds.
 *   madicp_map_download_f32  rows [first_row, rows) into out_xyz, their number in *out_n; MADICP_ERR_CAPACITY when capacity_rows
 *                            is smaller: *out_n is the number needed and out_xyz is not written (the export's convention);
 *                            MADICP_ERR_INVALID for a null argument, an unknown id, a first_row outside [0, rows].
 *   madicp_map_download_attr the words of rows [first_row, rows), madicp_map_download_f32's conventions; MADICP_ERR_INVALID as well
 *                            on a map made without the column, out_attr not written.
 *   madicp_map_clear         forgets the rows, keeps the block.     madicp_map_release  frees everything.
 *   madicp_map_prune         removes rows by RANGE: row j stays iff its STORED float row is within `radius` of `center` —
 *                            dx = (double)row[0] - center[0] ..., dx dx + (dy dy + dz dz) <= radius radius in fp64 without
 *                            contraction (export_point.h: map_row_kept); exactly `radius` stays, a row that fails the comparison
 *                            for any reason leaves.  Kept rows keep their relative order (a stable compaction), their keys and
 *                            attribute words move with them; the keys of removed rows leave K, so a later point of such a voxel
 *                            is new again and is appended at the end.  Keys are the stored ones, never recomputed from floats.
 *                            *out_removed rows left, the map holds *out_rows; watermark in [0, rows]: *out_watermark is the number
 *                            of kept rows among rows [0, watermark) — a consumer that had fetched rows [0, watermark) has fetched
 *                            exactly rows [0, *out_watermark) of the pruned map.  The block's capacity is unchanged.  The map stays
 *                            a function of the sequence of folds and prunes alone; a prune that removes nothing leaves every later
 *                            answer what it would have been.  MADICP_ERR_INVALID, map unchanged and nothing launched, for a null
 *                            argument, an unknown id, a non-finite center, a radius that is not finite and > 0 or whose square is
 *                            not finite, a watermark outside [0, rows].  An empty map answers 0, 0, 0.  The builder's scratch is
 *                            not touched (legal while a look-ahead build is in flight); transiently one more block of the map's
 *                            capacity, as for a growth.  One host synchronisation, whatever the size of the map.
 *   madicp_map_clear_rays    the OTHER call that removes rows: free-space clearing by the rays of a scan.  With qo and q[i] the
 *                            sensor origin and point i of the cloud taken into the map frame by (R, t) (the export's position rule),
 *                            d = q[i] - qo per axis and L = sqrt(dx dx + (dy dy + dz dz)), ray i is SAMPLED one voxel edge apart:
 *                            K = min(floor((L - margin) / voxel), 4096) samples if L is finite and L - margin >= voxel, else none;
 *                            sample k = 1 .. K is s = qo + d * f per axis, f = (k * voxel) / L — fp64 without contraction
 *                            (export_point.h: ray_length, ray_sample_count, ray_sample).  The candidate keys of the samples are
 *                            TRAVERSED, the candidate keys of the end points q[i] are OCCUPIED by this scan — also those of rays
 *                            that walk nothing (a NaN or infinite point has no key and protects nothing); a sample outside the
 *                            key range is skipped and the walk goes on.  Row j leaves iff its STORED key is traversed and not
 *                            occupied.  Sampling is not an exact voxel traversal — a ray can cut a corner between two samples —
 *                            and a ray ends 4096 samples from the origin: what lies beyond stays.  Kept rows, keys, attribute
 *                            words, the three answers and the watermark exactly as for madicp_map_prune; the result is a function
 *                            of (map, cloud, pose, origin, margin) alone.  The cloud is only read.  MADICP_ERR_INVALID, map
 *                            unchanged and nothing launched, for a null argument, an unknown id, a non-finite R, t or origin, a
 *                            margin that is not finite and >= 0, a watermark outside [0, rows].  An empty map or an empty cloud
 *                            answers 0, rows, watermark without a launch.  The builder's scratch is neither used nor grown (legal
 *                            while a look-ahead build is in flight, and in a context that has only seen small clouds);
 *                            transiently one more block of the map's capacity.  One host synchronisation, whatever M and n.
 * THE REMOVAL LOG — how a consumer that mirrors the map learns which rows have left.  A map is TRACKING REMOVALS or not (not: the
 * default, and everything above as it is: no launch, no allocation, no synchronisation more).  On a tracking map every
 * madicp_map_prune or madicp_map_clear_rays that removes rows appends the removed rows with index below `watermark` — exactly the
 * rows that the consumer who passed this watermark has fetched — to the map's removal log, in row order: one entry is the row's
 * stored key (uint64: unique among live rows, the identity a consumer can hold — an index moves at a prune, equal float rows can
 * have different keys), its three stored floats and, on a map with the attribute column, its word.  Removed rows at or above the
 * watermark are not logged: they were never delivered.  The call adds exactly watermark - *out_watermark entries, so the host
 * knows the log's length from answers it already reads: no new synchronisation.  The map after the call, the three answers and
 * the watermark are what they are without tracking, bit for bit; a removal that removes nothing logs nothing.  TAKING copies
 * all entries out, oldest first, and empties the log (its memory is kept); madicp_map_clear empties it too, madicp_map_release
 * frees it.  CAPACITY: a prune or a clearing on a tracking map whose log already holds >= max_rows entries is refused with
 * MADICP_ERR_CAPACITY, map and log unchanged, nothing launched, nothing written (decided without looking at a row, after the
 * arguments are found valid); before a launch, memory for log_n + min(watermark, rows) entries is ensured, so the log never
 * holds memory for more than 2 max_rows entries (20 bytes each, 24 with the column), in a block of its own that grows
 * geometrically.  THE INVARIANT: a consumer that keeps key -> (row, word), at every poll first deletes the taken log's keys (each
 * is present, within one poll they are distinct) and then inserts the new rows [its watermark, rows) by key (none is present),
 * holds exactly the device map, for any polling cadence.  Removals first: a voxel cleared and refilled between two polls is in
 * both lists.
 *   madicp_map_track_removed  on != 0: the map tracks removals from now on; 0: it does not, and the log is freed.  Legal at any
 *                             time.  MADICP_ERR_INVALID for a null ctx or an unknown id.
 *   madicp_map_removed_count  the entries the log holds (0 on a map that is not tracking).
 *   madicp_map_take_removed   all entries into out_keys (n), out_xyz (n, 3) and, where out_attr is not null, out_attr (n), their
 *                             number in *out_n; then the log is empty.  MADICP_ERR_CAPACITY when capacity is smaller: *out_n is
 *                             the number needed, nothing is written, the log is kept.  MADICP_ERR_INVALID, nothing written, for
 *                             a null argument (out_attr may be null), an unknown id, a map that is not tracking, an out_attr on
 *                             a map without the column.  All copies in front of ONE host synchronisation.
 *   madicp_map_download_keys  the stored keys of rows [first_row, rows), madicp_map_download_f32's conventions.
 *   madicp_map_download_rows  the columns of rows [first_row, rows) — out_xyz, and out_keys and out_attr where not null — with
 *                             their copies in front of ONE host synchronisation; madicp_map_download_f32's conventions, and
 *                             MADICP_ERR_INVALID for an out_attr on a map without the column.
 * EVIDENCE.  A map of madicp_map_create_ev keeps a hit/miss count per row: one more 32-bit word e, 1 <= e <= cap, under three
 * parameters fixed at creation, hit >= 1, miss >= 1, hit <= cap <= 2^31 - 1 (the rule, integers only, is
 * csrc/common/export_point.h's, shared with the host twin).  With N the candidate keys of a folded cloud:
 *   fold      a row the fold creates gets e = hit; a row that was there before the fold and whose stored key is in N gets
 *             e = min(e + hit, cap) — ONCE per fold, however many points fall into the voxel; other rows are not touched
 *   clearing  madicp_map_clear_rays: a row whose stored key is in T \ O is MISSED — e > miss: it stays with e - miss; else it
 *             leaves, through the same close-up, watermark and removal log as on a plain map.  Every row is covered, below and above
 *             the watermark; rows in O and rows not in T are not touched; the decrements hold even when no row leaves
 *   prune, growth: the word travels with its row; madicp_map_clear forgets it with the rows.  The removal log's entries carry none.
 * With hit = miss = cap = 1 the map is the plain map in every row, key, count and log entry.  A fold's hits are found by one more
 * kernel behind the claim (fe::map_hit: one lane per point, one elected per voxel and fold by an integer exchange on a stamp word
 * of the voxel's table slot), the misses by the mark kernel of the clearing itself (fe::map_clear_mark_ev, one lane per row): no
 * host synchronisation is added to either call, and the result is a function of the sequence of (cloud, pose) alone.
 *   madicp_map_create_ev            madicp_map_create's arguments, with_attr != 0 for the attribute column as well, and the three
 *                                   parameters; MADICP_ERR_INVALID for what map_evidence_refusal refuses.  The block gains the
 *                                   column ev (cap x 4 bytes) and two 32-bit words per table slot (the slot's row, the slot's fold
 *                                   stamp): 20 more bytes per row of capacity — 64 instead of 44, 68 instead of 48.
 *   madicp_map_download_evidence    the words of rows [first_row, rows), madicp_map_download_attr's conventions: *out_n set,
 *                                   MADICP_ERR_CAPACITY when capacity_rows is smaller, MADICP_ERR_INVALID on a map made without
 *                                   the column.  One host synchronisation.
 *   madicp_map_download_min_evidence the rows with e >= min_e, in row order, compacted on the device (a mark kernel, the tile scan
 *                                   and one gather into a transient block of the call's own; the builder's scratch is not
 *                                   touched): out_xyz, and out_keys, out_attr, out_ev where not null.  *out_n is always set to
 *                                   their number; MADICP_ERR_CAPACITY, nothing written, when capacity_rows is smaller;
 *                                   MADICP_ERR_INVALID on a map without the column or for an out_attr on a map without that
 *                                   one.  TWO host synchronisations: the count, then the rows (none on an empty map, one where
 *                                   no row qualifies or the buffer is short).
 * MOMENTS.  A map of madicp_map_create_mom keeps, per row, the count, the sums and the sums of products of every point that fell into
 * its voxel — ten unsigned 64-bit words n | S1[3] | S2[6] (xx, xy, xz, yy, yz, zz) over 16-bit offsets inside the voxel — and serves
 * a centroid and a PCA normal per row from them (the rule, the offsets, the surfel formula and why nothing can wrap:
 * csrc/common/voxel_moments.h, shared with the host twin).  One more creation parameter, max_count, 1 .. 2^31: a row takes ALL
 * candidate points of a fold that fall into its voxel iff its n before that fold is < max_count, the creating point included, else
 * none — it freezes at the end of the fold that brings it to or past max_count, whatever the order of arrival within the fold.
 *   fold      one more kernel behind the rows' scatter and in front of the fold's one wait (fe::map_moments: one lane per point; the
 *             lanes of a wavefront that fall into one voxel side by side add up in registers and issue ten 64-bit integer atomics
 *             together; the add on n returns, and the one that reaches max_count stamps the row's freeze word with the fold's
 *             ordinal): no host synchronisation is added, no float atomic is used, and the words are a function of the sequence
 *             of (cloud, pose) alone.  Moments never decide which rows exist: rows, keys, attribute, evidence and log
 *             are those of the same map without them.  The ordinal is a 32-bit count of the map's folds since creation or
 *             madicp_map_clear; the fold that would need ordinal 2^32 - 1 is refused with MADICP_ERR_CAPACITY
 *   prune, clearing, growth: the ten words and the freeze word travel with their row; madicp_map_clear forgets them with the rows.
 *             The removal log's entries carry NO moments: a consumer that wants a removed row's statistics reads them before.
 *   madicp_map_create_mom         madicp_map_create's arguments, with_attr != 0 for the attribute column, evidence = {hit, miss, cap}
 *                                 or null, and max_count; MADICP_ERR_INVALID for what map_evidence_refusal or map_moments_refusal
 *                                 refuse.  The block gains mom (cap x 80) and the freeze words (cap x 4), and the slot_row words of an
 *                                 evidence map where it has none: 84 more bytes per row of capacity, 92 on a map without evidence.
 *   madicp_map_download_moments   the ten words of rows [first_row, rows) as (rows, 10) uint64: madicp_map_download_f32's refusals,
 *                                 MADICP_ERR_INVALID on a map without moments.  One host synchronisation.
 *   madicp_map_download_surfels   per row of [first_row, rows): centroid (3 floats), and where not null the normal (3 floats, zero for
 *                                 n < 3, sign not part of the contract), the eigenvalues of the covariance in m^2, ascending
 *                                 (3 floats), and n as uint32 — computed on the device (fe::map_surfels, one lane per
 *                                 row, fp64) into a transient block: one kernel, one copy chain, ONE host synchronisation.  The same
 *                                 refusals.  Centroid and count are bit-equal to the host twin's; eigenvalues and normals go
 *                                 through atan2 / cos / sin and agree to the last bits only.  THE ZERO RULE: an eigenvalue that
 *                                 is not above 2^-24 of the largest plus 4 x 2^-52 max(S2_aa / n) — what the solve can tell
 *                                 from zero, measured (csrc/common/voxel_moments.h) — is delivered as +0.0: never negative, and
 *                                 identical or collinear points have eig1 == 0 whatever their rounding noise, which is what
 *                                 madicp_map_register_cloud's `eig1 > 0` refuses; an exact plane has eig0 == 0 < eig1.
 * QUERY.  Everything above writes the map or downloads it; madicp_map_query_cloud ASKS it, where it lives, what it holds at the
 * points of a resident cloud: per point the nearest row of its voxel neighbourhood.  The rule (one source with the host twin:
 * csrc/common/export_point.h — export_cells, query_cell_key, query_d2, query_before), fp64 and integers only, no library function,
 * so every output is bit-equal between device, host twin and a numpy restatement:
 *   point i goes through (R, t) by the export's position rule to q.  No candidate (a cell outside [-2^20, 2^20), NaN, infinite):
 *   row -1, d2 +inf, key all ones, words 0.  Else its NEIGHBOURHOOD is the cells cell + o, o in {-reach .. reach}^3, reach 0 or 1;
 *   a cell with an axis outside the key range is skipped, nothing wraps.  For every row j whose STORED key is the key of a cell of
 *   the neighbourhood: dx = q[0] - (double)row[0] ..., d2 = dx dx + (dy dy + dz dz) — madicp_map_prune's association, from the
 *   stored float row.  The answer is the row with the smallest (d2, j), lexicographically: a tie goes to the lower row index; no
 *   such row: as for no candidate.  A minimum does not depend on the order of its arguments: the result is a function of (map,
 *   cloud, pose, reach) alone, whatever the launch geometry.
 *   out_row (int32), out_d2 (float64), out_keys (uint64: the matched row's stored key), out_attr, out_ev (its words): n entries
 *   each, any of them null where not wanted — all five null is the SCORING form: only the counts come back.
 *   out_counts[3] (always): the points that are candidates, those with row >= 0, and those of them with d2 <= max_dist max_dist
 *   (the product in fp64; max_dist = +inf gives within == matched) — integer sums (per-wavefront ballots, integer atomics).
 *   madicp_map_query_cloud   MADICP_ERR_INVALID, nothing written and nothing launched, for a null ctx, R, t or out_counts, an
 *                            unknown id, a non-finite R or t, a reach other than 0 and 1, a max_dist that is NaN or negative, an
 *                            out_attr on a map without the attribute column, an out_ev on a map without the evidence column;
 *                            MADICP_ERR_CAPACITY, the same, when a per-point buffer is given and capacity_points < n.  An empty
 *                            cloud answers 0, 0, 0 without a launch.  The map is only read: every column, the table, the removal
 *                            log and every later answer are what they would be without the call.  Kernel: one lane per point, at reach 1
 *                            the 27 cells one after the other (fe::map_query_lanes; a form with 32 lanes per point was built and
 *                            measured slower, profiles/map_query_time.md); a
 *                            map without the slot-to-row column (plain and attribute maps: their 44 / 48 bytes per row do not
 *                            change) gets a transient one in the call's scratch first (fe::map_slot_rows, one lane per row).  The
 *                            scratch is the call's own, pooled: the builder's is not touched (legal while a look-ahead build is in
 *                            flight).  One host synchronisation, whatever n and M.
 * SCORING MANY POSES.  A relocalisation, a loop-closure search or a drift check has not one pose but a cloud of hypotheses;
 * madicp_map_score_poses gives the query's three counts at each of n_poses poses in ONE call.  The rule (one source with the host
 * twin: csrc/common/export_point.h — map_score_refusal, score_takes_part and the query's own functions):
 *   poses is (n_poses, 12) doubles: R row-major, then t — the first 12 entries of a row of madicp_map_register_cloud's out_trace.
 *   Point i TAKES PART iff i % stride == 0, stride >= 1: subsampling, a hypothesis search does not need every point.
 *   out_counts[3 k .. 3 k + 2] = {candidates, matched, within} are madicp_map_query_cloud's out_counts for the cloud of the points
 *   that take part, at pose k: the same position rule, candidate decision, neighbourhood, (d2, row) order and d2 <= max_dist
 *   max_dist in fp64.  Sums of integers: a function of (map, cloud, poses, reach, max_dist, stride) alone, whatever the launch
 *   geometry — bit-equal between device, host twin, a numpy restatement and n_poses separate scoring queries.
 *   madicp_map_score_poses   MADICP_ERR_INVALID, nothing written and nothing launched, for a null ctx, poses or out_counts, an
 *                            unknown id, n_poses outside 1 .. 4096, a non-finite entry in ANY pose (the whole call is refused), a
 *                            reach other than 0 and 1, a max_dist that is NaN or negative, a stride < 1.  The map is only read, as
 *                            by the query.  Kernel (fe::map_score_poses): a workgroup stages a chunk of 64 poses in LDS (96 B
 *                            each), a lane loads its point once and scores it at every pose of the chunk, several poses' gathers
 *                            in flight per lane; per pose ballots and popcounts per wavefront, 64-bit integer LDS counters, one
 *                            64-bit integer global atomic per workgroup, pose and count — no float atomics, nothing wraps.  The
 *                            scratch is the call's own, pooled (counts, poses and, on plain and attribute maps, the transient
 *                            slot-to-row array): the builder's is not touched.  Everything runs on the copy stream — one memset,
 *                            the pose upload, the kernels, one copy out — and ends in ONE host synchronisation, whatever n, M and
 *                            n_poses (profiles/map_score_time.md).
 * MERGING SAVED ROWS.  Every column of a map can be downloaded; madicp_map_merge_rows puts a batch of such rows back — a map
 * restored after a restart (a merge into an empty map), a prior map loaded, two maps of one frame and voxel size joined.  The rule
 * (one source with the host twin: csrc/common/map_merge.h — map_merge_refusal, merge_evidence, and voxel_moments.h's freeze):
 *   a batch is n entries (keys[i], xyz[3 i .. 3 i + 2] float32, attr[i], ev[i], mom[10 i .. 10 i + 9]); attr, ev and mom are given
 *   exactly when the map has that column and null otherwise.  A merge is ONE fold: on a moments map it takes the next fold ordinal.
 *   Rows: the keys the map does not hold become one new row each, in ascending order of the LOWEST index that carries the key; xyz
 *   and attr are that entry's, copied bit for bit (NaN payloads, -0.0), the stored key is the entry's; nothing checks that xyz lies
 *   in the key's voxel.  Rows the map holds keep xyz, attr and position.  Evidence: with s the sum of ev over a key's entries, a
 *   new row gets min(s, cap), a row that held e gets min(e + s, cap); the per-slot hit stamps of the folds are not touched.  Moments:
 *   a row takes ALL entries of its key iff its n before the merge is < max_count (a new row: 0), else none; the ten words add; the
 *   add that reaches max_count freezes the row with the merge's ordinal.  Integer sums and a lowest index: a function of (map,
 *   batch) alone, bit-equal between device, host twin and a numpy restatement, whatever the launch geometry.
 *   madicp_map_merge_rows    *out_added rows were appended, the map holds *out_rows.  MADICP_ERR_INVALID, the map untouched, nothing
 *                            written and nothing launched, for a null ctx, out_added or out_rows, an unknown id, n < 0 or > 2^30, a
 *                            voxel that is not == the map's, a column given that the map lacks or (n > 0) lacking that it has, a
 *                            key with bit 63 set, an ev outside 1 .. 2^31 - 1, a mom count < 1, an S1 word > 65535 count or an S2
 *                            word > 65535^2 count, counts that sum past 2^31 - 1.  MADICP_ERR_CAPACITY, the same, when rows + n >
 *                            max_rows (the fold's conservative rule), on a moments map past its last fold ordinal, and while a
 *                            look-ahead build is in flight (the builder's scratch).  n == 0 is legal and does nothing.  The batch
 *                            goes up in one staged copy into a transient pooled block; kernels fe::rows_claim, fe::voxel_mark, the
 *                            tile scan, fe::rows_append and, on evidence and moments maps, fe::rows_combine (a 32-bit
 *                            compare-and-swap loop and ten 64-bit integer atomic adds per entry — no float atomics); everything
 *                            on the copy stream, ONE host synchronisation, for the count (one more where the map grows).
 * REGISTER.  madicp_map_register_cloud gives the pose that FITS a resident cloud to a moments map: `iterations` rounds of
 * point-to-plane Gauss-Newton against the map's surfels, all on the device.  The rule (one source with the host twin:
 * csrc/common/map_align.h), fp64 and integers only, no contraction, no library function in the linearisation:
 *   the surfel columns are those of madicp_map_download_surfels, bit for bit — the call runs fe::map_surfels itself, ONCE per call,
 *   into its own scratch.  Point i at pose (R, t): q and the candidate decision as in the query; its row j is the QUERY's answer at
 *   params->reach; matched iff j >= 0, within iff also d2 <= max_dist max_dist; an INLIER iff within, count[j] >= min_count,
 *   (double)eig[j][1] > 0 and (double)eig[j][0] <= flat (double)eig[j][1].  For an inlier, with c, n the float32 centroid and normal
 *   taken to double: e = n0 (q0 - c0) + (n1 (q1 - c1) + n2 (q2 - c2)); m = n^T R (each entry x0 + (x1 + x2)); J = [m, p x m] — the
 *   reference's Jacobian for the right-multiplied update; s = |e| > rho ? rho / |e| : 1 (rho = +inf: no robust kernel); 28 terms
 *   H(r, c) = (s J[r]) J[c] (r >= c, packed column by column), b[r] = (s J[r]) e, chi2 = (s e) e.  Every other point adds +0.0.
 *   THE SUM is the adjacent-pair binary tree over the term vectors in point order, padded with +0.0 to a power of two — a function
 *   of (map, cloud, pose, parameters) alone, whatever the launch geometry; numpy reproduces it with reshapes.  No float atomics.
 *   Round k linearises at X_k and takes X_{k+1} from the product's one update step (solve_pose: dx = H^-1 (-b), X <- X * dX); an
 *   all-zero H leaves the pose where it is.
 *   out_trace ((iterations + 1) x 40 doubles): row k = X_k (R row-major, t) | H (21, packed) | b (6) | chi2 of the linearisation at
 *   X_k; row `iterations` is the one at the RETURNED pose — its H is the information a consumer wants beside the pose.
 *   out_counts ((iterations + 1) x 4): candidates, matched, within, inliers of the same linearisations.
 *   iterations = 0 is the LINEARISE-ONLY form, the only one in which out_row (int32) / out_e (float64, +0.0 for a point that is no
 *   inlier) may be given: n entries each.
 *   madicp_map_register_cloud  MADICP_ERR_INVALID, nothing written and nothing launched, for a null ctx, R, t, params, out_R, out_t,
 *                            out_trace or out_counts, an unknown id, a map without moments, a non-finite R or t, a reach other
 *                            than 0 and 1, a max_dist that is NaN or negative, a rho that is NaN or <= 0, a min_count below 3, a
 *                            flat outside (0, 1], iterations outside 0 .. 64, a per-point buffer with iterations > 0;
 *                            MADICP_ERR_CAPACITY, the same, when a per-point buffer is given and capacity_points < n.  An empty
 *                            map is legal: every point is unmatched, the sums are zero, the pose comes back as given.  The map
 *                            is only read.  Kernels: fe::map_surfels; per round fe::map_align_terms (one lane per point, a
 *                            workgroup per 256 consecutive points, the terms in registers: a wavefront butterfly and two levels
 *                            in LDS), fe::map_align_join (256 partial rows per workgroup until one is left) and
 *                            fe::map_align_step (one wavefront); one closing linearisation; the copies.  Everything on the copy
 *                            stream, the scratch the call's own, pooled.  ONE host synchronisation, whatever n, M and iterations.
 * Several maps per context are independent.  Bit-equal to madicp_host_map_* (madicp_host.h) for every sequence of folds, prunes,
 * clearings, takes and queries. */
int madicp_map_create(madicp_ctx* ctx, double voxel, int64_t initial_rows, int64_t max_rows, int* out_map_id);
int madicp_map_insert_cloud(madicp_ctx* ctx, int map_id, int cloud_id, const double R[9], const double t[3], int64_t* out_added,
                            int64_t* out_rows);
int madicp_map_size(madicp_ctx* ctx, int map_id, int64_t* out_rows);
int madicp_map_download_f32(madicp_ctx* ctx, int map_id, int64_t first_row, float* out_xyz, int64_t capacity_rows, int64_t* out_n);
int madicp_map_create_attr(madicp_ctx* ctx, double voxel, int64_t initial_rows, int64_t max_rows, int* out_map_id);
int madicp_map_download_attr(madicp_ctx* ctx, int map_id, int64_t first_row, uint32_t* out_attr, int64_t capacity_rows, int64_t* out_n);
int madicp_map_prune(madicp_ctx* ctx, int map_id, const double center[3], double radius, int64_t watermark, int64_t* out_removed,
                     int64_t* out_rows, int64_t* out_watermark);
int madicp_map_clear_rays(madicp_ctx* ctx, int map_id, int cloud_id, const double R[9], const double t[3], const double origin[3],
                          double margin, int64_t watermark, int64_t* out_removed, int64_t* out_rows, int64_t* out_watermark);
int madicp_map_track_removed(madicp_ctx* ctx, int map_id, int on);
int madicp_map_removed_count(madicp_ctx* ctx, int map_id, int64_t* out_n);
int madicp_map_take_removed(madicp_ctx* ctx, int map_id, uint64_t* out_keys, float* out_xyz, uint32_t* out_attr, int64_t capacity,
                            int64_t* out_n);
int madicp_map_download_keys(madicp_ctx* ctx, int map_id, int64_t first_row, uint64_t* out_keys, int64_t capacity_rows, int64_t* out_n);
int madicp_map_download_rows(madicp_ctx* ctx, int map_id, int64_t first_row, float* out_xyz, uint64_t* out_keys, uint32_t* out_attr,
                             int64_t capacity_rows, int64_t* out_n);
int madicp_map_create_ev(madicp_ctx* ctx, double voxel, int64_t initial_rows, int64_t max_rows, int with_attr, uint32_t hit, uint32_t miss,
                         uint32_t cap, int* out_map_id);
int madicp_map_download_evidence(madicp_ctx* ctx, int map_id, int64_t first_row, uint32_t* out_ev, int64_t capacity_rows, int64_t* out_n);
int madicp_map_download_min_evidence(madicp_ctx* ctx, int map_id, uint32_t min_e, float* out_xyz, uint64_t* out_keys, uint32_t* out_attr,
                                     uint32_t* out_ev, int64_t capacity_rows, int64_t* out_n);
int madicp_map_create_mom(madicp_ctx* ctx, double voxel, int64_t initial_rows, int64_t max_rows, int with_attr, const uint32_t evidence[3],
                          uint32_t max_count, int* out_map_id);
int madicp_map_download_moments(madicp_ctx* ctx, int map_id, int64_t first_row, uint64_t* out, int64_t capacity_rows, int64_t* out_n);
int madicp_map_download_surfels(madicp_ctx* ctx, int map_id, int64_t first_row, float* out_centroid, float* out_normal, float* out_eig,
                                uint32_t* out_count, int64_t capacity_rows, int64_t* out_n);
int madicp_map_query_cloud(madicp_ctx* ctx, int map_id, int cloud_id, const double R[9], const double t[3], int reach, double max_dist,
                           int32_t* out_row, double* out_d2, uint64_t* out_keys, uint32_t* out_attr, uint32_t* out_ev,
                           int64_t capacity_points, uint64_t out_counts[3]);
#ifndef MADICP_MAP_ALIGN_PARAMS_DEFINED
#define MADICP_MAP_ALIGN_PARAMS_DEFINED
typedef struct {
  int reach;          /* 0: the point's own voxel, 1: the 27 around it */
  double max_dist;    /* >= 0, +inf legal */
  double rho;         /* > 0, +inf: no robust kernel */
  uint32_t min_count; /* >= 3 */
  double flat;        /* in (0, 1]: eig0 <= flat eig1 */
} madicp_map_align_params;
#endif
int madicp_map_register_cloud(madicp_ctx* ctx, int map_id, int cloud_id, const double R[9], const double t[3],
                              const madicp_map_align_params* params, int iterations, double out_R[9], double out_t[3],
                              double* out_trace /* (iterations + 1) x 40: X[12] | H[21] | b[6] | chi2 */,
                              uint64_t* out_counts /* (iterations + 1) x 4 */, int32_t* out_row, double* out_e,
                              int64_t capacity_points);
int madicp_map_score_poses(madicp_ctx* ctx, int map_id, int cloud_id, const double* poses, int64_t n_poses, int reach, double max_dist,
                           int64_t stride, uint64_t* out_counts /* n_poses x 3 */);
int madicp_map_merge_rows(madicp_ctx* ctx, int map_id, double voxel, const uint64_t* keys, const float* xyz, const uint32_t* attr,
                          const uint32_t* ev, const uint64_t* mom, int64_t n, int64_t* out_added, int64_t* out_rows);
int madicp_map_clear(madicp_ctx* ctx, int map_id);
int madicp_map_release(madicp_ctx* ctx, int map_id);
/* MADtree::build + getLeafs + the upload, all on the device (mad_tree.cpp:47-142,154-163): the tree of the cloud becomes
 * a resident tree exactly like one given to madicp_tree_upload (same node format, madicp_tree_download returns it).
 * Same decisions as the reference node by node, the reference's member order (the permutation utils.h:37-52 leaves), and
 * for the nodes of at most 32 points its summation order: same topology and leaf representatives as the host builder on
 * every scan tried, centroids and covariances of small nodes bit for bit.  Not the same bits everywhere: larger nodes add in
 * a parallel shape and the eigen-solver's trigonometry comes from the device library (mad_icp_amd/csrc/hip/tree_build.hip.h);
 * bit-reproducible run to run.  The cloud is left untouched.  Synchronises the copy stream once (the leaf count sizes the tree).
 * The contract (tests/test_gpu_default_path_parity.py): the kernels' decisions are bit-exact on any
 * tree; host-built trees are the reference's; against device-built trees N of D decisions per registration differ from the
 * reference's, all at nodes within S of their split plane — measured N = 0 of D = 324 832 decisions (16 keyframes) and 0 of
 * 1 516 352 (64 keyframes) at four poses each, so S has no value: no pair of those problems passes within 1e-7 m of a plane
 * and the device-built planes lie within ~1e-12 m of the reference's.  Every internal node is held to its members'
 * centroid within the float64 summation bound and to their principal axis with at most 4 x the reference's own residual
 * (measured 2.34 x); nodes of at most 32 points have the reference's centroid bit for bit.
 * Depth limit: a tree of up to 95 levels below the root is built (one launch step per level, 96 steps); a deeper one — 97 or more
 * collinear points a constant factor apart, one point peeled per split — is refused with MADICP_ERR_INVALID, "tree build: tree
 * deeper than the supported 96 levels", from here and from madicp_tree_build_end: no tree id is issued, nothing is left behind, the
 * context builds on.  (The reference recurses without a limit; a 120 k-point scan at b_max 0.2 is 17 levels deep.)
 * A build is a function of (cloud, b_max, b_min): what the context built before changes how the launches are sized, never a bit
 * of the tree or of its records (tests/test_gpu_tree_build_history.py). */
int madicp_tree_build(madicp_ctx* ctx, int cloud_id, double b_max, double b_min, int* out_tree_id, int32_t* out_n_leaves);
/* The same construction as a look-ahead, for a caller that has the NEXT scan in hand while the current one registers
 * (what Pipeline::prefetch does with the device front-end on).  _begin copies the (n,3) float64 scan to the device and
 * enqueues the whole level loop on a stream of its own — the library's BUILD stream, so that neither the registration on
 * the compute stream nor its feed on the copy stream queues behind it — and returns without waiting; _end waits for the
 * leaf count, sizes and emits the tree and returns its id.  One look-ahead per context: a second _begin, or
 * madicp_tree_build / madicp_cloud_ingest_f32 / madicp_cloud_ingest_records / madicp_cloud_ingest_sources / madicp_cloud_deskew /
 * madicp_cloud_deskew_stamped / madicp_cloud_deskew_own_stamps / madicp_tree_build_stats before the _end, return
 * MADICP_ERR_CAPACITY (they share the builder's scratch).  Registrations, uploads, transforms, searches and releases are
 * free to run in between.  The tree is the one madicp_cloud_upload + madicp_tree_build give for the same scan, bit for bit. */
int madicp_tree_build_begin(madicp_ctx* ctx, const double* xyz, int64_t n, double b_max, double b_min);
int madicp_tree_build_end(madicp_ctx* ctx, int* out_tree_id, int32_t* out_n_leaves);
/* drops a look-ahead whose scan never came (waits for the device work, frees the copy of the scan); no-op without one */
int madicp_tree_build_cancel(madicp_ctx* ctx);
int madicp_tree_info(madicp_ctx* ctx, int tree_id, int32_t* out_n_nodes, int32_t* out_n_leaves);
/* diagnostics of the last madicp_tree_build on this context: out[0] deepest level, out[1] nodes handled one-per-lane, out[2..65] nodes handled one-per-wavefront per level, out[66..129] nodes handled chip-wide per level */
int madicp_tree_build_stats(madicp_ctx* ctx, int32_t out[130]);

/* ---- multi-GPU: keyframe trees sharded across ranks, one all-reduce of (H,b) per GN round ---------- */
/* Peer-mapped mailboxes: keyframe sharding WITHOUT a collective between two rounds (option "shard_p2p" = 1, default 0; additive,
 * one node, at most 8 ranks).  The per-round join of the ranks' adders — the reference's serial sum of mad_icp.cpp:106-109, 30
 * doubles per scan — is then done inside the next round kernel's prologue: workgroup 0 writes this rank's sums as tagged
 * granules into every peer's mailbox, every workgroup polls the peers' rows in the own mailbox and adds them in rank order
 * (all ranks the same bits).  The matched flags of the last round (a leaf is an inlier if ANY keyframe on ANY rank matched it:
 * mad_icp.cpp:85, pipeline.cpp:197-204) travel the same way, 32 flags per tagged word, OR-ed by the closing kernel — for moving
 * sets of up to 131 072 leaves; larger ones OR them through the communicator as before.  A sharded registration is then the
 * single-GPU launch sequence with NO collective and no host step: it is captured in a hipGraph and streams its results out like
 * a single-GPU one.
 *   madicp_p2p_export: allocates this rank's mailbox (the first time), ZEROES it and returns its 64-byte hipIpcMemHandle_t.
 *                      Fine-grained device memory; where the runtime cannot export that, the call fails unless option
 *                      "p2p_allow_coarse" = 1 (coarse-grained memory promises no visibility of a peer's stores to a running
 *                      kernel: acceptable only for ranks that share ONE device).  get_option "p2p_fine_grained" says which.
 *   madicp_p2p_attach: `handles` = n_ranks x 64 bytes in rank order (gathered by the caller — torch.distributed, MPI ...);
 *                      needs madicp_comm_init / madicp_comm_init_host first, with the same n_ranks / rank, and an export SINCE
 *                      the last attach: a session is export -> gather (a point every rank passes) -> attach, so that every
 *                      mailbox is clean before any rank can begin a registration of the session, whose counter restarts at 0.
 *   madicp_p2p_detach: unmaps the peers' mailboxes (madicp_comm_destroy does it too).
 * A peer whose row does not arrive within "comm_timeout_ms" fails the registration with MADICP_ERR_COMM — once per
 * registration, not once per round — and the session is over (the ranks' counters may disagree from there on): later sharded
 * registrations fail with MADICP_ERR_COMM until every rank has exported and attached again.  Every rank must submit the same
 * sequence of sharded registrations (as with any collective). */
int madicp_p2p_export(madicp_ctx* ctx, uint8_t out_handle[64]);
int madicp_p2p_attach(madicp_ctx* ctx, const uint8_t* handles, int n_ranks, int rank);
int madicp_p2p_detach(madicp_ctx* ctx);

/* Replaces the serial sum of per-thread adders at mad_icp.cpp:106-109.  unique_id: the 128-byte
 * ncclUniqueId produced by madicp_comm_unique_id on rank 0 and distributed by the caller (e.g. a
 * torch.distributed broadcast).  After this call every registration on the context all-reduces
 * [H(21) b(6) n] over the communicator after each round and ORs the matched flags after the last.  With a
 * communicator a registration may be given K = 0 trees (a rank that owns no keyframe still joins every collective,
 * contributing zeros).  get_option "comm_ranks" (read-only) says how many ranks the installed communicator — this one or
 * madicp_comm_init_host's — has, 0 without one; "comm_rank" this context's rank in it, -1 without one. */
int madicp_comm_unique_id(uint8_t out_id[128]);
int madicp_comm_init(madicp_ctx* ctx, const uint8_t unique_id[128], int n_ranks, int rank);
int madicp_comm_destroy(madicp_ctx* ctx);

/* The same sharded registration over a HOST-STAGED transport supplied by the caller (MPI, gloo, a socket ...) instead of
 * RCCL: after every round's icp_reduce the library copies this rank's [H(21) b(6) n v w] per scan to pinned host memory,
 * waits for that copy (only this rank's own kernels are in front of it: no peer can stall it), calls `fn` — which must
 * leave the element-wise reduction over all ranks in `buf` on every rank, and whose own time-out is the only bound on a
 * peer that never joins ("comm_timeout_ms" covers RCCL's collectives, not the caller's transport) — and copies the totals
 * back in front of the next round; the matched flags go through the same
 * call once with MADICP_REDUCE_MAX_U8.  Kernel sequence, summation order inside a rank and the K = 0 rank are exactly
 * those of the RCCL path: it is the way to run (and test) the multi-rank product path where RCCL cannot form a
 * communicator — e.g. two ranks sharing one GPU — and a fallback where there is no xGMI/RDMA path between the ranks.
 * One host round trip per round, so not capturable in a hipGraph and slower than RCCL (tens of microseconds per round).
 * `fn` returns 0 on success; anything else fails the registration with MADICP_ERR_COMM.  madicp_comm_destroy ends it. */
#define MADICP_REDUCE_SUM_F64 0
#define MADICP_REDUCE_MAX_U8 1
typedef int (*madicp_host_allreduce_fn)(void* user, void* buf, int64_t count, int kind);
int madicp_comm_init_host(madicp_ctx* ctx, int n_ranks, int rank, madicp_host_allreduce_fn fn, void* user);

#ifdef __cplusplus
}
#endif
#endif /* MADICP_HIP_H */
