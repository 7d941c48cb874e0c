// Pipeline — the odometry frame step.  Same constructor, same public methods and the same by-value
// compute(stamp, cloud) as the reference class (mad_icp/src/odometry/pipeline.h:45-103), so
// apps/cpp_runners/bin_runner.cpp:106-186 and the pybind module keep working unchanged.
//
// What moved: the data association + Gauss-Newton loop (pipeline.cpp:166-193) runs on the MI355X through
// libmadicp_hip.so.  Every scan's MAD-tree is uploaded once, when it is built (asynchronously, on the library's copy
// stream), and stays in HBM while the frame is in the 10-frame window or a keyframe: the scan's moving leaves are taken
// from the resident tree, applyTransform runs on the device (pipeline.cpp:224), promotion to keyframe
// (pipeline.cpp:234-253) is a pointer move, and leaving the window / eviction (pipeline.cpp:229-232,254-257) returns
// the buffers to the library's pool without a synchronisation.  What stayed on the CPU: tree construction of the
// incoming scan, deskew, the constant-velocity predictor, keyframe selection.
//
// Additive: prefetch(next_cloud) starts building the NEXT scan's tree on another thread — the build does not depend
// on the current pose (pipeline.cpp:140-141 builds in the sensor frame).  compute() itself is synchronous, so what the
// build overlaps is whatever runs until the compute() of that scan.  Up to three look-aheads are kept beside the scan being
// consumed, each matched to its scan by size and end points, so a caller that reads ahead (bin_runner / the launcher on a
// dataset) issues prefetch(i + d) before compute(i).  Averaged over a drive at 120 k points the frame takes 2.5 ms without,
// 1.67 ms with d = 1, 1.41 ms with d = 2, 1.29 ms with d = 3 (tools/lookahead_probe.py), with the reference's own trees bit
// for bit.  Individual frames are bimodal — one that waits about a build's length, then d quick ones of 0.7 ms: a build's
// critical path (2.1-2.6 ms inside the pipeline) does not get shorter with more threads, so depth d buys d builds per build
// latency until the 16 threads are busy.  With the
// device front-end on, prefetch(i + 1) before compute(i) hands over the NEXT scan; compute(i) starts its construction on the
// library's build stream (madicp_tree_build_begin) as soon as its own registration is submitted: the host side of that build
// (staging, launches, the wait for the leaf count) is hidden behind the registration and the frame becomes device-bound
// (0.90 -> 0.64 ms; the kernels of the two streams interleave, profiles/r3_o_lookahead_overlap.md); one look-ahead there.  For
// deskewed datasets the tree needs the previous poses: prefetch() then computes the pose-independent half of deskew ahead —
// the azimuth of every point and their order (deskew.h).
//
// Additive: computeStamped(stamp, cloud, stamps) — a scan with the acquisition time of every point (what a PointCloud2 carries)
// is motion-compensated from those times instead of the reference's azimuth guess, on the device or on the host (deskew.h).
#pragma once
#include <array>
#include <cstddef>
#include <deque>
#include <future>
#include <memory>
#include <vector>

#include "deskew.h"
#include "ingest_records.h"
#include "map_store.h"
#include "keyframe_ledger.h"
#include "linalg.h"
#include "mad_icp.h"
#include "mad_tree.h"
#include "types.h"
#include "vel_estimator.h"

namespace madicp_host {

// tools/constants.h:31-35
static constexpr int CHUNKS = 1024;
static constexpr int SMOOTHING_T = 10;
static constexpr int MAX_ICP_ITS = 15;
static constexpr int FRAME_WINDOW = 10;

struct Frame {  // tools/frame.h:37-52; the tree is owned here
  Pose frame_to_map_ = Pose::identity();
  std::unique_ptr<MADtree> tree_;  // (a keyframe of a sharded Pipeline: on the rank that owns it only)
  ContainerType host_leaves_;      // sharded, keyframe owned by another rank: its leaf means, map frame (modelLeaves())
  double stamp_ = 0.;
  double weight_ = 0.;
  int frame_ = 0;
};

class Pipeline {
 public:
  Pipeline(double sensor_hz, bool deskew, double b_max, double rho_ker, double p_th, double b_min, double b_ratio,
           int num_keyframes, int num_threads, bool realtime);
  ~Pipeline();

  const Matrix4d currentPose() const { return toMatrix(frame_to_map_); }
  const std::vector<Matrix4d> trajectory() const;
  const Matrix4d keyframePose() const { return toMatrix(keyframe_to_map_); }
  bool isInitialized() const { return is_initialized_; }
  size_t currentID() const { return seq_; }
  size_t keyframeID() const { return seq_keyframe_; }
  bool isMapUpdated() { return is_map_updated_; }
  const ContainerType currentLeaves();
  const ContainerType modelLeaves();
  void compute(const double& curr_stamp, ContainerType curr_cloud_mem);

  // additive (not in the reference): start building the tree of the scan that the NEXT compute() will be given
  void prefetch(ContainerType next_cloud);
  // additive: the same two calls on a VIEW of the caller's points (n x 3 doubles, only read during the call) — what the
  // Python bindings use, so that a frame does not begin with a 3 MB allocation + copy of its by-value argument
  void computeView(const double& curr_stamp, const Vector3d* curr_cloud, size_t n);
  void prefetchView(const Vector3d* next_cloud, size_t n);

  // additive (not in the reference): a scan WITH the acquisition time of every point — stamps[i] in [0, 1], 0 = scan start,
  // 1 = scan end, what a PointCloud2 reader extracts from the `t` / `timestamp` / `time` field.  Where the reference deskews
  // (deskew = true and two poses exist: pipeline.cpp:138-139) the scan is motion-compensated from the stamps instead of the
  // azimuth guess of pipeline.cpp:79-123 — same time model, same pose table, the chunk read off the stamp (deskew.h) — on the
  // device (madicp_cloud_deskew_stamped) or, host front-end, by deskew_cloud_stamped; the points keep their input order.
  // With deskew = false, and on the first two frames, the stamps are not used: the call IS compute() / computeView(), look-ahead
  // hits included.  An azimuth order prefetch() computed ahead for this scan is dropped unused; there is no look-ahead for
  // stamped frames.  std::invalid_argument for a null pointer, an empty cloud or stamps.size() != cloud.size().
  void computeStamped(const double& curr_stamp, ContainerType curr_cloud, const std::vector<double>& stamps);
  void computeStampedView(const double& curr_stamp, const Vector3d* curr_cloud, const double* stamps, size_t n);

  // additive: the device front-end.  When on, compute() uploads the scan once and deskew
  // (pipeline.cpp:79-123) and MADtree::build (mad_tree.cpp:47-130) run on the MI355X; the tree never exists on the host
  // unless currentLeaves() / modelLeaves() ask for it.  Default: ON (round 5: for deskew = false; round 6: for deskewed
  // datasets too); the MAD_ICP_GPU_BUILD environment variable ("0" = the host builder, whose trees are the reference's bit
  // for bit) and this call override it.  Device-built trees have the host builder's topology, member order and leaf
  // representatives and differ from host-built ones in the last bits of their larger nodes (mad_icp_amd/csrc/hip/
  // tree_build.hip.h): without deskew poses stay within ~1e-12 m of the oracle pipeline's over full-size drives; with deskew
  // ONE frame from the oracle's state is the oracle's frame to 1e-5 (tests/test_gpu_deskew_one_step.py), and a drive stays
  // inside the envelope the reference shows against itself (the compensated cloud depends on the previous poses' last bits
  // and tree construction is chaotic in its input: tests/test_gpu_frontend_oracle.py).
  void setDeviceFrontEnd(bool on) {
    if (!on) dropDeviceLookAhead();
    device_frontend_ = on;
  }
  bool deviceFrontEnd() const { return device_frontend_; }

  // additive: the REGISTERED SCAN out.  With setKeepScan(true) — default off: nothing changes, not a launch — the cloud the frame's
  // tree was built from is retained until the next compute*(), setKeepScan(false) or destruction: the cloud after deskew where
  // deskew is due, the cloud as given (or as ingested: range-filtered, merged over the rig) on the first frames and with
  // deskew = false; azimuth deskew leaves it in azimuth order.  Every compute* entry point retains.  Device front-end: the frame's
  // resident cloud is kept instead of going back to the pool after the build (one pool buffer more in use, no copy); host
  // front-end: a host copy is taken before the builder permutes the points.  While the option is on the device look-ahead is not
  // begun — prefetch() stays legal and the frame builds synchronously, the restriction stamped and records frames already carry
  // (a look-ahead build owns its own copy of the scan and gives back only the tree).  Poses, keyframe ids and isMapUpdated()
  // are the same bit for bit with the option on or off.  A sharded Pipeline keeps and exports its own copy on every rank.
  void setKeepScan(bool on);
  bool keepScan() const { return keep_scan_; }
  size_t registeredScanSize() const { return have_kept_ ? kept_n_ : 0; }  // points of the retained scan (0: none)
  // The retained scan as float32 rows (x, y, z) into out[0, 3 * capacity): map_frame = true takes it through the pose of the frame
  // just computed (currentPose()), false through the identity — the sensor frame at the pose's reference time.  voxel == 0: every
  // point in the cloud's order; voxel > 0: the lowest-index point of every voxel of that edge, in ascending index order (the
  // rule of madicp_cloud_export_f32, include/madicp_hip.h — device front-end: that call, host front-end: its twin
  // madicp_host_cloud_export_f32; the same bits for the same cloud and pose).  Returns the rows written; registeredScanSize()
  // rows always suffice.  std::logic_error when the option is off or no frame has been computed since it was turned on;
  // std::invalid_argument for a null buffer, a voxel that is negative or not finite, a capacity smaller than the rows needed
  // (nothing is written then).
  size_t registeredScan(float* out, size_t capacity, double voxel, bool map_frame);
  // additive: the per-point ATTRIBUTE (include/madicp_hip.h: one 32-bit word per point, the bytes of one record field zero-extended,
  // never converted).  A frame whose sources name an attribute field (RecordSource::A — computeSourcesStamped, or
  // computeRecordsStamped's overload with a field) carries the column beside its points through the ingest and both deskews (the
  // azimuth deskew permutes it with the points), on either front-end; the retained scan keeps it.  registeredScanAttribute returns
  // the words of exactly the rows registeredScan(…, voxel, map_frame) returns (which points own a voxel depends on the frame the
  // voxels are cut in; at voxel 0 it does not matter); registeredScanWithAttribute returns rows and words from ONE export.  Same
  // refusals as registeredScan; std::logic_error as well when the retained scan carries no attribute.
  size_t registeredScanAttribute(uint32_t* out, size_t capacity, double voxel, bool map_frame = true);
  size_t registeredScanWithAttribute(float* out_xyz, uint32_t* out_attr, size_t capacity, double voxel, bool map_frame);
  int registeredScanAttributeType() const { return have_kept_ && kept_has_attr_ ? kept_attr_type_ : kAttrNone; }  // kAttr*: the field's type

  // additive: MAP ACCUMULATION.  With setMapAccumulation(voxel_size > 0) — default off: nothing changes, not a launch — every
  // compute* entry point ends by folding the cloud its tree was built from (the cloud registeredScan(0, ...) returns, in that row
  // order) through the frame's pose (currentPose()) into an append-only voxel map: one float32 row per voxel of edge voxel_size,
  // the first point ever to fall into it; later arrivals are dropped where the map lives (the rule of madicp_map_insert_cloud,
  // include/madicp_hip.h).  keyframes_only: only frames that end with isMapUpdated() true are folded.  max_points bounds the
  // map (default kMapMaxPointsDefault = 2^24 rows: 0.7 GB of device memory at 44 bytes per row of capacity, allocated
  // geometrically from 2^18 rows up); a fold is refused when the map's rows plus the frame's points would exceed it: compute*
  // still returns its pose, accumulation stops and mapOverflowed() answers true until clearMap().  voxel_size == 0 turns the
  // option off and frees the map; another voxel size, keyframes_only or max_points starts a new, empty map.  Device front-end:
  // the frame's resident cloud is folded on the device, no copy (madicp_map_*); host front-end: the bit-equal host twin
  // (voxel_map.h).  Independent of setKeepScan; like it, turning the option on drops the device look-ahead and none is begun
  // while it is on — prefetch() stays legal and the frame builds synchronously: a tree built ahead comes without its scan.
  // Poses, keyframe ids and isMapUpdated() are the same bit for bit with the option on or off.  A sharded Pipeline holds the
  // whole map on every rank (poses are bit-equal across ranks, so the maps are).  std::invalid_argument for a voxel_size that
  // is negative or not finite, max_points outside 1 .. 2^30.
  static constexpr size_t kMapMaxPointsDefault = size_t(1) << 24;
  // with_attribute: the map is made with the attribute column (madicp_map_create_attr / VoxelMap's) — a row keeps its owning
  // point's word; frames that arrive without an attribute (compute, computeRecords ...) contribute the word 0.  mapAttribute
  // runs beside mapCloud: the words of rows [first_row, mapSize()), the same refusals; std::logic_error without the column.
  // evidence: null — the default: nothing changes, not a launch, not an allocation, the same pose and map bits — or {hit, miss,
  // cap}: the map is made with the EVIDENCE column (madicp_map_create_ev / VoxelMap's; include/madicp_hip.h has the rule): every
  // fold reinforces the voxels it hits, once per fold, up to cap; a clearing (setMapClearing, mapClearRays) takes miss from the
  // voxels it sees through, and a row leaves only when its evidence is used up.  The frame order stays fold, clearing, range
  // prune: a fold's own hits are occupied in its clearing, so one scan never both reinforces and weakens a voxel.  Another
  // triple starts a new, empty map; std::invalid_argument for hit < 1, miss < 1, cap < hit, cap > 2^31 - 1.
  // mapEvidence: the words of rows [first_row, mapSize()), mapCloud's refusals; mapConfirmed: the rows with word >= min_evidence
  // in row order — xyz, and keys / attr / ev where not null — compacted where the map lives (madicp_map_download_min_evidence),
  // returns their number (at most mapSize(): a buffer that holds that many always suffices); std::invalid_argument for a null xyz
  // or a capacity below that number (nothing written).  Both: std::logic_error while accumulation is off or without the column.
  void setMapAccumulation(double voxel_size, bool keyframes_only = false, size_t max_points = kMapMaxPointsDefault,
                          bool with_attribute = false, const uint32_t* evidence = nullptr, uint32_t moments_max_count = 0);
  // moments_max_count: 0 — the default: nothing changes, not a launch, not an allocation, the same pose and map bits — or 1 .. 2^31:
  // the map is made with per-voxel MOMENTS (madicp_map_create_mom / VoxelMap's; csrc/common/voxel_moments.h has the rule): every
  // fold adds its points to the count, sums and sums of products of the voxels they fall into, a row taking whole folds while its
  // count is below moments_max_count; the words follow their rows through clearings and prunes.  It combines freely with
  // with_attribute and evidence; another value starts a new, empty map; std::invalid_argument above 2^31.
  // mapMoments: the ten 64-bit words (n, S1[3], S2[6]) of rows [first_row, mapSize()) as (rows, 10), mapCloud's refusals.
  // mapSurfels: per row of the window the centroid (3 floats) and, where not null, the normal (3 floats, zero below three points,
  // sign free), the covariance's eigenvalues in m^2 ascending (3 floats) and the count — computed where the map lives
  // (madicp_map_download_surfels); the same refusals.  Both: std::logic_error while accumulation is off or without the moments.
  // The removal log and MapMirror carry no moments — a row's change after it was delivered: a consumer re-reads mapSurfels.
  bool mapWithMoments() const { return map_spec_.mom > 0; }
  size_t mapMoments(uint64_t* out, size_t capacity, size_t first_row = 0);
  size_t mapSurfels(float* centroid, float* normal, float* eig, uint32_t* count, size_t capacity, size_t first_row = 0);
  bool mapWithEvidence() const { return map_spec_.with_ev; }
  size_t mapEvidence(uint32_t* out, size_t capacity, size_t first_row = 0);
  size_t mapConfirmed(uint32_t min_evidence, float* out_xyz, uint64_t* out_keys, uint32_t* out_attr, uint32_t* out_ev, size_t capacity);
  bool mapWithAttribute() const { return map_spec_.with_attr; }
  int mapAttributeType() const { return map_attr_type_; }  // the field type of the last attribute frame folded (kAttrNone: none yet)
  size_t mapAttribute(uint32_t* out, size_t capacity, size_t first_row = 0);
  double mapVoxelSize() const { return map_spec_.voxel; }  // 0: off
  bool mapOverflowed() const { return map_overflowed_; }
  size_t mapSize();  // rows the map holds; std::logic_error while the option is off (mapCloud and clearMap too)
  // rows [first_row, mapSize()) as float32 (x, y, z) into out[0, 3 * capacity): rows are never changed or removed by a fold, so
  // a consumer fetches what was added since it last looked with first_row = the size it saw then (across prunes — setMapRange,
  // mapPrune — rows move down: mapNewRows below keeps the place instead).  Returns the rows written;
  // std::invalid_argument for a null buffer, first_row > mapSize(), a capacity below mapSize() - first_row (nothing written).
  size_t mapCloud(float* out, size_t capacity, size_t first_row = 0);
  void clearMap();  // forgets the rows (and the overflow), keeps the memory; mapRemoved() and mapNewRows' cursor start again at 0
  // additive: A MAP THAT FOLLOWS THE VEHICLE.  setMapRange(radius > 0) — default 0, off: not a launch, not an allocation — lets
  // foldFrame() PRUNE the map (madicp_map_prune / VoxelMap::prune: rows whose stored float position is farther than radius from
  // a centre leave, with their voxels, and the kept rows close up in order) at the translation of the frame's pose:
  //   (a) after a successful fold, when that position is at least radius / 4 from the centre of the last prune (squared
  //       distances, fp64); the position of the first frame folded while a range is set counts as a prune centre, so a parked
  //       vehicle never prunes;
  //   (b) before a fold that the capacity rule would refuse (rows + n > max_points), once, at the position of the frame before
  //       it; only if the fold is still refused does mapOverflowed() become true.
  // The policy is a function of the poses alone: both front-ends and every rank of a sharded Pipeline prune identically.  It has
  // an effect only while setMapAccumulation is on.  std::invalid_argument for a radius that is negative or not finite or whose
  // square is not finite.  mapPrune: the same operation by hand, returns the rows removed (0 before the first fold);
  // std::logic_error while accumulation is off, std::invalid_argument for what madicp_map_prune refuses.  mapRemoved(): rows
  // removed since the map was made or cleared.
  // mapCloud(first_row) and mapAttribute index the map AS IT IS NOW: a prune moves rows down, so a consumer that streams the map
  // incrementally across prunes uses mapNewRows instead — the rows (and with out_attr, on a map with the column, their words)
  // added since its previous call, mapNewRowCount() of them.  The Pipeline keeps that consumer's cursor and hands it through every
  // prune as the watermark: every row is delivered at most once, whatever was pruned in between.  A row that is added AND pruned
  // between two calls is never delivered — that happens only with a radius below the sensor's range.  Returns the rows written;
  // std::invalid_argument for a null buffer or a capacity below mapNewRowCount() (nothing written, the cursor stays).
  void setMapRange(double radius);
  double mapRange() const { return map_range_; }  // 0: off
  size_t mapPrune(const double center[3], double radius);
  size_t mapRemoved() const { return map_removed_; }
  size_t mapNewRowCount();
  size_t mapNewRows(float* out, size_t capacity, uint32_t* out_attr = nullptr, uint64_t* out_keys = nullptr);
  // additive: A MAP THAT A CONSUMER CAN MIRROR.  Every row has an identity that survives prunes: its stored 64-bit voxel key, unique
  // among the rows the map holds (mapKeys: the keys of rows [first_row, mapSize()), mapCloud's refusals; mapNewRows' out_keys: the
  // keys of the new rows; with keys or words the columns come through madicp_map_download_rows, their copies before one wait).
  // setMapTrackRemoved(true) — default off: not a launch, not an allocation, the same pose and map bits — makes the map keep a
  // REMOVAL LOG (include/madicp_hip.h has the rule): foldFrame, mapPrune and mapClearRays pass mapNewRows' cursor as watermark, so
  // the log holds exactly the rows that were delivered and have left since — key, float row and, on a map with the column, word.
  // mapRemovedRows takes it (mapRemovedRowCount() entries, oldest first; attr may be null), and a consumer that at every poll
  // first deletes the removed keys and then inserts mapNewRows' rows by key holds exactly the map (mad_icp_amd/map_mirror.py).  It
  // takes effect on the current map and on any made later, and survives a front-end switch as the map does; clearMap() empties
  // the log.  The log is bounded by max_points: once it holds that many entries, foldFrame, mapPrune and mapClearRays SKIP their
  // removal — map and mirror stay consistent, mapRemovedLogFull() answers true until the next mapRemovedRows() — and a skipped range
  // prune before a fold the capacity rule refuses ends in mapOverflowed(), as without a range: asking for removals and never
  // fetching them ends there.  std::logic_error while accumulation is off; mapRemovedRows: also while tracking is off, or with
  // attr on a map without the column; std::invalid_argument for a null buffer or a capacity below mapRemovedRowCount() (nothing
  // written, the log is kept).
  void setMapTrackRemoved(bool on);
  bool mapTrackRemoved() const { return map_track_removed_; }
  size_t mapRemovedRowCount();
  size_t mapRemovedRows(uint64_t* keys, float* rows, uint32_t* attr, size_t capacity);
  bool mapRemovedLogFull() const { return map_log_full_; }
  size_t mapKeys(uint64_t* out, size_t capacity, size_t first_row = 0);
  // additive: FREE-SPACE CLEARING.  setMapClearing(true) — default off: not a launch, not an allocation, the same pose bits — lets
  // foldFrame() call madicp_map_clear_rays / VoxelMap::clearRays after every successful fold and before the range prune (a), with
  // the cloud it has just folded, the frame's pose and `origin`, the sensor's position in the cloud's frame: the rows whose voxel a
  // ray of the scan is sampled in (one voxel edge apart, stopping `margin` metres short of the point) and no point of the scan lies
  // in leave, with their voxels — what moved through the scene does not stay in the map.  mapNewRows' cursor is the watermark, as
  // for a prune; mapRemoved() counts both kinds of removal.  It has an effect only while setMapAccumulation is on.  The rule
  // samples, it does not traverse: shallow rays over ground that the scan samples sparsely remove ground voxels between the rings —
  // margin and the voxel size are the consumer's knobs.  std::invalid_argument for a margin that is negative or not finite, a
  // non-finite origin (null: the cloud's origin).  mapClearRays: the same operation by hand over n points xyz (n, 3) at pose
  // (R, t), returns the rows removed (0 before the first fold); std::logic_error while accumulation is off, std::invalid_argument
  // for what madicp_map_clear_rays refuses.
  void setMapClearing(bool on, double margin = 0.0, const double origin[3] = nullptr);
  bool mapClearing() const { return map_clearing_; }
  size_t mapClearRays(const double* xyz, size_t n, const double R[9], const double t[3], const double origin[3], double margin = 0.0);
  // additive: ASKING THE MAP.  mapQuery: for each of the n points xyz (n, 3) taken through (R, t), the nearest row of its voxel
  // neighbourhood (reach 0: its own voxel, 1: the 27 around it; include/madicp_hip.h: madicp_map_query_cloud has the rule) — row
  // (int32, -1: none), d2 (+inf: none), the row's stored key (all ones: none) and its attribute and evidence words (0: none), each
  // buffer of n entries or null, and counts = {candidates, matched, within max_dist}, always.  With all five buffers null it is the
  // scoring form (mapOverlap in the bindings): nothing per point is copied.  Device front-end: the points are uploaded as
  // mapClearRays uploads them and asked where the map lives (one host synchronisation); host front-end: the bit-equal host twin.
  // Before the first fold the map is empty: every candidate is unmatched.  The map is only read.  std::logic_error while
  // accumulation is off and for attr / ev on a map without that column; std::invalid_argument for a null argument, a non-finite R
  // or t, a reach other than 0 and 1, a max_dist that is NaN or negative.
  // setMapOverlap(on, reach, max_dist) — default off: not a launch, not an allocation, the same pose and map bits — lets foldFrame()
  // ask the map about the frame's cloud at the frame's pose BEFORE it folds it (behind a capacity prune of setMapRange, if one runs);
  // mapFrameOverlap() answers that frame's three counts: how much of the scan the map already knew.  Zeros when the fold was
  // skipped by keyframes_only, when it was refused (mapOverflowed()) and before the first frame.  With the option on, poses,
  // keyframe decisions and every map column are bit for bit what they are with it off.  The counts come back through the query's
  // own wait: one host synchronisation more per folded frame on the device front-end (profiles/map_query_time.md).  A sharded
  // Pipeline holds the whole map on every rank: the answers are the same on every rank, nothing is exchanged.
  void mapQuery(const double* xyz, size_t n, const double R[9], const double t[3], int reach, double max_dist, int32_t* row, double* d2,
                uint64_t* keys, uint32_t* attr, uint32_t* ev, uint64_t counts[3]);
  // additive: REGISTERING A SCAN AGAINST THE MAP.  mapRegister: `iterations` (0 .. 64) rounds of point-to-plane Gauss-Newton of the n
  // points xyz (n, 3) against the surfels of the moments map, from the pose (R, t) (include/madicp_hip.h: madicp_map_register_cloud
  // and csrc/common/map_align.h have the rule) — out_R / out_t: the pose after the last round; trace ((iterations + 1) x 40: X | H
  // packed | b | chi2) and counts ((iterations + 1) x 4: candidates, matched, within, inliers): row k the linearisation at X_k, the
  // last one at the returned pose.  iterations == 0 is the linearise-only form, the only one that takes row (int32) / e (float64),
  // n entries each or null.  Device front-end: the points are uploaded as mapQuery uploads them and every round runs where the map
  // lives (one host synchronisation); host front-end: the host twin.  Before the first fold the map is empty: zero sums, the pose
  // as given.  The map is only read and the pipeline's own pose is never touched.  std::logic_error while accumulation is off or
  // without moments; std::invalid_argument for a null argument and for what madicp_map_register_cloud refuses.
  void mapRegister(const double* xyz, size_t n, const double R[9], const double t[3], const AlignParams& params, int iterations,
                   double out_R[9], double out_t[3], double* trace, uint64_t* counts, int32_t* row = nullptr, double* e = nullptr);
  // additive: MANY HYPOTHESES.  mapScorePoses: mapQuery's three counts (candidates, matched, within max_dist) of the n points xyz at
  // each of n_poses poses — (n_poses, 12) doubles, R row-major then t — over the points i with i % stride == 0, counts (n_poses x 3):
  // row k is what the scoring form of mapQuery answers for the subsampled cloud at pose k (include/madicp_hip.h:
  // madicp_map_score_poses has the rule).  Device front-end: ONE upload of the points, one launch sequence, ONE host
  // synchronisation whatever n, the map's size and n_poses; host front-end: the bit-equal host twin.  Before the first fold the map
  // is empty: every candidate is unmatched.  The map is only read.  std::logic_error while accumulation is off;
  // std::invalid_argument for a null argument, n_poses outside 1 .. 4096, a non-finite entry in any pose, a reach other than 0 and
  // 1, a max_dist that is NaN or negative, a stride < 1.
  // mapRelocalize: under ONE borrow of the scan (one upload on the device front-end) it (1) scores all n_poses poses as
  // mapScorePoses does, (2) ranks them by (within descending, index ascending) and (3) registers the first min(refine, n_poses) of
  // them as mapRegister does — every point, no stride, `iterations` rounds from the hypothesis' own pose.  It IS that composition
  // and equals it bit for bit.  Per refined hypothesis r, in rank order: out_index[r], out_scores (3: its score counts), out_poses
  // (12: the registered pose), out_sums (28) and out_counts (4: candidates, matched, within, inliers) of the closing linearisation;
  // *out_best is the r with the most closing inliers, a tie to the better rank.  Returns min(refine, n_poses).  The pipeline's own
  // pose is never touched and the map is only read.  Host synchronisations on the device front-end: 1 + refine (the scoring call's
  // one, then one per registration), behind the upload.  std::logic_error while accumulation is off or without moments;
  // std::invalid_argument for refine outside 1 .. 64 and for what mapScorePoses and mapRegister refuse.
  static constexpr int kRelocalizeMaxRefine = 64;
  void mapScorePoses(const double* xyz, size_t n, const double* poses, size_t n_poses, int reach, double max_dist, int64_t stride,
                     uint64_t* counts);
  size_t mapRelocalize(const double* xyz, size_t n, const double* poses, size_t n_poses, int reach, double max_dist, int64_t stride, int refine,
                       const AlignParams& params, int iterations, int32_t* out_index, uint64_t* out_scores, double* out_poses,
                       double* out_sums, uint64_t* out_counts, size_t* out_best);
  // additive: SAVED ROWS BACK IN.  mapMergeRows merges a batch of n saved rows into the map as ONE fold (include/madicp_hip.h:
  // madicp_map_merge_rows and csrc/common/map_merge.h have the rule): keys (n), rows (n, 3) float32 and attribute (n) / evidence (n) /
  // moments (n, 10) exactly where the map has that column, null otherwise — what mapKeys, mapCloud, mapAttribute, mapEvidence and
  // mapMoments hand out, of this pipeline or of another with the same voxel size and columns.  A map restored after a restart is a
  // merge before the first frame: where no map exists yet the call makes one — on the device iff deviceFrontEnd(), else the host
  // twin — under foldFrame's lock and look-ahead cancellation, and the first fold then finds that map.  The merged rows are NEW rows
  // to mapNewRows() (the cursor does not move), so a mirror fed across a merge still equals the map.  *out_added: the rows
  // appended; returns the rows the map holds.  Nothing runs unless called: poses and map bits without a call are unchanged.
  // std::logic_error while accumulation is off; std::invalid_argument for what madicp_map_merge_rows refuses as invalid;
  // std::runtime_error for a capacity refusal (rows + n > max_points, the last fold ordinal) — the map, the cursor and the overflow
  // flag are as they were, and a map the call would have made is not kept.
  size_t mapMergeRows(const uint64_t* keys, const float* rows, const uint32_t* attribute, const uint32_t* evidence, const uint64_t* moments,
                      size_t n, size_t* out_added);
  const uint32_t* mapEvidenceParams() const { return map_spec_.ev; }  // hit, miss, cap ({1, 1, 1} without evidence)
  uint32_t mapMomentsMaxCount() const { return map_spec_.mom; }        // 0: no moments
  // setMapAlignment(on, iterations, params) — default off: not a launch, not an allocation, the same pose and map bits — lets
  // foldFrame(), inside its one borrow of the frame's cloud and BEFORE the fold, register that cloud against the map as it stands,
  // from the frame's own pose (a drift check of the odometry against its own map).  The result is only REPORTED: mapFrameAlignment()
  // holds the pose after `iterations` rounds, the sums and counts of the closing linearisation, and chi2 and counts of the first;
  // valid is false for a frame that was not folded, while the option is off and on a map without moments.  The pipeline's pose is
  // never changed by it: with the option on, poses, keyframe decisions and every map column are bit for bit what they are with it
  // off.  One host synchronisation more per folded frame on the device front-end.  std::invalid_argument for what
  // madicp_map_register_cloud refuses of the parameters, std::logic_error when the accumulation is on without moments.
  struct FrameAlignment {
    bool valid = false;
    int iterations = 0;
    double R[9] = {}, t[3] = {};       // the pose after the rounds
    double sums[kAlignTerms] = {};     // H (21, packed) | b (6) | chi2 of the linearisation at that pose
    uint64_t counts[kAlignCounts] = {};
    double first_chi2 = 0.0;           // ... and of the one at the frame's own pose
    uint64_t first_counts[kAlignCounts] = {};
  };
  void setMapAlignment(bool on, int iterations = 5, const AlignParams& params = AlignParams());
  bool mapAlignmentOn() const { return map_alignment_; }
  const FrameAlignment& mapFrameAlignment() const { return map_frame_alignment_; }
  void setMapOverlap(bool on, int reach = 1, double max_dist = kQueryNoDistance);
  bool mapOverlapOn() const { return map_overlap_; }
  const uint64_t* mapFrameOverlap() const { return map_frame_overlap_; }
  // additive: one frame straight from sensor records — float32 (x, y, z, intensity ...) `stride_floats` apart, range
  // filter and optional KITTI correction as in apps/cpp_runners/bin_runner.cpp:126-166 — ingest, deskew, build and
  // registration all on the device (implies the device front-end for this frame)
  void computeRecords(const double& curr_stamp, const float* records, size_t n_records, int stride_floats, double min_range,
                      double max_range, bool kitti_correction);

  // additive: one frame straight from a driver's BYTE records with a time field (a PointCloud2-style buffer: `layout.step` bytes
  // apart, float32 x / y / z and a uint32 / float32 / float64 time at byte offsets, any alignment — madicp_record_layout).
  // The frame of computeSourcesStamped (below) for ONE plain source — identity extrinsic, the clock as it is — behind this call's
  // own refusals.  Device front-end: range filter, compaction and the stamps normalised over the scan, on the device — then,
  // where the reference deskews, madicp_cloud_deskew_own_stamps from the stamps the cloud carries, build and registration: the
  // time column never exists on the host.  Host front-end: the host twin (ingest_records.h), then
  // deskew_cloud_stamped and the host builder — the same bits.  t_range: null = the min / max time over the message, else
  // {t_begin, t_end}.  With layout.t_type == kTimeNone the frame is computeRecords' on the same coordinates, azimuth deskew
  // included; with deskew = false the time field is ignored entirely.  No look-ahead for records.  std::invalid_argument for
  // no records or a layout / t_range the ingest refuses.
  void computeRecordsStamped(const double& curr_stamp, const void* data, size_t n_records, const RecordLayout& layout, double min_range,
                             double max_range, bool kitti_correction, const double* t_range);
  // ... with one more field of the record carried as the points' attribute (above: registeredScanAttribute)
  void computeRecordsStamped(const double& curr_stamp, const void* data, size_t n_records, const RecordLayout& layout, double min_range,
                             double max_range, bool kitti_correction, const double* t_range, const AttrField& attribute);

  // additive: one frame from SEVERAL sensors' byte records (a multi-head rig: every source in its own sensor frame, with its own
  // layout, range bounds, sensor -> base extrinsic and time scale / offset onto one common clock — RecordSource, ingest_point.h).
  // Device front-end: madicp_cloud_ingest_sources — one staged copy, one chain of launches, one synchronisation whatever n is —
  // then deskew by the merged cloud's own stamps, build and registration, as computeRecordsStamped.  Host front-end: the host
  // twin (ingest_records.h: ingest_sources), then computeStamped / compute — the same bits.  t_range: null = the min / max time
  // over all sources on the common clock, else {t_begin, t_end} there.  With deskew = false the time fields and t_range are
  // ignored.  std::invalid_argument for what the ingest refuses (record_sources_refusal) and when no record survives.
  void computeSourcesStamped(const double& curr_stamp, const RecordSource* sources, int n_sources, const double* t_range);

  // additive: the keyframe map sharded over the ranks of a node.  Every rank runs ONE Pipeline and is
  // fed the same scans in the same order; setShard(rank, world) makes this one keep the tree of a keyframe only when
  // keyframe_owner(ordinal, world) == rank (csrc/common/keyframe_owner.h; ordinal: promotion order, the first scan is 0) and
  // register against its own trees alone — the library joins the ranks' adders round by round, because the process-wide
  // context (madicp_host_device_ctx()) holds a communicator of `world` ranks, which the CALLER installs before the first
  // compute() (madicp_comm_init / madicp_comm_init_host, optionally the peer mailboxes; Python: sharded.shard_pipeline does all
  // of it).  Every rank ends each registration with the same X, H, b and matched count bit for bit, so every rank takes the
  // same promotion decision without any further exchange: keyframeID(), keyframePose(), isMapUpdated(), currentID(),
  // numKeyframes() and modelLeaves() answer on every rank as on one GPU (a non-owner keeps a promoted tree's leaf means as a
  // host copy and gives the tree's HBM back).  Each rank still builds / deskews every scan itself and keeps the whole frame
  // window resident: any frame may be promoted.
  // Only legal before the first compute() (std::logic_error after it); std::invalid_argument unless 0 <= rank < world, and for
  // realtime = true with world > 1 (the round count comes from each rank's own wall clock and would differ between ranks,
  // which a collective does not survive).  world == 1: exactly the unsharded Pipeline.  prefetch() stays legal.
  // A communicator failure (MADICP_ERR_COMM from the submission or the collect: a rank that never joined, a broken transport)
  // surfaces from compute() as the std::runtime_error of every device failure; the ranks' states may have parted by then, so
  // the Pipeline — on every rank — is unusable from there on: destroy it, re-create the communicator, start a new one.
  void setShard(int rank, int world);
  int shardRank() const { return ledger_.rank(); }
  int shardWorld() const { return ledger_.world(); }
  size_t numLocalKeyframes() const { return ledger_.numLocal(); }  // keyframes whose tree THIS rank holds

  // instrumentation (not in the reference)
  double lastInliersRatio() const { return last_inliers_ratio_; }
  int lastRounds() const { return last_rounds_; }  // GN rounds the last frame ran (realtime = true can cut them short)
  // Test seam for realtime = true: with pre_ms >= 0 the wall clock of the budget rule (pipeline.cpp:160-169) is replaced by
  // a model — this frame's preprocessing took pre_ms, a GN round takes round_ms — so the round count is a deterministic
  // function that can be held to the reference's per-round check (tests/test_boundary.py); pre_ms < 0: the wall clock again.
  void setTimingForTest(double pre_ms, double round_ms) { virtual_pre_ms_ = pre_ms; virtual_round_ms_ = round_ms; }
  double lastIcpMs() const { return last_icp_ms_; }
  double lastBuildMs() const { return last_build_ms_; }
  // the last frame's registration split: submission, the look-ahead begun beside it, the wait for the result (ms)
  std::array<double, 3> lastIcpPhasesMs() const { return {icp_.phase_ms_[0], icp_.phase_ms_[1], icp_.phase_ms_[2]}; }
  size_t numKeyframes() const { return keyframes_.size(); }
  size_t lookAheadHits() const { return look_ahead_hits_; }  // frames whose tree had been built ahead (prefetch)

  static Matrix4d toMatrix(const Pose& p);

 protected:
  void initialize(const double& curr_stamp, ContainerType& curr_cloud);
  void deskew(ContainerType& curr_cloud, const Pose& T_prev, const Pose& T_now, const DeskewOrder* prep = nullptr);
  void naiveVelocity(const Pose& T_prev, const Pose& T_now, double* vel6) const;  // pipeline.cpp:82-86
  // deskew (if due; from `stamps`, one per point, when given) + build + release of the cloud
  // (`own_stamps`: from the stamps the cloud carries itself — madicp_cloud_ingest_records)
  std::unique_ptr<MADtree> buildOnDevice(int cloud_id, const double* stamps = nullptr, size_t n_stamps = 0, bool own_stamps = false);
  std::unique_ptr<MADtree> uploadAndBuild(const Vector3d* cloud, size_t n, const double* stamps = nullptr);  // madicp_cloud_upload + buildOnDevice
  void ingestPrologue();  // the builder's scratch is this frame's: no look-ahead of this Pipeline or another one holds it
  template <class Ingest>  // (pipeline.cpp only) the device half of computeRecords / computeSources: `ingest` returns the cloud id
  void computeIngested(const double& curr_stamp, bool own_stamps, Ingest&& ingest);
  // computeSourcesStamped behind its refusals; computeRecordsStamped is this for the one plain source
  void computeSources(const double& curr_stamp, const RecordSource* sources, int n_sources, const double* t_range, const char* who);
  void computeWithTree(const double& curr_stamp, std::unique_ptr<MADtree> current_tree, ContainerType* curr_cloud, double t_pre);

  MADicp icp_;
  VelEstimator vel_estimator_;
  Pose frame_to_map_;
  Pose keyframe_to_map_;
  double current_velocity_[6];
  std::deque<std::unique_ptr<Frame>> keyframes_;
  std::deque<std::unique_ptr<Frame>> frames_;
  std::vector<Pose> trajectory_;
  MADtree* current_tree_view_ = nullptr;  // the last scan's tree (owned by a Frame in frames_ / keyframes_)
  const ContainerType* current_leaves_host_ = nullptr;  // ... or, sharded, its leaf means where the tree was promoted and released
  KeyframeLedger ledger_;                 // which keyframe ordinals are in the window, which of them this rank owns
  void checkShardCommunicator();          // sharded: the context's communicator is the one setShard() was told about
  void pushKeyframe(std::unique_ptr<Frame> frame);  // keyframes_ push + eviction by the ledger; a non-owner releases the tree
  size_t current_num_leaves_ = 0;
  // what a look-ahead result is matched to its scan by: size, end points and a digest of a strided sample of the points
  struct DevKey {
    size_t n = 0;
    Vector3d first{}, last{};
    uint64_t digest = 0;
    static DevKey of(const ContainerType& c);
    bool matches(const ContainerType& c) const;
    static DevKey of(const Vector3d* c, size_t n);
    bool matches(const Vector3d* c, size_t n) const;
  };
  // look-ahead builds: up to three scans ahead of the one being consumed (kMaxLookAhead), each matched to its scan by its
  // key (a prefetch(i + 1) issued BEFORE compute(i) must not cost scan i its tree)
  template <class T>
  struct LookAhead {
    DevKey key;
    std::future<T> result;
  };
  using Prefetched = LookAhead<LinearTree>;
  // the look-ahead made for exactly this scan, if `ahead` holds one: handed out in *hit and taken off the queue, with the
  // older ones in front of it (scans that never came; each is waited for)
  template <class T>
  static bool takeLookAhead(std::deque<LookAhead<T>>& ahead, const Vector3d* cloud, size_t n, LookAhead<T>* hit);
  static constexpr size_t kMaxLookAhead = 4;  // scan i being consumed, up to three more building
  std::deque<Prefetched> prefetched_;
  void waitPrefetched();  // every look-ahead build has finished (their trees stay available)
  // device front-end: ONE construction in flight on the library's build stream (`dev_pending_`), and the tree of the scan
  // before it, collected when the next look-ahead was begun (`dev_ready_`) — with the call order prefetch(i + 1),
  // compute(i) the tree of scan i is collected at prefetch(i + 1) and scan i + 1 is built while scan i registers
  // deskewed datasets: the tree needs the two previous poses, but the azimuth order of the scan does not — that half of
  // Pipeline::deskew (atan2 per point, the sort: most of a deskewed frame on the host) is what prefetch() computes ahead
  using DeskewAhead = LookAhead<DeskewOrder>;
  std::deque<DeskewAhead> deskew_ahead_;
  unsigned dev_pending_ = 0;  // ticket (MADtree::beginDeviceBuild), 0: none
  ContainerType dev_next_cloud_;  // the scan prefetch() was given, staged and begun by compute() WHILE its registration is in
                                  // flight (the host side of a begin — 3 MB into pinned memory, ~60 launches — is a third of
                                  // a millisecond that would otherwise sit in front of the registration)
  bool dev_next_staged_ = false;  // dev_next_cloud_ holds a scan that has not been begun (the vector keeps its memory between scans)
  void beginStagedLookAhead();
  DevKey dev_pending_key_, dev_ready_key_;
  std::unique_ptr<MADtree> dev_ready_;
  void collectDeviceLookAhead();  // dev_pending_ -> dev_ready_
  void dropDeviceLookAhead(bool staged_too = true);  // forget both (and the scan staged for the next frame)
  // the retained scan (setKeepScan): a resident cloud of the context generation that issued its id, or a host copy
  bool keep_scan_ = false, have_kept_ = false;
  int kept_cloud_id_ = -1;
  unsigned kept_generation_ = 0;
  ContainerType kept_host_;
  size_t kept_n_ = 0;
  // its attribute column: inside the resident cloud, or kept_attr_ beside the host copy.  A records frame announces its column
  // (frame_attr_type_, host front-end: the words in frame_attr_) before it enters compute*; whoever retains the scan takes it over
  bool kept_has_attr_ = false;
  int kept_attr_type_ = 0;
  std::vector<uint32_t> kept_attr_;
  int frame_attr_type_ = 0;  // kAttrNone: the frame being computed carries no attribute
  std::vector<uint32_t> frame_attr_;
  void permuteFrameAttr(const DeskewOrder& order);  // host azimuth deskew: the column follows the points
  void dropKeptScan();                        // forget it; the device buffer goes back to the pool
  void keepHostScan(const ContainerType& c);  // host front-end: the copy, when the option (or map accumulation) is on
  // map accumulation (setMapAccumulation): map_spec_ is what the map is made from (voxel 0: off), map_ the map itself — one
  // MapStore (map_store.h), null until the first frame is folded.  foldFrame decides where it lives, once: a fresh map goes where
  // that frame's scan does — the device map, with its id and context generation inside the store, or the host twin.  From then on
  // the retained scan reaches the store as a ScanRef (keptScan) and, when the front-end was switched and it lies on the other
  // side, crosses once per frame through a ScanBorrow, its column with it.  No method below knows which side the map is on.
  MapSpec map_spec_;
  bool map_keyframes_only_ = false, map_overflowed_ = false;
  int map_attr_type_ = 0;
  std::unique_ptr<MapStore> map_;
  void dropMap();
  ScanRef keptScan() const;                                // the retained scan, where it lies
  void mapCheck(int rc, const std::string& who) const;     // a refusal of the store: std::runtime_error, `who` + the store's reason
  size_t settleRemoval(int rc, int64_t removed, int64_t mark);  // the log-full / cursor / mapRemoved() rule of every removal
  // what mapCloud .. mapSurfels share: the refusals, in `who`'s name (missing: why the map lacks the column asked for, or null);
  // false: the window is empty.  mapColumn (pipeline.cpp only): then the rows of the window, one column of MapColumns, from the store
  bool mapWindow(const std::string& who, const char* missing, const void* out, const char* holds, size_t capacity, size_t first_row);
  template <class T>
  size_t mapColumn(const char* name, const char* missing, T* MapColumns::*column, T* out, size_t capacity, size_t first_row);
  // setMapRange: the centre of the last prune and the position of the frame before this one (foldFrame's policy), the consumer's
  // cursor (mapNewRows) and the rows removed so far
  double map_range_ = 0.0;
  double map_prune_center_[3] = {0.0, 0.0, 0.0}, map_last_position_[3] = {0.0, 0.0, 0.0};
  bool map_have_center_ = false, map_have_last_ = false;
  size_t map_cursor_ = 0, map_removed_ = 0;
  bool map_clearing_ = false;  // setMapClearing
  bool map_track_removed_ = false, map_log_full_ = false;  // setMapTrackRemoved; a removal was skipped because the log is full
  double map_clear_margin_ = 0.0, map_clear_origin_[3] = {0.0, 0.0, 0.0};
  bool map_overlap_ = false;  // setMapOverlap: foldFrame asks the map about the frame before it folds it
  int map_overlap_reach_ = 1;
  double map_overlap_max_dist_ = kQueryNoDistance;
  uint64_t map_frame_overlap_[3] = {0, 0, 0};
  bool map_alignment_ = false;  // setMapAlignment: foldFrame registers the frame against the map before it folds it, and only reports
  int map_align_iterations_ = 5;
  AlignParams map_align_params_;
  FrameAlignment map_frame_alignment_;
  size_t pruneMapAt(const double center[3], double radius);  // MapStore::prune with the cursor as watermark (mapPrune's refusals; 0 before the first fold)
  void foldFrame();  // the end of every compute*: folds the retained scan, then lets it go unless setKeepScan holds it
  double virtual_pre_ms_ = -1.0, virtual_round_ms_ = 0.0;
  int last_rounds_ = 0;
  double round_ms_estimate_ = 0.05;  // device time of one GN round, from the previous frame (realtime budget)
  bool device_frontend_ = false;
  bool deskew_, realtime_;
  int num_keyframes_, num_threads_, max_parallel_levels_;
  double sensor_hz_, b_max_, p_th_, b_min_;
  size_t seq_ = 0;
  size_t seq_keyframe_ = 0;
  bool is_initialized_ = false;
  bool is_map_updated_ = false;
  float loop_time_;
  double last_inliers_ratio_ = 0., last_icp_ms_ = 0., last_build_ms_ = 0.;
  size_t look_ahead_hits_ = 0;
};

}  // namespace madicp_host

// the reference declares these names at global scope; keep them reachable the same way
using madicp_host::ContainerType;
using madicp_host::Pipeline;
