#include "pipeline.h"

#include "cloud_export.h"
#include "deskew.h"
#include "device.h"
#include "task_pool.h"

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <limits>
#include <stdexcept>
#include <string>
#include <utility>

namespace madicp_host {

namespace {
double now_ms() {
  using clk = std::chrono::steady_clock;
  return std::chrono::duration<double, std::milli>(clk::now().time_since_epoch()).count();
}
}  // namespace

Matrix4d Pipeline::toMatrix(const Pose& p) {
  Matrix4d M;
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) M(r, c) = p.R[3 * r + c];
    M(r, 3) = p.t[r];
  }
  M(3, 0) = M(3, 1) = M(3, 2) = 0.0;
  M(3, 3) = 1.0;
  return M;
}

Pipeline::Pipeline(double sensor_hz, bool deskew, double b_max, double rho_ker, double p_th, double b_min,
                   double b_ratio, int num_keyframes, int num_threads, bool realtime)
  : icp_(b_max, rho_ker, b_ratio, num_threads),
    vel_estimator_(sensor_hz),
    deskew_(deskew),
    realtime_(realtime),
    num_keyframes_(num_keyframes),
    num_threads_(num_threads),
    sensor_hz_(sensor_hz),
    b_max_(b_max),
    p_th_(p_th),
    b_min_(b_min) {
  ledger_.configure(0, 1, num_keyframes);
  frame_to_map_ = Pose::identity();
  keyframe_to_map_ = Pose::identity();
  std::memset(current_velocity_, 0, sizeof(current_velocity_));
  loop_time_ = (1. / sensor_hz_) * 1000;
  max_parallel_levels_ = static_cast<int>(std::log2(num_threads));  // pipeline.cpp:64
  TaskPool::instance().set_limit(num_threads);  // omp_set_num_threads(num_threads), pipeline.cpp:65
  // The device front-end is the DEFAULT: an unmodified caller gets deskew (where the dataset asks for it) and MAD-tree
  // construction on the MI355X.  Round 5 made it so for deskew = false (tests/test_gpu_frontend_oracle.py holds that path to
  // the oracle pipeline directly); round 6 for deskew = true too: ONE frame — deskew, build, registration — from the oracle's
  // state is the oracle's frame to 1e-5 m / 1e-5 rad (tests/test_gpu_deskew_one_step.py), and over a drive neither path is
  // bit-stable anyway (the reference is not against itself: tests/envelope.py), so nothing but 3 ms per frame spoke for the
  // host path there.  MAD_ICP_GPU_BUILD=0 keeps the host builder (the reference's trees bit for bit); setDeviceFrontEnd()
  // overrides the environment.
  device_frontend_ = true;
  if (const char* e = std::getenv("MAD_ICP_GPU_BUILD")) {
    if (e[0] == '1') device_frontend_ = true;
    if (e[0] == '0') device_frontend_ = false;
  }
}

void Pipeline::waitPrefetched() {
  for (Prefetched& p : prefetched_)
    if (p.result.valid()) p.result.wait();
  for (DeskewAhead& a : deskew_ahead_)
    if (a.result.valid()) a.result.wait();
}

template <class T>
bool Pipeline::takeLookAhead(std::deque<LookAhead<T>>& ahead, const Vector3d* cloud, size_t n, LookAhead<T>* hit) {
  for (size_t q = 0; q < ahead.size(); ++q) {
    if (!ahead[q].key.matches(cloud, n)) continue;
    for (size_t d = 0; d < q; ++d) {
      if (ahead.front().result.valid()) ahead.front().result.wait();
      ahead.pop_front();
    }
    *hit = std::move(ahead.front());
    ahead.pop_front();
    return true;
  }
  return false;
}

// A look-ahead result belongs to the scan it was computed from: size, end points and a digest of a strided sample of the
// points (up to 1024 of them, every coordinate's bit pattern) — a re-filtered, jittered or padded copy with the same size
// and end points does not get another scan's tree.
static uint64_t cloud_digest(const Vector3d* c, size_t n) {
  const size_t step = std::max<size_t>(1, n / 1024);
  uint64_t h = 0x9e3779b97f4a7c15ull ^ n;
  for (size_t i = 0; i < n; i += step) {
    uint64_t w[3];
    std::memcpy(w, c[i].data(), 24);
    for (int k = 0; k < 3; ++k) {
      h ^= w[k] + 0x9e3779b97f4a7c15ull + (h << 6) + (h >> 2);
      h = (h << 13) | (h >> 51);
    }
  }
  return h;
}
Pipeline::DevKey Pipeline::DevKey::of(const Vector3d* c, size_t n) {
  DevKey k;
  k.n = n;
  if (n) {
    k.first = c[0];
    k.last = c[n - 1];
    k.digest = cloud_digest(c, n);
  }
  return k;
}
bool Pipeline::DevKey::matches(const Vector3d* c, size_t count) const {
  return n == count && n > 0 && std::memcmp(first.data(), c[0].data(), 24) == 0 &&
         std::memcmp(last.data(), c[n - 1].data(), 24) == 0 && digest == cloud_digest(c, n);
}
Pipeline::DevKey Pipeline::DevKey::of(const ContainerType& c) { return of(c.data(), c.size()); }
bool Pipeline::DevKey::matches(const ContainerType& c) const { return matches(c.data(), c.size()); }

void Pipeline::collectDeviceLookAhead() {
  if (!dev_pending_) return;
  const unsigned ticket = dev_pending_;
  dev_pending_ = 0;
  dev_ready_.reset();  // (an older collected tree whose scan never came)
  dev_ready_ = MADtree::collectDeviceBuild(ticket);  // (null: cancelled by a synchronous build of another Pipeline)
  dev_ready_key_ = dev_pending_key_;
}

void Pipeline::beginStagedLookAhead() {
  if (!dev_next_staged_) return;
  dev_next_staged_ = false;  // (the buffer keeps its memory for the next scan: see prefetchView)
  collectDeviceLookAhead();  // (the one slot: whatever was in flight is collected first)
  dev_pending_ = MADtree::beginDeviceBuild(dev_next_cloud_, b_max_, b_min_);
  if (!dev_pending_) return;
  dev_pending_key_ = DevKey::of(dev_next_cloud_);
}

void Pipeline::dropDeviceLookAhead(bool staged_too) {
  if (staged_too) dev_next_staged_ = false;
  if (dev_pending_) {
    MADtree::cancelDeviceBuild(dev_pending_);
    dev_pending_ = 0;
  }
  dev_ready_.reset();
}

Pipeline::~Pipeline() {  // Frames own their trees; trees release their HBM copies
  waitPrefetched();
  try {
    dropDeviceLookAhead();
  } catch (...) {
  }
  dropKeptScan();
  dropMap();
}

// ---- the retained scan (pipeline.h: setKeepScan / registeredScan) ---------------------------------------------------------------
void Pipeline::dropKeptScan() {
  if (kept_cloud_id_ >= 0) {
    DeviceLock lock(Device::mutex());
    // (an id belongs to the context generation that issued it: after Device::shutdown() there is nothing to give back)
    if (madicp_ctx* ctx = Device::current(kept_generation_)) madicp_cloud_release(ctx, kept_cloud_id_);
    kept_cloud_id_ = -1;
  }
  kept_host_.clear();
  kept_attr_.clear();
  kept_has_attr_ = false;
  kept_attr_type_ = kAttrNone;
  have_kept_ = false;
  kept_n_ = 0;
}

void Pipeline::keepHostScan(const ContainerType& c) {
  // (the column the frame announced is taken over here, or let go with the scan)
  const int attr_type = frame_attr_type_;
  std::vector<uint32_t> attr = std::move(frame_attr_);
  frame_attr_type_ = kAttrNone;
  frame_attr_.clear();
  if (!keep_scan_ && map_spec_.voxel == 0.0) return;
  dropKeptScan();
  kept_host_ = c;
  kept_n_ = c.size();
  have_kept_ = true;
  if (attr_type != kAttrNone && attr.size() == c.size()) {
    kept_attr_ = std::move(attr);
    kept_has_attr_ = true;
    kept_attr_type_ = attr_type;
  }
}

// The host azimuth deskew leaves the point with the i-th smallest azimuth at position i (deskew.h): the frame's column follows.
// With ties the order is std::sort's own of (azimuth, point) pairs; sorting (azimuth, index) pairs with the same comparator makes
// the same comparisons in the same sequence — the algorithm never looks at the payload — and so leaves the same permutation.
void Pipeline::permuteFrameAttr(const DeskewOrder& order) {
  const size_t n = frame_attr_.size();
  if (order.azimuth.size() != n) return;
  std::vector<uint32_t> out(n);
  if (!order.ties && order.order.size() == n) {
    for (size_t i = 0; i < n; ++i) out[i] = frame_attr_[order.order[i]];
  } else {
    std::vector<std::pair<double, uint32_t>> sorted(n);
    for (size_t i = 0; i < n; ++i) sorted[i] = std::make_pair(order.azimuth[i], frame_attr_[i]);
    std::sort(sorted.begin(), sorted.end(),
              [](const std::pair<double, uint32_t>& a, const std::pair<double, uint32_t>& b) -> bool { return a.first < b.first; });
    for (size_t i = 0; i < n; ++i) out[i] = sorted[i].second;
  }
  frame_attr_.swap(out);
}

void Pipeline::setKeepScan(bool on) {
  if (on == keep_scan_) return;
  keep_scan_ = on;
  if (on) {
    dropDeviceLookAhead();  // (a tree built ahead comes without its scan: the next frame builds synchronously)
  } else {
    dropKeptScan();
  }
}

// ---- map accumulation (pipeline.h: setMapAccumulation) -----------------------------------------------------------------------
// The map itself is a MapStore (map_store.h): the device map or the host twin, decided once, in foldFrame, when the first frame is
// folded.  Everything below asks the store and turns its return codes into this class's exceptions — written once for both sides.
void Pipeline::dropMap() {
  map_.reset();  // (a device map gives its id back while the context generation that issued it lives)
  map_overflowed_ = false;
  map_have_center_ = map_have_last_ = false;
  map_cursor_ = map_removed_ = 0;
  map_log_full_ = false;
}

void Pipeline::mapCheck(int rc, const std::string& who) const {
  if (rc != MADICP_OK) throw std::runtime_error(who + map_->lastError());
}

ScanRef Pipeline::keptScan() const {
  if (kept_cloud_id_ >= 0) return ScanRef::cloud(kept_cloud_id_, kept_generation_, static_cast<int64_t>(kept_n_), kept_has_attr_);
  const bool attr = kept_has_attr_ && kept_attr_.size() == kept_host_.size();
  return ScanRef::host(kept_host_.empty() ? nullptr : kept_host_[0].data(), attr ? kept_attr_.data() : nullptr,
                       static_cast<int64_t>(kept_host_.size()));
}

void Pipeline::setMapAccumulation(double voxel_size, bool keyframes_only, size_t max_points, bool with_attribute, const uint32_t* evidence,
                                  uint32_t moments_max_count) {
  if (!std::isfinite(voxel_size) || voxel_size < 0.0)
    throw std::invalid_argument("Pipeline::setMapAccumulation: voxel_size must be finite and >= 0 (0 = off)");
  if (voxel_size > 0.0 && (max_points < 1 || max_points > static_cast<size_t>(kMapMaxRows)))
    throw std::invalid_argument("Pipeline::setMapAccumulation: max_points must be 1 .. 2^30");
  if (voxel_size > 0.0 && evidence)
    if (const char* why = map_evidence_refusal(evidence[0], evidence[1], evidence[2]))
      throw std::invalid_argument(std::string("Pipeline::setMapAccumulation: ") + why);
  if (voxel_size > 0.0 && moments_max_count > 0)
    if (const char* why = map_moments_refusal(moments_max_count)) throw std::invalid_argument(std::string("Pipeline::setMapAccumulation: ") + why);
  MapSpec spec;  // (off: the default spec, whatever else was asked for)
  if (voxel_size > 0.0) {
    spec.voxel = voxel_size;
    spec.max_rows = static_cast<int64_t>(max_points);
    spec.first_rows = std::min<int64_t>(spec.max_rows, int64_t(1) << 18);
    spec.with_attr = with_attribute;
    spec.with_ev = evidence != nullptr;
    if (evidence) std::copy(evidence, evidence + 3, spec.ev);
    spec.mom = moments_max_count;
  }
  if (spec == map_spec_ && (spec.voxel == 0.0 || keyframes_only == map_keyframes_only_)) return;
  dropMap();
  const bool was_on = map_spec_.voxel > 0.0;
  map_spec_ = spec;
  map_keyframes_only_ = keyframes_only;
  map_attr_type_ = kAttrNone;
  if (spec.voxel > 0.0) {
    if (!was_on) dropDeviceLookAhead();  // (a tree built ahead comes without its scan: the next frame builds synchronously)
  } else {
    map_track_removed_ = false;  // (setMapTrackRemoved is an option of the accumulation: off with it)
    if (!keep_scan_) dropKeptScan();
  }
}

void Pipeline::foldFrame() {
  if (map_spec_.voxel == 0.0) return;
  std::fill(map_frame_overlap_, map_frame_overlap_ + 3, uint64_t(0));  // (a frame that is not folded answers zeros)
  map_frame_alignment_.valid = false;                                    // (... and no alignment)
  if (have_kept_ && !map_overflowed_ && (!map_keyframes_only_ || is_map_updated_)) {
    // (b) a fold the capacity rule would refuse: the rows out of range of the frame before this one give way first, once
    if (map_range_ > 0.0 && map_ && map_have_last_ && mapSize() + kept_n_ > static_cast<size_t>(map_spec_.max_rows)) {
      pruneMapAt(map_last_position_, map_range_);
      std::copy(map_last_position_, map_last_position_ + 3, map_prune_center_);
      map_have_center_ = true;
    }
    // a fresh map goes where the frame's scan lives; a device map's frame holds the device lock from the creation to the clearing
    const bool device = map_ ? map_->onDevice() : kept_cloud_id_ >= 0;
    std::unique_lock<std::recursive_mutex> lock(Device::mutex(), std::defer_lock);
    if (device) lock.lock();
    if (!map_) {
      if (device)
        map_ = make_device_map_store(map_spec_);
      else
        map_ = std::make_unique<HostMapStore>(map_spec_, fetch_resident_scan);
      if (map_track_removed_) mapCheck(map_->trackRemoved(true), "Pipeline: ");
    }
    if (device) MADtree::cancelDeviceBuild(0);  // the fold needs the builder's scratch: a look-ahead of another Pipeline gives way
    int64_t added = 0, rows = 0;
    int rc;
    {
      // a scan from the other side (the front-end was switched) crosses once — its column with it — for the query, the fold and the clearing
      ScanBorrow borrow(*map_, keptScan());
      const ScanRef& scan = borrow.scan();
      if (map_overlap_)  // setMapOverlap: what the map knows of this frame, asked before the frame is folded
        mapCheck(map_->query(scan, frame_to_map_.R, frame_to_map_.t, map_overlap_reach_, map_overlap_max_dist_, nullptr, nullptr, nullptr, nullptr,
                             nullptr, 0, map_frame_overlap_),
                 "Pipeline: the overlap query: ");
      if (map_alignment_ && map_spec_.mom > 0) {  // setMapAlignment: the frame registered against the map as it stands, reported only
        FrameAlignment& a = map_frame_alignment_;
        std::vector<double> trace(static_cast<size_t>(kAlignTraceRow) * (map_align_iterations_ + 1));
        std::vector<uint64_t> counts(static_cast<size_t>(kAlignCounts) * (map_align_iterations_ + 1));
        mapCheck(map_->align(scan, frame_to_map_.R, frame_to_map_.t, map_align_params_, map_align_iterations_, a.R, a.t, trace.data(),
                             counts.data(), nullptr, nullptr, 0),
                 "Pipeline: the frame's alignment: ");
        a.valid = true;
        a.iterations = map_align_iterations_;
        const double* last = trace.data() + static_cast<size_t>(kAlignTraceRow) * map_align_iterations_;
        const uint64_t* last_counts = counts.data() + static_cast<size_t>(kAlignCounts) * map_align_iterations_;
        std::memcpy(a.sums, last + 12, sizeof(a.sums));
        std::memcpy(a.counts, last_counts, sizeof(a.counts));
        a.first_chi2 = trace[kAlignTraceRow - 1];
        std::copy(counts.begin(), counts.begin() + kAlignCounts, a.first_counts);
      }
      rc = map_->insert(scan, frame_to_map_.R, frame_to_map_.t, &added, &rows);
      if (rc != MADICP_ERR_CAPACITY) mapCheck(rc, "Pipeline: the fold: ");
      // setMapClearing: what the cloud just folded sees through leaves, before the range prune below
      if (rc == MADICP_OK && map_clearing_) {
        int64_t removed = 0, mark = 0;
        const int crc = map_->clearRays(scan, frame_to_map_.R, frame_to_map_.t, map_clear_origin_, map_clear_margin_,
                                        static_cast<int64_t>(map_cursor_), &removed, &rows, &mark);
        settleRemoval(crc, removed, mark);
      }
    }
    if (device) lock.unlock();
    if (rc == MADICP_ERR_CAPACITY) map_overflowed_ = true;
    if (rc != MADICP_OK) std::fill(map_frame_overlap_, map_frame_overlap_ + 3, uint64_t(0));  // (refused: not folded)
    if (rc != MADICP_OK) map_frame_alignment_.valid = false;
    if (rc == MADICP_OK && map_spec_.with_attr && kept_has_attr_) map_attr_type_ = kept_attr_type_;
    // (a) the vehicle has moved a quarter of the range since the last prune: squared distances, fp64 — the poses alone decide
    if (rc == MADICP_OK && map_range_ > 0.0) {
      const double* p = frame_to_map_.t;
      const double dx = p[0] - map_prune_center_[0], dy = p[1] - map_prune_center_[1], dz = p[2] - map_prune_center_[2];
      const double step = map_range_ / 4.0;
      const bool due = map_have_center_ && dx * dx + (dy * dy + dz * dz) >= step * step;
      if (due) pruneMapAt(p, map_range_);
      if (due || !map_have_center_) std::copy(p, p + 3, map_prune_center_);
      map_have_center_ = true;
    }
  }
  std::copy(frame_to_map_.t, frame_to_map_.t + 3, map_last_position_);
  map_have_last_ = true;
  if (!keep_scan_) dropKeptScan();
}

void Pipeline::setMapRange(double radius) {
  if (!std::isfinite(radius) || radius < 0.0 || !std::isfinite(radius * radius))
    throw std::invalid_argument("Pipeline::setMapRange: radius must be finite and >= 0 (0 = off), and so must its square");
  map_range_ = radius;
}

// What every removal ends with — foldFrame's clearing, pruneMapAt, mapClearRays: a removal refused because the log is full is
// skipped (map and mirror agree, mapRemovedLogFull() says so); any other refusal is an error; else the cursor follows the rows
// that closed up below it.  Returns the rows removed.
size_t Pipeline::settleRemoval(int rc, int64_t removed, int64_t mark) {
  if (rc == MADICP_ERR_CAPACITY && map_track_removed_) {
    map_log_full_ = true;
    return 0;
  }
  mapCheck(rc, "Pipeline: a removal from the map: ");
  map_cursor_ = static_cast<size_t>(mark);
  map_removed_ += static_cast<size_t>(removed);
  return static_cast<size_t>(removed);
}

size_t Pipeline::pruneMapAt(const double center[3], double radius) {
  // (held to the one rule here, so also while no frame has been folded yet: then there is nothing to remove)
  if (const char* why = map_prune_refusal(center, radius)) throw std::invalid_argument(std::string("Pipeline::mapPrune: ") + why);
  int64_t removed = 0, rows = 0, mark = static_cast<int64_t>(map_cursor_);
  int rc = MADICP_OK;
  if (map_) rc = map_->prune(center, radius, static_cast<int64_t>(map_cursor_), &removed, &rows, &mark);
  if (rc == MADICP_ERR_INVALID) throw std::invalid_argument("Pipeline::mapPrune: " + map_->lastError());
  return settleRemoval(rc, removed, mark);
}

size_t Pipeline::mapPrune(const double center[3], double radius) {
  if (map_spec_.voxel == 0.0) throw std::logic_error("Pipeline::mapPrune: setMapAccumulation(voxel_size > 0) first");
  if (!center) throw std::invalid_argument("Pipeline::mapPrune: null center");
  return pruneMapAt(center, radius);
}

void Pipeline::setMapClearing(bool on, double margin, const double origin[3]) {
  const double zero[3] = {0.0, 0.0, 0.0};
  const double* o = origin ? origin : zero;
  if (!std::isfinite(margin) || margin < 0.0) throw std::invalid_argument("Pipeline::setMapClearing: margin must be finite and >= 0");
  if (!std::isfinite(o[0]) || !std::isfinite(o[1]) || !std::isfinite(o[2]))
    throw std::invalid_argument("Pipeline::setMapClearing: origin must be finite");
  map_clearing_ = on;
  map_clear_margin_ = margin;
  std::copy(o, o + 3, map_clear_origin_);
}

size_t Pipeline::mapClearRays(const double* xyz, size_t n, const double R[9], const double t[3], const double origin[3], double margin) {
  if (map_spec_.voxel == 0.0) throw std::logic_error("Pipeline::mapClearRays: setMapAccumulation(voxel_size > 0) first");
  if ((!xyz && n > 0) || !R || !t || !origin) throw std::invalid_argument("Pipeline::mapClearRays: null argument");
  if (const char* why = map_clear_refusal(R, t, origin, margin)) throw std::invalid_argument(std::string("Pipeline::mapClearRays: ") + why);
  int64_t removed = 0, rows = 0, mark = static_cast<int64_t>(map_cursor_);
  int rc = MADICP_OK;  // (no frame folded yet: nothing to remove)
  if (map_)
    rc = map_->clearRays(ScanRef::host(xyz, nullptr, static_cast<int64_t>(n)), R, t, origin, margin, static_cast<int64_t>(map_cursor_), &removed,
                         &rows, &mark);
  if (rc == MADICP_ERR_INVALID) throw std::invalid_argument("Pipeline::mapClearRays: " + map_->lastError());
  return settleRemoval(rc, removed, mark);
}

void Pipeline::setMapOverlap(bool on, int reach, double max_dist) {
  if (reach != 0 && reach != 1) throw std::invalid_argument("Pipeline::setMapOverlap: reach must be 0 or 1");
  if (!(max_dist >= 0.0)) throw std::invalid_argument("Pipeline::setMapOverlap: max_dist must be >= 0 and not NaN");
  map_overlap_ = on;
  map_overlap_reach_ = reach;
  map_overlap_max_dist_ = max_dist;
  if (!on) std::fill(map_frame_overlap_, map_frame_overlap_ + 3, uint64_t(0));
}

void Pipeline::mapQuery(const double* xyz, size_t n, const double R[9], const double t[3], int reach, double max_dist, int32_t* row, double* d2,
                        uint64_t* keys, uint32_t* attr, uint32_t* ev, uint64_t counts[3]) {
  if (map_spec_.voxel == 0.0) throw std::logic_error("Pipeline::mapQuery: setMapAccumulation(voxel_size > 0) first");
  if (attr && !map_spec_.with_attr)
    throw std::logic_error("Pipeline::mapQuery: the map was made without the attribute (setMapAccumulation's with_attribute)");
  if (ev && !map_spec_.with_ev) throw std::logic_error("Pipeline::mapQuery: the map was made without evidence (setMapAccumulation's evidence)");
  if ((!xyz && n > 0) || !R || !t || !counts) throw std::invalid_argument("Pipeline::mapQuery: null argument");
  if (n > static_cast<size_t>(kMapMaxRows)) throw std::invalid_argument("Pipeline::mapQuery: at most 2^30 points");
  if (const char* why = map_query_refusal(R, t, reach, max_dist)) throw std::invalid_argument(std::string("Pipeline::mapQuery: ") + why);
  std::unique_ptr<MapStore> empty;  // before the first fold and for no point at all: an empty host map of the same kind answers
  if (!map_ || n == 0) {
    MapSpec kind = map_spec_;
    kind.first_rows = kind.max_rows = 1;
    empty = std::make_unique<HostMapStore>(kind);
  }
  MapStore& map = empty ? *empty : *map_;
  const int64_t n64 = static_cast<int64_t>(n);
  const int rc = map.query(ScanRef::host(xyz, nullptr, n64), R, t, reach, max_dist, row, d2, keys, attr, ev, n64, counts);
  if (rc == MADICP_ERR_INVALID) throw std::invalid_argument("Pipeline::mapQuery: " + map.lastError());
  if (rc != MADICP_OK) throw std::runtime_error("Pipeline::mapQuery: " + map.lastError());
}

void Pipeline::setMapAlignment(bool on, int iterations, const AlignParams& params) {
  if (iterations < 0 || iterations > kAlignMaxIterations) throw std::invalid_argument("Pipeline::setMapAlignment: iterations must be 0 .. 64");
  const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, z[3] = {0, 0, 0};
  if (const char* why = map_align_refusal(I, z, params.reach, params.max_dist, params.rho, params.min_count, params.flat))
    throw std::invalid_argument(std::string("Pipeline::setMapAlignment: ") + why);
  if (on && map_spec_.voxel > 0.0 && map_spec_.mom == 0)
    throw std::logic_error("Pipeline::setMapAlignment: the map was made without moments (setMapAccumulation's moments)");
  map_alignment_ = on;
  map_align_iterations_ = iterations;
  map_align_params_ = params;
  if (!on) map_frame_alignment_.valid = false;
}

void Pipeline::mapRegister(const double* xyz, size_t n, const double R[9], const double t[3], const AlignParams& params, int iterations,
                           double out_R[9], double out_t[3], double* trace, uint64_t* counts, int32_t* row, double* e) {
  if (map_spec_.voxel == 0.0) throw std::logic_error("Pipeline::mapRegister: setMapAccumulation(voxel_size > 0) first");
  if (map_spec_.mom == 0) throw std::logic_error("Pipeline::mapRegister: the map was made without moments (setMapAccumulation's moments)");
  if ((!xyz && n > 0) || !R || !t || !out_R || !out_t || !trace || !counts) throw std::invalid_argument("Pipeline::mapRegister: null argument");
  if (n > static_cast<size_t>(kMapMaxRows)) throw std::invalid_argument("Pipeline::mapRegister: at most 2^30 points");
  if (const char* why = map_align_refusal(R, t, params.reach, params.max_dist, params.rho, params.min_count, params.flat))
    throw std::invalid_argument(std::string("Pipeline::mapRegister: ") + why);
  if (iterations < 0 || iterations > kAlignMaxIterations) throw std::invalid_argument("Pipeline::mapRegister: iterations must be 0 .. 64");
  if ((row || e) && iterations > 0)
    throw std::invalid_argument("Pipeline::mapRegister: per-point buffers belong to the linearise-only form (iterations == 0)");
  std::unique_ptr<MapStore> empty;  // before the first fold and for no point at all: an empty host map of the same kind answers
  if (!map_ || n == 0) {
    MapSpec kind = map_spec_;
    kind.first_rows = kind.max_rows = 1;
    empty = std::make_unique<HostMapStore>(kind);
  }
  MapStore& map = empty ? *empty : *map_;
  const int64_t n64 = static_cast<int64_t>(n);
  const int rc = map.align(ScanRef::host(xyz, nullptr, n64), R, t, params, iterations, out_R, out_t, trace, counts, row, e, n64);
  if (rc == MADICP_ERR_INVALID) throw std::invalid_argument("Pipeline::mapRegister: " + map.lastError());
  if (rc != MADICP_OK) throw std::runtime_error("Pipeline::mapRegister: " + map.lastError());
}

void Pipeline::mapScorePoses(const double* xyz, size_t n, const double* poses, size_t n_poses, int reach, double max_dist, int64_t stride,
                             uint64_t* counts) {
  if (map_spec_.voxel == 0.0) throw std::logic_error("Pipeline::mapScorePoses: setMapAccumulation(voxel_size > 0) first");
  if ((!xyz && n > 0) || !poses || !counts) throw std::invalid_argument("Pipeline::mapScorePoses: null argument");
  if (n > static_cast<size_t>(kMapMaxRows)) throw std::invalid_argument("Pipeline::mapScorePoses: at most 2^30 points");
  const int64_t k64 = n_poses > static_cast<size_t>(kScoreMaxPoses) ? kScoreMaxPoses + 1 : static_cast<int64_t>(n_poses);
  if (const char* why = map_score_refusal(poses, k64, reach, max_dist, stride))
    throw std::invalid_argument(std::string("Pipeline::mapScorePoses: ") + why);
  std::unique_ptr<MapStore> empty;  // before the first fold and for no point at all: an empty host map of the same kind answers
  if (!map_ || n == 0) {
    MapSpec kind = map_spec_;
    kind.first_rows = kind.max_rows = 1;
    empty = std::make_unique<HostMapStore>(kind);
  }
  MapStore& map = empty ? *empty : *map_;
  const int rc = map.score(ScanRef::host(xyz, nullptr, static_cast<int64_t>(n)), poses, k64, reach, max_dist, stride, counts);
  if (rc == MADICP_ERR_INVALID) throw std::invalid_argument("Pipeline::mapScorePoses: " + map.lastError());
  if (rc != MADICP_OK) throw std::runtime_error("Pipeline::mapScorePoses: " + map.lastError());
}

size_t Pipeline::mapRelocalize(const double* xyz, size_t n, const double* poses, size_t n_poses, int reach, double max_dist, int64_t stride,
                               int refine, const AlignParams& params, int iterations, int32_t* out_index, uint64_t* out_scores,
                               double* out_poses, double* out_sums, uint64_t* out_counts, size_t* out_best) {
  if (map_spec_.voxel == 0.0) throw std::logic_error("Pipeline::mapRelocalize: setMapAccumulation(voxel_size > 0) first");
  if (map_spec_.mom == 0) throw std::logic_error("Pipeline::mapRelocalize: the map was made without moments (setMapAccumulation's moments)");
  if ((!xyz && n > 0) || !poses || !out_index || !out_scores || !out_poses || !out_sums || !out_counts || !out_best)
    throw std::invalid_argument("Pipeline::mapRelocalize: null argument");
  if (n > static_cast<size_t>(kMapMaxRows)) throw std::invalid_argument("Pipeline::mapRelocalize: at most 2^30 points");
  if (refine < 1 || refine > kRelocalizeMaxRefine) throw std::invalid_argument("Pipeline::mapRelocalize: refine must be 1 .. 64");
  const int64_t k64 = n_poses > static_cast<size_t>(kScoreMaxPoses) ? kScoreMaxPoses + 1 : static_cast<int64_t>(n_poses);
  if (const char* why = map_score_refusal(poses, k64, reach, max_dist, stride))
    throw std::invalid_argument(std::string("Pipeline::mapRelocalize: ") + why);
  if (const char* why = map_align_refusal(poses, poses + 9, params.reach, params.max_dist, params.rho, params.min_count, params.flat))
    throw std::invalid_argument(std::string("Pipeline::mapRelocalize: ") + why);
  if (iterations < 0 || iterations > kAlignMaxIterations) throw std::invalid_argument("Pipeline::mapRelocalize: iterations must be 0 .. 64");
  std::unique_ptr<MapStore> empty;  // before the first fold and for no point at all: an empty host map of the same kind answers
  if (!map_ || n == 0) {
    MapSpec kind = map_spec_;
    kind.first_rows = kind.max_rows = 1;
    empty = std::make_unique<HostMapStore>(kind);
  }
  MapStore& map = empty ? *empty : *map_;
  auto check_rc = [&](int rc) {
    if (rc == MADICP_ERR_INVALID) throw std::invalid_argument("Pipeline::mapRelocalize: " + map.lastError());
    if (rc != MADICP_OK) throw std::runtime_error("Pipeline::mapRelocalize: " + map.lastError());
  };
  const size_t K = static_cast<size_t>(k64), m = std::min<size_t>(static_cast<size_t>(refine), K);
  ScanBorrow scan(map, ScanRef::host(xyz, nullptr, static_cast<int64_t>(n)));  // ONE borrow: the scan goes up once
  std::vector<uint64_t> scores(3 * K);
  check_rc(map.score(scan.scan(), poses, k64, reach, max_dist, stride, scores.data()));
  std::vector<int32_t> order(K);
  for (size_t k = 0; k < K; ++k) order[k] = static_cast<int32_t>(k);
  // (within descending, index ascending): a strict total order, the ranking is a function of the integers alone
  std::partial_sort(order.begin(), order.begin() + m, order.end(), [&](int32_t a, int32_t b) {
    return scores[3 * a + 2] > scores[3 * b + 2] || (scores[3 * a + 2] == scores[3 * b + 2] && a < b);
  });
  std::vector<double> trace(kAlignTraceRow * (static_cast<size_t>(iterations) + 1));
  std::vector<uint64_t> counts(kAlignCounts * (static_cast<size_t>(iterations) + 1));
  size_t best = 0;
  for (size_t r = 0; r < m; ++r) {
    const size_t k = static_cast<size_t>(order[r]);
    const double* X = poses + kScorePoseDoubles * k;
    check_rc(map.align(scan.scan(), X, X + 9, params, iterations, out_poses + 12 * r, out_poses + 12 * r + 9, trace.data(), counts.data(),
                       nullptr, nullptr, 0));
    out_index[r] = order[r];
    std::copy(scores.begin() + 3 * k, scores.begin() + 3 * k + 3, out_scores + 3 * r);
    std::copy(trace.end() - kAlignTerms, trace.end(), out_sums + kAlignTerms * r);
    std::copy(counts.end() - kAlignCounts, counts.end(), out_counts + kAlignCounts * r);
    if (out_counts[kAlignCounts * r + 3] > out_counts[kAlignCounts * best + 3]) best = r;  // (a tie stays with the better rank)
  }
  *out_best = best;
  return m;
}

size_t Pipeline::mapMergeRows(const uint64_t* keys, const float* rows, const uint32_t* attribute, const uint32_t* evidence,
                              const uint64_t* moments, size_t n, size_t* out_added) {
  if (map_spec_.voxel == 0.0) throw std::logic_error("Pipeline::mapMergeRows: setMapAccumulation(voxel_size > 0) first");
  if (!out_added) throw std::invalid_argument("Pipeline::mapMergeRows: null argument");
  if (n > static_cast<size_t>(kMapMaxRows)) throw std::invalid_argument("Pipeline::mapMergeRows: at most 2^30 entries");
  // a fresh map goes where the front-end's scans will live; a device map's merge holds the device lock like a fold
  const bool device = map_ ? map_->onDevice() : device_frontend_;
  std::unique_lock<std::recursive_mutex> lock(Device::mutex(), std::defer_lock);
  if (device) lock.lock();
  std::unique_ptr<MapStore> fresh;  // (kept only if the merge succeeds: a refusal leaves everything as it was)
  if (!map_) {
    if (device)
      fresh = make_device_map_store(map_spec_);
    else
      fresh = std::make_unique<HostMapStore>(map_spec_, fetch_resident_scan);
    if (map_track_removed_ && fresh->trackRemoved(true) != MADICP_OK) throw std::runtime_error("Pipeline::mapMergeRows: " + fresh->lastError());
  }
  MapStore& map = fresh ? *fresh : *map_;
  if (device) MADtree::cancelDeviceBuild(0);  // the merge needs the builder's scratch: a look-ahead of another Pipeline gives way
  int64_t added = 0, size = 0;
  const int rc = map.merge(map_spec_.voxel, keys, rows, attribute, evidence, moments, static_cast<int64_t>(n), &added, &size);
  if (rc == MADICP_ERR_INVALID) throw std::invalid_argument("Pipeline::mapMergeRows: " + map.lastError());
  if (rc != MADICP_OK) throw std::runtime_error("Pipeline::mapMergeRows: " + map.lastError());
  if (fresh) map_ = std::move(fresh);
  *out_added = static_cast<size_t>(added);
  return static_cast<size_t>(size);
}

size_t Pipeline::mapNewRowCount() {
  if (map_spec_.voxel == 0.0) throw std::logic_error("Pipeline::mapNewRows: setMapAccumulation(voxel_size > 0) first");
  return mapSize() - map_cursor_;
}

size_t Pipeline::mapNewRows(float* out, size_t capacity, uint32_t* out_attr, uint64_t* out_keys) {
  const size_t m = mapNewRowCount();
  if (!out) throw std::invalid_argument("Pipeline::mapNewRows: null buffer");
  if (out_attr && !map_spec_.with_attr)
    throw std::logic_error("Pipeline::mapNewRows: the map was made without the attribute (setMapAccumulation's with_attribute)");
  if (capacity < m)
    throw std::invalid_argument("Pipeline::mapNewRows: the buffer holds " + std::to_string(capacity) + " rows, " + std::to_string(m) +
                                " are new");
  if (m == 0) return 0;
  size_t got = 0;
  if (out_keys || out_attr) {  // more than one column: through the one call — on the device, their copies in front of ONE wait
    MapColumns cols;
    cols.xyz = out;
    cols.keys = out_keys;
    cols.attr = out_attr;
    int64_t rows = 0;
    mapCheck(map_->download(static_cast<int64_t>(map_cursor_), cols, static_cast<int64_t>(capacity), &rows), "Pipeline::mapNewRows: ");
    got = static_cast<size_t>(rows);
  } else {
    got = mapCloud(out, capacity, map_cursor_);
  }
  map_cursor_ += got;
  return got;
}

// ---- the window downloads (pipeline.h: mapCloud .. mapSurfels) ------------------------------------------------------------------
bool Pipeline::mapWindow(const std::string& who, const char* missing, const void* out, const char* holds, size_t capacity, size_t first_row) {
  if (map_spec_.voxel == 0.0) throw std::logic_error(who + "setMapAccumulation(voxel_size > 0) first");
  if (missing) throw std::logic_error(who + missing);
  if (!out) throw std::invalid_argument(who + "null buffer");
  const size_t size = mapSize();
  if (first_row > size) throw std::invalid_argument(who + "first_row is beyond the map's " + std::to_string(size) + " rows");
  if (capacity < size - first_row)
    throw std::invalid_argument(who + holds + " " + std::to_string(capacity) + " rows, the window needs " + std::to_string(size - first_row));
  return size > first_row;
}
template <class T>
size_t Pipeline::mapColumn(const char* name, const char* missing, T* MapColumns::*column, T* out, size_t capacity, size_t first_row) {
  const std::string who = std::string("Pipeline::") + name + ": ";
  if (!mapWindow(who, missing, out, "the buffer holds", capacity, first_row)) return 0;
  MapColumns cols;
  cols.*column = out;
  int64_t rows = 0;
  mapCheck(map_->download(static_cast<int64_t>(first_row), cols, static_cast<int64_t>(capacity), &rows), who);
  return static_cast<size_t>(rows);
}
namespace {
constexpr const char* kNoMapAttr = "the map was made without the attribute (setMapAccumulation's with_attribute)";
constexpr const char* kNoMapEvidence = "the map was made without evidence (setMapAccumulation's evidence)";
constexpr const char* kNoMapMoments = "the map was made without moments (setMapAccumulation's moments_max_count)";
}  // namespace

size_t Pipeline::mapKeys(uint64_t* out, size_t capacity, size_t first_row) {
  return mapColumn("mapKeys", nullptr, &MapColumns::keys, out, capacity, first_row);
}
size_t Pipeline::mapCloud(float* out, size_t capacity, size_t first_row) {
  return mapColumn("mapCloud", nullptr, &MapColumns::xyz, out, capacity, first_row);
}
size_t Pipeline::mapAttribute(uint32_t* out, size_t capacity, size_t first_row) {
  return mapColumn("mapAttribute", map_spec_.with_attr ? nullptr : kNoMapAttr, &MapColumns::attr, out, capacity, first_row);
}
size_t Pipeline::mapEvidence(uint32_t* out, size_t capacity, size_t first_row) {
  return mapColumn("mapEvidence", map_spec_.with_ev ? nullptr : kNoMapEvidence, &MapColumns::ev, out, capacity, first_row);
}
size_t Pipeline::mapMoments(uint64_t* out, size_t capacity, size_t first_row) {
  return mapColumn("mapMoments", map_spec_.mom ? nullptr : kNoMapMoments, &MapColumns::moments, out, capacity, first_row);
}
size_t Pipeline::mapSurfels(float* centroid, float* normal, float* eig, uint32_t* count, size_t capacity, size_t first_row) {
  const std::string who = "Pipeline::mapSurfels: ";
  if (!mapWindow(who, map_spec_.mom ? nullptr : kNoMapMoments, centroid, "the buffers hold", capacity, first_row)) return 0;
  int64_t rows = 0;
  mapCheck(map_->downloadSurfels(static_cast<int64_t>(first_row), centroid, normal, eig, count, static_cast<int64_t>(capacity), &rows), who);
  return static_cast<size_t>(rows);
}

// ---- the removal log (pipeline.h: setMapTrackRemoved) -------------------------------------------------------------------------
void Pipeline::setMapTrackRemoved(bool on) {
  if (map_spec_.voxel == 0.0) throw std::logic_error("Pipeline::setMapTrackRemoved: setMapAccumulation(voxel_size > 0) first");
  if (on == map_track_removed_) return;
  if (map_) mapCheck(map_->trackRemoved(on), "Pipeline::setMapTrackRemoved: ");
  map_track_removed_ = on;
  if (!on) map_log_full_ = false;
}

size_t Pipeline::mapRemovedRowCount() {
  if (map_spec_.voxel == 0.0) throw std::logic_error("Pipeline::mapRemovedRows: setMapAccumulation(voxel_size > 0) first");
  int64_t n = 0;  // (no frame folded yet: none)
  if (map_) mapCheck(map_->removedCount(&n), "Pipeline::mapRemovedRows: ");
  return static_cast<size_t>(n);
}

size_t Pipeline::mapRemovedRows(uint64_t* keys, float* rows, uint32_t* attr, size_t capacity) {
  const size_t m = mapRemovedRowCount();
  if (!map_track_removed_) throw std::logic_error("Pipeline::mapRemovedRows: setMapTrackRemoved(true) first");
  if (!keys || !rows) throw std::invalid_argument("Pipeline::mapRemovedRows: null buffer");
  if (attr && !map_spec_.with_attr)
    throw std::logic_error("Pipeline::mapRemovedRows: the map was made without the attribute (setMapAccumulation's with_attribute)");
  if (capacity < m)
    throw std::invalid_argument("Pipeline::mapRemovedRows: the buffers hold " + std::to_string(capacity) + " rows, the log has " +
                                std::to_string(m));
  map_log_full_ = false;
  if (m == 0) return 0;
  int64_t n = 0;
  mapCheck(map_->takeRemoved(keys, rows, attr, static_cast<int64_t>(capacity), &n), "Pipeline::mapRemovedRows: ");
  return static_cast<size_t>(n);
}

size_t Pipeline::mapSize() {
  if (map_spec_.voxel == 0.0) throw std::logic_error("Pipeline::mapSize: setMapAccumulation(voxel_size > 0) first");
  int64_t rows = 0;  // (no frame folded yet: none)
  if (map_) mapCheck(map_->size(&rows), "Pipeline::mapSize: ");
  return static_cast<size_t>(rows);
}

size_t Pipeline::mapConfirmed(uint32_t min_evidence, float* out_xyz, uint64_t* out_keys, uint32_t* out_attr, uint32_t* out_ev, size_t capacity) {
  if (map_spec_.voxel == 0.0) throw std::logic_error("Pipeline::mapConfirmed: setMapAccumulation(voxel_size > 0) first");
  if (!map_spec_.with_ev) throw std::logic_error("Pipeline::mapConfirmed: the map was made without evidence (setMapAccumulation's evidence)");
  if (out_attr && !map_spec_.with_attr)
    throw std::logic_error("Pipeline::mapConfirmed: the map was made without the attribute (setMapAccumulation's with_attribute)");
  if (!out_xyz) throw std::invalid_argument("Pipeline::mapConfirmed: null buffer");
  int64_t rows = 0;
  int rc = MADICP_OK;  // (no frame folded yet: none qualifies)
  if (map_) rc = map_->downloadMinEvidence(min_evidence, out_xyz, out_keys, out_attr, out_ev, static_cast<int64_t>(capacity), &rows);
  if (rc == MADICP_ERR_CAPACITY)
    throw std::invalid_argument("Pipeline::mapConfirmed: the buffers hold " + std::to_string(capacity) + " rows, " + std::to_string(rows) +
                                " qualify");
  mapCheck(rc, "Pipeline::mapConfirmed: ");
  return static_cast<size_t>(rows);
}

void Pipeline::clearMap() {
  if (map_spec_.voxel == 0.0) throw std::logic_error("Pipeline::clearMap: setMapAccumulation(voxel_size > 0) first");
  map_overflowed_ = false;
  map_have_center_ = false;
  map_cursor_ = map_removed_ = 0;
  map_log_full_ = false;
  if (map_) mapCheck(map_->clear(), "Pipeline::clearMap: ");
}

size_t Pipeline::registeredScan(float* out, size_t capacity, double voxel, bool map_frame) {
  if (!keep_scan_) throw std::logic_error("Pipeline::registeredScan: setKeepScan(true) first");
  if (!have_kept_) throw std::logic_error("Pipeline::registeredScan: no frame has been computed since setKeepScan(true)");
  if (!out) throw std::invalid_argument("Pipeline::registeredScan: null buffer");
  if (!std::isfinite(voxel) || voxel < 0.0) throw std::invalid_argument("Pipeline::registeredScan: voxel must be finite and >= 0");
  const Pose X = map_frame ? frame_to_map_ : Pose::identity();
  const int64_t cap = static_cast<int64_t>(std::min<size_t>(capacity, size_t(1) << 40));
  int64_t rows = 0;
  int rc;
  if (kept_cloud_id_ >= 0) {
    DeviceLock lock(Device::mutex());
    madicp_ctx* ctx = Device::current(kept_generation_);
    if (!ctx) throw std::logic_error("Pipeline::registeredScan: the device context the scan lived in is gone");
    MADtree::cancelDeviceBuild(0);  // the export needs the builder's scratch: a look-ahead of another Pipeline gives way
    rc = madicp_cloud_export_f32(ctx, kept_cloud_id_, X.R, X.t, voxel, out, cap, &rows);
    if (rc != MADICP_OK && rc != MADICP_ERR_CAPACITY) check(rc, "madicp_cloud_export_f32");
  } else {
    rc = cloud_export_f32(kept_host_.empty() ? nullptr : kept_host_[0].data(), static_cast<int64_t>(kept_host_.size()), X.R, X.t, voxel,
                          out, cap, &rows);
    if (rc != MADICP_OK && rc != MADICP_ERR_CAPACITY)
      throw std::runtime_error("Pipeline::registeredScan: the host export refused its arguments");
  }
  if (rc == MADICP_ERR_CAPACITY)
    throw std::invalid_argument("Pipeline::registeredScan: the buffer holds " + std::to_string(capacity) + " rows, the scan needs " +
                                std::to_string(rows));
  return static_cast<size_t>(rows);
}

size_t Pipeline::registeredScanAttribute(uint32_t* out, size_t capacity, double voxel, bool map_frame) {
  // (the rows themselves into a buffer of its own: no more of them than the scan has points)
  std::vector<float> xyz(3 * std::max<size_t>(std::min(capacity, registeredScanSize()), 1));
  return registeredScanWithAttribute(xyz.data(), out, std::min(capacity, xyz.size() / 3), voxel, map_frame);
}

size_t Pipeline::registeredScanWithAttribute(float* out_xyz, uint32_t* out, size_t capacity, double voxel, bool map_frame) {
  if (!keep_scan_) throw std::logic_error("Pipeline::registeredScanAttribute: setKeepScan(true) first");
  if (!have_kept_) throw std::logic_error("Pipeline::registeredScanAttribute: no frame has been computed since setKeepScan(true)");
  if (!kept_has_attr_) throw std::logic_error("Pipeline::registeredScanAttribute: the retained scan carries no attribute");
  if (!out || !out_xyz) throw std::invalid_argument("Pipeline::registeredScanAttribute: null buffer");
  if (!std::isfinite(voxel) || voxel < 0.0) throw std::invalid_argument("Pipeline::registeredScanAttribute: voxel must be finite and >= 0");
  const Pose X = map_frame ? frame_to_map_ : Pose::identity();
  const int64_t cap_rows = static_cast<int64_t>(std::min<size_t>(capacity, size_t(1) << 40));
  int64_t rows = 0;
  int rc;
  if (kept_cloud_id_ >= 0) {
    DeviceLock lock(Device::mutex());
    madicp_ctx* ctx = Device::current(kept_generation_);
    if (!ctx) throw std::logic_error("Pipeline::registeredScanAttribute: the device context the scan lived in is gone");
    MADtree::cancelDeviceBuild(0);  // the export needs the builder's scratch: a look-ahead of another Pipeline gives way
    rc = madicp_cloud_export_f32_attr(ctx, kept_cloud_id_, X.R, X.t, voxel, out_xyz, out, cap_rows, &rows);
    if (rc != MADICP_OK && rc != MADICP_ERR_CAPACITY) check(rc, "madicp_cloud_export_f32_attr");
  } else {
    rc = cloud_export_f32_attr(kept_host_.empty() ? nullptr : kept_host_[0].data(), kept_attr_.data(), static_cast<int64_t>(kept_host_.size()),
                               X.R, X.t, voxel, out_xyz, out, cap_rows, &rows);
    if (rc != MADICP_OK && rc != MADICP_ERR_CAPACITY)
      throw std::runtime_error("Pipeline::registeredScanAttribute: the host export refused its arguments");
  }
  if (rc == MADICP_ERR_CAPACITY)
    throw std::invalid_argument("Pipeline::registeredScanAttribute: the buffer holds " + std::to_string(capacity) + " rows, the scan needs " +
                                std::to_string(rows));
  return static_cast<size_t>(rows);
}

const std::vector<Matrix4d> Pipeline::trajectory() const {
  std::vector<Matrix4d> out;
  out.reserve(trajectory_.size());
  for (const Pose& p : trajectory_) out.push_back(toMatrix(p));
  return out;
}

// pipeline.cpp:82-86
void Pipeline::naiveVelocity(const Pose& T_prev, const Pose& T_now, double* vel) const {
  naive_velocity(T_prev, T_now, sensor_hz_, vel);
}

// pipeline.cpp:79-123 — motion compensation in 1024 azimuth chunks, host version (deskew.h; the device front-end runs
// madicp_cloud_deskew instead).  `prep`: the pose-independent half, when prefetch() computed it ahead.
void Pipeline::deskew(ContainerType& cloud, const Pose& T_prev, const Pose& T_now, const DeskewOrder* prep) {
  deskew_cloud(cloud, T_prev, T_now, sensor_hz_, prep, nullptr);
}

// pipeline.cpp:267-284
void Pipeline::initialize(const double& curr_stamp, ContainerType& cloud) {
  auto frame = std::make_unique<Frame>();
  frame->frame_ = int(seq_);
  frame->frame_to_map_ = frame_to_map_;
  frame->stamp_ = curr_stamp;
  frame->tree_ = std::make_unique<MADtree>(std::move(cloud), b_max_, b_min_, max_parallel_levels_);
  current_num_leaves_ = size_t(frame->tree_->numLeaves());
  current_tree_view_ = frame->tree_.get();
  if (ledger_.world() == 1 || madicp::keyframe_owner(0, ledger_.world()) == ledger_.rank())
    frame->tree_->deviceId();  // first keyframe: resident from now on (sharded: on its owner)
  pushKeyframe(std::move(frame));
  trajectory_.push_back(Pose::identity());
  is_initialized_ = true;
  is_map_updated_ = true;
  seq_++;
}

// The scan as a VIEW (the bindings' entry point: pybind hands a by-value ContainerType over as a fresh 3 MB allocation + copy
// per call, and fresh pages cost ~1 us each — 0.35 ms per cloud, twice per look-ahead frame, which is what the "look-ahead
// cliff" of rounds 3-5 was: profiles/r5_u_lookahead_canary.md).  The memory is only read during the call.
void Pipeline::prefetchView(const Vector3d* next_cloud, size_t n) {
  if (!next_cloud || n == 0) return;
  if (device_frontend_) {
    // the tree is built on the GPU — a host build would only compete for the CPU — and the look-ahead is the library's:
    // collect the construction in flight (the scan about to be consumed), start this one beside the coming registration
    if (deskew_) return;  // (the tree needs the previous pose)
    if (keep_scan_ || map_spec_.voxel > 0.0) return;  // (a look-ahead build gives back the tree alone, not the scan: pipeline.h, setKeepScan)
    // begun by the next compute(), behind its registration's submission; assign() into a buffer that lives as long as the
    // Pipeline: after the first frames no allocation, no fresh pages
    dev_next_cloud_.assign(next_cloud, next_cloud + n);
    dev_next_staged_ = true;
    if (!is_initialized_ || (!dev_pending_ && !dev_ready_)) beginStagedLookAhead();  // (nothing to hide behind yet)
    return;
  }
  prefetch(ContainerType(next_cloud, next_cloud + n));
}

void Pipeline::prefetch(ContainerType next_cloud) {
  if (next_cloud.empty()) return;
  if (device_frontend_) {
    prefetchView(next_cloud.data(), next_cloud.size());
    return;
  }
  // with deskew the tree is built from the motion-compensated cloud, which needs the pose of the frame before it — but the
  // azimuth of every point and their order do not (deskew.h): that half is started now
  if (deskew_ && is_initialized_) {
    while (deskew_ahead_.size() >= kMaxLookAhead) {
      if (deskew_ahead_.front().result.valid()) deskew_ahead_.front().result.wait();
      deskew_ahead_.pop_front();
    }
    DeskewAhead a;
    a.key = DevKey::of(next_cloud);
    a.result = std::async(std::launch::async, [cloud = std::move(next_cloud)]() { return deskew_order(cloud); });
    deskew_ahead_.push_back(std::move(a));
    return;
  }
  while (prefetched_.size() >= kMaxLookAhead) {  // the oldest one makes room (its build is waited for)
    if (prefetched_.front().result.valid()) prefetched_.front().result.wait();
    prefetched_.pop_front();
  }
  Prefetched p;
  p.key = DevKey::of(next_cloud);
  const double b_max = b_max_, b_min = b_min_;
  const int levels = max_parallel_levels_;
  p.result = std::async(std::launch::async, [cloud = std::move(next_cloud), b_max, b_min, levels]() mutable {
    return build_tree(cloud.front().data(), static_cast<int64_t>(cloud.size()), b_max, b_min, levels);
  });
  prefetched_.push_back(std::move(p));
}

// the device front-end for one frame: the cloud is resident; deskew when the reference would (pipeline.cpp:138-139),
// build, hand the cloud's buffer back
std::unique_ptr<MADtree> Pipeline::buildOnDevice(int cloud_id, const double* stamps, size_t n_stamps, bool own_stamps) {
  DeviceLock lock(Device::mutex());
  madicp_ctx* ctx = Device::ctx();
  MADtree::cancelDeviceBuild(0);  // deskew and build need the builder's scratch: a look-ahead of another Pipeline gives way
  dropKeptScan();                 // (the scan retained for the frame before)
  const int attr_type = frame_attr_type_;  // (the column the frame announced lives in the cloud: both deskews keep it aligned)
  frame_attr_type_ = kAttrNone;
  std::unique_ptr<MADtree> tree;
  try {
    if (is_initialized_ && deskew_ && trajectory_.size() > 1) {
      double vel[6];
      naiveVelocity(trajectory_[trajectory_.size() - 2], trajectory_[trajectory_.size() - 1], vel);
      if (own_stamps)
        check(madicp_cloud_deskew_own_stamps(ctx, cloud_id, vel, sensor_hz_, nullptr), "madicp_cloud_deskew_own_stamps");
      else if (stamps)
        check(madicp_cloud_deskew_stamped(ctx, cloud_id, stamps, static_cast<int64_t>(n_stamps), vel, sensor_hz_, nullptr),
              "madicp_cloud_deskew_stamped");
      else
        check(madicp_cloud_deskew(ctx, cloud_id, vel, sensor_hz_, nullptr), "madicp_cloud_deskew");
    }
    tree = std::make_unique<MADtree>(MADtree::DeviceCloud{cloud_id}, b_max_, b_min_);
  } catch (...) {
    madicp_cloud_release(ctx, cloud_id);
    throw;
  }
  // retained instead (map accumulation alone: until the frame's fold): the buffer goes back to the pool when the next frame,
  // setKeepScan(false) or the end drops it
  if (keep_scan_ || map_spec_.voxel > 0.0) {
    int64_t n = 0;
    check(madicp_cloud_size(ctx, cloud_id, &n), "madicp_cloud_size");
    kept_cloud_id_ = cloud_id;
    kept_generation_ = Device::generation();
    kept_n_ = static_cast<size_t>(n);
    have_kept_ = true;
    kept_has_attr_ = attr_type != kAttrNone;
    kept_attr_type_ = attr_type;
    return tree;
  }
  check(madicp_cloud_release(ctx, cloud_id), "madicp_cloud_release");
  return tree;
}

std::unique_ptr<MADtree> Pipeline::uploadAndBuild(const Vector3d* cloud, size_t n, const double* stamps) {
  int cloud_id = -1;
  {
    DeviceLock lock(Device::mutex());
    check(madicp_cloud_upload(Device::ctx(), cloud[0].data(), static_cast<int64_t>(n), &cloud_id), "madicp_cloud_upload");
  }
  return buildOnDevice(cloud_id, stamps, stamps ? n : 0);
}

void Pipeline::ingestPrologue() {
  waitPrefetched();
  dropDeviceLookAhead();          // (ingest shares the builder's scratch ...
  MADtree::cancelDeviceBuild(0);  //  ... with every Pipeline of the process)
}

// The device half of a frame whose scan is ingested on the device: the builder's scratch is claimed, `ingest` — run under the
// device lock — returns the cloud's id, then deskew (`own_stamps`: by the stamps the cloud carries), build and registration.
template <class Ingest>
void Pipeline::computeIngested(const double& curr_stamp, bool own_stamps, Ingest&& ingest) {
  is_map_updated_ = false;
  const double t_pre = now_ms();
  ingestPrologue();
  int cloud_id = -1;
  {
    DeviceLock lock(Device::mutex());
    cloud_id = ingest();
  }
  computeWithTree(curr_stamp, buildOnDevice(cloud_id, nullptr, 0, own_stamps), nullptr, t_pre);
}

void Pipeline::computeRecords(const double& curr_stamp, const float* records, size_t n_records, int stride_floats,
                              double min_range, double max_range, bool kitti_correction) {
  is_map_updated_ = false;
  if (!records || n_records == 0) throw std::invalid_argument("Pipeline::computeRecords: no records");
  computeIngested(curr_stamp, false, [&] {
    int cloud_id = -1;
    int64_t kept = 0;
    check(madicp_cloud_ingest_f32(Device::ctx(), records, static_cast<int64_t>(n_records), stride_floats, min_range, max_range,
                                  kitti_correction ? 1 : 0, &cloud_id, &kept),
          "madicp_cloud_ingest_f32");
    return cloud_id;
  });
}

// A frame from a driver's byte records (pipeline.h): its own refusals, then the frame of the one plain source.
void Pipeline::computeRecordsStamped(const double& curr_stamp, const void* data, size_t n_records, const RecordLayout& layout,
                                     double min_range, double max_range, bool kitti_correction, const double* t_range) {
  if (!data || n_records == 0) throw std::invalid_argument("Pipeline::computeRecordsStamped: no records");
  if (!record_layout_ok(layout)) throw std::invalid_argument("Pipeline::computeRecordsStamped: bad record layout");
  if (n_records > 0x3fffffff) throw std::invalid_argument("Pipeline::computeRecordsStamped: 1 .. 2^30 records");
  if (t_range && !(std::isfinite(t_range[0]) && std::isfinite(t_range[1]) && t_range[1] > t_range[0]))
    throw std::invalid_argument("Pipeline::computeRecordsStamped: t_range needs two finite values, t_end > t_begin");
  const RecordSource S = plain_source(data, static_cast<int64_t>(n_records), layout, min_range, max_range, kitti_correction);
  computeSources(curr_stamp, &S, 1, t_range, "Pipeline::computeRecordsStamped");
}

void Pipeline::computeRecordsStamped(const double& curr_stamp, const void* data, size_t n_records, const RecordLayout& layout,
                                     double min_range, double max_range, bool kitti_correction, const double* t_range,
                                     const AttrField& attribute) {
  if (!data || n_records == 0) throw std::invalid_argument("Pipeline::computeRecordsStamped: no records");
  if (n_records > 0x3fffffff) throw std::invalid_argument("Pipeline::computeRecordsStamped: 1 .. 2^30 records");
  RecordSource S = plain_source(data, static_cast<int64_t>(n_records), layout, min_range, max_range, kitti_correction);
  S.A = attribute;
  if (const char* why = record_sources_refusal(&S, 1, t_range)) throw std::invalid_argument(std::string("Pipeline::computeRecordsStamped: ") + why);
  computeSources(curr_stamp, &S, 1, t_range, "Pipeline::computeRecordsStamped");
}

// A frame from several sensors' byte records (pipeline.h)
void Pipeline::computeSourcesStamped(const double& curr_stamp, const RecordSource* sources, int n_sources, const double* t_range) {
  if (const char* why = record_sources_refusal(sources, n_sources, t_range))
    throw std::invalid_argument(std::string("Pipeline::computeSourcesStamped: ") + why);
  computeSources(curr_stamp, sources, n_sources, t_range, "Pipeline::computeSourcesStamped");
}

// ... for sources that passed record_sources_refusal (`who`: the entry, for what is still refused).  The time fields matter only
// where stamps can: deskew = true and layouts that have one — everywhere else the layouts are taken without it, so nothing is
// normalised, stored or read.
void Pipeline::computeSources(const double& curr_stamp, const RecordSource* sources, int n_sources, const double* t_range,
                              const char* who) {
  RecordSource src[kMaxSources];
  int64_t total = 0;
  for (int s = 0; s < n_sources; ++s) {
    src[s] = sources[s];
    if (!deskew_) src[s].L.t_type = kTimeNone;
    total += src[s].n;
  }
  if (!deskew_) t_range = nullptr;
  const bool stamped = deskew_ && sources[0].L.t_type != kTimeNone;
  // The attribute column (sources that name a field: all of them or none): announced to whoever retains the frame's scan
  // (buildOnDevice / keepHostScan take it over) and forgotten again however the frame ends.
  const int attr_type = sources[0].A.type;
  struct FrameAttr {
    Pipeline* p;
    ~FrameAttr() {
      p->frame_attr_type_ = kAttrNone;
      p->frame_attr_.clear();
    }
  } frame_attr{this};
  if (device_frontend_) {
    madicp_record_source cs[MADICP_MAX_SOURCES];
    madicp_attr_field fields[MADICP_MAX_SOURCES];
    for (int s = 0; s < n_sources; ++s) {
      cs[s] = record_source_to<madicp_record_source>(src[s]);
      fields[s] = madicp_attr_field{src[s].A.off, src[s].A.type};
    }
    frame_attr_type_ = attr_type;
    computeIngested(curr_stamp, stamped, [&] {
      int cloud_id = -1;
      int64_t kept = 0;
      check(madicp_cloud_ingest_sources_attr(Device::ctx(), cs, n_sources, attr_type != kAttrNone ? fields : nullptr, t_range, &cloud_id,
                                             &kept, nullptr, nullptr),
            "madicp_cloud_ingest_sources");
      return cloud_id;
    });
    return;
  }
  ContainerType cloud(static_cast<size_t>(total));
  std::vector<double> stamps(stamped ? static_cast<size_t>(total) : 0);
  std::vector<uint32_t> words(attr_type != kAttrNone ? static_cast<size_t>(total) : 0);
  int64_t kept = 0;
  if (ingest_sources_attr(src, n_sources, t_range, cloud[0].data(), stamped ? stamps.data() : nullptr,
                          attr_type != kAttrNone ? words.data() : nullptr, &kept, nullptr, nullptr) != 0)
    throw std::invalid_argument(std::string(who) + ": bad arguments");
  if (kept < 1) throw std::invalid_argument(std::string(who) + ": no point survives the range filter");
  cloud.resize(static_cast<size_t>(kept));
  if (attr_type != kAttrNone) {
    words.resize(static_cast<size_t>(kept));
    frame_attr_ = std::move(words);
    frame_attr_type_ = attr_type;
  }
  if (stamped) {
    stamps.resize(static_cast<size_t>(kept));
    computeStamped(curr_stamp, std::move(cloud), stamps);
  } else {
    compute(curr_stamp, std::move(cloud));
  }
}

// pipeline.cpp:125-265, the device front-end's half: the scan is only READ (key of a look-ahead, or the upload), so a view does
void Pipeline::computeView(const double& curr_stamp, const Vector3d* curr_cloud, size_t n) {
  if (!curr_cloud || n == 0) throw std::invalid_argument("Pipeline::compute: empty cloud");
  if (!device_frontend_) {  // the host builder takes the points over: it needs its own copy
    compute(curr_stamp, ContainerType(curr_cloud, curr_cloud + n));
    return;
  }
  is_map_updated_ = false;
  // a tree built ahead for exactly this scan?
  std::unique_ptr<MADtree> current_tree;
  const double t_pre = now_ms();
  waitPrefetched();
  if (dev_ready_ && dev_ready_key_.matches(curr_cloud, n)) {
    current_tree = std::move(dev_ready_);  // collected when the next look-ahead was begun
  } else if (dev_pending_ && dev_pending_key_.matches(curr_cloud, n)) {
    collectDeviceLookAhead();
    current_tree = std::move(dev_ready_);
  }
  if (current_tree) ++look_ahead_hits_;
  if (!current_tree) {
    // Nothing looked ahead for THIS scan.  A construction in flight is then most likely for the NEXT one (a caller whose
    // first scan came without a prefetch stays one ahead from there on): it is collected and kept — the synchronous build
    // below needs the builder's scratch, so it has to be finished either way — not thrown away.
    collectDeviceLookAhead();
    current_tree = uploadAndBuild(curr_cloud, n);
  }
  computeWithTree(curr_stamp, std::move(current_tree), nullptr, t_pre);
}

// A scan with per-point acquisition times (pipeline.h).  The stamps matter under exactly the condition the reference deskews;
// everywhere else this is compute().
void Pipeline::computeStampedView(const double& curr_stamp, const Vector3d* curr_cloud, const double* stamps, size_t n) {
  if (!curr_cloud || !stamps || n == 0) throw std::invalid_argument("Pipeline::computeStamped: empty cloud or no timestamps");
  if (!(deskew_ && trajectory_.size() > 1)) {
    computeView(curr_stamp, curr_cloud, n);
    return;
  }
  is_map_updated_ = false;
  const double t_pre = now_ms();
  waitPrefetched();
  std::unique_ptr<MADtree> current_tree;
  if (device_frontend_) {
    collectDeviceLookAhead();  // (the synchronous build needs the builder's scratch: as in computeView)
    current_tree = uploadAndBuild(curr_cloud, n, stamps);
  } else {
    // the azimuth order prefetch() computed ahead for this scan (and older ones: scans that never came) is not needed
    DeskewAhead unused;
    if (takeLookAhead(deskew_ahead_, curr_cloud, n, &unused) && unused.result.valid()) unused.result.wait();
    ContainerType cloud(curr_cloud, curr_cloud + n);  // (the host builder takes the points over)
    deskew_cloud_stamped(cloud, stamps, trajectory_[trajectory_.size() - 2], trajectory_[trajectory_.size() - 1], sensor_hz_, nullptr);
    keepHostScan(cloud);
    current_tree = std::make_unique<MADtree>(std::move(cloud), b_max_, b_min_, max_parallel_levels_);
  }
  computeWithTree(curr_stamp, std::move(current_tree), nullptr, t_pre);
}

void Pipeline::computeStamped(const double& curr_stamp, ContainerType curr_cloud, const std::vector<double>& stamps) {
  if (curr_cloud.empty()) throw std::invalid_argument("Pipeline::computeStamped: empty cloud");
  if (stamps.size() != curr_cloud.size()) throw std::invalid_argument("Pipeline::computeStamped: one timestamp per point");
  if (!(deskew_ && trajectory_.size() > 1)) {
    compute(curr_stamp, std::move(curr_cloud));
    return;
  }
  computeStampedView(curr_stamp, curr_cloud.data(), stamps.data(), curr_cloud.size());
}

// pipeline.cpp:125-265
void Pipeline::compute(const double& curr_stamp, ContainerType curr_cloud) {
  if (curr_cloud.empty()) throw std::invalid_argument("Pipeline::compute: empty cloud");
  if (device_frontend_) {
    computeView(curr_stamp, curr_cloud.data(), curr_cloud.size());
    return;
  }
  is_map_updated_ = false;
  // a tree built ahead for exactly this scan?
  std::unique_ptr<MADtree> current_tree;
  const double t_pre = now_ms();
  if (!prefetched_.empty() && !(deskew_ && is_initialized_ && trajectory_.size() > 1)) {
    // the look-ahead built for exactly this scan, if there is one; older look-aheads are for scans that never came
    Prefetched p;
    if (takeLookAhead(prefetched_, curr_cloud.data(), curr_cloud.size(), &p)) {
      current_tree = std::make_unique<MADtree>(p.result.get());  // (waits for the builder thread)
      ++look_ahead_hits_;
    }
  }
  computeWithTree(curr_stamp, std::move(current_tree), &curr_cloud, t_pre);
}

// the frame step once the scan's tree exists (or, host path, is still to be built from *cloud)
void Pipeline::computeWithTree(const double& curr_stamp, std::unique_ptr<MADtree> current_tree, ContainerType* cloud,
                               double t_pre) {
  current_leaves_host_ = nullptr;
  // host front-end, the scan as given (first frame, no deskew due, or a tree built ahead for it): retained before the builder
  // takes the points over; the deskewed one is retained below
  const bool deskew_due = is_initialized_ && !current_tree && deskew_ && trajectory_.size() > 1;
  if (cloud && !deskew_due) keepHostScan(*cloud);
  if (!is_initialized_) {
    if (current_tree) {
      auto frame = std::make_unique<Frame>();
      frame->frame_ = int(seq_);
      frame->frame_to_map_ = frame_to_map_;
      frame->stamp_ = curr_stamp;
      frame->tree_ = std::move(current_tree);
      frame->tree_->deviceId();
      current_num_leaves_ = size_t(frame->tree_->numLeaves());
      current_tree_view_ = frame->tree_.get();
      pushKeyframe(std::move(frame));
      trajectory_.push_back(Pose::identity());
      is_initialized_ = true;
      is_map_updated_ = true;
      seq_++;
    } else {
      initialize(curr_stamp, *cloud);
    }
    foldFrame();
    return;
  }

  if (!current_tree) {
    if (deskew_ && trajectory_.size() > 1) {
      // the azimuth order computed ahead for exactly this scan, if there is one (older ones: scans that never came)
      DeskewOrder ahead;
      DeskewAhead a;
      bool have = takeLookAhead(deskew_ahead_, cloud->data(), cloud->size(), &a);
      if (have) {
        ahead = a.result.get();
        ++look_ahead_hits_;
      }
      if (frame_attr_type_ != kAttrNone) {  // the frame's attribute column follows the points into azimuth order
        if (!have) {
          ahead = deskew_order(*cloud);
          have = true;
        }
        permuteFrameAttr(ahead);
      }
      deskew(*cloud, trajectory_[trajectory_.size() - 2], trajectory_[trajectory_.size() - 1], have ? &ahead : nullptr);
      keepHostScan(*cloud);
    }
    current_tree = std::make_unique<MADtree>(std::move(*cloud), b_max_, b_min_, max_parallel_levels_);
  }
  // resident from now on (frame window, maybe keyframe later); the copy runs on the library's copy stream while the
  // host goes on, and the moving leaves are read from it on the device (pipeline.cpp:143-144,154)
  current_tree->deviceId();
  current_num_leaves_ = size_t(current_tree->numLeaves());
  last_build_ms_ = now_ms() - t_pre;

  // constant-velocity prediction (pipeline.cpp:146-152)
  double dx[6];
  for (int i = 0; i < 6; ++i) dx[i] = current_velocity_[i] * 1. / sensor_hz_;
  const Pose prediction = compose(frame_to_map_, motion_from_twist(dx));

  icp_.setMoving(*current_tree);
  icp_.init(prediction);

  const float preprocessing_time = virtual_pre_ms_ >= 0 ? float(virtual_pre_ms_) : float(now_ms() - t_pre);
  if (virtual_pre_ms_ >= 0) round_ms_estimate_ = virtual_round_ms_;
  const double t_icp = now_ms();
  // The reference re-checks its wall-clock budget before every round: round k runs iff preprocessing + the k rounds run
  // so far + ONE MORE round's time (its `icp_time` term: the duration of the round before, counted a second time) still
  // fit loop_time - 5 ms (pipeline.cpp:167-169).  The device loop is one submission, so the same test is turned into a
  // round count BEFORE it starts, at the per-round time the previous frame measured: with budget B and round time t,
  // rounds = 0 if B < 0, else max(1, floor(B / t)) (round 0 is tested with icp_time = 0), capped at MAX_ICP_ITS — all of
  // them unless the budget is nearly spent: a round is ~0.02 ms here.
  int rounds = MAX_ICP_ITS;
  if (realtime_) {
    const double remaining = double(loop_time_) - 5.0 - double(preprocessing_time);
    rounds = remaining < 0 ? 0
                           : int(std::min<double>(MAX_ICP_ITS, std::max(1.0, std::floor(remaining / std::max(round_ms_estimate_, 1e-3)))));
  }
  int matched_leaves = 0;
  if (rounds > 0) {
    std::vector<MADtree*> fixed;
    fixed.reserve(keyframes_.size());
    for (auto& f : keyframes_)
      if (f->tree_) fixed.push_back(f->tree_.get());  // (sharded: this rank's keyframes — none at all is legal there)
    if (ledger_.world() > 1) checkShardCommunicator();
    // (cut short: the matched flags are the OR over the rounds that ran — the reference resets them in iteration
    // MAX_ICP_ITS - 1 only — and the launch goes kernel by kernel, no graph is instantiated for an odd round count)
    const bool looking_ahead = device_frontend_ && (dev_pending_ || dev_next_staged_);
    icp_.compute(fixed, rounds, rounds < MAX_ICP_ITS, [this]() {
      if (device_frontend_) beginStagedLookAhead();
    }, looking_ahead);
    matched_leaves = icp_.numMatched();
  }
  last_icp_ms_ = now_ms() - t_icp;
  last_rounds_ = rounds;
  if (rounds > 0) round_ms_estimate_ = last_icp_ms_ / rounds;

  frame_to_map_ = icp_.X_;
  const double inliers_ratio = double(matched_leaves) / double(current_num_leaves_);
  last_inliers_ratio_ = inliers_ratio;
  trajectory_.push_back(frame_to_map_);

  std::vector<Pose> odom_window;
  for (int i = std::max(0, int(trajectory_.size()) - SMOOTHING_T); i < int(trajectory_.size()); ++i)
    odom_window.push_back(trajectory_[i]);
  vel_estimator_.init(current_velocity_);
  vel_estimator_.setOdometry(odom_window);
  vel_estimator_.oneRound();
  std::memcpy(current_velocity_, vel_estimator_.X_, sizeof(current_velocity_));

  auto current_frame = std::make_unique<Frame>();
  current_frame->frame_ = int(seq_);
  current_frame->frame_to_map_ = frame_to_map_;
  current_frame->stamp_ = curr_stamp;
  current_frame->weight_ = det_of_inverse6(icp_.H_adder_);  // pipeline.cpp:223
  // device copy: transformed now, stream-ordered behind the registration; host copy: when somebody reads it
  current_tree->applyTransform(frame_to_map_.R, frame_to_map_.t);
  current_frame->tree_ = std::move(current_tree);
  current_tree_view_ = current_frame->tree_.get();

  frames_.push_back(std::move(current_frame));
  if (frames_.size() > size_t(FRAME_WINDOW)) frames_.pop_front();  // its HBM buffers go back to the library's pool

  if (inliers_ratio < p_th_) {  // keyframe promotion (pipeline.cpp:234-262)
    double best_weight = std::numeric_limits<double>::max();
    int new_seq = 0;
    size_t best = frames_.size();
    for (size_t i = 0; i < frames_.size(); ++i) {
      if (frames_[i]->weight_ < best_weight) {
        best_weight = frames_[i]->weight_;
        new_seq = frames_[i]->frame_;
        best = i;
      }
    }
    if (best < frames_.size()) {  // (all-NaN weights would dereference null in the reference; skip instead)
      std::unique_ptr<Frame> best_frame;
      while (!frames_.empty() && frames_.front()->frame_ <= new_seq) {
        if (frames_.front()->frame_ == new_seq) best_frame = std::move(frames_.front());
        frames_.pop_front();
      }
      // promotion is a pointer move: the tree has been resident, in the map frame, since its own frame
      keyframe_to_map_ = best_frame->frame_to_map_;
      pushKeyframe(std::move(best_frame));  // (and the eviction: buffers back to the pool)
      is_map_updated_ = true;
      seq_keyframe_ = new_seq;
    }
  }
  seq_++;
  foldFrame();
}

// the reference's current_leaves_ are pointers into the current tree, so after compute() they read map-frame means
// (pipeline.cpp:290-297); here they are materialised when asked for (the visualiser), not every frame
// pipeline.cpp:290-297: `current_leaves_` is filled by the first REGISTERED frame (pipeline.cpp:143-144); initialize() (:267-283)
// leaves it empty, so the reference returns nothing after the first scan — mirrored
const ContainerType Pipeline::currentLeaves() {
  if (trajectory_.size() <= 1) return ContainerType{};
  if (current_leaves_host_) return *current_leaves_host_;  // (sharded: the scan was promoted and its tree is another rank's)
  return current_tree_view_ ? current_tree_view_->leafMeans() : ContainerType{};
}

// (sharded: every rank returns the FULL map — the device tree's leaves where this rank owns the keyframe, the host copy taken
// at promotion elsewhere)
const ContainerType Pipeline::modelLeaves() {  // pipeline.cpp:299-308
  ContainerType leaves;
  for (auto& frame : keyframes_) {
    if (!frame->tree_) {
      leaves.insert(leaves.end(), frame->host_leaves_.begin(), frame->host_leaves_.end());
      continue;
    }
    const ContainerType l = frame->tree_->leafMeans();
    leaves.insert(leaves.end(), l.begin(), l.end());
  }
  return leaves;
}

void Pipeline::setShard(int rank, int world) {
  if (is_initialized_ || seq_ != 0) throw std::logic_error("Pipeline::setShard: only before the first compute()");
  if (world < 1 || rank < 0 || rank >= world) throw std::invalid_argument("Pipeline::setShard: need 0 <= rank < world");
  if (realtime_ && world > 1)
    throw std::invalid_argument("Pipeline::setShard: realtime = true cannot be sharded (the round count comes from each rank's "
                                "own wall clock and would differ between the ranks)");
  ledger_.configure(rank, world, num_keyframes_);
}

// pipeline.cpp:252-257 through the ledger: the new keyframe enters the (global) window on every rank, its tree stays on the
// rank that owns its ordinal; the oldest one leaves on every rank, its tree is freed where it was
void Pipeline::pushKeyframe(std::unique_ptr<Frame> frame) {
  const KeyframeLedger::Step step = ledger_.promote();
  if (!step.promoted.local && frame->tree_) {
    frame->host_leaves_ = frame->tree_->leafMeans();  // (already in the map frame: transformed in its own frame's compute())
    if (frame->tree_.get() == current_tree_view_) {
      current_tree_view_ = nullptr;
      current_leaves_host_ = &frame->host_leaves_;  // (the Frame is heap-allocated: the address survives the deque)
    }
    frame->tree_.reset();  // the HBM goes back to the library's pool
  }
  keyframes_.push_back(std::move(frame));
  if (step.evicted) keyframes_.pop_front();
}

// a sharded registration against a context without the communicator would silently register against this rank's part of the
// map alone: refuse it
void Pipeline::checkShardCommunicator() {
  DeviceLock lock(Device::mutex());
  int64_t ranks = 0, rank = -1;
  check(madicp_ctx_get_option(Device::ctx(), "comm_ranks", &ranks), "madicp_ctx_get_option");
  check(madicp_ctx_get_option(Device::ctx(), "comm_rank", &rank), "madicp_ctx_get_option");
  if (ranks != ledger_.world() || rank != ledger_.rank())
    throw std::runtime_error("Pipeline: setShard(" + std::to_string(ledger_.rank()) + ", " + std::to_string(ledger_.world()) +
                             ") but the device context's communicator has " + std::to_string(ranks) + " ranks, this one rank " +
                             std::to_string(rank) + " (install it on madicp_host_device_ctx() before the first compute())");
}

}  // namespace madicp_host
