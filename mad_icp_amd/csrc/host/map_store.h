// MapStore — what Pipeline needs of a voxel map, whichever side the map lives on: the host twin (HostMapStore: a VoxelMap, here) or
// the device map behind madicp_map_* (DeviceMapStore: device_map_store.cpp).  The vocabulary is the one both sides already share — the
// int return codes of include/madicp_hip.h (kMapOk / kMapInvalid / kMapCapacity here), int64_t counts, the same out-parameters — so a
// method of Pipeline is written once and a store only forwards: the device store calls, per operation, exactly one C entry point.
// A SCAN reaches a store as a ScanRef — host pointers or a resident cloud — and crosses to the store's side, when it lies on the
// other one, through a ScanBorrow: one upload (madicp_cloud_upload, madicp_cloud_set_attr) or one download (madicp_cloud_download,
// madicp_cloud_attr), undone when the borrow ends.  An operation given a scan from the other side borrows it for its own duration;
// a caller with several operations on one scan (Pipeline::foldFrame) holds one borrow around them and passes borrow.scan().
// Header-only up to here, like voxel_map.h: this file and voxel_map.cpp need nothing of HIP.
#pragma once
#include <algorithm>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "voxel_map.h"

namespace madicp_host {

// what a map is made from (Pipeline::setMapAccumulation); voxel == 0: accumulation is off and nothing else counts
struct MapSpec {
  double voxel = 0.0;
  int64_t first_rows = 1, max_rows = 1;
  bool with_attr = false, with_ev = false;
  uint32_t ev[3] = {1, 1, 1};  // hit, miss, cap — {1, 1, 1} without evidence
  uint32_t mom = 0;            // moments_max_count (0: no moments)
  bool operator==(const MapSpec& o) const {
    return voxel == o.voxel && first_rows == o.first_rows && max_rows == o.max_rows && with_attr == o.with_attr && with_ev == o.with_ev &&
           std::equal(ev, ev + 3, o.ev) && mom == o.mom;
  }
};

// a scan of n points: host pointers (xyz (n, 3), attr one word per point or null), or a resident cloud of the context generation
// that issued its id (has_attr: the cloud carries the column)
struct ScanRef {
  const double* xyz = nullptr;
  const uint32_t* attr = nullptr;
  int cloud_id = -1;
  unsigned generation = 0;
  int64_t n = 0;
  bool has_attr = false;
  bool resident() const { return cloud_id >= 0; }
  static ScanRef host(const double* xyz, const uint32_t* attr, int64_t n) {
    ScanRef s;
    s.xyz = n > 0 ? xyz : nullptr;
    s.attr = attr;
    s.n = n;
    s.has_attr = attr != nullptr;
    return s;
  }
  static ScanRef cloud(int cloud_id, unsigned generation, int64_t n, bool has_attr) {
    ScanRef s;
    s.cloud_id = cloud_id;
    s.generation = generation;
    s.n = n;
    s.has_attr = has_attr;
    return s;
  }
};

// one window download's buffers: xyz alone, keys alone, attr alone, ev alone, moments alone — that column's own download — or xyz
// with keys and / or attr (the columns of madicp_map_download_rows, their copies before one wait)
struct MapColumns {
  float* xyz = nullptr;
  uint64_t* keys = nullptr;
  uint32_t* attr = nullptr;
  uint32_t* ev = nullptr;
  uint64_t* moments = nullptr;  // as (rows, 10)
};
enum class MapWindow { kNone, kXyz, kKeys, kAttr, kEv, kMoments, kRows };
inline MapWindow map_window(const MapColumns& c) {
  const int others = (c.keys ? 1 : 0) + (c.attr ? 1 : 0) + (c.ev ? 1 : 0) + (c.moments ? 1 : 0);
  if (c.xyz) return c.ev || c.moments ? MapWindow::kNone : others ? MapWindow::kRows : MapWindow::kXyz;
  if (others != 1) return MapWindow::kNone;
  return c.keys ? MapWindow::kKeys : c.attr ? MapWindow::kAttr : c.ev ? MapWindow::kEv : MapWindow::kMoments;
}

class MapStore {
 public:
  virtual ~MapStore() = default;
  virtual bool onDevice() const = 0;
  // why the last call was refused, for an exception's text
  virtual std::string lastError() const = 0;

  virtual int size(int64_t* out_rows) = 0;
  virtual int insert(const ScanRef& scan, const double* R, const double* t, int64_t* out_added, int64_t* out_rows) = 0;
  // madicp_map_merge_rows / VoxelMap::merge_rows: n saved entries, the columns null where the map has none
  virtual int merge(double voxel, const uint64_t* keys, const float* xyz, const uint32_t* attr, const uint32_t* ev, const uint64_t* mom,
                    int64_t n, int64_t* out_added, int64_t* out_rows) = 0;
  virtual int prune(const double* center, double radius, int64_t watermark, int64_t* out_removed, int64_t* out_rows, int64_t* out_watermark) = 0;
  virtual int clearRays(const ScanRef& scan, const double* R, const double* t, const double* origin, double margin, int64_t watermark,
                        int64_t* out_removed, int64_t* out_rows, int64_t* out_watermark) = 0;
  virtual int query(const ScanRef& scan, const double* R, const double* t, int reach, double max_dist, int32_t* out_row, double* out_d2,
                    uint64_t* out_keys, uint32_t* out_attr, uint32_t* out_ev, int64_t capacity_points, uint64_t* out_counts) = 0;
  // madicp_map_score_poses / VoxelMap::score: poses (n_poses, 12), out_counts n_poses x 3
  virtual int score(const ScanRef& scan, const double* poses, int64_t n_poses, int reach, double max_dist, int64_t stride,
                    uint64_t* out_counts) = 0;
  // madicp_map_register_cloud / VoxelMap::align: out_trace (iterations + 1) x 40, out_counts (iterations + 1) x 4
  virtual int align(const ScanRef& scan, const double* R, const double* t, const AlignParams& params, int iterations, double* out_R,
                    double* out_t, double* out_trace, uint64_t* out_counts, int32_t* out_row, double* out_e, int64_t capacity_points) = 0;
  virtual int trackRemoved(bool on) = 0;
  virtual int removedCount(int64_t* out_n) = 0;
  virtual int takeRemoved(uint64_t* out_keys, float* out_xyz, uint32_t* out_attr, int64_t capacity, int64_t* out_n) = 0;
  virtual int download(int64_t first_row, const MapColumns& out, int64_t capacity_rows, int64_t* out_n) = 0;
  virtual int downloadMinEvidence(uint32_t min_e, float* out_xyz, uint64_t* out_keys, uint32_t* out_attr, uint32_t* out_ev, int64_t capacity_rows,
                                  int64_t* out_n) = 0;
  virtual int downloadSurfels(int64_t first_row, float* out_centroid, float* out_normal, float* out_eig, uint32_t* out_count,
                              int64_t capacity_rows, int64_t* out_n) = 0;
  virtual int clear() = 0;

 protected:
  friend class ScanBorrow;
  // `scan` on this store's side: itself where it already is, else its copy there — std::runtime_error when the crossing fails;
  // uncross gives a copy that cross made back and does not throw.  One crossing at a time.
  virtual ScanRef cross(const ScanRef& scan) = 0;
  virtual void uncross(const ScanRef& crossed) noexcept = 0;
};

class ScanBorrow {
 public:
  ScanBorrow(MapStore& store, const ScanRef& scan) : store_(store), scan_(store.cross(scan)), crossed_(scan_.resident() != scan.resident()) {}
  ~ScanBorrow() {
    if (crossed_) store_.uncross(scan_);
  }
  ScanBorrow(const ScanBorrow&) = delete;
  ScanBorrow& operator=(const ScanBorrow&) = delete;
  const ScanRef& scan() const { return scan_; }

 private:
  MapStore& store_;
  const ScanRef scan_;
  const bool crossed_;
};

// how a host store gets at a resident scan: scan.n points into xyz and, where attr is not null, their words; throws what the
// device layer throws.  Pipeline hands fetch_resident_scan (device_map_store.cpp) over; a store that is never shown a resident
// scan needs none.
using ScanFetch = void (*)(const ScanRef& scan, double* xyz, uint32_t* attr);

class HostMapStore final : public MapStore {
 public:
  explicit HostMapStore(const MapSpec& spec, ScanFetch fetch = nullptr)
      : map_(spec.voxel, spec.first_rows, spec.max_rows, spec.with_attr, spec.with_ev, spec.ev[0], spec.ev[1], spec.ev[2], spec.mom), fetch_(fetch) {}
  bool onDevice() const override { return false; }
  std::string lastError() const override { return "the host voxel map refused its arguments"; }

  int size(int64_t* out_rows) override {
    *out_rows = map_.size();
    return kMapOk;
  }
  int insert(const ScanRef& scan, const double* R, const double* t, int64_t* out_added, int64_t* out_rows) override {
    ScanBorrow b(*this, scan);
    return map_.insert(b.scan().xyz, b.scan().n, R, t, out_added, out_rows, b.scan().attr);
  }
  int merge(double voxel, const uint64_t* keys, const float* xyz, const uint32_t* attr, const uint32_t* ev, const uint64_t* mom, int64_t n,
            int64_t* out_added, int64_t* out_rows) override {
    return map_.merge_rows(voxel, keys, xyz, attr, ev, mom, n, out_added, out_rows);
  }
  int prune(const double* center, double radius, int64_t watermark, int64_t* out_removed, int64_t* out_rows, int64_t* out_watermark) override {
    return map_.prune(center, radius, watermark, out_removed, out_rows, out_watermark);
  }
  int clearRays(const ScanRef& scan, const double* R, const double* t, const double* origin, double margin, int64_t watermark,
                int64_t* out_removed, int64_t* out_rows, int64_t* out_watermark) override {
    ScanBorrow b(*this, scan);
    return map_.clearRays(b.scan().xyz, b.scan().n, R, t, origin, margin, watermark, out_removed, out_rows, out_watermark);
  }
  int query(const ScanRef& scan, const double* R, const double* t, int reach, double max_dist, int32_t* out_row, double* out_d2,
            uint64_t* out_keys, uint32_t* out_attr, uint32_t* out_ev, int64_t capacity_points, uint64_t* out_counts) override {
    ScanBorrow b(*this, scan);
    return map_.query(b.scan().xyz, b.scan().n, R, t, reach, max_dist, out_row, out_d2, out_keys, out_attr, out_ev, capacity_points, out_counts);
  }
  int score(const ScanRef& scan, const double* poses, int64_t n_poses, int reach, double max_dist, int64_t stride,
            uint64_t* out_counts) override {
    ScanBorrow b(*this, scan);
    return map_.score(b.scan().xyz, b.scan().n, poses, n_poses, reach, max_dist, stride, out_counts);
  }
  int align(const ScanRef& scan, const double* R, const double* t, const AlignParams& p, int iterations, double* out_R, double* out_t,
            double* out_trace, uint64_t* out_counts, int32_t* out_row, double* out_e, int64_t capacity_points) override {
    ScanBorrow b(*this, scan);
    return map_.align(b.scan().xyz, b.scan().n, R, t, p.reach, p.max_dist, p.rho, p.min_count, p.flat, iterations, out_R, out_t, out_trace,
                      out_counts, out_row, out_e, capacity_points);
  }
  int trackRemoved(bool on) override {
    map_.track_removed(on);
    return kMapOk;
  }
  int removedCount(int64_t* out_n) override {
    *out_n = map_.removed_count();
    return kMapOk;
  }
  int takeRemoved(uint64_t* out_keys, float* out_xyz, uint32_t* out_attr, int64_t capacity, int64_t* out_n) override {
    return map_.take_removed(out_keys, out_xyz, out_attr, capacity, out_n);
  }
  int download(int64_t first_row, const MapColumns& out, int64_t capacity_rows, int64_t* out_n) override {
    switch (map_window(out)) {
      case MapWindow::kXyz: return map_.download(first_row, out.xyz, capacity_rows, out_n);
      case MapWindow::kKeys: return map_.download_keys(first_row, out.keys, capacity_rows, out_n);
      case MapWindow::kAttr: return map_.download_attr(first_row, out.attr, capacity_rows, out_n);
      case MapWindow::kEv: return map_.download_evidence(first_row, out.ev, capacity_rows, out_n);
      case MapWindow::kMoments: return map_.download_moments(first_row, out.moments, capacity_rows, out_n);
      case MapWindow::kRows: return map_.download_rows(first_row, out.xyz, out.keys, out.attr, capacity_rows, out_n);
      case MapWindow::kNone: break;
    }
    return kMapInvalid;
  }
  int downloadMinEvidence(uint32_t min_e, float* out_xyz, uint64_t* out_keys, uint32_t* out_attr, uint32_t* out_ev, int64_t capacity_rows,
                          int64_t* out_n) override {
    return map_.download_min_evidence(min_e, out_xyz, out_keys, out_attr, out_ev, capacity_rows, out_n);
  }
  int downloadSurfels(int64_t first_row, float* out_centroid, float* out_normal, float* out_eig, uint32_t* out_count, int64_t capacity_rows,
                      int64_t* out_n) override {
    return map_.download_surfels(first_row, out_centroid, out_normal, out_eig, out_count, capacity_rows, out_n);
  }
  int clear() override {
    map_.clear();
    return kMapOk;
  }

 protected:
  // a resident scan comes down once, its column with it where the map and the scan both carry one
  ScanRef cross(const ScanRef& scan) override {
    if (!scan.resident()) return scan;
    if (!fetch_) throw std::logic_error("HostMapStore: a resident scan, and no way to fetch it");
    const bool attr = map_.with_attr() && scan.has_attr;
    down_xyz_.resize(3 * static_cast<size_t>(scan.n));
    down_attr_.resize(attr ? static_cast<size_t>(scan.n) : 0);
    fetch_(scan, down_xyz_.data(), attr ? down_attr_.data() : nullptr);
    return ScanRef::host(down_xyz_.data(), attr ? down_attr_.data() : nullptr, scan.n);
  }
  void uncross(const ScanRef&) noexcept override {}  // (the buffers keep their memory for the next crossing)

 private:
  VoxelMap map_;
  ScanFetch fetch_;
  std::vector<double> down_xyz_;
  std::vector<uint32_t> down_attr_;
};

// device_map_store.cpp: a fresh, empty device map of the process-wide context (std::runtime_error when it cannot be made), and the
// ScanFetch over madicp_cloud_download / madicp_cloud_attr
std::unique_ptr<MapStore> make_device_map_store(const MapSpec& spec);
void fetch_resident_scan(const ScanRef& scan, double* xyz, uint32_t* attr);

}  // namespace madicp_host
