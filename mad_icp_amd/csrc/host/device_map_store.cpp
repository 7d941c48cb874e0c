// DeviceMapStore — the MapStore (map_store.h) over a device voxel map: every operation is ONE entry point of include/madicp_hip.h on
// the map's id, under the device lock and in the context generation that issued the id.  Nothing is launched, allocated or waited
// for here that the entry point does not do itself.
#include "device.h"
#include "map_store.h"

namespace madicp_host {

namespace {

// The one way to the device for an id of `generation`: the lock, the live context if it is still that generation — else the
// std::logic_error of a `what` that outlived its context — and the call.  what == null: giving an id back, which does not throw —
// an id belongs to the context generation that issued it, after Device::shutdown() there is nothing to give back.
template <class Call>
int on_device(unsigned generation, const char* what, Call&& call) {
  DeviceLock lock(Device::mutex());
  madicp_ctx* ctx = Device::current(generation);
  if (!ctx && !what) return MADICP_OK;
  if (!ctx) throw std::logic_error(std::string("Pipeline: the device context the ") + what + " lived in is gone");
  return call(ctx);
}

class DeviceMapStore final : public MapStore {
 public:
  // the one place that chooses among the four creations
  explicit DeviceMapStore(const MapSpec& s) : with_attr_(s.with_attr) {
    DeviceLock lock(Device::mutex());
    madicp_ctx* ctx = Device::ctx();
    if (s.mom > 0)
      check(madicp_map_create_mom(ctx, s.voxel, s.first_rows, s.max_rows, s.with_attr ? 1 : 0, s.with_ev ? s.ev : nullptr, s.mom, &id_),
            "madicp_map_create_mom");
    else if (s.with_ev)
      check(madicp_map_create_ev(ctx, s.voxel, s.first_rows, s.max_rows, s.with_attr ? 1 : 0, s.ev[0], s.ev[1], s.ev[2], &id_),
            "madicp_map_create_ev");
    else if (s.with_attr)
      check(madicp_map_create_attr(ctx, s.voxel, s.first_rows, s.max_rows, &id_), "madicp_map_create_attr");
    else
      check(madicp_map_create(ctx, s.voxel, s.first_rows, s.max_rows, &id_), "madicp_map_create");
    generation_ = Device::generation();
  }
  ~DeviceMapStore() override {
    on_device(generation_, nullptr, [&](madicp_ctx* ctx) { return madicp_map_release(ctx, id_); });
  }
  bool onDevice() const override { return true; }
  std::string lastError() const override { return std::string(entry_) + ": " + madicp_last_error(); }

  int size(int64_t* out_rows) override {
    return call("madicp_map_size", [&](madicp_ctx* ctx) { return madicp_map_size(ctx, id_, out_rows); });
  }
  int insert(const ScanRef& scan, const double* R, const double* t, int64_t* out_added, int64_t* out_rows) override {
    ScanBorrow b(*this, scan);
    return call("madicp_map_insert_cloud",
                [&](madicp_ctx* ctx) { return madicp_map_insert_cloud(ctx, id_, b.scan().cloud_id, R, t, out_added, out_rows); });
  }
  int merge(double voxel, const uint64_t* keys, const float* xyz, const uint32_t* attr, const uint32_t* ev, const uint64_t* mom, int64_t n,
            int64_t* out_added, int64_t* out_rows) override {
    return call("madicp_map_merge_rows",
                [&](madicp_ctx* ctx) { return madicp_map_merge_rows(ctx, id_, voxel, keys, xyz, attr, ev, mom, n, out_added, out_rows); });
  }
  int prune(const double* center, double radius, int64_t watermark, int64_t* out_removed, int64_t* out_rows, int64_t* out_watermark) override {
    return call("madicp_map_prune",
                [&](madicp_ctx* ctx) { return madicp_map_prune(ctx, id_, center, radius, watermark, out_removed, out_rows, out_watermark); });
  }
  int clearRays(const ScanRef& scan, const double* R, const double* t, const double* origin, double margin, int64_t watermark,
                int64_t* out_removed, int64_t* out_rows, int64_t* out_watermark) override {
    if (!scan.resident() && scan.n == 0) {  // (no ray: nothing to upload, nothing removed, not a call)
      *out_removed = 0;
      *out_watermark = watermark;
      return MADICP_OK;
    }
    ScanBorrow b(*this, scan);
    return call("madicp_map_clear_rays", [&](madicp_ctx* ctx) {
      return madicp_map_clear_rays(ctx, id_, b.scan().cloud_id, R, t, origin, margin, watermark, out_removed, out_rows, out_watermark);
    });
  }
  int query(const ScanRef& scan, const double* R, const double* t, int reach, double max_dist, int32_t* out_row, double* out_d2,
            uint64_t* out_keys, uint32_t* out_attr, uint32_t* out_ev, int64_t capacity_points, uint64_t* out_counts) override {
    ScanBorrow b(*this, scan);
    return call("madicp_map_query_cloud", [&](madicp_ctx* ctx) {
      return madicp_map_query_cloud(ctx, id_, b.scan().cloud_id, R, t, reach, max_dist, out_row, out_d2, out_keys, out_attr, out_ev,
                                    capacity_points, out_counts);
    });
  }
  int score(const ScanRef& scan, const double* poses, int64_t n_poses, int reach, double max_dist, int64_t stride,
            uint64_t* out_counts) override {
    ScanBorrow b(*this, scan);
    return call("madicp_map_score_poses", [&](madicp_ctx* ctx) {
      return madicp_map_score_poses(ctx, id_, b.scan().cloud_id, poses, n_poses, reach, max_dist, stride, out_counts);
    });
  }
  int align(const ScanRef& scan, const double* R, const double* t, const AlignParams& p, int iterations, double* out_R, double* out_t,
            double* out_trace, uint64_t* out_counts, int32_t* out_row, double* out_e, int64_t capacity_points) override {
    ScanBorrow b(*this, scan);
    const madicp_map_align_params params{p.reach, p.max_dist, p.rho, p.min_count, p.flat};
    return call("madicp_map_register_cloud", [&](madicp_ctx* ctx) {
      return madicp_map_register_cloud(ctx, id_, b.scan().cloud_id, R, t, &params, iterations, out_R, out_t, out_trace, out_counts, out_row,
                                       out_e, capacity_points);
    });
  }
  int trackRemoved(bool on) override {
    return call("madicp_map_track_removed", [&](madicp_ctx* ctx) { return madicp_map_track_removed(ctx, id_, on ? 1 : 0); });
  }
  int removedCount(int64_t* out_n) override {
    return call("madicp_map_removed_count", [&](madicp_ctx* ctx) { return madicp_map_removed_count(ctx, id_, out_n); });
  }
  int takeRemoved(uint64_t* out_keys, float* out_xyz, uint32_t* out_attr, int64_t capacity, int64_t* out_n) override {
    return call("madicp_map_take_removed",
                [&](madicp_ctx* ctx) { return madicp_map_take_removed(ctx, id_, out_keys, out_xyz, out_attr, capacity, out_n); });
  }
  int download(int64_t first_row, const MapColumns& out, int64_t capacity_rows, int64_t* out_n) override {
    switch (map_window(out)) {
      case MapWindow::kXyz:
        return call("madicp_map_download_f32",
                    [&](madicp_ctx* ctx) { return madicp_map_download_f32(ctx, id_, first_row, out.xyz, capacity_rows, out_n); });
      case MapWindow::kKeys:
        return call("madicp_map_download_keys",
                    [&](madicp_ctx* ctx) { return madicp_map_download_keys(ctx, id_, first_row, out.keys, capacity_rows, out_n); });
      case MapWindow::kAttr:
        return call("madicp_map_download_attr",
                    [&](madicp_ctx* ctx) { return madicp_map_download_attr(ctx, id_, first_row, out.attr, capacity_rows, out_n); });
      case MapWindow::kEv:
        return call("madicp_map_download_evidence",
                    [&](madicp_ctx* ctx) { return madicp_map_download_evidence(ctx, id_, first_row, out.ev, capacity_rows, out_n); });
      case MapWindow::kMoments:
        return call("madicp_map_download_moments",
                    [&](madicp_ctx* ctx) { return madicp_map_download_moments(ctx, id_, first_row, out.moments, capacity_rows, out_n); });
      case MapWindow::kRows:
        return call("madicp_map_download_rows", [&](madicp_ctx* ctx) {
          return madicp_map_download_rows(ctx, id_, first_row, out.xyz, out.keys, out.attr, capacity_rows, out_n);
        });
      case MapWindow::kNone: break;
    }
    entry_ = "MapStore::download: no such combination of columns";
    return MADICP_ERR_INVALID;
  }
  int downloadMinEvidence(uint32_t min_e, float* out_xyz, uint64_t* out_keys, uint32_t* out_attr, uint32_t* out_ev, int64_t capacity_rows,
                          int64_t* out_n) override {
    return call("madicp_map_download_min_evidence", [&](madicp_ctx* ctx) {
      return madicp_map_download_min_evidence(ctx, id_, min_e, out_xyz, out_keys, out_attr, out_ev, capacity_rows, out_n);
    });
  }
  int downloadSurfels(int64_t first_row, float* out_centroid, float* out_normal, float* out_eig, uint32_t* out_count, int64_t capacity_rows,
                      int64_t* out_n) override {
    return call("madicp_map_download_surfels", [&](madicp_ctx* ctx) {
      return madicp_map_download_surfels(ctx, id_, first_row, out_centroid, out_normal, out_eig, out_count, capacity_rows, out_n);
    });
  }
  int clear() override {
    return call("madicp_map_clear", [&](madicp_ctx* ctx) { return madicp_map_clear(ctx, id_); });
  }

 protected:
  // a host scan goes up once, its column with it where the map and the scan both carry one; the temporary cloud is released on
  // every path out (here, or by the borrow's end)
  ScanRef cross(const ScanRef& scan) override {
    if (scan.resident()) return scan;
    int cloud_id = -1;
    check(call("madicp_cloud_upload", [&](madicp_ctx* ctx) { return madicp_cloud_upload(ctx, scan.xyz, scan.n, &cloud_id); }),
          "madicp_cloud_upload");
    const ScanRef up = ScanRef::cloud(cloud_id, generation_, scan.n, with_attr_ && scan.attr);
    if (up.has_attr) {
      const int rc = call("madicp_cloud_set_attr", [&](madicp_ctx* ctx) { return madicp_cloud_set_attr(ctx, cloud_id, scan.attr, scan.n); });
      if (rc != MADICP_OK) {
        uncross(up);
        check(rc, "madicp_cloud_set_attr");
      }
    }
    return up;
  }
  void uncross(const ScanRef& crossed) noexcept override {
    on_device(generation_, nullptr, [&](madicp_ctx* ctx) { return madicp_cloud_release(ctx, crossed.cloud_id); });
  }

 private:
  template <class Call>
  int call(const char* entry, Call&& c) {
    entry_ = entry;
    return on_device(generation_, "map", c);
  }

  int id_ = -1;
  unsigned generation_ = 0;
  const bool with_attr_;
  const char* entry_ = "";  // the entry point called last: lastError() names it
};

}  // namespace

std::unique_ptr<MapStore> make_device_map_store(const MapSpec& spec) { return std::make_unique<DeviceMapStore>(spec); }

void fetch_resident_scan(const ScanRef& scan, double* xyz, uint32_t* attr) {
  on_device(scan.generation, "scan", [&](madicp_ctx* ctx) {
    check(madicp_cloud_download(ctx, scan.cloud_id, xyz, scan.n), "madicp_cloud_download");
    if (attr) check(madicp_cloud_attr(ctx, scan.cloud_id, attr, scan.n), "madicp_cloud_attr");
    return MADICP_OK;
  });
}

}  // namespace madicp_host
