// The host twin of the device voxel map (csrc/hip/frontend.hip.h: voxel_claim / voxel_mark / voxel_rows / map_rehash; map_prune_mark /
// map_compact; ray_flags / map_clear_mark): a set of float32 rows that folds append to and prune and clearRays alone remove from, one per voxel, the first point ever to fall into a voxel.  The per-point arithmetic is
// csrc/common/export_point.h, shared with the device kernels and the export — the KEY comes from the fp64 position, never from the
// float that is stored.  "Lowest index of the new points of a key" is the order of one sequential pass here, two integer atomics
// behind a kernel boundary there: the map is a function of the sequence of (cloud, pose) alone either way.  Header-only, like
// ingest_records.h: Pipeline (host front-end), the C entry points madicp_host_map_* (voxel_map.cpp) and the thinned export
// (cloud_export.h: one fold into a temporary map) use the one class.  Every translation unit that includes this is compiled without
// floating-point contraction.
// A map made `with_attr` holds one more column: the 32-bit attribute word of every row — its OWNING point's, 0 where the folded
// cloud carries none (madicp_map_create_attr).
// A map made `with_ev` holds the evidence column (export_point.h has the rule: map_evidence_hit / map_evidence_miss): a fold
// reinforces the rows it hits, once per fold, a clearing weakens the rows it sees through, and a row leaves only when its evidence
// is used up (madicp_map_create_ev).
// A map made with `moments_max_count` > 0 holds the moments (../common/voxel_moments.h has the rule): ten 64-bit words per row over
// the points that fell into its voxel, the freeze word beside them, and a key -> row index where the others need only the set
// (madicp_map_create_mom).  The freeze is the device's mechanism, run sequentially: closed_at and the fold ordinal.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../common/export_point.h"
#include "../common/map_align.h"
#include "../common/map_merge.h"
#include "../common/voxel_moments.h"
#include "linalg.h"  // ldlt6_solve, exp_so3: the host's update step (align)

namespace madicp_host {

constexpr int kMapOk = 0, kMapInvalid = -1, kMapCapacity = -4;  // MADICP_OK, MADICP_ERR_INVALID, MADICP_ERR_CAPACITY

class VoxelMap {
 public:
  VoxelMap(double voxel, int64_t initial_rows, int64_t max_rows, bool with_attr = false, bool with_ev = false, uint32_t hit = 1,
           uint32_t miss = 1, uint32_t cap = 1, uint32_t moments_max_count = 0)
      : voxel_(voxel), max_rows_(max_rows), with_attr_(with_attr), with_ev_(with_ev), hit_(hit), miss_(miss), cap_(cap),
        with_mom_(moments_max_count > 0), max_count_(moments_max_count) {
    const size_t first = static_cast<size_t>(std::min(initial_rows, max_rows));
    rows_.reserve(3 * first);
    keys_.reserve(first);
    row_keys_.reserve(first);
    if (with_attr_) attr_.reserve(first);
    if (with_ev_) ev_.reserve(first);
    if (with_mom_) {
      mom_.reserve(kMomentWords * first);
      closed_at_.reserve(first);
      row_of_.reserve(first);
    }
  }
  bool with_ev() const { return with_ev_; }
  bool with_moments() const { return with_mom_; }
  double voxel() const { return voxel_; }
  bool with_attr() const { return with_attr_; }
  int64_t size() const { return static_cast<int64_t>(rows_.size() / 3); }

  // include/madicp_host.h: madicp_host_map_insert / _insert_attr — attr: one word per point, or null (the rows' words are 0)
  int insert(const double* xyz, int64_t n, const double* R, const double* t, int64_t* out_added, int64_t* out_rows,
             const uint32_t* attr = nullptr) {
    if (!out_added || !out_rows || n < 0 || n > kMapMaxRows || (!xyz && n > 0)) return kMapInvalid;
    if (export_refusal(R, t, voxel_)) return kMapInvalid;
    if (size() + n > max_rows_) return kMapCapacity;  // (conservative: decided before a point is looked at, as on the device)
    if (with_mom_ && n > 0 && ordinal_ > kMomentsLastOrdinal) return kMapCapacity;  // (2^32 - 1 folds since creation or clear)
    const int64_t before = size();
    std::unordered_set<uint64_t> met;  // evidence maps: the candidate keys that met a row (this fold's own rows among them)
    for (int64_t i = 0; i < n; ++i) {
      double q[3];
      export_position(xyz + 3 * i, R, t, q);
      const uint64_t key = export_key(q, voxel_);
      if (key == kExportNoKey) continue;
      if (!keys_.insert(key).second) {
        if (with_ev_) met.insert(key);
        if (with_mom_) take_point(row_of_.find(key)->second, q);
        continue;
      }
      for (int k = 0; k < 3; ++k) rows_.push_back(export_value(q[k]));
      row_keys_.push_back(key);
      if (with_attr_) attr_.push_back(attr ? attr[i] : 0u);
      if (with_ev_) ev_.push_back(hit_);
      if (with_mom_) {  // (the creating point is the row's first)
        mom_.insert(mom_.end(), kMomentWords, uint64_t(0));
        closed_at_.push_back(kMomentsNeverClosed);
        row_of_[key] = size() - 1;
        take_point(size() - 1, q);
      }
    }
    if (with_mom_ && n > 0) ++ordinal_;
    if (with_ev_ && !met.empty())  // the rows that were there before the fold: once per fold
      for (int64_t j = 0; j < before; ++j)
        if (met.count(row_keys_[j])) ev_[j] = map_evidence_hit(ev_[j], hit_, cap_);
    *out_added = size() - before;
    *out_rows = size();
    return kMapOk;
  }

  // include/madicp_host.h: madicp_host_map_merge_rows — a batch of saved rows merged in (../common/map_merge.h has the rule): one
  // sequential pass, which IS "the lowest index that carries a new key, in ascending order".  A map without moments has no key -> row
  // index; an evidence map then makes a transient one of its own — over ALL its rows, O(rows) per call whatever n: fine for a
  // restore and for a twin, not for many small batches — a plain map needs none (a key it holds changes nothing).
  int merge_rows(double voxel, const uint64_t* keys, const float* xyz, const uint32_t* attr, const uint32_t* ev, const uint64_t* mom,
                 int64_t n, int64_t* out_added, int64_t* out_rows) {
    if (!out_added || !out_rows) return kMapInvalid;
    bool capacity = false;
    if (map_merge_refusal(MergeBatch{keys, xyz, attr, ev, mom, n}, voxel,
                          MergeTarget{voxel_, with_attr_, with_ev_, with_mom_, size(), max_rows_, ordinal_}, &capacity))
      return capacity ? kMapCapacity : kMapInvalid;
    const int64_t before = size();
    std::unordered_map<uint64_t, int64_t> own_index;
    if (with_ev_ && !with_mom_ && n > 0) {
      own_index.reserve(row_keys_.size() + static_cast<size_t>(n));
      for (int64_t j = 0; j < before; ++j) own_index[row_keys_[j]] = j;
    }
    std::unordered_map<uint64_t, int64_t>* index = with_mom_ ? &row_of_ : with_ev_ ? &own_index : nullptr;
    for (int64_t i = 0; i < n; ++i) {
      const uint64_t key = keys[i];
      int64_t r = -1;
      if (keys_.insert(key).second) {
        r = size();
        rows_.resize(rows_.size() + 3);
        std::memcpy(rows_.data() + 3 * r, xyz + 3 * i, 3 * sizeof(float));  // (bits, not values: a NaN keeps its payload)
        row_keys_.push_back(key);
        if (with_attr_) attr_.push_back(attr[i]);
        if (with_ev_) ev_.push_back(0u);
        if (with_mom_) {
          mom_.insert(mom_.end(), kMomentWords, uint64_t(0));
          closed_at_.push_back(kMomentsNeverClosed);
        }
        if (index) (*index)[key] = r;
      } else if (index) {
        r = index->find(key)->second;
      }
      if (with_ev_) ev_[r] = merge_evidence(ev_[r], ev[i], cap_);
      if (with_mom_ && moment_row_takes(closed_at_[r], ordinal_)) {
        const uint64_t* E = mom + kMomentWords * i;
        uint64_t* M = mom_.data() + kMomentWords * r;
        if (moment_closes(M[0], static_cast<uint32_t>(E[0]), max_count_)) closed_at_[r] = ordinal_;
        for (int k = 0; k < kMomentWords; ++k) M[k] += E[k];
      }
    }
    if (with_mom_ && n > 0) ++ordinal_;
    *out_added = size() - before;
    *out_rows = size();
    return kMapOk;
  }

  // include/madicp_host.h: madicp_host_map_download_f32 / _attr / _keys / _evidence / _moments — rows [first_row, size()) of one
  // column; invalid on a map without it
  int download(int64_t first_row, float* out, int64_t capacity_rows, int64_t* out_n) const {
    return download_column(true, rows_, 3, first_row, out, capacity_rows, out_n);
  }
  int download_attr(int64_t first_row, uint32_t* out, int64_t capacity_rows, int64_t* out_n) const {
    return download_column(with_attr_, attr_, 1, first_row, out, capacity_rows, out_n);
  }
  int download_keys(int64_t first_row, uint64_t* out, int64_t capacity_rows, int64_t* out_n) const {
    return download_column(true, row_keys_, 1, first_row, out, capacity_rows, out_n);
  }
  int download_evidence(int64_t first_row, uint32_t* out, int64_t capacity_rows, int64_t* out_n) const {
    return download_column(with_ev_, ev_, 1, first_row, out, capacity_rows, out_n);
  }
  int download_moments(int64_t first_row, uint64_t* out, int64_t capacity_rows, int64_t* out_n) const {  // as (rows, 10)
    return download_column(with_mom_, mom_, kMomentWords, first_row, out, capacity_rows, out_n);
  }
  // include/madicp_host.h: madicp_host_map_download_rows — the columns of rows [first_row, size()): keys and words where asked for
  int download_rows(int64_t first_row, float* out_xyz, uint64_t* out_keys, uint32_t* out_attr, int64_t capacity_rows, int64_t* out_n) const {
    const int rc = download_column(!out_attr || with_attr_, rows_, 3, first_row, out_xyz, capacity_rows, out_n);
    if (rc == kMapOk && out_keys) copy_window(row_keys_, 1, first_row, *out_n, out_keys);
    if (rc == kMapOk && out_attr) copy_window(attr_, 1, first_row, *out_n, out_attr);
    return rc;
  }

  // include/madicp_host.h: madicp_host_map_download_min_evidence — the rows whose word is >= min_e, in row order, with the columns
  // asked for; a short buffer is not written
  int download_min_evidence(uint32_t min_e, float* out_xyz, uint64_t* out_keys, uint32_t* out_attr, uint32_t* out_ev, int64_t capacity_rows,
                            int64_t* out_n) const {
    if (!with_ev_ || !out_xyz || !out_n || (out_attr && !with_attr_)) return kMapInvalid;
    const int64_t m = size();
    int64_t d = 0;
    for (int64_t j = 0; j < m; ++j) d += ev_[j] >= min_e ? 1 : 0;
    *out_n = d;
    if (capacity_rows < d) return kMapCapacity;
    d = 0;
    for (int64_t j = 0; j < m; ++j) {
      if (ev_[j] < min_e) continue;
      for (int k = 0; k < 3; ++k) out_xyz[3 * d + k] = rows_[3 * j + k];
      if (out_keys) out_keys[d] = row_keys_[j];
      if (out_attr) out_attr[d] = attr_[j];
      if (out_ev) out_ev[d] = ev_[j];
      ++d;
    }
    return kMapOk;
  }

  // include/madicp_host.h: madicp_host_map_download_surfels — map_surfel of rows [first_row, size()): centroid, and normal /
  // eigenvalues / count where asked for
  int download_surfels(int64_t first_row, float* out_centroid, float* out_normal, float* out_eig, uint32_t* out_count, int64_t capacity_rows,
                       int64_t* out_n) const {
    const int rc = window(with_mom_, out_centroid, first_row, capacity_rows, out_n);
    for (int64_t j = 0; rc == kMapOk && j < *out_n; ++j) {
      const int64_t r = first_row + j;
      float nrm[3], eig[3];
      uint32_t count;
      map_surfel(mom_.data() + kMomentWords * r, row_keys_[r], voxel_, out_centroid + 3 * j, nrm, eig, &count);
      for (int k = 0; k < 3; ++k) {
        if (out_normal) out_normal[3 * j + k] = nrm[k];
        if (out_eig) out_eig[3 * j + k] = eig[k];
      }
      if (out_count) out_count[j] = count;
    }
    return rc;
  }

  // include/madicp_host.h: madicp_host_map_track_removed / _removed_count / _take_removed — the removal log (madicp_hip.h has the
  // rule): what prune and clearRays remove below their watermark, oldest first, until it is taken.  Turning it off frees the log.
  void track_removed(bool on) {
    track_ = on;
    if (!on) {
      std::vector<uint64_t>().swap(log_keys_);
      std::vector<float>().swap(log_rows_);
      std::vector<uint32_t>().swap(log_attr_);
    }
  }
  bool tracking() const { return track_; }
  int64_t removed_count() const { return static_cast<int64_t>(log_keys_.size()); }
  int take_removed(uint64_t* out_keys, float* out_xyz, uint32_t* out_attr, int64_t capacity, int64_t* out_n) {
    if (!track_ || !out_keys || !out_xyz || !out_n || (out_attr && !with_attr_)) return kMapInvalid;
    const int64_t n = removed_count();
    *out_n = n;
    if (capacity < n) return kMapCapacity;
    if (n > 0) {
      std::memcpy(out_keys, log_keys_.data(), sizeof(uint64_t) * static_cast<size_t>(n));
      std::memcpy(out_xyz, log_rows_.data(), sizeof(float) * 3 * static_cast<size_t>(n));
      if (out_attr) std::memcpy(out_attr, log_attr_.data(), sizeof(uint32_t) * static_cast<size_t>(n));
    }
    log_keys_.clear();  // (keeps the memory)
    log_rows_.clear();
    log_attr_.clear();
    return kMapOk;
  }

  // include/madicp_host.h: madicp_host_map_prune — rows beyond `radius` of `center` leave (map_row_kept, from the stored float row),
  // their keys leave the set; the kept rows close up in order, keys and attribute words with them: one sequential stable pass.
  // *out_watermark: the kept rows among [0, watermark).
  int prune(const double* center, double radius, int64_t watermark, int64_t* out_removed, int64_t* out_rows, int64_t* out_watermark) {
    if (!center || !out_removed || !out_rows || !out_watermark) return kMapInvalid;
    if (map_prune_refusal(center, radius)) return kMapInvalid;
    if (watermark < 0 || watermark > size()) return kMapInvalid;
    if (log_full()) return kMapCapacity;
    const double r2 = radius * radius;
    close_up([&](int64_t j) { return map_row_kept(rows_.data() + 3 * j, center, r2); }, watermark, out_removed, out_rows, out_watermark);
    return kMapOk;
  }

  // include/madicp_host.h: madicp_host_map_clear_rays — the rays of a scan (export_point.h: ray_length / ray_sample_count / ray_sample)
  // from `origin` to every point of the cloud, both taken into the map frame by (R, t): the candidate keys of the samples are
  // traversed, those of the end points occupied; a row leaves iff its STORED key is traversed and not occupied.  Two sets, then
  // prune's stable pass.  On an evidence map such a row is MISSED: it loses `miss` and leaves only when that uses its word up.
  int clearRays(const double* xyz, int64_t n, const double* R, const double* t, const double* origin, double margin, int64_t watermark,
                int64_t* out_removed, int64_t* out_rows, int64_t* out_watermark) {
    if (!out_removed || !out_rows || !out_watermark || n < 0 || n > kMapMaxRows || (!xyz && n > 0)) return kMapInvalid;
    if (map_clear_refusal(R, t, origin, margin)) return kMapInvalid;
    if (watermark < 0 || watermark > size()) return kMapInvalid;
    if (log_full()) return kMapCapacity;
    std::unordered_set<uint64_t> traversed, occupied;
    if (size() > 0 && n > 0) {
      double qo[3];
      export_position(origin, R, t, qo);
      for (int64_t i = 0; i < n; ++i) {
        double q[3], d[3], s[3];
        export_position(xyz + 3 * i, R, t, q);
        const uint64_t end = export_key(q, voxel_);
        if (end != kExportNoKey) occupied.insert(end);
        const double L = ray_length(qo, q, d);
        const int K = ray_sample_count(L, margin, voxel_);
        uint64_t last = kExportNoKey;
        for (int k = 1; k <= K; ++k) {
          ray_sample(qo, d, L, k, voxel_, s);
          const uint64_t key = export_key(s, voxel_);
          if (key == last || key == kExportNoKey) continue;
          last = key;
          if (keys_.count(key)) traversed.insert(key);  // (a key that owns no row cannot remove one)
        }
      }
    }
    close_up(
        [&](int64_t j) {
          if (!traversed.count(row_keys_[j]) || occupied.count(row_keys_[j])) return true;
          return with_ev_ && map_evidence_miss(&ev_[j], miss_);
        },
        watermark, out_removed, out_rows, out_watermark);
    return kMapOk;
  }

  // include/madicp_host.h: madicp_host_map_query — the nearest row per point (export_point.h has the rule: export_cells,
  // query_cell_key, query_d2, query_before), the map only read.  Per-point buffers may be null; counts = {candidates, matched,
  // within max_dist}.  A map without moments has no key -> row index: the call makes a transient one of its own.
  int query(const double* xyz, int64_t n, const double* R, const double* t, int reach, double max_dist, int32_t* out_row, double* out_d2,
            uint64_t* out_keys, uint32_t* out_attr, uint32_t* out_ev, int64_t capacity_points, uint64_t* out_counts) const {
    if (!out_counts || n < 0 || n > kMapMaxRows || (!xyz && n > 0)) return kMapInvalid;
    if (map_query_refusal(R, t, reach, max_dist)) return kMapInvalid;
    if ((out_attr && !with_attr_) || (out_ev && !with_ev_)) return kMapInvalid;
    if ((out_row || out_d2 || out_keys || out_attr || out_ev) && capacity_points < n) return kMapCapacity;
    std::unordered_map<uint64_t, int64_t> own_index;
    if (!with_mom_ && n > 0) {
      own_index.reserve(row_keys_.size());
      for (int64_t j = 0; j < size(); ++j) own_index[row_keys_[j]] = j;
    }
    const std::unordered_map<uint64_t, int64_t>& index = with_mom_ ? row_of_ : own_index;
    const double md2 = max_dist * max_dist;
    uint64_t candidates = 0, matched = 0, within = 0;
    for (int64_t i = 0; i < n; ++i) {
      double q[3];
      export_position(xyz + 3 * i, R, t, q);
      int32_t cell[3], best = -1;
      double best_d2 = kQueryNoDistance;
      if (export_cells(q, voxel_, cell)) {
        ++candidates;
        for (int c = reach ? 0 : kQueryOwnCell; c < (reach ? kQueryCells : kQueryOwnCell + 1); ++c) {
          uint64_t key;
          if (!query_cell_key(cell, c, &key)) continue;
          const auto it = index.find(key);
          if (it == index.end()) continue;
          const int32_t j = static_cast<int32_t>(it->second);
          const double d2 = query_d2(q, rows_.data() + 3 * it->second);
          if (query_before(d2, j, best_d2, best)) {
            best_d2 = d2;
            best = j;
          }
        }
      }
      if (best >= 0) {
        ++matched;
        if (best_d2 <= md2) ++within;
      }
      if (out_row) out_row[i] = best;
      if (out_d2) out_d2[i] = best_d2;
      if (out_keys) out_keys[i] = best >= 0 ? row_keys_[best] : kExportNoKey;
      if (out_attr) out_attr[i] = best >= 0 ? attr_[best] : 0u;
      if (out_ev) out_ev[i] = best >= 0 ? ev_[best] : 0u;
    }
    out_counts[0] = candidates;
    out_counts[1] = matched;
    out_counts[2] = within;
    return kMapOk;
  }

  // include/madicp_host.h: madicp_host_map_score — query()'s three counts at each of n_poses poses (export_point.h has the rule:
  // map_score_refusal, score_takes_part), over the points i with i % stride == 0; out_counts is n_poses x 3.  The map is only read;
  // the transient key -> row index of a map without moments is made once per call, not once per pose.
  int score(const double* xyz, int64_t n, const double* poses, int64_t n_poses, int reach, double max_dist, int64_t stride,
            uint64_t* out_counts) const {
    if (!out_counts || n < 0 || n > kMapMaxRows || (!xyz && n > 0)) return kMapInvalid;
    if (map_score_refusal(poses, n_poses, reach, max_dist, stride)) return kMapInvalid;
    std::unordered_map<uint64_t, int64_t> own_index;
    if (!with_mom_ && n > 0) {
      own_index.reserve(row_keys_.size());
      for (int64_t j = 0; j < size(); ++j) own_index[row_keys_[j]] = j;
    }
    const std::unordered_map<uint64_t, int64_t>& index = with_mom_ ? row_of_ : own_index;
    const double md2 = max_dist * max_dist;
    for (int64_t k = 0; k < n_poses; ++k) {
      const double* R = poses + kScorePoseDoubles * k;
      const double* t = R + 9;
      uint64_t candidates = 0, matched = 0, within = 0;
      for (int64_t i = 0; i < n; i += stride) {  // (i % stride == 0: score_takes_part)
        double q[3];
        export_position(xyz + 3 * i, R, t, q);
        int32_t cell[3], best = -1;
        double best_d2 = kQueryNoDistance;
        if (!export_cells(q, voxel_, cell)) continue;
        ++candidates;
        for (int c = reach ? 0 : kQueryOwnCell; c < (reach ? kQueryCells : kQueryOwnCell + 1); ++c) {
          uint64_t key;
          if (!query_cell_key(cell, c, &key)) continue;
          const auto it = index.find(key);
          if (it == index.end()) continue;
          const int32_t j = static_cast<int32_t>(it->second);
          const double d2 = query_d2(q, rows_.data() + 3 * it->second);
          if (query_before(d2, j, best_d2, best)) {
            best_d2 = d2;
            best = j;
          }
        }
        if (best >= 0) {
          ++matched;
          if (best_d2 <= md2) ++within;
        }
      }
      out_counts[3 * k] = candidates;
      out_counts[3 * k + 1] = matched;
      out_counts[3 * k + 2] = within;
    }
    return kMapOk;
  }

  // include/madicp_host.h: madicp_host_map_register — `iterations` rounds of point-to-plane Gauss-Newton against the surfels
  // (../common/map_align.h has the rule: align_inlier, align_terms, align_tree), the map only read.  The surfels are map_surfel of
  // every row, once per call; the row of a point is query()'s; the step is ldlt6_solve and exp_so3 of linalg.h.  out_trace:
  // (iterations + 1) x 40, out_counts: (iterations + 1) x 4; out_row / out_e only with iterations == 0.
  int align(const double* xyz, int64_t n, const double* R, const double* t, int reach, double max_dist, double rho, uint32_t min_count,
            double flat, int iterations, double* out_R, double* out_t, double* out_trace, uint64_t* out_counts, int32_t* out_row,
            double* out_e, int64_t capacity_points) const {
    if (!out_R || !out_t || !out_trace || !out_counts || n < 0 || n > kMapMaxRows || (!xyz && n > 0)) return kMapInvalid;
    if (!with_mom_ || map_align_refusal(R, t, reach, max_dist, rho, min_count, flat)) return kMapInvalid;
    if (iterations < 0 || iterations > kAlignMaxIterations || ((out_row || out_e) && iterations > 0)) return kMapInvalid;
    if ((out_row || out_e) && capacity_points < n) return kMapCapacity;
    const size_t m = static_cast<size_t>(size());
    std::vector<float> centroid(3 * m), normal(3 * m), eig(3 * m);
    std::vector<uint32_t> count(m);
    for (size_t j = 0; j < m; ++j)
      map_surfel(mom_.data() + kMomentWords * j, row_keys_[j], voxel_, &centroid[3 * j], &normal[3 * j], &eig[3 * j], &count[j]);
    std::vector<int32_t> row(static_cast<size_t>(n));
    std::vector<double> d2(static_cast<size_t>(n)), x(kAlignTerms * static_cast<size_t>(n > 0 ? n : 1));
    const double md2 = max_dist * max_dist;
    double X[12];
    std::memcpy(X, R, 9 * sizeof(double));
    std::memcpy(X + 9, t, 3 * sizeof(double));
    std::vector<double> trace(static_cast<size_t>(kAlignTraceRow) * (iterations + 1));
    std::vector<uint64_t> counts(static_cast<size_t>(kAlignCounts) * (iterations + 1));
    for (int k = 0; k <= iterations; ++k) {  // (round `iterations` is the closing linearisation: no update)
      uint64_t* cnt = counts.data() + kAlignCounts * k;
      if (query(xyz, n, X, X + 9, reach, max_dist, row.data(), d2.data(), nullptr, nullptr, nullptr, n, cnt) != kMapOk) return kMapInvalid;
      std::fill(x.begin(), x.end(), 0.0);
      for (int64_t i = 0; i < n; ++i) {
        const int32_t j = row[i];
        double e = 0.0;
        if (j >= 0 && align_inlier(d2[i] <= md2, count[j], &eig[3 * j], min_count, flat)) {
          double q[3];
          export_position(xyz + 3 * i, X, X + 9, q);
          e = align_terms(xyz + 3 * i, X, q, &centroid[3 * j], &normal[3 * j], rho, &x[kAlignTerms * i]);
          ++cnt[3];
        }
        if (out_row) out_row[i] = j;
        if (out_e) out_e[i] = e;
      }
      align_tree(x.data(), n > 0 ? n : 1);
      double* row_k = trace.data() + kAlignTraceRow * k;
      std::memcpy(row_k, X, sizeof(X));
      std::memcpy(row_k + 12, x.data(), kAlignTerms * sizeof(double));
      if (k < iterations) align_step(x.data(), X);
    }
    std::memcpy(out_R, X, 9 * sizeof(double));
    std::memcpy(out_t, X + 9, 3 * sizeof(double));
    std::memcpy(out_trace, trace.data(), trace.size() * sizeof(double));
    std::memcpy(out_counts, counts.data(), counts.size() * sizeof(uint64_t));
    return kMapOk;
  }

  void clear() {  // (keeps the memory, forgets the rows)
    rows_.clear();
    keys_.clear();
    row_keys_.clear();
    attr_.clear();
    ev_.clear();
    mom_.clear();
    closed_at_.clear();
    row_of_.clear();
    ordinal_ = 0;
    log_keys_.clear();
    log_rows_.clear();
    log_attr_.clear();
  }

 private:
  // what every window download starts with: the column is there (present), the buffers, first_row within [0, size()]; then *out_n
  // = the window's rows, and a buffer too small for them
  int window(bool present, const void* out, int64_t first_row, int64_t capacity_rows, int64_t* out_n) const {
    if (!present || !out || !out_n || first_row < 0 || first_row > size()) return kMapInvalid;
    *out_n = size() - first_row;
    return capacity_rows < *out_n ? kMapCapacity : kMapOk;
  }
  template <class T>
  static void copy_window(const std::vector<T>& col, int per_row, int64_t first_row, int64_t m, T* out) {
    if (m > 0) std::memcpy(out, col.data() + per_row * first_row, sizeof(T) * per_row * static_cast<size_t>(m));
  }
  template <class T>
  int download_column(bool present, const std::vector<T>& col, int per_row, int64_t first_row, T* out, int64_t capacity_rows, int64_t* out_n) const {
    const int rc = window(present, out, first_row, capacity_rows, out_n);
    if (rc == kMapOk) copy_window(col, per_row, first_row, *out_n, out);
    return rc;
  }

  // a removal on a tracking map whose log holds max_rows entries or more is refused: decided without looking at a row
  bool log_full() const { return track_ && removed_count() >= max_rows_; }

  // the one way rows leave: row j stays iff kept(j) — asked once per row, in row order; the kept rows close up in order, keys, attribute and evidence words with them, the keys
  // of the others leave the set.  *out_watermark: the kept rows among [0, watermark).  On a tracking map the rows that leave from
  // below the watermark go to the removal log, in row order.
  template <class Kept>
  void close_up(Kept kept, int64_t watermark, int64_t* out_removed, int64_t* out_rows, int64_t* out_watermark) {
    const int64_t m = size();
    int64_t d = 0, mark = 0;
    for (int64_t j = 0; j < m; ++j) {
      if (j == watermark) mark = d;
      if (!kept(j)) {
        keys_.erase(row_keys_[j]);
        if (track_ && j < watermark) {
          log_keys_.push_back(row_keys_[j]);
          for (int k = 0; k < 3; ++k) log_rows_.push_back(rows_[3 * j + k]);
          if (with_attr_) log_attr_.push_back(attr_[j]);
        }
        continue;
      }
      if (d != j) {
        for (int k = 0; k < 3; ++k) rows_[3 * d + k] = rows_[3 * j + k];
        row_keys_[d] = row_keys_[j];
        if (with_attr_) attr_[d] = attr_[j];
        if (with_ev_) ev_[d] = ev_[j];
        if (with_mom_) {
          std::copy(mom_.begin() + kMomentWords * j, mom_.begin() + kMomentWords * (j + 1), mom_.begin() + kMomentWords * d);
          closed_at_[d] = closed_at_[j];
        }
      }
      ++d;
    }
    if (watermark == m) mark = d;
    rows_.resize(3 * static_cast<size_t>(d));
    row_keys_.resize(static_cast<size_t>(d));
    if (with_attr_) attr_.resize(static_cast<size_t>(d));
    if (with_ev_) ev_.resize(static_cast<size_t>(d));
    if (with_mom_) {
      mom_.resize(kMomentWords * static_cast<size_t>(d));
      closed_at_.resize(static_cast<size_t>(d));
      if (d < m) {  // (rows moved: the index follows them)
        row_of_.clear();
        for (int64_t j = 0; j < d; ++j) row_of_[row_keys_[j]] = j;
      }
    }
    *out_removed = m - d;
    *out_rows = d;
    *out_watermark = mark;
  }

  // one Gauss-Newton update of the pose X (R row-major | t) from the 28 sums (map_align.h's packing): dx = H^-1 (-b) by the LDLT of
  // linalg.h, X <- X * (exp_so3(dx[3 .. 5]), dx[0 .. 2]) — MADicp::updateState (mad_icp.cpp:105-117 of the reference)
  static void align_step(const double* total, double* X) {
    double H[36], nb[6], dx[6], dR[9], Rn[9], rt[3];
    int v = 0;
    for (int c = 0; c < 6; ++c)
      for (int r = c; r < 6; ++r) H[6 * r + c] = H[6 * c + r] = total[v++];
    for (int r = 0; r < 6; ++r) nb[r] = -total[21 + r];
    ldlt6_solve(H, nb, dx);
    exp_so3(dx + 3, dR);
    matmul3(X, dR, Rn);
    matvec3(X, dx, rt);
    for (int i = 0; i < 3; ++i) X[9 + i] = rt[i] + X[9 + i];
    std::memcpy(X, Rn, sizeof(Rn));
  }

  // one candidate point into row r (voxel_moments.h: moment_row_takes / moment_closes — the device's map_moments, one point at a time)
  void take_point(int64_t r, const double* q) {
    if (!moment_row_takes(closed_at_[r], ordinal_)) return;
    uint32_t w[3];
    moment_offset(q, voxel_, w);
    uint64_t c[9];
    moment_terms(w, c);
    uint64_t* M = mom_.data() + kMomentWords * r;
    if (moment_closes(M[0], 1, max_count_)) closed_at_[r] = ordinal_;
    M[0] += 1;
    for (int k = 0; k < 9; ++k) M[1 + k] += c[k];
  }

  double voxel_;
  int64_t max_rows_;
  bool with_attr_;
  bool with_ev_;
  uint32_t hit_, miss_, cap_;  // the evidence rule's parameters (export_point.h)
  std::vector<float> rows_;
  std::vector<uint32_t> attr_;
  std::vector<uint32_t> ev_;  // evidence maps: one word per row, 1 .. cap_
  bool with_mom_;
  uint32_t max_count_, ordinal_ = 0;              // moments maps: the freeze bound, the folds since creation or clear
  std::vector<uint64_t> mom_;                     // (rows, 10)
  std::vector<uint32_t> closed_at_;               // the ordinal of the fold that froze the row, all ones = none yet
  std::unordered_map<uint64_t, int64_t> row_of_;  // key -> row
  std::vector<uint64_t> row_keys_;  // the key of every row (prune erases by it: a float row cannot reproduce its key)
  std::unordered_set<uint64_t> keys_;
  bool track_ = false;  // the removal log: entries of (key, float row, word), oldest first
  std::vector<uint64_t> log_keys_;
  std::vector<float> log_rows_;
  std::vector<uint32_t> log_attr_;
};

}  // namespace madicp_host
