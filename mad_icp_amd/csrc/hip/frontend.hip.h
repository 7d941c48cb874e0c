// Scan ingest and motion compensation on the device: what happens to a scan between the sensor
// driver and MADtree::build, for callers that keep the scan in HBM (madicp_cloud_*):
//   ingest : float32 (x, y, z, intensity) records -> fp64 points, range filter, NaN filter, optional KITTI vertical
//            angle correction — apps/cpp_runners/bin_runner.cpp:126-166 of the reference
//   deskew : Pipeline::deskew, mad_icp/src/odometry/pipeline.cpp:79-123 — azimuth sort + per-chunk constant-velocity
//            compensation
//   ingest of raw byte records (additive): a driver's PointCloud2-style buffer — any record step, fields at any alignment, a
//            uint32 / float32 / float64 time field — to a filtered cloud that carries its own normalised stamps
//   ingest of several sources' byte records (additive): the buffers of a multi-head rig, each in its own frame and on its own
//            clock, to ONE base-frame cloud with one set of stamps — the same chain of launches whatever their number
//   deskew from per-point timestamps (additive, the reference has none): the same time model with the chunk read off the
//            acquisition time the sensor driver delivers for every point — one streaming kernel, input order kept
//   export (additive, the way OUT): a resident cloud taken through a pose, written as float32 and thinned to the lowest-index point
//            of every voxel — a hash table of voxel keys claimed with integer atomics, then the tile scan and one scatter
// All of it is HBM-bound streaming work (24-32 bytes per point per pass); the kernels are coalesced grid-stride
// passes, the sort is rocPRIM's radix sort, scans are the three-kernel tile scans of tree_build.hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hip.h"  // solve_pose: the one Gauss-Newton update step (map_align_step)
#include "tree_build.hip.h"
#include "../common/ingest_point.h"
#include "../common/export_point.h"
#include "../common/voxel_moments.h"
#include "../common/map_align.h"
#include "../common/map_merge.h"

#pragma clang fp contract(off)

namespace madicp {
namespace fe {

// ---- upload of a cloud whose coordinates are all exactly floats (every LiDAR driver delivers float32: a KITTI .bin, a
// PointCloud2): half the bytes cross PCIe and are widened here — the same doubles, bit for bit ----------------------
__global__ __launch_bounds__(256) void cloud_widen_f32(const float* __restrict__ in, double* __restrict__ out, long n3) {
  const long i = 4 * ((long)blockIdx.x * blockDim.x + threadIdx.x);
  if (i + 3 < n3) {
    const float4 v = *reinterpret_cast<const float4*>(in + i);
    out[i] = (double)v.x; out[i + 1] = (double)v.y; out[i + 2] = (double)v.z; out[i + 3] = (double)v.w;
  } else {
    for (long k = i; k < n3; ++k) out[k] = (double)in[k];
  }
}

// ---- ingest ----------------------------------------------------------------------------------------------------
// keep[i] = the record survives bin_runner.cpp:149-151: NOT (|p| < min_range or |p| > max_range or a NaN coordinate),
// |p| evaluated in float like Eigen::Vector3f::norm(), compared in double: madicp_host::ingest_drops
// (csrc/common/ingest_point.h, shared with the byte-record kernels below and the host twin).
__global__ void ingest_mark(const float* __restrict__ rec, long n, int stride, double min_range, double max_range,
                            uint32_t* __restrict__ keep) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i <= n; i += (long)gridDim.x * blockDim.x) {
    uint32_t k = 0;
    if (i < n) {
      const bool drop = madicp_host::ingest_drops(rec[i * stride], rec[i * stride + 1], rec[i * stride + 2], min_range, max_range);
      k = drop ? 0u : 1u;
    }
    keep[i] = k;  // (entry n: the scan needs a terminator)
  }
}
// compaction in input order + conversion + the "kitti magic correction" (bin_runner.cpp:153-158): rotate the point by
// VERTICAL_ANGLE_OFFSET about the normalised p x (0,0,1).  sin / cos of the constant angle come from the host (libm).
// The arithmetic is madicp_host::ingest_point (csrc/common/ingest_point.h).
__global__ void ingest_scatter(const float* __restrict__ rec, long n, int stride, const uint32_t* __restrict__ keep,
                               const uint32_t* __restrict__ pos, int kitti, double sin_a, double cos_a, double* __restrict__ out) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    if (!keep[i]) continue;
    double o[3];
    madicp_host::ingest_point(rec[i * stride], rec[i * stride + 1], rec[i * stride + 2], kitti, sin_a, cos_a, o);
    const long d = pos[i];
    out[3 * d] = o[0]; out[3 * d + 1] = o[1]; out[3 * d + 2] = o[2];
  }
}

// ---- ingest of raw byte records with a time field -----------------------------------------------------------------------------
// What a LiDAR driver delivers (a PointCloud2-style buffer): records `step` bytes apart — ANY step from 12 to 256, so with 13 or
// 22 every record sits at another alignment — float32 x / y / z at byte offsets, and a uint32 / float32 / float64 time field (a
// float64 at offset 18 is never 8-aligned).  No lane may therefore load a field from global memory with a typed load.  Instead
// a workgroup takes a TILE of consecutive records, copies the tile's bytes into LDS with coalesced aligned 16-byte loads (the
// tail with dword loads), and each lane assembles its record's fields from LDS bytes (madicp_host::record_f32 / record_time:
// memcpy, never a cast of the address).
// Tile size: records_per_tile(step) records — 256 up to a step of 64 bytes, 128 up to 128, 64 up to 256 — so that a tile is at
// most 16 KiB of LDS whatever the step: at the cap (256 records x 256 bytes = 64 KiB) two workgroups would fill a CU's 160 KiB
// and leave three quarters of its wave slots empty, with 16 KiB the LDS never limits the eight 256-thread workgroups a CU can
// hold.  Every tile size times any step is a multiple of 64 bytes: a tile starts 16-byte aligned.  (Chosen from the resource
// numbers alone; this path has not been timed.)
// The last tile's loads round its length up to a dword: up to 3 bytes past the records, which the caller's buffers cover
// (madicp_cloud_ingest_records).  Loop bounds come from the record count, never from the tile size.
constexpr int kRecTileDwords = 4096;  // 16 KiB
constexpr int kRecMaxBlocks = 4096;   // workgroups of sources_mark (one pair of partial extremes each)
__host__ __device__ inline int records_per_tile(int step) { return step <= 64 ? 256 : (step <= 128 ? 128 : 64); }

struct RecordsResult {  // what the host reads back after the mark pass, in one copy
  double t0, t1;        // the range the stamps are normalised over
  int32_t kept, pad;
};

// `src`: 16-byte aligned start of a tile in global memory, `n_bytes` <= 4 * kRecTileDwords
__device__ inline void records_stage(const unsigned char* __restrict__ src, int n_bytes, uint32_t* __restrict__ s_tile) {
  const int n_dw = (n_bytes + 3) >> 2, n_q = n_dw >> 2;
  const uint4* src_q = reinterpret_cast<const uint4*>(src);
  uint4* dst_q = reinterpret_cast<uint4*>(s_tile);
  for (int k = threadIdx.x; k < n_q; k += blockDim.x) dst_q[k] = src_q[k];
  const uint32_t* src_d = reinterpret_cast<const uint32_t*>(src);
  for (int k = 4 * n_q + threadIdx.x; k < n_dw; k += blockDim.x) s_tile[k] = src_d[k];
}

// The join of a 256-thread workgroup's (mn, mx) pairs, left in thread 0: a 64-lane xor butterfly, four per-wave slots in LDS,
// lane 0 joins them.  Plain comparisons and a fixed shape, no floating-point atomics: min / max do not depend on the order once
// the sign of a zero extreme is canonicalised (records_range).
__device__ inline void block_minmax(double& mn, double& mx) {
  __shared__ double s_mn[4], s_mx[4];
  for (int m = 32; m > 0; m >>= 1) {
    const double a = __shfl_xor(mn, m, 64), b = __shfl_xor(mx, m, 64);
    if (a < mn) mn = a;
    if (b > mx) mx = b;
  }
  if ((threadIdx.x & 63) == 0) {
    s_mn[threadIdx.x >> 6] = mn;
    s_mx[threadIdx.x >> 6] = mx;
  }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < 4; ++w) {
      if (s_mn[w] < mn) mn = s_mn[w];
      if (s_mx[w] > mx) mx = s_mx[w];
    }
}

// one workgroup: the join of the workgroups' extremes, canonicalised as t + 0.0 (a -0.0 extreme becomes +0.0: which of two equal
// zeros a reduction keeps depends on its shape) — or the caller's explicit range — and the survivor count the scan left, into the
// one block the host copies back
__global__ __launch_bounds__(256) void records_range(const double* __restrict__ part, int n_part, int has_time, int explicit_range,
                                                     double e0, double e1, const int32_t* __restrict__ total,
                                                     RecordsResult* __restrict__ res) {
  double mn = __builtin_huge_val(), mx = -__builtin_huge_val();
  if (has_time && !explicit_range)
    for (int k = threadIdx.x; k < n_part; k += blockDim.x) {
      const double a = part[2 * k], b = part[2 * k + 1];
      if (a < mn) mn = a;
      if (b > mx) mx = b;
    }
  block_minmax(mn, mx);
  if (threadIdx.x == 0) {
    res->t0 = explicit_range ? e0 : mn + 0.0;
    res->t1 = explicit_range ? e1 : mx + 0.0;
    res->kept = *total;
    res->pad = 0;
  }
}

// ---- ... of ONE OR SEVERAL sources' byte records into one cloud: the only mark / scatter pair for byte records -------------------
// (madicp_cloud_ingest_records is the one PLAIN source, madicp_host::plain_source: a table of one entry whose flags skip
// sensor_to_base and take the clock as it is, zero trips of source_of_tile's loop.)
// A multi-head rig delivers S buffers per frame, each in its own sensor frame, often with its own record step and time type, each
// time field counting from its own message header (madicp_cloud_ingest_sources).  All of them are staged into ONE device buffer,
// every source at a 64-byte aligned offset, and the two kernels below walk ONE grid-stride loop over the GLOBAL tile index: the
// tiles of source 0, then those of source 1 ... — a source's tiles hold records_per_tile(its step) records, so the 16 KiB tile and
// everything said about it above holds unchanged.  keep[] / pos[] are indexed by GLOBAL record (source 0's records, then source
// 1's ...): the one scan of sources_mark's caller gives the concatenated order, keep[total] is its terminator.
// The table of the sources travels BY VALUE as a kernel argument (1.6 KB of the 4 KB a launch may carry): it is wave-uniform, the
// workgroup finds the source of its tile with at most kMaxSources - 1 scalar comparisons and reads the entry through scalar loads.
// Per record, madicp_host's rules (csrc/common/ingest_point.h): the range filter on the raw floats in the SENSOR's frame with the
// source's own bounds; the time on the common clock (source_clock) — its finiteness, the extremes and the stamp are all judged
// there; the point through ingest_point (the KITTI rotation belongs to the sensor frame) and then sensor_to_base.
constexpr int kSrcKitti = 1, kSrcIdentity = 2, kSrcClockAsIs = 4;  // SourceEntry::flags (decided once, on the host)
struct SourceEntry {
  long byte_off;    // of the source's first record in the staged buffer, a multiple of 64
  long first_tile;  // global index of its first tile
  long first_rec;   // global index of its first record: the base into keep[] / pos[]
  long n;           // records
  madicp_host::RecordLayout L;
  madicp_host::AttrField A;  // read by sources_scatter only, and only where it is given an attribute column
  int32_t per_tile, flags;
  double min_range, max_range;
  double t_scale, t_offset;
  double R[9], t[3];
};
struct SourceTable {
  int32_t n_sources, has_time;
  long n_tiles, n_total;
  SourceEntry src[madicp_host::kMaxSources];
};
static_assert(sizeof(SourceTable) <= 2048, "the table is a kernel argument");

// the source a global tile belongs to (first_tile ascends with the source)
__device__ inline int source_of_tile(const SourceTable& T, long tile) {
  int s = 0;
  for (int k = 1; k < T.n_sources; ++k)
    if (tile >= T.src[k].first_tile) s = k;
  return s;
}

// mark pass: keep[g] (entry n_total: the scan's terminator) and, per workgroup, the min / max of the FINITE times — on the COMMON
// clock — of ALL its records, dropped ones included (the reference's point_cloud2.py:90-93 takes the whole message): part[2 b],
// part[2 b + 1]; +inf / -inf where a workgroup saw none (block_minmax).
__global__ __launch_bounds__(256) void sources_mark(const unsigned char* __restrict__ rec, SourceTable T, uint32_t* __restrict__ keep,
                                                    double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) uint32_t s_tile[kRecTileDwords];
  const unsigned char* s_bytes = reinterpret_cast<const unsigned char*>(s_tile);
  double mn = __builtin_huge_val(), mx = -__builtin_huge_val();
  for (long tile = blockIdx.x; tile < T.n_tiles; tile += gridDim.x) {
    const SourceEntry& E = T.src[source_of_tile(T, tile)];
    const madicp_host::RecordLayout L = E.L;
    const long first = (tile - E.first_tile) * E.per_tile;  // within the source
    const int cnt = (int)min((long)E.per_tile, E.n - first);
    records_stage(rec + E.byte_off + first * L.step, cnt * L.step, s_tile);
    __syncthreads();
    if ((int)threadIdx.x < cnt) {
      const unsigned char* p = s_bytes + threadIdx.x * L.step;
      const bool drop = madicp_host::ingest_drops(madicp_host::record_f32(p + L.off_x), madicp_host::record_f32(p + L.off_y),
                                                  madicp_host::record_f32(p + L.off_z), E.min_range, E.max_range);
      keep[E.first_rec + first + threadIdx.x] = drop ? 0u : 1u;
      if (T.has_time) {
        const double tc = madicp_host::source_clock(madicp_host::record_time(p + L.off_t, L.t_type), E.flags & kSrcClockAsIs, E.t_scale,
                                                    E.t_offset);
        if (madicp_host::time_is_finite(tc)) {
          if (tc < mn) mn = tc;
          if (tc > mx) mx = tc;
        }
      }
    }
    __syncthreads();  // (the next trip overwrites the tile)
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) keep[T.n_total] = 0;
  block_minmax(mn, mx);
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = mn;
    part[2 * blockIdx.x + 1] = mx;
  }
}

// what the host reads back in its one copy: records_range's block, and — only for a caller that asks — the survivors per source
struct SourcesResult {
  RecordsResult r;
  int32_t kept_of[madicp_host::kMaxSources];
};
// one wavefront, launched only for a caller that asks for the counts: survivors of source s = pos[first record of the next
// source] - pos[its own first record] (pos[total] is the scan's last entry: the survivor count)
__global__ __launch_bounds__(64) void sources_counts(SourceTable T, const uint32_t* __restrict__ pos, SourcesResult* __restrict__ res) {
  const int s = threadIdx.x;
  if (s >= T.n_sources) return;
  const long end = s + 1 < T.n_sources ? T.src[s + 1].first_rec : T.n_total;
  res->kept_of[s] = (int32_t)(pos[end] - pos[T.src[s].first_rec]);
}

// scatter pass: the same staging; the survivors' points (madicp_host::ingest_point, the arithmetic of ingest_scatter) taken to
// the base frame and their stamps normalised on the common clock (madicp_host::record_stamp over the range records_range left in
// device memory) to the survivor's position, input order kept.  stamps == nullptr: sources without a time field.  attr == nullptr
// (a kernel argument: the branch is wave-uniform): no attribute is carried; else the survivor's word (madicp_host::record_attr of
// the source's field, from the tile already staged in LDS) goes to the survivor's position too.
__global__ __launch_bounds__(256) void sources_scatter(const unsigned char* __restrict__ rec, SourceTable T, const uint32_t* __restrict__ keep,
                                                       const uint32_t* __restrict__ pos, double sin_a, double cos_a,
                                                       const RecordsResult* __restrict__ res, double* __restrict__ out,
                                                       double* __restrict__ stamps, uint32_t* __restrict__ attr) {
  __shared__ __attribute__((aligned(16))) uint32_t s_tile[kRecTileDwords];
  const unsigned char* s_bytes = reinterpret_cast<const unsigned char*>(s_tile);
  const double t0 = res->t0, t1 = res->t1;
  for (long tile = blockIdx.x; tile < T.n_tiles; tile += gridDim.x) {
    const SourceEntry& E = T.src[source_of_tile(T, tile)];
    const madicp_host::RecordLayout L = E.L;
    const long first = (tile - E.first_tile) * E.per_tile;
    const int cnt = (int)min((long)E.per_tile, E.n - first);
    records_stage(rec + E.byte_off + first * L.step, cnt * L.step, s_tile);
    __syncthreads();
    const long g = E.first_rec + first + threadIdx.x;
    if ((int)threadIdx.x < cnt && keep[g]) {
      const unsigned char* p = s_bytes + threadIdx.x * L.step;
      double o[3];
      madicp_host::ingest_point(madicp_host::record_f32(p + L.off_x), madicp_host::record_f32(p + L.off_y),
                                madicp_host::record_f32(p + L.off_z), E.flags & kSrcKitti, sin_a, cos_a, o);
      if (!(E.flags & kSrcIdentity)) madicp_host::sensor_to_base(E.R, E.t, o);
      const long d = pos[g];
      out[3 * d] = o[0]; out[3 * d + 1] = o[1]; out[3 * d + 2] = o[2];
      if (stamps) {
        const double tc = madicp_host::source_clock(madicp_host::record_time(p + L.off_t, L.t_type), E.flags & kSrcClockAsIs, E.t_scale,
                                                    E.t_offset);
        stamps[d] = madicp_host::record_stamp(tc, t0, t1);
      }
      if (attr) attr[d] = madicp_host::record_attr(p + E.A.off, E.A.type);
    }
    __syncthreads();
  }
}

// ---- deskew ----------------------------------------------------------------------------------------------------
// pipeline.cpp:89-97: azimuth of every point, then an ascending sort by it (radix sort of (azimuth, index) pairs)
__global__ void deskew_keys(const double* __restrict__ xyz, long n, double* __restrict__ key, uint32_t* __restrict__ idx) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    key[i] = atan2(xyz[3 * i + 1], xyz[3 * i]);
    idx[i] = (uint32_t)i;
  }
}

// pipeline.cpp:108-122 walks the sorted points from the largest azimuth down and moves to the next time chunk at most
// ONCE per point, when the point's azimuth is below the current threshold.  With d = n-1-j the position in that walk,
// T_d = number of thresholds above the point's azimuth (thresholds decrease: a binary search in the host-made table of
// the reference's own running `angle`), the chunk after point d is  k_d = min(k_{d-1} + 1, T_d)  =  d + min(1, min_{j<=d}
// (T_j - j)): a prefix minimum.  g[d] = T_d - d is written here, in WALK order (d ascending).
__global__ void deskew_targets(const double* __restrict__ key_sorted, long n, const double* __restrict__ thresholds, int n_thr,
                               int32_t* __restrict__ g) {
  for (long d = blockIdx.x * (long)blockDim.x + threadIdx.x; d < n; d += (long)gridDim.x * blockDim.x) {
    const double a = key_sorted[n - 1 - d];
    // thresholds[k] strictly decreasing; T = #{k : a < thresholds[k]} = first k with !(a < thresholds[k])
    int lo = 0, hi = n_thr;
    while (lo < hi) {
      const int m = (lo + hi) >> 1;
      if (a < thresholds[m]) lo = m + 1; else hi = m;
    }
    g[d] = lo - (int)d;
  }
}

// inclusive prefix minimum of g over d, three kernels like the tile scan (1024 per workgroup)
__global__ __launch_bounds__(256) void pmin_tiles(const int32_t* __restrict__ g, long n, int32_t* __restrict__ tile_min) {
  __shared__ int s_w[4];
  const long base = (long)blockIdx.x * tb::kScanTile + threadIdx.x * 4;
  int v = 0x7fffffff;
  for (int k = 0; k < 4; ++k)
    if (base + k < n) v = min(v, g[base + k]);
  for (int m = 32; m > 0; m >>= 1) v = min(v, __shfl_xor(v, m, 64));
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) tile_min[blockIdx.x] = min(min(s_w[0], s_w[1]), min(s_w[2], s_w[3]));
}
// one workgroup: tile_min[t] <- min over the tiles BEFORE t (exclusive), sequential carry over 256-wide strips
__global__ __launch_bounds__(256) void pmin_top(int32_t* __restrict__ tile_min, int n_tiles) {
  __shared__ int s_w[4];
  __shared__ int s_carry;
  if (threadIdx.x == 0) s_carry = 0x7fffffff;
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int base = 0; base < n_tiles; base += 256) {
    const int i = base + threadIdx.x;
    const int v = i < n_tiles ? tile_min[i] : 0x7fffffff;
    int incl = v;
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(incl, d, 64);
      if (lane >= d) incl = min(incl, o);
    }
    if (lane == 63) s_w[wv] = incl;
    __syncthreads();
    int before = s_carry;                       // everything before this strip
    for (int k = 0; k < wv; ++k) before = min(before, s_w[k]);
    const int excl_in_wave = __shfl_up(incl, 1, 64);
    const int excl = (lane == 0) ? before : min(before, excl_in_wave);
    if (i < n_tiles) tile_min[i] = excl;
    __syncthreads();
    if (threadIdx.x == 255) s_carry = min(before, incl);
    __syncthreads();
  }
}
// the chunk of every point and its compensated position: out[j] = pose[k_d] * p_sorted[j]  (pipeline.cpp:121; the
// output is in azimuth order, like the reference's).  poses: (n_poses, 12) R row-major | t, made by the host with the
// reference's own running time (pipeline.cpp:103-106,113-117).
__global__ __launch_bounds__(256) void deskew_apply(const double* __restrict__ xyz, const uint32_t* __restrict__ idx_sorted, long n,
                                                    const int32_t* __restrict__ g, const int32_t* __restrict__ tile_min,
                                                    const double* __restrict__ poses, int n_poses, double* __restrict__ out,
                                                    int32_t* __restrict__ chunk_of /* optional, walk order */) {
  __shared__ int s_w[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long base = (long)blockIdx.x * tb::kScanTile + threadIdx.x * 4;  // walk positions d
  int m[4], v = 0x7fffffff;
  for (int k = 0; k < 4; ++k) {
    m[k] = (base + k < n) ? g[base + k] : 0x7fffffff;
    v = min(v, m[k]);
  }
  int incl = v;
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(incl, d, 64);
    if (lane >= d) incl = min(incl, o);
  }
  if (lane == 63) s_w[wv] = incl;
  __syncthreads();
  int before = tile_min[blockIdx.x];
  for (int k = 0; k < wv; ++k) before = min(before, s_w[k]);
  const int up = __shfl_up(incl, 1, 64);
  int run = (lane == 0) ? before : min(before, up);
  for (int k = 0; k < 4; ++k) {
    const long d = base + k;
    if (d >= n) break;
    run = min(run, m[k]);
    int kd = (int)d + min(1, run);  // k_d
    kd = max(0, min(kd, n_poses - 1));
    const long j = n - 1 - d;
    const long src = idx_sorted[j];
    const double x = xyz[3 * src], y = xyz[3 * src + 1], z = xyz[3 * src + 2];
    const double* P = poses + 12 * (long)kd;
#ifdef MADICP_XFORM_HOMOGENEOUS  // (Isometry3d * Vector3d in the homogeneous-product order: oracle/linalg.h apply())
    out[3 * j] = ((P[0] * x + P[1] * y) + P[2] * z) + P[9];
    out[3 * j + 1] = ((P[3] * x + P[4] * y) + P[5] * z) + P[10];
    out[3 * j + 2] = ((P[6] * x + P[7] * y) + P[8] * z) + P[11];
#else
    out[3 * j] = P[9] + madicp_host::sum3s(P[0] * x, P[1] * y, P[2] * z);
    out[3 * j + 1] = P[10] + madicp_host::sum3s(P[3] * x, P[4] * y, P[5] * z);
    out[3 * j + 2] = P[11] + madicp_host::sum3s(P[6] * x, P[7] * y, P[8] * z);
#endif
    if (chunk_of) chunk_of[d] = kd;
  }
}
// the attribute column of a cloud that deskew_apply re-orders, taken along: deskew_apply leaves point idx_sorted[j] at position j
__global__ __launch_bounds__(256) void attr_gather(const uint32_t* __restrict__ attr_in, const uint32_t* __restrict__ idx_sorted, long n,
                                                   uint32_t* __restrict__ attr_out) {
  for (long j = blockIdx.x * (long)blockDim.x + threadIdx.x; j < n; j += (long)gridDim.x * blockDim.x) attr_out[j] = attr_in[idx_sorted[j]];
}

// ---- deskew from per-point timestamps ---------------------------------------------------------------------------------
// For sensors whose driver delivers the acquisition time of every point (a PointCloud2 `t` / `timestamp` / `time` field,
// normalised to [0, 1] over the scan): the chunk of a point is a function of that point alone — no azimuth, no sort, no
// prefix minimum.  s in [0, 1] -> k = floor(s * 1023 + 0.5) clamped to [0, 1023] (round half up: a stamp on the boundary
// (k + 0.5) / 1023 belongs to chunk k + 1); NaN — time unknown — is the scan's end, the frame the pose refers to.  Evaluated in
// fp64 WITHOUT contraction (the pragma above): a fused s * 1023 + 0.5 rounds the other way on some boundaries, and the host
// twin (csrc/host/deskew.cpp: deskew_cloud_stamped) must take the same side.  +-inf and out-of-range stamps are clamped
// before the conversion to int.  out[i] = pose[k_i] * p[i], in INPUT order; poses: (1024, 12) as for deskew_apply, gathered
// through L2 (neighbouring points carry neighbouring stamps: a wavefront reads one or two poses).
constexpr int kStampChunks = 1024;  // CHUNKS, tools/constants.h:31
__device__ __host__ inline int stamp_chunk(double s) {
  if (s != s) return kStampChunks - 1;
  const double q = floor(s * double(kStampChunks - 1) + 0.5);
  if (q <= 0.0) return 0;
  if (q >= double(kStampChunks - 1)) return kStampChunks - 1;
  return (int)q;
}
__global__ __launch_bounds__(256) void deskew_stamped(const double* __restrict__ xyz, const double* __restrict__ stamps, long n,
                                                      const double* __restrict__ poses, double* __restrict__ out,
                                                      int32_t* __restrict__ chunk_of /* optional, input order */) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int k = stamp_chunk(stamps[i]);
    const double x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    const double* P = poses + 12 * (long)k;
#ifdef MADICP_XFORM_HOMOGENEOUS
    out[3 * i] = ((P[0] * x + P[1] * y) + P[2] * z) + P[9];
    out[3 * i + 1] = ((P[3] * x + P[4] * y) + P[5] * z) + P[10];
    out[3 * i + 2] = ((P[6] * x + P[7] * y) + P[8] * z) + P[11];
#else
    out[3 * i] = P[9] + madicp_host::sum3s(P[0] * x, P[1] * y, P[2] * z);
    out[3 * i + 1] = P[10] + madicp_host::sum3s(P[3] * x, P[4] * y, P[5] * z);
    out[3 * i + 2] = P[11] + madicp_host::sum3s(P[6] * x, P[7] * y, P[8] * z);
#endif
    if (chunk_of) chunk_of[i] = k;
  }
}

// ---- voxel thinning: a resident cloud folded into a table of voxels, one row per NEW voxel ----------------------------------------
// The rule is madicp_host's (csrc/common/export_point.h: export_position, export_value, export_key — shared with the host twins; the
// key comes from the fp64 position, never from the stored float).  The table is open addressing over `slots` 64-bit keys, empty =
// all ones, linear probing from export_slot0, a slot found or claimed with a 64-bit compare-and-swap: whoever wins, the slot ends up
// holding that key, and a slot never changes once it is set.  Beside every key sits a 32-bit owner word with three states:
//   kMapNever (all ones)   no fold has owned the slot yet — what the ONE memset that empties the table leaves
//   kMapSettled (0)        the slot's key got its row in an EARLIER fold: its points are not new
//   1 .. n                 contended in THIS fold: the lowest index + 1 seen so far (atomicMin; i + 1 >= 1, so the settled word can
//                          never be won, and an atomicMin that meets it leaves it settled)
//   voxel_claim  one lane per point: position, key, the key's slot found or claimed, atomicMin(owner, i + 1) unless settled
//   voxel_mark   behind a kernel boundary (every claim has finished): mark[i] = candidate and owner[slot_of[i]] == i + 1 — the
//                lowest index of a NEW key
//   tile scan    tb_scan_tiles / tb_scan_top / tb_scan_apply: S[i] = marks before i, the total = rows added
//   voxel_rows   marked points: the position, recomputed, as three floats at row first_row + S[i]; where asked for, the row's 64-bit
//                key beside it and the slot settled.  Every slot claimed in a fold has a lowest-index point, so a settling fold
//                leaves none contended: between its folds every owner is kMapNever or kMapSettled.
//   map_rehash   growth: the stored keys of rows [0, M) into a fresh, larger table — all distinct, so claim only — owners settled
// Determinism: "the lowest index of every new voxel" is decided by two integer atomics whose results commute and is read only behind
// a kernel boundary.  Which lane wins a compare-and-swap decides WHERE a key sits, never WHETHER it is in the table or which index
// owns it: the rows are a function of the sequence of (cloud, pose) alone, whatever the launch geometry, the table size or the
// number of growths.  Termination: the table is never more than half full (the callers see to it), so a probe always meets an empty
// slot or its key.  Contention: a plain (relaxed, device-scope) load in front of each atomic skips it where it can no longer change
// anything — a slot that already holds the key, an owner that is already <= i + 1 (owners only fall within a fold, so a stale value
// only costs the atomic it would have saved).  All points in ONE voxel is the worst case: one compare-and-swap wins, the lanes of
// the first wavefronts serialise on one owner word, everybody later reads a smaller owner and passes.  Correct; not tuned for.
// The export (madicp_cloud_export_f32) is the FIRST fold into a scratch table of 2 n slots that the next call wipes: no keys stored,
// nothing settled; voxel == 0 skips the table and sends every point to row i.  The map (madicp_map_*) keeps its table between folds,
// stores every row's key (growth re-inserts from them: a float row cannot reproduce its key) and settles what it appended.
constexpr uint32_t kExportNoSlot = 0xffffffffu;  // slot_of[] of a point that is no candidate
constexpr uint32_t kMapNever = 0xffffffffu, kMapSettled = 0u;
struct ExportPose {  // by value, wave-uniform: scalar loads
  double R[9], t[3];
};
__device__ inline uint32_t export_slot0(uint64_t key, uint32_t slots) {
  uint64_t h = key;  // (the 64-bit finaliser of MurmurHash3: neighbouring cells differ in a few low bits of each 21-bit field)
  h ^= h >> 33; h *= 0xff51afd7ed558ccdull;
  h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull;
  h ^= h >> 33;
  return __umulhi((uint32_t)(h >> 32), slots);  // [0, slots) without a division
}
__device__ inline uint32_t map_find_or_claim(unsigned long long* __restrict__ keys, uint32_t slots, unsigned long long key) {
  uint32_t s = export_slot0(key, slots);
  for (;;) {
    unsigned long long seen = __hip_atomic_load(&keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (seen == madicp_host::kExportNoKey) seen = atomicCAS(&keys[s], (unsigned long long)madicp_host::kExportNoKey, key);
    if (seen == madicp_host::kExportNoKey || seen == key) return s;  // claimed now, or this key's already
    s = (s + 1 == slots) ? 0u : s + 1;
  }
}
__global__ __launch_bounds__(256) void voxel_claim(const double* __restrict__ xyz, long n, ExportPose X, double voxel,
                                                   unsigned long long* __restrict__ keys, uint32_t* __restrict__ owner, uint32_t slots,
                                                   uint32_t* __restrict__ slot_of) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const double p[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
    double q[3];
    madicp_host::export_position(p, X.R, X.t, q);
    const unsigned long long key = madicp_host::export_key(q, voxel);
    uint32_t s = kExportNoSlot;
    if (key != madicp_host::kExportNoKey) {
      s = map_find_or_claim(keys, slots, key);
      // (kMapSettled is 0 and never above i + 1)
      if (__hip_atomic_load(&owner[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > (uint32_t)i + 1u) atomicMin(&owner[s], (uint32_t)i + 1u);
    }
    slot_of[i] = s;
  }
}
__global__ __launch_bounds__(256) void voxel_mark(const uint32_t* __restrict__ slot_of, const uint32_t* __restrict__ owner, long n,
                                                  uint32_t* __restrict__ mark) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i <= n; i += (long)gridDim.x * blockDim.x) {
    uint32_t m = 0;
    if (i < n) {
      const uint32_t s = slot_of[i];
      m = (s != kExportNoSlot && owner[s] == (uint32_t)i + 1u) ? 1u : 0u;
    }
    mark[i] = m;  // (entry n: the scan needs a terminator)
  }
}
// Null arguments (kernel arguments: the branches are wave-uniform) switch parts off.  mark / pos: every point, at row first_row + i.
// row_keys: no key is stored, and none is recomputed (three fp64 divisions per row).  owner / slot_of: nothing settles.
// row_attr: no attribute column beside the rows; else every row written gets its owning point's word, or 0 where the cloud carries
// none (attr == nullptr).  row_ev: no evidence column; else every row written gets `hit`.  slot_row (evidence and moments maps):
// learns the row of every slot that settles.  row_mom / row_closed (moments maps): every row written starts from ten zero words
// and "never closed" — fe::map_moments, behind this kernel, counts its points, the creating one included.
__global__ __launch_bounds__(256) void voxel_rows(const double* __restrict__ xyz, long n, ExportPose X, double voxel,
                                                  const uint32_t* __restrict__ mark, const uint32_t* __restrict__ pos,
                                                  const uint32_t* __restrict__ slot_of, uint32_t* __restrict__ owner, long first_row,
                                                  float* __restrict__ rows, unsigned long long* __restrict__ row_keys,
                                                  const uint32_t* __restrict__ attr, uint32_t* __restrict__ row_attr,
                                                  uint32_t* __restrict__ row_ev, uint32_t hit, uint32_t* __restrict__ slot_row,
                                                  unsigned long long* __restrict__ row_mom, uint32_t* __restrict__ row_closed) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    if (mark && !mark[i]) continue;
    const double p[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
    double q[3];
    madicp_host::export_position(p, X.R, X.t, q);
    const long d = first_row + (mark ? (long)pos[i] : i);
    rows[3 * d] = madicp_host::export_value(q[0]);
    rows[3 * d + 1] = madicp_host::export_value(q[1]);
    rows[3 * d + 2] = madicp_host::export_value(q[2]);
    if (row_keys) row_keys[d] = madicp_host::export_key(q, voxel);
    if (row_attr) row_attr[d] = attr ? attr[i] : 0u;
    if (row_ev) row_ev[d] = hit;                      // (an evidence map: the new row's word)
    if (slot_row) slot_row[slot_of[i]] = (uint32_t)d;  // (where its slot's row is — what map_hit and map_moments read)
    if (row_mom) {
      for (int k = 0; k < madicp_host::kMomentWords; ++k) row_mom[madicp_host::kMomentWords * d + k] = 0ull;
      row_closed[d] = madicp_host::kMomentsNeverClosed;
    }
    if (owner) owner[slot_of[i]] = kMapSettled;  // (one marked point per slot: nobody else writes it in this kernel)
  }
}
__global__ __launch_bounds__(256) void map_rehash(const unsigned long long* __restrict__ row_keys, long n_rows,
                                                  unsigned long long* __restrict__ keys, uint32_t* __restrict__ owner, uint32_t slots,
                                                  uint32_t* __restrict__ slot_row /* evidence and moments maps, else null */) {
  for (long r = blockIdx.x * (long)blockDim.x + threadIdx.x; r < n_rows; r += (long)gridDim.x * blockDim.x) {
    const uint32_t s = map_find_or_claim(keys, slots, row_keys[r]);
    owner[s] = kMapSettled;
    if (slot_row) slot_row[s] = (uint32_t)r;
  }
}

// ---- evidence: the hits of a fold (madicp_map_create_ev; the rule is csrc/common/export_point.h's map_evidence_hit) -----------------
// An evidence map has two more 32-bit words beside every table slot: slot_row, the row of the slot's key — written where a slot
// settles (voxel_rows) and where the table is refilled (map_rehash: at a growth and behind every removal, so it follows its row
// through both) — and stamp, the number of the last fold that hit the slot (all ones: none since the table was last emptied; the
// host counts the folds from 0 again at every wipe and wipes before the count could reach all ones).
//   map_hit  behind voxel_claim's kernel boundary, one lane per point: a slot whose owner is kMapSettled belongs to a row OLDER than
//            this fold (the fold's own slots are contended until voxel_rows settles them, which runs behind this kernel);
//            atomicExch(stamp[s], fold_no) hands the previous stamp to every lane and exactly ONE of a voxel's lanes sees another
//            fold's: that lane does the plain saturating add on ev[slot_row[s]] — no other lane touches that word in this kernel.
// Determinism: who is elected does not matter, only that one is — the result is "+ hit once per voxel and fold", a function of the
// sequence of (cloud, pose) alone.  Contention: a relaxed agent-scope load in front of the exchange skips it once the stamp is this
// fold's (within a fold a stamp only ever becomes fold_no, so a stale value costs one exchange); all points in ONE voxel serialise
// on one word for the first wavefronts and read the stamp afterwards.
__global__ __launch_bounds__(256) void map_hit(const uint32_t* __restrict__ slot_of, const uint32_t* __restrict__ owner, long n,
                                               const uint32_t* __restrict__ slot_row, uint32_t* __restrict__ stamp, uint32_t fold_no,
                                               uint32_t* __restrict__ ev, uint32_t hit, uint32_t cap) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const uint32_t s = slot_of[i];
    if (s == kExportNoSlot || owner[s] != kMapSettled) continue;
    if (__hip_atomic_load(&stamp[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == fold_no) continue;
    if (atomicExch(&stamp[s], fold_no) == fold_no) continue;
    const uint32_t r = slot_row[s];
    ev[r] = madicp_host::map_evidence_hit(ev[r], hit, cap);
  }
}

// ---- moments: count, sums and sums of products of the points of every voxel (madicp_map_create_mom) ------------------------------
// The rule is csrc/common/voxel_moments.h's, shared with the host twin: a 16-bit offset per axis inside the voxel, ten unsigned
// 64-bit words per row (n, S1[3], S2[6]), and max_count, past which a row takes no further fold.
//   map_moments  behind voxel_rows, one lane per point: by then every slot of the fold is settled and slot_row knows the row of every
//                slot, this fold's new rows included (their words zeroed by voxel_rows).  A candidate lane recomputes q and w and
//                finds r = slot_row[slot_of[i]]; a lane skips a row iff closed_at[r] holds an ordinal other than "never" and other
//                than this fold's.  Neighbouring returns share voxels, so the lanes of a wavefront that hold a RUN of equal rows
//                (adjacent lanes, the same r) add their ten terms up in registers first — a segmented inclusive scan over the run
//                by shuffles, six steps — and the run's last lane issues the ten 64-bit integer atomics for all of them.  The add
//                on n is the one that RETURNS: the single run that sees old < max_count <= old + cnt (the intervals [old, old + cnt)
//                of a row's runs tile its count) stores the fold's ordinal into closed_at[r].
// Determinism: within a fold closed_at[r] only goes from "never" to this fold's ordinal, and a lane proceeds on either, so what a
// racing load returns decides nothing; a row closed by an earlier fold is skipped by every lane.  "All candidate points of the fold,
// or none, by n before the fold" is therefore decided without a second launch; and the sums are integer sums, associative and
// commutative — how the points are grouped into runs, which depends on the launch geometry, changes no bit: the words are a
// function of the sequence of (cloud, pose) alone.  No float atomics.  Contention: all points in ONE voxel is one run per wavefront,
// ten atomics per 64 points on ten words — correct, not tuned for.
// -DMADICP_MOMENTS_PLAIN (a measurement aid, tools/map_moments_time.py --variant): the form without the scan, ten atomics per
// point — the same bits, measured 0.044 ms slower per fold of 120 k points (profiles/map_moments_time.md).
__device__ inline unsigned long long shfl_up_u64(unsigned long long v, int d) {
  const uint32_t lo = __shfl_up((uint32_t)v, d), hi = __shfl_up((uint32_t)(v >> 32), d);
  return ((unsigned long long)hi << 32) | lo;
}
__global__ __launch_bounds__(256) void map_moments(const double* __restrict__ xyz, long n, ExportPose X, double voxel,
                                                   const uint32_t* __restrict__ slot_of, const uint32_t* __restrict__ slot_row,
                                                   unsigned long long* __restrict__ mom, uint32_t* __restrict__ closed_at, uint32_t ordinal,
                                                   uint32_t max_count) {
  constexpr uint32_t kNoRow = 0xffffffffu;  // no candidate, or a row that takes nothing in this fold (rows are < 2^30)
  const int lane = threadIdx.x & 63;
  // (blockDim and the stride are multiples of 64: i - lane is the wavefront's, so all its lanes leave the loop together)
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i - lane < n; i += (long)gridDim.x * blockDim.x) {
    uint32_t r = kNoRow;
    uint32_t a[4] = {0, 0, 0, 0};  // n, S1: at most 64 x 65535 within a wavefront
    unsigned long long b[6] = {0, 0, 0, 0, 0, 0};
    if (i < n) {
      const uint32_t s = slot_of[i];
      if (s != kExportNoSlot) {
        const uint32_t row = slot_row[s];
        if (madicp_host::moment_row_takes(__hip_atomic_load(&closed_at[row], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), ordinal)) {
          r = row;
          const double p[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
          double q[3];
          madicp_host::export_position(p, X.R, X.t, q);
          uint32_t w[3];
          madicp_host::moment_offset(q, voxel, w);
          uint64_t c[9];
          madicp_host::moment_terms(w, c);
          a[0] = 1;
          for (int k = 0; k < 3; ++k) a[1 + k] = w[k];
          for (int k = 0; k < 6; ++k) b[k] = c[3 + k];
        }
      }
    }
#ifndef MADICP_MOMENTS_PLAIN
    const uint32_t left = __shfl_up(r, 1);
    const unsigned long long heads = __ballot(lane == 0 || left != r);  // the lanes that start a run
    const int head = 63 - __clzll(heads & ((2ull << lane) - 1ull));    // (lane 63: 2 << 63 wraps to 0, minus 1 is all ones)
    for (int d = 1; d < 64; d <<= 1) {
      uint32_t ua[4];
      unsigned long long ub[6];
      for (int k = 0; k < 4; ++k) ua[k] = __shfl_up(a[k], d);
      for (int k = 0; k < 6; ++k) ub[k] = shfl_up_u64(b[k], d);
      if (lane - d >= head) {
        for (int k = 0; k < 4; ++k) a[k] += ua[k];
        for (int k = 0; k < 6; ++k) b[k] += ub[k];
      }
    }
    const bool last = lane == 63 || ((heads >> (lane + 1)) & 1ull);
#else
    const bool last = true;
#endif
    if (last && r != kNoRow) {
      unsigned long long* M = mom + (size_t)madicp_host::kMomentWords * r;
      const unsigned long long old = atomicAdd(&M[0], (unsigned long long)a[0]);
      if (madicp_host::moment_closes(old, a[0], max_count))
        __hip_atomic_store(&closed_at[r], ordinal, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      for (int k = 0; k < 3; ++k) atomicAdd(&M[1 + k], (unsigned long long)a[1 + k]);
      for (int k = 0; k < 6; ++k) atomicAdd(&M[4 + k], b[k]);
    }
  }
}
//   map_surfels  one lane per row of the window [first_row, M): the row's ten words and stored key through madicp_host::map_surfel
//                into a transient block of the call's own — centroid, normal, eigenvalues (three floats each) and the count
__global__ __launch_bounds__(256) void map_surfels(const unsigned long long* __restrict__ mom, const unsigned long long* __restrict__ row_keys,
                                                   long first_row, long n_rows, double voxel, float* __restrict__ centroid,
                                                   float* __restrict__ normal, float* __restrict__ eig, uint32_t* __restrict__ count) {
  for (long j = blockIdx.x * (long)blockDim.x + threadIdx.x; j < n_rows - first_row; j += (long)gridDim.x * blockDim.x) {
    const long r = first_row + j;
    uint64_t M[madicp_host::kMomentWords];
    for (int k = 0; k < madicp_host::kMomentWords; ++k) M[k] = mom[madicp_host::kMomentWords * r + k];
    float c[3], nrm[3], e[3];
    uint32_t cnt;
    madicp_host::map_surfel(M, row_keys[r], voxel, c, nrm, e, &cnt);
    for (int k = 0; k < 3; ++k) {
      centroid[3 * j + k] = c[k];
      normal[3 * j + k] = nrm[k];
      eig[3 * j + k] = e[k];
    }
    count[j] = cnt;
  }
}

// ---- merging saved rows: a batch of downloaded rows folded back into a map (madicp_map_merge_rows) --------------------------------
// The rule is csrc/common/map_merge.h's, shared with the host twin.  The batch lies in a transient device block of the call's own
// (MergeRows: null where the map has no such column); the table, the owner words and the per-fold scratch are the fold's, and so is
// the shape — claim, mark, tile scan, append — with the batch's keys in place of the keys of positions:
//   rows_claim    one lane per entry: the entry's key found or claimed (map_find_or_claim), atomicMin(owner, i + 1) unless settled, with
//                 voxel_claim's two relaxed loads in front of the atomics; slot_of[i] is always a slot (a key has no bit 63: every entry
//                 is a candidate)
//   voxel_mark / tile scan   unchanged: mark[i] = the lowest index of a key the map did not hold, S[i] = marks before i
//   rows_append   marked entries: key, the three floats and the attribute word COPIED as 32-bit words (NaN payloads and -0.0 are bits)
//                 to row first_row + S[i]; the evidence word starts at 0, the ten moment words at 0 and closed_at at "never" — what
//                 rows_combine adds to; slot_row learns the row and the owner settles (one marked entry per slot)
//   rows_combine  evidence and moments maps only, behind rows_append (every slot settled, slot_row complete), one lane per entry:
//                 r = slot_row[slot_of[i]].  Evidence: a 32-bit compare-and-swap loop new = merge_evidence(old, e_i, cap).  Moments:
//                 where moment_row_takes(closed_at[r], ordinal), ten 64-bit integer atomicAdds; the add on n is the one that RETURNS
//                 and the single entry that sees old < max_count <= old + n_i stores the merge's ordinal into closed_at[r] — exactly
//                 map_moments' mechanism, an entry's n_i in place of a run's count.
// Determinism: rows are decided as in the fold — two integer atomics whose results commute, read behind a kernel boundary.  The
// evidence word is a saturating sum: min(min(e + a, cap) + b, cap) == min(e + a + b, cap), so the order in which the swaps succeed
// changes no bit; a loop that reads cap leaves at once (the word only rises within the kernel, so a stale value costs one swap).
// The moment words are integer sums, and within a merge closed_at[r] only goes from "never" to this merge's ordinal, a lane proceeds
// on either: what a racing load returns decides nothing.  A function of (map, batch) alone, whatever the launch geometry.  No float
// atomics.  Contention: a saved map has ONE entry per key — ten uncontended atomics per entry; all entries on ONE key serialise on
// one evidence word and ten moment words, one atomic per entry and word: correct, not tuned for.
struct MergeRows {  // by value: the batch's columns on the device
  const unsigned long long* keys;
  const uint32_t* xyz;  // (n, 3) the floats' bits
  const uint32_t* attr;
  const uint32_t* ev;
  const unsigned long long* mom;  // (n, 10)
};
__global__ __launch_bounds__(256) void rows_claim(const unsigned long long* __restrict__ batch_keys, long n,
                                                  unsigned long long* __restrict__ keys, uint32_t* __restrict__ owner, uint32_t slots,
                                                  uint32_t* __restrict__ slot_of) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const uint32_t s = map_find_or_claim(keys, slots, batch_keys[i]);
    // (kMapSettled is 0 and never above i + 1)
    if (__hip_atomic_load(&owner[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > (uint32_t)i + 1u) atomicMin(&owner[s], (uint32_t)i + 1u);
    slot_of[i] = s;
  }
}
// Null arguments (kernel arguments: the branches are wave-uniform) are the columns the map lacks: B.attr / row_attr, row_ev with
// slot_row, row_mom with row_closed.
__global__ __launch_bounds__(256) void rows_append(MergeRows B, long n, const uint32_t* __restrict__ mark, const uint32_t* __restrict__ pos,
                                                   const uint32_t* __restrict__ slot_of, uint32_t* __restrict__ owner, long first_row,
                                                   uint32_t* __restrict__ rows, unsigned long long* __restrict__ row_keys,
                                                   uint32_t* __restrict__ row_attr, uint32_t* __restrict__ row_ev,
                                                   uint32_t* __restrict__ slot_row, unsigned long long* __restrict__ row_mom,
                                                   uint32_t* __restrict__ row_closed) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    if (!mark[i]) continue;
    const long d = first_row + (long)pos[i];
    rows[3 * d] = B.xyz[3 * i];
    rows[3 * d + 1] = B.xyz[3 * i + 1];
    rows[3 * d + 2] = B.xyz[3 * i + 2];
    row_keys[d] = B.keys[i];
    if (row_attr) row_attr[d] = B.attr[i];
    if (row_ev) row_ev[d] = 0u;  // (rows_combine adds the entries' words, this one's among them)
    if (slot_row) slot_row[slot_of[i]] = (uint32_t)d;
    if (row_mom) {
      for (int k = 0; k < madicp_host::kMomentWords; ++k) row_mom[madicp_host::kMomentWords * d + k] = 0ull;
      row_closed[d] = madicp_host::kMomentsNeverClosed;
    }
    owner[slot_of[i]] = kMapSettled;  // (one marked entry per slot: nobody else writes it in this kernel)
  }
}
__global__ __launch_bounds__(256) void rows_combine(MergeRows B, long n, const uint32_t* __restrict__ slot_of,
                                                    const uint32_t* __restrict__ slot_row, uint32_t* __restrict__ ev, uint32_t cap,
                                                    unsigned long long* __restrict__ mom, uint32_t* __restrict__ closed_at, uint32_t ordinal,
                                                    uint32_t max_count) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const uint32_t r = slot_row[slot_of[i]];
    if (ev) {
      const uint32_t e_i = B.ev[i];
      uint32_t old = __hip_atomic_load(&ev[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      for (;;) {
        const uint32_t next = madicp_host::merge_evidence(old, e_i, cap);
        if (next == old) break;  // (e_i >= 1: only at cap, and the word does not fall within this kernel)
        const uint32_t seen = atomicCAS(&ev[r], old, next);
        if (seen == old) break;
        old = seen;
      }
    }
    if (mom && madicp_host::moment_row_takes(__hip_atomic_load(&closed_at[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), ordinal)) {
      const unsigned long long* E = B.mom + (size_t)madicp_host::kMomentWords * i;
      unsigned long long* M = mom + (size_t)madicp_host::kMomentWords * r;
      const unsigned long long n_i = E[0];  // (1 .. 2^31 - 1: map_merge_refusal)
      const unsigned long long old = atomicAdd(&M[0], n_i);
      if (madicp_host::moment_closes(old, (uint32_t)n_i, max_count))
        __hip_atomic_store(&closed_at[r], ordinal, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      for (int k = 1; k < madicp_host::kMomentWords; ++k) atomicAdd(&M[k], E[k]);
    }
  }
}

// ---- pruning the map: rows beyond a radius of a centre leave, the kept ones close up in order (madicp_map_prune) -------------------
// The rule is madicp_host::map_row_kept (csrc/common/export_point.h, shared with the host twin): fp64, from the STORED float row.
//   map_prune_mark  one lane per row: mark[j] = the row stays; mark[M] = 0, the scan's terminator (as in voxel_mark)
//   tile scan       over marks and positions of the prune's own (a map is many clouds: not the builder's S / tile_sums)
//   map_compact     one lane per row: a kept row's stored key, three floats and, where the column exists, its word to row S[j] of the
//                   DESTINATION block — coalesced reads, monotone writes; whether row j stays is read off the scan, S[j + 1] != S[j],
//                   so the marks are dead by now and the lane of row 0 leaves {S[M], S[watermark]} in `res` (the caller lays it over
//                   them): both answers of a prune in one small copy.  ev / out_ev: the evidence column, a null-able pair like attr;
//                   mom / out_mom with closed_at / out_closed_at: the moments (ten words a row) and their freeze word, likewise
// The table is then emptied by the one memset and refilled by map_rehash over the kept keys, which leaves every owner kMapNever or
// kMapSettled — what the folds rely on.  Determinism: a comparison per row and an exclusive scan; nothing depends on the geometry.
struct PruneSphere {  // by value, wave-uniform: scalar loads
  double c[3], r2;
};
__global__ __launch_bounds__(256) void map_prune_mark(const float* __restrict__ rows, long n_rows, PruneSphere Q, uint32_t* __restrict__ mark) {
  for (long j = blockIdx.x * (long)blockDim.x + threadIdx.x; j <= n_rows; j += (long)gridDim.x * blockDim.x) {
    uint32_t m = 0;
    if (j < n_rows) {
      const float row[3] = {rows[3 * j], rows[3 * j + 1], rows[3 * j + 2]};
      m = madicp_host::map_row_kept(row, Q.c, Q.r2) ? 1u : 0u;
    }
    mark[j] = m;  // (entry n_rows: the scan needs a terminator)
  }
}
// the row columns of a block as a kernel takes them, by value — one for where rows come from, one for where they go (null: no such column)
struct MapRows {
  unsigned long long* keys;
  float* xyz;
  uint32_t *attr, *ev;
  unsigned long long* mom;
  uint32_t* closed_at;
};
// (the bodies take the columns as __restrict__ parameters, the kernels below hand them the structs' members: a struct member cannot
// promise that the columns do not overlap, and without the promise every one of a row's moment words waits for the one before it)
__device__ __forceinline__ void map_compact_rows(const uint32_t* __restrict__ pos, long n_rows, long watermark,
                                                 const unsigned long long* __restrict__ row_keys, const float* __restrict__ rows,
                                                 const uint32_t* __restrict__ attr, unsigned long long* __restrict__ out_keys,
                                                 float* __restrict__ out_rows, uint32_t* __restrict__ out_attr, uint32_t* __restrict__ res,
                                                 const uint32_t* __restrict__ ev, uint32_t* __restrict__ out_ev,
                                                 const unsigned long long* __restrict__ mom, unsigned long long* __restrict__ out_mom,
                                                 const uint32_t* __restrict__ closed_at, uint32_t* __restrict__ out_closed_at) {
  for (long j = blockIdx.x * (long)blockDim.x + threadIdx.x; j < n_rows; j += (long)gridDim.x * blockDim.x) {
    if (j == 0) {
      res[0] = pos[n_rows];
      res[1] = pos[watermark];
    }
    const long d = pos[j];
    if ((long)pos[j + 1] == d) continue;
    out_keys[d] = row_keys[j];
    out_rows[3 * d] = rows[3 * j];
    out_rows[3 * d + 1] = rows[3 * j + 1];
    out_rows[3 * d + 2] = rows[3 * j + 2];
    if (attr) out_attr[d] = attr[j];
    if (ev) out_ev[d] = ev[j];
    if (mom) {
      for (int k = 0; k < madicp_host::kMomentWords; ++k) out_mom[madicp_host::kMomentWords * d + k] = mom[madicp_host::kMomentWords * j + k];
      out_closed_at[d] = closed_at[j];
    }
  }
}
__global__ __launch_bounds__(256) void map_compact(const uint32_t* pos, long n_rows, long watermark, MapRows in, MapRows out, uint32_t* res) {
  map_compact_rows(pos, n_rows, watermark, in.keys, in.xyz, in.attr, out.keys, out.xyz, out.attr, res, in.ev, out.ev, in.mom, out.mom,
                   in.closed_at, out.closed_at);
}
// The removal log of a tracking map (madicp_map_track_removed): map_compact's complement over the rows below the watermark, beside it
// behind the same scan.  One lane per row j < n_below = min(watermark, M): row j leaves iff pos[j + 1] == pos[j], and its place in
// the log is base + (j - pos[j]) — the rows removed before j, behind the `base` entries the log already holds: no second scan, no
// atomics, coalesced reads, monotone writes.  Reads the scan and the OLD block only, never the marks (in the clearing path the scan
// lies over the dead ray flags, and map_compact's lane 0 writes its two answers over the first marks).  At most n_below entries are
// written: the caller has ensured base + n_below.
__device__ __forceinline__ void map_log_removed_rows(const uint32_t* __restrict__ pos, long n_below, long base,
                                                     const unsigned long long* __restrict__ row_keys, const float* __restrict__ rows,
                                                     const uint32_t* __restrict__ attr, unsigned long long* __restrict__ log_keys,
                                                     float* __restrict__ log_rows, uint32_t* __restrict__ log_attr) {
  for (long j = blockIdx.x * (long)blockDim.x + threadIdx.x; j < n_below; j += (long)gridDim.x * blockDim.x) {
    const long d = pos[j];
    if ((long)pos[j + 1] != d) continue;
    const long e = base + (j - d);
    log_keys[e] = row_keys[j];
    log_rows[3 * e] = rows[3 * j];
    log_rows[3 * e + 1] = rows[3 * j + 1];
    log_rows[3 * e + 2] = rows[3 * j + 2];
    if (attr) log_attr[e] = attr[j];
  }
}
__global__ __launch_bounds__(256) void map_log_removed(const uint32_t* pos, long n_below, long base, MapRows in, MapRows log) {
  map_log_removed_rows(pos, n_below, base, in.keys, in.xyz, in.attr, log.keys, log.xyz, log.attr);
}

// ---- clearing the map by a scan's rays: rows whose voxel a ray passes through and no point of the scan lies in leave ----------------
// (madicp_map_clear_rays).  The rule is csrc/common/export_point.h's, shared with the host twin: ray_length, ray_sample_count,
// ray_sample, export_key.  A second way to produce the marks of a prune; behind them everything is the prune's.
//   ray_flags       ONE WAVEFRONT PER RAY: lane l takes the samples k = l + 1, l + 65, ... of the ray, so a wavefront's time is its own
//                   ray's length / 64 and rays of 2 m and 80 m side by side in the cloud do not wait for each other; lane 0 also takes
//                   the end point.  A key is looked up in the LIVE table with map_find — the table is only read: a key that is not in
//                   it owns no row and is skipped — and its bit set in `flags`, one 32-bit word per table slot in scratch of the call's
//                   own: bit 0 traversed, bit 1 occupied.  A lane whose key equals its left neighbour's (sample k - 1; lane 0: lane 63
//                   of the pass before) skips the probe: that lane does it.
//   map_clear_mark  one lane per row: the slot of the row's stored key (always present), mark[j] = the row stays = its flags are not
//                   exactly "traversed"; mark[M] = 0, the scan's terminator
// Determinism: the flags are ORs of bits, which commute, read only behind a kernel boundary; the table is not written.  Nothing
// depends on the geometry or on timing.  Contention: a relaxed agent-scope load in front of each atomicOr skips it once the bit is
// there (bits are only ever set, so a stale value costs one atomic and nothing else); all rays through ONE voxel serialise on one
// word for the first wavefronts and read the bit afterwards.  Termination: the table is at most half full, so a probe meets an empty
// slot or its key; a ray walks at most kRayMaxSamples samples.
constexpr uint32_t kRayTraversed = 1u, kRayOccupied = 2u;
__device__ inline uint32_t map_find(const unsigned long long* __restrict__ keys, uint32_t slots, unsigned long long key) {
  uint32_t s = export_slot0(key, slots);
  for (;;) {
    const unsigned long long seen = keys[s];
    if (seen == key) return s;
    if (seen == madicp_host::kExportNoKey) return kExportNoSlot;
    s = (s + 1 == slots) ? 0u : s + 1;
  }
}
__device__ inline void ray_flag(uint32_t* __restrict__ flags, uint32_t slot, uint32_t bit) {
  if (!(__hip_atomic_load(&flags[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) atomicOr(&flags[slot], bit);
}
struct RayFrame {  // by value, wave-uniform: scalar loads
  ExportPose X;
  double o[3], margin;  // the sensor origin in the cloud's frame
};
__global__ __launch_bounds__(256) void ray_flags(const double* __restrict__ xyz, long n, RayFrame F, double voxel,
                                                 const unsigned long long* __restrict__ keys, uint32_t slots, uint32_t* __restrict__ flags) {
  const int lane = threadIdx.x & 63;
  const long waves = ((long)gridDim.x * blockDim.x) >> 6;
  double qo[3];
  madicp_host::export_position(F.o, F.X.R, F.X.t, qo);
  for (long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6; i < n; i += waves) {  // (wave-uniform)
    const double p[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
    double q[3], d[3];
    madicp_host::export_position(p, F.X.R, F.X.t, q);
    if (lane == 0) {
      const unsigned long long end = madicp_host::export_key(q, voxel);
      const uint32_t s = end != madicp_host::kExportNoKey ? map_find(keys, slots, end) : kExportNoSlot;
      if (s != kExportNoSlot) ray_flag(flags, s, kRayOccupied);
    }
    const double L = madicp_host::ray_length(qo, q, d);
    const int K = madicp_host::ray_sample_count(L, F.margin, voxel);
    unsigned long long carry = madicp_host::kExportNoKey;  // the key of sample k0 (lane 63 of the pass before)
    for (int k0 = 0; k0 < K; k0 += 64) {  // (wave-uniform bounds: the shuffles below see every lane)
      const int k = k0 + lane + 1;
      unsigned long long key = madicp_host::kExportNoKey;
      if (k <= K) {
        double s[3];
        madicp_host::ray_sample(qo, d, L, k, voxel, s);
        key = madicp_host::export_key(s, voxel);
      }
      unsigned long long left = __shfl_up(key, 1);
      if (lane == 0) left = carry;
      carry = __shfl(key, 63);
      if (key != madicp_host::kExportNoKey && key != left) {
        const uint32_t slot = map_find(keys, slots, key);
        if (slot != kExportNoSlot) ray_flag(flags, slot, kRayTraversed);
      }
    }
  }
}
__global__ __launch_bounds__(256) void map_clear_mark(const unsigned long long* __restrict__ row_keys, long n_rows,
                                                      const unsigned long long* __restrict__ keys, uint32_t slots,
                                                      const uint32_t* __restrict__ flags, uint32_t* __restrict__ mark) {
  for (long j = blockIdx.x * (long)blockDim.x + threadIdx.x; j <= n_rows; j += (long)gridDim.x * blockDim.x) {
    uint32_t m = 0;
    if (j < n_rows) {
      const uint32_t s = map_find(keys, slots, row_keys[j]);
      m = (s == kExportNoSlot || (flags[s] & (kRayTraversed | kRayOccupied)) != kRayTraversed) ? 1u : 0u;
    }
    mark[j] = m;  // (entry n_rows: the scan needs a terminator)
  }
}
// The mark of a clearing on an EVIDENCE map (madicp_map_create_ev), in map_clear_mark's place: one lane per row, so no two lanes
// meet on a word.  A row whose flags are exactly "traversed" is MISSED (csrc/common/export_point.h: map_evidence_miss): it loses
// `miss` in place, on the live column, and stays unless that uses its word up — the decrements hold whether or not any row leaves,
// and map_compact, behind the scan, copies the words as they are then.  ray_flags is the plain map's.
__global__ __launch_bounds__(256) void map_clear_mark_ev(const unsigned long long* __restrict__ row_keys, long n_rows,
                                                         const unsigned long long* __restrict__ keys, uint32_t slots,
                                                         const uint32_t* __restrict__ flags, uint32_t* __restrict__ ev, uint32_t miss,
                                                         uint32_t* __restrict__ mark) {
  for (long j = blockIdx.x * (long)blockDim.x + threadIdx.x; j <= n_rows; j += (long)gridDim.x * blockDim.x) {
    uint32_t m = 0;
    if (j < n_rows) {
      const uint32_t s = map_find(keys, slots, row_keys[j]);
      m = 1u;
      if (s != kExportNoSlot && (flags[s] & (kRayTraversed | kRayOccupied)) == kRayTraversed) {
        uint32_t e = ev[j];
        m = madicp_host::map_evidence_miss(&e, miss) ? 1u : 0u;
        ev[j] = e;
      }
    }
    mark[j] = m;  // (entry n_rows: the scan needs a terminator)
  }
}
// the mark of madicp_map_download_min_evidence: mark[j] = the row's word is at least min_e; mark[M] = 0, the scan's terminator
__global__ __launch_bounds__(256) void map_ev_mark(const uint32_t* __restrict__ ev, long n_rows, uint32_t min_e, uint32_t* __restrict__ mark) {
  for (long j = blockIdx.x * (long)blockDim.x + threadIdx.x; j <= n_rows; j += (long)gridDim.x * blockDim.x)
    mark[j] = (j < n_rows && ev[j] >= min_e) ? 1u : 0u;
}

// ---- querying the map: the nearest row per point of a cloud (madicp_map_query_cloud) ------------------------------------------------
// The rule is csrc/common/export_point.h's, shared with the host twin: export_cells, query_cell_key, query_d2, query_before.  The map
// is only read — the table through map_find, the slot's row, the stored float row — and the answers go to scratch of the call's own.
//   map_slot_rows    maps WITHOUT the slot_row column (plain and attribute maps): one lane per row stores j at the slot map_find
//                    returns for row_keys[j], into a transient array of the call's own; slots that hold no key are never read
//   map_query_lanes  one lane per point: reach 0 is one probe, reach 1 the 27 cells one after the other, unrolled — 27 dependent
//                    gather chains per point (key, slot's row, 12-byte row), all latency, of which the unrolled form keeps several
//                    in flight per lane.  The product's kernel for both reaches.
//   map_query_coop   -DMADICP_QUERY_COOP (a measurement aid, tools/map_query_time.py --variant): reach 1 with 32 lanes per point,
//                    two points per wavefront-step: a wavefront takes 64 consecutive points, lane l computes q and the cells of
//                    point base + l once; in step s half h (lanes 32 h .. 32 h + 31) gets the point of lane 32 h + s by shuffles,
//                    lane c < 27 of the half probes cell c, a 5-step butterfly minimum over (d2, row) runs within the half and
//                    lane 32 h + s — the point's owner — keeps it.  After at most 32 steps every lane holds its own point's
//                    answer: the per-point stores are coalesced.  A half with no point left (the cloud's last wavefront) takes
//                    part in every shuffle with the neutral (+inf, -1); loop bounds are wave-uniform.  The same bits, measured
//                    0.028 ms SLOWER per scoring query of 120 k points (profiles/map_query_time.md): the same number of
//                    wavefronts walks 32 steps of one probe each instead of 27 probes whose loads overlap — not kept as default.
// Determinism: a minimum over (d2, row) with a strict total order does not depend on how its arguments are grouped, so the
// geometry changes no bit.  Counts: per-wavefront ballots and popcounts, lane 0 adds three 64-bit integers — no float atomics.
struct QueryMap {  // by value: what the query reads of a map
  const unsigned long long* keys;
  uint32_t slots;
  const uint32_t* slot_row;  // the map's own column, or the call's transient array
  const float* xyz;
  long n_rows;
  const unsigned long long* row_keys;
  const uint32_t* attr;  // null: none asked for
  const uint32_t* ev;
};
struct QueryOut {  // by value: the call's scratch; null where a column was not asked for
  int32_t* row;
  double* d2;
  unsigned long long* keys;
  uint32_t* attr;
  uint32_t* ev;
  unsigned long long* counts;  // candidates, matched, within
};
__global__ __launch_bounds__(256) void map_slot_rows(const unsigned long long* __restrict__ row_keys, long n_rows,
                                                     const unsigned long long* __restrict__ keys, uint32_t slots,
                                                     uint32_t* __restrict__ slot_row) {
  for (long j = blockIdx.x * (long)blockDim.x + threadIdx.x; j < n_rows; j += (long)gridDim.x * blockDim.x) {
    const uint32_t s = map_find(keys, slots, row_keys[j]);
    if (s != kExportNoSlot) slot_row[s] = (uint32_t)j;
  }
}
// cell c of the neighbourhood of `cell`: (d2, row) becomes its row's where that comes before
__device__ inline void query_probe(const QueryMap& M, const double* q, const int32_t* cell, int c, double* d2, int32_t* row) {
  uint64_t key;
  if (!madicp_host::query_cell_key(cell, c, &key)) return;
  const uint32_t s = map_find(M.keys, M.slots, key);
  if (s == kExportNoSlot) return;
  const uint32_t j = M.slot_row[s];
  if ((long)j >= M.n_rows) return;  // (never: every slot that holds a key knows its row)
  const float r[3] = {M.xyz[3 * (size_t)j], M.xyz[3 * (size_t)j + 1], M.xyz[3 * (size_t)j + 2]};
  const double d = madicp_host::query_d2(q, r);
  if (madicp_host::query_before(d, (int32_t)j, *d2, *row)) {
    *d2 = d;
    *row = (int32_t)j;
  }
}
// what every lane of a wavefront ends a pass with: its point's columns (i < n) and the wavefront's three counts
__device__ inline void query_finish(long i, long n, bool candidate, double d2, int32_t row, double md2, const QueryMap& M, const QueryOut& O) {
  if (i < n) {
    if (O.row) O.row[i] = row;
    if (O.d2) O.d2[i] = d2;
    if (O.keys) O.keys[i] = row >= 0 ? M.row_keys[row] : (unsigned long long)madicp_host::kExportNoKey;
    if (O.attr) O.attr[i] = row >= 0 ? M.attr[row] : 0u;
    if (O.ev) O.ev[i] = row >= 0 ? M.ev[row] : 0u;
  }
  const bool matched = i < n && row >= 0;
  const unsigned long long a = __popcll(__ballot(i < n && candidate));
  const unsigned long long b = __popcll(__ballot(matched));
  const unsigned long long w = __popcll(__ballot(matched && d2 <= md2));
  if ((threadIdx.x & 63) == 0) {
    if (a) atomicAdd(&O.counts[0], a);
    if (b) atomicAdd(&O.counts[1], b);
    if (w) atomicAdd(&O.counts[2], w);
  }
}
__global__ __launch_bounds__(256) void map_query_lanes(const double* __restrict__ xyz, long n, ExportPose X, double voxel, int reach,
                                                       double md2, QueryMap M, QueryOut O) {
  const int lane = threadIdx.x & 63;
  // (blockDim and the stride are multiples of 64: i - lane is the wavefront's, so all its lanes leave the loop together)
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i - lane < n; i += (long)gridDim.x * blockDim.x) {
    bool candidate = false;
    double d2 = madicp_host::kQueryNoDistance;
    int32_t row = -1;
    if (i < n) {
      const double p[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
      double q[3];
      int32_t cell[3];
      madicp_host::export_position(p, X.R, X.t, q);
      candidate = madicp_host::export_cells(q, voxel, cell);
      if (candidate && reach == 0) query_probe(M, q, cell, madicp_host::kQueryOwnCell, &d2, &row);
      if (candidate && reach != 0) {
#pragma unroll
        for (int c = 0; c < madicp_host::kQueryCells; ++c) query_probe(M, q, cell, c, &d2, &row);
      }
    }
    query_finish(i, n, candidate, d2, row, md2, M, O);
  }
}
__global__ __launch_bounds__(256) void map_query_coop(const double* __restrict__ xyz, long n, ExportPose X, double voxel, double md2,
                                                      QueryMap M, QueryOut O) {
  const int lane = threadIdx.x & 63, c = lane & 31, first = lane & 32;  // first: lane 0 of this lane's half
  const long waves = ((long)gridDim.x * blockDim.x) >> 6;
  for (long base = ((((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6) << 6); base < n; base += waves << 6) {  // (wave-uniform)
    const long i = base + lane;
    int candidate = 0;
    double q[3] = {0.0, 0.0, 0.0};
    int32_t cell[3] = {0, 0, 0};
    if (i < n) {
      const double p[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
      madicp_host::export_position(p, X.R, X.t, q);
      candidate = madicp_host::export_cells(q, voxel, cell) ? 1 : 0;
    }
    double best_d2 = madicp_host::kQueryNoDistance;
    int32_t best = -1;
    const int steps = n - base < 32 ? (int)(n - base) : 32;  // (wave-uniform; the second half never holds more points than the first)
    for (int s = 0; s < steps; ++s) {
      const int owner = first + s;  // the lane whose point this half takes now: no candidate when it has none
      const int live = __shfl(candidate, owner);
      double pq[3];
      int32_t pcell[3];
      for (int k = 0; k < 3; ++k) {
        pq[k] = __shfl(q[k], owner);
        pcell[k] = __shfl(cell[k], owner);
      }
      double d2 = madicp_host::kQueryNoDistance;
      int32_t row = -1;
      if (live && c < madicp_host::kQueryCells) query_probe(M, pq, pcell, c, &d2, &row);
      for (int d = 1; d < 32; d <<= 1) {  // (lane ^ d stays within the half)
        const double od2 = __shfl_xor(d2, d);
        const int32_t orow = __shfl_xor(row, d);
        if (madicp_host::query_before(od2, orow, d2, row)) {
          d2 = od2;
          row = orow;
        }
      }
      if (c == s) {
        best_d2 = d2;
        best = row;
      }
    }
    query_finish(i, n, candidate != 0, best_d2, best, md2, M, O);
  }
}

// ---- registering a scan against the map's surfels (madicp_map_register_cloud; csrc/common/map_align.h has the rule) -----------------
// K Gauss-Newton rounds of point-to-plane terms against the surfels fe::map_surfels wrote into the call's scratch, the pose and every
// sum resident on the device:
//   map_align_pose   the caller's pose into the device pose (a launch, not a copy: nothing of the host is read later)
//   map_align_terms  one lane per point, block k covers points [256 k, 256 k + 256) — NOT a grid-stride loop: the block index fixes
//                    the position in the tree.  The pose is read from device memory; the row is the query's (query_probe); the 28
//                    terms stay in registers and align_block_sum adds them: a wavefront's xor-butterfly over 64 consecutive points
//                    is six levels of the adjacent-pair tree (fp addition commutes: both lanes of a pair get the same bits), two
//                    levels through LDS make the workgroup's row.  Counts: ballots, popcounts, integer atomics.  out_row / out_e:
//                    the linearise-only form's per-point columns, null otherwise.
//   map_align_join   the same eight levels over 256 consecutive partial rows per workgroup (a missing row is +0.0), launched until
//                    one row is left: 120 000 points are 469 rows, then 2, then 1
//   map_align_step   one wavefront: the total into LDS, solve_pose (kernels.hip.h — the product's one update step), X_{k+1} over
//                    the device pose, and the round's trace row X_k | H | b | chi2; update = 0 is the closing linearisation
// Determinism: the association of every addition is fixed by point index alone.  No float atomics.
struct AlignSurfels {  // by value: the surfel columns in the call's scratch
  const float* centroid;
  const float* normal;
  const float* eig;
  const uint32_t* count;
};
struct AlignGates {  // by value, wave-uniform
  double md2, rho, flat;
  uint32_t min_count;
  int reach;
};
__global__ __launch_bounds__(64) void map_align_pose(ExportPose X, double* __restrict__ pose) {
  if (threadIdx.x < 9) pose[threadIdx.x] = X.R[threadIdx.x];
  else if (threadIdx.x < 12) pose[threadIdx.x] = X.t[threadIdx.x - 9];
}
// eight levels of the tree over the 256 vectors a workgroup's lanes hold, in lane order, into one row (whole workgroup of 256)
__device__ __forceinline__ void align_block_sum(double (&x)[madicp_host::kAlignTerms], double* __restrict__ out_row) {
  __shared__ double s_part[4][madicp_host::kAlignTerms];
#pragma unroll
  for (int c = 0; c < madicp_host::kAlignTerms; ++c) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) x[c] = x[c] + __shfl_xor(x[c], d, 64);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int c = 0; c < madicp_host::kAlignTerms; ++c) s_part[threadIdx.x >> 6][c] = x[c];
  }
  __syncthreads();
  if (threadIdx.x < madicp_host::kAlignTerms)
    out_row[threadIdx.x] = (s_part[0][threadIdx.x] + s_part[1][threadIdx.x]) + (s_part[2][threadIdx.x] + s_part[3][threadIdx.x]);
}
__global__ __launch_bounds__(256) void map_align_terms(const double* __restrict__ xyz, long n, const double* __restrict__ pose, double voxel,
                                                       AlignGates G, QueryMap M, AlignSurfels S, double* __restrict__ partials,
                                                       unsigned long long* __restrict__ counts, int32_t* __restrict__ out_row,
                                                       double* __restrict__ out_e) {
  const long i = (long)blockIdx.x * madicp_host::kAlignBlock + threadIdx.x;
  double x[madicp_host::kAlignTerms];
#pragma unroll
  for (int c = 0; c < madicp_host::kAlignTerms; ++c) x[c] = 0.0;
  bool candidate = false, within = false, inlier = false;
  int32_t row = -1;
  if (i < n) {
    double R[9], t[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = pose[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = pose[9 + k];
    const double p[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
    double q[3], d2 = madicp_host::kQueryNoDistance, e = 0.0;
    int32_t cell[3];
    madicp_host::export_position(p, R, t, q);
    candidate = madicp_host::export_cells(q, voxel, cell);
    if (candidate && G.reach == 0) query_probe(M, q, cell, madicp_host::kQueryOwnCell, &d2, &row);
    if (candidate && G.reach != 0) {
#pragma unroll
      for (int c = 0; c < madicp_host::kQueryCells; ++c) query_probe(M, q, cell, c, &d2, &row);
    }
    within = row >= 0 && d2 <= G.md2;
    if (within) {
      const size_t j = 3 * (size_t)row;
      const float eg[3] = {S.eig[j], S.eig[j + 1], S.eig[j + 2]};
      inlier = madicp_host::align_inlier(true, S.count[row], eg, G.min_count, G.flat);
      if (inlier) {
        const float c[3] = {S.centroid[j], S.centroid[j + 1], S.centroid[j + 2]};
        const float nrm[3] = {S.normal[j], S.normal[j + 1], S.normal[j + 2]};
        e = madicp_host::align_terms(p, R, q, c, nrm, G.rho, x);
      }
    }
    if (out_row) out_row[i] = row;
    if (out_e) out_e[i] = e;
  }
  const unsigned long long a = __popcll(__ballot(candidate));
  const unsigned long long b = __popcll(__ballot(row >= 0));
  const unsigned long long w = __popcll(__ballot(within));
  const unsigned long long in = __popcll(__ballot(inlier));
  if ((threadIdx.x & 63) == 0) {
    if (a) atomicAdd(&counts[0], a);
    if (b) atomicAdd(&counts[1], b);
    if (w) atomicAdd(&counts[2], w);
    if (in) atomicAdd(&counts[3], in);
  }
  align_block_sum(x, partials + (size_t)madicp_host::kAlignTerms * blockIdx.x);
}
__global__ __launch_bounds__(256) void map_align_join(const double* __restrict__ in, long rows, double* __restrict__ out) {
  const long r = (long)blockIdx.x * madicp_host::kAlignBlock + threadIdx.x;
  double x[madicp_host::kAlignTerms];
#pragma unroll
  for (int c = 0; c < madicp_host::kAlignTerms; ++c) x[c] = r < rows ? in[(size_t)madicp_host::kAlignTerms * r + c] : 0.0;
  align_block_sum(x, out + (size_t)madicp_host::kAlignTerms * blockIdx.x);
}
__global__ __launch_bounds__(64) void map_align_step(const double* __restrict__ total_row, double* pose, int update,
                                                     double* __restrict__ trace_row) {
  __shared__ double s_total[madicp_host::kAlignTerms];
  const int lane = threadIdx.x;
  const double xk = lane < 12 ? pose[lane] : 0.0;  // (X_k, before the update goes over it)
  if (lane < madicp_host::kAlignTerms) s_total[lane] = total_row[lane];
  wave_lds_order();
  if (lane < 12) trace_row[lane] = xk;
  else if (lane < madicp_host::kAlignTraceRow) trace_row[lane] = s_total[lane - 12];
  if (update) {  // (wave-uniform)
    double X[12], Xn[12], H[36], b[6], moved[2];
#pragma unroll
    for (int k = 0; k < 12; ++k) X[k] = pose[k];
    solve_pose(s_total, X, true, Xn, H, b, moved, lane);
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < 12; ++k) pose[k] = Xn[k];
    }
  }
}

// ---- scoring many poses: the query's three counts at each of K poses (madicp_map_score_poses) ----------------------------------------
// The rule is csrc/common/export_point.h's (score_takes_part and the query's own), shared with the host twin.  map_score_poses:
//   grid       x: passes over the points that take part (one lane per point, grid-stride); y: chunks of kScoreChunk poses
//   LDS        the chunk's poses (96 B each; slots past the last pose hold zeros and are never scored) and 3 64-bit counters per pose
//   a pass     a lane loads its point ONCE and scores it at every pose of the chunk, kScorePosesPerStep<REACH> poses per step, the
//              rest one at a time (score_step<REACH, 1>); the bounds are the workgroup's, so every lane of a wavefront walks the same
//              steps and a lane past the last point takes part with "no candidate"
//   a step     the gathers of its P poses run STAGE BY STAGE, not probe by probe: first every chain's table slot is loaded (P chains
//              at reach 0; P x 9 at reach 1, one z-layer of the 27 cells at a time), then the rare collision walks, then every
//              chain's slot row, then every chain's 12-byte row — so P or 9 P independent loads are in flight per lane where
//              map_find's loop, called probe by probe, has one.  The walk of a chain is map_find's: the same slot, the same answer.
//   counts     per pose three ballots and popcounts per wavefront, lane 0 adds them to the LDS counters (64-bit integer adds:
//              nothing wraps whatever n); after the last pass one 64-bit integer global atomic per non-zero counter.  No float
//              atomics: sums of integers, the same whatever the geometry.
constexpr int kScoreChunk = 64;
template <int REACH>
struct ScoreGeometry {
  static constexpr int kPosesPerStep = REACH ? 2 : 8;
  static constexpr int kCellsPerStage = REACH ? 9 : 1;  // per pose: one z-layer of the neighbourhood, or the point's own cell
  static constexpr int kStages = REACH ? 3 : 1;
};
template <int REACH, int P>
__device__ inline void score_step(const QueryMap& M, const double* __restrict__ sp, unsigned long long* __restrict__ sc, bool have,
                                  const double* p, double voxel, double md2, int lane) {
  constexpr int C = ScoreGeometry<REACH>::kCellsPerStage, B = P * C;
  double q[P][3], best[P];
  int32_t cell[P][3], brow[P];
  bool cand[P];
#pragma unroll
  for (int u = 0; u < P; ++u) {
    madicp_host::export_position(p, sp + madicp_host::kScorePoseDoubles * u, sp + madicp_host::kScorePoseDoubles * u + 9, q[u]);
    cand[u] = madicp_host::export_cells(q[u], voxel, cell[u]) && have;
    best[u] = madicp_host::kQueryNoDistance;
    brow[u] = -1;
  }
#pragma unroll
  for (int l = 0; l < ScoreGeometry<REACH>::kStages; ++l) {
    unsigned long long seen[B];
    uint64_t key[B];
    uint32_t slot[B], row[B];
    bool live[B];
#pragma unroll
    for (int b = 0; b < B; ++b) {  // every chain's first slot: B loads in flight
      key[b] = 0;
      live[b] = cand[b / C] && madicp_host::query_cell_key(cell[b / C], REACH ? C * l + b % C : madicp_host::kQueryOwnCell, &key[b]);
      slot[b] = export_slot0(key[b], M.slots);
      seen[b] = live[b] ? M.keys[slot[b]] : (unsigned long long)madicp_host::kExportNoKey;
    }
#pragma unroll
    for (int b = 0; b < B; ++b) {  // (map_find's walk from where the first load left it: rare)
      while (seen[b] != key[b] && seen[b] != madicp_host::kExportNoKey) {
        slot[b] = (slot[b] + 1 == M.slots) ? 0u : slot[b] + 1;
        seen[b] = M.keys[slot[b]];
      }
      live[b] = live[b] && seen[b] == key[b];
    }
#pragma unroll
    for (int b = 0; b < B; ++b) {
      row[b] = live[b] ? M.slot_row[slot[b]] : 0xffffffffu;
      live[b] = live[b] && (long)row[b] < M.n_rows;  // (never false for a found key: every slot that holds a key knows its row)
    }
    float r[B][3];
#pragma unroll
    for (int b = 0; b < B; ++b) {
#pragma unroll
      for (int a = 0; a < 3; ++a) r[b][a] = live[b] ? M.xyz[3 * (size_t)row[b] + a] : 0.0f;
    }
#pragma unroll
    for (int b = 0; b < B; ++b) {
      const double d = madicp_host::query_d2(q[b / C], r[b]);
      if (live[b] && madicp_host::query_before(d, (int32_t)row[b], best[b / C], brow[b / C])) {
        best[b / C] = d;
        brow[b / C] = (int32_t)row[b];
      }
    }
  }
#pragma unroll
  for (int u = 0; u < P; ++u) {
    const bool matched = brow[u] >= 0;
    const unsigned long long a = __popcll(__ballot(cand[u]));
    const unsigned long long m = __popcll(__ballot(matched));
    const unsigned long long w = __popcll(__ballot(matched && best[u] <= md2));
    if (lane == 0) {
      if (a) atomicAdd(&sc[3 * u], a);
      if (m) atomicAdd(&sc[3 * u + 1], m);
      if (w) atomicAdd(&sc[3 * u + 2], w);
    }
  }
}
// n_take: the points that take part, (n - 1) / stride + 1; point s of them is point s * stride of the cloud
template <int REACH>
__global__ __launch_bounds__(256) void map_score_poses(const double* __restrict__ xyz, long n_take, long stride,
                                                       const double* __restrict__ poses, int n_poses, double voxel, double md2, QueryMap M,
                                                       unsigned long long* __restrict__ counts) {
  constexpr int P = ScoreGeometry<REACH>::kPosesPerStep, kD = madicp_host::kScorePoseDoubles;
  static_assert(kScoreChunk % P == 0, "a chunk is whole steps");
  __shared__ double sp[kScoreChunk * kD];
  __shared__ unsigned long long sc[kScoreChunk * 3];
  const int k0 = blockIdx.y * kScoreChunk;
  const int kc = n_poses - k0 < kScoreChunk ? n_poses - k0 : kScoreChunk;  // (>= 1: gridDim.y is ceil(n_poses / kScoreChunk))
  for (int v = threadIdx.x; v < kScoreChunk * kD; v += blockDim.x) sp[v] = v < kc * kD ? poses[(size_t)k0 * kD + v] : 0.0;
  for (int v = threadIdx.x; v < kScoreChunk * 3; v += blockDim.x) sc[v] = 0ull;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  // (blockDim and the stride are multiples of 64: s - lane is the wavefront's, so all its lanes leave the loop together)
  for (long s = blockIdx.x * (long)blockDim.x + threadIdx.x; s - lane < n_take; s += (long)gridDim.x * blockDim.x) {
    const bool have = s < n_take;
    double p[3] = {0.0, 0.0, 0.0};
    if (have) {
      const size_t i = (size_t)s * (size_t)stride;
      p[0] = xyz[3 * i];
      p[1] = xyz[3 * i + 1];
      p[2] = xyz[3 * i + 2];
    }
    int k = 0;
    for (; k + P <= kc; k += P) score_step<REACH, P>(M, sp + kD * k, sc + 3 * k, have, p, voxel, md2, lane);
    for (; k < kc; ++k) score_step<REACH, 1>(M, sp + kD * k, sc + 3 * k, have, p, voxel, md2, lane);
  }
  __syncthreads();
  for (int v = threadIdx.x; v < kc * 3; v += blockDim.x)
    if (sc[v]) atomicAdd(&counts[(size_t)k0 * 3 + v], sc[v]);
}

}  // namespace fe
}  // namespace madicp
