/* madicp_host.h — C ABI of libmadicp_host.so: the host-side (CPU) half that FEEDS the HIP path.
 * Only the MAD-tree construction lives here (it stays on the CPU in this slice — SURVEY §8 row f-1 moves it
 * to the GPU later); nearest-neighbour search and registration are in madicp_hip.h and have no CPU path.
 */
#ifndef MADICP_HOST_H
#define MADICP_HOST_H

#include <stdint.h>

#include "madicp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct madicp_host_tree madicp_host_tree;

/* MADtree constructor / build (mad_icp/src/tools/mad_tree.cpp:35-130) + getLeafs (:154-163).
 * points: (n,3) float64, NOT modified (the library works on a private copy, as the reference's by-value
 * ContainerType arguments do: pipeline.h:71, mad_tree_wrapper.h:36).  Returns NULL if n <= 0. */
madicp_host_tree* madicp_host_tree_build(const double* points, int64_t n, double b_max, double b_min,
                                         int max_parallel_level);
void madicp_host_tree_free(madicp_host_tree* t);
int32_t madicp_host_tree_num_nodes(const madicp_host_tree* t);
int32_t madicp_host_tree_num_leaves(const madicp_host_tree* t);
/* the linear node array, ready for madicp_tree_upload */
const madicp_node* madicp_host_tree_nodes(const madicp_host_tree* t);
/* node index of every leaf in getLeafs() order */
const int32_t* madicp_host_tree_leaf_nodes(const madicp_host_tree* t);
/* leaf means (L,3) in getLeafs() order — what MADicp::setMoving consumes (mad_icp.cpp:53-55, :78) */
void madicp_host_tree_leaf_means(const madicp_host_tree* t, double* out);
/* MADtree::applyTransform on the host copy (mad_tree.cpp:165-172); R row-major */
void madicp_host_tree_transform(madicp_host_tree* t, const double R[9], const double tr[3]);

/* MADicp::updateState after the adders have been joined (mad_icp.cpp:111-116): dx = LDLT(H).solve(-b),
 * X <- X * [expSO3(dx[3:6]), dx[0:3]].  H row-major 36 (lower triangle read), X: R row-major 9 + t 3, in place.
 * Host counterpart of the device-side solve; used by the staged multi-rank driver (mad_icp_amd/sharded.py). */
void madicp_host_gn_update(const double H[36], const double b[6], double X[12]);
/* det(H^-1), the keyframe weight of pipeline.cpp:223 */
double madicp_host_det_of_inverse6(const double H[36]);

/* max |mean_i - mean_0|_2 over the internal nodes with finite means — the rho2 argument of madicp_tree_upload_trusted */
double madicp_host_tree_rho2(const madicp_host_tree* t);

/* The thread budget of the host tree builder (the caller included), process-wide — what Pipeline's num_threads
 * argument sets, like the reference's omp_set_num_threads(num_threads) (pipeline.cpp:64-65). */
void madicp_host_set_threads(int n);

/* Test hook: `split` of utils.h:37-52 about the plane (mean, normal) applied to points (n,3) IN PLACE, by the
 * reference's own loop (impl 0) or by the builder's flag-driven closed form (impl 1); returns the split position
 * (first point of the right part), -1 on bad arguments.  Both must leave the same permutation. */
int64_t madicp_host_debug_partition(double* points, int64_t n, const double mean[3], const double normal[3], int impl);
/* Test hook: MADtree::build on the CALLER's buffer — points (n,3) are permuted in place exactly like the reference permutes
 * its private copy (utils.h:37-52 at every internal node, and mad_tree.cpp:76-84 at every leaf: the representative is
 * written over the leaf's first member); returns the number of leaves, -1 on bad arguments. */
int64_t madicp_host_debug_tree_points(double* points, int64_t n, double b_max, double b_min, int max_parallel_level);
/* Pipeline::deskew (mad_icp/src/odometry/pipeline.cpp:79-123) on its own, in place, output in azimuth order; poses as 12
 * doubles (R row-major, t).  route 0: the azimuth order from the task pool (unique when the azimuths are distinct), the
 * reference's serial std::sort of (azimuth, point) pairs when two of them tie; route 1: always the reference's route.
 * Returns 1 when the parallel order was used, 0 when the serial route ran, < 0 on bad arguments.  out_velocity6 (optional):
 * naive_vel of pipeline.cpp:82-86. */
int madicp_host_debug_deskew(double* points, int64_t n, const double T_prev[12], const double T_now[12], double sensor_hz, int route,
                             double* out_velocity6);
/* Motion compensation from per-point timestamps on the host (csrc/host/deskew.h: deskew_cloud_stamped — what a Pipeline
 * with the host front-end runs for computeStamped), in place, INPUT order kept: the host twin of madicp_cloud_deskew_stamped
 * (madicp_hip.h: same chunk rule, same pose table, same evaluation order — bit-equal for the same velocity).  stamps01 (n):
 * acquisition time of every point, 0 = scan start, 1 = scan end; the velocity is naive_vel of pipeline.cpp:82-86 from the two
 * poses (12 doubles each: R row-major, t).  out_velocity6, out_chunks (n, the chunk of every point): optional.  Returns 0,
 * < 0 on bad arguments (a null pointer, n < 0, sensor_hz <= 0), the buffer untouched. */
int madicp_host_deskew_stamped(double* points, const double* stamps01, int64_t n, const double T_prev[12], const double T_now[12],
                               double sensor_hz, double* out_velocity6, int32_t* out_chunks);

/* The host twin of madicp_cloud_ingest_records (madicp_hip.h: the same rules, the same per-record source
 * csrc/common/ingest_point.h, bit-equal): a driver's byte records -> the range-filtered points in input order and their stamps
 * normalised over the scan; what a Pipeline with the host front-end runs for computeRecordsStamped.  Every field is read through
 * memcpy; nothing past data[n_records * point_step) is touched.  out_xyz: room for (n_records, 3) doubles; out_stamps01: room
 * for n_records doubles (optional; not written without a time field); the first *out_n rows / values are written.
 * out_t_range (optional): the t0, t1 used.  Returns 0 — also when no record survives (*out_n = 0) — and -1 for the arguments
 * madicp_cloud_ingest_records refuses with MADICP_ERR_INVALID, nothing written. */
int madicp_host_ingest_records(const void* data, int64_t n_records, const madicp_record_layout* layout, double min_range,
                               double max_range, int kitti_correction, const double* t_range, double* out_xyz, double* out_stamps01,
                               int64_t* out_n, double out_t_range[2]);
/* The host twin of madicp_cloud_ingest_sources (madicp_hip.h: the same rules from the same per-record source, bit-equal):
 * several sensors' byte records -> one base-frame cloud, source 0's survivors first, with one set of stamps on the common
 * clock; what a Pipeline with the host front-end runs for computeSourcesStamped.  out_xyz: room for (total records, 3) doubles;
 * out_stamps01: room for that many doubles (optional; not written without a time field); out_n_per_source (n_sources values),
 * out_t_range: optional.  Nothing past data[n_records * point_step) of any source is touched.  Returns 0 — also when no record
 * survives (*out_n = 0) — and -1 for the arguments madicp_cloud_ingest_sources refuses with MADICP_ERR_INVALID, nothing
 * written. */
int madicp_host_ingest_sources(const madicp_record_source* sources, int n_sources, const double* t_range, double* out_xyz,
                               double* out_stamps01, int64_t* out_n, int64_t* out_n_per_source, double out_t_range[2]);
/* The host twin of madicp_cloud_ingest_sources_attr (madicp_hip.h: a per-point attribute — the same word per record from the same
 * csrc/common/ingest_point.h: record_attr, bit-equal): madicp_host_ingest_sources with `fields`, one per source, and the survivors'
 * words in out_attr (room for one per record of all sources; the first *out_n are written).  fields == NULL: no attribute,
 * out_attr is not written and may be null — madicp_host_ingest_sources.  -1, nothing written, as well for what
 * madicp_cloud_ingest_sources_attr refuses and for a null out_attr with fields that name an attribute. */
int madicp_host_ingest_sources_attr(const madicp_record_source* sources, int n_sources, const madicp_attr_field* fields,
                                    const double* t_range, double* out_xyz, double* out_stamps01, uint32_t* out_attr, int64_t* out_n,
                                    int64_t* out_n_per_source, double out_t_range[2]);
/* The host twin of madicp_cloud_export_f32 (madicp_hip.h: the same rule from the same per-point source
 * csrc/common/export_point.h, bit-equal): xyz (n, 3) float64, n >= 0, taken through (R row-major, t) and written as float32
 * rows, every point in cloud order (voxel == 0) or the lowest-index point of every voxel in ascending index order (voxel > 0);
 * what a Pipeline with the host front-end runs for registeredScan().  xyz is only read.  Returns MADICP_OK with the row count in
 * *out_n (0 is legal: no candidate) and rows [0, *out_n) of out_xyz written; MADICP_ERR_CAPACITY when capacity_rows is smaller
 * than the rows needed — *out_n is that number, out_xyz is not written; MADICP_ERR_INVALID, nothing written at all, for a null
 * argument, n < 0 or > 2^30, a non-finite entry of R or t, a voxel that is negative or not finite. */
int madicp_host_cloud_export_f32(const double* xyz, int64_t n, const double R[9], const double t[3], double voxel, float* out_xyz,
                                 int64_t capacity_rows, int64_t* out_n);
/* ... and of madicp_cloud_export_f32_attr: attr (n words) is the cloud's attribute column, out_attr (capacity_rows words) gets the
 * word of every row written — its owning point's.  The rows are madicp_host_cloud_export_f32's.  MADICP_ERR_INVALID as well for a
 * null attr or out_attr; on MADICP_ERR_CAPACITY neither buffer is written. */
int madicp_host_cloud_export_f32_attr(const double* xyz, const uint32_t* attr, int64_t n, const double R[9], const double t[3],
                                      double voxel, float* out_xyz, uint32_t* out_attr, int64_t capacity_rows, int64_t* out_n);
/* The host twin of the device voxel map madicp_map_* (madicp_hip.h: the same rule from the same per-point source
 * csrc/common/export_point.h, bit-equal for every sequence of folds): an append-only set of float32 rows, the first point ever
 * to fall into each voxel; what a Pipeline with the host front-end runs for setMapAccumulation().
 *   _create        voxel finite and > 0, initial_rows >= 1 (a reservation: it never shows in the result), 1 <= max_rows <= 2^30;
 *                  MADICP_ERR_INVALID otherwise, *out_map not written.
 *   _insert        folds xyz (n, 3) float64, n >= 0, only read, through (R row-major, t): *out_added rows were appended, the map
 *                  holds *out_rows.  MADICP_ERR_CAPACITY, map unchanged, when rows + n > max_rows; MADICP_ERR_INVALID, map
 *                  unchanged and nothing written, for a null argument (xyz may be null when n == 0), n < 0 or > 2^30, a
 *                  non-finite entry of R or t.
 *   _download_f32  rows [first_row, rows) into out_xyz, their number in *out_n; MADICP_ERR_CAPACITY when capacity_rows is smaller
 *                  — *out_n is the number needed, out_xyz is not written; MADICP_ERR_INVALID for a null argument or a first_row
 *                  outside [0, rows].
 *   _clear         forgets the rows, keeps the memory.   _destroy  frees everything (null: nothing).
 *   _create_attr   the same map with the attribute column (madicp_map_create_attr): every row has a 32-bit word, its owning point's.
 *   _insert_attr   _insert with the cloud's column attr (n words; null: the cloud carries none, its rows get the word 0 — what
 *                  _insert does on such a map).  On a map made without the column attr is ignored.
 *   _download_attr the words of rows [first_row, rows), _download_f32's conventions; MADICP_ERR_INVALID on a map made without
 *                  the column, out_attr not written.
 *   _prune         the twin of madicp_map_prune (madicp_hip.h has the rule): rows farther than `radius` from `center` leave, with
 *                  their keys; the kept rows close up in order.  *out_removed rows left, the map holds *out_rows, *out_watermark
 *                  is the number of kept rows among rows [0, watermark).  MADICP_ERR_INVALID, map unchanged and nothing written,
 *                  for a null argument, a non-finite center, a radius that is not finite and > 0 or whose square is not finite,
 *                  a watermark outside [0, rows].  One sequential pass.
 *   _clear_rays    the twin of madicp_map_clear_rays (madicp_hip.h has the rule): the rays from `origin` to the n points of xyz,
 *                  all taken into the map frame by (R, t), are sampled one voxel edge apart; a row leaves iff its stored key is
 *                  the key of a sample and not the key of an end point.  Answers as for _prune.  MADICP_ERR_INVALID, map
 *                  unchanged and nothing written, for a null argument (xyz may be null when n == 0), n < 0, a non-finite R, t or
 *                  origin, a margin that is not finite and >= 0, a watermark outside [0, rows].  Two sets and one pass.
 *   _track_removed / _removed_count / _take_removed / _download_keys / _download_rows
 *                  the twins of madicp_map_track_removed and its neighbours (madicp_hip.h has the rule of the removal log): on a
 *                  tracking map _prune and _clear_rays append the rows they remove from below the watermark — stored key, float
 *                  row, word — to the log, in the one stable pass; they are refused with MADICP_ERR_CAPACITY, nothing changed,
 *                  while the log holds >= max_rows entries.  Codes and "nothing written" as on the device.
 *   _create_ev / _download_evidence / _download_min_evidence
 *                  the twins of madicp_map_create_ev and its neighbours (madicp_hip.h has the rule of the evidence column): a map
 *                  with one more 32-bit word per row, 1 .. cap — a fold gives hit to the rows it creates and adds hit, once per
 *                  fold and saturating at cap, to the older rows it falls into; _clear_rays takes miss from a row it would
 *                  otherwise remove and removes it only when that uses the word up.  with_attr != 0: the attribute column as
 *                  well.  MADICP_ERR_INVALID for hit < 1, miss < 1, cap < hit, cap > 2^31 - 1, and for both downloads on a map
 *                  made without the column.  _download_min_evidence: the rows with word >= min_e in row order, out_keys /
 *                  out_attr / out_ev null where not wanted; *out_n is always their number, MADICP_ERR_CAPACITY, nothing
 *                  written, when capacity_rows is smaller.
 *   _create_mom / _download_moments / _download_surfels
 *                  the twins of madicp_map_create_mom and its neighbours (madicp_hip.h and csrc/common/voxel_moments.h have the
 *                  rule): ten 64-bit moment words per row, max_count, the same refusals and codes.  Words, centroid and count are
 *                  bit-equal to the device's; eigenvalues and normals agree to the last bits (libm against the device library).
 *                  The zero rule is the device's, one source: an eigenvalue not above 2^-24 of the largest plus
 *                  4 x 2^-52 max(S2_aa / n) is delivered as +0.0, so a voxel of identical or collinear points has eig1 == 0 and
 *                  _register's `eig1 > 0` refuses it.
 *   _query         the twin of madicp_map_query_cloud (madicp_hip.h has the rule): for each of the n points of xyz taken through
 *                  (R, t), the row with the smallest (d2, row) among the rows whose stored key is a cell of the point's
 *                  neighbourhood (reach 0: its own cell, 1: the 27 around it); out_row / out_d2 / out_keys / out_attr / out_ev
 *                  null where not wanted, out_counts = {candidates, matched, within max_dist}.  The map is only read.  The same
 *                  refusals and codes, nothing written; xyz may be null when n == 0.  Every output bit-equal to the device's.
 *   _score         the twin of madicp_map_score_poses (madicp_hip.h has the rule): _query's three counts at each of n_poses poses —
 *                  (n_poses, 12) doubles, R row-major then t — over the points i of xyz with i % stride == 0; out_counts is
 *                  n_poses x 3.  The map is only read.  The same refusals (null poses or out_counts, n_poses outside 1 .. 4096, a
 *                  non-finite entry in any pose, reach, max_dist, stride < 1), nothing written.  n == 0 is legal here (xyz may
 *                  then be null): zeros.  Every count equal to the device's.
 *   _register      the twin of madicp_map_register_cloud (madicp_hip.h and csrc/common/map_align.h have the rule): `iterations`
 *                  rounds of point-to-plane Gauss-Newton of the n points of xyz against the map's surfels — its own map_surfel of
 *                  every row, computed once per call — the same gates, terms and adjacent-pair tree sum; the step is the host's
 *                  LDLT solve and exponential.  Trace, counts, out_row / out_e (iterations == 0 only) as on the device, the same
 *                  refusals and codes, nothing written.  n == 0 is legal here (xyz may then be null): zero sums, the pose as
 *                  given.  Fed the same surfel bits the sums are bit-equal to the device's; the surfels' normals and eigenvalues
 *                  agree to the last bits only, and so do poses: within the pose contract, not to the bit.
 *   _merge_rows    the twin of madicp_map_merge_rows (madicp_hip.h and csrc/common/map_merge.h have the rule): n saved entries —
 *                  keys (n), xyz (n, 3) float32, and attr (n) / ev (n) / mom (n, 10) exactly where the map has that column, null
 *                  otherwise — merged in as ONE fold: a key the map lacks becomes a row (the lowest index that carries it, bits
 *                  copied), evidence adds and saturates, moments add under the freeze rule.  *out_added rows were appended, the
 *                  map holds *out_rows.  The same refusals and codes from the same one pass (map_merge_refusal), the map
 *                  unchanged and nothing written; n == 0 is legal (the columns may then be null) and does nothing.  Every column
 *                  bit-equal to the device's. */
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
typedef struct madicp_host_map madicp_host_map;
int madicp_host_map_create(double voxel, int64_t initial_rows, int64_t max_rows, madicp_host_map** out_map);
int madicp_host_map_insert(madicp_host_map* map, const double* xyz, int64_t n, const double R[9], const double t[3], int64_t* out_added,
                           int64_t* out_rows);
int madicp_host_map_size(const madicp_host_map* map, int64_t* out_rows);
int madicp_host_map_download_f32(const madicp_host_map* map, int64_t first_row, float* out_xyz, int64_t capacity_rows, int64_t* out_n);
int madicp_host_map_create_attr(double voxel, int64_t initial_rows, int64_t max_rows, madicp_host_map** out_map);
int madicp_host_map_insert_attr(madicp_host_map* map, const double* xyz, const uint32_t* attr, int64_t n, const double R[9],
                                const double t[3], int64_t* out_added, int64_t* out_rows);
int madicp_host_map_download_attr(const madicp_host_map* map, int64_t first_row, uint32_t* out_attr, int64_t capacity_rows, int64_t* out_n);
int madicp_host_map_prune(madicp_host_map* map, const double center[3], double radius, int64_t watermark, int64_t* out_removed,
                          int64_t* out_rows, int64_t* out_watermark);
int madicp_host_map_clear_rays(madicp_host_map* map, const double* xyz, int64_t n, const double R[9], const double t[3],
                               const double origin[3], double margin, int64_t watermark, int64_t* out_removed, int64_t* out_rows,
                               int64_t* out_watermark);
int madicp_host_map_track_removed(madicp_host_map* map, int on);
int madicp_host_map_removed_count(const madicp_host_map* map, int64_t* out_n);
int madicp_host_map_take_removed(madicp_host_map* map, uint64_t* out_keys, float* out_xyz, uint32_t* out_attr, int64_t capacity,
                                 int64_t* out_n);
int madicp_host_map_download_keys(const madicp_host_map* map, int64_t first_row, uint64_t* out_keys, int64_t capacity_rows, int64_t* out_n);
int madicp_host_map_download_rows(const madicp_host_map* map, int64_t first_row, float* out_xyz, uint64_t* out_keys, uint32_t* out_attr,
                                  int64_t capacity_rows, int64_t* out_n);
int madicp_host_map_create_ev(double voxel, int64_t initial_rows, int64_t max_rows, int with_attr, uint32_t hit, uint32_t miss, uint32_t cap,
                              madicp_host_map** out_map);
int madicp_host_map_download_evidence(const madicp_host_map* map, int64_t first_row, uint32_t* out_ev, int64_t capacity_rows, int64_t* out_n);
int madicp_host_map_download_min_evidence(const madicp_host_map* map, uint32_t min_e, float* out_xyz, uint64_t* out_keys, uint32_t* out_attr,
                                          uint32_t* out_ev, int64_t capacity_rows, int64_t* out_n);
int madicp_host_map_create_mom(double voxel, int64_t initial_rows, int64_t max_rows, int with_attr, const uint32_t evidence[3],
                               uint32_t max_count, madicp_host_map** out_map);
int madicp_host_map_download_moments(const madicp_host_map* map, int64_t first_row, uint64_t* out, int64_t capacity_rows, int64_t* out_n);
int madicp_host_map_download_surfels(const madicp_host_map* map, int64_t first_row, float* out_centroid, float* out_normal, float* out_eig,
                                     uint32_t* out_count, int64_t capacity_rows, int64_t* out_n);
int madicp_host_map_query(const madicp_host_map* map, const double* xyz, int64_t n, const double R[9], const double t[3], int reach,
                          double max_dist, int32_t* out_row, double* out_d2, uint64_t* out_keys, uint32_t* out_attr, uint32_t* out_ev,
                          int64_t capacity_points, uint64_t out_counts[3]);
int madicp_host_map_score(const madicp_host_map* map, const double* xyz, int64_t n, const double* poses, int64_t n_poses, int reach,
                          double max_dist, int64_t stride, uint64_t* out_counts);
int madicp_host_map_register(const madicp_host_map* map, const double* xyz, int64_t n, const double R[9], const double t[3],
                             const madicp_map_align_params* params, int iterations, double out_R[9], double out_t[3],
                             double* out_trace, uint64_t* out_counts, int32_t* out_row, double* out_e, int64_t capacity_points);
int madicp_host_map_merge_rows(madicp_host_map* map, double voxel, const uint64_t* keys, const float* xyz, const uint32_t* attr,
                               const uint32_t* ev, const uint64_t* mom, int64_t n, int64_t* out_added, int64_t* out_rows);
int madicp_host_map_clear(madicp_host_map* map);
void madicp_host_map_destroy(madicp_host_map* map);

/* ---- the keyframe map sharded over the ranks of a node (Pipeline::setShard, csrc/host/pipeline.h) ---- */
/* The rank that owns the keyframe of ORDINAL k — promotion order: the first scan is 0, every promotion adds 1; not the frame
 * id, which has gaps — among `world` ranks: rows of `world`, alternate rows reversed (csrc/common/keyframe_owner.h; the same
 * function as mad_icp_amd.sharded.keyframe_owner).  -1 on bad arguments (k < 0, world < 1). */
int madicp_host_keyframe_owner(int64_t k, int world);
/* The process-wide device context every host class (MADtree, MADicp, Pipeline) works on, created on first use; NULL when no
 * device is usable (madicp_last_error()).  Owned by the library: never pass it to madicp_ctx_destroy.  What a caller installs
 * the communicator of a sharded Pipeline in — madicp_comm_init / madicp_comm_init_host, madicp_p2p_export / _attach, option
 * "shard_p2p" — before Pipeline::setShard and the first compute().  Calls on it from other threads than the Pipeline's must
 * not overlap a compute() (the C ABI is not re-entrant). */
madicp_ctx* madicp_host_device_ctx(void);

/* Test hooks: the window bookkeeping of a (sharded) Pipeline on its own, no device involved (csrc/host/keyframe_ledger.h —
 * the class Pipeline pushes and evicts its keyframes by).  _create: NULL unless 0 <= rank < world and num_keyframes >= 1.
 * _promote: one keyframe promotion; *out_ordinal its ordinal, *out_evicted the ordinal the overflowing window dropped or -1;
 * returns 1 when this rank owns the promoted keyframe, 0 when not, -1 on a null ledger.  _window: the ordinals in the window,
 * oldest first, and whether this rank holds each one's tree (up to `capacity` entries written; returns the window's size).
 * _num_local: how many of them this rank holds. */
typedef struct madicp_host_ledger madicp_host_ledger;
madicp_host_ledger* madicp_host_debug_ledger_create(int rank, int world, int num_keyframes);
void madicp_host_debug_ledger_free(madicp_host_ledger* l);
int madicp_host_debug_ledger_promote(madicp_host_ledger* l, int64_t* out_ordinal, int64_t* out_evicted);
int64_t madicp_host_debug_ledger_window(const madicp_host_ledger* l, int64_t* out_ordinals, uint8_t* out_local, int64_t capacity);
int64_t madicp_host_debug_ledger_num_local(const madicp_host_ledger* l);

#ifdef __cplusplus
}
#endif
#endif /* MADICP_HOST_H */
