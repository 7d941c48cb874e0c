// Part of madicp_capi.hip (included at its end): the device front-end — scans resident in HBM (madicp_cloud_*), ingest
// and deskew, MAD-tree construction on the device (row f-1).  Everything runs on the context's copy
// stream: like a tree upload it feeds the registrations, so the front-end of scan i+1 overlaps the registration of scan i,
// and the compute stream is only made to wait (by event) where it reads the result.  The one exception is the look-ahead
// build (madicp_tree_build_begin / _end): it runs on a stream of its own, so that a registration's feed — which IS on the
// copy stream — never queues behind half a millisecond of level kernels.
//
// One host synchronisation per build: after the last level the host reads 1 KB of counters (leaf count, top size,
// rho, error flags) because the launch geometry and the buffer sizes of everything downstream need the leaf count.

namespace {

struct DevCloud {
  double* xyz = nullptr;  // (n,3)
  double* stamps = nullptr;  // (n) normalised acquisition times, the cloud's order: clouds of madicp_cloud_ingest_records only (pooled)
  uint32_t* attr = nullptr;  // (n) one 32-bit attribute word per point, the cloud's order: madicp_cloud_ingest_sources_attr / _set_attr (pooled)
  int64_t n = 0;
  hipEvent_t ready = nullptr;  // recorded on the copy stream behind whatever produced xyz
};

// the columns of one device block (../common/map_layout.h has the list and the layout): null where the block has none
struct MapCols {
  char* col[kMapColumns] = {};
  void point(char* block, const MapLayout& L) {
    for (int c = 0; c < kMapColumns; ++c) col[c] = L.has(c) ? block + L.off[c] : nullptr;
  }
  template <class T>
  T* at(MapColumn c) const { return reinterpret_cast<T*>(col[c]); }
  unsigned long long* keys() const { return at<unsigned long long>(kColKeys); }  // (slots) the table's keys, empty = all ones
  uint32_t* owner() const { return at<uint32_t>(kColOwner); }                    // (slots) fe::kMapNever / kMapSettled / contended
  unsigned long long* row_keys() const { return at<unsigned long long>(kColRowKeys); }
  float* xyz() const { return at<float>(kColXyz); }
  uint32_t* attr() const { return at<uint32_t>(kColAttr); }
  uint32_t* ev() const { return at<uint32_t>(kColEv); }
  uint32_t* slot_row() const { return at<uint32_t>(kColSlotRow); }
  uint32_t* stamp() const { return at<uint32_t>(kColStamp); }  // (slots) all ones = not hit since the wipe
  uint32_t* closed_at() const { return at<uint32_t>(kColClosedAt); }
  unsigned long long* mom() const { return at<unsigned long long>(kColMom); }
  // what fe::map_compact / fe::map_log_removed read rows from and write them to
  fe::MapRows moving() const { return {row_keys(), xyz(), attr(), ev(), mom(), closed_at()}; }
};

// a voxel map (madicp_map_*): one device block for `cap` rows and 2 cap table slots
struct DevMap : MapCols {
  double voxel = 0.0;
  int64_t max_rows = 0, cap = 0, rows = 0;  // rows: what the map holds — exact, the host reads every fold's count
  char* block = nullptr;
  bool with_attr = false;  // madicp_map_create_attr
  uint32_t slots = 0;
  // evidence (madicp_map_create_ev): the rows' words, and beside every table slot the row of its key and the number of the last
  // fold that hit it (fe::map_hit); fold_no counts the folds since the stamps were last wiped
  bool with_ev = false;
  uint32_t ev_hit = 1, ev_miss = 1, ev_cap = 1, fold_no = 0;
  // moments (madicp_map_create_mom; csrc/common/voxel_moments.h has the rule): ten 64-bit words per row and the row's freeze word —
  // the ordinal of the fold that brought it to max_count, all ones while it still takes points.  slot_row exists on these maps too.
  // ordinal counts the folds since creation or madicp_map_clear; no table wipe resets it
  bool with_mom = false;
  uint32_t mom_max_count = 0, ordinal = 0;
  // the removal log (madicp_map_track_removed): a block of its own — the map's is swapped by every prune and growth — with the
  // logged columns (map_log_layout), of which the first log_n entries are live; allocated at the first removal that can log
  bool track = false;
  char* log_block = nullptr;
  int64_t log_cap = 0, log_n = 0;
  MapCols log;
};

// grow-only scratch of the tree builder / deskew / ingest
struct FrontScratch {
  char* block = nullptr;
  size_t cap = 0;
  int64_t n_cap = 0;  // points the block was laid out for
  tb::Params P{};
  uint32_t* S = nullptr;         // (n + 1) scan result
  uint32_t* tile_sums = nullptr; // (n / 1024 + 2)
  // deskew
  double* key[2] = {nullptr, nullptr};
  uint32_t* idx[2] = {nullptr, nullptr};
  int32_t* g = nullptr;
  int32_t* tile_min = nullptr;
  double* table = nullptr;       // thresholds | poses
  char* sort_tmp = nullptr;
  size_t sort_tmp_bytes = 0;
  tb::State* h_state = nullptr;  // pinned: copy of the device State (diagnostics, big clouds)
  tb::HostLine* h_line = nullptr; // pinned: what a build publishes to the host (tb_finish_b)
  int build_seq = 0;
  bool state_stale = false;      // h_state is older than the device State
  double* h_table = nullptr;     // pinned, same layout as `table`
  hipEvent_t h_table_read = nullptr;
  // ingest of byte records: the workgroups' partial time extremes, the result block (range and survivor count, the survivors per
  // source behind them) and its pinned copy
  double* rec_part = nullptr;    // (2 * fe::kRecMaxBlocks)
  fe::SourcesResult* rec_res = nullptr;
  fe::SourcesResult* h_rec_res = nullptr;
  // a construction between its two halves (tree_build_begin_on / tree_build_end_on)
  struct InFlight {
    bool active = false;
    bool lookahead = false;  // begun by madicp_tree_build_begin: owns `cloud`
    hipStream_t s = nullptr;
    tb::Params P{};
    int64_t n = 0;
    bool chip = false;
    int chip_grid = 0, level_grid = 0, n_tiles = 0, levels_done = 0;
    int quiet_from = -1;   // levels past this one are expected to be empty (FrontScratch::last_depth + 1)
    bool use_need = false; // size the steps' launches from the previous build's HostLine::need
    int seq = 0;           // what tb_finish_b will publish (direct scan path)
    DevCloud cloud;        // look-ahead only
    // the emission enqueued behind the summary into a block sized from the previous scan's leaf count (tree_build_begin_on)
    bool pre = false;
    int pre_leaf_cap = 0;
    int pre_steps = 0;     // levels_done when it was enqueued: extra levels afterwards make it worthless
    DevTree pre_tree;
  } fly;
  int last_need[tb::kNeedSteps] = {};  // workgroups every step of the previous build had work for (HostLine::need); -1: unknown
  bool have_need = false;
  int last_leaves = 0;     // leaves of the previous build on this scratch (the next scan of the same sensor: within a few per cent)
  int last_depth = -1;     // deepest level of the previous build on this scratch (consecutive scans: the same +- 1)
  int64_t last_n = 0;      // ... and that build's point count (the hint is for consecutive scans of one sensor, not for any cloud)
};

constexpr int kDeskewTableMax = 1040;  // > CHUNKS + a few: thresholds fall below -pi after ~1024 steps

}  // namespace

// per context, so that contexts driven from different host threads share nothing
struct madicp_ctx::Front {
  std::unordered_map<int, DevCloud> clouds;
  std::unordered_map<int, DevMap> maps;
  FrontScratch scratch;
};

namespace {

madicp_ctx::Front& front_of(madicp_ctx* ctx) {
  if (!ctx->front) ctx->front = new madicp_ctx::Front();
  return *ctx->front;
}

size_t sort_temp_bytes(int64_t n);  // (defined below, needs rocPRIM)

// the builder's scratch has one owner at a time: between madicp_tree_build_begin and _end it is the look-ahead
int busy_with_lookahead(madicp_ctx* ctx) {
  if (ctx->front && ctx->front->scratch.fly.active)
    return fail(MADICP_ERR_CAPACITY, "a look-ahead tree build is in flight on this context: madicp_tree_build_end (or _cancel) first");
  return MADICP_OK;
}

// The scratch's sub-buffers for `nc` points, walked once: over a null base for the block's size, over the block for the pointers.
// (The order and the sizes fix the byte count and every sub-buffer's place in the block.)
size_t carve_scratch(FrontScratch& fs, char* base, int64_t nc) {
  const size_t n = (size_t)nc;
  const size_t slots = n / tb::kChunk + tb::kMaxBig + 8;
  size_t off = 0;
  auto carve = [&](auto*& p, size_t count) {
    using T = std::remove_reference_t<decltype(*p)>;
    p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off = align_up(off + sizeof(T) * count);
  };
  tb::Params& P = fs.P;
  carve(P.st, 1);
  carve(P.buf[0], 3 * n);
  carve(P.buf[1], 3 * n);
  carve(P.nodes, 2 * n);
  P.node_cap = static_cast<int32_t>(std::min<int64_t>(2 * nc, 0x7ffffff0));
  carve(P.q[0], n / tb::kSmallMax + 64);  // wave-regime nodes hold > kSmallMax points
  carve(P.q[1], n / tb::kSmallMax + 64);
  carve(P.team[0], n / tb::kTeamMin + 64);
  carve(P.team[1], n / tb::kTeamMin + 64);
  carve(P.big[0], tb::kMaxBig);
  carve(P.big[1], tb::kMaxBig);
  carve(P.small[0], n);
  carve(P.small[1], n);
  carve(P.leaf_start, n + 8);
  carve(fs.S, n + 8);
  carve(fs.tile_sums, n / tb::kScanTile + 8);
  P.S = fs.S;
  P.tile_sums = fs.tile_sums;
  carve(P.partLR, 18 * slots * (tb::kChipLevels + 1));
  P.part_stride = (long)(18 * slots);
  carve(P.part2, 8 * slots);
  carve(P.tab, n + 8);
  carve(P.top_ids, kTopMax);
  carve(P.top_link, kTopMax);
  carve(P.top_front, 2 + 2 * 1024);
  carve(fs.key[0], n);
  carve(fs.key[1], n);
  carve(fs.idx[0], n);
  carve(fs.idx[1], n);
  carve(fs.g, n);
  carve(fs.tile_min, n / tb::kScanTile + 8);
  carve(fs.table, kDeskewTableMax * 13);
  carve(fs.rec_part, 2 * fe::kRecMaxBlocks);
  carve(fs.rec_res, 1);
  fs.sort_tmp_bytes = sort_temp_bytes(nc);
  carve(fs.sort_tmp, fs.sort_tmp_bytes);
  return off;
}

int ensure_scratch(madicp_ctx* ctx, int64_t n, FrontScratch** out) {
  FrontScratch& fs = front_of(ctx).scratch;
  *out = &fs;
  if (!fs.h_state) {
    HIP_TRY(hipHostMalloc(&fs.h_state, sizeof(tb::State), hipHostMallocDefault));
    HIP_TRY(hipHostMalloc(&fs.h_line, sizeof(tb::HostLine), hipHostMallocDefault));
    std::memset(fs.h_line, 0, sizeof(tb::HostLine));
    HIP_TRY(hipHostMalloc(&fs.h_table, sizeof(double) * kDeskewTableMax * 13, hipHostMallocDefault));
    HIP_TRY(hipEventCreateWithFlags(&fs.h_table_read, hipEventDisableTiming));
    HIP_TRY(hipHostMalloc(&fs.h_rec_res, sizeof(fe::SourcesResult), hipHostMallocDefault));
  }
  if (n <= fs.n_cap) return MADICP_OK;
  if (fs.block) {
    HIP_TRY(hipStreamSynchronize(ctx->copy));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (ctx->build) HIP_TRY(hipStreamSynchronize(ctx->build));
    HIP_TRY(hipFree(fs.block));
    fs.block = nullptr;
    fs.cap = 0;
    fs.n_cap = 0;
  }
  const int64_t nc = n + n / 8 + 1024;  // head-room: consecutive scans differ by a few per cent
  fs.P = tb::Params{};
  const size_t bytes = carve_scratch(fs, nullptr, nc);
  HIP_TRY(hipMalloc(&fs.block, bytes));
  fs.cap = bytes;
  fs.n_cap = nc;
  carve_scratch(fs, fs.block, nc);
  return MADICP_OK;
}

void front_destroy(madicp_ctx* ctx) {  // called by madicp_ctx_destroy (streams already drained)
  if (!ctx->front) return;
  for (auto& c : ctx->front->clouds)
    if (c.second.ready) hipEventDestroy(c.second.ready);  // (the device buffers belong to the pool)
  for (auto& m : ctx->front->maps) {
    if (m.second.block) hipFree(m.second.block);
    if (m.second.log_block) hipFree(m.second.log_block);
  }
  FrontScratch& fs = ctx->front->scratch;
  if (fs.fly.pre) {  // (a construction that was begun and never ended: its pre-sized tree block goes back with the pool)
    pool_free(ctx, fs.fly.pre_tree.block, nullptr);
    fs.fly.pre = false;
  }
  if (fs.block) hipFree(fs.block);
  if (fs.h_state) hipHostFree(fs.h_state);
  if (fs.h_line) hipHostFree(fs.h_line);
  if (fs.h_table) hipHostFree(fs.h_table);
  if (fs.h_rec_res) hipHostFree(fs.h_rec_res);
  if (fs.h_table_read) hipEventDestroy(fs.h_table_read);
  delete ctx->front;
  ctx->front = nullptr;
}

DevCloud* find_cloud(madicp_ctx* ctx, int id) {
  if (!ctx->front) return nullptr;
  auto it = ctx->front->clouds.find(id);
  return it == ctx->front->clouds.end() ? nullptr : &it->second;
}

int new_cloud(madicp_ctx* ctx, int64_t n, DevCloud* out) {
  void* p = nullptr;
  RC_TRY(pool_alloc(ctx, sizeof(double) * 3 * (size_t)std::max<int64_t>(n, 1), ctx->copy, &p));
  out->xyz = static_cast<double*>(p);
  out->n = n;
  HIP_TRY(hipEventCreateWithFlags(&out->ready, hipEventDisableTiming));
  return MADICP_OK;
}

// a cloud that was allocated but never registered (an error on the way): buffer back to the pool, event destroyed
int drop_cloud(madicp_ctx* ctx, DevCloud& c, int rc) {
  EventRef after;
  if (fence_event(ctx, &after) != MADICP_OK) after = nullptr;
  pool_free(ctx, c.xyz, after);
  pool_free(ctx, c.stamps, after);
  pool_free(ctx, c.attr, after);
  if (c.ready) hipEventDestroy(c.ready);
  c = DevCloud{};
  return rc;
}
#define CLOUD_TRY(expr)                                                                                          \
  do {                                                                                                           \
    hipError_t e_ = (expr);                                                                                      \
    if (e_ != hipSuccess) return drop_cloud(ctx, c, fail(MADICP_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_))); \
  } while (0)

// the tile scan of marks[0 .. n] (entry n: the terminator) into S, its total into *d_total: three launches, nothing waited for
hipError_t scan_marks(hipStream_t s, const uint32_t* marks, int64_t n, uint32_t* S, uint32_t* tile_sums, int32_t* d_total) {
  const int tiles = map_scan_tiles((size_t)n, tb::kScanTile);
  hipLaunchKernelGGL(tb::tb_scan_tiles, dim3(tiles), dim3(256), 0, s, marks, (int)n, tile_sums);
  hipLaunchKernelGGL(tb::tb_scan_top, dim3(1), dim3(256), 0, s, tile_sums, tiles, d_total);
  hipLaunchKernelGGL(tb::tb_scan_apply, dim3(tiles), dim3(256), 0, s, marks, (int)n, (const uint32_t*)tile_sums, S);
  return hipGetLastError();
}

// dst[i] = (float)src[i] for a block of values; false as soon as a block holds a value that is not exactly a float (NaN included:
// it compares unequal to itself; -0.0 and +-inf pass and survive the round trip).  Four doubles per instruction where the host
// has AVX2 (the plain loop, two per instruction with SSE2, was slower than the copy it replaces: 95 us against 58 for a scan).
bool block_to_f32_exact_plain(const double* src, float* dst, size_t count) {
  int bad = 0;
  for (size_t i = 0; i < count; ++i) {
    const float f = static_cast<float>(src[i]);
    dst[i] = f;
    bad |= (static_cast<double>(f) != src[i]);
  }
  return bad == 0;
}
#if !defined(__HIP_DEVICE_COMPILE__) && defined(__x86_64__)
}  // namespace
#include <immintrin.h>
namespace {
__attribute__((target("avx2"))) bool block_to_f32_exact_avx2(const double* src, float* dst, size_t count) {
  __m256d bad = _mm256_setzero_pd();
  size_t i = 0;
  for (; i + 8 <= count; i += 8) {
    const __m256d x0 = _mm256_loadu_pd(src + i), x1 = _mm256_loadu_pd(src + i + 4);
    const __m128 f0 = _mm256_cvtpd_ps(x0), f1 = _mm256_cvtpd_ps(x1);
    _mm_storeu_ps(dst + i, f0);
    _mm_storeu_ps(dst + i + 4, f1);
    bad = _mm256_or_pd(bad, _mm256_or_pd(_mm256_cmp_pd(_mm256_cvtps_pd(f0), x0, _CMP_NEQ_UQ), _mm256_cmp_pd(_mm256_cvtps_pd(f1), x1, _CMP_NEQ_UQ)));
  }
  return _mm256_movemask_pd(bad) == 0 && block_to_f32_exact_plain(src + i, dst + i, count - i);
}
__attribute__((target("avx512f"))) bool block_to_f32_exact_avx512(const double* src, float* dst, size_t count) {
  __mmask8 bad = 0;
  size_t i = 0;
  for (; i + 16 <= count; i += 16) {
    const __m512d x0 = _mm512_loadu_pd(src + i), x1 = _mm512_loadu_pd(src + i + 8);
    const __m256 f0 = _mm512_cvtpd_ps(x0), f1 = _mm512_cvtpd_ps(x1);
    _mm256_storeu_ps(dst + i, f0);
    _mm256_storeu_ps(dst + i + 8, f1);
    bad |= _mm512_cmp_pd_mask(_mm512_cvtps_pd(f0), x0, _CMP_NEQ_UQ) | _mm512_cmp_pd_mask(_mm512_cvtps_pd(f1), x1, _CMP_NEQ_UQ);
  }
  return bad == 0 && block_to_f32_exact_plain(src + i, dst + i, count - i);
}
int host_simd_level() {  // 2: AVX-512F, 1: AVX2, 0: neither
  static const int level = __builtin_cpu_supports("avx512f") ? 2 : (__builtin_cpu_supports("avx2") ? 1 : 0);
  return level;
}
#else
bool block_to_f32_exact_avx2(const double* src, float* dst, size_t count) { return block_to_f32_exact_plain(src, dst, count); }
bool block_to_f32_exact_avx512(const double* src, float* dst, size_t count) { return block_to_f32_exact_plain(src, dst, count); }
int host_simd_level() { return 0; }
#endif
bool block_to_f32_exact(const double* src, float* dst, size_t count) {
  constexpr size_t kBlock = 8192;  // (a cloud of genuine doubles is found out in its first block)
  const int simd = host_simd_level();
  for (size_t b = 0; b < count; b += kBlock) {
    const size_t len = std::min(kBlock, count - b);
    const bool ok = simd == 2 ? block_to_f32_exact_avx512(src + b, dst + b, len)
                              : (simd == 1 ? block_to_f32_exact_avx2(src + b, dst + b, len) : block_to_f32_exact_plain(src + b, dst + b, len));
    if (!ok) return false;
  }
  return true;
}

// The caller's cloud (pageable host memory) -> pinned staging -> `d_xyz` on stream `s`, staged and sent in pieces: the copy
// engine moves piece k while the host stages piece k + 1.  A cloud whose coordinates are ALL exactly floats — what a sensor
// driver, a KITTI .bin or a PointCloud2 delivers, converted to double by the caller — crosses PCIe as floats (half the
// bytes, half the transfer time in front of the builder's first kernel) and is widened on the device: the same doubles, bit
// for bit.  The first value that is not a float (synthetic double-precision noise: the first point) sends the rest the plain way.
int stage_and_send_cloud(madicp_ctx* ctx, const double* xyz, int64_t n, double* d_xyz, hipStream_t s) {
  const size_t n3 = 3 * (size_t)n;
  const size_t bytes = sizeof(double) * n3;
  StagingSlots& st = ctx->staging;
  int hb = 0;
  char* stage = nullptr;
  RC_TRY(st.acquire(bytes, &hb, &stage));
  size_t done3 = 0;  // values already on their way as floats
  void* d_f32 = nullptr;
  if (ctx->opt.upload_f32 && n3 >= 4096) {
    float* hf = reinterpret_cast<float*>(stage);
    const size_t piece3 = std::max<size_t>((n3 / 2 + 3) / 4 * 4, (size_t)64 << 10);  // two pieces (half the bytes: half the pieces)
    for (size_t off = 0; off < n3; off += piece3) {
      const size_t len = std::min(piece3, n3 - off);
      if (!block_to_f32_exact(xyz + off, hf + off, len)) break;
      if (!d_f32) {  // (one device block per staging block: the event that frees the staging block is behind the widening too)
        if (st.d_f32_cap[hb] < sizeof(float) * n3) {
          if (st.d_f32[hb]) HIP_TRY(hipFree(st.d_f32[hb]));
          st.d_f32[hb] = nullptr;
          st.d_f32_cap[hb] = 0;
          const size_t cap = sizeof(float) * (n3 + n3 / 4);
          HIP_TRY(hipMalloc(&st.d_f32[hb], cap));
          st.d_f32_cap[hb] = cap;
        }
        d_f32 = st.d_f32[hb];
      }
      HIP_TRY(hipMemcpyAsync(static_cast<float*>(d_f32) + off, hf + off, sizeof(float) * len, hipMemcpyHostToDevice, s));
      done3 = off + len;
    }
    if (done3 > 0) {
      hipLaunchKernelGGL(fe::cloud_widen_f32, dim3((unsigned)((done3 / 4 + 256) / 256)), dim3(256), 0, s, (const float*)d_f32, d_xyz, (long)done3);
      HIP_TRY(hipGetLastError());
    }
    if (done3 == n3) {
      HIP_TRY(st.sent(hb, s));
      return MADICP_OK;
    }
  }
  {  // (the rest — everything, for a cloud of genuine doubles — as doubles, behind the floats' region of the staging block)
    const size_t off0 = sizeof(double) * done3;
    const size_t piece = std::max<size_t>(align_up(bytes / 4), 256 << 10);
    for (size_t off = off0; off < bytes; off += piece) {
      const size_t len = std::min(piece, bytes - off);
      std::memcpy(stage + off, reinterpret_cast<const char*>(xyz) + off, len);
      HIP_TRY(hipMemcpyAsync(reinterpret_cast<char*>(d_xyz) + off, stage + off, len, hipMemcpyHostToDevice, s));
    }
  }
  HIP_TRY(st.sent(hb, s));
  return MADICP_OK;
}

// the epilogue of everything that makes a cloud: it gets its id
int register_cloud(madicp_ctx* ctx, const DevCloud& c, int* out_id) {
  const int id = ctx->next_id++;
  front_of(ctx).clouds[id] = c;
  *out_id = id;
  return MADICP_OK;
}

// the prologue of the float32-row ingest: the rows — `bytes` of them, sent as `padded` >= bytes with the rest zero — go through
// the pinned staging into buf[0] of a scratch sized for them (a point of the scratch is 24 bytes, a KITTI record 16: wider
// records ask for a scratch laid out for proportionally more points)
int stage_records(madicp_ctx* ctx, const void* data, int64_t n_records, size_t bytes, size_t padded, FrontScratch** fs, void** d_rec) {
  RC_TRY(busy_with_lookahead(ctx));
  HIP_TRY(hipSetDevice(ctx->device));
  const int64_t n_layout = std::max<int64_t>(n_records, (int64_t)((padded + 23) / 24));
  if (n_layout > 0x3fffffff) return fail(MADICP_ERR_INVALID, "records too large");
  RC_TRY(ensure_scratch(ctx, n_layout, fs));
  int hb = 0;
  char* stage = nullptr;
  RC_TRY(ctx->staging.acquire(padded, &hb, &stage));
  std::memcpy(stage, data, bytes);
  std::memset(stage + bytes, 0, padded - bytes);
  *d_rec = (*fs)->P.buf[0];
  HIP_TRY(hipMemcpyAsync(*d_rec, stage, padded, hipMemcpyHostToDevice, ctx->copy));
  HIP_TRY(ctx->staging.sent(hb, ctx->copy));
  return MADICP_OK;
}

// Byte records -> ONE filtered base-frame cloud with one set of stamps on a common clock: the chain behind
// madicp_cloud_ingest_sources and madicp_cloud_ingest_records (kernels: fe::sources_mark, fe::records_range, fe::sources_scatter),
// for sources the caller has VALIDATED (madicp_host::record_sources_refusal).  All sources go through ONE acquisition of the
// pinned staging and ONE host-to-device copy into buf[0] of the scratch, each at a 64-byte aligned offset (a tile then starts
// 16-byte aligned whatever the steps in front of it), the gaps zeroed: the last tile of a source loads up to 3 bytes past its
// records.  Mark, scan, range, one copy of the result block, one synchronisation, scatter — whatever the number of sources.
// Sources that name an attribute field (RecordSource::A, all of them or none) give the cloud its attribute column, allocated from
// the pool beside the stamps and filled by the same scatter: no further launch.
int ingest_sources_on(madicp_ctx* ctx, const madicp_host::RecordSource* src, int n_sources, const double* t_range, int* out_cloud_id,
                      int64_t* out_n, int64_t* out_n_per_source, double out_t_range[2]) {
  // the table of the sources: where each one's bytes, tiles and records begin
  fe::SourceTable T{};
  T.n_sources = n_sources;
  T.has_time = src[0].L.t_type != madicp_host::kTimeNone ? 1 : 0;
  size_t staged = 0;  // bytes of the one copy
  for (int s = 0; s < n_sources; ++s) {
    fe::SourceEntry& E = T.src[s];
    const size_t bytes = (size_t)src[s].L.step * (size_t)src[s].n;
    E.byte_off = (long)((staged + 63) & ~(size_t)63);
    E.first_tile = T.n_tiles;
    E.first_rec = T.n_total;
    E.n = (long)src[s].n;
    E.L = src[s].L;
    E.A = src[s].A;
    E.per_tile = fe::records_per_tile(E.L.step);
    E.flags = (src[s].kitti ? fe::kSrcKitti : 0) | (madicp_host::source_extrinsic_is_identity(src[s].R, src[s].t) ? fe::kSrcIdentity : 0) |
              (madicp_host::source_clock_as_is(src[s].t_scale, src[s].t_offset) ? fe::kSrcClockAsIs : 0);
    E.min_range = src[s].min_range;
    E.max_range = src[s].max_range;
    E.t_scale = src[s].t_scale;
    E.t_offset = src[s].t_offset;
    std::memcpy(E.R, src[s].R, sizeof(E.R));
    std::memcpy(E.t, src[s].t, sizeof(E.t));
    T.n_tiles += (E.n + E.per_tile - 1) / E.per_tile;
    T.n_total += E.n;
    staged = (size_t)E.byte_off + ((bytes + 3) & ~(size_t)3);  // what the source's last tile's dword loads reach
  }
  const int64_t n_total = T.n_total;
  // (a point of the scratch is 24 bytes: wider records ask for a scratch laid out for proportionally more points)
  const int64_t n_layout = std::max<int64_t>(n_total, (int64_t)((staged + 23) / 24));
  if (n_layout > 0x3fffffff) return fail(MADICP_ERR_INVALID, "records too large");
  RC_TRY(busy_with_lookahead(ctx));
  HIP_TRY(hipSetDevice(ctx->device));
  FrontScratch* fs = nullptr;
  RC_TRY(ensure_scratch(ctx, n_layout, &fs));
  {
    int hb = 0;
    char* stage = nullptr;
    RC_TRY(ctx->staging.acquire(staged, &hb, &stage));
    size_t at = 0;
    for (int s = 0; s < n_sources; ++s) {
      const size_t bytes = (size_t)src[s].L.step * (size_t)src[s].n;
      std::memset(stage + at, 0, (size_t)T.src[s].byte_off - at);
      std::memcpy(stage + T.src[s].byte_off, src[s].data, bytes);
      at = (size_t)T.src[s].byte_off + bytes;
    }
    std::memset(stage + at, 0, staged - at);
    HIP_TRY(hipMemcpyAsync(fs->P.buf[0], stage, staged, hipMemcpyHostToDevice, ctx->copy));
    HIP_TRY(ctx->staging.sent(hb, ctx->copy));
  }
  const unsigned char* d_rec = reinterpret_cast<const unsigned char*>(fs->P.buf[0]);
  uint32_t* keep = fs->P.leaf_start;
  const int blocks = static_cast<int>(std::min<int64_t>(T.n_tiles, std::min<int64_t>((int64_t)ctx->n_cus * 8, fe::kRecMaxBlocks)));
  hipLaunchKernelGGL(fe::sources_mark, dim3(blocks), dim3(256), 0, ctx->copy, d_rec, T, keep, fs->rec_part);
  HIP_TRY(scan_marks(ctx->copy, keep, n_total, fs->S, fs->tile_sums, &fs->P.st->n_leaves));
  hipLaunchKernelGGL(fe::records_range, dim3(1), dim3(256), 0, ctx->copy, (const double*)fs->rec_part, blocks, T.has_time,
                     (T.has_time && t_range) ? 1 : 0, t_range ? t_range[0] : 0.0, t_range ? t_range[1] : 0.0,
                     (const int32_t*)&fs->P.st->n_leaves, &fs->rec_res->r);
  if (out_n_per_source)  // (the survivors per source ride in the same copy)
    hipLaunchKernelGGL(fe::sources_counts, dim3(1), dim3(64), 0, ctx->copy, T, (const uint32_t*)fs->S, fs->rec_res);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(fs->h_rec_res, fs->rec_res, out_n_per_source ? sizeof(fe::SourcesResult) : sizeof(fe::RecordsResult),
                         hipMemcpyDeviceToHost, ctx->copy));
  HIP_TRY(hipStreamSynchronize(ctx->copy));  // the size of the result decides the allocation; the range comes with it
  const int64_t kept = fs->h_rec_res->r.kept;
  if (kept < 1) return fail(MADICP_ERR_INVALID, "no point of any source survives the range filter");
  DevCloud c;
  RC_TRY(new_cloud(ctx, kept, &c));
  if (T.has_time) {
    void* p = nullptr;
    const int rc = pool_alloc(ctx, sizeof(double) * (size_t)kept, ctx->copy, &p);
    if (rc != MADICP_OK) return drop_cloud(ctx, c, rc);
    c.stamps = static_cast<double*>(p);
  }
  if (src[0].A.type != madicp_host::kAttrNone) {
    void* p = nullptr;
    const int rc = pool_alloc(ctx, sizeof(uint32_t) * (size_t)kept, ctx->copy, &p);
    if (rc != MADICP_OK) return drop_cloud(ctx, c, rc);
    c.attr = static_cast<uint32_t*>(p);
  }
  const double angle = madicp_host::ingest_kitti_angle();  // libm sin / cos like Eigen::AngleAxisd
  hipLaunchKernelGGL(fe::sources_scatter, dim3(blocks), dim3(256), 0, ctx->copy, d_rec, T, (const uint32_t*)keep, (const uint32_t*)fs->S,
                     std::sin(angle), std::cos(angle), (const fe::RecordsResult*)&fs->rec_res->r, c.xyz, c.stamps, c.attr);
  CLOUD_TRY(hipGetLastError());
  CLOUD_TRY(hipEventRecord(c.ready, ctx->copy));
  *out_n = kept;
  if (out_n_per_source)
    for (int s = 0; s < n_sources; ++s) out_n_per_source[s] = fs->h_rec_res->kept_of[s];
  if (out_t_range) {
    out_t_range[0] = fs->h_rec_res->r.t0;
    out_t_range[1] = fs->h_rec_res->r.t1;
  }
  return register_cloud(ctx, c, out_cloud_id);
}

}  // namespace

extern "C" {

int madicp_cloud_upload(madicp_ctx* ctx, const double* xyz, int64_t n, int* out_cloud_id) {
  if (!ctx || !xyz || !out_cloud_id) return fail(MADICP_ERR_INVALID, "null argument");
  if (n < 1 || n > 0x3fffffff) return fail(MADICP_ERR_INVALID, "a cloud holds 1 .. 2^30 points");
  HIP_TRY(hipSetDevice(ctx->device));
  DevCloud c;
  RC_TRY(new_cloud(ctx, n, &c));
  // pinned staging shared with the tree uploads (two buffers, alternating)
  {
    const int rc = stage_and_send_cloud(ctx, xyz, n, c.xyz, ctx->copy);
    if (rc != MADICP_OK) return drop_cloud(ctx, c, rc);
  }
  CLOUD_TRY(hipEventRecord(c.ready, ctx->copy));
  return register_cloud(ctx, c, out_cloud_id);
}

int madicp_cloud_release(madicp_ctx* ctx, int cloud_id) {
  if (!ctx) return fail(MADICP_ERR_INVALID, "ctx is null");
  DevCloud* c = find_cloud(ctx, cloud_id);
  if (!c) return fail(MADICP_ERR_INVALID, "unknown cloud id");
  HIP_TRY(hipSetDevice(ctx->device));
  EventRef after;
  RC_TRY(fence_event(ctx, &after));
  pool_free(ctx, c->xyz, after);
  pool_free(ctx, c->stamps, after);
  pool_free(ctx, c->attr, after);
  if (c->ready) hipEventDestroy(c->ready);
  ctx->front->clouds.erase(cloud_id);
  return MADICP_OK;
}

int madicp_cloud_size(madicp_ctx* ctx, int cloud_id, int64_t* out_n) {
  if (!ctx || !out_n) return fail(MADICP_ERR_INVALID, "null argument");
  DevCloud* c = find_cloud(ctx, cloud_id);
  if (!c) return fail(MADICP_ERR_INVALID, "unknown cloud id");
  *out_n = c->n;
  return MADICP_OK;
}

int madicp_cloud_download(madicp_ctx* ctx, int cloud_id, double* out_xyz, int64_t n) {
  if (!ctx || !out_xyz) return fail(MADICP_ERR_INVALID, "null argument");
  DevCloud* c = find_cloud(ctx, cloud_id);
  if (!c) return fail(MADICP_ERR_INVALID, "unknown cloud id");
  if (n != c->n) return fail(MADICP_ERR_INVALID, "n mismatch");
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipMemcpyAsync(out_xyz, c->xyz, sizeof(double) * 3 * (size_t)n, hipMemcpyDeviceToHost, ctx->copy));
  HIP_TRY(hipStreamSynchronize(ctx->copy));
  return MADICP_OK;
}

int madicp_cloud_ingest_f32(madicp_ctx* ctx, const float* records, int64_t n_records, int stride_floats, double min_range,
                            double max_range, int kitti_correction, int* out_cloud_id, int64_t* out_n) {
  if (!ctx || !records || !out_cloud_id || !out_n) return fail(MADICP_ERR_INVALID, "null argument");
  if (n_records < 1 || n_records > 0x3fffffff) return fail(MADICP_ERR_INVALID, "1 .. 2^30 records");
  if (stride_floats < 3) return fail(MADICP_ERR_INVALID, "a record holds at least x, y, z");
  FrontScratch* fs = nullptr;
  void* d_raw = nullptr;
  const size_t bytes = sizeof(float) * (size_t)stride_floats * (size_t)n_records;
  RC_TRY(stage_records(ctx, records, n_records, bytes, bytes, &fs, &d_raw));
  const float* d_rec = static_cast<const float*>(d_raw);
  uint32_t* keep = fs->P.leaf_start;
  const int blocks = grid_256(ctx, n_records);
  hipLaunchKernelGGL(fe::ingest_mark, dim3(blocks), dim3(256), 0, ctx->copy, d_rec, (long)n_records, stride_floats,
                     min_range, max_range, keep);
  HIP_TRY(scan_marks(ctx->copy, keep, n_records, fs->S, fs->tile_sums, &fs->P.st->n_leaves));
  HIP_TRY(hipMemcpyAsync(&fs->h_state->n_leaves, &fs->P.st->n_leaves, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->copy));
  HIP_TRY(hipStreamSynchronize(ctx->copy));  // the size of the result decides the allocation
  const int64_t kept = fs->h_state->n_leaves;
  if (kept < 1) return fail(MADICP_ERR_INVALID, "no point survives the range filter");
  DevCloud c;
  RC_TRY(new_cloud(ctx, kept, &c));
  const double angle = madicp_host::ingest_kitti_angle();  // libm sin / cos like Eigen::AngleAxisd
  hipLaunchKernelGGL(fe::ingest_scatter, dim3(blocks), dim3(256), 0, ctx->copy, d_rec, (long)n_records, stride_floats,
                     (const uint32_t*)keep, (const uint32_t*)fs->S, kitti_correction ? 1 : 0, std::sin(angle), std::cos(angle), c.xyz);
  CLOUD_TRY(hipGetLastError());
  CLOUD_TRY(hipEventRecord(c.ready, ctx->copy));
  *out_n = kept;
  return register_cloud(ctx, c, out_cloud_id);
}

// A driver's byte records -> a filtered cloud with its own normalised stamps (include/madicp_hip.h): the chain above for the one
// plain source, behind this entry's own refusals.
int madicp_cloud_ingest_records(madicp_ctx* ctx, const void* data, int64_t n_records, const madicp_record_layout* layout,
                                double min_range, double max_range, int kitti_correction, const double* t_range, int* out_cloud_id,
                                int64_t* out_n, double out_t_range[2]) {
  if (!ctx || !data || !layout || !out_cloud_id || !out_n) return fail(MADICP_ERR_INVALID, "null argument");
  if (n_records < 1 || n_records > 0x3fffffff) return fail(MADICP_ERR_INVALID, "1 .. 2^30 records");
  const madicp_host::RecordSource src = madicp_host::plain_source(
      data, n_records, {layout->point_step, layout->off_x, layout->off_y, layout->off_z, layout->off_t, layout->t_type}, min_range,
      max_range, kitti_correction != 0);
  if (const char* why = madicp_host::record_sources_refusal(&src, 1, t_range)) return fail(MADICP_ERR_INVALID, why);
  return ingest_sources_on(ctx, &src, 1, t_range, out_cloud_id, out_n, nullptr, out_t_range);
}

// Several sources' byte records -> one cloud (include/madicp_hip.h): the refusals, then the chain above.  `fields`: one attribute
// field per source, or null — no attribute is carried.
int madicp_cloud_ingest_sources_attr(madicp_ctx* ctx, const madicp_record_source* sources, int n_sources, const madicp_attr_field* fields,
                                     const double* t_range, int* out_cloud_id, int64_t* out_n, int64_t* out_n_per_source,
                                     double out_t_range[2]) {
  if (!ctx || !sources || !out_cloud_id || !out_n) return fail(MADICP_ERR_INVALID, "null argument");
  if (n_sources < 1 || n_sources > MADICP_MAX_SOURCES) return fail(MADICP_ERR_INVALID, "1 .. 8 sources");
  madicp_host::RecordSource src[MADICP_MAX_SOURCES];
  for (int s = 0; s < n_sources; ++s) {
    src[s] = madicp_host::record_source_of(sources[s]);
    if (fields) src[s].A = madicp_host::AttrField{fields[s].offset, fields[s].type};
  }
  if (const char* why = madicp_host::record_sources_refusal(src, n_sources, t_range)) return fail(MADICP_ERR_INVALID, why);
  return ingest_sources_on(ctx, src, n_sources, t_range, out_cloud_id, out_n, out_n_per_source, out_t_range);
}
int madicp_cloud_ingest_sources(madicp_ctx* ctx, const madicp_record_source* sources, int n_sources, const double* t_range,
                                int* out_cloud_id, int64_t* out_n, int64_t* out_n_per_source, double out_t_range[2]) {
  return madicp_cloud_ingest_sources_attr(ctx, sources, n_sources, nullptr, t_range, out_cloud_id, out_n, out_n_per_source, out_t_range);
}

// a resident cloud gets an attribute column (or its column new words): through the pinned staging, on the copy stream
int madicp_cloud_set_attr(madicp_ctx* ctx, int cloud_id, const uint32_t* attr, int64_t n) {
  if (!ctx || !attr) return fail(MADICP_ERR_INVALID, "null argument");
  DevCloud* c = find_cloud(ctx, cloud_id);
  if (!c) return fail(MADICP_ERR_INVALID, "unknown cloud id");
  if (n != c->n) return fail(MADICP_ERR_INVALID, "n mismatch: one word per point of the cloud");
  HIP_TRY(hipSetDevice(ctx->device));
  const size_t bytes = sizeof(uint32_t) * (size_t)n;
  if (!c->attr) {
    void* p = nullptr;
    RC_TRY(pool_alloc(ctx, bytes, ctx->copy, &p));
    c->attr = static_cast<uint32_t*>(p);
  }
  int hb = 0;
  char* stage = nullptr;
  RC_TRY(ctx->staging.acquire(bytes, &hb, &stage));
  std::memcpy(stage, attr, bytes);
  HIP_TRY(hipMemcpyAsync(c->attr, stage, bytes, hipMemcpyHostToDevice, ctx->copy));
  HIP_TRY(ctx->staging.sent(hb, ctx->copy));
  return MADICP_OK;
}

int madicp_cloud_attr(madicp_ctx* ctx, int cloud_id, uint32_t* out_attr, int64_t n) {
  if (!ctx || !out_attr) return fail(MADICP_ERR_INVALID, "null argument");
  DevCloud* c = find_cloud(ctx, cloud_id);
  if (!c) return fail(MADICP_ERR_INVALID, "unknown cloud id");
  if (!c->attr) return fail(MADICP_ERR_INVALID, "the cloud carries no attribute");
  if (n != c->n) return fail(MADICP_ERR_INVALID, "n mismatch");
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipMemcpyAsync(out_attr, c->attr, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost, ctx->copy));
  HIP_TRY(hipStreamSynchronize(ctx->copy));
  return MADICP_OK;
}

}  // extern "C"

// ---- deskew --------------------------------------------------------------------------------------------------------
#include <rocprim/rocprim.hpp>

namespace {
size_t sort_temp_bytes(int64_t n) {
  size_t bytes = 0;
  double* k = nullptr;
  uint32_t* v = nullptr;
  (void)rocprim::radix_sort_pairs(nullptr, bytes, k, k, v, v, (size_t)n, 0, 64, (hipStream_t) nullptr);
  return bytes + 256;
}

// The reference's running threshold and time (pipeline.cpp:99-106,109-117), tabulated with its own arithmetic (repeated
// subtraction / addition), and the pose of every chunk by the host's expSO3 (libm, like the reference): poses[12 k] =
// [expMapSO3(omega t_k) row-major | v t_k], t_0 = -1/hz, t_{k+1} = t_k + (1/hz) / 1023.  One table for both deskews: the azimuth
// walk reads thresholds and poses (`count` = kDeskewTableMax), the stamped path the first CHUNKS poses (thr = nullptr).
// Returns the number of thresholds that can still be undercut.
int deskew_table(const double velocity[6], double sensor_hz, int count, double* thr, double* poses) {
  constexpr int CHUNKS = fe::kStampChunks;  // tools/constants.h:31
  const double ts = 1. / sensor_hz;
  const double resolution = 2 * M_PI / double(CHUNKS);
  const double delta = ts / double(CHUNKS - 1);
  double angle = M_PI - resolution;
  double t = -ts;
  int n_thr = 0;
  for (int k = 0; k < count; ++k) {
    double dx[6];
    for (int i = 0; i < 6; ++i) dx[i] = velocity[i] * t;
    double* Pk = poses + 12 * k;
    {  // lie_algebra.h:39-52, with the reference's first-order branch
      const double* w = dx + 3;
      const double th2 = dotc(w[0], w[1], w[2], w[0], w[1], w[2]);
      const double th = std::sqrt(th2);
      const double W[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
      if (th2 < 1e-8) {
        for (int i = 0; i < 9; ++i) Pk[i] = ((i % 4 == 0) ? 1.0 : 0.0) + W[i];
      } else {
        double K[9], cK[9];
        const double omc = 2.0 * std::sin(th / 2.0) * std::sin(th / 2.0);
        const double s = std::sin(th);
        for (int i = 0; i < 9; ++i) {
          K[i] = W[i] / th;
          cK[i] = omc * K[i];
        }
        for (int r = 0; r < 3; ++r)
          for (int q = 0; q < 3; ++q) {
            const double kk = cK[3 * r] * K[q] + (cK[3 * r + 1] * K[3 + q] + cK[3 * r + 2] * K[6 + q]);
            Pk[3 * r + q] = (((r == q) ? 1.0 : 0.0) + s * K[3 * r + q]) + kk;
          }
      }
      Pk[9] = dx[0]; Pk[10] = dx[1]; Pk[11] = dx[2];
    }
    if (thr) thr[k] = angle;
    if (angle >= -M_PI - resolution) n_thr = k + 1;  // thresholds at or below -pi can never be undercut again
    angle -= resolution;
    t += delta;
  }
  return n_thr;
}

// an entry point's prologue once its cloud is found: the scratch, free of a look-ahead and sized for the cloud
int deskew_prologue(madicp_ctx* ctx, const DevCloud* c, double sensor_hz, FrontScratch** fs) {
  if (!(sensor_hz > 0.0)) return fail(MADICP_ERR_INVALID, "sensor_hz must be positive");
  RC_TRY(busy_with_lookahead(ctx));
  HIP_TRY(hipSetDevice(ctx->device));
  return ensure_scratch(ctx, c->n, fs);
}

// deskew_table through its pinned copy to the scratch's `table` ([kDeskewTableMax thresholds | poses], both deskews keep the
// poses in the same place): `count` poses, with the thresholds in front of them or without
int send_deskew_table(madicp_ctx* ctx, FrontScratch* fs, const double velocity[6], double sensor_hz, int count, bool thresholds, int* n_thr) {
  HIP_TRY(hipEventSynchronize(fs->h_table_read));
  *n_thr = deskew_table(velocity, sensor_hz, count, thresholds ? fs->h_table : nullptr, fs->h_table + kDeskewTableMax);
  const size_t skip = thresholds ? 0 : kDeskewTableMax;
  HIP_TRY(hipMemcpyAsync(fs->table + skip, fs->h_table + skip, sizeof(double) * (kDeskewTableMax - skip + 12 * (size_t)count),
                         hipMemcpyHostToDevice, ctx->copy));
  HIP_TRY(hipEventRecord(fs->h_table_read, ctx->copy));
  return MADICP_OK;
}

// The compensated cloud replaces the input: `launch(fresh)` enqueues the kernel that writes the points into a fresh buffer, the
// old one goes back to the pool behind it — with the cloud's stamps (`drop_stamps`) where the new order no longer lines up
// with them.  The attribute column is never dropped: a `reorders` launch gets a fresh column as well, which it fills with the
// words in the new order and which replaces the old one together with the points (null when the cloud carries none); a launch
// that keeps the input order leaves the column alone.  `out_chunks` (debugging / parity aid): the time chunk of every point,
// which the kernel left in `d_chunks`.
template <class Launch>
int replace_points(madicp_ctx* ctx, DevCloud* c, const char* what, bool reorders, int32_t* out_chunks, const int32_t* d_chunks,
                   Launch launch) {
  const bool drop_stamps = reorders;
  void* fresh = nullptr;
  RC_TRY(pool_alloc(ctx, sizeof(double) * 3 * (size_t)c->n, ctx->copy, &fresh));
  void* fresh_attr = nullptr;
  if (reorders && c->attr) {
    const int rc = pool_alloc(ctx, sizeof(uint32_t) * (size_t)c->n, ctx->copy, &fresh_attr);
    if (rc != MADICP_OK) {
      pool_free(ctx, fresh, nullptr);
      return rc;
    }
  }
  launch(static_cast<double*>(fresh), static_cast<uint32_t*>(fresh_attr));
  EventRef after;
  {  // a failure from here on must not leak the fresh buffer: the cloud keeps its old points
    const hipError_t le = hipGetLastError();
    const int frc = le == hipSuccess ? fence_event(ctx, &after) : MADICP_OK;
    if (le != hipSuccess || frc != MADICP_OK) {
      hipStreamSynchronize(ctx->copy);
      pool_free(ctx, fresh, nullptr);
      pool_free(ctx, fresh_attr, nullptr);
      return le != hipSuccess ? fail(MADICP_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(le)) : frc;
    }
  }
  pool_free(ctx, c->xyz, after);
  c->xyz = static_cast<double*>(fresh);
  if (drop_stamps) {
    pool_free(ctx, c->stamps, after);
    c->stamps = nullptr;
  }
  if (fresh_attr) {
    pool_free(ctx, c->attr, after);
    c->attr = static_cast<uint32_t*>(fresh_attr);
  }
  HIP_TRY(hipEventRecord(c->ready, ctx->copy));
  if (out_chunks) {
    HIP_TRY(hipMemcpyAsync(out_chunks, d_chunks, sizeof(int32_t) * (size_t)c->n, hipMemcpyDeviceToHost, ctx->copy));
    HIP_TRY(hipStreamSynchronize(ctx->copy));
  }
  return MADICP_OK;
}
}  // namespace

extern "C" {

int madicp_cloud_deskew(madicp_ctx* ctx, int cloud_id, const double velocity[6], double sensor_hz, int32_t* out_chunks) {
  if (!ctx || !velocity) return fail(MADICP_ERR_INVALID, "null argument");
  DevCloud* c = find_cloud(ctx, cloud_id);
  if (!c) return fail(MADICP_ERR_INVALID, "unknown cloud id");
  FrontScratch* fs = nullptr;
  RC_TRY(deskew_prologue(ctx, c, sensor_hz, &fs));
  const int64_t n = c->n;
  int n_thr = 0;
  RC_TRY(send_deskew_table(ctx, fs, velocity, sensor_hz, kDeskewTableMax, true, &n_thr));
  const int n_poses = std::min(n_thr + 1, kDeskewTableMax);
  const int blocks = grid_256(ctx, n);
  hipLaunchKernelGGL(fe::deskew_keys, dim3(blocks), dim3(256), 0, ctx->copy, (const double*)c->xyz, (long)n, fs->key[0], fs->idx[0]);
  HIP_TRY(hipGetLastError());
  size_t tmp_bytes = fs->sort_tmp_bytes;
  HIP_TRY(rocprim::radix_sort_pairs(fs->sort_tmp, tmp_bytes, fs->key[0], fs->key[1], fs->idx[0], fs->idx[1], (size_t)n, 0, 64,
                                    ctx->copy));
  hipLaunchKernelGGL(fe::deskew_targets, dim3(blocks), dim3(256), 0, ctx->copy, (const double*)fs->key[1], (long)n,
                     (const double*)fs->table, n_thr, fs->g);
  const int tiles = static_cast<int>((n + tb::kScanTile - 1) / tb::kScanTile);
  hipLaunchKernelGGL(fe::pmin_tiles, dim3(tiles), dim3(256), 0, ctx->copy, (const int32_t*)fs->g, (long)n, fs->tile_min);
  hipLaunchKernelGGL(fe::pmin_top, dim3(1), dim3(256), 0, ctx->copy, fs->tile_min, tiles);
  // (the points end up in azimuth order — the chunks, when asked for, in walk order, largest azimuth first — and stamps in
  // input order would no longer line up)
  int32_t* d_chunks = out_chunks ? reinterpret_cast<int32_t*>(fs->P.small[0]) : nullptr;
  return replace_points(ctx, c, "deskew", true, out_chunks, d_chunks, [&](double* fresh, uint32_t* fresh_attr) {
    hipLaunchKernelGGL(fe::deskew_apply, dim3(tiles), dim3(256), 0, ctx->copy, (const double*)c->xyz, (const uint32_t*)fs->idx[1], (long)n,
                       (const int32_t*)fs->g, (const int32_t*)fs->tile_min, (const double*)(fs->table + kDeskewTableMax), n_poses, fresh,
                       d_chunks);
    if (fresh_attr)  // (the sorted index is still in the scratch)
      hipLaunchKernelGGL(fe::attr_gather, dim3(blocks), dim3(256), 0, ctx->copy, (const uint32_t*)c->attr, (const uint32_t*)fs->idx[1], (long)n,
                         fresh_attr);
  });
}

}  // extern "C"

namespace {
// the second half of both stamped deskews: `d_stamps` (n, device memory, ordered on the copy stream) -> the cloud compensated
// in place of its points
int deskew_stamped_on(madicp_ctx* ctx, DevCloud* c, FrontScratch* fs, const double* d_stamps, const double velocity[6], double sensor_hz,
                      int32_t* out_chunks) {
  const int64_t n = c->n;
  int n_thr = 0;  // (this path reads no thresholds)
  RC_TRY(send_deskew_table(ctx, fs, velocity, sensor_hz, fe::kStampChunks, false, &n_thr));
  const double* d_poses = fs->table + kDeskewTableMax;
  int32_t* d_chunks = out_chunks ? reinterpret_cast<int32_t*>(fs->P.small[0]) : nullptr;  // (input order)
  const int blocks = grid_256(ctx, n);
  return replace_points(ctx, c, "deskew_stamped", false, out_chunks, d_chunks, [&](double* fresh, uint32_t*) {
    hipLaunchKernelGGL(fe::deskew_stamped, dim3(blocks), dim3(256), 0, ctx->copy, (const double*)c->xyz, d_stamps, (long)n, d_poses, fresh,
                       d_chunks);
  });
}

fe::ExportPose export_pose(const double R[9], const double t[3]) {
  fe::ExportPose X;
  std::memcpy(X.R, R, sizeof(X.R));
  std::memcpy(X.t, t, sizeof(X.t));
  return X;
}

// a voxel table (frontend.hip.h) where it lies: a map's own block, or buf[0] of the scratch for an export
struct VoxelTable {
  unsigned long long* keys;  // (slots) empty = all ones
  uint32_t* owner;           // (slots) fe::kMapNever / kMapSettled / contended
  uint32_t slots;
};
// what a fold into an evidence map needs beside the table (DevMap has the columns)
struct FoldEvidence {
  uint32_t *ev, *slot_row, *stamp;
  uint32_t fold_no, hit, cap;
};
// what a fold into a moments map needs (slot_row: the same array as FoldEvidence's where the map has both)
struct FoldMoments {
  unsigned long long* mom;
  uint32_t *closed_at, *slot_row;
  uint32_t ordinal, max_count;
};

// One fold of a resident cloud (n >= 1 points) through X into table T, on the copy stream: fe::voxel_claim, fe::voxel_mark, the
// tile scan, fe::voxel_rows — the lowest-index point of every voxel T has not settled yet, as float rows from `first_row` of `rows`
// on, in input order.  row_keys: where the rows' keys go, or null; settle: whether the rows' slots settle (a table that lives on).
// row_attr: where the rows' attribute words go (the owning point's, 0 where the cloud carries no column), or null.
// E: an evidence map's columns, or null — the fold's rows get `hit`, and fe::map_hit, behind the claim, reinforces the older rows
// the cloud falls into (no launch without it).
// Mo: a moments map's columns, or null — fe::map_moments, behind voxel_rows (every slot settled, slot_row complete, the new rows'
// words zeroed) and in front of the one wait, adds every candidate point to its row (no launch without it).
// The caller keeps T at most half full.  The per-fold scratch lives in idle parts of the builder's scratch, which the caller owns
// (busy_with_lookahead, ensure_scratch for n) and which does not grow:
//   idx[0]  slot_of[]   leaf_start  the marks   S / tile_sums  the scan   rec_res->r.kept  the scan's total
// The rows are enqueued BEHIND the scan, before the host knows the count, and they are ready when it arrives: ONE synchronisation.
int voxel_fold(madicp_ctx* ctx, FrontScratch* fs, const DevCloud* c, const fe::ExportPose& X, double voxel, VoxelTable T, bool settle,
               float* rows, int64_t first_row, unsigned long long* row_keys, uint32_t* row_attr, int64_t* out_added,
               const FoldEvidence* E = nullptr, const FoldMoments* Mo = nullptr) {
  const int64_t n = c->n;
  uint32_t* slot_of = fs->idx[0];
  uint32_t* mark = fs->P.leaf_start;
  const int blocks = grid_256(ctx, n);
  hipLaunchKernelGGL(fe::voxel_claim, dim3(blocks), dim3(256), 0, ctx->copy, (const double*)c->xyz, (long)n, X, voxel, T.keys, T.owner,
                     T.slots, slot_of);
  hipLaunchKernelGGL(fe::voxel_mark, dim3(blocks), dim3(256), 0, ctx->copy, (const uint32_t*)slot_of, (const uint32_t*)T.owner, (long)n, mark);
  if (E)  // (in front of voxel_rows: what this fold claimed is still contended, only older rows' slots are settled)
    hipLaunchKernelGGL(fe::map_hit, dim3(blocks), dim3(256), 0, ctx->copy, (const uint32_t*)slot_of, (const uint32_t*)T.owner, (long)n,
                       (const uint32_t*)E->slot_row, E->stamp, E->fold_no, E->ev, E->hit, E->cap);
  HIP_TRY(scan_marks(ctx->copy, mark, n, fs->S, fs->tile_sums, &fs->rec_res->r.kept));
  HIP_TRY(hipMemcpyAsync(&fs->h_rec_res->r.kept, &fs->rec_res->r.kept, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->copy));
  hipLaunchKernelGGL(fe::voxel_rows, dim3(blocks), dim3(256), 0, ctx->copy, (const double*)c->xyz, (long)n, X, voxel, (const uint32_t*)mark,
                     (const uint32_t*)fs->S, (const uint32_t*)(settle ? slot_of : nullptr), settle ? T.owner : nullptr, (long)first_row,
                     rows, row_keys, (const uint32_t*)c->attr, row_attr, E ? E->ev : nullptr, E ? E->hit : 0u,
                     E ? E->slot_row : (Mo ? Mo->slot_row : nullptr), Mo ? Mo->mom : nullptr, Mo ? Mo->closed_at : nullptr);
  if (Mo)
    hipLaunchKernelGGL(fe::map_moments, dim3(blocks), dim3(256), 0, ctx->copy, (const double*)c->xyz, (long)n, X, voxel,
                       (const uint32_t*)slot_of, (const uint32_t*)Mo->slot_row, Mo->mom, Mo->closed_at, Mo->ordinal, Mo->max_count);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(ctx->copy));  // the count
  *out_added = fs->h_rec_res->r.kept;
  return MADICP_OK;
}
}  // namespace

extern "C" {

// Motion compensation from the acquisition time of every point (fe::deskew_stamped): the same time model and pose table as
// above, the chunk taken from the point's own stamp.  One kernel; the cloud keeps its input order.
int madicp_cloud_deskew_stamped(madicp_ctx* ctx, int cloud_id, const double* stamps01, int64_t n, const double velocity[6],
                                double sensor_hz, int32_t* out_chunks) {
  if (!ctx || !stamps01 || !velocity) return fail(MADICP_ERR_INVALID, "null argument");
  DevCloud* c = find_cloud(ctx, cloud_id);
  if (!c) return fail(MADICP_ERR_INVALID, "unknown cloud id");
  if (n != c->n) return fail(MADICP_ERR_INVALID, "n mismatch: one stamp per point of the cloud");
  FrontScratch* fs = nullptr;
  RC_TRY(deskew_prologue(ctx, c, sensor_hz, &fs));
  // the stamps: pinned staging shared with the cloud and tree uploads -> key[0] of the scratch
  const size_t bytes = sizeof(double) * (size_t)n;
  int hb = 0;
  char* stage = nullptr;
  RC_TRY(ctx->staging.acquire(bytes, &hb, &stage));
  std::memcpy(stage, stamps01, bytes);
  double* d_stamps = fs->key[0];
  HIP_TRY(hipMemcpyAsync(d_stamps, stage, bytes, hipMemcpyHostToDevice, ctx->copy));
  HIP_TRY(ctx->staging.sent(hb, ctx->copy));
  return deskew_stamped_on(ctx, c, fs, d_stamps, velocity, sensor_hz, out_chunks);
}

// ... and from the stamps the cloud carries itself (madicp_cloud_ingest_records): nothing crosses PCIe but the pose table
int madicp_cloud_deskew_own_stamps(madicp_ctx* ctx, int cloud_id, const double velocity[6], double sensor_hz, int32_t* out_chunks) {
  if (!ctx || !velocity) return fail(MADICP_ERR_INVALID, "null argument");
  DevCloud* c = find_cloud(ctx, cloud_id);
  if (!c) return fail(MADICP_ERR_INVALID, "unknown cloud id");
  if (!c->stamps) return fail(MADICP_ERR_INVALID, "the cloud carries no stamps (madicp_cloud_ingest_records with a time field makes one that does)");
  FrontScratch* fs = nullptr;
  RC_TRY(deskew_prologue(ctx, c, sensor_hz, &fs));
  return deskew_stamped_on(ctx, c, fs, c->stamps, velocity, sensor_hz, out_chunks);
}

int madicp_cloud_stamps(madicp_ctx* ctx, int cloud_id, double* out_stamps01, int64_t n) {
  if (!ctx || !out_stamps01) return fail(MADICP_ERR_INVALID, "null argument");
  DevCloud* c = find_cloud(ctx, cloud_id);
  if (!c) return fail(MADICP_ERR_INVALID, "unknown cloud id");
  if (!c->stamps) return fail(MADICP_ERR_INVALID, "the cloud carries no stamps");
  if (n != c->n) return fail(MADICP_ERR_INVALID, "n mismatch");
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipMemcpyAsync(out_stamps01, c->stamps, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, ctx->copy));
  HIP_TRY(hipStreamSynchronize(ctx->copy));
  return MADICP_OK;
}

// A resident cloud OUT: through (R, t), as float32 rows, thinned to the lowest-index point of every voxel (include/madicp_hip.h):
// the first fold (voxel_fold) of the cloud into an empty table, nothing kept afterwards.  The cloud is only read.  Table and rows
// live in idle parts of the builder's scratch too, which this call owns like every other madicp_cloud_* call:
//   buf[0]  (24 bytes per point)  the table: 2 n 64-bit keys, behind them 2 n 32-bit owners — exactly 24 n bytes, set to all
//                                 ones by ONE memset (the empty key and the never-owned word are both all ones)
//   buf[1]  the float rows (12 of its 24 bytes per point)
//           madicp_cloud_export_f32_attr: behind the rows, in 4 of buf[1]'s 12 idle bytes per point, the rows' attribute words
// The fold writes scratch only, so a refusal for capacity still leaves out_xyz alone.  Two synchronisations: the count, then the
// rows (voxel == 0: no table, every point a row, the count is the cloud's size — one).
}  // extern "C"
namespace {
int cloud_export_on(madicp_ctx* ctx, int cloud_id, const double R[9], const double t[3], double voxel, float* out_xyz, bool want_attr,
                    uint32_t* out_attr, int64_t capacity_rows, int64_t* out_n) {
  if (!ctx || !R || !t || !out_xyz || !out_n || (want_attr && !out_attr)) return fail(MADICP_ERR_INVALID, "null argument");
  DevCloud* c = find_cloud(ctx, cloud_id);
  if (!c) return fail(MADICP_ERR_INVALID, "unknown cloud id");
  if (want_attr && !c->attr) return fail(MADICP_ERR_INVALID, "the cloud carries no attribute");
  if (const char* why = madicp_host::export_refusal(R, t, voxel)) return fail(MADICP_ERR_INVALID, why);
  RC_TRY(busy_with_lookahead(ctx));
  const int64_t n = c->n;
  if (voxel == 0.0 && capacity_rows < n) {
    *out_n = n;
    return fail(MADICP_ERR_CAPACITY, "out_xyz holds fewer rows than the cloud has points");
  }
  HIP_TRY(hipSetDevice(ctx->device));
  FrontScratch* fs = nullptr;
  RC_TRY(ensure_scratch(ctx, n, &fs));
  const fe::ExportPose X = export_pose(R, t);
  float* d_rows = reinterpret_cast<float*>(fs->P.buf[1]);
  uint32_t* d_row_attr = want_attr ? reinterpret_cast<uint32_t*>(d_rows + 3 * n) : nullptr;
  int64_t rows = n;
  if (voxel == 0.0) {
    hipLaunchKernelGGL(fe::voxel_rows, dim3(grid_256(ctx, n)), dim3(256), 0, ctx->copy, (const double*)c->xyz, (long)n, X, voxel,
                       (const uint32_t*)nullptr, (const uint32_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr, 0L, d_rows,
                       (unsigned long long*)nullptr, (const uint32_t*)c->attr, d_row_attr, (uint32_t*)nullptr, 0u, (uint32_t*)nullptr,
                       (unsigned long long*)nullptr, (uint32_t*)nullptr);
    HIP_TRY(hipGetLastError());
  } else {
    VoxelTable T;
    T.slots = static_cast<uint32_t>(2 * n);  // (n <= 2^30)
    T.keys = reinterpret_cast<unsigned long long*>(fs->P.buf[0]);
    T.owner = reinterpret_cast<uint32_t*>(T.keys + T.slots);
    HIP_TRY(hipMemsetAsync(T.keys, 0xff, (sizeof(unsigned long long) + sizeof(uint32_t)) * (size_t)T.slots, ctx->copy));
    RC_TRY(voxel_fold(ctx, fs, c, X, voxel, T, false, d_rows, 0, nullptr, d_row_attr, &rows));
    *out_n = rows;  // the count decides whether the caller's buffer is large enough
    if (capacity_rows < rows) return fail(MADICP_ERR_CAPACITY, "out_xyz holds fewer rows than the export needs (*out_n)");
    if (rows == 0) return MADICP_OK;  // (no candidate: every point outside the 2^21 cells per axis, or not finite)
  }
  HIP_TRY(hipMemcpyAsync(out_xyz, d_rows, sizeof(float) * 3 * (size_t)rows, hipMemcpyDeviceToHost, ctx->copy));
  if (want_attr) HIP_TRY(hipMemcpyAsync(out_attr, d_row_attr, sizeof(uint32_t) * (size_t)rows, hipMemcpyDeviceToHost, ctx->copy));
  HIP_TRY(hipStreamSynchronize(ctx->copy));
  *out_n = rows;
  return MADICP_OK;
}
}  // namespace
extern "C" {
int madicp_cloud_export_f32(madicp_ctx* ctx, int cloud_id, const double R[9], const double t[3], double voxel, float* out_xyz,
                            int64_t capacity_rows, int64_t* out_n) {
  return cloud_export_on(ctx, cloud_id, R, t, voxel, out_xyz, false, nullptr, capacity_rows, out_n);
}
// ... with the attribute word of every row beside it (the cloud must carry a column)
int madicp_cloud_export_f32_attr(madicp_ctx* ctx, int cloud_id, const double R[9], const double t[3], double voxel, float* out_xyz,
                                 uint32_t* out_attr, int64_t capacity_rows, int64_t* out_n) {
  return cloud_export_on(ctx, cloud_id, R, t, voxel, out_xyz, true, out_attr, capacity_rows, out_n);
}

}  // extern "C"

// ---- the voxel map: registered scans accumulated on the device (include/madicp_hip.h: madicp_map_*) ---------------------------------
// Every insert is one voxel_fold into a table that persists; fe::map_rehash refills it at a growth (frontend.hip.h has the rule and
// the determinism argument).  A map owns ONE device block laid out for `cap` rows and 2 cap table slots: ../common/map_layout.h has
// the columns, their order and the bytes per row of capacity.
// Growth invariant: before a fold of n points into M rows, M + n <= cap — so the table is never more than half full and every
// probe ends; where it would not hold, a block for max(M + n, min(2 cap, max_rows)) rows is allocated, the row columns move by device
// copy, map_rehash refills the table, the old block is freed.  The host knows M exactly: every fold ends with ONE synchronisation,
// for the count (none more at a growth but the one in front of freeing the old block).  A fold uses the builder's scratch: it is
// refused with MADICP_ERR_CAPACITY while a look-ahead build is in flight.  Everything runs on the copy stream.
namespace {

// the ONE memset that empties the table; on an evidence map a second one for the slots' fold stamps, and the folds count from 0 again
hipError_t map_stamp_wipe(madicp_ctx* ctx, DevMap* m) {
  m->fold_no = 0;
  return hipMemsetAsync(m->stamp(), 0xff, sizeof(uint32_t) * (size_t)m->slots, ctx->copy);
}
hipError_t map_table_wipe(madicp_ctx* ctx, DevMap* m) {
  hipError_t e = hipMemsetAsync(m->block, 0xff, kMapTableBytesPerRow * (size_t)m->cap, ctx->copy);
  if (e == hipSuccess && m->with_ev) e = map_stamp_wipe(ctx, m);
  return e;
}

int map_block_alloc(madicp_ctx* ctx, int64_t cap, DevMap* m, bool wipe = true) {
  const MapLayout L = map_layout((size_t)cap, m->with_attr, m->with_ev, m->with_mom);
  char* block = nullptr;
  HIP_TRY(hipMalloc(&block, L.bytes));
  m->block = block;
  m->cap = cap;
  m->slots = static_cast<uint32_t>(2 * cap);
  m->point(block, L);
  hipError_t e = wipe ? map_table_wipe(ctx, m) : hipSuccess;  // (a prune wipes the table itself, later)
  if (e != hipSuccess) {
    hipFree(block);
    *m = DevMap{};
    return fail(MADICP_ERR_DEVICE, std::string("hipMemsetAsync: ") + hipGetErrorString(e));
  }
  return MADICP_OK;
}

// the first n entries of the row columns that src and dst both have, device to device on the copy stream
hipError_t map_move_rows(madicp_ctx* ctx, const MapCols& dst, const MapCols& src, size_t n) {
  hipError_t e = hipSuccess;
  for (int c = 0; c < kMapColumns && e == hipSuccess; ++c)
    if (kMapColumnTable[c].row && src.col[c] && dst.col[c])
      e = hipMemcpyAsync(dst.col[c], src.col[c], kMapColumnTable[c].bytes() * n, hipMemcpyDeviceToDevice, ctx->copy);
  return e;
}

// Device-to-host copies on the copy stream behind whatever is enqueued (e: its error so far), each only where the caller gave a
// buffer, then the ONE wait — which an earlier error does not spare: nothing may be in flight into the caller's buffers
struct CopyOut {
  void* dst;  // null: not asked for
  const void* src;
  size_t bytes;
};
int copies_then_wait(madicp_ctx* ctx, hipError_t e, const CopyOut* list, int count, const char* what) {
  for (int i = 0; i < count && e == hipSuccess; ++i)
    if (list[i].dst) e = hipMemcpyAsync(list[i].dst, list[i].src, list[i].bytes, hipMemcpyDeviceToHost, ctx->copy);
  const hipError_t w = hipStreamSynchronize(ctx->copy);
  if (e == hipSuccess) e = w;
  return e == hipSuccess ? MADICP_OK : fail(MADICP_ERR_DEVICE, std::string(what) + hipGetErrorString(e));
}
// ... of `n` rows from row `first` on of every column `out` has a buffer for
int map_rows_out(madicp_ctx* ctx, const MapCols& src, const MapCols& out, int64_t first, int64_t n, const char* what) {
  CopyOut list[kMapColumns];
  int count = 0;
  for (int c = 0; c < kMapColumns; ++c)
    if (out.col[c]) list[count++] = {out.col[c], src.col[c] + kMapColumnTable[c].bytes() * (size_t)first, kMapColumnTable[c].bytes() * (size_t)n};
  return copies_then_wait(ctx, hipSuccess, list, count, what);
}
// the caller's buffers of a download, by column (null: not asked for)
MapCols map_out(void* xyz, void* keys, void* attr, void* ev = nullptr, void* mom = nullptr) {
  MapCols o;
  o.col[kColXyz] = static_cast<char*>(xyz);
  o.col[kColRowKeys] = static_cast<char*>(keys);
  o.col[kColAttr] = static_cast<char*>(attr);
  o.col[kColEv] = static_cast<char*>(ev);
  o.col[kColMom] = static_cast<char*>(mom);
  return o;
}

// a block that holds `need` rows (<= max_rows): the rows move, the table is refilled from their keys
int map_grow(madicp_ctx* ctx, DevMap* m, int64_t need) {
  DevMap g = *m;
  RC_TRY(map_block_alloc(ctx, std::max(need, std::min(2 * m->cap, m->max_rows)), &g));
  hipError_t e = hipSuccess;
  if (m->rows > 0) {
    e = map_move_rows(ctx, g, *m, (size_t)m->rows);
    if (e == hipSuccess) {
      const int blocks = grid_256(ctx, m->rows);
      hipLaunchKernelGGL(fe::map_rehash, dim3(blocks), dim3(256), 0, ctx->copy, (const unsigned long long*)g.row_keys(), (long)m->rows,
                         g.keys(), g.owner(), g.slots, g.slot_row());
      e = hipGetLastError();
    }
  }
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->copy);  // (the old block is read until here)
  if (e != hipSuccess) {
    hipFree(g.block);
    return fail(MADICP_ERR_DEVICE, std::string("voxel map growth: ") + hipGetErrorString(e));
  }
  hipFree(m->block);
  *m = g;
  return MADICP_OK;
}

// Memory for `need` log entries in front of a removal on a tracking map: a block for max(need, min(2 log_cap, 2 max_rows)) entries, the
// live entries moved by device copy on the copy stream.  The block it replaces is handed back in *old_block: the caller frees it
// behind the removal's own one wait (map_log_settle), so a log growth adds no synchronisation.  log_n is not touched.
int map_log_reserve(madicp_ctx* ctx, DevMap* m, int64_t need, char** old_block) {
  *old_block = nullptr;
  if (need <= m->log_cap) return MADICP_OK;
  const int64_t log_cap = std::max(need, std::min(2 * m->log_cap, 2 * m->max_rows));
  const MapLayout L = map_log_layout((size_t)log_cap, m->with_attr);
  char* block = nullptr;
  HIP_TRY(hipMalloc(&block, L.bytes));
  MapCols g;
  g.point(block, L);
  const hipError_t e = m->log_n > 0 ? map_move_rows(ctx, g, m->log, (size_t)m->log_n) : hipSuccess;
  if (e != hipSuccess) {
    hipStreamSynchronize(ctx->copy);
    hipFree(block);
    return fail(MADICP_ERR_DEVICE, std::string("voxel map removal log: ") + hipGetErrorString(e));
  }
  *old_block = m->log_block;
  m->log_block = block;
  m->log_cap = log_cap;
  m->log = g;
  return MADICP_OK;
}

// behind a removal (rc: what it returned, logged: the entries it added): the replaced log block is freed — behind the removal's
// wait; an error may have returned in front of it — and the log's length moves only on success
void map_log_settle(madicp_ctx* ctx, DevMap* m, char* old_block, int rc, int64_t logged) {
  if (old_block) {
    if (rc != MADICP_OK) hipStreamSynchronize(ctx->copy);
    hipFree(old_block);
  }
  if (rc == MADICP_OK && m->track) m->log_n += logged;
}

// The tail every removal shares (madicp_map_prune, madicp_map_clear_rays).  The caller has allocated the FRESH block g of the same
// capacity — the shape of a growth, and its transient cost: one more block — and enqueued the kernel that leaves mark[0 .. M] in g's
// table region (not yet a table; W: where the removal's scratch lies in it, map_layout.h); here: the tile scan of the marks into S,
// map_compact into g, which leaves {rows kept, kept below the watermark} over the first two marks, which nobody reads after the
// scan: ONE small copy, ONE synchronisation.
// Behind it nothing reads the old block any more: it is freed, the table wiped and refilled from the kept keys on the stream, in
// front of whatever fold comes next.  Nothing removed: the fresh block is dropped, the map is not touched at all.
// A tracking map (the caller has ensured its log, map_log_reserve) has map_log_removed beside map_compact: behind the scan, in front
// of the one wait and of the wipe.  It reads S and the old block only — in the clearing path S lies over the dead ray flags, and
// map_compact leaves its answers over the first marks — and writes the log; the caller moves log_n (map_log_settle).
int map_remove_marked(madicp_ctx* ctx, DevMap* m, DevMap& g, const MapScratch& W, int64_t watermark, const char* what, int64_t* out_kept,
                      int64_t* out_watermark) {
  const int64_t M = m->rows;
  uint32_t* mark = reinterpret_cast<uint32_t*>(g.block + W.mark);
  uint32_t* S = reinterpret_cast<uint32_t*>(g.block + W.S);
  hipError_t e = scan_marks(ctx->copy, mark, M, S, reinterpret_cast<uint32_t*>(g.block + W.tile_sums), reinterpret_cast<int32_t*>(g.block + W.total));
  hipLaunchKernelGGL(fe::map_compact, dim3(grid_256(ctx, M + 1)), dim3(256), 0, ctx->copy, (const uint32_t*)S, (long)M, (long)watermark,
                     m->moving(), g.moving(), mark);
  if (const int64_t below = std::min(watermark, M); m->track && below > 0)
    hipLaunchKernelGGL(fe::map_log_removed, dim3(grid_256(ctx, below)), dim3(256), 0, ctx->copy, (const uint32_t*)S, (long)below, (long)m->log_n,
                       m->moving(), m->log.moving());
  uint32_t res[2] = {0, 0};
  if (e == hipSuccess) e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(res, mark, sizeof(res), hipMemcpyDeviceToHost, ctx->copy);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->copy);  // the counts (the old block is read until here)
  const int64_t kept = res[0];
  if (e == hipSuccess && kept < M) {
    e = map_table_wipe(ctx, &g);
    if (e == hipSuccess && kept > 0) {
      hipLaunchKernelGGL(fe::map_rehash, dim3(grid_256(ctx, kept)), dim3(256), 0, ctx->copy, (const unsigned long long*)g.row_keys(), (long)kept,
                         g.keys(), g.owner(), g.slots, g.slot_row());
      e = hipGetLastError();
    }
  }
  if (e != hipSuccess || kept == M) {
    if (e != hipSuccess) hipStreamSynchronize(ctx->copy);
    hipFree(g.block);
    if (e != hipSuccess) return fail(MADICP_ERR_DEVICE, std::string(what) + hipGetErrorString(e));
  } else {
    hipFree(m->block);
    g.rows = kept;
    *m = g;
  }
  *out_kept = kept;
  *out_watermark = res[1];
  return MADICP_OK;
}

// The rows of *m that stay within sphere Q.  The fresh block's table region holds the prune's scratch (map_prune_scratch) until the
// memset that makes it a table; the builder's scratch (sized by the largest CLOUD) is not touched.
int map_prune_on(madicp_ctx* ctx, DevMap* m, const fe::PruneSphere& Q, int64_t watermark, int64_t* out_kept, int64_t* out_watermark) {
  const int64_t M = m->rows;
  DevMap g = *m;
  RC_TRY(map_block_alloc(ctx, m->cap, &g, false));
  const MapScratch W = map_prune_scratch((size_t)m->cap, (size_t)M, tb::kScanTile);
  hipLaunchKernelGGL(fe::map_prune_mark, dim3(grid_256(ctx, M + 1)), dim3(256), 0, ctx->copy, (const float*)m->xyz(), (long)M, Q,
                     reinterpret_cast<uint32_t*>(g.block + W.mark));
  return map_remove_marked(ctx, m, g, W, watermark, "voxel map prune: ", out_kept, out_watermark);
}

// The rows of *m that the rays of cloud c do not clear.  The fresh block's table region holds the clearing's scratch
// (map_clear_scratch: the flags, one per slot of the LIVE table, zeroed by the one memset, and S over them once they are dead) until
// the memset that makes it a table.  The live table is only read; the builder's scratch is not touched.
int map_clear_rays_on(madicp_ctx* ctx, DevMap* m, const DevCloud* c, const fe::RayFrame& F, int64_t watermark, int64_t* out_kept,
                      int64_t* out_watermark) {
  const int64_t M = m->rows;
  DevMap g = *m;
  RC_TRY(map_block_alloc(ctx, m->cap, &g, false));
  const MapScratch W = map_clear_scratch((size_t)m->cap, (size_t)M, tb::kScanTile);
  uint32_t* flags = reinterpret_cast<uint32_t*>(g.block + W.flags);
  uint32_t* mark = reinterpret_cast<uint32_t*>(g.block + W.mark);
  const hipError_t e = hipMemsetAsync(flags, 0, sizeof(uint32_t) * (size_t)m->slots, ctx->copy);
  if (e != hipSuccess) {
    hipFree(g.block);
    return fail(MADICP_ERR_DEVICE, std::string("voxel map clearing: ") + hipGetErrorString(e));
  }
  hipLaunchKernelGGL(fe::ray_flags, dim3(grid_256(ctx, 64 * c->n)), dim3(256), 0, ctx->copy, (const double*)c->xyz, (long)c->n, F, m->voxel,
                     (const unsigned long long*)m->keys(), m->slots, flags);
  if (m->with_ev)  // (the misses, in place on the live column: they hold whether or not a row leaves)
    hipLaunchKernelGGL(fe::map_clear_mark_ev, dim3(grid_256(ctx, M + 1)), dim3(256), 0, ctx->copy, (const unsigned long long*)m->row_keys(),
                       (long)M, (const unsigned long long*)m->keys(), m->slots, (const uint32_t*)flags, m->ev(), m->ev_miss, mark);
  else
    hipLaunchKernelGGL(fe::map_clear_mark, dim3(grid_256(ctx, M + 1)), dim3(256), 0, ctx->copy, (const unsigned long long*)m->row_keys(), (long)M,
                       (const unsigned long long*)m->keys(), m->slots, (const uint32_t*)flags, mark);
  return map_remove_marked(ctx, m, g, W, watermark, "voxel map clearing: ", out_kept, out_watermark);
}

constexpr const char* kMapNoAttr = "the map was made without the attribute column (madicp_map_create_attr makes one with it)";
constexpr const char* kMapLogFull = "the map's removal log holds max_rows entries or more (madicp_map_take_removed empties it)";
constexpr const char* kMapNoMoments = "the map was made without the moments (madicp_map_create_mom makes one with them)";
constexpr const char* kMapNoEvidence = "the map was made without the evidence column (madicp_map_create_ev makes one with it)";

DevMap* find_map(madicp_ctx* ctx, int id) {
  if (!ctx->front) return nullptr;
  auto it = ctx->front->maps.find(id);
  return it == ctx->front->maps.end() ? nullptr : &it->second;
}

int map_create_on(madicp_ctx* ctx, double voxel, int64_t initial_rows, int64_t max_rows, bool with_attr, int* out_map_id,
                  const uint32_t* evidence = nullptr /* {hit, miss, cap} */, const uint32_t* max_count = nullptr /* moments */) {
  if (!ctx || !out_map_id) return fail(MADICP_ERR_INVALID, "null argument");
  if (const char* why = madicp_host::map_create_refusal(voxel, initial_rows, max_rows)) return fail(MADICP_ERR_INVALID, why);
  if (evidence)
    if (const char* why = madicp_host::map_evidence_refusal(evidence[0], evidence[1], evidence[2])) return fail(MADICP_ERR_INVALID, why);
  if (max_count)
    if (const char* why = madicp_host::map_moments_refusal(*max_count)) return fail(MADICP_ERR_INVALID, why);
  HIP_TRY(hipSetDevice(ctx->device));
  DevMap m;
  m.voxel = voxel;
  if (max_count) {
    m.with_mom = true;
    m.mom_max_count = *max_count;
  }
  m.max_rows = max_rows;
  m.with_attr = with_attr;
  if (evidence) {
    m.with_ev = true;
    m.ev_hit = evidence[0];
    m.ev_miss = evidence[1];
    m.ev_cap = evidence[2];
  }
  RC_TRY(map_block_alloc(ctx, std::min(initial_rows, max_rows), &m));
  const int id = ctx->next_id++;
  front_of(ctx).maps[id] = m;
  *out_map_id = id;
  return MADICP_OK;
}

// What every window download starts with, in this order of refusals: a null argument (out: the one buffer the call cannot do
// without), an unknown map, a column the map lacks (need; kColXyz: none), first_row outside [0, rows]; then *out_n is the window's
// rows, and a buffer too small for them is refused with `short_buffer`, which names the caller's buffers.  *rows: what is left to
// copy — 0: the call is over.
int map_window(madicp_ctx* ctx, int map_id, MapColumn need, int64_t first_row, const void* out, int64_t capacity_rows, const char* short_buffer,
               int64_t* out_n, DevMap** m, int64_t* rows) {
  *rows = 0;
  if (!ctx || !out || !out_n) return fail(MADICP_ERR_INVALID, "null argument");
  *m = find_map(ctx, map_id);
  if (!*m) return fail(MADICP_ERR_INVALID, "unknown map id");
  if (!(*m)->col[need]) return fail(MADICP_ERR_INVALID, need == kColAttr ? kMapNoAttr : need == kColEv ? kMapNoEvidence : kMapNoMoments);
  if (first_row < 0 || first_row > (*m)->rows) return fail(MADICP_ERR_INVALID, "first_row outside [0, rows]");
  *out_n = (*m)->rows - first_row;
  if (capacity_rows < *out_n) return fail(MADICP_ERR_CAPACITY, short_buffer);
  if (*out_n > 0) HIP_TRY(hipSetDevice(ctx->device));
  *rows = *out_n;
  return MADICP_OK;
}
// ... and a download of the map's own columns is: the window's rows of every column `out` asks for
int map_download(madicp_ctx* ctx, int map_id, MapColumn need, int64_t first_row, const void* must, const MapCols& out, int64_t capacity_rows,
                 const char* short_buffer, int64_t* out_n) {
  DevMap* m = nullptr;
  int64_t rows = 0;
  RC_TRY(map_window(ctx, map_id, need, first_row, must, capacity_rows, short_buffer, out_n, &m, &rows));
  return rows == 0 ? MADICP_OK : map_rows_out(ctx, *m, out, first_row, rows, "voxel map download: ");
}

// What madicp_map_prune and madicp_map_clear_rays share around `remove`, the one that makes its marks (map_prune_on /
// map_clear_rays_on behind the caller's arguments): the refusals, the log's memory in front of it, the log's length behind it, the
// three answers.  run: false where nothing can leave — nothing is launched
template <class Remove>
int map_removal(madicp_ctx* ctx, DevMap* m, bool run, int64_t watermark, Remove remove, int64_t* out_removed, int64_t* out_rows,
                int64_t* out_watermark) {
  if (watermark < 0 || watermark > m->rows) return fail(MADICP_ERR_INVALID, "watermark outside [0, rows]");
  if (m->track && m->log_n >= m->max_rows) return fail(MADICP_ERR_CAPACITY, kMapLogFull);
  const int64_t before = m->rows;
  int64_t kept = before, mark = watermark;
  if (run) {
    HIP_TRY(hipSetDevice(ctx->device));
    char* old_log = nullptr;
    if (m->track && watermark > 0) RC_TRY(map_log_reserve(ctx, m, m->log_n + watermark, &old_log));
    const int rc = remove(&kept, &mark);
    map_log_settle(ctx, m, old_log, rc, watermark - mark);
    RC_TRY(rc);
  }
  *out_removed = before - kept;
  *out_rows = kept;
  *out_watermark = mark;
  return MADICP_OK;
}
}  // namespace
extern "C" {
int madicp_map_create(madicp_ctx* ctx, double voxel, int64_t initial_rows, int64_t max_rows, int* out_map_id) {
  return map_create_on(ctx, voxel, initial_rows, max_rows, false, out_map_id);
}
int madicp_map_create_attr(madicp_ctx* ctx, double voxel, int64_t initial_rows, int64_t max_rows, int* out_map_id) {
  return map_create_on(ctx, voxel, initial_rows, max_rows, true, out_map_id);
}
int madicp_map_create_ev(madicp_ctx* ctx, double voxel, int64_t initial_rows, int64_t max_rows, int with_attr, uint32_t hit, uint32_t miss,
                         uint32_t cap, int* out_map_id) {
  const uint32_t evidence[3] = {hit, miss, cap};
  return map_create_on(ctx, voxel, initial_rows, max_rows, with_attr != 0, out_map_id, evidence);
}
int madicp_map_create_mom(madicp_ctx* ctx, double voxel, int64_t initial_rows, int64_t max_rows, int with_attr, const uint32_t evidence[3],
                          uint32_t max_count, int* out_map_id) {
  return map_create_on(ctx, voxel, initial_rows, max_rows, with_attr != 0, out_map_id, evidence, &max_count);
}

int madicp_map_insert_cloud(madicp_ctx* ctx, int map_id, int cloud_id, const double R[9], const double t[3], int64_t* out_added,
                            int64_t* out_rows) {
  if (!ctx || !R || !t || !out_added || !out_rows) return fail(MADICP_ERR_INVALID, "null argument");
  DevMap* m = find_map(ctx, map_id);
  if (!m) return fail(MADICP_ERR_INVALID, "unknown map id");
  DevCloud* c = find_cloud(ctx, cloud_id);
  if (!c) return fail(MADICP_ERR_INVALID, "unknown cloud id");
  if (const char* why = madicp_host::export_refusal(R, t, m->voxel)) return fail(MADICP_ERR_INVALID, why);
  RC_TRY(busy_with_lookahead(ctx));
  const int64_t n = c->n;
  if (m->rows + n > m->max_rows) return fail(MADICP_ERR_CAPACITY, "the map's rows and the cloud's points together exceed max_rows");
  if (n == 0) {
    *out_added = 0;
    *out_rows = m->rows;
    return MADICP_OK;
  }
  if (m->with_mom && m->ordinal > madicp_host::kMomentsLastOrdinal)
    return fail(MADICP_ERR_CAPACITY, "the moments map has folded 2^32 - 1 clouds since it was made or cleared (madicp_map_clear starts again)");
  HIP_TRY(hipSetDevice(ctx->device));
  FrontScratch* fs = nullptr;
  RC_TRY(ensure_scratch(ctx, n, &fs));
  if (m->rows + n > m->cap) RC_TRY(map_grow(ctx, m, m->rows + n));
  int64_t added = 0;
  const FoldMoments Mo{m->mom(), m->closed_at(), m->slot_row(), m->ordinal, m->mom_max_count};
  FoldEvidence E{};
  if (m->with_ev) {
    if (m->fold_no == fe::kMapNever) HIP_TRY(map_stamp_wipe(ctx, m));  // (2^32 - 1 folds without a removal or a growth)
    E = FoldEvidence{m->ev(), m->slot_row(), m->stamp(), m->fold_no++, m->ev_hit, m->ev_cap};
  }
  RC_TRY(voxel_fold(ctx, fs, c, export_pose(R, t), m->voxel, VoxelTable{m->keys(), m->owner(), m->slots}, true, m->xyz(), m->rows,
                    m->row_keys(), m->attr(), &added, m->with_ev ? &E : nullptr, m->with_mom ? &Mo : nullptr));
  if (m->with_mom) ++m->ordinal;
  m->rows += added;
  *out_added = added;
  *out_rows = m->rows;
  return MADICP_OK;
}

// A batch of saved rows merged in as ONE fold (csrc/common/map_merge.h has the rule, frontend.hip.h the kernels and the determinism
// argument).  Busy and scratch rules are the fold's: the per-fold scratch lies in the builder's (slot_of, marks, scan, total — as in
// voxel_fold), growth keeps the table at most half full.  The batch itself goes through the pinned staging in ONE copy into a
// transient pooled block of the call's own —
//   keys (n x 8) | mom (n x 80) | xyz (n x 12) | attr (n x 4) | ev (n x 4)
// of which only the columns the map has are there — and that block goes back behind the wait.  Claim, mark, scan, the count's copy,
// append and (evidence and moments maps) combine are enqueued before the host knows the count: ONE synchronisation for the result —
// in the sense of every staged upload: acquiring the staging slot waits for the copy that last used it, and a growth adds its own wait.
int madicp_map_merge_rows(madicp_ctx* ctx, int map_id, double voxel, const uint64_t* keys, const float* xyz, const uint32_t* attr,
                          const uint32_t* ev, const uint64_t* mom, int64_t n, int64_t* out_added, int64_t* out_rows) {
  if (!ctx || !out_added || !out_rows) return fail(MADICP_ERR_INVALID, "null argument");
  DevMap* m = find_map(ctx, map_id);
  if (!m) return fail(MADICP_ERR_INVALID, "unknown map id");
  RC_TRY(busy_with_lookahead(ctx));  // (in front of the O(n) pass, as the fold asks first)
  bool capacity = false;
  if (const char* why = madicp_host::map_merge_refusal(
          madicp_host::MergeBatch{keys, xyz, attr, ev, mom, n}, voxel,
          madicp_host::MergeTarget{m->voxel, m->with_attr, m->with_ev, m->with_mom, m->rows, m->max_rows, m->ordinal}, &capacity))
    return fail(capacity ? MADICP_ERR_CAPACITY : MADICP_ERR_INVALID, why);
  if (n == 0) {
    *out_added = 0;
    *out_rows = m->rows;
    return MADICP_OK;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  FrontScratch* fs = nullptr;
  RC_TRY(ensure_scratch(ctx, n, &fs));
  const size_t N = (size_t)n;
  size_t off = 0;
  auto place = [&](bool wanted, size_t bytes) {
    const size_t at = off;
    if (wanted) off = align_up(off + bytes);
    return at;
  };
  const size_t at_keys = place(true, 8 * N), at_mom = place(m->with_mom, 8 * madicp_host::kMomentWords * N), at_xyz = place(true, 12 * N);
  const size_t at_attr = place(m->with_attr, 4 * N), at_ev = place(m->with_ev, 4 * N);
  int hb = 0;
  char* stage = nullptr;
  RC_TRY(ctx->staging.acquire(off, &hb, &stage));
  std::memcpy(stage + at_keys, keys, 8 * N);
  if (m->with_mom) std::memcpy(stage + at_mom, mom, 8 * madicp_host::kMomentWords * N);
  std::memcpy(stage + at_xyz, xyz, 12 * N);
  if (m->with_attr) std::memcpy(stage + at_attr, attr, 4 * N);
  if (m->with_ev) std::memcpy(stage + at_ev, ev, 4 * N);
  void* p = nullptr;
  RC_TRY(pool_alloc(ctx, off, ctx->copy, &p));
  char* block = static_cast<char*>(p);
  // growth last of what can fail in front of the launches: a call that cannot get its staging or its block has not touched the map's
  if (m->rows + n > m->cap) {
    const int rc = map_grow(ctx, m, m->rows + n);
    if (rc != MADICP_OK) {
      pool_free(ctx, block, nullptr);  // (nothing was enqueued on it)
      return rc;
    }
  }
  const fe::MergeRows B{reinterpret_cast<const unsigned long long*>(block + at_keys), reinterpret_cast<const uint32_t*>(block + at_xyz),
                        m->with_attr ? reinterpret_cast<const uint32_t*>(block + at_attr) : nullptr,
                        m->with_ev ? reinterpret_cast<const uint32_t*>(block + at_ev) : nullptr,
                        m->with_mom ? reinterpret_cast<const unsigned long long*>(block + at_mom) : nullptr};
  uint32_t* slot_of = fs->idx[0];
  uint32_t* mark = fs->P.leaf_start;
  const int blocks = grid_256(ctx, n);
  hipError_t e = hipMemcpyAsync(block, stage, off, hipMemcpyHostToDevice, ctx->copy);
  if (e == hipSuccess) e = ctx->staging.sent(hb, ctx->copy);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(fe::rows_claim, dim3(blocks), dim3(256), 0, ctx->copy, B.keys, (long)n, m->keys(), m->owner(), m->slots, slot_of);
    hipLaunchKernelGGL(fe::voxel_mark, dim3(blocks), dim3(256), 0, ctx->copy, (const uint32_t*)slot_of, (const uint32_t*)m->owner(), (long)n, mark);
    e = scan_marks(ctx->copy, mark, n, fs->S, fs->tile_sums, &fs->rec_res->r.kept);
  }
  if (e == hipSuccess) e = hipMemcpyAsync(&fs->h_rec_res->r.kept, &fs->rec_res->r.kept, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->copy);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(fe::rows_append, dim3(blocks), dim3(256), 0, ctx->copy, B, (long)n, (const uint32_t*)mark, (const uint32_t*)fs->S,
                       (const uint32_t*)slot_of, m->owner(), (long)m->rows, reinterpret_cast<uint32_t*>(m->xyz()), m->row_keys(), m->attr(),
                       m->ev(), m->slot_row(), m->mom(), m->closed_at());
    if (m->with_ev || m->with_mom)
      hipLaunchKernelGGL(fe::rows_combine, dim3(blocks), dim3(256), 0, ctx->copy, B, (long)n, (const uint32_t*)slot_of,
                         (const uint32_t*)m->slot_row(), m->ev(), m->ev_cap, m->mom(), m->closed_at(), m->ordinal, m->mom_max_count);
    e = hipGetLastError();
  }
  const hipError_t w = hipStreamSynchronize(ctx->copy);  // the count
  if (e == hipSuccess) e = w;
  pool_free(ctx, block, nullptr);  // (behind the wait: nothing is in flight on it)
  if (e != hipSuccess) return fail(MADICP_ERR_DEVICE, std::string("voxel map merge: ") + hipGetErrorString(e));
  const int64_t added = fs->h_rec_res->r.kept;
  if (m->with_mom) ++m->ordinal;
  m->rows += added;
  *out_added = added;
  *out_rows = m->rows;
  return MADICP_OK;
}

int madicp_map_size(madicp_ctx* ctx, int map_id, int64_t* out_rows) {
  if (!ctx || !out_rows) return fail(MADICP_ERR_INVALID, "null argument");
  DevMap* m = find_map(ctx, map_id);
  if (!m) return fail(MADICP_ERR_INVALID, "unknown map id");
  *out_rows = m->rows;
  return MADICP_OK;
}

// the window downloads: map_window's prologue, the copies in front of ONE wait (map_rows_out)
int madicp_map_download_f32(madicp_ctx* ctx, int map_id, int64_t first_row, float* out_xyz, int64_t capacity_rows, int64_t* out_n) {
  return map_download(ctx, map_id, kColXyz, first_row, out_xyz, map_out(out_xyz, nullptr, nullptr), capacity_rows,
                      "out_xyz holds fewer rows than the window has (*out_n)", out_n);
}
int madicp_map_download_attr(madicp_ctx* ctx, int map_id, int64_t first_row, uint32_t* out_attr, int64_t capacity_rows, int64_t* out_n) {
  return map_download(ctx, map_id, kColAttr, first_row, out_attr, map_out(nullptr, nullptr, out_attr), capacity_rows,
                      "out_attr holds fewer rows than the window has (*out_n)", out_n);
}
int madicp_map_download_keys(madicp_ctx* ctx, int map_id, int64_t first_row, uint64_t* out_keys, int64_t capacity_rows, int64_t* out_n) {
  return map_download(ctx, map_id, kColXyz, first_row, out_keys, map_out(nullptr, out_keys, nullptr), capacity_rows,
                      "out_keys holds fewer rows than the window has (*out_n)", out_n);
}
int madicp_map_download_rows(madicp_ctx* ctx, int map_id, int64_t first_row, float* out_xyz, uint64_t* out_keys, uint32_t* out_attr,
                             int64_t capacity_rows, int64_t* out_n) {
  return map_download(ctx, map_id, out_attr ? kColAttr : kColXyz, first_row, out_xyz, map_out(out_xyz, out_keys, out_attr), capacity_rows,
                      "the buffers hold fewer rows than the window has (*out_n)", out_n);
}
int madicp_map_download_evidence(madicp_ctx* ctx, int map_id, int64_t first_row, uint32_t* out_ev, int64_t capacity_rows, int64_t* out_n) {
  return map_download(ctx, map_id, kColEv, first_row, out_ev, map_out(nullptr, nullptr, nullptr, out_ev), capacity_rows,
                      "out_ev holds fewer rows than the window has (*out_n)", out_n);
}
int madicp_map_download_moments(madicp_ctx* ctx, int map_id, int64_t first_row, uint64_t* out, int64_t capacity_rows, int64_t* out_n) {
  return map_download(ctx, map_id, kColMom, first_row, out, map_out(nullptr, nullptr, nullptr, nullptr, out), capacity_rows,
                      "out holds fewer rows than the window has (*out_n)", out_n);
}

// The surfels of rows [first_row, M): fe::map_surfels, one lane per row, into a transient block of the call's own
//   centroid (rows x 12) | normal (rows x 12) | eig (rows x 12) | count (rows x 4)
// then the copies of what the caller asked for in ONE chain behind the kernel, ONE wait.
int madicp_map_download_surfels(madicp_ctx* ctx, int map_id, int64_t first_row, float* out_centroid, float* out_normal, float* out_eig,
                                uint32_t* out_count, int64_t capacity_rows, int64_t* out_n) {
  DevMap* m = nullptr;
  int64_t rows = 0;
  RC_TRY(map_window(ctx, map_id, kColMom, first_row, out_centroid, capacity_rows, "the buffers hold fewer rows than the window has (*out_n)",
                    out_n, &m, &rows));
  if (rows == 0) return MADICP_OK;
  const size_t R = (size_t)rows;
  char* block = nullptr;
  HIP_TRY(hipMalloc(&block, 40 * R));
  float* d_centroid = reinterpret_cast<float*>(block);
  float* d_normal = d_centroid + 3 * R;
  float* d_eig = d_normal + 3 * R;
  uint32_t* d_count = reinterpret_cast<uint32_t*>(d_eig + 3 * R);
  hipLaunchKernelGGL(fe::map_surfels, dim3(grid_256(ctx, rows)), dim3(256), 0, ctx->copy, (const unsigned long long*)m->mom(),
                     (const unsigned long long*)m->row_keys(), (long)first_row, (long)m->rows, m->voxel, d_centroid, d_normal, d_eig, d_count);
  const CopyOut outs[] = {{out_centroid, d_centroid, 12 * R}, {out_normal, d_normal, 12 * R}, {out_eig, d_eig, 12 * R}, {out_count, d_count, 4 * R}};
  const int rc = copies_then_wait(ctx, hipGetLastError(), outs, 4, "voxel map surfel download: ");
  hipFree(block);
  return rc;
}

// The rows whose word is at least min_e, compacted on the device into a transient block of the call's own (the builder's scratch
// is sized by the largest CLOUD and may be a look-ahead's): M entries of keys | xyz | attr | ev, and behind them a prune's scratch.
// fe::map_ev_mark, the tile scan, and map_compact as the one gather (watermark 0: it leaves the count over the first mark).  Two
// waits: the count — which decides whether the caller's buffers are large enough — then the rows.
int madicp_map_download_min_evidence(madicp_ctx* ctx, int map_id, uint32_t min_e, float* out_xyz, uint64_t* out_keys, uint32_t* out_attr,
                                     uint32_t* out_ev, int64_t capacity_rows, int64_t* out_n) {
  if (!ctx || !out_xyz || !out_n) return fail(MADICP_ERR_INVALID, "null argument");
  DevMap* m = find_map(ctx, map_id);
  if (!m) return fail(MADICP_ERR_INVALID, "unknown map id");
  if (!m->with_ev) return fail(MADICP_ERR_INVALID, kMapNoEvidence);
  if (out_attr && !m->with_attr) return fail(MADICP_ERR_INVALID, kMapNoAttr);
  const int64_t M = m->rows;
  *out_n = 0;
  if (M == 0) return MADICP_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  const MapLayout L = map_layout_of((size_t)M, 0, map_bit(kColRowKeys) | map_bit(kColXyz) | map_bit(kColAttr) | map_bit(kColEv));
  const MapScratch W = map_prune_scratch((size_t)M, (size_t)M, tb::kScanTile);
  char* block = nullptr;
  HIP_TRY(hipMalloc(&block, L.bytes + W.bytes));
  MapCols found;  // (no moments: the gather leaves them where they are)
  found.point(block, L);
  uint32_t* mark = reinterpret_cast<uint32_t*>(block + L.bytes + W.mark);
  uint32_t* S = reinterpret_cast<uint32_t*>(block + L.bytes + W.S);
  fe::MapRows in = m->moving();
  in.mom = nullptr;
  hipLaunchKernelGGL(fe::map_ev_mark, dim3(grid_256(ctx, M + 1)), dim3(256), 0, ctx->copy, (const uint32_t*)m->ev(), (long)M, min_e, mark);
  hipError_t e = scan_marks(ctx->copy, mark, M, S, reinterpret_cast<uint32_t*>(block + L.bytes + W.tile_sums),
                            reinterpret_cast<int32_t*>(block + L.bytes + W.total));
  hipLaunchKernelGGL(fe::map_compact, dim3(grid_256(ctx, M + 1)), dim3(256), 0, ctx->copy, (const uint32_t*)S, (long)M, 0L, in, found.moving(),
                     mark);
  uint32_t res[2] = {0, 0};
  if (e == hipSuccess) e = hipGetLastError();
  const CopyOut count{res, mark, sizeof(res)};
  int rc = copies_then_wait(ctx, e, &count, 1, "voxel map evidence download: ");  // the count
  if (rc == MADICP_OK) {
    *out_n = res[0];
    if (capacity_rows < *out_n)
      rc = fail(MADICP_ERR_CAPACITY, "the buffers hold fewer rows than qualify (*out_n)");
    else if (*out_n > 0)  // the rows
      rc = map_rows_out(ctx, found, map_out(out_xyz, out_keys, out_attr, out_ev), 0, *out_n, "voxel map evidence download: ");
  }
  hipFree(block);
  return rc;
}

int madicp_map_track_removed(madicp_ctx* ctx, int map_id, int on) {
  if (!ctx) return fail(MADICP_ERR_INVALID, "null argument");
  DevMap* m = find_map(ctx, map_id);
  if (!m) return fail(MADICP_ERR_INVALID, "unknown map id");
  m->track = on != 0;
  if (!m->track && m->log_block) {  // (every call that wrote or read the log has ended with a wait: nothing is in flight on it)
    HIP_TRY(hipSetDevice(ctx->device));
    hipFree(m->log_block);
    m->log_block = nullptr;
    m->log = MapCols{};
    m->log_cap = 0;
  }
  if (!m->track) m->log_n = 0;
  return MADICP_OK;
}

int madicp_map_removed_count(madicp_ctx* ctx, int map_id, int64_t* out_n) {
  if (!ctx || !out_n) return fail(MADICP_ERR_INVALID, "null argument");
  DevMap* m = find_map(ctx, map_id);
  if (!m) return fail(MADICP_ERR_INVALID, "unknown map id");
  *out_n = m->log_n;
  return MADICP_OK;
}

int madicp_map_take_removed(madicp_ctx* ctx, int map_id, uint64_t* out_keys, float* out_xyz, uint32_t* out_attr, int64_t capacity,
                            int64_t* out_n) {
  if (!ctx || !out_keys || !out_xyz || !out_n) return fail(MADICP_ERR_INVALID, "null argument");
  DevMap* m = find_map(ctx, map_id);
  if (!m) return fail(MADICP_ERR_INVALID, "unknown map id");
  if (!m->track) return fail(MADICP_ERR_INVALID, "the map does not track removals (madicp_map_track_removed)");
  if (out_attr && !m->with_attr) return fail(MADICP_ERR_INVALID, kMapNoAttr);
  const int64_t n = m->log_n;
  *out_n = n;
  if (capacity < n) return fail(MADICP_ERR_CAPACITY, "the buffers hold fewer entries than the removal log has (*out_n)");
  if (n == 0) return MADICP_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  RC_TRY(map_rows_out(ctx, m->log, map_out(out_xyz, out_keys, out_attr), 0, n, "voxel map removal log: "));
  m->log_n = 0;  // (the memory is kept)
  return MADICP_OK;
}

int madicp_map_prune(madicp_ctx* ctx, int map_id, const double center[3], double radius, int64_t watermark, int64_t* out_removed,
                     int64_t* out_rows, int64_t* out_watermark) {
  if (!ctx || !center || !out_removed || !out_rows || !out_watermark) return fail(MADICP_ERR_INVALID, "null argument");
  DevMap* m = find_map(ctx, map_id);
  if (!m) return fail(MADICP_ERR_INVALID, "unknown map id");
  if (const char* why = madicp_host::map_prune_refusal(center, radius)) return fail(MADICP_ERR_INVALID, why);
  fe::PruneSphere Q;
  std::memcpy(Q.c, center, sizeof(Q.c));
  Q.r2 = radius * radius;
  return map_removal(
      ctx, m, m->rows > 0, watermark, [&](int64_t* kept, int64_t* mark) { return map_prune_on(ctx, m, Q, watermark, kept, mark); }, out_removed,
      out_rows, out_watermark);
}

int madicp_map_clear_rays(madicp_ctx* ctx, int map_id, int cloud_id, const double R[9], const double t[3], const double origin[3],
                          double margin, int64_t watermark, int64_t* out_removed, int64_t* out_rows, int64_t* out_watermark) {
  if (!ctx || !R || !t || !origin || !out_removed || !out_rows || !out_watermark) return fail(MADICP_ERR_INVALID, "null argument");
  DevMap* m = find_map(ctx, map_id);
  if (!m) return fail(MADICP_ERR_INVALID, "unknown map id");
  DevCloud* c = find_cloud(ctx, cloud_id);
  if (!c) return fail(MADICP_ERR_INVALID, "unknown cloud id");
  if (const char* why = madicp_host::map_clear_refusal(R, t, origin, margin)) return fail(MADICP_ERR_INVALID, why);
  fe::RayFrame F;
  F.X = export_pose(R, t);
  std::memcpy(F.o, origin, sizeof(F.o));
  F.margin = margin;
  return map_removal(  // (an empty map or an empty cloud: nothing can leave, nothing is launched)
      ctx, m, m->rows > 0 && c->n > 0, watermark, [&](int64_t* kept, int64_t* mark) { return map_clear_rays_on(ctx, m, c, F, watermark, kept, mark); },
      out_removed, out_rows, out_watermark);
}

// The nearest row per point (fe::map_query_lanes; csrc/common/export_point.h has the rule).  The map's block is
// only read.  The call's scratch is ONE pooled block of its own — the builder's is not touched —
//   counts (3 x 8) | d2 (n x 8) | keys (n x 8) | row (n x 4) | attr (n x 4) | ev (n x 4) | slot_row (slots x 4)
// of which only what the caller asked for is there, and the last only on a map without the column (fe::map_slot_rows fills it).
// One memset for the counts, the kernels, the copies of what was asked for, ONE wait.
int madicp_map_query_cloud(madicp_ctx* ctx, int map_id, int cloud_id, const double R[9], const double t[3], int reach, double max_dist,
                           int32_t* out_row, double* out_d2, uint64_t* out_keys, uint32_t* out_attr, uint32_t* out_ev,
                           int64_t capacity_points, uint64_t out_counts[3]) {
  if (!ctx || !R || !t || !out_counts) return fail(MADICP_ERR_INVALID, "null argument");
  DevMap* m = find_map(ctx, map_id);
  if (!m) return fail(MADICP_ERR_INVALID, "unknown map id");
  DevCloud* c = find_cloud(ctx, cloud_id);
  if (!c) return fail(MADICP_ERR_INVALID, "unknown cloud id");
  if (const char* why = madicp_host::map_query_refusal(R, t, reach, max_dist)) return fail(MADICP_ERR_INVALID, why);
  if (out_attr && !m->with_attr) return fail(MADICP_ERR_INVALID, kMapNoAttr);
  if (out_ev && !m->with_ev) return fail(MADICP_ERR_INVALID, kMapNoEvidence);
  const int64_t n = c->n;
  if ((out_row || out_d2 || out_keys || out_attr || out_ev) && capacity_points < n)
    return fail(MADICP_ERR_CAPACITY, "the per-point buffers hold fewer entries than the cloud has points");
  if (n == 0) {
    out_counts[0] = out_counts[1] = out_counts[2] = 0;
    return MADICP_OK;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  const size_t N = (size_t)n;
  const bool own_slot_row = !m->slot_row();
  size_t off = align_up(3 * sizeof(uint64_t));
  auto place = [&](bool wanted, size_t bytes) {
    const size_t at = off;
    if (wanted) off = align_up(off + bytes);
    return at;
  };
  const size_t at_d2 = place(out_d2, 8 * N), at_keys = place(out_keys, 8 * N), at_row = place(out_row, 4 * N);
  const size_t at_attr = place(out_attr, 4 * N), at_ev = place(out_ev, 4 * N), at_slot_row = place(own_slot_row, 4 * (size_t)m->slots);
  void* p = nullptr;
  RC_TRY(pool_alloc(ctx, off, ctx->copy, &p));
  char* block = static_cast<char*>(p);
  auto at = [&](bool wanted, size_t where) { return wanted ? block + where : nullptr; };
  fe::QueryOut O;
  O.counts = reinterpret_cast<unsigned long long*>(block);
  O.d2 = reinterpret_cast<double*>(at(out_d2, at_d2));
  O.keys = reinterpret_cast<unsigned long long*>(at(out_keys, at_keys));
  O.row = reinterpret_cast<int32_t*>(at(out_row, at_row));
  O.attr = reinterpret_cast<uint32_t*>(at(out_attr, at_attr));
  O.ev = reinterpret_cast<uint32_t*>(at(out_ev, at_ev));
  uint32_t* slot_row = own_slot_row ? reinterpret_cast<uint32_t*>(block + at_slot_row) : m->slot_row();
  const fe::QueryMap Q{m->keys(), m->slots, slot_row, m->xyz(), (long)m->rows, m->row_keys(), out_attr ? m->attr() : nullptr,
                       out_ev ? m->ev() : nullptr};
  hipError_t e = hipMemsetAsync(O.counts, 0, 3 * sizeof(uint64_t), ctx->copy);
  if (e == hipSuccess) {
    if (own_slot_row && m->rows > 0)
      hipLaunchKernelGGL(fe::map_slot_rows, dim3(grid_256(ctx, m->rows)), dim3(256), 0, ctx->copy, (const unsigned long long*)m->row_keys(),
                         (long)m->rows, (const unsigned long long*)m->keys(), m->slots, slot_row);
    const double md2 = max_dist * max_dist;
#ifdef MADICP_QUERY_COOP  // (the measurement's other leg, tools/map_query_time.py --variant: measured slower, the same bits)
    if (reach == 1)
      hipLaunchKernelGGL(fe::map_query_coop, dim3(grid_256(ctx, n)), dim3(256), 0, ctx->copy, (const double*)c->xyz, (long)n,
                         export_pose(R, t), m->voxel, md2, Q, O);
    else
#endif
      hipLaunchKernelGGL(fe::map_query_lanes, dim3(grid_256(ctx, n)), dim3(256), 0, ctx->copy, (const double*)c->xyz, (long)n,
                         export_pose(R, t), m->voxel, reach, md2, Q, O);
    e = hipGetLastError();
  }
  uint64_t counts[3] = {0, 0, 0};
  const CopyOut outs[] = {{counts, O.counts, sizeof(counts)}, {out_row, O.row, 4 * N},   {out_d2, O.d2, 8 * N},
                          {out_keys, O.keys, 8 * N},          {out_attr, O.attr, 4 * N}, {out_ev, O.ev, 4 * N}};
  const int rc = copies_then_wait(ctx, e, outs, 6, "voxel map query: ");
  pool_free(ctx, block, nullptr);  // (behind the wait: nothing is in flight on it)
  if (rc == MADICP_OK) std::memcpy(out_counts, counts, sizeof(counts));
  return rc;
}

// The query's three counts at each of n_poses poses (fe::map_score_poses; csrc/common/export_point.h has the rule).  The map's block
// is only read.  The call's scratch is ONE pooled block of its own — the builder's is not touched —
//   counts (K x 3 x 8) | poses (K x 96) | slot_row (slots x 4)
// the last only on a map without the column (fe::map_slot_rows fills it).  Everything on the copy stream: one memset for the counts,
// the pose upload, the kernels, one copy out, ONE wait, whatever n, M and K.
int madicp_map_score_poses(madicp_ctx* ctx, int map_id, int cloud_id, const double* poses, int64_t n_poses, int reach, double max_dist,
                           int64_t stride, uint64_t* out_counts) {
  if (!ctx || !poses || !out_counts) return fail(MADICP_ERR_INVALID, "null argument");
  DevMap* m = find_map(ctx, map_id);
  if (!m) return fail(MADICP_ERR_INVALID, "unknown map id");
  DevCloud* c = find_cloud(ctx, cloud_id);
  if (!c) return fail(MADICP_ERR_INVALID, "unknown cloud id");
  if (const char* why = madicp_host::map_score_refusal(poses, n_poses, reach, max_dist, stride)) return fail(MADICP_ERR_INVALID, why);
  const int64_t n = c->n;
  const size_t K = (size_t)n_poses;
  if (n <= 0) {  // (never: a resident cloud holds at least one point)
    std::fill(out_counts, out_counts + 3 * K, uint64_t(0));
    return MADICP_OK;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  const int64_t n_take = (n - 1) / stride + 1;
  const bool own_slot_row = !m->slot_row();
  const size_t at_poses = align_up(8 * 3 * K), at_slot_row = align_up(at_poses + 8 * madicp_host::kScorePoseDoubles * K);
  void* p = nullptr;
  RC_TRY(pool_alloc(ctx, own_slot_row ? at_slot_row + 4 * (size_t)m->slots : at_slot_row, ctx->copy, &p));
  char* block = static_cast<char*>(p);
  unsigned long long* d_counts = reinterpret_cast<unsigned long long*>(block);
  double* d_poses = reinterpret_cast<double*>(block + at_poses);
  uint32_t* slot_row = own_slot_row ? reinterpret_cast<uint32_t*>(block + at_slot_row) : m->slot_row();
  const fe::QueryMap Q{m->keys(), m->slots, slot_row, m->xyz(), (long)m->rows, m->row_keys(), nullptr, nullptr};
  hipError_t e = hipMemsetAsync(d_counts, 0, 8 * 3 * K, ctx->copy);
  if (e == hipSuccess)
    e = hipMemcpyAsync(d_poses, poses, 8 * madicp_host::kScorePoseDoubles * K, hipMemcpyHostToDevice, ctx->copy);
  if (e == hipSuccess) {
    if (own_slot_row && m->rows > 0)
      hipLaunchKernelGGL(fe::map_slot_rows, dim3(grid_256(ctx, m->rows)), dim3(256), 0, ctx->copy, (const unsigned long long*)m->row_keys(),
                         (long)m->rows, (const unsigned long long*)m->keys(), m->slots, slot_row);
    // chunks of poses in y; in x as many workgroups as the points that take part fill, the whole grid about 8 per CU
    const unsigned chunks = (unsigned)((n_poses + fe::kScoreChunk - 1) / fe::kScoreChunk);
    const int64_t per_chunk = std::max<int64_t>(((int64_t)ctx->n_cus * 8 + chunks - 1) / chunks, 1);
    const dim3 grid((unsigned)std::min<int64_t>((n_take + 255) / 256, per_chunk), chunks);
    const double md2 = max_dist * max_dist;
    if (reach == 0)
      hipLaunchKernelGGL(fe::map_score_poses<0>, grid, dim3(256), 0, ctx->copy, (const double*)c->xyz, (long)n_take, (long)stride,
                         (const double*)d_poses, (int)n_poses, m->voxel, md2, Q, d_counts);
    else
      hipLaunchKernelGGL(fe::map_score_poses<1>, grid, dim3(256), 0, ctx->copy, (const double*)c->xyz, (long)n_take, (long)stride,
                         (const double*)d_poses, (int)n_poses, m->voxel, md2, Q, d_counts);
    e = hipGetLastError();
  }
  std::vector<uint64_t> counts(3 * K);
  const CopyOut outs[] = {{counts.data(), d_counts, 8 * 3 * K}};
  const int rc = copies_then_wait(ctx, e, outs, 1, "voxel map scoring: ");
  pool_free(ctx, block, nullptr);  // (behind the wait: nothing is in flight on it)
  if (rc == MADICP_OK) std::memcpy(out_counts, counts.data(), 8 * 3 * K);
  return rc;
}

// `iterations` Gauss-Newton rounds of a resident cloud against the map's surfels (csrc/common/map_align.h has the rule).  The
// map's block is only read.  The call's scratch is ONE pooled block of its own — the builder's is not touched —
//   counts ((K + 1) x 4 x 8) | pose (12 x 8) | trace ((K + 1) x 40 x 8) | partial rows A (ceil(n / 256) x 28 x 8) | partial rows B
//   (ceil(rows A / 256) x 28 x 8) | e (n x 8) | centroid, normal, eig (M x 12 each) | count (M x 4) | row (n x 4) | slot_row
// of which the per-point columns are there only where asked for and the last only on a map without the column (none with moments
// today).  One memset for the counts, fe::map_surfels once, K x (terms, joins, step), the closing linearisation, the copies, ONE wait.
int madicp_map_register_cloud(madicp_ctx* ctx, int map_id, int cloud_id, const double R[9], const double t[3],
                              const madicp_map_align_params* params, int iterations, double out_R[9], double out_t[3], double* out_trace,
                              uint64_t* out_counts, int32_t* out_row, double* out_e, int64_t capacity_points) {
  if (!ctx || !R || !t || !params || !out_R || !out_t || !out_trace || !out_counts) return fail(MADICP_ERR_INVALID, "null argument");
  DevMap* m = find_map(ctx, map_id);
  if (!m) return fail(MADICP_ERR_INVALID, "unknown map id");
  DevCloud* c = find_cloud(ctx, cloud_id);
  if (!c) return fail(MADICP_ERR_INVALID, "unknown cloud id");
  if (!m->with_mom) return fail(MADICP_ERR_INVALID, kMapNoMoments);
  if (const char* why = madicp_host::map_align_refusal(R, t, params->reach, params->max_dist, params->rho, params->min_count, params->flat))
    return fail(MADICP_ERR_INVALID, why);
  if (iterations < 0 || iterations > madicp_host::kAlignMaxIterations) return fail(MADICP_ERR_INVALID, "iterations: 0 .. 64");
  if ((out_row || out_e) && iterations > 0)
    return fail(MADICP_ERR_INVALID, "per-point buffers belong to the linearise-only form (iterations == 0)");
  const int64_t n = c->n;
  if ((out_row || out_e) && capacity_points < n)
    return fail(MADICP_ERR_CAPACITY, "the per-point buffers hold fewer entries than the cloud has points");
  if (n <= 0) return fail(MADICP_ERR_INVALID, "the cloud is empty");  // (never: a resident cloud holds at least one point)
  HIP_TRY(hipSetDevice(ctx->device));
  constexpr size_t kT = madicp_host::kAlignTerms, kRow = madicp_host::kAlignTraceRow, kC = madicp_host::kAlignCounts;
  const size_t N = (size_t)n, M = (size_t)m->rows, K1 = (size_t)iterations + 1;
  const int64_t rows_a = (n + madicp_host::kAlignBlock - 1) / madicp_host::kAlignBlock;
  const int64_t rows_b = (rows_a + madicp_host::kAlignBlock - 1) / madicp_host::kAlignBlock;
  const bool own_slot_row = !m->slot_row();
  size_t off = 0;
  auto place = [&](bool wanted, size_t bytes) {
    const size_t at = off;
    if (wanted) off = align_up(off + bytes);
    return at;
  };
  const size_t at_counts = place(true, 8 * kC * K1), at_pose = place(true, 8 * 12), at_trace = place(true, 8 * kRow * K1);
  const size_t at_a = place(true, 8 * kT * (size_t)rows_a), at_b = place(true, 8 * kT * (size_t)rows_b), at_e = place(out_e, 8 * N);
  const size_t at_centroid = place(true, 12 * M), at_normal = place(true, 12 * M), at_eig = place(true, 12 * M), at_count = place(true, 4 * M);
  const size_t at_row = place(out_row, 4 * N), at_slot_row = place(own_slot_row, 4 * (size_t)m->slots);
  void* p = nullptr;
  RC_TRY(pool_alloc(ctx, off, ctx->copy, &p));
  char* block = static_cast<char*>(p);
  unsigned long long* d_counts = reinterpret_cast<unsigned long long*>(block + at_counts);
  double* d_pose = reinterpret_cast<double*>(block + at_pose);
  double* d_trace = reinterpret_cast<double*>(block + at_trace);
  double* d_rows[2] = {reinterpret_cast<double*>(block + at_a), reinterpret_cast<double*>(block + at_b)};
  double* d_e = out_e ? reinterpret_cast<double*>(block + at_e) : nullptr;
  int32_t* d_row = out_row ? reinterpret_cast<int32_t*>(block + at_row) : nullptr;
  float* d_centroid = reinterpret_cast<float*>(block + at_centroid);
  float* d_normal = reinterpret_cast<float*>(block + at_normal);
  float* d_eig = reinterpret_cast<float*>(block + at_eig);
  uint32_t* d_count = reinterpret_cast<uint32_t*>(block + at_count);
  uint32_t* slot_row = own_slot_row ? reinterpret_cast<uint32_t*>(block + at_slot_row) : m->slot_row();
  const fe::QueryMap Q{m->keys(), m->slots, slot_row, m->xyz(), (long)m->rows, m->row_keys(), nullptr, nullptr};
  const fe::AlignSurfels S{d_centroid, d_normal, d_eig, d_count};
  const fe::AlignGates G{params->max_dist * params->max_dist, params->rho, params->flat, params->min_count, params->reach};
  hipError_t e = hipMemsetAsync(d_counts, 0, 8 * kC * K1, ctx->copy);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(fe::map_align_pose, dim3(1), dim3(64), 0, ctx->copy, export_pose(R, t), d_pose);
    if (m->rows > 0) {
      if (own_slot_row)
        hipLaunchKernelGGL(fe::map_slot_rows, dim3(grid_256(ctx, m->rows)), dim3(256), 0, ctx->copy, (const unsigned long long*)m->row_keys(),
                           (long)m->rows, (const unsigned long long*)m->keys(), m->slots, slot_row);
      hipLaunchKernelGGL(fe::map_surfels, dim3(grid_256(ctx, m->rows)), dim3(256), 0, ctx->copy, (const unsigned long long*)m->mom(),
                         (const unsigned long long*)m->row_keys(), 0L, (long)m->rows, m->voxel, d_centroid, d_normal, d_eig, d_count);
    }
    for (int k = 0; k <= iterations; ++k) {  // (round `iterations` is the closing linearisation: no update)
      hipLaunchKernelGGL(fe::map_align_terms, dim3((unsigned)rows_a), dim3(256), 0, ctx->copy, (const double*)c->xyz, (long)n,
                         (const double*)d_pose, m->voxel, G, Q, S, d_rows[0], d_counts + kC * (size_t)k, d_row, d_e);
      int from = 0;
      for (int64_t rows = rows_a; rows > 1; from ^= 1) {  // 256 rows a workgroup: A -> B -> A ... until one row is left
        const int64_t next = (rows + madicp_host::kAlignBlock - 1) / madicp_host::kAlignBlock;
        hipLaunchKernelGGL(fe::map_align_join, dim3((unsigned)next), dim3(256), 0, ctx->copy, (const double*)d_rows[from], (long)rows,
                           d_rows[from ^ 1]);
        rows = next;
      }
      hipLaunchKernelGGL(fe::map_align_step, dim3(1), dim3(64), 0, ctx->copy, (const double*)d_rows[from], d_pose, k < iterations ? 1 : 0,
                         d_trace + kRow * (size_t)k);
    }
    e = hipGetLastError();
  }
  double X[12];
  std::vector<double> trace(kRow * K1);
  std::vector<uint64_t> counts(kC * K1);
  const CopyOut outs[] = {{X, d_pose, sizeof(X)},  {trace.data(), d_trace, 8 * kRow * K1}, {counts.data(), d_counts, 8 * kC * K1},
                          {out_row, d_row, 4 * N}, {out_e, d_e, 8 * N}};
  const int rc = copies_then_wait(ctx, e, outs, 5, "voxel map registration: ");
  pool_free(ctx, block, nullptr);  // (behind the wait: nothing is in flight on it)
  if (rc == MADICP_OK) {
    std::memcpy(out_R, X, 9 * sizeof(double));
    std::memcpy(out_t, X + 9, 3 * sizeof(double));
    std::memcpy(out_trace, trace.data(), 8 * kRow * K1);
    std::memcpy(out_counts, counts.data(), 8 * kC * K1);
  }
  return rc;
}

int madicp_map_clear(madicp_ctx* ctx, int map_id) {
  if (!ctx) return fail(MADICP_ERR_INVALID, "null argument");
  DevMap* m = find_map(ctx, map_id);
  if (!m) return fail(MADICP_ERR_INVALID, "unknown map id");
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(map_table_wipe(ctx, m));
  m->rows = 0;
  m->ordinal = 0;  // (the moments and freeze words go with their rows: voxel_rows starts every new row afresh)
  m->log_n = 0;  // (the log's memory is kept)
  return MADICP_OK;
}

int madicp_map_release(madicp_ctx* ctx, int map_id) {
  if (!ctx) return fail(MADICP_ERR_INVALID, "null argument");
  DevMap* m = find_map(ctx, map_id);
  if (!m) return fail(MADICP_ERR_INVALID, "unknown map id");
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipStreamSynchronize(ctx->copy));
  HIP_TRY(hipFree(m->block));
  if (m->log_block) hipFree(m->log_block);
  ctx->front->maps.erase(map_id);
  return MADICP_OK;
}

}  // extern "C"

// ---- MAD-tree construction on the device ------------------------------------------------------------------------------
namespace {

// the level kernels of steps [from, to) of the construction in flight, on its stream
// The breadth-first layout of the tree's LDS-staged top is made in three parts, each as the first workgroup of a level launch.
// Part [a, b) reads the nodes of levels a .. b, so they must be FINISHED, and a node of level L is finished by step L + 5 at
// the latest, not L: a small node born during the chip levels waits for step kChipLevels, and its descendants follow one
// step per level from there (a child of the root's small child, level 2, is step 7).  Hence step b + 6.  (Looking at the
// nodes themselves does not work: the array is not cleared between builds, an unwritten slot looks like last build's node.)
struct TopPart { int from, to, step; };
#ifndef MADICP_TB_TOP_EARLY  // (development: -DMADICP_TB_TOP_EARLY=5 runs the parts at step b + 1 — the schedule that looks right and is
#define MADICP_TB_TOP_EARLY 0  //  a race: the 200-frame drive of tests/test_gpu_frontend.py ended 1.8e-2 m off the host path with it)
#endif
constexpr int kTopLag = tb::kChipLevels - MADICP_TB_TOP_EARLY;
constexpr TopPart kTopParts[3] = {{0, 6, 6 + kTopLag}, {6, 9, 9 + kTopLag}, {9, kTopLevels, kTopLevels + kTopLag}};
static_assert(kTopLevels + kTopLag < 20, "the last part needs a step among the twenty that are always launched");

int tb_run_levels(FrontScratch& fs, int from, int to) {
  FrontScratch::InFlight& f = fs.fly;
  const tb::Params& P = f.P;
  hipStream_t s = f.s;
  for (int level = from; level < to; ++level) {
    if (f.chip && level < tb::kChipLevels) {
      hipLaunchKernelGGL(tb::tb_chip_stats, dim3(f.chip_grid), dim3(256), 0, s, P, level);
      hipLaunchKernelGGL(tb::tb_chip_scatter, dim3(f.chip_grid), dim3(256), 0, s, P, level);
    }
    if (level < P.first_step) continue;  // (wave / quad nodes born up here wait for step first_step: tree_build.hip.h)
    // a level has at most 2^level nodes: the early levels get a handful of workgroups, not the full grid (hundreds of
    // workgroups that only look at an empty queue still cost their dispatch)
    const int64_t nodes_max = level < 30 ? std::min<int64_t>((int64_t)1 << level, f.n) : f.n;
    // (+ one workgroup per team-regime node: at most n / kTeamMin of them, and none on a level that holds fewer nodes)
    const int64_t team_max = std::min<int64_t>(nodes_max, f.n / tb::kTeamMin);
    int grid = static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(f.level_grid, (nodes_max + 3) / 4 + (nodes_max + 63) / 64 + 1) + team_max));
    // levels the previous build did not reach are launched all the same (this tree may be deeper) but with a small grid — the
    // queues are walked with a stride, so any grid is correct, and 1 600 workgroups that find an empty queue cost 4.6 us
    if (f.quiet_from >= 0 && level > f.quiet_from) grid = std::min(grid, 96);
    // ... and a step the previous scan of this sensor had little work for gets a launch of that size + half (the queues are
    // walked with a stride: a larger crop is slower for one build, never wrong)
    if (f.use_need && level < tb::kNeedSteps) grid = std::min(grid, fs.last_need[level] + fs.last_need[level] / 2 + 24);
    // the breadth-first layout of the tree's LDS-staged top: the FIRST workgroup of three level launches (kTopParts above)
    int bfs_from = 0, bfs_to = 0;
    for (const TopPart& tp : kTopParts)
      if (level == tp.step) { bfs_from = tp.from; bfs_to = tp.to; }
    hipLaunchKernelGGL(tb::tb_level, dim3(grid + (bfs_to > bfs_from ? 1 : 0)), dim3(256), 0, s, P, level, bfs_from, bfs_to, kTopLevels, kTopMax);
  }
  return MADICP_OK;
}

// What the host needs before it can size the tree — leaf count (scan of the leaf starts), root mean, rho, size of the
// LDS-staged top, error flags, whether a queue is still waiting — arrives in fs.h_line.  Two halves: the kernels that
// produce it (direct scan path only; huge clouds do everything in the second half) ...
int tb_summary_enqueue(FrontScratch& fs, int next_step, bool again) {
  FrontScratch::InFlight& f = fs.fly;
  if (again)  // (a fresh State is all zero; a second summary must not add to the first)
    HIP_TRY(hipMemsetAsync(&f.P.st->n_leaves, 0, offsetof(tb::State, q_count) - offsetof(tb::State, n_leaves), f.s));  // the results line
  if (f.n_tiles > tb::kScanDirectMax) return MADICP_OK;
  f.seq = ++fs.build_seq;
  hipLaunchKernelGGL(tb::tb_finish_a, dim3(f.n_tiles + 64), dim3(256), 0, f.s, f.P, kTopLevels, f.n_tiles);
  hipLaunchKernelGGL(tb::tb_finish_b, dim3(f.n_tiles), dim3(256), 0, f.s, f.P, f.n_tiles, next_step, fs.h_line, f.seq);
  HIP_TRY(hipGetLastError());
  return MADICP_OK;
}
// ... and the wait for it
int tb_summary_wait(madicp_ctx* ctx, FrontScratch& fs, int next_step) {
  FrontScratch::InFlight& f = fs.fly;
  tb::HostLine& hl = *fs.h_line;
  if (f.n_tiles <= tb::kScanDirectMax) {
    // (unbounded: a build has no ticket to collect again, and no collective behind it; option "wait_mode" alone applies)
    const SeqWait w = wait_for_seq(ctx, &hl.seq, f.seq, WaitLimits{ctx->opt.wait_mode, 0, 0}, 0, f.s);
    if (w.outcome == WaitOutcome::FinishedSilent) return fail(MADICP_ERR_DEVICE, "tree build: finished without publishing its summary");
    if (w.outcome == WaitOutcome::StreamError)
      return fail(MADICP_ERR_DEVICE, std::string("tree build: ") + hipGetErrorString((hipError_t)w.stream_error));
    return MADICP_OK;
  }
  // huge clouds: three-kernel scan, summary, the State copied back
  HIP_TRY(scan_marks(f.s, f.P.leaf_start, f.n, fs.S, fs.tile_sums, &f.P.st->n_leaves));
  hipLaunchKernelGGL(tb::tb_summary, dim3(64), dim3(256), 0, f.s, f.P, kTopLevels);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(fs.h_state, f.P.st, sizeof(tb::State), hipMemcpyDeviceToHost, f.s));
  HIP_TRY(hipStreamSynchronize(f.s));
  const tb::State& h = *fs.h_state;
  hl.n_nodes = h.n_nodes.v; hl.error = h.n_nodes.error; hl.n_leaves = h.n_leaves; hl.n_top = h.n_top;
  hl.max_level = h.max_level; hl.n_valid = h.n_valid; hl.rho_bits = h.rho_bits;
  hl.pending_wave = h.q_count[next_step].v + h.team_count[next_step].v; hl.pending_quad = h.small_count[next_step].v;
  for (int i = 0; i < 3; ++i) hl.origin[i] = h.origin[i];
  return MADICP_OK;
}

// first half of a construction: everything up to the summary of step 20 is enqueued on `s`; nothing is waited for
int tree_build_begin_on(madicp_ctx* ctx, FrontScratch& fs, const double* d_xyz, int64_t n, double b_max, double b_min, hipStream_t s) {
  FrontScratch::InFlight& f = fs.fly;
  f.s = s;
  f.n = n;
  f.P = fs.P;
  f.P.cloud = d_xyz;
  f.P.n_points = static_cast<int32_t>(n);
  f.P.b_max = b_max;
  f.P.b_min = b_min;
  f.chip = n > tb::kChipMin;
  f.P.first_step = f.chip ? tb::kChipLevels : 0;
  // (State and leaf-start marks are cleared by tb_init itself)
  {  // one workgroup for the State and the root, some to clear the leaf-start marks, and (chip regime) one per chunk of the root for its sums
    const int clear_wgs = static_cast<int>(std::min<int64_t>((n + 4096) / 4096, 512));
    const int sum_wgs = f.chip ? static_cast<int>((n + tb::kChunk - 1) / tb::kChunk) : 0;
    hipLaunchKernelGGL(tb::tb_init, dim3(1 + clear_wgs + sum_wgs), dim3(256), 0, s, f.P, clear_wgs);
  }
  f.chip_grid = static_cast<int>(std::min<int64_t>(n / tb::kChunk + tb::kMaxBig, (int64_t)ctx->n_cus * 4));
  // one wave per wave-regime node (at most n / 33 of them on a level) and four lanes per small node (most levels hold far
  // fewer than the n of them this bound allows for: the queues are walked with a stride)
  f.level_grid = static_cast<int>(std::max<int64_t>(1, std::min<int64_t>((int64_t)ctx->n_cus * 8, n / (4 * (tb::kSmallMax + 1)) + n / 256 + 1)));
  f.n_tiles = static_cast<int>((n + 1 + tb::kScanTile - 1) / tb::kScanTile);
  // a 120 k-point scan at b_max = 0.2 is 17 levels deep; deeper trees (dense maps, b_max -> 0) take the loop in the second half
  f.levels_done = 20;
  // (a STEP lags the level it finishes by up to kChipLevels - 1: a small node born while the chip regime runs waits for step
  // first_step, and its descendants follow one step per level — so the steps up to last_depth + kChipLevels can hold real
  // queues and keep their grid; and a build on another cloud size than the last one forgets the hint)
  const bool similar = fs.last_n > 0 && n >= fs.last_n - fs.last_n / 8 && n <= fs.last_n + fs.last_n / 8;
  // the previous scan of this sensor was last_depth levels deep: one spare step behind it instead of the fixed twenty (a step
  // that finds its queues empty is still a launch: ~5 us) — never fewer than the breadth-first layout of the top needs
  // (kTopParts), and a deeper tree takes the loop in the second half as before
  if (similar && fs.last_depth >= 0) f.levels_done = std::min(20, std::max(fs.last_depth + 2, kTopLevels + kTopLag + 1));
  f.quiet_from = (fs.last_depth >= 0 && similar) ? fs.last_depth + tb::kChipLevels : -1;
  f.use_need = similar && fs.have_need;
  RC_TRY(tb_run_levels(fs, 0, f.levels_done));
  HIP_TRY(hipGetLastError());
  RC_TRY(tb_summary_enqueue(fs, f.levels_done, false));
  // The emission, enqueued NOW — behind the summary, without the host's 10-11 us in between — into a block sized from the
  // previous scan's leaf count: consecutive scans of one sensor differ by a few per cent.  tb_emit then takes the counts from
  // the State on the device; a tree that does not fit writes nothing and tree_build_end_on emits again (the old sequence).
  f.pre = false;
  if (similar && fs.last_leaves > 0 && f.n_tiles <= tb::kScanDirectMax) {
    const int leaf_cap = static_cast<int>(std::min<int64_t>(n, (int64_t)fs.last_leaves + fs.last_leaves / 8 + 256));
    const size_t node_cap = 2 * (size_t)leaf_cap - 1, top_cap = (size_t)kTopMax - 1;
    DevTree t;
    void* blk = nullptr;
    RC_TRY(pool_alloc(ctx, layout_tree_block(t, nullptr, node_cap, (size_t)leaf_cap, top_cap).total, s, &blk));
    layout_tree_block(t, static_cast<char*>(blk), node_cap, (size_t)leaf_cap, top_cap);
    hipLaunchKernelGGL(tb::tb_emit, dim3(((int)node_cap + 255) / 256 + ((int)top_cap + 255) / 256), dim3(256), 0, s, f.P, (int)node_cap, t.nodes,
                       t.cnodes, t.leaves, (int)top_cap, t.top_dfs, t.top_link, t.top_exit, t.top, 0.0, 0.0, 0.0, leaf_cap);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
      pool_free(ctx, blk, nullptr);
      return fail(MADICP_ERR_DEVICE, std::string("tb_emit: ") + hipGetErrorString(e));
    }
    f.pre = true;
    f.pre_leaf_cap = leaf_cap;
    f.pre_steps = f.levels_done;
    f.pre_tree = t;
  }
  f.active = true;
  return MADICP_OK;
}

// the pre-sized emission of a construction that will not use it (too small, deeper tree, error, cancel): block back to the pool
void drop_pre_tree(madicp_ctx* ctx, FrontScratch::InFlight& f) {
  if (!f.pre) return;
  EventRef after;
  if (fence_event(ctx, &after) != MADICP_OK) after = nullptr;
  pool_free(ctx, f.pre_tree.block, after);
  f.pre = false;
  f.pre_tree = DevTree{};
}

// second half: the host learns the leaf count (deeper trees: more levels first), the tree is sized, emitted, compacted
int tree_build_end_on(madicp_ctx* ctx, FrontScratch& fs, int* out_tree_id, int32_t* out_n_leaves) {
  FrontScratch::InFlight& f = fs.fly;
  hipStream_t s = f.s;
  const tb::Params& P = f.P;
  tb::HostLine& hl = *fs.h_line;
  f.active = false;  // (whatever happens below, the scratch is free again: every error path leaves the stream drained or dead)
  auto pending = [&]() { return hl.pending_wave > 0 || hl.pending_quad > 0; };
  {
    int rc = tb_summary_wait(ctx, fs, f.levels_done);
    while (rc == MADICP_OK && hl.error == 0 && f.levels_done < tb::kMaxLevels && pending()) {
      const int to = std::min(f.levels_done + 8, tb::kMaxLevels);
      rc = tb_run_levels(fs, f.levels_done, to);
      f.levels_done = to;
      if (rc == MADICP_OK) rc = tb_summary_enqueue(fs, f.levels_done, true);
      if (rc == MADICP_OK) rc = tb_summary_wait(ctx, fs, f.levels_done);
    }
    if (rc != MADICP_OK) {
      drop_pre_tree(ctx, f);
      return rc;
    }
  }
  fs.state_stale = true;
  fs.last_depth = hl.error == 0 ? hl.max_level : -1;
  fs.last_n = f.n;
  fs.last_leaves = hl.error == 0 ? hl.n_leaves : 0;
  fs.have_need = hl.error == 0 && f.n_tiles <= tb::kScanDirectMax;
  if (fs.have_need) std::memcpy(fs.last_need, hl.need, sizeof(fs.last_need));
  const bool pre_ok = f.pre && f.pre_steps == f.levels_done && hl.error == 0 && !pending() && hl.n_leaves >= 1 &&
                      hl.n_leaves <= f.pre_leaf_cap;
  if (!pre_ok) drop_pre_tree(ctx, f);
  if (hl.error == 1) return fail(MADICP_ERR_DEVICE, "tree build: node capacity exceeded");
  if (hl.error == 2 || pending()) return fail(MADICP_ERR_INVALID, "tree build: tree deeper than the supported 96 levels");
  const int32_t n_leaves = hl.n_leaves, n_nodes = 2 * hl.n_leaves - 1;
  if (n_leaves < 1 || hl.n_nodes != n_nodes || hl.n_valid != n_nodes) {
    drop_pre_tree(ctx, f);
    return fail(MADICP_ERR_DEVICE, "tree build: inconsistent node count (" + std::to_string(hl.n_nodes) + " nodes, " +
                                       std::to_string(hl.n_valid) + " finished, " + std::to_string(n_leaves) + " leaves)");
  }
  struct { int32_t n_top; unsigned long long rho_bits; double origin[3]; } st{hl.n_top, hl.rho_bits, {hl.origin[0], hl.origin[1], hl.origin[2]}};
  DevTree t;
  if (pre_ok) {  // already emitted (tree_build_begin_on), into a block with head-room
    t = f.pre_tree;
    f.pre = false;
    f.pre_tree = DevTree{};
  }
  t.n_nodes = n_nodes;
  t.n_leaves = n_leaves;
  t.n_top = std::min<int32_t>(st.n_top, kTopMax - 1);
  double rho;
  std::memcpy(&rho, &st.rho_bits, sizeof(rho));
  t.rho2 = rho;
  const size_t nt = (size_t)t.n_top;
  if (pre_ok) {
    if (!nt) t.top_exit = nullptr, t.top_dfs = nullptr, t.top_link = nullptr, t.top = nullptr;
    set_desc(t, st.origin);
  } else {
    void* blk = nullptr;
    RC_TRY(pool_alloc(ctx, layout_tree_block(t, nullptr, (size_t)n_nodes, (size_t)n_leaves, nt).total, s, &blk));
    layout_tree_block(t, static_cast<char*>(blk), (size_t)n_nodes, (size_t)n_leaves, nt);
    set_desc(t, st.origin);
    // ONE launch: the DFS-preorder node array, the screening / dense leaf records and the staged top (tree_build.hip.h)
    hipLaunchKernelGGL(tb::tb_emit, dim3((n_nodes + 255) / 256 + (t.n_top + 255) / 256), dim3(256), 0, s, P, n_nodes, t.nodes, t.cnodes, t.leaves,
                       t.n_top, t.top_dfs, t.top_link, t.top_exit, t.top, st.origin[0], st.origin[1], st.origin[2], 0);
  }
  hipError_t e = hipGetLastError();
  int rc = MADICP_OK;
  if (e == hipSuccess && rc == MADICP_OK) e = hipEventCreateWithFlags(&t.ready, hipEventDisableTiming);
  if (e == hipSuccess && rc == MADICP_OK) e = hipEventRecord(t.ready, s);
  // a tree from the build stream: the copy stream feeds registrations from trees it believes it produced itself
  // (moving_from_leaves, transforms' staging), so it is put behind the event once, here
  if (e == hipSuccess && rc == MADICP_OK && s != ctx->copy) e = hipStreamWaitEvent(ctx->copy, t.ready, 0);
  if (e != hipSuccess || rc != MADICP_OK) {
    hipStreamSynchronize(s);
    release_tree(ctx, t, nullptr);
    return rc != MADICP_OK ? rc : fail(MADICP_ERR_DEVICE, std::string("tree build: ") + hipGetErrorString(e));
  }
  const int id = ctx->next_id++;
  ctx->trees[id] = t;
  *out_tree_id = id;
  if (out_n_leaves) *out_n_leaves = n_leaves;
  return MADICP_OK;
}

}  // namespace

extern "C" {

int madicp_tree_build(madicp_ctx* ctx, int cloud_id, double b_max, double b_min, int* out_tree_id, int32_t* out_n_leaves) {
  if (!ctx || !out_tree_id) return fail(MADICP_ERR_INVALID, "null argument");
  DevCloud* c = find_cloud(ctx, cloud_id);
  if (!c) return fail(MADICP_ERR_INVALID, "unknown cloud id");
  RC_TRY(busy_with_lookahead(ctx));
  HIP_TRY(hipSetDevice(ctx->device));
  FrontScratch* fs = nullptr;
  RC_TRY(ensure_scratch(ctx, c->n, &fs));
  fs->fly.lookahead = false;
  RC_TRY(tree_build_begin_on(ctx, *fs, c->xyz, c->n, b_max, b_min, ctx->copy));
  return tree_build_end_on(ctx, *fs, out_tree_id, out_n_leaves);
}

int madicp_tree_build_begin(madicp_ctx* ctx, const double* xyz, int64_t n, double b_max, double b_min) {
  if (!ctx || !xyz) return fail(MADICP_ERR_INVALID, "null argument");
  if (n < 1 || n > 0x3fffffff) return fail(MADICP_ERR_INVALID, "a cloud holds 1 .. 2^30 points");
  RC_TRY(busy_with_lookahead(ctx));
  HIP_TRY(hipSetDevice(ctx->device));
  {
    // The look-ahead pays when construction and registration run BACK TO BACK on the device (the runtime's default hardware
    // queue map: 0.78 -> 0.65 ms per frame) and not when they run side by side and slow each other down — which is what
    // GPU_MAX_HW_QUEUES > 4 gives (0.82 -> 0.82: DESIGN.md 9.4, bench.py's lookahead_in_a_plain_process).  A multi-rank process
    // wants the many queues for its collectives: said once, so that the combination is a decision and not an accident.
    static bool warned = false;
    const char* q = std::getenv("GPU_MAX_HW_QUEUES");
    if (!warned && q && std::atoi(q) > 4) {
      warned = true;
      std::fprintf(stderr, "madicp: a look-ahead tree build was begun with GPU_MAX_HW_QUEUES=%s: measured on MI355X, the look-ahead "
                           "shortens a frame under the runtime's default queue map (0.78 -> 0.65 ms) and does not with more than four "
                           "hardware queues (0.82 -> 0.82 ms); without prefetch() the frame is the same either way\n", q);
    }
  }
  if (!ctx->build) {
    // MADICP_BUILD_CUS=<n> (experiment): the look-ahead construction only gets the first n CUs, so that its level
    // kernels cannot spread over the CUs a registration round wants all of — whatever hardware queues the runtime maps the two
    // streams to
    // (a measurement aid: only in the measurement build, -DMADICP_MEASURE)
#ifdef MADICP_MEASURE
    const char* e = std::getenv("MADICP_BUILD_CUS");
    const int n_build = e ? std::atoi(e) : 0;
#else
    const int n_build = 0;
#endif
    if (n_build > 0 && n_build < ctx->n_cus) {
      const int words = (ctx->n_cus + 31) / 32;
      std::vector<uint32_t> mask((size_t)words, 0u);
      for (int cu = 0; cu < n_build; ++cu) mask[(size_t)cu / 32] |= 1u << (cu % 32);
      if (hipExtStreamCreateWithCUMask(&ctx->build, (uint32_t)words, mask.data()) != hipSuccess) {
        (void)hipGetLastError();
        ctx->build = nullptr;
      }
    }
    if (!ctx->build) HIP_TRY(hipStreamCreateWithFlags(&ctx->build, hipStreamNonBlocking));
  }
  FrontScratch* fs = nullptr;
  RC_TRY(ensure_scratch(ctx, n, &fs));
  hipStream_t s = ctx->build;
  // the scratch's previous users ran on the copy stream (ingest, deskew, a synchronous build's tail): behind them
  {
    EventRef ev;
    RC_TRY(fence_event(ctx, &ev));
    HIP_TRY(hipStreamWaitEvent(s, ev->ev_copy, 0));
  }
  // the scan: staged through the pinned buffers the uploads share, copied on the BUILD stream
  DevCloud c;
  {
    void* p = nullptr;
    RC_TRY(pool_alloc(ctx, sizeof(double) * 3 * (size_t)n, s, &p));
    c.xyz = static_cast<double*>(p);
    c.n = n;
  }
  {
    const int rc = stage_and_send_cloud(ctx, xyz, n, c.xyz, s);
    if (rc != MADICP_OK) return drop_cloud(ctx, c, rc);
  }
  // Option "build_after_registration" (experiment, default off): the construction's KERNELS wait for whatever the compute stream
  // holds right now — the registration this look-ahead was begun beside.  Built to test the hypothesis that the look-ahead
  // cliff (0.67 ms per frame in one process configuration, 1.5 in the others) is the two kernel sets fighting for the CUs;
  // measured: it is not — with the construction strictly behind the registration the other configurations stay at 1.5-2.1 ms
  // (profiles/r5_lookahead_matrix.md).
  if (ctx->opt.build_after_registration) {
    if (!ctx->ev_build_gate) CLOUD_TRY(hipEventCreateWithFlags(&ctx->ev_build_gate, hipEventDisableTiming));
    CLOUD_TRY(hipEventRecord(ctx->ev_build_gate, ctx->stream));
    CLOUD_TRY(hipStreamWaitEvent(s, ctx->ev_build_gate, 0));
  }
  fs->fly.lookahead = true;
  const int rc = tree_build_begin_on(ctx, *fs, c.xyz, n, b_max, b_min, s);
  if (rc != MADICP_OK) {
    hipStreamSynchronize(s);
    return drop_cloud(ctx, c, rc);
  }
  fs->fly.cloud = c;
  return MADICP_OK;
}

int madicp_tree_build_end(madicp_ctx* ctx, int* out_tree_id, int32_t* out_n_leaves) {
  if (!ctx || !out_tree_id) return fail(MADICP_ERR_INVALID, "null argument");
  if (!ctx->front || !ctx->front->scratch.fly.active || !ctx->front->scratch.fly.lookahead)
    return fail(MADICP_ERR_INVALID, "no look-ahead tree build in flight");
  HIP_TRY(hipSetDevice(ctx->device));
  FrontScratch& fs = ctx->front->scratch;
  const int rc = tree_build_end_on(ctx, fs, out_tree_id, out_n_leaves);
  // the level kernels — the only readers of the scan — are behind the summary the host has just seen (or the stream is drained)
  DevCloud c = fs.fly.cloud;
  fs.fly.cloud = DevCloud{};
  if (rc != MADICP_OK) hipStreamSynchronize(fs.fly.s);
  return drop_cloud(ctx, c, rc);
}

int madicp_tree_build_cancel(madicp_ctx* ctx) {
  if (!ctx) return fail(MADICP_ERR_INVALID, "ctx is null");
  if (!ctx->front || !ctx->front->scratch.fly.active || !ctx->front->scratch.fly.lookahead) return MADICP_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  FrontScratch& fs = ctx->front->scratch;
  const hipError_t e = hipStreamSynchronize(fs.fly.s);
  fs.fly.active = false;
  fs.state_stale = true;
  drop_pre_tree(ctx, fs.fly);
  DevCloud c = fs.fly.cloud;
  fs.fly.cloud = DevCloud{};
  drop_cloud(ctx, c, MADICP_OK);
  if (e != hipSuccess) return fail(MADICP_ERR_DEVICE, std::string("tree build: ") + hipGetErrorString(e));
  return MADICP_OK;
}

int madicp_tree_info(madicp_ctx* ctx, int tree_id, int32_t* out_n_nodes, int32_t* out_n_leaves) {
  if (!ctx) return fail(MADICP_ERR_INVALID, "ctx is null");
  auto it = ctx->trees.find(tree_id);
  if (it == ctx->trees.end()) return fail(MADICP_ERR_INVALID, "unknown tree id");
  if (out_n_nodes) *out_n_nodes = it->second.n_nodes;
  if (out_n_leaves) *out_n_leaves = it->second.n_leaves;
  return MADICP_OK;
}

// Diagnostics (tests): the points of the last synchronous build on this context in the order the construction left them —
// every leaf's members in the order the splits above it produced (reference: the caller's container after MADtree::build,
// mad_tree.cpp:95-97 with utils.h:37-52, except that the reference also overwrites a leaf's first member with its
// representative, mad_tree.cpp:76-84).  Valid until the next build, ingest or deskew on the context.
#ifdef MADICP_MEASURE
int madicp_debug_tree_build_points(madicp_ctx* ctx, double* out_xyz, int64_t n) {
  if (!ctx || !out_xyz) return fail(MADICP_ERR_INVALID, "null argument");
  if (!ctx->front || !ctx->front->scratch.block || !ctx->front->scratch.h_line) return fail(MADICP_ERR_INVALID, "no build yet");
  RC_TRY(busy_with_lookahead(ctx));
  FrontScratch& fs = ctx->front->scratch;
  const tb::Params& P = fs.fly.P;
  if (n != P.n_points) return fail(MADICP_ERR_INVALID, "n is not the size of the last build's cloud");
  HIP_TRY(hipSetDevice(ctx->device));
  void* d_out = nullptr;
  RC_TRY(pool_alloc(ctx, sizeof(double) * 3 * (size_t)n, ctx->copy, &d_out));
  const int n_nodes = fs.h_line->n_nodes;
  hipLaunchKernelGGL(tb::tb_debug_order, dim3((n_nodes + 3) / 4), dim3(256), 0, ctx->copy, P, n_nodes, static_cast<double*>(d_out));
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(out_xyz, d_out, sizeof(double) * 3 * (size_t)n, hipMemcpyDeviceToHost, ctx->copy);
  const hipError_t e2 = hipStreamSynchronize(ctx->copy);
  pool_free(ctx, d_out, nullptr);
  if (e != hipSuccess || e2 != hipSuccess)
    return fail(MADICP_ERR_DEVICE, std::string("tree build points: ") + hipGetErrorString(e != hipSuccess ? e : e2));
  return MADICP_OK;
}

// Diagnostics (tests): the rho a tree's screening test runs with (TreeDesc::rho, kernels.hip.h: it has to bound |m - o|_1 of
// every internal node, whoever made it — validate_nodes on the host, the builder's atomicMax, a chain of transforms).
int madicp_debug_tree_rho(madicp_ctx* ctx, int tree_id, double* out_rho) {
  if (!ctx || !out_rho) return fail(MADICP_ERR_INVALID, "null argument");
  auto it = ctx->trees.find(tree_id);
  if (it == ctx->trees.end()) return fail(MADICP_ERR_INVALID, "unknown tree id");
  *out_rho = it->second.desc.rho;
  return MADICP_OK;
}
#endif  // MADICP_MEASURE

// per-level node counts of the last build on this context (diagnostics for tests / tools): out[0] = levels reached,
// out[1] = lane-regime sub-trees, then 2 x 64 ints: wave-regime and chip-regime nodes per level
int madicp_tree_build_stats(madicp_ctx* ctx, int32_t out[130]) {
  if (!ctx || !out) return fail(MADICP_ERR_INVALID, "null argument");
  if (!ctx->front || !ctx->front->scratch.h_state || !ctx->front->scratch.block) return fail(MADICP_ERR_INVALID, "no build yet");
  RC_TRY(busy_with_lookahead(ctx));
  FrontScratch& fs = ctx->front->scratch;
  if (fs.state_stale) {  // (a build publishes one line to the host; the per-level counters are fetched when asked for)
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(fs.h_state, fs.P.st, sizeof(tb::State), hipMemcpyDeviceToHost, ctx->copy));
    HIP_TRY(hipStreamSynchronize(ctx->copy));
    fs.state_stale = false;
  }
  const tb::State& st = *fs.h_state;
  out[0] = st.max_level;
  int lanes = 0;
  for (int i = 0; i <= tb::kMaxLevels; ++i) lanes += st.small_count[i].v;
  out[1] = lanes;
  for (int i = 0; i < 64; ++i) {
    out[2 + i] = st.q_count[i].v;
    out[66 + i] = st.big_count[i].v;
  }
#ifdef MADICP_TB_CHECK
  out[129] = st.n_nodes.pad_[0];  // development: mismatches counted by the in-kernel self-check
#endif
  return MADICP_OK;
}

}  // extern "C"

#ifdef MADICP_TB_STAMPS
// development only (tools/tb_stamps.py): reset / fetch the per-wave wall-clock stamps of tb_level
extern "C" int madicp_debug_tb_stamps(madicp_ctx* ctx, unsigned long long* out, int reset) {
  if (!ctx) return MADICP_ERR_INVALID;
  hipStreamSynchronize(ctx->copy);
  const size_t bytes = sizeof(unsigned long long) * 24 * 512 * 4 * 16;
  if (reset) {
    std::vector<unsigned long long> init(24 * 512 * 4 * 16, 0ull);
    return hipMemcpyToSymbol(HIP_SYMBOL(madicp::tb::g_tb_stamps), init.data(), bytes) == hipSuccess ? 0 : MADICP_ERR_DEVICE;
  }
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(madicp::tb::g_tb_stamps), bytes) == hipSuccess ? 0 : MADICP_ERR_DEVICE;
}
#endif
