// Where everything lies in a device voxel map (madicp_map_*), decided on the host alone: the column list, the byte offsets of a
// block's columns, and the scratch the two removals lay over a fresh block's table region.  No HIP in here: plain C++17, checked on
// the CPU by tests/cpp/map_layout_check.cpp; frontend_capi.inc.h takes every pointer into a map's block from these functions and
// loops over kMapColumnTable wherever rows move (growth, the removal log, the downloads).
//
// A map owns ONE device block for `cap` rows and 2 cap table slots, the columns it has side by side in the order of MapColumn,
// each starting at a multiple of its element size (which only ever pads in front of `mom`), absent columns taking no room:
//   keys | owner                     the table: 24 bytes per row of capacity, emptied by ONE memset to all ones
//   row_keys | xyz | attr | ev       what the rows hold, in row order (attr: madicp_map_create_attr, ev: madicp_map_create_ev)
//   slot_row | stamp                 per table slot: the row of its key (evidence or moments), the last fold that hit it (evidence)
//   closed_at | mom                  the rows' freeze words and ten moment words (madicp_map_create_mom)
// 44 bytes per row of capacity, 48 with attr; + 20 with evidence; + 84 with moments on an evidence map, + 92 without evidence.
#pragma once
#include <stddef.h>

namespace madicp {

enum MapColumn { kColKeys, kColOwner, kColRowKeys, kColXyz, kColAttr, kColEv, kColSlotRow, kColStamp, kColClosedAt, kColMom, kMapColumns };

struct MapColumnInfo {
  const char* name;
  size_t elem;  // bytes per element
  size_t per;   // elements per row (a row column) or per table slot (a table column)
  bool row;     // a row column moves with the rows (growth, compaction); a table column is wiped and refilled (map_rehash)
  bool logged;  // ... and the removal log (madicp_map_track_removed) carries it
  size_t bytes() const { return elem * per; }
};
inline constexpr MapColumnInfo kMapColumnTable[kMapColumns] = {
    {"keys", 8, 1, false, false}, {"owner", 4, 1, false, false},    {"row_keys", 8, 1, true, true},   {"xyz", 4, 3, true, true},
    {"attr", 4, 1, true, true},   {"ev", 4, 1, true, false},        {"slot_row", 4, 1, false, false}, {"stamp", 4, 1, false, false},
    {"closed_at", 4, 1, true, false}, {"mom", 8, 10, true, false},
};
constexpr size_t kMapTableBytesPerRow = 2 * (8 + 4);  // keys | owner of the two slots per row of capacity

constexpr unsigned map_bit(MapColumn c) { return 1u << c; }
// the columns a map has: slot_row with evidence or with moments
constexpr unsigned map_columns(bool with_attr, bool with_ev, bool with_mom) {
  return map_bit(kColKeys) | map_bit(kColOwner) | map_bit(kColRowKeys) | map_bit(kColXyz) | (with_attr ? map_bit(kColAttr) : 0u) |
         (with_ev ? map_bit(kColEv) | map_bit(kColStamp) : 0u) | (with_ev || with_mom ? map_bit(kColSlotRow) : 0u) |
         (with_mom ? map_bit(kColClosedAt) | map_bit(kColMom) : 0u);
}

struct MapLayout {
  unsigned columns = 0;           // bit c: column c is there
  size_t off[kMapColumns] = {};   // an absent column: where it would start (it takes no room)
  size_t bytes = 0;
  bool has(int c) const { return (columns >> c) & 1u; }
};

// the columns of `columns` for `rows` rows and `slots` table slots, side by side
inline MapLayout map_layout_of(size_t rows, size_t slots, unsigned columns) {
  MapLayout L;
  L.columns = columns;
  for (int c = 0; c < kMapColumns; ++c) {
    const MapColumnInfo& I = kMapColumnTable[c];
    if (L.has(c)) L.bytes = (L.bytes + I.elem - 1) / I.elem * I.elem;
    L.off[c] = L.bytes;
    if (L.has(c)) L.bytes += I.bytes() * (I.row ? rows : slots);
  }
  return L;
}
// a map's block
inline MapLayout map_layout(size_t cap, bool with_attr, bool with_ev, bool with_mom) {
  return map_layout_of(cap, 2 * cap, map_columns(with_attr, with_ev, with_mom));
}
// a removal log's block for `log_cap` entries: the logged columns of a map
inline MapLayout map_log_layout(size_t log_cap, bool with_attr) {
  unsigned logged = 0;
  for (int c = 0; c < kMapColumns; ++c)
    if (kMapColumnTable[c].logged) logged |= 1u << c;
  return map_layout_of(log_cap, 0, logged & map_columns(with_attr, false, false));
}

// ---- the scratch of a removal of M rows (1 <= M <= cap), laid over the FRESH block's table region until the memset that makes it a
// table: byte offsets of 32-bit words.  mark and S hold M + 1 words (the scan's terminator), tile_sums one per scan tile, total one.
struct MapScratch {
  size_t flags = 0, mark = 0, S = 0, tile_sums = 0, total = 0, bytes = 0;
  int tiles = 0;
};
constexpr int map_scan_tiles(size_t M, int scan_tile) { return static_cast<int>((M + 1 + scan_tile - 1) / scan_tile); }
// madicp_map_prune:   mark | S | tile_sums | total — 8 (M + 1) + 4 tiles + 4 bytes
inline MapScratch map_prune_scratch(size_t /*cap*/, size_t M, int scan_tile) {
  MapScratch s;
  s.tiles = map_scan_tiles(M, scan_tile);
  s.S = 4 * (M + 1);
  s.tile_sums = s.S + 4 * (M + 1);
  s.total = s.tile_sums + 4 * (size_t)s.tiles;
  s.bytes = s.total + 4;
  return s;
}
// madicp_map_clear_rays:   flags (one per slot of the LIVE table: 2 cap) | mark | tile_sums | total, and S laid over the flags, which
// are dead once the marks are made (M + 1 <= 2 cap) — 8 cap + 4 (M + 1) + 4 tiles + 4 bytes
inline MapScratch map_clear_scratch(size_t cap, size_t M, int scan_tile) {
  MapScratch s;
  s.tiles = map_scan_tiles(M, scan_tile);
  s.mark = 4 * 2 * cap;
  s.tile_sums = s.mark + 4 * (M + 1);
  s.total = s.tile_sums + 4 * (size_t)s.tiles;
  s.bytes = s.total + 4;
  return s;
}

}  // namespace madicp
