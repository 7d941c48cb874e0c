// CPU check of mad_icp_amd/csrc/common/map_layout.h — where the columns of a device voxel map lie in its block, and where the two
// removals lay their scratch over a fresh block's table region.  The expected offsets are the formulae of the map_block_alloc the
// header replaced, transcribed; the memory-safety facts that code only argued in a comment (columns disjoint and aligned, both
// scratch overlays within the 24 cap bytes of the table region) are checked for every column combination and capacity below.
// Test infrastructure; compiled and run by tests/test_map_layout.py.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "map_layout.h"

using namespace madicp;

namespace {

long g_checks = 0, g_failed = 0;

void expect(bool ok, const char* what, size_t cap, int combo, size_t a = 0, size_t b = 0) {
  ++g_checks;
  if (ok) return;
  if (++g_failed <= 20) std::printf("FAILED %s: cap %zu attr/ev/mom %d%d%d  (%zu, %zu)\n", what, cap, combo & 1, (combo >> 1) & 1, combo >> 2, a, b);
}

// the block layout as map_block_alloc computed it before the header existed
void check_block(size_t c, bool with_attr, bool with_ev, bool with_mom, int combo) {
  const MapLayout L = map_layout(c, with_attr, with_ev, with_mom);
  const size_t row_bytes = with_attr ? 48 : 44;
  const bool with_slot_row = with_ev || with_mom;
  const size_t closed_off = (row_bytes + (with_ev ? 12 : 0) + (with_slot_row ? 8 : 0)) * c;
  const size_t mom_off = (closed_off + 4 * c + 7) & ~size_t(7);
  const bool present[kMapColumns] = {true, true, true, true, with_attr, with_ev, with_slot_row, with_ev, with_mom, with_mom};
  const size_t want[kMapColumns] = {0,
                                    16 * c,
                                    24 * c,
                                    32 * c,
                                    44 * c,
                                    row_bytes * c,
                                    (row_bytes + (with_ev ? 4 : 0)) * c,
                                    (row_bytes + 12) * c,
                                    closed_off,
                                    mom_off};
  for (int k = 0; k < kMapColumns; ++k) {
    expect(L.has(k) == present[k], kMapColumnTable[k].name, c, combo, L.has(k), present[k]);
    if (present[k]) expect(L.off[k] == want[k], kMapColumnTable[k].name, c, combo, L.off[k], want[k]);
  }
  expect(L.bytes == (with_mom ? mom_off + 80 * c : closed_off), "block bytes", c, combo, L.bytes, with_mom ? mom_off + 80 * c : closed_off);

  // ascending, disjoint, aligned to the element size; an absent column takes no room
  size_t end = 0;
  for (int k = 0; k < kMapColumns; ++k) {
    const MapColumnInfo& I = kMapColumnTable[k];
    const size_t bytes = I.bytes() * (I.row ? c : 2 * c);
    expect(L.off[k] >= end, "ascending and disjoint", c, combo, L.off[k], end);
    if (!L.has(k)) {
      expect(k + 1 == kMapColumns ? L.off[k] == L.bytes : L.off[k + 1] == L.off[k], "an absent column takes no room", c, combo, k, L.off[k]);
      continue;
    }
    expect(L.off[k] % I.elem == 0, "aligned to its element", c, combo, L.off[k], I.elem);
    end = L.off[k] + bytes;
  }
  expect(end == L.bytes, "the last column ends the block", c, combo, end, L.bytes);
  expect(kMapColumnTable[kColKeys].elem == 8 && kMapColumnTable[kColRowKeys].elem == 8 && kMapColumnTable[kColMom].elem == 8,
         "64-bit columns", c, combo);
  expect(L.off[kColRowKeys] == kMapTableBytesPerRow * c, "the table region is 24 cap bytes", c, combo, L.off[kColRowKeys], 24 * c);

  // the documented bytes per row of capacity (pipeline.h, README.md): 24 for the table, then ...
  const size_t per_row = (with_attr ? 24 : 20) + (with_ev ? 20 : 0) + (with_mom ? (with_ev ? 84 : 92) : 0);
  expect(L.bytes >= (24 + per_row) * c && L.bytes <= (24 + per_row) * c + 7, "documented bytes per row", c, combo, L.bytes, (24 + per_row) * c);

  // the removal log: keys | xyz | attr, 20 or 24 bytes an entry
  const MapLayout G = map_log_layout(c, with_attr);
  expect(G.columns == (map_bit(kColRowKeys) | map_bit(kColXyz) | (with_attr ? map_bit(kColAttr) : 0u)), "log columns", c, combo, G.columns);
  expect(G.off[kColRowKeys] == 0 && G.off[kColXyz] == 8 * c && G.off[kColAttr] == 20 * c && G.bytes == (with_attr ? 24 : 20) * c, "log layout", c,
         combo, G.bytes);
}

struct Span {
  size_t at, bytes;
};
bool disjoint(const Span& a, const Span& b) { return a.at + a.bytes <= b.at || b.at + b.bytes <= a.at; }

// both overlays for a removal of M rows of a map of capacity cap
void check_scratch(size_t cap, size_t M, int tile) {
  const size_t tiles = (M + 1 + tile - 1) / tile;
  const MapScratch P = map_prune_scratch(cap, M, tile), C = map_clear_scratch(cap, M, tile);
  expect((size_t)P.tiles == tiles && (size_t)C.tiles == tiles, "scan tiles", cap, tile, P.tiles, tiles);
  // prune: mark | S | tile_sums | total
  const Span p[4] = {{P.mark, 4 * (M + 1)}, {P.S, 4 * (M + 1)}, {P.tile_sums, 4 * tiles}, {P.total, 4}};
  for (int i = 0; i < 4; ++i)
    for (int j = i + 1; j < 4; ++j) expect(disjoint(p[i], p[j]), "prune scratch disjoint", cap, tile, M, 4 * i + j);
  expect(P.mark == 0 && P.S == 4 * (M + 1) && P.tile_sums == 8 * (M + 1) && P.total == 8 * (M + 1) + 4 * tiles, "prune scratch as it was", cap,
         tile, M);
  expect(P.bytes == P.total + 4 && P.bytes <= 24 * cap, "prune scratch within the table region", cap, tile, M, P.bytes);
  // clearing: flags | mark | tile_sums | total, S over the flags
  const Span c[4] = {{C.flags, 4 * 2 * cap}, {C.mark, 4 * (M + 1)}, {C.tile_sums, 4 * tiles}, {C.total, 4}};
  for (int i = 0; i < 4; ++i)
    for (int j = i + 1; j < 4; ++j) expect(disjoint(c[i], c[j]), "clearing scratch disjoint", cap, tile, M, 4 * i + j);
  const Span S = {C.S, 4 * (M + 1)};
  expect(S.at == C.flags && S.bytes <= c[0].bytes, "S lies within the flags", cap, tile, M, S.bytes);
  for (int j = 1; j < 4; ++j) expect(disjoint(S, c[j]), "S overlaps the flags only", cap, tile, M, j);
  expect(C.flags == 0 && C.mark == 8 * cap && C.tile_sums == 8 * cap + 4 * (M + 1) && C.total == C.tile_sums + 4 * tiles,
         "clearing scratch as it was", cap, tile, M);
  expect(C.bytes == C.total + 4 && C.bytes <= 24 * cap, "clearing scratch within the table region", cap, tile, M, C.bytes);
}

}  // namespace

int main() {
  std::vector<size_t> caps;
  for (size_t c = 1; c <= 70; ++c) caps.push_back(c);
  for (size_t c : {size_t(4095), size_t(4096), size_t(4097), size_t(1) << 18, size_t(1) << 24}) caps.push_back(c);
  for (size_t cap : caps) {
    for (int combo = 0; combo < 8; ++combo) check_block(cap, combo & 1, (combo >> 1) & 1, combo >> 2, combo);
    // scan tile 4096, and 1024: the tile of the scan the map's removals run (tb::kScanTile)
    for (int tile : {4096, 1024}) {
      if (cap <= 70)
        for (size_t M = 1; M <= cap; ++M) check_scratch(cap, M, tile);
      else
        for (size_t M : {size_t(1), cap - 1, cap}) check_scratch(cap, M, tile);
    }
  }
  std::printf("%ld checks, %ld failed\n", g_checks, g_failed);
  if (g_failed == 0) std::printf("map layout ok\n");
  return g_failed == 0 ? 0 : 1;
}
