// mesh_clean_plan.h -- the host arithmetic behind the launches of mesh_clean.hip, in one place: the rows of a dilation tile that
// fit the LDS budget next to their halo, the workgroup counts, the refusal conditions of a structuring element, and the iteration
// caps of the union-find.  Integers only: no HIP, no device, no state -- a plain C++17 compiler accepts this header, and
// tests/host/mesh_clean_plan_check.cpp runs it under the address and undefined-behaviour sanitizers.
#pragma once
#include <cstdint>

namespace psdf {
namespace mesh_clean_plan {

constexpr int PLAN_OK = 0, PLAN_ERR_ARG = -1, PLAN_ERR_UNSUPPORTED = -2;

// the row distance is a byte: the distance along the row to the nearest set pixel, HD_FAR when it is HD_FAR or more (or there is
// none).  A half-width of HD_FAR would accept "no set pixel in this row" -- hence the largest half-width accepted.
constexpr int HD_FAR = 255;
constexpr int MAX_HALF_WIDTH = 254;
// a dilation workgroup owns TILE_COLS columns (one lane each: four waves, eight packed words per row) and stages
// tile_rows + 2 r rows of row distances, one byte each, in LDS_BYTES of LDS
constexpr int TILE_COLS = 256;
constexpr int LDS_BYTES = 64 * 1024;
constexpr int LDS_ROWS = LDS_BYTES / TILE_COLS;
// rows of the structuring element: at least one output row has to fit next to the halo
constexpr int MAX_ELEMENT_ROWS = LDS_ROWS - 1;   // odd: r <= 127
// rows of an image per workgroup of the row-distance kernel: one wave each
constexpr int ROWS_PER_GROUP = 4;
// next to the tile, every wave of a dilation workgroup keeps one bit per staged row ("this row can hit in my 64 columns")
// and the workgroup a copy of the half-widths, one byte per row of the element
constexpr int LIVE_WORDS = LDS_ROWS / 64;
constexpr int LIVE_BYTES = ROWS_PER_GROUP * LIVE_WORDS * 8 + LDS_ROWS;
// entities numbered with int32 on the device
constexpr int64_t MAX_COUNT = 0x7fffffffll;

struct DilatePlan {
  int status;               // PLAN_OK, or why there is no plan (every other field 0)
  int radius;               // r: the element has 2 r + 1 rows
  int tile_rows;            // output rows per workgroup: min(LDS_ROWS - 2 r, H)
  int staged_rows;          // tile_rows + 2 r <= LDS_ROWS
  int tiles_x, tiles_y;     // tiles per view
  int words_per_row;        // ceil(W / 32)
  int64_t workgroups;       // n * tiles_y * tiles_x, of the dilation
  int64_t row_groups;       // ceil(n * H / ROWS_PER_GROUP), of the row distance
};

// n views of H x W; half_widths [count]: the half-width of every row of the element, top to bottom
inline DilatePlan dilate_plan(int64_t n, int64_t H, int64_t W, const int* half_widths, int64_t count) {
  DilatePlan p{};
  p.status = PLAN_ERR_ARG;
  if (n < 0 || H < 1 || W < 1 || !half_widths || count < 1 || (count & 1) == 0) return p;
  for (int64_t k = 0; k < count && k <= MAX_ELEMENT_ROWS; k++)
    if (half_widths[k] < 0 || half_widths[k] > MAX_HALF_WIDTH) return p;
  p.status = PLAN_ERR_UNSUPPORTED;
  if (count > MAX_ELEMENT_ROWS || H > MAX_COUNT || W > MAX_COUNT - TILE_COLS) return p;
  const int r = (int)(count / 2);
  const int64_t room = LDS_ROWS - 2 * r;
  const int tile_rows = (int)(room < H ? room : H);
  const int64_t tiles_x = (W + TILE_COLS - 1) / TILE_COLS, tiles_y = (H + tile_rows - 1) / tile_rows;
  // (n * tiles and n * H stay far below 2^63: each factor is below 2^31 and the products are checked one at a time)
  if (tiles_x * tiles_y > MAX_COUNT || (n > 0 && tiles_x * tiles_y > MAX_COUNT / n)) return p;
  if (n > 0 && (H + ROWS_PER_GROUP - 1) / ROWS_PER_GROUP > MAX_COUNT / n) return p;
  p.status = PLAN_OK;
  p.radius = r;
  p.tile_rows = tile_rows;
  p.staged_rows = tile_rows + 2 * r;
  p.tiles_x = (int)tiles_x;
  p.tiles_y = (int)tiles_y;
  p.words_per_row = (int)((W + 31) / 32);
  p.workgroups = n * tiles_x * tiles_y;
  p.row_groups = (n * H + ROWS_PER_GROUP - 1) / ROWS_PER_GROUP;
  return p;
}

// The union-find keeps parent[i] <= i, so a walk to the root from node i visits strictly decreasing indices: at most i + 1 <= n
// of them, whatever other threads do meanwhile.  A hook by compare-and-swap fails only when another thread hooked the same root
// first, and a forest over n nodes takes n - 1 hooks in all.  Both loops are therefore done within n + 1 rounds when the
// structure is sound; a thread that exceeds the cap raises the error flag instead of spinning.
inline int64_t union_find_cap(int64_t n) { return (n < 0 ? 0 : n) + 1; }

}  // namespace mesh_clean_plan
}  // namespace psdf
