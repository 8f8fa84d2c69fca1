// Stand-alone check of permuto_sdf_amd/csrc/mesh_clean_plan.h: includes nothing else of the project, is compiled by
// tests/test_mesh_clean_host.py with -fsanitize=address,undefined -fno-sanitize-recover=all and compares the plans with values
// derived by hand.
#include <cstdio>
#include <vector>

#include "mesh_clean_plan.h"

using namespace psdf::mesh_clean_plan;

static int failures = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      fprintf(stderr, "line %d: %s is false\n", __LINE__, #cond);    \
      failures++;                                                    \
    }                                                                \
  } while (0)

int main() {
  static_assert(LDS_ROWS == 256 && MAX_ELEMENT_ROWS == 255 && TILE_COLS == 256 && MAX_HALF_WIDTH == 254 && HD_FAR == 255 &&
                LIVE_WORDS == 4 && LIVE_BYTES == 384, "");
  {   // the protocol's case: 64 views of 1200 x 1600 under 101 rows.  r = 50, 256 - 100 = 156 output rows per tile,
      // ceil(1200 / 156) = 8 and ceil(1600 / 256) = 7 tiles, 50 words per row, 64 * 56 workgroups, 64 * 1200 / 4 row groups
    std::vector<int> hw(101, 50);
    const DilatePlan p = dilate_plan(64, 1200, 1600, hw.data(), 101);
    CHECK(p.status == PLAN_OK && p.radius == 50 && p.tile_rows == 156 && p.staged_rows == 256);
    CHECK(p.tiles_x == 7 && p.tiles_y == 8 && p.words_per_row == 50 && p.workgroups == 3584 && p.row_groups == 19200);
    // an image shorter than the tile: its 150 rows and the 100 of halo
    const DilatePlan q = dilate_plan(3, 150, 200, hw.data(), 101);
    CHECK(q.status == PLAN_OK && q.tile_rows == 150 && q.staged_rows == 250 && q.tiles_x == 1 && q.tiles_y == 1);
    CHECK(q.words_per_row == 7 && q.workgroups == 3 && q.row_groups == 113);
    hw[7] = 255;
    CHECK(dilate_plan(3, 150, 200, hw.data(), 101).status == PLAN_ERR_ARG);
    hw[7] = -1;
    CHECK(dilate_plan(3, 150, 200, hw.data(), 101).status == PLAN_ERR_ARG);
    hw[7] = 254;
    CHECK(dilate_plan(3, 150, 200, hw.data(), 101).status == PLAN_OK);
  }
  {   // one pixel, one row
    const int hw = 0;
    const DilatePlan p = dilate_plan(1, 1, 1, &hw, 1);
    CHECK(p.status == PLAN_OK && p.radius == 0 && p.tile_rows == 1 && p.staged_rows == 1 && p.tiles_x == 1 && p.tiles_y == 1);
    CHECK(p.words_per_row == 1 && p.workgroups == 1 && p.row_groups == 1);
    const DilatePlan w = dilate_plan(2, 7, 33, &hw, 1);
    CHECK(w.status == PLAN_OK && w.words_per_row == 2 && w.tile_rows == 7 && w.workgroups == 2 && w.row_groups == 4);
    const DilatePlan none = dilate_plan(0, 7, 33, &hw, 1);
    CHECK(none.status == PLAN_OK && none.workgroups == 0 && none.row_groups == 0);
    CHECK(dilate_plan(-1, 7, 33, &hw, 1).status == PLAN_ERR_ARG);
    CHECK(dilate_plan(1, 0, 33, &hw, 1).status == PLAN_ERR_ARG);
    CHECK(dilate_plan(1, 7, 0, &hw, 1).status == PLAN_ERR_ARG);
    CHECK(dilate_plan(1, 7, 33, nullptr, 1).status == PLAN_ERR_ARG);
    CHECK(dilate_plan(1, 7, 33, &hw, 0).status == PLAN_ERR_ARG);
    // 7 x 5 tiles of 256 x 256 for every one of 2^31 - 1 views: more workgroups than a launch numbers
    CHECK(dilate_plan(0x7fffffffll, 1200, 1600, &hw, 1).status == PLAN_ERR_UNSUPPORTED);
    CHECK(dilate_plan(1, 0x80000000ll, 4, &hw, 1).status == PLAN_ERR_UNSUPPORTED);
  }
  {   // the tallest element: 255 rows leave two output rows per tile; 257 do not fit; an even count has no centre
    std::vector<int> hw(257, 3);
    const DilatePlan p = dilate_plan(1, 7, 300, hw.data(), 255);
    CHECK(p.status == PLAN_OK && p.radius == 127 && p.tile_rows == 2 && p.staged_rows == 256 && p.tiles_y == 4 && p.tiles_x == 2);
    CHECK(p.workgroups == 8 && p.words_per_row == 10);
    CHECK(dilate_plan(1, 7, 300, hw.data(), 257).status == PLAN_ERR_UNSUPPORTED);
    CHECK(dilate_plan(1, 7, 300, hw.data(), 2).status == PLAN_ERR_ARG);
  }
  CHECK(union_find_cap(0) == 1 && union_find_cap(5) == 6 && union_find_cap(-3) == 1 && union_find_cap(0x7fffffffll) == 0x80000000ll);
  if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
  else printf("mesh_clean_plan_check: all checks passed\n");
  return failures != 0;
}
