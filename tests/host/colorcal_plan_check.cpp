// Stand-alone check of permuto_sdf_amd/csrc/colorcal_plan.h: host-only integer arithmetic, compiled as plain C++17 with
// -fsanitize=address,undefined -fno-sanitize-recover=all by tests/test_colorcal_host.py and run as a program of its own.  Every
// count is swept over the borders of its formula (a row, a workgroup, the grid cap, the largest count the ABI takes) and held
// against the formula written out a second time, with wide integers.
#include <climits>
#include <cstdio>

#include "colorcal_plan.h"

namespace plan = psdf::colorcal_plan;

static int failures = 0;
#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) {                                                        \
      if (failures < 20) fprintf(stderr, "line %d: %s\n", __LINE__, #cond); \
      failures++;                                                         \
    }                                                                     \
  } while (0)

int main() {
  // ---- a ray is a row of 16 lanes: rows tile the wave and the workgroup
  CHECK(plan::ROW == 16 && 64 % plan::ROW == 0 && plan::BLOCK % 64 == 0 && plan::RAYS_PER_BLOCK * plan::ROW == plan::BLOCK);
  CHECK(plan::COLS == 6 && plan::COLS <= plan::ROW);     // lane j < COLS of a row writes column j
  const int cap = plan::MAX_RAY_GRID * plan::RAYS_PER_BLOCK;
  const int rays[] = {1, 15, 16, 17, 255, 256, 257, 512, cap - 1, cap, cap + 1, 3 * cap + 5, plan::MAX_RAYS - 1, plan::MAX_RAYS};
  for (int R : rays) {
    const int g = plan::ray_grid(R);
    const __int128 want = ((__int128)R + plan::RAYS_PER_BLOCK - 1) / plan::RAYS_PER_BLOCK;
    CHECK(g == (int)(want < plan::MAX_RAY_GRID ? want : plan::MAX_RAY_GRID) && g >= 1);
    // rows first + k * grid * RAYS_PER_BLOCK cover [0, R), and the counter of a row stays an int one step past the end
    CHECK((__int128)g * plan::RAYS_PER_BLOCK >= (R < cap ? R : cap));
    const __int128 passes = ((__int128)R + (__int128)g * plan::RAYS_PER_BLOCK - 1) / ((__int128)g * plan::RAYS_PER_BLOCK);
    CHECK(passes * g * plan::RAYS_PER_BLOCK + plan::RAYS_PER_BLOCK <= (__int128)INT_MAX + 1);
    CHECK((__int128)R + (__int128)g * plan::RAYS_PER_BLOCK <= INT_MAX);
  }
  CHECK(plan::ray_grid(512) == 32 && plan::ray_grid(1) == 1 && plan::ray_grid(17) == 2);
  CHECK(plan::ray_grid(0) == plan::PLAN_ERR_ARG && plan::ray_grid(-1) == plan::PLAN_ERR_ARG && plan::ray_grid(INT_MIN) == plan::PLAN_ERR_ARG);
  CHECK(plan::ray_grid(plan::MAX_RAYS + 1) == plan::PLAN_ERR_UNSUPPORTED && plan::ray_grid(INT_MAX) == plan::PLAN_ERR_UNSUPPORTED);

  // ---- the counts
  CHECK(plan::check_counts(0, 1, 0) == plan::PLAN_OK && plan::check_counts(212, 4, 3) == plan::PLAN_OK);
  CHECK(plan::check_counts(plan::MAX_SAMPLES, plan::MAX_IMAGES, plan::MAX_IMAGES - 1) == plan::PLAN_OK);
  CHECK(3 * (__int128)plan::MAX_SAMPLES <= INT_MAX);
  CHECK(plan::check_counts(-1, 4, 0) == plan::PLAN_ERR_ARG && plan::check_counts(INT64_MIN, 4, 0) == plan::PLAN_ERR_ARG);
  CHECK(plan::check_counts(1, 0, 0) == plan::PLAN_ERR_ARG && plan::check_counts(1, -5, 0) == plan::PLAN_ERR_ARG);
  CHECK(plan::check_counts(1, 4, -1) == plan::PLAN_ERR_ARG && plan::check_counts(1, 4, 4) == plan::PLAN_ERR_ARG);
  CHECK(plan::check_counts(plan::MAX_SAMPLES + 1, 4, 0) == plan::PLAN_ERR_UNSUPPORTED && plan::check_counts(INT64_MAX, 4, 0) == plan::PLAN_ERR_UNSUPPORTED);
  CHECK(plan::check_counts(1, plan::MAX_IMAGES + 1, 0) == plan::PLAN_ERR_UNSUPPORTED && plan::check_counts(1, INT_MAX, 0) == plan::PLAN_ERR_UNSUPPORTED);

  // ---- the fold: one thread per (image, column)
  const int images[] = {1, 4, 42, 43, 49, 256, 1000, plan::MAX_IMAGES};
  for (int I : images) {
    const int g = plan::fold_grid(I);
    const __int128 want = ((__int128)I * plan::COLS + plan::BLOCK - 1) / plan::BLOCK;
    CHECK(g == (int)want && (__int128)g * plan::BLOCK >= (__int128)I * plan::COLS && g >= 1);
  }
  CHECK(plan::fold_grid(4) == 1 && plan::fold_grid(42) == 1 && plan::fold_grid(43) == 2);
  CHECK(plan::fold_grid(0) == plan::PLAN_ERR_ARG && plan::fold_grid(-1) == plan::PLAN_ERR_ARG);
  CHECK(plan::fold_grid(plan::MAX_IMAGES + 1) == plan::PLAN_ERR_UNSUPPORTED && plan::fold_grid(INT_MAX) == plan::PLAN_ERR_UNSUPPORTED);

  if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
  else printf("colorcal_plan_check: all checks passed\n");
  return failures ? 1 : 0;
}
