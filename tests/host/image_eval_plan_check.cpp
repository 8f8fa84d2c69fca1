// Stand-alone check of permuto_sdf_amd/csrc/image_eval_plan.h: no HIP, no device, its own main.  tests/test_image_eval_host.py
// compiles it with -fsanitize=address,undefined -fno-sanitize-recover=all and runs it.  The expected values below were derived by
// hand from the rules the header states (the factors are Python's own round(min_side / 256)); exit status = failed checks.
#include <cstdio>

#include "image_eval_plan.h"

using namespace psdf::image_eval_plan;

static int failures = 0;

static void check(bool ok, const char* what) {
  if (!ok) {
    failures++;
    fprintf(stderr, "FAILED: %s\n", what);
  }
}
#define CHECK(...) check((__VA_ARGS__), #__VA_ARGS__)

int main() {
  // the pooling factor: ties go to the even neighbour (384 / 256 = 1.5 -> 2, 640 / 256 = 2.5 -> 2, 896 / 256 = 3.5 -> 4)
  {
    const int side[] = {1, 11, 255, 256, 383, 384, 385, 639, 640, 641, 895, 896, 897, 1200, 1408, 1920};
    const int want[] = {1, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 4, 4, 5, 6, 8};   // 1408 / 256 = 5.5 -> 6, 1920 / 256 = 7.5 -> 8
    for (int i = 0; i < 16; i++) CHECK(pooling_factor(side[i]) == want[i]);
    CHECK(pooling_factor(0x7fffffff) == 8388608);   // (2^31 - 1) / 256 = 8388607 remainder 255
  }
  // four 1200 x 1600 RGB views: f = 5, 240 x 320 pooled, 230 x 310 map, 15 x 10 tiles of 16 x 32, 3 x 150 partials per image
  {
    const Plan p = plan(4, 3, 1200, 1600, 11, true);
    CHECK(p.status == PLAN_OK && p.factor == 5 && p.ph == 240 && p.pw == 320 && p.mh == 230 && p.mw == 310);
    CHECK(p.tiles_y == 15 && p.tiles_x == 10 && p.ssim_partials == 450 && p.ssim_workspace_bytes == 4 * 450 * 8);
    CHECK(p.sq_partials == 938 && p.sq_workspace_bytes == 4 * 938 * 8);   // 1 920 000 / 2048 = 937.5
    const Plan q = plan(4, 3, 1200, 1600, 11, false);
    CHECK(q.status == PLAN_OK && q.factor == 1 && q.ph == 1200 && q.mh == 1190 && q.mw == 1590 && q.tiles_y == 75 && q.tiles_x == 50);
  }
  // remainders are dropped: 390 / 2 = 195, 641 / 3 = 213, 650 / 3 = 216
  {
    const Plan a = plan(1, 1, 384, 390, 11, true);
    CHECK(a.status == PLAN_OK && a.factor == 2 && a.ph == 192 && a.pw == 195 && a.mh == 182 && a.mw == 185);
    CHECK(a.tiles_y == 12 && a.tiles_x == 6 && a.ssim_partials == 72);
    const Plan b = plan(1, 3, 641, 650, 11, true);
    CHECK(b.status == PLAN_OK && b.factor == 3 && b.ph == 213 && b.pw == 216 && b.mh == 203 && b.mw == 206);
    CHECK(b.tiles_y == 13 && b.tiles_x == 7 && b.ssim_partials == 3 * 91);
  }
  // the smallest image, and the edges of a tile
  {
    const Plan one = plan(1, 1, 11, 11, 11, true);
    CHECK(one.status == PLAN_OK && one.mh == 1 && one.mw == 1 && one.tiles_y == 1 && one.tiles_x == 1 && one.sq_partials == 1);
    CHECK(plan(1, 1, TILE_H + 10, TILE_W + 10, 11, true).tiles_y == 1 && plan(1, 1, TILE_H + 10, TILE_W + 10, 11, true).tiles_x == 1);
    CHECK(plan(1, 1, TILE_H + 11, TILE_W + 10, 11, true).tiles_y == 2 && plan(1, 1, TILE_H + 10, TILE_W + 11, 11, true).tiles_x == 2);
    CHECK(plan(2, 1, 3 * TILE_H + 11, 3 * TILE_W + 11, 11, true).ssim_partials == 16);
    CHECK(plan(0, 3, 64, 64, 11, true).status == PLAN_OK && plan(0, 3, 64, 64, 11, true).ssim_workspace_bytes == 0);
    CHECK(sq_partials(1, 1) == 1 && sq_partials(1, 2048) == 1 && sq_partials(1, 2049) == 2 && sq_partials(0, 5) == -1);
  }
  // refusals: a pooled side shorter than the window, an even window, a window the tile does not hold, no image
  CHECK(plan(1, 3, 10, 100, 11, true).status == PLAN_ERR_ARG);
  CHECK(plan(1, 3, 100, 10, 11, true).status == PLAN_ERR_ARG);
  CHECK(plan(1, 3, 100, 100, 10, true).status == PLAN_ERR_ARG);
  CHECK(plan(1, 3, 100, 100, 0, true).status == PLAN_ERR_ARG);
  CHECK(plan(1, 3, 100, 100, MAX_KERNEL, true).status == PLAN_OK);
  CHECK(plan(1, 3, 100, 100, MAX_KERNEL + 2, true).status == PLAN_ERR_ARG);
  CHECK(plan(-1, 3, 100, 100, 11, true).status == PLAN_ERR_ARG && plan(1, 0, 100, 100, 11, true).status == PLAN_ERR_ARG);
  CHECK(plan(1, 3, 0, 100, 11, true).status == PLAN_ERR_ARG && plan(1, 3, 100, 0, 11, true).status == PLAN_ERR_ARG);
  // more workgroups than a launch has
  CHECK(plan((int64_t)1 << 31, 1, 11, 11, 11, true).status == PLAN_ERR_UNSUPPORTED);
  CHECK(plan(MAX_GRID, 1, 11, 11, 11, true).status == PLAN_OK);
  CHECK(plan(MAX_GRID, 2, 11, 11, 11, true).status == PLAN_ERR_UNSUPPORTED);
  CHECK(plan(3, 0x7fffffff, 0x7fffffff, 0x7fffffff, 11, false).status == PLAN_ERR_UNSUPPORTED);
  // the window: normalised, symmetric, the Gaussian's ratios
  {
    double w[MAX_KERNEL];
    CHECK(gaussian_weights(11, 1.5, w));
    double sum = 0;
    for (int i = 0; i < 11; i++) sum += w[i];
    CHECK(std::fabs(sum - 1.0) <= 4e-16);
    for (int i = 0; i < 5; i++) CHECK(w[i] == w[10 - i] && w[i] < w[i + 1]);
    CHECK(std::fabs(w[4] / w[5] - std::exp(-1.0 / 4.5)) <= 4e-16 && std::fabs(w[0] / w[5] - std::exp(-25.0 / 4.5)) <= 4e-16);
    CHECK(std::fabs(w[5] - 0.26601172486179436) <= 1e-15);   // 1 / sum of exp(-d^2 / 4.5), d = -5 .. 5
    CHECK(gaussian_weights(1, 1.5, w) && w[0] == 1.0);
    CHECK(gaussian_weights(MAX_KERNEL, 0.5, w) && w[0] > 0.0);
    CHECK(!gaussian_weights(10, 1.5, w) && !gaussian_weights(MAX_KERNEL + 2, 1.5, w) && !gaussian_weights(11, 0.0, w));
    CHECK(!gaussian_weights(11, NAN, w) && !gaussian_weights(11, INFINITY, w));
  }
  // two workgroups of the SSIM kernel share a CU's 160 KiB of LDS
  CHECK(LDS_BYTES <= 64 * 1024 && 2 * LDS_BYTES <= 160 * 1024);
  CHECK(TILE_H * TILE_W % BLOCK == 0 && SQ_PIXELS == 2048);
  if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
  else printf("image_eval_plan_check: all checks passed\n");
  return failures;
}
