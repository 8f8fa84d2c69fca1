// Stand-alone check of permuto_sdf_amd/csrc/neus_render_plan.h: host-only integer arithmetic, compiled as plain C++17 with
// -fsanitize=address,undefined -fno-sanitize-recover=all by tests/test_neus_render_host.py and run as a program of its own.  Every
// count is swept over the borders of its formula (the register chunks, the single-group limit, a workgroup, the grid cap, the
// largest count the ABI takes) and held against the formula written out a second time, with wide integers.
#include <cstdio>

#include "neus_render_plan.h"

namespace plan = psdf::neus_render_plan;

static int failures = 0;
#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) {                                                        \
      if (failures < 20) fprintf(stderr, "line %d: %s\n", __LINE__, #cond); \
      failures++;                                                         \
    }                                                                     \
  } while (0)

int main() {
  // ---- register chunks of the ray backward: the smallest K in {1, 2, 4} with 64 K >= max_per_ray
  for (int n = -3; n <= 300; n++) {
    const int K = plan::chunks(n);
    if (n < 1) CHECK(K == plan::PLAN_ERR_ARG);
    else if (n > 256) CHECK(K == plan::PLAN_ERR_UNSUPPORTED);
    else {
      CHECK(K == 1 || K == 2 || K == 4);
      CHECK(64 * K >= n);
      CHECK(K == 1 || 64 * (K / 2) < n);
    }
  }
  CHECK(plan::chunks(64) == 1 && plan::chunks(65) == 2 && plan::chunks(128) == 2 && plan::chunks(129) == 4 && plan::chunks(256) == 4);
  CHECK(plan::chunks(257) == plan::PLAN_ERR_UNSUPPORTED && plan::chunks(1) == 1 && plan::chunks(0) == plan::PLAN_ERR_ARG);
  CHECK(plan::chunks(0x7fffffff) == plan::PLAN_ERR_UNSUPPORTED && plan::chunks(-0x7fffffff - 1) == plan::PLAN_ERR_ARG);

  // ---- the loss tail: one workgroup up to the single-group limit (the trainer's cap of 8192 rays lies inside it), above it a
  // capped grid with a workspace of TERMS doubles per workgroup and a finishing launch
  const int64_t lim = plan::SINGLE_GROUP_RAYS;
  CHECK(lim == (int64_t)plan::BLOCK * plan::RAYS_PER_THREAD_SINGLE && lim >= 8192);
  const int64_t pass = (int64_t)plan::BLOCK * plan::MAX_GRID;
  const int64_t rays[] = {0, 1, 63, 255, 256, 257, 512, lim - 1, lim, lim + 1, pass - 1, pass, pass + 1, 3 * pass + 5, plan::MAX_RAYS - 1,
                          plan::MAX_RAYS};
  for (int64_t R : rays) {
    const plan::LossPlan p = plan::loss_plan(R);
    CHECK(p.status == plan::PLAN_OK);
    if (R == 0) {
      CHECK(p.grid == 0 && p.finish == 0 && p.workspace_bytes == 0);
    } else if (R <= lim) {
      CHECK(p.grid == 1 && p.finish == 0 && p.workspace_bytes == 0);
      CHECK((__int128)plan::BLOCK * plan::RAYS_PER_THREAD_SINGLE >= R);       // a thread walks at most 32 rays
    } else {
      const __int128 groups = ((__int128)R + plan::BLOCK - 1) / plan::BLOCK;
      CHECK(p.finish == 1 && p.grid == (int)(groups < plan::MAX_GRID ? groups : plan::MAX_GRID));
      CHECK(p.grid > 1 && p.grid <= plan::MAX_GRID);
      CHECK(p.workspace_bytes == (int64_t)p.grid * plan::TERMS * 8);
      CHECK((__int128)p.grid * plan::BLOCK >= (R < pass ? R : pass));         // threads first + k * grid * BLOCK cover [0, R)
    }
    CHECK(3 * (__int128)R <= 0x7fffffff);           // the colour entries stay an int
  }
  CHECK(plan::loss_plan(lim).grid == 1 && plan::loss_plan(lim).workspace_bytes == 0);
  CHECK(plan::loss_plan(lim + 1).grid == 33 && plan::loss_plan(lim + 1).workspace_bytes == 33 * 16 && plan::loss_plan(lim + 1).finish == 1);
  CHECK(plan::loss_plan(-1).status == plan::PLAN_ERR_ARG && plan::loss_plan(-1).grid == 0 && plan::loss_plan(-1).workspace_bytes == 0);
  CHECK(plan::loss_plan(INT64_MIN).status == plan::PLAN_ERR_ARG);
  CHECK(plan::loss_plan(plan::MAX_RAYS + 1).status == plan::PLAN_ERR_UNSUPPORTED && plan::loss_plan(INT64_MAX).status == plan::PLAN_ERR_UNSUPPORTED);

  if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
  else printf("neus_render_plan_check: all checks passed\n");
  return failures ? 1 : 0;
}
