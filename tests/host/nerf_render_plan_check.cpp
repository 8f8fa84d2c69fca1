// Stand-alone check of permuto_sdf_amd/csrc/nerf_render_plan.h: host-only integer arithmetic, compiled as plain C++17 with
// -fsanitize=address,undefined -fno-sanitize-recover=all by tests/test_nerf_host.py and run as a program of its own.  Every count
// is swept over the borders of its formula (a workgroup, the grid cap, the register chunks, the largest count the ABI takes) and
// held against the formula written out a second time, with wide integers.
#include <cstdio>
#include <initializer_list>

#include "nerf_render_plan.h"

namespace plan = psdf::nerf_render_plan;

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
  CHECK(plan::chunks(0x7fffffff) == plan::PLAN_ERR_UNSUPPORTED && plan::chunks(-0x7fffffff - 1) == plan::PLAN_ERR_ARG);

  // ---- the loss reduce
  const int64_t pass = plan::RAYS_PER_PASS;
  CHECK(pass == (int64_t)plan::BLOCK * plan::MAX_GRID);
  const int64_t rays[] = {0, 1, 63, 255, 256, 257, 512, pass - 1, pass, pass + 1, 3 * pass + 5, plan::MAX_RAYS - 1, plan::MAX_RAYS};
  for (int64_t R : rays) {
    const plan::LossPlan p = plan::loss_plan(R);
    CHECK(p.status == plan::PLAN_OK);
    const __int128 groups = ((__int128)R + plan::BLOCK - 1) / plan::BLOCK;
    CHECK(p.grid == (int)(groups < plan::MAX_GRID ? groups : plan::MAX_GRID));
    CHECK(p.grid >= 0 && p.grid <= plan::MAX_GRID && (R == 0) == (p.grid == 0));
    CHECK(p.workspace_bytes == (int64_t)p.grid * plan::TERMS * 8);
    // every ray is walked: threads first + k * grid * BLOCK cover [0, R)
    if (p.grid > 0) CHECK((__int128)p.grid * plan::BLOCK >= (R < pass ? R : pass));
    CHECK(3 * (__int128)R <= 0x7fffffff);           // the colour entries stay an int
  }
  CHECK(plan::loss_plan(512).grid == 2 && plan::loss_plan(512).workspace_bytes == 32);
  CHECK(plan::loss_plan(-1).status == plan::PLAN_ERR_ARG && plan::loss_plan(-1).grid == 0 && plan::loss_plan(-1).workspace_bytes == 0);
  CHECK(plan::loss_plan(INT64_MIN).status == plan::PLAN_ERR_ARG);
  CHECK(plan::loss_plan(plan::MAX_RAYS + 1).status == plan::PLAN_ERR_UNSUPPORTED && plan::loss_plan(INT64_MAX).status == plan::PLAN_ERR_UNSUPPORTED);

  // ---- the head join: (tiles of BLOCK samples) x (row groups), one-dimensional
  CHECK(plan::FWD_GROUPS * plan::ROWS_PER_GROUP == plan::FEAT + plan::SH && plan::BWD_GROUPS * plan::ROWS_PER_GROUP == plan::FEAT);
  CHECK(plan::FEAT % plan::ROWS_PER_GROUP == 0);   // no group holds features and harmonics
  const int64_t samples[] = {0, 1, 63, 64, 65, 255, 256, 257, 1000, 16384, plan::MAX_SAMPLES};
  for (int64_t M : samples)
    for (int groups : {plan::FWD_GROUPS, plan::BWD_GROUPS}) {
      const int64_t g = plan::join_grid(M, groups);
      const __int128 want = (((__int128)M + plan::BLOCK - 1) / plan::BLOCK) * groups;
      CHECK(g == (int64_t)want && g >= 0 && g <= 0xffffffffll);
      CHECK((__int128)(g / groups) * plan::BLOCK >= M);
    }
  CHECK(plan::join_grid(1000, plan::FWD_GROUPS) == 40 && plan::join_grid(1000, plan::BWD_GROUPS) == 32);
  CHECK(plan::join_grid(-1, plan::FWD_GROUPS) == plan::PLAN_ERR_ARG && plan::join_grid(5, 0) == plan::PLAN_ERR_ARG);
  CHECK(plan::join_grid(plan::MAX_SAMPLES + 1, plan::FWD_GROUPS) == plan::PLAN_ERR_UNSUPPORTED);
  CHECK(plan::join_grid(INT64_MAX, plan::FWD_GROUPS) == plan::PLAN_ERR_UNSUPPORTED);
  CHECK(plan::join_grid(plan::MAX_SAMPLES, 1024) == plan::PLAN_ERR_UNSUPPORTED);      // a grid beyond 2^32 - 1

  if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
  else printf("nerf_render_plan_check: all checks passed\n");
  return failures ? 1 : 0;
}
