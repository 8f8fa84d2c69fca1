// Stand-alone check of permuto_sdf_amd/csrc/mesh_color_plan.h as plain C++17: the rows of the colour network's input for the real
// net, the chunk arithmetic at the edges of a chunk and beyond 2^31 vertices, and the refusals.  tests/test_mesh_color_host.py
// builds it with -fsanitize=address,undefined -fno-sanitize-recover=all and runs it: an overflowing product or a shift too far is
// a sanitizer report.
#include "mesh_color_plan.h"

#include <cstdio>
#include <initializer_list>

namespace plan = psdf::mesh_color_plan;

static int failures = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      fprintf(stderr, "line %d: %s\n", __LINE__, #cond);              \
      failures++;                                                     \
    }                                                                 \
  } while (0)

static void chunk_case(int64_t n, int64_t chunk, int64_t want_count, int64_t want_last) {
  int64_t count = -7, last = -7;
  CHECK(plan::chunks(n, chunk, &count, &last) == plan::PLAN_OK);
  CHECK(count == want_count);
  CHECK(last == want_last);
  // the chunks cover [0, n) exactly, every one of them non-empty and no larger than `chunk`
  if (count > 0) {
    CHECK(last >= 1 && last <= chunk);
    CHECK((count - 1) * chunk + last == n);
  } else {
    CHECK(n == 0 && last == 0);
  }
}

int main() {
  // the real net: a 24-level lattice with 2 features per level and the 3 coordinates appended, 25 SH values, the normal, 32
  // geometry features (models.py:349-350: 111 inputs)
  {
    plan::Rows r{};
    CHECK(plan::rows(24 * 2 + 3, 32, &r) == plan::PLAN_OK);
    CHECK(r.c_enc == 51 && r.c_sh == 76 && r.c_normal == 79 && r.c_geom == 111 && r.C == 111);
    // ... and with the points as a zero-padded pseudo-level (52 channels)
    CHECK(plan::rows(52, 32, &r) == plan::PLAN_OK);
    CHECK(r.c_enc == 52 && r.c_sh == 77 && r.c_normal == 80 && r.c_geom == 112 && r.C == 112);
    CHECK(plan::rows(1, 0, &r) == plan::PLAN_OK);
    CHECK(r.c_enc == 1 && r.c_sh == 26 && r.c_normal == 29 && r.c_geom == 29 && r.C == 29);
    CHECK(plan::SH == 25 && plan::NORMAL == 3 && plan::SH_DEGREE == 5 && plan::BLOCK % 64 == 0);
    CHECK(plan::rows(0, 32, &r) == plan::PLAN_ERR_ARG && plan::rows(-1, 32, &r) == plan::PLAN_ERR_ARG);
    CHECK(plan::rows(51, -1, &r) == plan::PLAN_ERR_ARG && plan::rows(51, 32, nullptr) == plan::PLAN_ERR_ARG);
    CHECK(plan::rows(plan::MAX_ROWS, 0, &r) == plan::PLAN_ERR_UNSUPPORTED);
    CHECK(plan::rows(0x7fffffff, 0x7fffffff, &r) == plan::PLAN_ERR_UNSUPPORTED);      // (a 64-bit sum: no int overflow)
    CHECK(plan::rows(plan::MAX_ROWS - 28, 0, &r) == plan::PLAN_OK && r.C == plan::MAX_ROWS);
  }
  // chunks
  for (int64_t chunk : {(int64_t)1, (int64_t)2, (int64_t)256, (int64_t)1 << 18, plan::MAX_LAUNCH}) {
    chunk_case(0, chunk, 0, 0);
    chunk_case(1, chunk, 1, 1);
    if (chunk > 1) chunk_case(chunk - 1, chunk, 1, chunk - 1);
    chunk_case(chunk, chunk, 1, chunk);
    chunk_case(chunk + 1, chunk, 2, 1);
    const int64_t big = ((int64_t)1 << 31) + 5;
    chunk_case(big, chunk, big / chunk + (big % chunk != 0), big % chunk ? big % chunk : chunk);
  }
  chunk_case(((int64_t)1 << 31) + 5, (int64_t)1 << 18, 8193, 5);
  chunk_case(600, 256, 3, 88);
  chunk_case(0x7fffffffffffffffll, plan::MAX_LAUNCH, 0x7fffffffffffffffll / plan::MAX_LAUNCH + 1, 0x7fffffffffffffffll % plan::MAX_LAUNCH);
  {
    int64_t count = 0, last = 0;
    CHECK(plan::chunks(-1, 256, &count, &last) == plan::PLAN_ERR_ARG);
    CHECK(plan::chunks(5, 0, &count, &last) == plan::PLAN_ERR_ARG && plan::chunks(5, -3, &count, &last) == plan::PLAN_ERR_ARG);
    CHECK(plan::chunks(5, 2, nullptr, &last) == plan::PLAN_ERR_ARG && plan::chunks(5, 2, &count, nullptr) == plan::PLAN_ERR_ARG);
    CHECK(plan::chunks(5, plan::MAX_LAUNCH + 1, &count, &last) == plan::PLAN_ERR_UNSUPPORTED);
  }
  // the grid of a launch
  CHECK(plan::grid(1) == 1 && plan::grid(256) == 1 && plan::grid(257) == 2 && plan::grid(plan::MAX_LAUNCH) == 8388608);
  CHECK(plan::grid(0) == plan::PLAN_ERR_ARG && plan::grid(-5) == plan::PLAN_ERR_ARG);
  CHECK(plan::grid(plan::MAX_LAUNCH + 1) == plan::PLAN_ERR_UNSUPPORTED);
  // the whole plan: C against the width the colour MLP takes
  {
    plan::Plan p{};
    CHECK(plan::plan(51, 32, 111, 600, 256, &p) == plan::PLAN_OK);
    CHECK(p.r.C == 111 && p.r.c_enc == 51 && p.nr_chunks == 3 && p.last_chunk == 88);
    CHECK(plan::plan(51, 32, 111, 0, 256, &p) == plan::PLAN_OK && p.nr_chunks == 0 && p.last_chunk == 0);
    CHECK(plan::plan(51, 32, 112, 600, 256, &p) == plan::PLAN_ERR_ARG);      // another width than the MLP's
    CHECK(plan::plan(52, 32, 111, 600, 256, &p) == plan::PLAN_ERR_ARG);
    CHECK(plan::plan(51, 32, 111, -1, 256, &p) == plan::PLAN_ERR_ARG && plan::plan(51, 32, 111, 600, 0, &p) == plan::PLAN_ERR_ARG);
    CHECK(plan::plan(51, 32, 111, 600, 256, nullptr) == plan::PLAN_ERR_ARG);
    CHECK(plan::plan(51, 32, 111, 600, plan::MAX_LAUNCH + 1, &p) == plan::PLAN_ERR_UNSUPPORTED);
  }
  if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
  else printf("mesh_color_plan_check: all checks passed\n");
  return failures ? 1 : 0;
}
