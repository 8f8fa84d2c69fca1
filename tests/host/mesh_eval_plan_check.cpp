// Stand-alone check of permuto_sdf_amd/csrc/mesh_eval_plan.h: no HIP, no device, its own main.  tests/test_mesh_eval_host.py
// compiles it with -fsanitize=address,undefined -fno-sanitize-recover=all and runs it.  Every expected value below was derived
// by hand from the rules the header states (the numbers are chosen so that every edge is exact in fp32); exit status = failed
// checks.
#include <cstdio>

#include "mesh_eval_plan.h"

using namespace psdf::mesh_eval_plan;

static int failures = 0;

static void check(bool ok, const char* what) {
  if (!ok) {
    failures++;
    fprintf(stderr, "FAILED: %s\n", what);
  }
}
#define CHECK(...) check((__VA_ARGS__), #__VA_ARGS__)

static GridPlan cube(double lo, double hi, int64_t n, double min_edge, int64_t budget) {
  const double a[3] = {lo, lo, lo}, b[3] = {hi, hi, hi};
  return grid_plan(a, b, n, min_edge, budget);
}

int main() {
  // a degenerate box: all points equal.  With a radius the edge is radius x (1 + 1/512), one cell
  {
    const double p[3] = {1.0, 2.0, 3.0};
    const GridPlan g = grid_plan(p, p, 5, 0.25, DEFAULT_CELL_BUDGET);
    CHECK(g.status == PLAN_OK && g.edge == 0.25048828125f && g.cells == 1);
    CHECK(g.dims[0] == 1 && g.dims[1] == 1 && g.dims[2] == 1);
    CHECK(g.origin[0] == 1.f && g.origin[1] == 2.f && g.origin[2] == 3.f);
  }
  // one point, no radius: one cell of edge 1
  {
    const double p[3] = {-7.5, 0.0, 2.0};
    const GridPlan g = grid_plan(p, p, 1, 0.0, DEFAULT_CELL_BUDGET);
    CHECK(g.status == PLAN_OK && g.edge == 1.f && g.cells == 1 && g.origin[0] == -7.5f);
    CHECK(query_blocks(g.dims) == 1);
  }
  // the radius decides: box 10^3, 1 000 points (4 x 600 / 1000 = 2.4 -> 1.549 per cell would be wider: take 10 000 points, 0.49)
  {
    const GridPlan g = cube(0.0, 10.0, 10000, 1.0, DEFAULT_CELL_BUDGET);
    CHECK(g.status == PLAN_OK && g.edge == 1.001953125f);
    CHECK(g.dims[0] == 10 && g.dims[1] == 10 && g.dims[2] == 10 && g.cells == 1000);   // floor(10 / 1.00195) + 1
  }
  // the point count decides: box 100^3, area 6 x 10^4, 960 000 points: sqrt(4 x 6 x 10^4 / 960 000) = 0.5; 201^3 cells
  {
    const GridPlan g = cube(0.0, 100.0, 960000, 0.0, DEFAULT_CELL_BUDGET);
    CHECK(g.status == PLAN_OK && g.edge == 0.5f && g.dims[0] == 201 && g.cells == 8120601);
    // ... and the budget forces it coarser: 0.625 -> 161^3, 0.78125 -> 129^3, 0.9765625 -> 103^3 = 1 092 727, 1.220703125 -> 82^3
    const GridPlan c = cube(0.0, 100.0, 960000, 0.0, 1000000);
    CHECK(c.status == PLAN_OK && c.edge == 1.220703125f && c.dims[0] == 82 && c.dims[1] == 82 && c.dims[2] == 82);
    CHECK(c.cells == 551368 && c.cells <= 1000000);
    CHECK(blocks_of(82) == 21 && query_blocks(c.dims) == 9261);
    // a budget of one cell: a single cell whatever the box
    const GridPlan one = cube(0.0, 100.0, 960000, 0.0, 1);
    CHECK(one.status == PLAN_OK && one.cells == 1 && one.edge > 100.f);
  }
  // a long thin cloud: 10^6 / 2048 = 488.28125 gives 2049 cells on x, one step coarser (610.3515625) gives 1639
  {
    const double a[3] = {0.0, 0.0, 0.0}, b[3] = {1e6, 0.0, 0.0};
    const GridPlan g = grid_plan(a, b, 10, 0.0, DEFAULT_CELL_BUDGET);
    CHECK(g.status == PLAN_OK && g.edge == 610.3515625f && g.dims[0] == 1639 && g.dims[1] == 1 && g.dims[2] == 1 && g.cells == 1639);
  }
  // point counts at and past the int32 limit; no points; bad boxes
  CHECK(cube(0.0, 1.0, MAX_POINTS, 0.0, DEFAULT_CELL_BUDGET).status == PLAN_OK);
  CHECK(MAX_POINTS == 2147483647ll);
  CHECK(cube(0.0, 1.0, MAX_POINTS + 1, 0.0, DEFAULT_CELL_BUDGET).status == PLAN_ERR_UNSUPPORTED);
  CHECK(cube(0.0, 1.0, (int64_t)1 << 40, 0.0, DEFAULT_CELL_BUDGET).cells == 0);
  CHECK(cube(0.0, 1.0, 0, 0.0, DEFAULT_CELL_BUDGET).status == PLAN_ERR_ARG);
  CHECK(cube(1.0, 0.0, 10, 0.0, DEFAULT_CELL_BUDGET).status == PLAN_ERR_ARG);
  CHECK(cube(0.0, NAN, 10, 0.0, DEFAULT_CELL_BUDGET).status == PLAN_ERR_ARG);
  CHECK(cube(0.0, 1.0, 10, -1.0, DEFAULT_CELL_BUDGET).status == PLAN_ERR_ARG);
  CHECK(cube(0.0, 1.0, 10, 0.0, 0).status == PLAN_ERR_ARG);
  // a budget past int32 is clamped: the cells stay below the key that marks a non-finite point
  {
    const GridPlan g = cube(0.0, 2047.0, MAX_POINTS, 1.0 / EDGE_MARGIN, (int64_t)1 << 40);
    CHECK(g.status == PLAN_OK && g.cells <= MAX_CELLS && g.dims[0] <= MAX_DIM);
  }
  CHECK(TILE_CAPACITY >= 256 && TILE_CAPACITY % 256 == 0 && TILE_CAPACITY * 16 <= 64 * 1024);
  CHECK(blocks_of(1) == 1 && blocks_of(4) == 1 && blocks_of(5) == 2 && blocks_of(MAX_DIM) == MAX_DIM / 4);
  if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
  else printf("mesh_eval_plan_check: all checks passed\n");
  return failures;
}
