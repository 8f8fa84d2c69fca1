// mesh_eval_plan.h -- the host arithmetic behind the launches of mesh_eval.hip, in one place: the uniform grid that bins a point
// cloud (origin, cell edge, dimensions, cell count), its refusal conditions and the capacity of the LDS tile of the cooperative
// nearest-neighbour kernel.  Integers, floats and doubles only: no HIP, no device, no state -- a plain C++17 compiler accepts this
// header, and tests/host/mesh_eval_plan_check.cpp runs it under the address and undefined-behaviour sanitizers.
#pragma once
#include <cmath>
#include <cstdint>

namespace psdf {
namespace mesh_eval_plan {

constexpr int PLAN_OK = 0, PLAN_ERR_ARG = -1, PLAN_ERR_UNSUPPORTED = -2;

// reference points per LDS tile of the cooperative kernel: 16 bytes each (x, y, z, position), 16 KiB per workgroup
constexpr int TILE_CAPACITY = 1024;
// cells per axis of a block of cells owned by one workgroup of the cooperative kernel: 1 << QUERY_BLOCK_LOG2
constexpr int QUERY_BLOCK_LOG2 = 2;
// points and cells are numbered with int32 on the device
constexpr int64_t MAX_POINTS = 0x7fffffffll;
constexpr int64_t MAX_CELLS = 0x7fffffffll - 1;   // (the key `cells` itself marks a non-finite point)
constexpr int64_t DEFAULT_CELL_BUDGET = (int64_t)1 << 24;
// Cells per axis.  A cell coordinate is t = fl(fl(p - origin) / edge), off its exact value by at most 2 * 2^-24 * MAX_DIM =
// 2^-12; two points no further apart than min_edge / EDGE_MARGIN therefore never land two cells apart (2 * 2^-12 < 2^-9), which
// is what a search over the 27 neighbouring cells relies on, and CELL_SLACK (in cells) covers the same error in the bound of the
// nearest-neighbour search.
constexpr int MAX_DIM = 2048;
constexpr double EDGE_MARGIN = 1.0 + 1.0 / 512.0;
constexpr float CELL_SLACK = 0.001f;
// the budget loop makes the edge coarser in steps of a quarter
constexpr double COARSEN = 1.25;

struct GridPlan {
  int status;        // PLAN_OK, or why there is no plan (every other field 0)
  float origin[3];   // the box's lower corner
  float edge;        // >= min_edge * EDGE_MARGIN
  int dims[3];       // cells per axis, 1 .. MAX_DIM
  int64_t cells;     // dims[0] * dims[1] * dims[2] <= cell_budget
};

inline int64_t cells_of(const double* ext, double edge, int* dims) {
  int64_t cells = 1;
  for (int a = 0; a < 3; a++) {
    const double d = std::floor(ext[a] / edge) + 1.0;   // the point at the upper corner gets a cell of its own
    dims[a] = d > (double)(2 * MAX_DIM) ? 2 * MAX_DIM : (int)d;
    cells *= dims[a];
  }
  return cells;
}

// lo, hi: bounding box of the finite points (fp32 values); n_points > 0; min_edge >= 0: the search radius of the caller (0: none).
// The edge is the largest of: min_edge * EDGE_MARGIN; the longest extent / MAX_DIM; sqrt(4 x surface area of the box / n_points)
// (four points per cell for a cloud that samples a surface) -- then coarser by COARSEN until the grid fits the budget.
inline GridPlan grid_plan(const double* lo, const double* hi, int64_t n_points, double min_edge, int64_t cell_budget) {
  GridPlan p{};
  p.status = PLAN_ERR_ARG;
  if (n_points <= 0 || cell_budget < 1 || !(min_edge >= 0.0) || !std::isfinite(min_edge)) return p;
  double ext[3];
  for (int a = 0; a < 3; a++) {
    if (!std::isfinite(lo[a]) || !std::isfinite(hi[a]) || hi[a] < lo[a]) return p;
    ext[a] = hi[a] - lo[a];
    if (!std::isfinite(ext[a])) return p;
  }
  p.status = PLAN_ERR_UNSUPPORTED;
  if (n_points > MAX_POINTS) return p;
  if (cell_budget > MAX_CELLS) cell_budget = MAX_CELLS;
  const double longest = ext[0] > ext[1] ? (ext[0] > ext[2] ? ext[0] : ext[2]) : (ext[1] > ext[2] ? ext[1] : ext[2]);
  const double area = 2.0 * (ext[0] * ext[1] + ext[1] * ext[2] + ext[2] * ext[0]);
  double edge = min_edge * EDGE_MARGIN;
  if (longest / MAX_DIM > edge) edge = longest / MAX_DIM;
  const double per_cell = std::sqrt(4.0 * area / (double)n_points);
  if (per_cell > edge) edge = per_cell;
  if (!(edge > 0.0)) edge = 1.0;   // all points equal and no radius: one cell of any size
  if (!std::isfinite(edge)) return p;
  // as fp32, never below the double (the device divides by the fp32 value)
  float ef = (float)edge;
  if ((double)ef < edge) ef = std::nextafterf(ef, INFINITY);
  if (!(ef > 0.f) || !std::isfinite(ef)) return p;
  int dims[3];
  int64_t cells = cells_of(ext, (double)ef, dims);
  while (cells > cell_budget || dims[0] > MAX_DIM || dims[1] > MAX_DIM || dims[2] > MAX_DIM) {
    ef = (float)((double)ef * COARSEN);
    if (!std::isfinite(ef)) return p;
    cells = cells_of(ext, (double)ef, dims);
  }
  p.status = PLAN_OK;
  for (int a = 0; a < 3; a++) {
    p.origin[a] = (float)lo[a];
    p.dims[a] = dims[a];
  }
  p.edge = ef;
  p.cells = cells;
  return p;
}

// blocks of cells of the cooperative kernel along one axis, and in all
inline int blocks_of(int dim) { return (dim + (1 << QUERY_BLOCK_LOG2) - 1) >> QUERY_BLOCK_LOG2; }
inline int64_t query_blocks(const int* dims) { return (int64_t)blocks_of(dims[0]) * blocks_of(dims[1]) * blocks_of(dims[2]); }

}  // namespace mesh_eval_plan
}  // namespace psdf
