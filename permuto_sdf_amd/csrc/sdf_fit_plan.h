// sdf_fit_plan.h -- the host arithmetic behind the launches of sdf_fit.hip, in one place: the workgroups of the batch kernel, the
// capped grid of the loss kernel, its partial sums and the bytes of the workspace they live in.  Integers only: no HIP, no device,
// no state -- a plain C++17 compiler accepts this header, and tests/host/sdf_fit_kernels_check.cpp runs it under the address and
// undefined-behaviour sanitizers.
#pragma once
#include <cstdint>

namespace psdf {
namespace sdf_fit_plan {

constexpr int PLAN_OK = 0, PLAN_ERR_ARG = -1, PLAN_ERR_UNSUPPORTED = -2;

constexpr int BLOCK = 256;        // threads of every workgroup of sdf_fit.hip
constexpr int TERMS = 4;          // eikonal, normal, surface |sdf|, off-surface
// The loss kernel runs at most MAX_GRID workgroups, two per CU of a 256-CU device; a thread walks the rows
// first + k * grid * BLOCK.  The reference's batch (33 000 rows) is 129 workgroups: one row per thread.
constexpr int MAX_GRID = 512;
constexpr int64_t ROWS_PER_PASS = (int64_t)BLOCK * MAX_GRID;   // rows the full grid covers in one pass
constexpr int64_t MAX_ROWS = 0x7fffffffll;                     // n_surf + n_off of one call

struct Plan {
  int status;                // PLAN_OK, or why there is no plan (every other field 0)
  int loss_grid;             // workgroups of the loss kernel = partial sums per term
  int64_t workspace_bytes;   // loss_grid * TERMS doubles
  int64_t batch_grid;        // workgroups of the batch kernel: one thread per row
};

inline Plan plan(int64_t n_surf, int64_t n_off) {
  Plan p{};
  p.status = PLAN_ERR_ARG;
  if (n_surf < 0 || n_off < 0) return p;
  p.status = PLAN_ERR_UNSUPPORTED;
  if (n_surf > MAX_ROWS || n_off > MAX_ROWS || n_surf + n_off > MAX_ROWS) return p;
  const int64_t N = n_surf + n_off, groups = (N + BLOCK - 1) / BLOCK;
  p.status = PLAN_OK;
  p.loss_grid = (int)(groups < MAX_GRID ? groups : MAX_GRID);
  p.workspace_bytes = (int64_t)p.loss_grid * TERMS * 8;
  p.batch_grid = groups;
  return p;
}

}  // namespace sdf_fit_plan
}  // namespace psdf
