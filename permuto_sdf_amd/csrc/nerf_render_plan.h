// nerf_render_plan.h -- the host arithmetic behind the launches of nerf_render.hip, in one place: the register chunks K the ray
// backward holds for a declared ray length, the capped grid of the loss kernel with its partial sums and the bytes of the
// workspace they live in, the grid of the head join.  Integers only: no HIP, no device, no state -- a plain C++17 compiler accepts
// this header, and tests/host/nerf_render_plan_check.cpp runs it under the address and undefined-behaviour sanitizers.
#pragma once
#include <cstdint>

namespace psdf {
namespace nerf_render_plan {

constexpr int PLAN_OK = 0, PLAN_ERR_ARG = -1, PLAN_ERR_UNSUPPORTED = -2;

constexpr int BLOCK = 256;          // threads of the workgroups of the loss tail and of the head join
constexpr int TERMS = 2;            // masked squared colour error, clipped binary cross entropy of the weight sum
// The loss kernel runs at most MAX_GRID workgroups, two per CU of a 256-CU device; a thread walks the rays
// first + k * grid * BLOCK.  The reference's batch (512 rays) is 2 workgroups: one ray per thread.
constexpr int MAX_GRID = 512;
constexpr int64_t RAYS_PER_PASS = (int64_t)BLOCK * MAX_GRID;
constexpr int64_t MAX_RAYS = 0x7fffffffll / 3;        // 3 R, the colour entries, is an int everywhere else in the library

// ---- the ray backward: a ray lives in K register chunks of CHUNK samples
constexpr int CHUNK = 64;
constexpr int MAX_PER_RAY = 4 * CHUNK;
// -> K = 1, 2 or 4 for max_per_ray <= 64, <= 128, <= 256;  PLAN_ERR_ARG below 1, PLAN_ERR_UNSUPPORTED above 256
inline int chunks(int max_per_ray) {
  if (max_per_ray < 1) return PLAN_ERR_ARG;
  if (max_per_ray > MAX_PER_RAY) return PLAN_ERR_UNSUPPORTED;
  return max_per_ray <= CHUNK ? 1 : (max_per_ray <= 2 * CHUNK ? 2 : 4);
}

// ---- the loss tail
struct LossPlan {
  int status;                // PLAN_OK, or why there is no plan (every other field 0)
  int grid;                  // workgroups of the loss kernel = partial sums per term
  int64_t workspace_bytes;   // grid * TERMS doubles
};

inline LossPlan loss_plan(int64_t nr_rays) {
  LossPlan p{};
  p.status = PLAN_ERR_ARG;
  if (nr_rays < 0) return p;
  p.status = PLAN_ERR_UNSUPPORTED;
  if (nr_rays > MAX_RAYS) return p;
  const int64_t groups = (nr_rays + BLOCK - 1) / BLOCK;
  p.status = PLAN_OK;
  p.grid = (int)(groups < MAX_GRID ? groups : MAX_GRID);
  p.workspace_bytes = (int64_t)p.grid * TERMS * 8;
  return p;
}

// ---- the head join: a workgroup owns BLOCK samples and ROWS_PER_GROUP rows of the output
constexpr int FEAT = 64;             // feature rows of NerfHash's density net that go through the GELU
constexpr int SH = 16;               // spherical harmonics of degree 4
constexpr int ROWS_PER_GROUP = 8;
constexpr int FWD_GROUPS = (FEAT + SH) / ROWS_PER_GROUP;     // 10: eight of features, two of harmonics
constexpr int BWD_GROUPS = FEAT / ROWS_PER_GROUP;            // 8 (the first also copies the density's gradient)
constexpr int64_t MAX_SAMPLES = 0x7fffffffll;

// -> workgroups of the join over M samples with `groups` row groups; < 0: PLAN_ERR_*
inline int64_t join_grid(int64_t M, int groups) {
  if (M < 0 || groups < 1) return PLAN_ERR_ARG;
  if (M > MAX_SAMPLES) return PLAN_ERR_UNSUPPORTED;
  const int64_t g = ((M + BLOCK - 1) / BLOCK) * groups;
  return g > 0xffffffffll ? (int64_t)PLAN_ERR_UNSUPPORTED : g;
}

}  // namespace nerf_render_plan
}  // namespace psdf
