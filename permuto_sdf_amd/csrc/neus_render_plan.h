// neus_render_plan.h -- the host arithmetic behind the launches of neus_render.hip, in one place: the register chunks K the ray
// backward holds for a declared ray length, and the shape of the loss tail's reduction -- one workgroup up to SINGLE_GROUP_RAYS
// rays (it adds into the loss itself: one launch), a capped grid with partial sums in the caller's workspace and a finishing
// launch above.  Integers only: no HIP, no device, no state -- a plain C++17 compiler accepts this header, and
// tests/host/neus_render_plan_check.cpp runs it under the address and undefined-behaviour sanitizers.
#pragma once
#include <cstdint>

namespace psdf {
namespace neus_render_plan {

constexpr int PLAN_OK = 0, PLAN_ERR_ARG = -1, PLAN_ERR_UNSUPPORTED = -2;

constexpr int BLOCK = 256;          // threads of the workgroups of the loss tail
constexpr int TERMS = 2;            // masked absolute colour error, clipped binary cross entropy of the weight sum
// One workgroup walks up to 32 rays per thread: the training step adapts its ray count between 64 and 8192 (train_step.py,
// _refresh_and_adapt), so a step's tail is always ONE launch; the serial part of a thread is 32 rays, a few microseconds.
constexpr int RAYS_PER_THREAD_SINGLE = 32;
constexpr int64_t SINGLE_GROUP_RAYS = (int64_t)BLOCK * RAYS_PER_THREAD_SINGLE;      // 8192
// Above it the kernel runs at most MAX_GRID workgroups, two per CU of a 256-CU device; a thread walks the rays
// first + k * grid * BLOCK.
constexpr int MAX_GRID = 512;
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
  int grid;                  // workgroups of the loss kernel
  int finish;                // 1: the partial sums go through the workspace and a finishing launch adds them
  int64_t workspace_bytes;   // finish ? grid * TERMS doubles : 0
};

inline LossPlan loss_plan(int64_t nr_rays) {
  LossPlan p{};
  p.status = PLAN_ERR_ARG;
  if (nr_rays < 0) return p;
  p.status = PLAN_ERR_UNSUPPORTED;
  if (nr_rays > MAX_RAYS) return p;
  p.status = PLAN_OK;
  if (nr_rays == 0) return p;
  if (nr_rays <= SINGLE_GROUP_RAYS) {
    p.grid = 1;
    return p;
  }
  const int64_t groups = (nr_rays + BLOCK - 1) / BLOCK;
  p.grid = (int)(groups < MAX_GRID ? groups : MAX_GRID);
  p.finish = 1;
  p.workspace_bytes = (int64_t)p.grid * TERMS * 8;
  return p;
}

}  // namespace neus_render_plan
}  // namespace psdf
