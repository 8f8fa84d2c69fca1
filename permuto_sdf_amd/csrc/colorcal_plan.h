// colorcal_plan.h -- the host arithmetic behind the launches of colorcal.hip, in one place: how many lanes share a ray, how many
// rays a workgroup holds and the capped grid over the rays, the grid of the fold over (image, column) pairs, the limits of the
// counts.  Integers only: no HIP, no device, no state -- a plain C++17 compiler accepts this header, and
// tests/host/colorcal_plan_check.cpp runs it under the address and undefined-behaviour sanitizers.
#pragma once
#include <cstdint>

namespace psdf {
namespace colorcal_plan {

constexpr int PLAN_OK = 0, PLAN_ERR_ARG = -1, PLAN_ERR_UNSUPPORTED = -2;

constexpr int BLOCK = 256;                       // threads of every workgroup of the file
// ---- the two sample kernels: a ray is shared by ROW lanes (one DPP row of a wave64), its samples strided over them
constexpr int ROW = 16;
constexpr int RAYS_PER_BLOCK = BLOCK / ROW;      // 16: four rays per wave, four waves
constexpr int MAX_RAY_GRID = 16384;              // beyond it a row walks the rays first + k * grid * RAYS_PER_BLOCK
constexpr int MAX_RAYS = 0x7fffffff - MAX_RAY_GRID * RAYS_PER_BLOCK;   // a row's ray counter may step once past the end
constexpr int64_t MAX_SAMPLES = 0x7fffffffll / 3;   // 3 M, the colour entries of the container, stays an int in ray ranges
constexpr int COLS = 6;                          // a row of g_ray: sum g_pre raw (3 channels), sum g_pre (3 channels)
// ---- the fold: a thread owns one (image, column) pair and walks the rays in ascending order
constexpr int MAX_IMAGES = 1 << 24;

// -> workgroups of a sample kernel over nr_rays rays (>= 1); < 0: PLAN_ERR_*
inline int ray_grid(int nr_rays) {
  if (nr_rays < 1) return PLAN_ERR_ARG;
  if (nr_rays > MAX_RAYS) return PLAN_ERR_UNSUPPORTED;
  const int64_t g = ((int64_t)nr_rays + RAYS_PER_BLOCK - 1) / RAYS_PER_BLOCK;
  return (int)(g < MAX_RAY_GRID ? g : MAX_RAY_GRID);
}

// the counts every entry takes: PLAN_OK, PLAN_ERR_ARG (no image, a fixed image outside [0, nr_images), a negative sample
// count) or PLAN_ERR_UNSUPPORTED (more than MAX_IMAGES images, more than MAX_SAMPLES samples)
inline int check_counts(int64_t nr_samples, int nr_images, int idx_fixed) {
  if (nr_samples < 0 || nr_images < 1 || idx_fixed < 0 || idx_fixed >= nr_images) return PLAN_ERR_ARG;
  if (nr_images > MAX_IMAGES || nr_samples > MAX_SAMPLES) return PLAN_ERR_UNSUPPORTED;
  return PLAN_OK;
}

// -> workgroups of the fold over nr_images images; < 0: PLAN_ERR_*
inline int fold_grid(int nr_images) {
  if (nr_images < 1) return PLAN_ERR_ARG;
  if (nr_images > MAX_IMAGES) return PLAN_ERR_UNSUPPORTED;
  return (int)(((int64_t)nr_images * COLS + BLOCK - 1) / BLOCK);
}

}  // namespace colorcal_plan
}  // namespace psdf
