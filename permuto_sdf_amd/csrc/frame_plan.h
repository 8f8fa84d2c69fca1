// frame_plan.h -- the host arithmetic behind the chunking of a rendered frame (frame.py, frame_rays.hip, frame_composite.hip):
// how many rays one chunk holds, how many chunks a frame takes and how long the last one is, and the ONE check of a chunk of
// pixels (or of the cells of a layer) that every writer of image planes makes.  Integers only: no HIP, no device,
// no state -- a plain C++17 compiler accepts this header, and tests/host/frame_plan_check.cpp runs it under the address and
// undefined-behaviour sanitizers.
//
// The occupancy march reserves at most max_nr_samples_per_ray uniform samples for a ray out of a pool of pool_samples; a ray
// whose reservation does not fit is dropped (rendered as empty).  rays x max_nr_samples_per_ray <= pool_samples is therefore the
// CONDITION under which no ray of a chunk can overflow the pool, not a tuning value: the chunk is the largest multiple of 64
// rays (whole waves of the ray kernel, whole workgroups' worth of the wave-per-ray kernels) that meets it, and never more than
// the frame.  The reference renders 3 000 rays per chunk (create_my_images.py:80): 640 chunks for a 1600 x 1200 view, against
// 59 here with its pool of 2 097 152 samples and 64 samples per ray.
#pragma once
#include <cstdint>

namespace psdf {
namespace frame_plan {

constexpr int PLAN_OK = 0, PLAN_ERR_ARG = -1, PLAN_ERR_UNSUPPORTED = -2;

constexpr int RAY_MULTIPLE = 64;
constexpr int64_t MAX_PIXELS = 0x7fffffffll;   // pixel and cell indices are int32: H W < 2^31, S S < 2^31

struct Plan {
  int status;                // PLAN_OK, or why there is no plan (every other field 0)
  int64_t pixels;            // H W
  int64_t rays_per_chunk;    // every chunk but the last
  int64_t chunks;
  int64_t last_chunk;        // rays of the last chunk, in [1, rays_per_chunk]
};

inline Plan plan(int H, int W, int max_nr_samples_per_ray, int64_t pool_samples) {
  Plan p{};
  p.status = PLAN_ERR_ARG;
  if (H < 1 || W < 1 || max_nr_samples_per_ray < 1) return p;
  if (pool_samples < (int64_t)RAY_MULTIPLE * max_nr_samples_per_ray) return p;
  const int64_t pixels = (int64_t)H * W;
  p.status = PLAN_ERR_UNSUPPORTED;
  if (pixels > MAX_PIXELS) return p;
  int64_t rays = pool_samples / max_nr_samples_per_ray;   // floor: rays * cap <= pool
  rays -= rays % RAY_MULTIPLE;                            // >= 64 by the refusal above
  if (rays > pixels) rays = pixels;
  p.status = PLAN_OK;
  p.pixels = pixels;
  p.rays_per_chunk = rays;
  p.chunks = (pixels + rays - 1) / rays;
  p.last_chunk = pixels - (p.chunks - 1) * rays;
  return p;
}

// the elements [first, first + count) of a rows x cols image (the pixels of a frame, the cells of a layer): PLAN_OK or the refusal
inline int check_range(int rows, int cols, int64_t first, int64_t count) {
  if (rows < 1 || cols < 1 || count < 1) return PLAN_ERR_ARG;
  const int64_t elements = (int64_t)rows * cols;
  if (elements > MAX_PIXELS) return PLAN_ERR_UNSUPPORTED;
  if (first < 0 || first > elements - count) return PLAN_ERR_ARG;
  return PLAN_OK;
}

}  // namespace frame_plan
}  // namespace psdf
