// Rays of a whole pinhole frame for gfx950, a range of pixels at a time: what the reference's create_rays_from_frame
// (permuto_sdf_py/utils/nerf_utils.py:459-500) builds with a meshgrid, a matrix inverse and five torch launches per frame.
//
// Pixel p of an H x W frame is (x, y) = (p % W, p / W), row-major with x innermost, centre at +0.5.  The arithmetic is that of
// rays_from_reel_kernel (sampling.hip), restated expression by expression -- (px - cx) / fx, R pc as written there, the + t
// then - t round trip, rsqrtf -- so that a ray rendered for evaluation is bit-for-bit the ray training drew for that pixel
// (tests/test_gpu_frame.py compares the two kernels).  The chunking of a frame is host arithmetic (frame_plan.h).
//
// One thread per ray, one-dimensional grid, no cross-lane operation: the file also compiles as C++ against
// tests/host/hip_on_host, where tests/host/frame_rays_check.cpp runs it.  The entries allocate nothing and never synchronise.
#include "psdf_common.h"
#include "frame_plan.h"
#include "../../include/psdf.h"

using namespace psdf;
namespace fplan = psdf::frame_plan;
static_assert(fplan::PLAN_OK == PSDF_OK && fplan::PLAN_ERR_ARG == PSDF_ERR_ARG && fplan::PLAN_ERR_UNSUPPORTED == PSDF_ERR_UNSUPPORTED);

namespace {

__global__ void __launch_bounds__(PSDF_BLOCK)
    frame_rays_kernel(int nr_rays, int pixel_first, int W, const float* __restrict__ K, const float* __restrict__ T,
                      float* __restrict__ origins, float* __restrict__ dirs) {
  const int i = blockIdx.x * PSDF_BLOCK + threadIdx.x;
  if (i >= nr_rays) return;
  const int pix = pixel_first + i;
  const float px = (float)((double)(float)(pix % W) + 0.5), py = (float)((double)(float)(pix / W) + 0.5);
  const float fx = K[0], fy = K[4], cx = K[2], cy = K[5];
  const v3 pc = mk3((px - cx) / fx, (py - cy) / fy, 1.0f);
  const v3 t = mk3(T[3], T[7], T[11]);   // row major [R|t]
  // R * pc as the sum of scaled columns, in column order (mat3 * float3 of the reference)
  v3 pw = mk3(T[0] * pc.x + T[1] * pc.y + T[2] * pc.z, T[4] * pc.x + T[5] * pc.y + T[6] * pc.z,
              T[8] * pc.x + T[9] * pc.y + T[10] * pc.z);
  pw = pw + t;
  const v3 d0 = pw - t;
  const v3 d = d0 * rsqrtf(dot3(d0, d0));
  st3(origins + 3 * (int64_t)i, t);
  st3(dirs + 3 * (int64_t)i, d);
}

}  // namespace

extern "C" {

int psdf_frame_plan(int H, int W, int max_nr_samples_per_ray, int64_t pool_samples, int64_t* out) {
  if (!out) return PSDF_ERR_ARG;
  const fplan::Plan p = fplan::plan(H, W, max_nr_samples_per_ray, pool_samples);
  if (p.status != fplan::PLAN_OK) return p.status;
  out[0] = p.rays_per_chunk;
  out[1] = p.chunks;
  out[2] = p.last_chunk;
  return PSDF_OK;
}

int psdf_frame_rays(int H, int W, const float* K, const float* tf_world_cam, int64_t pixel_first, int nr_rays, float* origins,
                    float* dirs, void* stream) {
  if (nr_rays <= 0) return PSDF_OK;
  if (!K || !tf_world_cam || !origins || !dirs) return PSDF_ERR_ARG;
  if (const int range = fplan::check_range(H, W, pixel_first, nr_rays)) return range;
  hipLaunchKernelGGL(frame_rays_kernel, dim3(psdf_blocks(nr_rays, PSDF_BLOCK)), dim3(PSDF_BLOCK), 0, (hipStream_t)stream, nr_rays,
                     (int)pixel_first, W, K, tf_world_cam, origins, dirs);
  PSDF_LAUNCH_CHECK();
  return PSDF_OK;
}

}  // extern "C"
