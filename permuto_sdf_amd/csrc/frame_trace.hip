// The last step of a sphere-traced frame for gfx950: one chunk of traced rays written into planar images.  What the reference's
// run_net_sphere_traced does after the networks (permuto_sdf_py/train_permuto_sdf.py:224-242): integrate_with_weights of the
// colours and of the SDF gradients with one sample per ray and a weight in {0, 1}, F.normalize of the integrated gradient, the
// weight sum, lin2nchw -- and rotate_normals_to_cam_frame (permuto_sdf_py/utils/common_utils.py:573-589) for the camera-frame
// normals.  The depth plane is new.
//
// The rays of the chunk that end on a valid surface point were compacted, in ray order, by psdf_trace_frame_select
// (sampling.hip): slot[ray] is the row of the ray in the dense arrays, -1 for the others.  One sample with weight 1 makes the
// integrals COPIES: a valid pixel holds the colour net's row and normalize_eps of the gradient's row bit for bit.  Per ray
//   rgb          rgb[slot]                                                      0 where nothing is hit (no background)
//   normals      g / max(|g|, eps), g = gradients[slot]  (normalize_eps)         0
//   normals_cam  normalize_eps(R n), R the rotation of tf_cam_world (optional)   0
//   weights_sum  1                                                               0
//   depth        ((px - ox) dx + (py - oy) dy) + (pz - oz) dz, p = pos[slot]     0
// at pixel pixel_first + ray: the surface pixel of frame_device.h (surface_hit, st_surface) and the colour beside it.
// Every pixel of the chunk is written exactly once: the planes need no zero fill.
// HBM traffic per ray: 28 B read (slot 4, origin 12, direction 12) and, for a valid ray, 36 B more (pos, gradient, rgb); 32 B
// written (44 B with camera normals).
//
// One thread per ray, one-dimensional grid, no cross-lane operation, no LDS: the file also compiles as C++ against
// tests/host/hip_on_host, where tests/host/frame_trace_check.cpp runs it.  The entry allocates nothing and never synchronises.
#include "frame_device.h"
#include "../../include/psdf.h"

using namespace psdf;

namespace {

__global__ void __launch_bounds__(PSDF_BLOCK)
    trace_frame_resolve_kernel(int nr_rays, const int* __restrict__ slot, const float* __restrict__ origins,
                               const float* __restrict__ dirs, const float* __restrict__ pos, const float* __restrict__ gradients,
                               const float* __restrict__ rgb, const float* __restrict__ rot, int64_t plane, int64_t pixel_first,
                               float* __restrict__ rgb_img, float* __restrict__ normals_img, float* __restrict__ normals_cam_img,
                               float* __restrict__ weights_sum_img, float* __restrict__ depth_img) {
  const int i = blockIdx.x * PSDF_BLOCK + threadIdx.x;
  if (i >= nr_rays) return;
  const int64_t pixel = pixel_first + i;
  const int s = slot[i];
  v3 colour = mk3(0.f, 0.f, 0.f);
  SurfacePixel px;
  if (s >= 0) {
    const v3 o = ld3(origins + 3 * (int64_t)i), d = ld3(dirs + 3 * (int64_t)i);
    colour = ld3(rgb + 3 * (int64_t)s);
    px = surface_hit(o, d, ld3(pos + 3 * (int64_t)s), ld3(gradients + 3 * (int64_t)s), normals_cam_img ? rot : nullptr);
  }
  st_planes(rgb_img, plane, pixel, colour);
  st_surface(px, plane, pixel, normals_img, normals_cam_img, weights_sum_img, depth_img);
}

}  // namespace

extern "C" {

int psdf_trace_frame_resolve(int nr_rays, int nr_valid, const int* slot, const float* origins, const float* dirs, const float* pos,
                             const float* gradients, const float* rgb, const float* rot_cam_world, int H, int W,
                             int64_t pixel_first, float* rgb_img, float* normals_img, float* normals_cam_img,
                             float* weights_sum_img, float* depth_img, void* stream) {
  if (nr_rays == 0) return PSDF_OK;
  if (nr_rays < 0 || nr_valid < 0 || nr_valid > nr_rays) return PSDF_ERR_ARG;
  if (!slot || !origins || !dirs || !rgb_img || !normals_img || !weights_sum_img || !depth_img) return PSDF_ERR_ARG;
  if (normals_cam_img && !rot_cam_world) return PSDF_ERR_ARG;
  // a chunk without a valid ray may come without the dense arrays: every slot is -1
  if (nr_valid > 0 && (!pos || !gradients || !rgb)) return PSDF_ERR_ARG;
  if (const int range = frame_plan::check_range(H, W, pixel_first, nr_rays)) return range;
  hipLaunchKernelGGL(trace_frame_resolve_kernel, dim3(psdf_blocks(nr_rays, PSDF_BLOCK)), dim3(PSDF_BLOCK), 0, (hipStream_t)stream,
                     nr_rays, slot, origins, dirs, pos, gradients, rgb, rot_cam_world, (int64_t)H * W, pixel_first, rgb_img, normals_img,
                     normals_cam_img, weights_sum_img, depth_img);
  PSDF_LAUNCH_CHECK();
  return PSDF_OK;
}

}  // extern "C"
