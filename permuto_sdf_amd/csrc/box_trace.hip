// Sphere tracing inside an axis-aligned box with no occupancy grid, for gfx950: the box of the reference
// (permuto_sdf_py/utils/aabb.py) and the `occupancy_grid=None` / `time_val` branch of its sphere_trace
// (permuto_sdf_py/utils/sdf_utils.py:120-218), the way train_sdf_from_mesh.py:193, train_4d_sdf.py:268 and
// experiments/visualization/vis_4d_sdf.py look at a fitted 3-D or 4-D SDF; and the writer of the image planes of such a view.
//
// The trace keeps one slot per ray (box_trace.py): begin -> [masked encode -> masked MLP -> step] x n -> masked final SDF and
// normal -> resolve.  Points are rows of `stride` P floats, P = 3, or 4 with the time in column 3: begin writes that column from a
// DEVICE float, so that a captured launch list follows a new time value without being captured again; step never touches it.
//
// The box comes as four host triples, computed by the caller in float32 in the reference's order: box_min = -sizes / 2 +
// translation and box_max = sizes - sizes / 2 + translation for the intersection (aabb.py:48-49), translation and half =
// sizes / 2 for the inside test (aabb.py:15-25, 33-39).  The arithmetic is the reference's, operation for operation: IEEE
// division per axis (a direction component of +-0 gives +-inf, or NaN for an origin on that face, and goes through the same
// comparisons), the swap, the running lo / hi from -+1e10, the two miss conditions, 0 for both depths on a miss, lo clamped at 0
// (a NaN stays), origin + t * dir as a product and a sum.
//
// One thread per ray, one-dimensional grid, no cross-lane operation, no LDS: the file also compiles as C++ against
// tests/host/hip_on_host, where tests/host/box_trace_kernels_check.cpp runs it.  The entries allocate nothing and never synchronise.
#include "frame_device.h"
#include "../../include/psdf.h"

using namespace psdf;

namespace {

struct BoxHit {
  float t_entry, t_exit;
  bool hit;
};

// aabb.py:47-100 for one ray
__device__ __forceinline__ BoxHit box_intersect(const Triple& bmin, const Triple& bmax, v3 o, v3 d) {
  const float oo[3] = {o.x, o.y, o.z}, dd[3] = {d.x, d.y, d.z};
  float lo = -1e10f, hi = 1e10f;
  bool invalid = false;
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const float a = (bmin.v[i] - oo[i]) / dd[i], b = (bmax.v[i] - oo[i]) / dd[i];
    const bool swap = a > b;
    const float dim_lo = swap ? b : a, dim_hi = swap ? a : b;
    invalid = invalid || dim_hi < lo || dim_lo > hi;
    lo = dim_lo > lo ? dim_lo : lo;
    hi = dim_hi < hi ? dim_hi : hi;
  }
  if (invalid) lo = hi = 0.f;
  lo = lo < 0.f ? 0.f : lo;
  return BoxHit{lo, hi, !invalid};
}

__global__ void __launch_bounds__(PSDF_BLOCK)
    box_ray_intersection_kernel(int nr_rays, Triple bmin, Triple bmax, const float* __restrict__ origins,
                                const float* __restrict__ dirs, float* __restrict__ t_entry, float* __restrict__ t_exit,
                                float* __restrict__ pts_entry, float* __restrict__ pts_exit, unsigned char* __restrict__ hit) {
  const int i = blockIdx.x * PSDF_BLOCK + threadIdx.x;
  if (i >= nr_rays) return;
  const v3 o = ld3(origins + 3 * (int64_t)i), d = ld3(dirs + 3 * (int64_t)i);
  const BoxHit h = box_intersect(bmin, bmax, o, d);
  t_entry[i] = h.t_entry;
  t_exit[i] = h.t_exit;
  st3(pts_entry + 3 * (int64_t)i, along(o, h.t_entry, d));
  st3(pts_exit + 3 * (int64_t)i, along(o, h.t_exit, d));
  hit[i] = h.hit ? 1 : 0;
}

__global__ void __launch_bounds__(PSDF_BLOCK)
    box_trace_begin_kernel(int nr_rays, int stride, Triple bmin, Triple bmax, const float* __restrict__ origins,
                           const float* __restrict__ dirs, const float* __restrict__ time, float* __restrict__ pts,
                           unsigned char* __restrict__ converged, unsigned char* __restrict__ no_hit) {
  const int i = blockIdx.x * PSDF_BLOCK + threadIdx.x;
  if (i >= nr_rays) return;
  const v3 o = ld3(origins + 3 * (int64_t)i), d = ld3(dirs + 3 * (int64_t)i);
  const BoxHit h = box_intersect(bmin, bmax, o, d);
  float* p = pts + (int64_t)stride * i;
  st3(p, h.hit ? along(o, h.t_entry, d) : o);      // a ray that misses stays at its origin and is never evaluated
  if (stride == 4) p[3] = time[0];
  const unsigned char miss = h.hit ? 0 : 1;
  converged[i] = miss;
  no_hit[i] = miss;
}

__global__ void __launch_bounds__(PSDF_BLOCK)
    box_trace_step_kernel(int nr_rays, int stride, Triple tr, Triple half, const float* __restrict__ dirs,
                          const float* __restrict__ sdf, float multiplier, float thresh, float* __restrict__ pts,
                          unsigned char* __restrict__ converged) {
  const int i = blockIdx.x * PSDF_BLOCK + threadIdx.x;
  if (i >= nr_rays) return;
  if (converged[i]) return;
  const float s = sdf[i];
  const v3 d = ld3(dirs + 3 * (int64_t)i);
  float* p = pts + (int64_t)stride * i;
  const v3 q = ld3(p) + (d * s) * multiplier;      // sdf_utils.py:167: pos + dirs * sdf * sdf_multiplier
  // sdf_utils.py:171-181: the SDF from before the move, then the moved point against the box
  const bool done = fabsf(s) < thresh || !box_inside(tr, half, q);
  st3(p, q);
  if (done) converged[i] = 1;
}

__global__ void __launch_bounds__(PSDF_BLOCK)
    box_trace_resolve_kernel(int nr_rays, int stride, const float* __restrict__ origins, const float* __restrict__ dirs,
                             const float* __restrict__ pts, const float* __restrict__ sdf_end, const float* __restrict__ gradients,
                             const unsigned char* __restrict__ no_hit, float coverage_thresh, const float* __restrict__ rot,
                             int64_t plane, int64_t pixel_first, float* __restrict__ normals_img,
                             float* __restrict__ normals_cam_img, float* __restrict__ weights_sum_img, float* __restrict__ depth_img) {
  const int i = blockIdx.x * PSDF_BLOCK + threadIdx.x;
  if (i >= nr_rays) return;
  const int64_t pixel = pixel_first + i;
  SurfacePixel px;
  // filter_unconverged_points, sdf_utils.py:226: a signed compare (a NaN is not covered)
  if (!no_hit[i] && sdf_end[i] < coverage_thresh) {
    const v3 o = ld3(origins + 3 * (int64_t)i), d = ld3(dirs + 3 * (int64_t)i);
    px = surface_hit(o, d, ld3(pts + (int64_t)stride * i), ld3(gradients + (int64_t)stride * i), normals_cam_img ? rot : nullptr);
  }
  st_surface(px, plane, pixel, normals_img, normals_cam_img, weights_sum_img, depth_img);
}

}  // namespace

extern "C" {

int psdf_box_ray_intersection(int nr_rays, const float* box_min, const float* box_max, const float* origins, const float* dirs,
                              float* t_entry, float* t_exit, float* pts_entry, float* pts_exit, uint8_t* hit, void* stream) {
  if (nr_rays == 0) return PSDF_OK;
  if (nr_rays < 0 || !box_min || !box_max || !origins || !dirs || !t_entry || !t_exit || !pts_entry || !pts_exit || !hit)
    return PSDF_ERR_ARG;
  hipLaunchKernelGGL(box_ray_intersection_kernel, dim3(psdf_blocks(nr_rays, PSDF_BLOCK)), dim3(PSDF_BLOCK), 0, (hipStream_t)stream,
                     nr_rays, triple(box_min), triple(box_max), origins, dirs, t_entry, t_exit, pts_entry, pts_exit, hit);
  PSDF_LAUNCH_CHECK();
  return PSDF_OK;
}

int psdf_box_trace_begin(int nr_rays, int stride, const float* box_min, const float* box_max, const float* origins,
                         const float* dirs, const float* time, float* pts, uint8_t* converged, uint8_t* no_hit, void* stream) {
  if (nr_rays == 0) return PSDF_OK;
  if (nr_rays < 0 || (stride != 3 && stride != 4) || !box_min || !box_max || !origins || !dirs || !pts || !converged || !no_hit)
    return PSDF_ERR_ARG;
  if (stride == 4 && !time) return PSDF_ERR_ARG;
  hipLaunchKernelGGL(box_trace_begin_kernel, dim3(psdf_blocks(nr_rays, PSDF_BLOCK)), dim3(PSDF_BLOCK), 0, (hipStream_t)stream,
                     nr_rays, stride, triple(box_min), triple(box_max), origins, dirs, time, pts, converged, no_hit);
  PSDF_LAUNCH_CHECK();
  return PSDF_OK;
}

int psdf_box_trace_step(int nr_rays, int stride, const float* translation, const float* half, const float* dirs, const float* sdf,
                        float multiplier, float thresh, float* pts, uint8_t* converged, void* stream) {
  if (nr_rays == 0) return PSDF_OK;
  if (nr_rays < 0 || (stride != 3 && stride != 4) || !translation || !half || !dirs || !sdf || !pts || !converged)
    return PSDF_ERR_ARG;
  hipLaunchKernelGGL(box_trace_step_kernel, dim3(psdf_blocks(nr_rays, PSDF_BLOCK)), dim3(PSDF_BLOCK), 0, (hipStream_t)stream,
                     nr_rays, stride, triple(translation), triple(half), dirs, sdf, multiplier, thresh, pts, converged);
  PSDF_LAUNCH_CHECK();
  return PSDF_OK;
}

int psdf_box_trace_resolve(int nr_rays, int stride, const float* origins, const float* dirs, const float* pts, const float* sdf_end,
                           const float* gradients, const uint8_t* no_hit, float coverage_thresh, const float* rot_cam_world, int H,
                           int W, int64_t pixel_first, float* normals_img, float* normals_cam_img, float* weights_sum_img,
                           float* depth_img, void* stream) {
  if (nr_rays == 0) return PSDF_OK;
  if (nr_rays < 0 || (stride != 3 && stride != 4)) return PSDF_ERR_ARG;
  if (!origins || !dirs || !pts || !sdf_end || !gradients || !no_hit || !normals_img || !weights_sum_img || !depth_img)
    return PSDF_ERR_ARG;
  if (normals_cam_img && !rot_cam_world) return PSDF_ERR_ARG;
  if (const int range = frame_plan::check_range(H, W, pixel_first, nr_rays)) return range;
  hipLaunchKernelGGL(box_trace_resolve_kernel, dim3(psdf_blocks(nr_rays, PSDF_BLOCK)), dim3(PSDF_BLOCK), 0, (hipStream_t)stream,
                     nr_rays, stride, origins, dirs, pts, sdf_end, gradients, no_hit, coverage_thresh, rot_cam_world, (int64_t)H * W,
                     pixel_first, normals_img, normals_cam_img, weights_sum_img, depth_img);
  PSDF_LAUNCH_CHECK();
  return PSDF_OK;
}

}  // extern "C"
