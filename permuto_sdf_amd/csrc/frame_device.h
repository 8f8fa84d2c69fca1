// frame_device.h -- what the writers of image planes share on the device (frame_composite.hip, frame_trace.hip, box_trace.hip,
// sdf_slice.hip; frame_rays.hip writes no plane and takes frame_plan.h alone): the store of a three-channel pixel, the camera-frame normal, the depth of a point along its
// ray, the pixel a surface point makes, and the reference's box test.  Every expression is written here ONCE, in the order of
// operations the kernels have always had; the library is built with -ffp-contract=off, so an expression that keeps its order
// keeps its bits (tests/test_gpu_frame_parent_bits.py pins them to the commit before the move).  The range check of a chunk of
// pixels is host arithmetic and lives in frame_plan.h, which this header brings along.
//
// No cross-lane operation and no LDS in what is defined here: a file that uses nothing else also compiles as C++ against
// tests/host/hip_on_host.
#pragma once
#include "composite_device.h"
#include "frame_plan.h"

// the entries return a plan's refusal as their own status
static_assert(psdf::frame_plan::PLAN_OK == PSDF_OK && psdf::frame_plan::PLAN_ERR_ARG == PSDF_ERR_ARG &&
                  psdf::frame_plan::PLAN_ERR_UNSUPPORTED == PSDF_ERR_UNSUPPORTED,
              "frame_plan.h and the C ABI number their refusals alike");

namespace {
using namespace psdf;

// channel c of pixel `pixel` of a planar [3, H, W] image, plane = H W
__device__ __forceinline__ void st_planes(float* __restrict__ img, int64_t plane, int64_t pixel, v3 a) {
  img[pixel] = a.x;
  img[plane + pixel] = a.y;
  img[2 * plane + pixel] = a.z;
}

// rotate_normals_to_cam_frame (permuto_sdf_py/utils/common_utils.py:573-589): R n with R the row-major rotation of tf_cam_world,
// normalised again
__device__ __forceinline__ v3 camera_normal(const float* __restrict__ rot, v3 nrm) {
  const v3 c = mk3(rot[0] * nrm.x + rot[1] * nrm.y + rot[2] * nrm.z, rot[3] * nrm.x + rot[4] * nrm.y + rot[5] * nrm.z,
                   rot[6] * nrm.x + rot[7] * nrm.y + rot[8] * nrm.z);
  return normalize_eps(c).y;
}

// dot(q, d) for q = p - o and a unit direction d: the distance of p from the camera centre along the ray, in this grouping
__device__ __forceinline__ float ray_depth(v3 q, v3 d) { return (q.x * d.x + q.y * d.y) + q.z * d.z; }

// What a traced ray leaves in the planes: zeros where nothing is hit; else the unit normal, the same in the camera's frame
// (zeros unless asked for), weight 1 and the depth.
struct SurfacePixel {
  v3 normal{0.f, 0.f, 0.f}, normal_cam{0.f, 0.f, 0.f};
  float weight = 0.f, depth = 0.f;
};

// the ray o + t d ends on the surface point p, where the SDF has the gradient g; rot: see camera_normal, null for no camera normal
__device__ __forceinline__ SurfacePixel surface_hit(v3 o, v3 d, v3 p, v3 g, const float* __restrict__ rot) {
  SurfacePixel s;
  s.normal = normalize_eps(g).y;
  if (rot) s.normal_cam = camera_normal(rot, s.normal);
  s.weight = 1.f;
  s.depth = ray_depth(p - o, d);
  return s;
}

// normals_cam_img may be null: that plane is not written
__device__ __forceinline__ void st_surface(const SurfacePixel& s, int64_t plane, int64_t pixel, float* __restrict__ normals_img,
                                           float* __restrict__ normals_cam_img, float* __restrict__ weights_sum_img,
                                           float* __restrict__ depth_img) {
  st_planes(normals_img, plane, pixel, s.normal);
  if (normals_cam_img) st_planes(normals_cam_img, plane, pixel, s.normal_cam);
  weights_sum_img[pixel] = s.weight;
  depth_img[pixel] = s.depth;
}

// a host triple (a corner, a translation, the half sizes of a box) as a kernel argument
struct Triple {
  float v[3];
};

__host__ inline Triple triple(const float* p) { return Triple{{p[0], p[1], p[2]}}; }

// AABB.check_point_inside_primitive (permuto_sdf_py/utils/aabb.py:28-42): strictly inside on all three axes about the translation
__device__ __forceinline__ bool box_inside(const Triple& tr, const Triple& half, v3 p) {
  const float q[3] = {p.x - tr.v[0], p.y - tr.v[1], p.z - tr.v[2]};
  bool in = true;
#pragma unroll
  for (int i = 0; i < 3; i++) in = in && q[i] < half.v[i] && q[i] > -half.v[i];
  return in;
}

}  // namespace
