// Evaluation-mode compositing of one chunk of a rendered frame for gfx950, written straight into planar images: what the
// reference's run_net does per chunk after the networks (permuto_sdf_py/train_permuto_sdf.py:137-142 foreground, :156-162
// background) and run_net_in_chunks does with the results (:190-207: list appends, torch.cat, lin2nchw), and
// rotate_normals_to_cam_frame (permuto_sdf_py/utils/common_utils.py:573-589) for the camera-frame normals.
//
// A wave owns a ray and sweeps its contiguous samples in chunks of 64 through sweep() of composite_device.h, the sweep of
// neus_composite_fwd_kernel / nerf_composite_fwd_kernel (composite_fused.hip): section-point or NeRF opacity, product scan with
// a carry; per-lane partial sums and one wave sum per quantity at the end.  From the ONE sweep over the samples the foreground
// kernel forms
//   radiance           sum w rgb                                   (integrate_fwd_kernel's order)
//   weight sum         sum w                                       (sum_ray_fwd_kernel's order)
//   gradient integral  G = sum w gradient                          (integrate_fwd_kernel's order; the gradients are read for the
//                                                                   opacity anyway: no extra bytes)
//   world normal       G / max(|G|, 1e-12)                         (normalize_eps, as normalize3's forward)
//   camera normal      normalize(R n), R the rotation of tf_cam_world (optional)
//   bg transmittance   the scan's carry, to a per-chunk [R] buffer that the background kernel reads
// and lane 0 stores them at pixel pixel_first + ray of the [3, H, W] / [1, H, W] planes.  Empty and overflowed rays hold
// radiance 0, normals 0, weight sum 0, transmittance 1: what run_net hands back for a chunk without samples (:124-129).
// HBM traffic: 44 B per sample read (sdf 4, dirs 12, gradients 12, dt 4, rgb 12) and nothing written per sample; per ray 8 B
// of range read, 4 B of transmittance and 40 B of planes written (52 B with camera normals).  The background kernel reads 20 B
// per sample (raw density 4, dt 4, rgb 12) and per ray 8 + 4 + 12 B, and writes 24 B.
//
// A NeRF foreground (permuto_sdf_py/train_nerf.py: run_net :66-71 per chunk, run_net_in_chunks :92-128 around it) has no surface
// and so no normal plane.  frame_render_nerf_kernel renders its container with the sweep, the opacity and the order of summation
// of nerf_render_fwd_kernel (nerf_render.hip) -- the planes hold the bits of psdf_nerf_render_forward -- and adds the expected
// depth sum w z, summed as a colour channel is, from the same sweep; it leaves the transmittance buffer that
// frame_composite_nerf_kernel reads.  HBM traffic: 20 B per sample read (raw density 4, dt 4, rgb 12), 24 B with the depth
// plane (z 4), nothing written per sample; per ray 8 B of range read, 4 B of transmittance and 16 B of planes written (20 B
// with the depth plane).
// Any ray length; no LDS; nothing allocates and nothing synchronises.
#include "frame_device.h"
#include "frame_plan.h"
#include "../../include/psdf.h"

using namespace psdf;

namespace {

__global__ void __launch_bounds__(PSDF_BLOCK)
    frame_composite_neus_kernel(int nr_rays, RayIndex ri, const float* __restrict__ sdf, const float* __restrict__ dirs,
                                const float* __restrict__ gradients, const float* __restrict__ dt, const float* __restrict__ rgb,
                                const float* __restrict__ inv_s_ptr, float cos_anneal_ratio, const float* __restrict__ rot,
                                int64_t plane, int64_t pixel_first, float* __restrict__ rgb_img, float* __restrict__ normals_img,
                                float* __restrict__ normals_cam_img, float* __restrict__ weights_sum_img,
                                float* __restrict__ transmittance) {
  const int lane = lane_id();
  const float inv_s = inv_s_ptr[0];
  RAY_LOOP(ray, nr_rays) {
    int s, e;
    ri.get(ray, s, e);
    const int64_t pixel = pixel_first + ray;
    if (!ri.valid(s, e)) {                  // an empty / overflowed ray renders nothing
      if (lane == 0) {
        const v3 zero = mk3(0.f, 0.f, 0.f);
        st_planes(rgb_img, plane, pixel, zero);
        st_planes(normals_img, plane, pixel, zero);
        if (normals_cam_img) st_planes(normals_cam_img, plane, pixel, zero);
        weights_sum_img[pixel] = 0.f;
        transmittance[ray] = 1.f;
      }
      continue;
    }
    float r = 0.f, g = 0.f, b = 0.f, ws = 0.f, gx = 0.f, gy = 0.f, gz = 0.f;
    v3 grad;                                // of the sample in flight: read ONCE, for the opacity and for the integral
    const float T_bg = sweep(
        s, e - s, lane,
        [&](int64_t m) {
          grad = ld3(gradients + 3 * m);
          return clip01(section(sdf[m], ld3(dirs + 3 * m), grad, dt[m], inv_s, cos_anneal_ratio).q);
        },
        [&](int64_t m, float a, float T) {
          const float w = a * T;
          r += w * rgb[3 * m];
          g += w * rgb[3 * m + 1];
          b += w * rgb[3 * m + 2];
          ws += w;
          gx += w * grad.x;
          gy += w * grad.y;
          gz += w * grad.z;
        });
    r = wave_sum(r);
    g = wave_sum(g);
    b = wave_sum(b);
    ws = wave_sum(ws);
    gx = wave_sum(gx);
    gy = wave_sum(gy);
    gz = wave_sum(gz);
    if (lane == 0) {
      st_planes(rgb_img, plane, pixel, mk3(r, g, b));
      const v3 nrm = normalize_eps(mk3(gx, gy, gz)).y;
      st_planes(normals_img, plane, pixel, nrm);
      if (normals_cam_img) st_planes(normals_cam_img, plane, pixel, camera_normal(rot, nrm));
      weights_sum_img[pixel] = ws;
      transmittance[ray] = T_bg;
    }
  }
}

__global__ void __launch_bounds__(PSDF_BLOCK)
    frame_composite_nerf_kernel(int nr_rays, RayIndex ri, const float* __restrict__ raw, const float* __restrict__ dt,
                                const float* __restrict__ rgb, const float* __restrict__ transmittance, int64_t plane,
                                int64_t pixel_first, float* __restrict__ rgb_img, float* __restrict__ rgb_bg_img) {
  const int lane = lane_id();
  RAY_LOOP(ray, nr_rays) {
    int s, e;
    ri.get(ray, s, e);
    float r = 0.f, g = 0.f, b = 0.f;
    if (ri.valid(s, e)) {
      sweep(
          s, e - s, lane, [&](int64_t m) { return nerf_alpha(raw[m], dt[m]).a; },
          [&](int64_t m, float a, float T) {
            const float w = a * T;
            r += w * rgb[3 * m];
            g += w * rgb[3 * m + 1];
            b += w * rgb[3 * m + 2];
          });
      r = wave_sum(r);
      g = wave_sum(g);
      b = wave_sum(b);
    }
    if (lane == 0) {
      const int64_t pixel = pixel_first + ray;
      const float t = transmittance[ray];
      const v3 tb = mk3(t * r, t * g, t * b);
      st_planes(rgb_img, plane, pixel, mk3(rgb_img[pixel] + tb.x, rgb_img[plane + pixel] + tb.y, rgb_img[2 * plane + pixel] + tb.z));
      st_planes(rgb_bg_img, plane, pixel, tb);
    }
  }
}

__global__ void __launch_bounds__(PSDF_BLOCK)
    frame_render_nerf_kernel(int nr_rays, RayIndex ri, const float* __restrict__ raw, const float* __restrict__ dt,
                             const float* __restrict__ z, const float* __restrict__ rgb, int64_t plane, int64_t pixel_first,
                             float* __restrict__ rgb_img, float* __restrict__ weights_sum_img, float* __restrict__ depth_img,
                             float* __restrict__ transmittance) {
  const int lane = lane_id();
  RAY_LOOP(ray, nr_rays) {
    int s, e;
    ri.get(ray, s, e);
    float r = 0.f, g = 0.f, b = 0.f, ws = 0.f, dz = 0.f, T_bg = 1.f;   // an empty / overflowed ray renders nothing
    if (ri.valid(s, e)) {
      T_bg = sweep(
          s, e - s, lane, [&](int64_t m) { return nerf_alpha(raw[m], dt[m]).a; },
          [&](int64_t m, float a, float T) {
            const float w = a * T;
            ws += w;
            r += w * rgb[3 * m];
            g += w * rgb[3 * m + 1];
            b += w * rgb[3 * m + 2];
            if (depth_img) dz += w * z[m];
          });
      r = wave_sum(r);
      g = wave_sum(g);
      b = wave_sum(b);
      ws = wave_sum(ws);
      if (depth_img) dz = wave_sum(dz);     // (a kernel argument: the whole wave takes the branch or none of it)
    }
    if (lane == 0) {
      const int64_t pixel = pixel_first + ray;
      st_planes(rgb_img, plane, pixel, mk3(r, g, b));
      weights_sum_img[pixel] = ws;
      if (depth_img) depth_img[pixel] = dz;
      transmittance[ray] = T_bg;
    }
  }
}

// the pixel range [pixel_first, pixel_first + nr_rays) of an H x W frame: frame_plan::check_range, 0 or the code to return

}  // namespace

extern "C" {

int psdf_frame_composite_neus(int nr_rays, const int* start_end, int equal, int fixed, int max_nr_samples, const float* sdf,
                              const float* dirs, const float* gradients, const float* dt, const float* rgb, const float* inv_s,
                              float cos_anneal_ratio, const float* rot_cam_world, int H, int W, int64_t pixel_first,
                              float* rgb_img, float* normals_img, float* normals_cam_img, float* weights_sum_img,
                              float* transmittance, void* stream) {
  if (nr_rays <= 0) return PSDF_OK;
  if (!inv_s || !rgb_img || !normals_img || !weights_sum_img || !transmittance || (!equal && !start_end)) return PSDF_ERR_ARG;
  if (max_nr_samples < 0 || (equal && fixed < 0) || (normals_cam_img && !rot_cam_world)) return PSDF_ERR_ARG;
  // a container without samples may come without sample tensors: every ray takes the empty branch
  if (max_nr_samples > 0 && (!sdf || !dirs || !gradients || !dt || !rgb)) return PSDF_ERR_ARG;
  if (const int status = frame_plan::check_range(H, W, pixel_first, nr_rays)) return status;
  hipLaunchKernelGGL(frame_composite_neus_kernel, dim3(ray_grid(nr_rays)), dim3(PSDF_BLOCK), 0, (hipStream_t)stream, nr_rays,
                     RayIndex{start_end, equal, fixed, max_nr_samples}, sdf, dirs, gradients, dt, rgb, inv_s, cos_anneal_ratio,
                     rot_cam_world, (int64_t)H * W, pixel_first, rgb_img, normals_img, normals_cam_img, weights_sum_img,
                     transmittance);
  PSDF_LAUNCH_CHECK();
  return PSDF_OK;
}

int psdf_frame_composite_nerf(int nr_rays, const int* start_end, int equal, int fixed, int max_nr_samples,
                              const float* raw_density, const float* dt, const float* rgb, const float* transmittance, int H,
                              int W, int64_t pixel_first, float* rgb_img, float* rgb_bg_img, void* stream) {
  if (nr_rays <= 0) return PSDF_OK;
  if (!transmittance || !rgb_img || !rgb_bg_img || (!equal && !start_end)) return PSDF_ERR_ARG;
  if (max_nr_samples < 0 || (equal && fixed < 0)) return PSDF_ERR_ARG;
  if (max_nr_samples > 0 && (!raw_density || !dt || !rgb)) return PSDF_ERR_ARG;
  if (const int status = frame_plan::check_range(H, W, pixel_first, nr_rays)) return status;
  hipLaunchKernelGGL(frame_composite_nerf_kernel, dim3(ray_grid(nr_rays)), dim3(PSDF_BLOCK), 0, (hipStream_t)stream, nr_rays,
                     RayIndex{start_end, equal, fixed, max_nr_samples}, raw_density, dt, rgb, transmittance, (int64_t)H * W,
                     pixel_first, rgb_img, rgb_bg_img);
  PSDF_LAUNCH_CHECK();
  return PSDF_OK;
}

int psdf_nerf_frame_render(int nr_rays, const int* start_end, int equal, int fixed, int max_nr_samples, const float* raw_density,
                           const float* dt, const float* z, const float* rgb, int H, int W, int64_t pixel_first, float* rgb_img,
                           float* weights_sum_img, float* depth_img, float* transmittance, void* stream) {
  if (nr_rays <= 0) return PSDF_OK;
  if (!rgb_img || !weights_sum_img || !transmittance || (!equal && !start_end)) return PSDF_ERR_ARG;
  if (max_nr_samples < 0 || (equal && fixed < 0)) return PSDF_ERR_ARG;
  // a container without samples may come without sample tensors; z is read for the depth plane alone
  if (max_nr_samples > 0 && (!raw_density || !dt || !rgb || (depth_img && !z))) return PSDF_ERR_ARG;
  if (const int status = frame_plan::check_range(H, W, pixel_first, nr_rays)) return status;
  hipLaunchKernelGGL(frame_render_nerf_kernel, dim3(ray_grid(nr_rays)), dim3(PSDF_BLOCK), 0, (hipStream_t)stream, nr_rays,
                     RayIndex{start_end, equal, fixed, max_nr_samples}, raw_density, dt, z, rgb, (int64_t)H * W, pixel_first,
                     rgb_img, weights_sum_img, depth_img, transmittance);
  PSDF_LAUNCH_CHECK();
  return PSDF_OK;
}

}  // extern "C"
