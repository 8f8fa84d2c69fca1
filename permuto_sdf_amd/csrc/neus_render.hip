// NeuS rendering of a FOREGROUND under a mask loss, for gfx950: the render with every per-ray output and its whole backward, and
// the loss tail of a `--with_mask` training step.
//
// The reference's masked runs (train_permuto_sdf.py:153-154,381-383) have no background model: the rendered colour is the
// foreground's alone and the per-ray weight sum is held to the image's mask by a clipped binary cross entropy.  composite_fused.hip
// renders the same sweep with radiance and background transmittance only -- no weight sum, no gradient into it -- which is why the
// masked step ran the per-operator chain (neus_alpha -> cumprod -> multiply -> integrate -> sum_over_each_ray).  Here:
//
//   (a) psdf_neus_render_forward / _backward: a wave owns a ray, as in composite_fused.hip, and everything a ray is made of comes
//       from composite_device.h (sweep, sweep_chunk, Transmittance, SuffixStep, section, section_backward, clip01, poison_ray).
//       forward : any ray length, one sweep: w = alpha T -> per-lane partial sums of w rgb and of w, one wave sum each per ray
//                 (the order of neus_composite_fwd_kernel: pred and bg have its bits; the weight sum is summed as
//                 nerf_render_fwd_kernel sums it).
//       backward: rays of at most 64 K samples held in registers (K = 1, 2, 4: neus_render_plan.h).  Sweep 1 recomputes the
//                 forward and forms g_w = <g_pred, rgb> + g_weights_sum and g_rgb = g_pred w; sweep 2 is that of
//                 neus_composite_bwd_kernel: suffix sums of g_w alpha T, the transmittance backward with g_bg bg, g_alpha =
//                 g_w T - g_om, section_backward -> g_sdf, g_gradients, g_inv_s.  Without g_weights_sum every output has the
//                 bits of psdf_neus_composite_backward: the sum <g_pred, rgb> is formed first, in its order, and g_weights_sum
//                 is added to it only when it is given.
//       HBM traffic per sample, counted from the operands: forward 32 B (sdf 4, dirs 12, gradients 12, dt 4) + 12 B (rgb, with
//       pred) = 44 B as the composite forward; backward 44 B read in sweep 1, sdf, dirs, gradients and dt once more in sweep 2
//       (32 B, cache hits at these ray lengths), 4 B (g_sdf) + 12 B (g_gradients) + 12 B (g_rgb) written.  Per ray 16 B forward
//       (pred, weights_sum), up to 20 B read backward.  The per-operator chain it replaces moves about 130 B per sample forward
//       and 250 B backward, in 6 + 9 launches.
//   (b) psdf_neus_mask_loss: the colour term of the step (l1_loss_kernel's) and the clipped cross entropy of the weight sum
//       (psdf_nerf_loss's, same constants, same rule at the two bounds), their weighted sum added to the step's accumulator and
//       both gradients, in one call.  Deterministic: per-thread sums in double in a fixed order, a __syncthreads tree, and no
//       floating-point atomics.  Up to neus_render_plan.h's SINGLE_GROUP_RAYS rays (8192: the trainer's cap) one workgroup does
//       it all and its first thread adds into the loss: one launch.  Above, a capped grid leaves partial sums in the caller's
//       workspace and a finishing launch adds them.
//
// (b) is a plain data-parallel kernel with a one-dimensional grid: the file also compiles as C++ against tests/host/hip_on_host,
// where tests/host/neus_mask_loss_check.cpp runs it (the ray kernels need wave shuffles, which that stand-in does not model: they
// are covered on the GPU).  The entries allocate nothing and never synchronise.
#include <type_traits>

#include "composite_device.h"
#include "neus_render_plan.h"
#include "../../include/psdf.h"

using namespace psdf;
namespace plan = psdf::neus_render_plan;

namespace {

constexpr int BLOCK = plan::BLOCK;
constexpr int TERMS = plan::TERMS;

// ------------------------------------------------------------------------------------------------------ (a) forward
__global__ void __launch_bounds__(PSDF_BLOCK)
    neus_render_fwd_kernel(int nr_rays, RayIndex ri, const float* __restrict__ sdf, const float* __restrict__ dirs,
                           const float* __restrict__ gradients, const float* __restrict__ dt, const float* __restrict__ rgb,
                           const float* __restrict__ inv_s_ptr, float cos_anneal_ratio, float* __restrict__ pred,
                           float* __restrict__ wsum, float* __restrict__ bg) {
  const int lane = lane_id();
  const float inv_s = inv_s_ptr[0];
  RAY_LOOP(ray, nr_rays) {
    int s, e;
    ri.get(ray, s, e);
    float r = 0.f, g = 0.f, b = 0.f, ws = 0.f, T_bg = 1.f;   // an empty / overflowed ray renders nothing, everything transmitted
    if (ri.valid(s, e)) {
      T_bg = sweep(
          s, e - s, lane,
          [&](int64_t m) {
            return clip01(section(sdf[m], ld3(dirs + 3 * m), ld3(gradients + 3 * m), dt[m], inv_s, cos_anneal_ratio).q);
          },
          [&](int64_t m, float a, float T) {
            const float w = a * T;
            ws += w;
            if (pred) {
              r += w * rgb[3 * m];
              g += w * rgb[3 * m + 1];
              b += w * rgb[3 * m + 2];
            }
          });
      r = wave_sum(r);
      g = wave_sum(g);
      b = wave_sum(b);
      ws = wave_sum(ws);
    }
    if (lane == 0) {
      if (pred) {
        pred[3 * ray] = r;
        pred[3 * ray + 1] = g;
        pred[3 * ray + 2] = b;
      }
      if (wsum) wsum[ray] = ws;
      if (bg) bg[ray] = T_bg;
    }
  }
}

// ----------------------------------------------------------------------------------------------------- (a) backward
template <int K>
__global__ void __launch_bounds__(PSDF_BLOCK)
    neus_render_bwd_kernel(int nr_rays, RayIndex ri, const float* __restrict__ g_pred, const float* __restrict__ g_wsum,
                           const float* __restrict__ g_bg, const float* __restrict__ sdf, const float* __restrict__ dirs,
                           const float* __restrict__ gradients, const float* __restrict__ dt, const float* __restrict__ rgb,
                           const float* __restrict__ inv_s_ptr, float cos_anneal_ratio, int compat, float* __restrict__ g_sdf,
                           float* __restrict__ g_gradients, float* __restrict__ g_rgb, float* __restrict__ g_inv_s) {
  const int lane = lane_id();
  const float inv_s = inv_s_ptr[0], rr = cos_anneal_ratio;
  float gs_acc = 0.f;
  RAY_LOOP(ray, nr_rays) {
    int s, e;
    ri.get(ray, s, e);
    if (!ri.valid(s, e)) continue;          // their per-sample gradients: zero-filled by the caller for such containers
    const int n = e - s;                    // <= 64 K is the CALLER'S promise (max_per_ray)
    if (n > 64 * K) {   // longer than the caller declared: fail loudly, every gradient of the ray becomes NaN
      poison_ray(s, n, lane, [&](int64_t m, float bad) {
        g_sdf[m] = bad;
        if (g_rgb) g_rgb[3 * m] = g_rgb[3 * m + 1] = g_rgb[3 * m + 2] = bad;
        if (g_gradients) st3(g_gradients + 3 * m, mk3(bad, bad, bad));
      });
      continue;
    }
    float gx = 0.f, gy = 0.f, gz = 0.f;
    if (g_pred) gx = g_pred[3 * ray], gy = g_pred[3 * ray + 1], gz = g_pred[3 * ray + 2];
    const float gws = g_wsum ? g_wsum[ray] : 0.f;
    float a_[K], T_[K], gw_[K], v_[K];
    Transmittance tr;
    // ---- sweep 1: the forward again, and what the integration and the weight sum hand back
#pragma unroll
    for (int k = 0; k < K; k++) {
      a_[k] = T_[k] = gw_[k] = v_[k] = 0.f;
      if (64 * k >= n) continue;            // wave-uniform
      const Sample c = sweep_chunk(tr, s, n, 64 * k, lane, [&](int64_t m) {
        return clip01(section(sdf[m], ld3(dirs + 3 * m), ld3(gradients + 3 * m), dt[m], inv_s, rr).q);
      });
      if (c.in) {
        float gw = gws;
        if (g_pred) {
          const float cx = rgb[3 * c.m], cy = rgb[3 * c.m + 1], cz = compat ? cy : rgb[3 * c.m + 2];
          gw = gx * cx + gy * cy + gz * cz;       // the composite backward's sum, in its order ...
          if (g_wsum) gw = gw + gws;              // ... and the weight sum's gradient on top of it only when there is one
        }
        if (g_rgb) {
          const float w = c.a * c.T;
          g_rgb[3 * c.m] = gx * w;
          g_rgb[3 * c.m + 1] = gy * w;
          g_rgb[3 * c.m + 2] = gz * w;
        }
        a_[k] = c.a;
        T_[k] = c.T;
        gw_[k] = gw;
        v_[k] = (gw * c.a) * c.T;          // g_T * T
      }
    }
    const float gb = (g_bg ? g_bg[ray] : 0.f) * tr.carry;   // carry == bg transmittance
    // ---- sweep 2, from the end of the ray: suffix sums, transmittance backward, opacity backward
    SuffixStep sfx;
#pragma unroll
    for (int k = K - 1; k >= 0; k--) {
      if (64 * k >= n) continue;            // wave-uniform
      const int i = 64 * k + lane;
      const float g_om = sfx.g_one_minus(v_[k], a_[k], &gb, i, n, lane);
      if (i < n) {
        const int64_t m = s + i;
        const float g_alpha = gw_[k] * T_[k] - g_om;
        const v3 dir = ld3(dirs + 3 * m);
        const float d = dt[m];
        const Section sc = section(sdf[m], dir, ld3(gradients + 3 * m), d, inv_s, rr);
        const SectionGrad sg = section_backward(sc, g_alpha, d, inv_s, rr);
        gs_acc += sg.g_inv_s;
        g_sdf[m] = sg.g_sdf;
        if (g_gradients) st3(g_gradients + 3 * m, sg.g_tc * dir);
      }
    }
  }
  if (g_inv_s) {      // one sum per wave, as neus_composite_bwd_kernel hands it over
    gs_acc = wave_sum(gs_acc);
    if (lane == 0 && gs_acc != 0.f) atomicAdd(g_inv_s, gs_acc);
  }
}

// The ray backward holds a ray in K register chunks: fn(int_c<K>) for the K of the plan header
template <int V>
using int_c = std::integral_constant<int, V>;
template <class Fn>
void for_chunk_count(int K, Fn&& fn) {
  if (K == 1) return fn(int_c<1>{});
  if (K == 2) return fn(int_c<2>{});
  return fn(int_c<4>{});
}

// ---------------------------------------------------------------------------------------------------- (b) the loss tail
struct LossArgs {
  float scale_rgb;     // 1 / (3 R)
  float scale_mask;    // mask_weight / R
  float lo, hi;        // the clip of the weight sum
};

// sums over the workgroup of the two accumulators, in a fixed order; every thread calls it, once per kernel
__device__ __forceinline__ void block_sums(double (*red)[BLOCK], int tid, const double* acc) {
  for (int k = 0; k < TERMS; k++) red[k][tid] = acc[k];
  __syncthreads();
  for (int s = BLOCK / 2; s > 0; s >>= 1) {
    if (tid < s)
      for (int k = 0; k < TERMS; k++) red[k][tid] += red[k][tid + s];
    __syncthreads();
  }
}

// loss += (float)(scale_rgb sum0 + scale_mask sum1), the weighting in double
__device__ __forceinline__ void add_to_loss(float* __restrict__ loss, const LossArgs& a, double sum0, double sum1) {
  loss[0] = loss[0] + (float)((double)a.scale_rgb * sum0 + (double)a.scale_mask * sum1);
}

// partials == NULL: the grid is one workgroup and its first thread adds the two weighted sums into loss[0]
__global__ void __launch_bounds__(BLOCK)
    neus_mask_loss_kernel(int64_t R, int64_t stride, const float* __restrict__ pred, const float* __restrict__ gt,
                          const unsigned char* __restrict__ hit, const float* __restrict__ wsum, const float* __restrict__ gt_mask,
                          LossArgs a, double* __restrict__ partials, float* __restrict__ loss, float* __restrict__ g_pred,
                          float* __restrict__ g_wsum) {
  __shared__ double red[TERMS][BLOCK];
  const int tid = (int)threadIdx.x;
  double acc[TERMS] = {0.0, 0.0};
  for (int64_t r = (int64_t)blockIdx.x * BLOCK + tid; r < R; r += stride) {
    const float h = hit ? (hit[r] ? 1.0f : 0.0f) : 1.0f;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const float d = pred[3 * r + c] - gt[3 * r + c];
      acc[0] += (double)(fabsf(d) * h);
      if (g_pred) g_pred[3 * r + c] = (d > 0.f ? a.scale_rgb : (d < 0.f ? -a.scale_rgb : 0.f)) * h;
    }
    const float w = wsum[r], t = gt_mask[r];
    const float c = w < a.lo ? a.lo : (w > a.hi ? a.hi : w);           // (a NaN stays a NaN, as in torch.clip)
    const float om = 1.0f - c;
    acc[1] += (double)(-(t * logf(c) + (1.0f - t) * logf(om)));
    float gw = 0.0f;
    if (w >= a.lo && w <= a.hi) gw = a.scale_mask * ((c - t) / (om * c));   // inside the closed interval the clip passes
    if (g_wsum) g_wsum[r] = gw;
  }
  block_sums(red, tid, acc);
  if (partials) {
    if (tid < TERMS) partials[(int64_t)blockIdx.x * TERMS + tid] = red[tid][0];
  } else if (tid == 0) {
    add_to_loss(loss, a, red[0][0], red[1][0]);
  }
}

// the partials of term k: thread t takes t, t + BLOCK, ... and then the tree
__global__ void __launch_bounds__(BLOCK)
    neus_mask_loss_finish_kernel(const double* __restrict__ partials, int groups, LossArgs a, float* __restrict__ loss) {
  __shared__ double red[TERMS][BLOCK];
  const int tid = (int)threadIdx.x;
  double acc[TERMS] = {0.0, 0.0};
  for (int i = tid; i < groups; i += BLOCK)
    for (int k = 0; k < TERMS; k++) acc[k] += partials[(int64_t)i * TERMS + k];
  block_sums(red, tid, acc);
  if (tid == 0) add_to_loss(loss, a, red[0][0], red[1][0]);
}

}  // namespace

extern "C" {

int psdf_neus_render_plan(int64_t nr_rays, int max_per_ray, int64_t* out) {
  if (!out) return PSDF_ERR_ARG;
  const plan::LossPlan p = plan::loss_plan(nr_rays);
  if (p.status != plan::PLAN_OK) return p.status;
  const int K = plan::chunks(max_per_ray);
  if (K < 0) return K;
  out[0] = K;
  out[1] = p.grid;
  out[2] = p.workspace_bytes;
  out[3] = plan::SINGLE_GROUP_RAYS;
  return PSDF_OK;
}

int psdf_neus_render_forward(int nr_rays, const int* start_end, int equal, int fixed, int max_nr_samples, const float* sdf,
                             const float* dirs, const float* gradients, const float* dt, const float* rgb, const float* inv_s,
                             float cos_anneal_ratio, float* pred, float* weights_sum, float* bg_transmittance, void* stream) {
  if (nr_rays <= 0) return PSDF_OK;
  if (!sdf || !dirs || !gradients || !dt || !inv_s || (pred && !rgb) || (!pred && !weights_sum && !bg_transmittance) ||
      (!equal && !start_end))
    return PSDF_ERR_ARG;
  hipLaunchKernelGGL(neus_render_fwd_kernel, dim3(ray_grid(nr_rays)), dim3(PSDF_BLOCK), 0, (hipStream_t)stream, nr_rays,
                     RayIndex{start_end, equal, fixed, max_nr_samples}, sdf, dirs, gradients, dt, rgb, inv_s, cos_anneal_ratio,
                     pred, weights_sum, bg_transmittance);
  PSDF_LAUNCH_CHECK();
  return PSDF_OK;
}

int psdf_neus_render_backward(int nr_rays, const int* start_end, int equal, int fixed, int max_nr_samples, int max_per_ray,
                              const float* grad_pred, const float* grad_weights_sum, const float* grad_bg_transmittance,
                              const float* sdf, const float* dirs, const float* gradients, const float* dt, const float* rgb,
                              const float* inv_s, float cos_anneal_ratio, int reference_compat, float* grad_sdf,
                              float* grad_gradients, float* grad_rgb, float* grad_inv_s, void* stream) {
  if (nr_rays <= 0) return PSDF_OK;
  if ((!grad_pred && !grad_weights_sum && !grad_bg_transmittance) || !sdf || !dirs || !gradients || !dt || !inv_s ||
      (grad_pred && !rgb) || !grad_sdf || (!equal && !start_end))
    return PSDF_ERR_ARG;
  const int K = plan::chunks(max_per_ray);
  if (K < 0) return K;
  const RayIndex ri{start_end, equal, fixed, max_nr_samples};
  for_chunk_count(K, [&](auto k) {
    hipLaunchKernelGGL(neus_render_bwd_kernel<decltype(k)::value>, dim3(ray_grid(nr_rays)), dim3(PSDF_BLOCK), 0,
                       (hipStream_t)stream, nr_rays, ri, grad_pred, grad_weights_sum, grad_bg_transmittance, sdf, dirs, gradients,
                       dt, rgb, inv_s, cos_anneal_ratio, reference_compat, grad_sdf, grad_gradients, grad_rgb, grad_inv_s);
  });
  PSDF_LAUNCH_CHECK();
  return PSDF_OK;
}

int psdf_neus_mask_loss(int64_t nr_rays, const float* pred, const float* gt, const unsigned char* hit, const float* weights_sum,
                        const float* gt_mask, float scale_rgb, float scale_mask, double* workspace, float* loss, float* grad_pred,
                        float* grad_weights_sum, void* stream) {
  if (nr_rays <= 0) return PSDF_OK;
  const plan::LossPlan p = plan::loss_plan(nr_rays);
  if (p.status != plan::PLAN_OK) return p.status;
  if (!pred || !gt || !weights_sum || !gt_mask || !loss || (p.finish && !workspace)) return PSDF_ERR_ARG;
  if (!(scale_rgb == scale_rgb) || !(scale_mask == scale_mask)) return PSDF_ERR_ARG;
  LossArgs a{};
  a.scale_rgb = scale_rgb;
  a.scale_mask = scale_mask;
  a.lo = 1e-3f;
  a.hi = (float)(1.0 - 1e-3);      // torch.clip(x, 1e-3, 1.0 - 1e-3) of a float tensor: the double bound, rounded to float
  const dim3 grid((unsigned)p.grid), block(BLOCK);
  const int64_t stride = (int64_t)p.grid * BLOCK;   // rays of one pass of the grid
  hipLaunchKernelGGL(neus_mask_loss_kernel, grid, block, 0, (hipStream_t)stream, nr_rays, stride, pred, gt, hit, weights_sum, gt_mask,
                     a, p.finish ? workspace : (double*)nullptr, loss, grad_pred, grad_weights_sum);
  PSDF_LAUNCH_CHECK();
  if (p.finish) {
    hipLaunchKernelGGL(neus_mask_loss_finish_kernel, dim3(1), block, 0, (hipStream_t)stream, (const double*)workspace, p.grid, a, loss);
    PSDF_LAUNCH_CHECK();
  }
  return PSDF_OK;
}

}  // extern "C"
