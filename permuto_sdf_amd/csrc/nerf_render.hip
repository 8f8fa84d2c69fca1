// NeRF training of a FOREGROUND, for gfx950: rendering with every per-ray output and its whole backward, the loss tail, and the
// glue between NerfHash's two nets.
//
// The reference trains a plain NeRF in permuto_sdf_py/train_nerf.py.  Its run_net (:61-89) renders the foreground container with
//   NerfHash's softplus (models.py:517) -> VolumeRenderingNerf.compute_weights + integrate (volume_rendering_modules.py:72-86,176-190)
// and keeps THREE per-ray results: the radiance, weights_sum (the mask loss of :206 holds it to the mask) and bg_transmittance
// (the background's colour is multiplied by it, :85).  composite_fused.hip renders the same sweep for the background role only:
// one output, one upstream gradient.  Here:
//
//   (a) psdf_nerf_render_forward / _backward: a wave owns a ray, as in composite_fused.hip, and everything a ray is made of comes
//       from composite_device.h (sweep, sweep_chunk, Transmittance, SuffixStep, nerf_alpha, poison_ray).
//       forward : any ray length, one sweep: w = alpha T -> per-lane partial sums of w rgb and of w, one wave sum each per ray
//                 (the order of nerf_composite_fwd_kernel: pred has the bits of its pred_bg); bg = T of the last sample.
//       backward: rays of at most 64 K samples held in registers (K = 1, 2, 4: nerf_render_plan.h).  Sweep 1 recomputes the
//                 forward and forms g_w = <g_pred, rgb> + g_weights_sum and g_rgb = g_pred w; sweep 2 walks the chunks from the
//                 ray's end: suffix sums of g_w alpha T, the transmittance backward with g_bg bg fed to SuffixStep::g_one_minus
//                 as neus_composite_bwd_kernel feeds it, g_alpha = g_w T - g_om, the opacity backward.
//       HBM traffic per sample, counted from the operands: forward 8 B (raw, dt) + 12 B (rgb, with pred); backward 20 B read in
//       sweep 1, raw and dt once more in sweep 2 (8 B, cache hits at these ray lengths), 4 + 12 B written.  The unfused chain
//       nerf_alpha -> cumprod -> multiply -> integrate -> sum_over_each_ray moves about 60 B forward and about 130 B backward.
//   (b) psdf_nerf_loss: the masked squared colour error of train_nerf.py:203 and the clipped binary cross entropy of :206, their
//       weighted sum and its gradient in one call.  The reduction is deterministic the way sdf_fit.hip's is: a fixed, capped
//       grid (nerf_render_plan.h), per-thread sums in double in a fixed order, a __syncthreads tree, partials in the caller's
//       workspace, a finishing launch.  No floating-point atomics.
//       torch's binary_cross_entropy clamps both logarithms at -100 and its backward divides by max((1 - c) c, eps): with c
//       clipped to [1e-3, 1 - 1e-3] neither is ever active, and neither is written here.
//   (c) psdf_nerf_head_join / _backward: [gelu(fd[1:65]); sh^T] and its backward, one launch each, a thread per sample column and
//       eight rows per workgroup: reads and writes of the feature-major side are contiguous over the samples, a thread reads its
//       harmonics as two 16-byte loads of its own row.  GELU: gelu_erf (gelu_device.h), value and derivative by torch's formula.
//
// (b) and (c) are plain data-parallel kernels with one-dimensional grids: the file also compiles as C++ against
// tests/host/hip_on_host, where tests/host/nerf_tail_kernels_check.cpp runs them (the ray kernels need wave shuffles, which that
// stand-in does not model: they are covered on the GPU).  The entries allocate nothing and never synchronise.
#include <type_traits>

#include "composite_device.h"
#include "gelu_device.h"
#include "nerf_render_plan.h"
#include "../../include/psdf.h"

using namespace psdf;
namespace plan = psdf::nerf_render_plan;

namespace {

constexpr int BLOCK = plan::BLOCK;
constexpr int TERMS = plan::TERMS;

// ------------------------------------------------------------------------------------------------------ (a) forward
__global__ void __launch_bounds__(PSDF_BLOCK)
    nerf_render_fwd_kernel(int nr_rays, RayIndex ri, const float* __restrict__ raw, const float* __restrict__ dt,
                           const float* __restrict__ rgb, float* __restrict__ pred, float* __restrict__ wsum, float* __restrict__ bg) {
  const int lane = lane_id();
  RAY_LOOP(ray, nr_rays) {
    int s, e;
    ri.get(ray, s, e);
    float r = 0.f, g = 0.f, b = 0.f, ws = 0.f, T_bg = 1.f;   // an empty / overflowed ray renders nothing, everything transmitted
    if (ri.valid(s, e)) {
      T_bg = sweep(
          s, e - s, lane, [&](int64_t m) { return nerf_alpha(raw[m], dt[m]).a; },
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
    nerf_render_bwd_kernel(int nr_rays, RayIndex ri, const float* __restrict__ g_pred, const float* __restrict__ g_wsum,
                           const float* __restrict__ g_bg, const float* __restrict__ raw, const float* __restrict__ dt,
                           const float* __restrict__ rgb, int compat, float* __restrict__ g_raw, float* __restrict__ g_rgb) {
  const int lane = lane_id();
  RAY_LOOP(ray, nr_rays) {
    int s, e;
    ri.get(ray, s, e);
    if (!ri.valid(s, e)) continue;          // their per-sample gradients: zero-filled by the caller for such containers
    const int n = e - s;                    // <= 64 K is the CALLER'S promise (max_per_ray)
    if (n > 64 * K) {   // longer than the caller declared: fail loudly, every gradient of the ray becomes NaN
      poison_ray(s, n, lane, [&](int64_t m, float bad) {
        g_raw[m] = bad;
        if (g_rgb) g_rgb[3 * m] = g_rgb[3 * m + 1] = g_rgb[3 * m + 2] = bad;
      });
      continue;
    }
    float gx = 0.f, gy = 0.f, gz = 0.f;
    if (g_pred) gx = g_pred[3 * ray], gy = g_pred[3 * ray + 1], gz = g_pred[3 * ray + 2];
    const float gs = g_wsum ? g_wsum[ray] : 0.f;
    float a_[K], T_[K], gw_[K], v_[K], e_[K];
    float ex;
    Transmittance tr;
    // ---- sweep 1: the forward again, and what the integration and the weight sum hand back
#pragma unroll
    for (int k = 0; k < K; k++) {
      a_[k] = T_[k] = gw_[k] = v_[k] = e_[k] = 0.f;
      if (64 * k >= n) continue;            // wave-uniform
      const Sample c = sweep_chunk(tr, s, n, 64 * k, lane, [&](int64_t m) {
        const NerfAlpha o = nerf_alpha(raw[m], dt[m]);
        ex = o.e;
        return o.a;
      });
      if (c.in) {
        float gw = gs;
        if (g_pred) {
          const float cx = rgb[3 * c.m], cy = rgb[3 * c.m + 1], cz = compat ? cy : rgb[3 * c.m + 2];
          gw = (gx * cx + gy * cy + gz * cz) + gs;
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
        e_[k] = ex;
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
        const float g_alpha = gw_[k] * T_[k] - g_om;                   // alpha enters as w = alpha T and as 1 - alpha + eps
        g_raw[m] = nerf_alpha_backward(g_alpha, e_[k], raw[m], dt[m]);
      }
    }
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
  float coef_rgb;      // 1 / (3 R)
  float coef_mask;     // mask_weight / R
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

__global__ void __launch_bounds__(BLOCK)
    nerf_loss_kernel(int64_t R, int64_t stride, const float* __restrict__ pred, const float* __restrict__ gt,
                     const unsigned char* __restrict__ hit, const float* __restrict__ wsum, const float* __restrict__ gt_mask,
                     LossArgs a, double* __restrict__ partials, float* __restrict__ g_pred, float* __restrict__ g_wsum) {
  __shared__ double red[TERMS][BLOCK];
  const int tid = (int)threadIdx.x;
  double acc[TERMS] = {0.0, 0.0};
  for (int64_t r = (int64_t)blockIdx.x * BLOCK + tid; r < R; r += stride) {
    const float h = hit ? (hit[r] ? 1.0f : 0.0f) : 1.0f;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const float d = gt[3 * r + c] - pred[3 * r + c];
      acc[0] += (double)((d * d) * h);
      if (g_pred) g_pred[3 * r + c] = -((2.0f * a.coef_rgb) * (d * h));
    }
    float gw = 0.0f;
    if (gt_mask) {
      const float w = wsum[r], t = gt_mask[r];
      const float c = w < a.lo ? a.lo : (w > a.hi ? a.hi : w);         // (a NaN stays a NaN, as in torch.clip)
      const float om = 1.0f - c;
      acc[1] += (double)(-(t * logf(c) + (1.0f - t) * logf(om)));
      if (w >= a.lo && w <= a.hi) gw = a.coef_mask * ((c - t) / (om * c));   // inside the closed interval the clip passes
    }
    if (g_wsum) g_wsum[r] = gw;
  }
  block_sums(red, tid, acc);
  if (tid < TERMS) partials[(int64_t)blockIdx.x * TERMS + tid] = red[tid][0];
}

struct FinishArgs {
  double count[TERMS];       // entries of the mean
  double weight[TERMS];
};

// terms[k] = (sum of the partials of term k: thread t takes t, t + BLOCK, ... and then the tree) / count;  loss += sum weight terms
__global__ void __launch_bounds__(BLOCK)
    nerf_loss_finish_kernel(const double* __restrict__ partials, int groups, FinishArgs f, float* __restrict__ terms,
                            float* __restrict__ loss) {
  __shared__ double red[TERMS][BLOCK];
  const int tid = (int)threadIdx.x;
  double acc[TERMS] = {0.0, 0.0};
  for (int i = tid; i < groups; i += BLOCK)
    for (int k = 0; k < TERMS; k++) acc[k] += partials[(int64_t)i * TERMS + k];
  block_sums(red, tid, acc);
  if (tid == 0) {
    double total = 0.0;
    for (int k = 0; k < TERMS; k++) {
      const double mean = f.count[k] > 0.0 ? red[k][0] / f.count[k] : 0.0;
      terms[k] = (float)mean;
      total += f.weight[k] * mean;
    }
    if (loss) loss[0] = loss[0] + (float)total;
  }
}

// ---------------------------------------------------------------------------------------------------- (c) the head join
// workgroup = (tile of BLOCK samples, group of ROWS_PER_GROUP output rows); thread = one sample column
__global__ void __launch_bounds__(BLOCK)
    head_join_kernel(int64_t M, const float* __restrict__ fd, const float* __restrict__ sh, float* __restrict__ x2) {
  const int group = (int)(blockIdx.x % plan::FWD_GROUPS);
  const int64_t m = (int64_t)(blockIdx.x / plan::FWD_GROUPS) * BLOCK + threadIdx.x;
  if (m >= M) return;
  const int row0 = group * plan::ROWS_PER_GROUP;
  if (row0 < plan::FEAT) {
#pragma unroll
    for (int j = 0; j < plan::ROWS_PER_GROUP; j++) {
      float h, gp;
      gelu_erf(fd[(int64_t)(1 + row0 + j) * M + m], h, gp);
      x2[(int64_t)(row0 + j) * M + m] = h;
    }
  } else {
    const float* src = sh + m * plan::SH + (row0 - plan::FEAT);       // 32 contiguous bytes of this sample's row
#pragma unroll
    for (int j = 0; j < plan::ROWS_PER_GROUP; j++) x2[(int64_t)(row0 + j) * M + m] = src[j];
  }
}

__global__ void __launch_bounds__(BLOCK)
    head_join_bwd_kernel(int64_t M, const float* __restrict__ g_rawd, const float* __restrict__ dX2, const float* __restrict__ fd,
                         float* __restrict__ g_fd) {
  const int group = (int)(blockIdx.x % plan::BWD_GROUPS);
  const int64_t m = (int64_t)(blockIdx.x / plan::BWD_GROUPS) * BLOCK + threadIdx.x;
  if (m >= M) return;
  if (group == 0) g_fd[m] = g_rawd[m];
  const int row0 = group * plan::ROWS_PER_GROUP;
#pragma unroll
  for (int j = 0; j < plan::ROWS_PER_GROUP; j++) {
    float h, gp;
    gelu_erf(fd[(int64_t)(1 + row0 + j) * M + m], h, gp);
    g_fd[(int64_t)(1 + row0 + j) * M + m] = dX2[(int64_t)(row0 + j) * M + m] * gp;
  }
}

}  // namespace

extern "C" {

int psdf_nerf_render_plan(int64_t nr_rays, int max_per_ray, int64_t* out) {
  if (!out) return PSDF_ERR_ARG;
  const plan::LossPlan p = plan::loss_plan(nr_rays);
  if (p.status != plan::PLAN_OK) return p.status;
  const int K = plan::chunks(max_per_ray);
  if (K < 0) return K;
  out[0] = p.grid;
  out[1] = p.workspace_bytes;
  out[2] = plan::RAYS_PER_PASS;
  out[3] = K;
  return PSDF_OK;
}

int psdf_nerf_render_forward(int nr_rays, const int* start_end, int equal, int fixed, int max_nr_samples, const float* raw_density,
                             const float* dt, const float* rgb, float* pred, float* weights_sum, float* bg_transmittance,
                             void* stream) {
  if (nr_rays <= 0) return PSDF_OK;
  if (!raw_density || !dt || (pred && !rgb) || (!pred && !weights_sum && !bg_transmittance) || (!equal && !start_end))
    return PSDF_ERR_ARG;
  hipLaunchKernelGGL(nerf_render_fwd_kernel, dim3(ray_grid(nr_rays)), dim3(PSDF_BLOCK), 0, (hipStream_t)stream, nr_rays,
                     RayIndex{start_end, equal, fixed, max_nr_samples}, raw_density, dt, rgb, pred, weights_sum, bg_transmittance);
  PSDF_LAUNCH_CHECK();
  return PSDF_OK;
}

int psdf_nerf_render_backward(int nr_rays, const int* start_end, int equal, int fixed, int max_nr_samples, int max_per_ray,
                              const float* grad_pred, const float* grad_weights_sum, const float* grad_bg_transmittance,
                              const float* raw_density, const float* dt, const float* rgb, int reference_compat,
                              float* grad_raw_density, float* grad_rgb, void* stream) {
  if (nr_rays <= 0) return PSDF_OK;
  if ((!grad_pred && !grad_weights_sum && !grad_bg_transmittance) || !raw_density || !dt || (grad_pred && !rgb) ||
      !grad_raw_density || (!equal && !start_end))
    return PSDF_ERR_ARG;
  const int K = plan::chunks(max_per_ray);
  if (K < 0) return K;
  const RayIndex ri{start_end, equal, fixed, max_nr_samples};
  for_chunk_count(K, [&](auto k) {
    hipLaunchKernelGGL(nerf_render_bwd_kernel<decltype(k)::value>, dim3(ray_grid(nr_rays)), dim3(PSDF_BLOCK), 0,
                       (hipStream_t)stream, nr_rays, ri, grad_pred, grad_weights_sum, grad_bg_transmittance, raw_density, dt, rgb,
                       reference_compat, grad_raw_density, grad_rgb);
  });
  PSDF_LAUNCH_CHECK();
  return PSDF_OK;
}

int psdf_nerf_loss(int64_t nr_rays, const float* pred, const float* gt, const unsigned char* hit, const float* weights_sum,
                   const float* gt_mask, float mask_weight, double* workspace, float* terms, float* loss, float* grad_pred,
                   float* grad_weights_sum, void* stream) {
  if (nr_rays <= 0) return PSDF_OK;
  const plan::LossPlan p = plan::loss_plan(nr_rays);
  if (p.status != plan::PLAN_OK) return p.status;
  if (!pred || !gt || !workspace || !terms || ((weights_sum == nullptr) != (gt_mask == nullptr))) return PSDF_ERR_ARG;
  if (!(mask_weight == mask_weight)) return PSDF_ERR_ARG;
  const bool mask = gt_mask != nullptr;
  LossArgs a{};
  FinishArgs f{};
  f.count[0] = 3.0 * (double)nr_rays;
  f.count[1] = mask ? (double)nr_rays : 0.0;
  f.weight[0] = 1.0;
  f.weight[1] = (double)mask_weight;
  a.coef_rgb = (float)(1.0 / f.count[0]);
  a.coef_mask = (float)((double)mask_weight / (double)nr_rays);
  a.lo = 1e-3f;
  a.hi = (float)(1.0 - 1e-3);      // torch.clip(x, 1e-3, 1.0 - 1e-3) of a float tensor: the double bound, rounded to float
  const dim3 grid((unsigned)p.grid), block(BLOCK);
  const int64_t stride = (int64_t)p.grid * BLOCK;   // rays of one pass of the grid
  hipLaunchKernelGGL(nerf_loss_kernel, grid, block, 0, (hipStream_t)stream, nr_rays, stride, pred, gt, hit, weights_sum, gt_mask, a,
                     workspace, grad_pred, grad_weights_sum);
  PSDF_LAUNCH_CHECK();
  hipLaunchKernelGGL(nerf_loss_finish_kernel, dim3(1), block, 0, (hipStream_t)stream, (const double*)workspace, p.grid, f, terms, loss);
  PSDF_LAUNCH_CHECK();
  return PSDF_OK;
}

int psdf_nerf_head_join(int64_t M, const float* fd, const float* sh, float* x2, void* stream) {
  if (M == 0) return PSDF_OK;
  const int64_t g = plan::join_grid(M, plan::FWD_GROUPS);
  if (g < 0) return (int)g;
  if (!fd || !sh || !x2) return PSDF_ERR_ARG;
  hipLaunchKernelGGL(head_join_kernel, dim3((unsigned)g), dim3(BLOCK), 0, (hipStream_t)stream, M, fd, sh, x2);
  PSDF_LAUNCH_CHECK();
  return PSDF_OK;
}

int psdf_nerf_head_join_backward(int64_t M, const float* grad_raw, const float* dX2, const float* fd, float* grad_fd, void* stream) {
  if (M == 0) return PSDF_OK;
  const int64_t g = plan::join_grid(M, plan::BWD_GROUPS);
  if (g < 0) return (int)g;
  if (!grad_raw || !dX2 || !fd || !grad_fd) return PSDF_ERR_ARG;
  hipLaunchKernelGGL(head_join_bwd_kernel, dim3((unsigned)g), dim3(BLOCK), 0, (hipStream_t)stream, M, grad_raw, dX2, fd, grad_fd);
  PSDF_LAUNCH_CHECK();
  return PSDF_OK;
}

}  // extern "C"
