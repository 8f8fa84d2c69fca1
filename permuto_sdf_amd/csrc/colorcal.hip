// Per-image colour calibration of NeRF training, fused, for gfx950.
//
// The reference's NeRF trainer (permuto_sdf_py/train_nerf.py:52,158-161) calibrates the raw colours of every sample with a gain
// and a bias of the image its ray was drawn from, before the sigmoid (models.py:520-523, Colorcal: models.py:678-729):
//     rgb = sigmoid(raw * (1 + weight_delta[img]) + bias[img]),      image idx_fixed keeps the identity.
// As torch operators that is a transpose copy, a per-sample ray index, two index_select, a multiply-add and a sigmoid per branch
// and direction, and two index_add_ (float atomics) at the end.  Here:
//
//   (a) psdf_colorcal_sigmoid_forward: raw_fm [3, M] (the colour head's feature-major output) -> rgb [M, 3].
//   (b) psdf_colorcal_sigmoid_backward: g_raw_fm [3, M] = g_rgb rgb (1 - rgb) w, and per ray the six sums g_ray [R, 6] =
//       [sum g_pre raw (3 channels), sum g_pre (3 channels)], g_pre = g_rgb rgb (1 - rgb).
//       In both a ray belongs to a ROW of 16 lanes (four rays per wave64), its samples strided over the lanes: the three row reads
//       of raw_fm are contiguous over the lanes, the [M, 3] accesses of a row cover one contiguous span.  The sums of (b): lane l
//       adds samples l, l + 16, l + 32, ... in that order, then a four-step butterfly (xor 8, 4, 2, 1) inside the row: the order
//       depends on the ray's sample count alone.  No atomics.
//   (c) psdf_colorcal_fold: g_ray of one or two branches -> g_weight_delta [I, 3], g_bias [I, 3].  A thread owns an (image, column)
//       pair and walks the rays in ascending order; at 512 rays and a few hundred images this is not where the time is.
//
// With w = 1, b = 0 (the fixed image, an img_idx outside [0, I), zero tables) z = raw * 1 + 0 is raw, and the forward is the
// expression of sigmoid_rows_kernel (neus.hip): the same bits.  The library is built with -ffp-contract=off: z takes two roundings,
// as torch's multiply and add do.  The entries allocate nothing and never synchronise.
//
// (a) and (c) use no cross-lane operation: the file also compiles as C++ against tests/host/hip_on_host, where
// tests/host/colorcal_kernels_check.cpp runs them; (b) is compiled there and never launched (its butterfly needs real lanes).
#include "colorcal_plan.h"
#include "composite_device.h"
#include "../../include/psdf.h"

using namespace psdf;
namespace plan = psdf::colorcal_plan;

namespace {

constexpr int BLOCK = plan::BLOCK;
constexpr int ROW = plan::ROW;
constexpr int COLS = plan::COLS;

struct Tables {
  const int* __restrict__ img_idx;          // [R]
  int nr_images, idx_fixed;
  const float* __restrict__ weight_delta;   // [I, 3]
  const float* __restrict__ bias;           // [I, 3]
};

struct Calib {
  float w[3], b[3];
  bool learned;      // false: the fixed image, or an image outside the tables -- identity, no gradient
};

// the calibration of a ray: the tables are read for images inside [0, nr_images) other than the fixed one, and for no other
__device__ __forceinline__ Calib calib_of(const Tables& t, int ray) {
  Calib c;
  const int img = t.img_idx[ray];
  c.learned = img >= 0 && img < t.nr_images && img != t.idx_fixed;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    c.w[k] = c.learned ? 1.0f + t.weight_delta[3 * img + k] : 1.0f;
    c.b[k] = c.learned ? t.bias[3 * img + k] : 0.0f;
  }
  return c;
}

// a ray the kernels process: RayIndex's rule, and a range inside the M samples the feature-major rows are indexed by
__device__ __forceinline__ bool owned(const RayIndex& ri, int s, int e, int64_t M) { return ri.valid(s, e) && s >= 0 && e > s && e <= M; }

// the rows of a workgroup walk the rays: row = 16 lanes
#define ROW_LOOP(ray, nr_rays)                                                                    \
  for (int ray = blockIdx.x * plan::RAYS_PER_BLOCK + ((int)threadIdx.x / ROW); ray < nr_rays; \
       ray += gridDim.x * plan::RAYS_PER_BLOCK)

// --------------------------------------------------------------------------------------------------------- (a) forward
__global__ void __launch_bounds__(BLOCK)
    colorcal_fwd_kernel(int nr_rays, RayIndex ri, int64_t M, const float* __restrict__ raw_fm, Tables t, float* __restrict__ rgb) {
  const int l = (int)threadIdx.x % ROW;
  ROW_LOOP(ray, nr_rays) {
    int s, e;
    ri.get(ray, s, e);
    if (!owned(ri, s, e, M)) continue;
    const Calib c = calib_of(t, ray);
    for (int64_t m = (int64_t)s + l; m < e; m += ROW) {
#pragma unroll
      for (int k = 0; k < 3; k++) {
        float z = raw_fm[(int64_t)k * M + m] * c.w[k];
        z = z + c.b[k];
        rgb[3 * m + k] = 1.0f / (1.0f + expf(-z));
      }
    }
  }
}

// -------------------------------------------------------------------------------------------------------- (b) backward
// sum over the 16 lanes of a row, the same bits in every lane (xor 8, 4, 2, 1 never leaves the row)
__device__ __forceinline__ float row_sum(float v) {
#pragma unroll
  for (int o = ROW / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ void __launch_bounds__(BLOCK)
    colorcal_bwd_kernel(int nr_rays, RayIndex ri, int64_t M, const float* __restrict__ g_rgb, const float* __restrict__ rgb,
                        const float* __restrict__ raw_fm, Tables t, float* __restrict__ g_raw_fm, float* __restrict__ g_ray) {
  const int l = (int)threadIdx.x % ROW;
  // every lane of the wave reaches the butterfly of every pass: the loop bound is the same for the four rows of a wave up to the
  // last pass, where rows past the end carry zeros through it
  const int passes = (nr_rays + (int)gridDim.x * plan::RAYS_PER_BLOCK - 1) / ((int)gridDim.x * plan::RAYS_PER_BLOCK);
  for (int p = 0; p < passes; p++) {
    const int ray = (p * (int)gridDim.x + (int)blockIdx.x) * plan::RAYS_PER_BLOCK + ((int)threadIdx.x / ROW);
    const bool in = ray < nr_rays;
    float acc[COLS] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    bool learned = false;
    if (in) {
      int s, e;
      ri.get(ray, s, e);
      if (owned(ri, s, e, M)) {
        const Calib c = calib_of(t, ray);
        learned = c.learned;
        for (int64_t m = (int64_t)s + l; m < e; m += ROW) {
#pragma unroll
          for (int k = 0; k < 3; k++) {
            const float y = rgb[3 * m + k];
            const float g_pre = g_rgb[3 * m + k] * y * (1.0f - y);
            g_raw_fm[(int64_t)k * M + m] = g_pre * c.w[k];
            if (learned) {
              acc[k] += g_pre * raw_fm[(int64_t)k * M + m];
              acc[3 + k] += g_pre;
            }
          }
        }
      }
    }
    float mine = 0.f;       // lane j < 6 of the row keeps column j
#pragma unroll
    for (int j = 0; j < COLS; j++) {
      const float sum = row_sum(acc[j]);
      if (l == j) mine = sum;
    }
    if (in && l < COLS) g_ray[(int64_t)COLS * ray + l] = learned ? mine : 0.f;
  }
}

// ------------------------------------------------------------------------------------------------------------ (c) fold
__global__ void __launch_bounds__(BLOCK)
    colorcal_fold_kernel(int nr_rays, const int* __restrict__ img_idx, int nr_images, int idx_fixed, const float* __restrict__ g_ray_a,
                         const float* __restrict__ g_ray_b, float* __restrict__ g_weight_delta, float* __restrict__ g_bias) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= (int64_t)nr_images * COLS) return;
  const int img = (int)(i / COLS), col = (int)(i % COLS);
  float acc = 0.f;
  if (img != idx_fixed) {
    for (int r = 0; r < nr_rays; r++) {
      if (img_idx[r] != img) continue;
      const float a = g_ray_a[(int64_t)COLS * r + col];
      acc += g_ray_b ? g_ray_b[(int64_t)COLS * r + col] + a : a;
    }
  }
  if (col < 3) g_weight_delta[3 * img + col] = acc;
  else g_bias[3 * img + (col - 3)] = acc;
}

}  // namespace

extern "C" {

int psdf_colorcal_sigmoid_forward(int nr_rays, const int* start_end, int equal, int fixed, int max_nr_samples, int64_t nr_samples,
                                  const float* raw_fm, const int* img_idx, int nr_images, int idx_fixed, const float* weight_delta,
                                  const float* bias, float* rgb, void* stream) {
  if (nr_rays <= 0 || nr_samples == 0) return PSDF_OK;
  const int status = plan::check_counts(nr_samples, nr_images, idx_fixed), grid = plan::ray_grid(nr_rays);
  if (status != plan::PLAN_OK) return status;
  if (grid < 0) return grid;
  if (!raw_fm || !img_idx || !weight_delta || !bias || !rgb || (!equal && !start_end)) return PSDF_ERR_ARG;
  hipLaunchKernelGGL(colorcal_fwd_kernel, dim3((unsigned)grid), dim3(BLOCK), 0, (hipStream_t)stream, nr_rays,
                     RayIndex{start_end, equal, fixed, max_nr_samples}, nr_samples, raw_fm,
                     Tables{img_idx, nr_images, idx_fixed, weight_delta, bias}, rgb);
  PSDF_LAUNCH_CHECK();
  return PSDF_OK;
}

int psdf_colorcal_sigmoid_backward(int nr_rays, const int* start_end, int equal, int fixed, int max_nr_samples, int64_t nr_samples,
                                   const float* grad_rgb, const float* rgb, const float* raw_fm, const int* img_idx, int nr_images,
                                   int idx_fixed, const float* weight_delta, const float* bias, float* grad_raw_fm, float* grad_ray,
                                   void* stream) {
  if (nr_rays <= 0) return PSDF_OK;
  const int status = plan::check_counts(nr_samples, nr_images, idx_fixed), grid = plan::ray_grid(nr_rays);
  if (status != plan::PLAN_OK) return status;
  if (grid < 0) return grid;
  if (!grad_ray || (!equal && !start_end)) return PSDF_ERR_ARG;
  // without samples no ray is processed and no sample pointer is read: every row of grad_ray becomes 0
  if (nr_samples > 0 && (!grad_rgb || !rgb || !raw_fm || !img_idx || !weight_delta || !bias || !grad_raw_fm)) return PSDF_ERR_ARG;
  hipLaunchKernelGGL(colorcal_bwd_kernel, dim3((unsigned)grid), dim3(BLOCK), 0, (hipStream_t)stream, nr_rays,
                     RayIndex{start_end, equal, fixed, max_nr_samples}, nr_samples, grad_rgb, rgb, raw_fm,
                     Tables{img_idx, nr_images, idx_fixed, weight_delta, bias}, grad_raw_fm, grad_ray);
  PSDF_LAUNCH_CHECK();
  return PSDF_OK;
}

int psdf_colorcal_fold(int nr_rays, const int* img_idx, int nr_images, int idx_fixed, const float* grad_ray_a, const float* grad_ray_b,
                       float* grad_weight_delta, float* grad_bias, void* stream) {
  if (nr_rays <= 0) return PSDF_OK;
  const int status = plan::check_counts(0, nr_images, idx_fixed);
  if (status != plan::PLAN_OK) return status;
  if (!img_idx || !grad_ray_a || !grad_weight_delta || !grad_bias) return PSDF_ERR_ARG;
  hipLaunchKernelGGL(colorcal_fold_kernel, dim3((unsigned)plan::fold_grid(nr_images)), dim3(BLOCK), 0, (hipStream_t)stream, nr_rays,
                     img_idx, nr_images, idx_fixed, grad_ray_a, grad_ray_b, grad_weight_delta, grad_bias);
  PSDF_LAUNCH_CHECK();
  return PSDF_OK;
}

}  // extern "C"
