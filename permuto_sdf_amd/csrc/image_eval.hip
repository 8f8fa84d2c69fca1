// Image evaluation for gfx950: the masked PSNR and SSIM the reference scores its held-out views with
// (permuto_sdf_py/experiments/evaluation/evaluate_psnr.py calls piq.psnr and piq.ssim on both images times the mask), on
// tensors that are already on the device, accumulated in float64.
//
// An image is a logical (N, C, H, W) tensor of fp32 or uint8 elements behind four element strides of its own, read in place: an
// NHWC buffer viewed as NCHW costs no copy.  A uint8 element v stands for double(v) / 255.  The optional mask is (N, 1, H, W), fp32
// or uint8, and multiplies both images; data_range divides both.  Every product and quotient is formed in double:
//   value(n, c, h, w) = element * mask(n, h, w) / data_range.
//
//   (a) squared difference: sum over (c, h, w) of (x - y)^2 per image.  A workgroup owns SQ_PIXELS consecutive pixels of one image
//       (a thread reads all channels of a pixel: the mask is read once, and NCHW and NHWC both read whole lines), writes ONE
//       partial sum to the workspace, and a finishing launch adds an image's partials in a fixed order.
//   (b) SSIM: one workgroup per (image, channel, tile of TILE_H x TILE_W map entries), one fused pass.  The loader averages every
//       f x f block of the inputs (stride f, remainders dropped: floor mode) straight into LDS -- no pooled image exists in memory;
//       the horizontal pass of the separable Gaussian runs from LDS into LDS for the five moments E[x], E[y], E[x^2], E[y^2],
//       E[xy]; the vertical pass runs from LDS, forms the map entry
//           (2 mx my + c1) / (mx^2 + my^2 + c1) * (2 sxy + c2) / (sxx + syy + c2)
//       over valid windows only, optionally stores it, and the workgroup writes one partial sum of its entries.  The finishing
//       launch adds the partials of an image in a fixed order and divides by C * mh * mw: mean over the map, then over channels.
//
// There are no floating-point atomics: every sum is a fixed sequence per thread followed by a __syncthreads tree over LDS, so the
// same input gives the same bits on every run.  Grids and blocks are one-dimensional and the block size is a compile-time
// constant: the file also compiles as C++ against tests/host/hip_on_host, where tests/host/image_eval_kernels_check.cpp runs it.
// The entries allocate nothing and never synchronise.
#include "psdf_common.h"
#include "image_eval_plan.h"
#include "../../include/psdf.h"

using namespace psdf;
namespace plan = psdf::image_eval_plan;

namespace {

constexpr int BLOCK = plan::BLOCK;

struct Image {
  const void* data;   // NULL: absent (the mask only)
  int64_t sn, sc, sh, sw;
  int u8;
};
struct Weights {
  double w[plan::MAX_KERNEL];
};

__device__ __forceinline__ double element(const Image& im, int64_t at) {
  return im.u8 ? (double)((const uint8_t*)im.data)[at] / 255.0 : (double)((const float*)im.data)[at];
}
__device__ __forceinline__ double mask_at(const Image& mask, int64_t n, int64_t h, int64_t w) {
  return mask.data ? element(mask, n * mask.sn + h * mask.sh + w * mask.sw) : 1.0;
}
__device__ __forceinline__ double value(const Image& im, int64_t n, int64_t c, int64_t h, int64_t w, double m, double data_range) {
  return element(im, n * im.sn + c * im.sc + h * im.sh + w * im.sw) * m / data_range;
}

// sum over the workgroup, in a fixed order; every thread calls it, once per kernel
__device__ __forceinline__ double block_sum(double* red, int tid, double v) {
  red[tid] = v;
  __syncthreads();
  for (int s = BLOCK / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  return red[0];
}

// ---- (a) squared difference ----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(BLOCK)
    sq_diff_kernel(Image pred, Image gt, Image mask, int C, int H, int W, int64_t per_image, double data_range,
                   double* __restrict__ partials) {
  __shared__ double red[BLOCK];
  const int tid = (int)threadIdx.x;
  const int64_t n = (int64_t)blockIdx.x / per_image, chunk = (int64_t)blockIdx.x % per_image;
  const int64_t pixels = (int64_t)H * W;
  double acc = 0.0;
  for (int i = 0; i < plan::SQ_PIXELS_PER_THREAD; i++) {
    const int64_t p = chunk * plan::SQ_PIXELS + (int64_t)i * BLOCK + tid;
    if (p >= pixels) break;
    const int64_t h = p / W, w = p % W;
    const double m = mask_at(mask, n, h, w);
    for (int c = 0; c < C; c++) {
      const double d = value(pred, n, c, h, w, m, data_range) - value(gt, n, c, h, w, m, data_range);
      acc += d * d;
    }
  }
  const double total = block_sum(red, tid, acc);
  if (tid == 0) partials[blockIdx.x] = total;
}

// out[n] = (sum of the per_image partials of image n, thread t taking t, t + BLOCK, ... and then the tree) / denom
__global__ void __launch_bounds__(BLOCK)
    finish_kernel(const double* __restrict__ partials, int64_t per_image, double denom, double* __restrict__ out) {
  __shared__ double red[BLOCK];
  const int tid = (int)threadIdx.x;
  const double* mine = partials + (int64_t)blockIdx.x * per_image;
  double acc = 0.0;
  for (int64_t i = tid; i < per_image; i += BLOCK) acc += mine[i];
  const double total = block_sum(red, tid, acc);
  if (tid == 0) out[blockIdx.x] = total / denom;
}

// ---- (b) SSIM --------------------------------------------------------------------------------------------------------------------
struct SsimShape {
  int C, f, mh, mw, tiles_y, tiles_x, K;
};

__global__ void __launch_bounds__(BLOCK)
    ssim_kernel(Image pred, Image gt, Image mask, SsimShape s, Weights weights, double data_range, double c1, double c2,
                double* __restrict__ partials, double* __restrict__ map) {
  __shared__ double tile_x[plan::IN_H * plan::IN_W], tile_y[plan::IN_H * plan::IN_W];
  __shared__ double rows[plan::MOMENTS][plan::IN_H * plan::TILE_W];
  __shared__ double red[BLOCK];
  __shared__ double wk[plan::MAX_KERNEL];
  const int tid = (int)threadIdx.x;
  int64_t b = (int64_t)blockIdx.x;
  const int tx = (int)(b % s.tiles_x);
  b /= s.tiles_x;
  const int ty = (int)(b % s.tiles_y);
  b /= s.tiles_y;
  const int64_t c = b % s.C, n = b / s.C;
  // the tile's first map entry = its first pooled pixel; the last window of the map ends on the last pooled row and column, so
  // every pooled pixel below lies inside the pooled image and every input pixel inside the image
  const int y0 = ty * plan::TILE_H, x0 = tx * plan::TILE_W;
  const int out_h = min(plan::TILE_H, s.mh - y0), out_w = min(plan::TILE_W, s.mw - x0);
  const int in_h = out_h + s.K - 1, in_w = out_w + s.K - 1;
  const int f = s.f, K = s.K;
  if (tid < K) wk[tid] = weights.w[tid];
  // pooling: the mean of f x f input values, row by row
  const double area = (double)(f * f);
  for (int i = tid; i < in_h * in_w; i += BLOCK) {
    const int r = i / in_w, q = i % in_w;
    const int64_t h0 = (int64_t)(y0 + r) * f, w0 = (int64_t)(x0 + q) * f;
    double sx = 0.0, sy = 0.0;
    for (int dy = 0; dy < f; dy++)
      for (int dx = 0; dx < f; dx++) {
        const double m = mask_at(mask, n, h0 + dy, w0 + dx);
        sx += value(pred, n, c, h0 + dy, w0 + dx, m, data_range);
        sy += value(gt, n, c, h0 + dy, w0 + dx, m, data_range);
      }
    tile_x[r * plan::IN_W + q] = sx / area;
    tile_y[r * plan::IN_W + q] = sy / area;
  }
  __syncthreads();
  // horizontal pass: the five moments of every row of the tile, at the tile's out_w columns
  for (int i = tid; i < in_h * out_w; i += BLOCK) {
    const int r = i / out_w, q = i % out_w;
    double ex = 0.0, ey = 0.0, exx = 0.0, eyy = 0.0, exy = 0.0;
    for (int k = 0; k < K; k++) {
      const double w = wk[k], x = tile_x[r * plan::IN_W + q + k], y = tile_y[r * plan::IN_W + q + k];
      ex += w * x;
      ey += w * y;
      exx += w * (x * x);
      eyy += w * (y * y);
      exy += w * (x * y);
    }
    const int at = r * plan::TILE_W + q;
    rows[0][at] = ex;
    rows[1][at] = ey;
    rows[2][at] = exx;
    rows[3][at] = eyy;
    rows[4][at] = exy;
  }
  __syncthreads();
  // vertical pass, the map entry and the thread's share of the tile's sum
  double acc = 0.0;
  for (int i = tid; i < out_h * out_w; i += BLOCK) {
    const int r = i / out_w, q = i % out_w;
    double mx = 0.0, my = 0.0, exx = 0.0, eyy = 0.0, exy = 0.0;
    for (int k = 0; k < K; k++) {
      const double w = wk[k];
      const int at = (r + k) * plan::TILE_W + q;
      mx += w * rows[0][at];
      my += w * rows[1][at];
      exx += w * rows[2][at];
      eyy += w * rows[3][at];
      exy += w * rows[4][at];
    }
    const double sxx = exx - mx * mx, syy = eyy - my * my, sxy = exy - mx * my;
    const double v = (2.0 * mx * my + c1) / (mx * mx + my * my + c1) * (2.0 * sxy + c2) / (sxx + syy + c2);
    acc += v;
    if (map) map[(((int64_t)n * s.C + c) * s.mh + (y0 + r)) * s.mw + (x0 + q)] = v;
  }
  const double total = block_sum(red, tid, acc);
  if (tid == 0) partials[blockIdx.x] = total;
}

inline bool image_of(const void* data, int u8, const int64_t* strides, Image& im) {
  if (!data || !strides) return false;
  for (int a = 0; a < 4; a++)
    if (strides[a] < 0) return false;
  im = Image{data, strides[0], strides[1], strides[2], strides[3], u8 ? 1 : 0};
  return true;
}
// an absent mask is a valid mask
inline bool mask_of(const void* data, int u8, const int64_t* strides, Image& im) {
  im = Image{nullptr, 0, 0, 0, 0, 0};
  return !data || image_of(data, u8, strides, im);
}
inline bool positive(double v) { return v > 0.0 && v <= 1.7976931348623157e308; }

}  // namespace

extern "C" {

int psdf_image_eval_plan(int64_t N, int C, int H, int W, int kernel_size, int downsample, int64_t* out) {
  if (!out) return PSDF_ERR_ARG;
  const plan::Plan p = plan::plan(N, C, H, W, kernel_size, downsample != 0);
  if (p.status != plan::PLAN_OK) return p.status;
  const int64_t fields[PSDF_IMAGE_EVAL_PLAN_FIELDS] = {p.factor, p.ph, p.pw, p.mh, p.mw, plan::TILE_H, plan::TILE_W, p.tiles_y,
                                                       p.tiles_x, p.ssim_workspace_bytes, p.sq_partials, p.sq_workspace_bytes,
                                                       plan::MAX_KERNEL, plan::LDS_BYTES};
  for (int i = 0; i < PSDF_IMAGE_EVAL_PLAN_FIELDS; i++) out[i] = fields[i];
  return PSDF_OK;
}

int64_t psdf_image_sq_diff_partials(int H, int W) { return plan::sq_partials(H, W); }

int psdf_image_sq_diff(const void* pred, int pred_u8, const int64_t* pred_strides, const void* gt, int gt_u8,
                       const int64_t* gt_strides, const void* mask, int mask_u8, const int64_t* mask_strides, int64_t N, int C, int H,
                       int W, double data_range, double* workspace, double* out, void* stream) {
  if (N < 0) return PSDF_ERR_ARG;
  if (N == 0) return PSDF_OK;
  Image p, g, m;
  if (C < 1 || H < 1 || W < 1 || !positive(data_range) || !workspace || !out) return PSDF_ERR_ARG;
  if (!image_of(pred, pred_u8, pred_strides, p) || !image_of(gt, gt_u8, gt_strides, g) || !mask_of(mask, mask_u8, mask_strides, m))
    return PSDF_ERR_ARG;
  const int64_t per_image = plan::sq_partials(H, W);
  if (N > plan::MAX_GRID || per_image > plan::MAX_GRID / N) return PSDF_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(sq_diff_kernel, dim3((unsigned)(N * per_image)), dim3(BLOCK), 0, (hipStream_t)stream, p, g, m, C, H, W,
                     per_image, data_range, workspace);
  PSDF_LAUNCH_CHECK();
  hipLaunchKernelGGL(finish_kernel, dim3((unsigned)N), dim3(BLOCK), 0, (hipStream_t)stream, (const double*)workspace, per_image, 1.0,
                     out);
  PSDF_LAUNCH_CHECK();
  return PSDF_OK;
}

int psdf_image_ssim(const void* pred, int pred_u8, const int64_t* pred_strides, const void* gt, int gt_u8, const int64_t* gt_strides,
                    const void* mask, int mask_u8, const int64_t* mask_strides, int64_t N, int C, int H, int W, double data_range,
                    int kernel_size, double kernel_sigma, double k1, double k2, int downsample, double* workspace, double* out,
                    double* map, void* stream) {
  if (N < 0) return PSDF_ERR_ARG;
  if (N == 0) return PSDF_OK;
  const plan::Plan pl = plan::plan(N, C, H, W, kernel_size, downsample != 0);
  if (pl.status != plan::PLAN_OK) return pl.status;
  Image p, g, m;
  Weights weights{};
  if (!positive(data_range) || !std::isfinite(k1) || !std::isfinite(k2) || !workspace || !out) return PSDF_ERR_ARG;
  if (!plan::gaussian_weights(kernel_size, kernel_sigma, weights.w)) return PSDF_ERR_ARG;
  if (!image_of(pred, pred_u8, pred_strides, p) || !image_of(gt, gt_u8, gt_strides, g) || !mask_of(mask, mask_u8, mask_strides, m))
    return PSDF_ERR_ARG;
  const SsimShape shape{C, pl.factor, pl.mh, pl.mw, pl.tiles_y, pl.tiles_x, kernel_size};
  hipLaunchKernelGGL(ssim_kernel, dim3((unsigned)(N * pl.ssim_partials)), dim3(BLOCK), 0, (hipStream_t)stream, p, g, m, shape, weights,
                     data_range, k1 * k1, k2 * k2, workspace, map);
  PSDF_LAUNCH_CHECK();
  hipLaunchKernelGGL(finish_kernel, dim3((unsigned)N), dim3(BLOCK), 0, (hipStream_t)stream, (const double*)workspace,
                     pl.ssim_partials, (double)C * (double)pl.mh * (double)pl.mw, out);
  PSDF_LAUNCH_CHECK();
  return PSDF_OK;
}

}  // extern "C"
