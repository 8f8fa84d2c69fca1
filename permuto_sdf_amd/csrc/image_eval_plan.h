// image_eval_plan.h -- the host arithmetic behind the launches of image_eval.hip, in one place: the pooling factor of the SSIM,
// the pooled and map extents, the tiling of the map over workgroups, the sizes of the partial-sum workspaces and the Gaussian
// window.  Integers and doubles only: no HIP, no device, no state -- a plain C++17 compiler accepts this header, and
// tests/host/image_eval_plan_check.cpp runs it under the address and undefined-behaviour sanitizers.
#pragma once
#include <cmath>
#include <cstdint>

namespace psdf {
namespace image_eval_plan {

constexpr int PLAN_OK = 0, PLAN_ERR_ARG = -1, PLAN_ERR_UNSUPPORTED = -2;

constexpr int BLOCK = 256;   // threads of every workgroup of image_eval.hip
// One workgroup of the SSIM kernel owns TILE_H x TILE_W entries of the map of one (image, channel).  Its LDS holds the pooled
// tile of both images with the window's halo, (TILE_H + K - 1) x (TILE_W + K - 1) doubles each, the five horizontally filtered
// moments, (TILE_H + K - 1) x TILE_W doubles each, the reduction's BLOCK doubles and the weights: LDS_BYTES at K = MAX_KERNEL,
// below 64 KiB, so two workgroups share the 160 KiB of a CU.
constexpr int TILE_H = 16, TILE_W = 32;
constexpr int MAX_KERNEL = 15;
constexpr int IN_H = TILE_H + MAX_KERNEL - 1, IN_W = TILE_W + MAX_KERNEL - 1;
constexpr int MOMENTS = 5;   // E[x], E[y], E[x^2], E[y^2], E[xy]
constexpr int LDS_BYTES = (2 * IN_H * IN_W + MOMENTS * IN_H * TILE_W + BLOCK + MAX_KERNEL) * 8;
// pixels (all channels of each) per workgroup of the squared-difference kernel: one partial sum per SQ_PIXELS pixels of an image
constexpr int SQ_PIXELS_PER_THREAD = 8;
constexpr int SQ_PIXELS = BLOCK * SQ_PIXELS_PER_THREAD;
constexpr int64_t MAX_GRID = 0x7fffffffll;   // workgroups of a 1-D launch

// max(1, round_half_even(min_side / 256)): Python's round(min(H, W) / 256), without a floating-point division
inline int pooling_factor(int min_side) {
  const int q = min_side / 256, r = min_side % 256;
  const int rounded = r > 128 ? q + 1 : (r == 128 ? q + (q & 1) : q);
  return rounded < 1 ? 1 : rounded;
}

// partial sums per image of the squared difference; -1: no such image
inline int64_t sq_partials(int H, int W) {
  if (H < 1 || W < 1) return -1;
  return ((int64_t)H * W + SQ_PIXELS - 1) / SQ_PIXELS;
}

struct Plan {
  int status;                     // PLAN_OK, or why there is no plan (every other field 0)
  int factor;                     // f: the images are averaged over f x f blocks, stride f, remainders dropped
  int ph, pw;                     // pooled extents: H / f, W / f
  int mh, mw;                     // extents of the map: ph - K + 1, pw - K + 1 (valid windows only)
  int tiles_y, tiles_x;           // workgroups along the map of one (image, channel)
  int64_t ssim_partials;          // per image: C * tiles_y * tiles_x
  int64_t ssim_workspace_bytes;   // N * ssim_partials doubles
  int64_t sq_partials;            // per image
  int64_t sq_workspace_bytes;     // N * sq_partials doubles
};

inline Plan plan(int64_t N, int C, int H, int W, int kernel_size, bool downsample) {
  Plan p{};
  p.status = PLAN_ERR_ARG;
  if (N < 0 || C < 1 || H < 1 || W < 1) return p;
  if (kernel_size < 1 || kernel_size % 2 == 0 || kernel_size > MAX_KERNEL) return p;
  const int f = downsample ? pooling_factor(H < W ? H : W) : 1;
  const int ph = H / f, pw = W / f;
  if (ph < kernel_size || pw < kernel_size) return p;
  const int mh = ph - kernel_size + 1, mw = pw - kernel_size + 1;
  const int tiles_y = (mh - 1) / TILE_H + 1, tiles_x = (mw - 1) / TILE_W + 1;
  const int64_t tiles = (int64_t)tiles_y * tiles_x, sq = sq_partials(H, W);
  p.status = PLAN_ERR_UNSUPPORTED;
  if (tiles > MAX_GRID) return p;   // (and C * tiles below stays inside int64)
  const int64_t per_image = (int64_t)C * tiles;
  if (N > MAX_GRID || (N > 0 && (per_image > MAX_GRID / N || sq > MAX_GRID / N))) return p;
  p.status = PLAN_OK;
  p.factor = f;
  p.ph = ph, p.pw = pw;
  p.mh = mh, p.mw = mw;
  p.tiles_y = tiles_y, p.tiles_x = tiles_x;
  p.ssim_partials = per_image;
  p.ssim_workspace_bytes = N * per_image * 8;
  p.sq_partials = sq;
  p.sq_workspace_bytes = N * sq * 8;
  return p;
}

// w[i] = exp(-d^2 / (2 sigma^2)) / sum, d = i - (k - 1) / 2: the separable factor of the window, normalised in double
// (summed in index order).  false: no such window.
inline bool gaussian_weights(int kernel_size, double sigma, double* w) {
  if (kernel_size < 1 || kernel_size % 2 == 0 || kernel_size > MAX_KERNEL || !(sigma > 0.0) || !std::isfinite(sigma)) return false;
  double sum = 0.0;
  for (int i = 0; i < kernel_size; i++) {
    const double d = (double)i - (double)(kernel_size - 1) / 2.0;
    w[i] = std::exp(-(d * d) / (2.0 * sigma * sigma));
    sum += w[i];
  }
  for (int i = 0; i < kernel_size; i++) w[i] /= sum;
  return true;
}

}  // namespace image_eval_plan
}  // namespace psdf
