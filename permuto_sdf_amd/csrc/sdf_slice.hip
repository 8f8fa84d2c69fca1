// Cross-sections of an SDF for gfx950: the layer of points of the reference's create_sdf_isolines
// (permuto_sdf_py/experiments/visualization/visualize_sdf_isolines.py:62-166, again in render_from_frame.py:71-166), its colour
// map with 15 iso-bands, and the depth test of the layer against a rendered view, which the reference leaves to its viewer.
// The network runs between these kernels on the masked kernels the tracers use (sdf_slice.py): points -> masked encode ->
// masked MLP (1-row head) -> colorize for a layer, cut_begin -> the same pair -> cut_resolve for a view.
//
// The layer.  Cell k of an S x S layer has row k / S (the y index) and column k % S (the x index), the order of the reference's
// transpose(0, 1).reshape(-1, 3).  Lattice coordinates are float32 in the reference's order, (float(i) / S - 0.5f) * 2.0f, times
// extent_scale (1: the reference's [-1, 1)); z is the layer depth.  The plane's axes are the COLUMNS of a row-major 3 x 3 host
// matrix A (the reference's cam.cam_axes()).  RESTATED, UNPINNED: the reference rotates in float64 inside easypbr
// (apply_model_matrix_to_cpu), whose source is absent; here component c of a point is (x A[c][0] + y A[c][1]) + z A[c][2] in
// float64, products and sums rounded one by one, rounded to float32 once.
//
// The colours.  base = table(map_range(sdf, 0, 0.3, 0.2, 1.0)), map_range as common_utils.py:150-154 with its clamp, in float32:
// out_lo + scale * (clamp(sdf) - in_lo), the scale a host float.  RESTATED, UNPINNED: easypbr's "pubu" table and its
// interpolation are absent; `table` is K control points [K, 3] on the device and table(t), t clamped to [0, 1], is evaluated in
// float32 in this order: u = t * float(K - 1); j = min(int(u), K - 2); f = u - float(j); channel = a + f * (b - a) with a, b the
// control points j and j + 1 -- a difference, a product, a sum.  A cell is in band i iff sdf > lo_i && sdf < hi_i in float32,
// both strict; the last matching band wins (the order in which the reference's loop overwrites); a NaN matches no band and
// takes the colour 0.  The band table (at most 32 lines) and the two map records travel in the kernel arguments.
//
// The cut.  For a ray o + t d of a view and the plane through z n (n the third axis): t = dot(n, z n - o) / dot(n, d) in
// float32, the point o + t d, in-plane coordinates dot(a0, p) and dot(a1, p).  The ray takes part iff the denominator is not 0,
// t > 0, both coordinates lie in [-extent, extent), the point is strictly inside the box, and the pixel has no surface
// (weights_sum == 0) or t < depth.
//
// The box test is AABB.check_point_inside_primitive (permuto_sdf_py/utils/aabb.py:28-42), strict about the translation:
// box_inside of frame_device.h, the one the box tracer steps with.  One thread per cell or per ray, one-dimensional grid, no cross-lane operation, no LDS, every
// element written by one thread: the file also compiles as C++ against tests/host/hip_on_host, where
// tests/host/sdf_slice_kernels_check.cpp runs it.  The entries allocate nothing and never synchronise.
#include "frame_device.h"
#include "sdf_slice_plan.h"
#include "../../include/psdf.h"

using namespace psdf;
namespace splan = psdf::sdf_slice_plan;

namespace {

struct Axes {
  float m[9];      // row major; column j is axis j
};

__host__ inline Axes axes9(const float* p) {
  Axes a;
  for (int i = 0; i < 9; i++) a.m[i] = p[i];
  return a;
}

// common_utils.py:150-154 (x is not a NaN here)
__device__ __forceinline__ float map_range(const splan::MapRange& m, float x) {
  const float c = x < m.in_lo ? m.in_lo : (x > m.in_hi ? m.in_hi : x);
  return m.out_lo + m.scale * (c - m.in_lo);
}

__device__ __forceinline__ v3 table_at(const float* __restrict__ table, int K, float t) {
  t = t < 0.f ? 0.f : (t > 1.f ? 1.f : t);
  const float u = t * (float)(K - 1);
  int j = (int)u;                            // u >= 0: the truncation is the floor
  j = j > K - 2 ? K - 2 : j;
  const float f = u - (float)j;
  const float* a = table + 3 * j;
  return mk3(a[0] + f * (a[3] - a[0]), a[1] + f * (a[4] - a[1]), a[2] + f * (a[5] - a[2]));
}

// visualize_sdf_isolines.py:119-138 for one value
__device__ __forceinline__ v3 iso_colour(float s, const float* __restrict__ table, int K, const splan::MapRange& base,
                                         const splan::Bands& bands) {
  if (s != s) return mk3(0.f, 0.f, 0.f);
  v3 c = table_at(table, K, map_range(base, s));
  for (int i = 0; i < bands.n; i++)
    if (s > bands.lo[i] && s < bands.hi[i]) c = mk3(bands.rgb[i][0], bands.rgb[i][1], bands.rgb[i][2]);
  return c;
}

__global__ void __launch_bounds__(splan::BLOCK)
    slice_points_kernel(int count, int first, int S, int stride, Axes A, float z, float extent_scale, Triple tr, Triple half,
                        const float* __restrict__ time, float* __restrict__ pts, unsigned char* __restrict__ skip) {
  const int i = blockIdx.x * splan::BLOCK + threadIdx.x;
  if (i >= count) return;
  const int k = first + i, row = k / S, col = k % S;
  const float Sf = (float)S;
  const float xf = (((float)col / Sf - 0.5f) * 2.0f) * extent_scale, yf = (((float)row / Sf - 0.5f) * 2.0f) * extent_scale;
  const double x = (double)xf, y = (double)yf, zz = (double)z;
  float q[3];
#pragma unroll
  for (int c = 0; c < 3; c++) q[c] = (float)((x * (double)A.m[3 * c] + y * (double)A.m[3 * c + 1]) + zz * (double)A.m[3 * c + 2]);
  const v3 p = mk3(q[0], q[1], q[2]);
  float* out = pts + (int64_t)stride * i;
  st3(out, p);
  if (stride == 4) out[3] = time[0];
  skip[i] = box_inside(tr, half, p) ? 0 : 1;
}

__global__ void __launch_bounds__(splan::BLOCK)
    slice_colorize_kernel(int count, int64_t first, int64_t plane, const float* __restrict__ sdf,
                          const unsigned char* __restrict__ skip, const float* __restrict__ table, int K, splan::MapRange base,
                          splan::Bands bands, float* __restrict__ rgb, float* __restrict__ sdf_img, float* __restrict__ inside_img) {
  const int i = blockIdx.x * splan::BLOCK + threadIdx.x;
  if (i >= count) return;
  const int64_t cell = first + i;
  v3 c = mk3(0.f, 0.f, 0.f);
  float s = 0.f, in = 0.f;
  if (!skip[i]) {
    s = sdf[i];
    in = 1.f;
    c = iso_colour(s, table, K, base, bands);
  }
  st_planes(rgb, plane, cell, c);
  sdf_img[cell] = s;
  inside_img[cell] = in;
}

__global__ void __launch_bounds__(splan::BLOCK)
    slice_cut_begin_kernel(int nr_rays, int stride, Axes A, float z, float extent, Triple tr, Triple half,
                           const float* __restrict__ origins, const float* __restrict__ dirs, const float* __restrict__ time,
                           int64_t pixel_first, const float* __restrict__ weights_sum_img, const float* __restrict__ depth_img,
                           float* __restrict__ pts, unsigned char* __restrict__ skip, float* __restrict__ t_out) {
  const int i = blockIdx.x * splan::BLOCK + threadIdx.x;
  if (i >= nr_rays) return;
  const v3 o = ld3(origins + 3 * (int64_t)i), d = ld3(dirs + 3 * (int64_t)i);
  const v3 a0 = mk3(A.m[0], A.m[3], A.m[6]), a1 = mk3(A.m[1], A.m[4], A.m[7]), n = mk3(A.m[2], A.m[5], A.m[8]);
  const float den = dot3(n, d), num = dot3(n, z * n - o);
  const float t = num / den;      // den == 0: an infinity or a NaN, which no comparison below accepts
  const v3 p = along(o, t, d);
  const float u = dot3(a0, p), v = dot3(a1, p);
  bool take = den != 0.f && t > 0.f && u >= -extent && u < extent && v >= -extent && v < extent && box_inside(tr, half, p);
  if (take) {
    const int64_t pixel = pixel_first + i;
    take = weights_sum_img[pixel] == 0.f || t < depth_img[pixel];
  }
  float* out = pts + (int64_t)stride * i;
  st3(out, take ? p : o);         // a ray that does not take part stays at its origin and is never evaluated
  if (stride == 4) out[3] = time[0];
  skip[i] = take ? 0 : 1;
  t_out[i] = take ? t : 0.f;
}

__global__ void __launch_bounds__(splan::BLOCK)
    slice_cut_resolve_kernel(int nr_rays, int64_t pixel_first, int64_t plane, const float* __restrict__ sdf,
                             const unsigned char* __restrict__ skip, const float* __restrict__ t, const float* __restrict__ table,
                             int K, splan::MapRange base, splan::Bands bands, float* __restrict__ rgb_img,
                             float* __restrict__ depth_img, float* __restrict__ weights_sum_img, float* __restrict__ slice_mask_img) {
  const int i = blockIdx.x * splan::BLOCK + threadIdx.x;
  if (i >= nr_rays) return;
  const int64_t pixel = pixel_first + i;
  if (skip[i]) {
    slice_mask_img[pixel] = 0.f;
    return;
  }
  st_planes(rgb_img, plane, pixel, iso_colour(sdf[i], table, K, base, bands));
  depth_img[pixel] = t[i];
  weights_sum_img[pixel] = 1.f;
  slice_mask_img[pixel] = 1.f;
}

// the colour arguments of colorize and cut_resolve -> the two records; PSDF_OK or PSDF_ERR_ARG
__host__ inline int colour_args(const float* table, int K, const float* base_map, int nr_lines, const float* band_lo,
                                const float* band_hi, const float* band_rgb, splan::MapRange* base, splan::Bands* bands) {
  if (!table || K < splan::MIN_TABLE || K > splan::MAX_TABLE || !base_map) return PSDF_ERR_ARG;
  if (splan::check_lines(nr_lines) != splan::PLAN_OK) return PSDF_ERR_ARG;
  if (nr_lines > 0 && (!band_lo || !band_hi || !band_rgb)) return PSDF_ERR_ARG;
  *base = splan::MapRange{base_map[0], base_map[1], base_map[2], base_map[3]};
  bands->n = nr_lines;
  for (int i = 0; i < splan::MAX_LINES; i++) {
    const bool on = i < nr_lines;
    bands->lo[i] = on ? band_lo[i] : 0.f;
    bands->hi[i] = on ? band_hi[i] : 0.f;
    for (int c = 0; c < 3; c++) bands->rgb[i][c] = on ? band_rgb[3 * i + c] : 0.f;
  }
  return PSDF_OK;
}

}  // namespace

extern "C" {

int psdf_slice_points(int S, int64_t first, int count, int stride, const float* axes, float z, float extent_scale,
                      const float* translation, const float* half, const float* time, float* pts, uint8_t* skip, void* stream) {
  if (count == 0) return PSDF_OK;
  if (splan::check_stride(stride) != splan::PLAN_OK) return PSDF_ERR_ARG;
  if (const int range = frame_plan::check_range(S, S, first, count)) return range;
  if (!axes || !translation || !half || !pts || !skip || (stride == 4 && !time)) return PSDF_ERR_ARG;
  hipLaunchKernelGGL(slice_points_kernel, dim3(splan::grid(count)), dim3(splan::BLOCK), 0, (hipStream_t)stream, count, (int)first, S,
                     stride, axes9(axes), z, extent_scale, triple(translation), triple(half), time, pts, skip);
  PSDF_LAUNCH_CHECK();
  return PSDF_OK;
}

int psdf_slice_colorize(int S, int64_t first, int count, const float* sdf, const uint8_t* skip, const float* table, int K,
                        const float* base_map, int nr_lines, const float* band_lo, const float* band_hi, const float* band_rgb,
                        float* rgb, float* sdf_img, float* inside_img, void* stream) {
  if (count == 0) return PSDF_OK;
  splan::MapRange base;
  splan::Bands bands;
  const int colours = colour_args(table, K, base_map, nr_lines, band_lo, band_hi, band_rgb, &base, &bands);
  if (colours != PSDF_OK) return colours;
  if (const int range = frame_plan::check_range(S, S, first, count)) return range;
  if (!sdf || !skip || !rgb || !sdf_img || !inside_img) return PSDF_ERR_ARG;
  hipLaunchKernelGGL(slice_colorize_kernel, dim3(splan::grid(count)), dim3(splan::BLOCK), 0, (hipStream_t)stream, count, first,
                     (int64_t)S * S, sdf, skip, table, K, base, bands, rgb, sdf_img, inside_img);
  PSDF_LAUNCH_CHECK();
  return PSDF_OK;
}

int psdf_slice_cut_begin(int nr_rays, int stride, const float* axes, float z, float extent, const float* translation,
                         const float* half, const float* origins, const float* dirs, const float* time, int H, int W,
                         int64_t pixel_first, const float* weights_sum_img, const float* depth_img, float* pts, uint8_t* skip,
                         float* t, void* stream) {
  if (nr_rays == 0) return PSDF_OK;
  if (splan::check_stride(stride) != splan::PLAN_OK) return PSDF_ERR_ARG;
  if (const int range = frame_plan::check_range(H, W, pixel_first, nr_rays)) return range;
  if (!axes || !translation || !half || !origins || !dirs || !weights_sum_img || !depth_img || !pts || !skip || !t)
    return PSDF_ERR_ARG;
  if (stride == 4 && !time) return PSDF_ERR_ARG;
  hipLaunchKernelGGL(slice_cut_begin_kernel, dim3(splan::grid(nr_rays)), dim3(splan::BLOCK), 0, (hipStream_t)stream, nr_rays, stride,
                     axes9(axes), z, extent, triple(translation), triple(half), origins, dirs, time, pixel_first, weights_sum_img,
                     depth_img, pts, skip, t);
  PSDF_LAUNCH_CHECK();
  return PSDF_OK;
}

int psdf_slice_cut_resolve(int nr_rays, const float* sdf, const uint8_t* skip, const float* t, const float* table, int K,
                           const float* base_map, int nr_lines, const float* band_lo, const float* band_hi, const float* band_rgb,
                           int H, int W, int64_t pixel_first, float* rgb_img, float* depth_img, float* weights_sum_img,
                           float* slice_mask_img, void* stream) {
  if (nr_rays == 0) return PSDF_OK;
  splan::MapRange base;
  splan::Bands bands;
  const int colours = colour_args(table, K, base_map, nr_lines, band_lo, band_hi, band_rgb, &base, &bands);
  if (colours != PSDF_OK) return colours;
  if (const int range = frame_plan::check_range(H, W, pixel_first, nr_rays)) return range;
  if (!sdf || !skip || !t || !rgb_img || !depth_img || !weights_sum_img || !slice_mask_img) return PSDF_ERR_ARG;
  hipLaunchKernelGGL(slice_cut_resolve_kernel, dim3(splan::grid(nr_rays)), dim3(splan::BLOCK), 0, (hipStream_t)stream, nr_rays,
                     pixel_first, (int64_t)H * W, sdf, skip, t, table, K, base, bands, rgb_img, depth_img, weights_sum_img,
                     slice_mask_img);
  PSDF_LAUNCH_CHECK();
  return PSDF_OK;
}

}  // extern "C"
