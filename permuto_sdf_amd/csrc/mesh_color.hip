// Per-vertex colour of an extracted surface, for gfx950: the glue around the colour network when it is asked about the vertices
// of a mesh (permuto_sdf_amd/mesh_color.py) instead of the samples of a ray.
//
// The colour network (RgbNet, models.py:310-391) takes x = [colour encoding | SH5(view direction) | normalize(sdf gradient) |
// geometry features].  Training assembles that from operators (ManualTrainer._fg_forward: an SH launch, a normalize launch, a
// torch.cat with two transposes) because a sample's view direction comes from its ray.  A vertex has no ray: its view direction
// is made up from its own normal, or from one eye position.  Hence
//
//   (a) psdf_mesh_color_inputs: vertex, SDF gradient, the SDF net's feature-major output -> rows [c_enc, C) of the colour
//       network's feature-major input x_fm [C, n] (the colour encoding's rows [0, c_enc) are written by the encode kernel, into
//       the same buffer), and optionally the view directions and the outward unit normals as [n, 3];
//   (b) psdf_mesh_color_finish: the colour head's feature-major output [3, n] -> float colours [n, 3] and 8-bit colours [n, 3].
//
// One thread per vertex; every feature-major access is contiguous over the lanes of a wave.  No atomics, no LDS, no cross-lane
// operation, nothing returns to the host.  The expressions are the ones the operators evaluate -- normalize_eps
// (composite_device.h: psdf_normalize3), sh_eval (sh_device.h: psdf_spherical_harmonics), 1 / (1 + expf(-z))
// (sigmoid_rows_kernel, neus.hip: psdf_sigmoid_rows) -- and the library is built with -ffp-contract=off: the same bits.
// The 8-bit rule is image_eval.to_u8's: clamp(rint(rgb * 255), 0, 255), ties to even.
//
// The file also compiles as C++ against tests/host/hip_on_host, where tests/host/mesh_color_kernels_check.cpp runs both kernels.
#include "mesh_color_plan.h"
#include "composite_device.h"
#include "sh_device.h"
#include "../../include/psdf.h"

using namespace psdf;
namespace plan = psdf::mesh_color_plan;

namespace {

constexpr int BLOCK = plan::BLOCK;

// --------------------------------------------------------------------------------------------------------- (a) inputs
__global__ void __launch_bounds__(BLOCK)
    mesh_color_inputs_kernel(int64_t n, const float* __restrict__ points, const float* __restrict__ gradients,
                             const float* __restrict__ y_fm, int g, int mode, const float* __restrict__ eye, float* __restrict__ x_fm,
                             int sh_row, float* __restrict__ dirs, float* __restrict__ normals) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  const v3 nrm = normalize_eps(ld3(gradients + 3 * i)).y;
  v3 d;
  if (mode == plan::MODE_CAMERA) d = normalize_eps(ld3(points + 3 * i) - ld3(eye)).y;
  else d = v3{-nrm.x, -nrm.y, -nrm.z};
  float* col = x_fm + i;      // this vertex's column; row r is col[r * n]
  sh_eval(plan::SH_DEGREE, d.x, d.y, d.z, ShRows{col + (int64_t)sh_row * n, n});
  const int64_t nr = (int64_t)sh_row + plan::SH;
  col[nr * n] = nrm.x;
  col[(nr + 1) * n] = nrm.y;
  col[(nr + 2) * n] = nrm.z;
  const int64_t gr = nr + plan::NORMAL;
  for (int k = 0; k < g; k++) col[(gr + k) * n] = y_fm[(int64_t)(1 + k) * n + i];      // row 0 of y_fm is the SDF
  if (dirs) st3(dirs + 3 * i, d);
  if (normals) st3(normals + 3 * i, nrm);
}

// --------------------------------------------------------------------------------------------------------- (b) finish
__global__ void __launch_bounds__(BLOCK)
    mesh_color_finish_kernel(int64_t n, const float* __restrict__ raw_fm, float* __restrict__ rgb, uint8_t* __restrict__ rgb_u8) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const float y = 1.0f / (1.0f + expf(-raw_fm[(int64_t)c * n + i]));
    if (rgb) rgb[3 * i + c] = y;
    // y lies in [0, 1] or is a NaN: rintf gives an integer in [0, 255], the clamp holds a NaN at 0 (fmaxf returns the bound)
    if (rgb_u8) rgb_u8[3 * i + c] = (uint8_t)fminf(fmaxf(rintf(y * 255.0f), 0.0f), 255.0f);
  }
}

}  // namespace

extern "C" {

int psdf_mesh_color_plan(int rgb_enc_width, int g, int mlp_in, int64_t n, int64_t chunk, int64_t* out) {
  if (!out) return PSDF_ERR_ARG;
  plan::Plan p;
  const int status = plan::plan(rgb_enc_width, g, mlp_in, n, chunk, &p);
  if (status != plan::PLAN_OK) return status;
  out[0] = p.r.c_enc, out[1] = p.r.c_sh, out[2] = p.r.c_normal, out[3] = p.r.c_geom, out[4] = p.r.C;
  out[5] = p.nr_chunks, out[6] = p.last_chunk;
  return PSDF_OK;
}

int psdf_mesh_color_inputs(int64_t n, const float* points, const float* gradients, const float* y_fm, int g, int mode,
                           const float* eye, float* x_fm, int C, int sh_row, float* dirs, float* normals, void* stream) {
  if (n == 0) return PSDF_OK;
  if (n < 0 || g < 0 || sh_row < 0 || (mode != plan::MODE_NORMAL && mode != plan::MODE_CAMERA)) return PSDF_ERR_ARG;
  // the rows written, [sh_row, sh_row + 25 + 3 + g), must be the LAST rows of x_fm [C, n]: nothing is written outside it
  if ((int64_t)sh_row + plan::SH + plan::NORMAL + g != (int64_t)C) return PSDF_ERR_ARG;
  if (!gradients || !x_fm || (g > 0 && !y_fm) || (mode == plan::MODE_CAMERA && (!points || !eye))) return PSDF_ERR_ARG;
  if (C > plan::MAX_ROWS) return PSDF_ERR_UNSUPPORTED;
  const int grid = plan::grid(n);
  if (grid < 0) return grid;
  hipLaunchKernelGGL(mesh_color_inputs_kernel, dim3((unsigned)grid), dim3(BLOCK), 0, (hipStream_t)stream, n, points, gradients, y_fm, g,
                     mode, eye, x_fm, sh_row, dirs, normals);
  PSDF_LAUNCH_CHECK();
  return PSDF_OK;
}

int psdf_mesh_color_finish(int64_t n, const float* raw_fm, float* rgb, uint8_t* rgb_u8, void* stream) {
  if (n == 0) return PSDF_OK;
  if (n < 0 || !raw_fm) return PSDF_ERR_ARG;
  const int grid = plan::grid(n);
  if (grid < 0) return grid;
  if (!rgb && !rgb_u8) return PSDF_OK;      // nothing asked for
  hipLaunchKernelGGL(mesh_color_finish_kernel, dim3((unsigned)grid), dim3(BLOCK), 0, (hipStream_t)stream, n, raw_fm, rgb, rgb_u8);
  PSDF_LAUNCH_CHECK();
  return PSDF_OK;
}

}  // extern "C"
