// Fitting the SDF network to an oriented point cloud, for gfx950: the batch of a step and the whole loss tail.
//
// The reference fits a field to a mesh in permuto_sdf_py/train_sdf_from_mesh.py and to a mesh sequence in train_4d_sdf.py, with
// the loss sdf_loss of permuto_sdf_py/utils/sdf_utils.py:16-57.  Two entries replace what those scripts do around the network:
//
//   (a) psdf_sdf_fit_batch: ONE launch writes a step's batch -- n_surf rows of the cloud (points [M, P] and normals [M, 3])
//       gathered by index, then n_off rows lo + u * (hi - lo) from uniform numbers u (train_sdf_from_mesh.py:118-123,
//       train_4d_sdf.py:200-208: randint, two index_select, rand_points_inside, rand, two cat).  P is 3, or 4 with time as the
//       last column.  AN INDEX IS CLAMPED TO [0, M - 1] BEFORE IT IS USED: a bad index reads the first or the last row of the
//       cloud, it cannot read outside it.
//   (b) psdf_sdf_fit_loss: the four terms of sdf_loss, their weighted sum and its gradient w.r.t. the SDF and the SDF gradient
//       in one call.  With g the first three columns of a row of `gradients` (the time column of a 4-D field does not enter,
//       train_4d_sdf.py:213), s its SDF value and n its normal:
//         0  mean over all rows      w | |g| - 1 |,   w = exp(-s^2 / (2 c^2)) under an eikonal clamp c, else 1 (w is a constant
//                                                     of differentiation: sdf_utils.py:24 detaches it)
//         1  mean over surface rows  1 - (g / max(|g|, 1e-8)) . (n / max(|n|, 1e-8))
//         2  mean over surface rows  |s|
//         3  mean over the others    exp(-sharpness |s|)
//       sign(0) = 0 in both absolute values, the gradient of |g| at g = 0 is 0, a mean over no rows is 0 and gives no gradient.
//       The clamp of term 1 acts on the VALUE of the norm only, its derivative stays that of |g| (F.cosine_similarity clamps
//       the norms in place outside the graph): d cos / d g = u / a - cos g / (a |g|), a = max(|g|, 1e-8), u = n / max(|n|, 1e-8).
//
// The reduction is deterministic: a fixed, capped grid (sdf_fit_plan.h); every thread adds its rows in a fixed order in double,
// a __syncthreads tree over LDS adds a workgroup's threads, each workgroup writes its four partial sums to the caller's
// workspace, and a one-workgroup finishing launch adds them in a fixed order.  There are no floating-point atomics -- the same
// inputs give the same bits on every call -- and nothing here is specific to the device compiler: the file also compiles as
// C++ against tests/host/hip_on_host, where tests/host/sdf_fit_kernels_check.cpp runs it.  Grids and blocks are one-dimensional,
// the block size is a compile-time constant.  The entries allocate nothing and never synchronise.
#include "psdf_common.h"
#include "sdf_fit_plan.h"
#include "../../include/psdf.h"

using namespace psdf;
namespace plan = psdf::sdf_fit_plan;

namespace {

constexpr int BLOCK = plan::BLOCK;
constexpr int TERMS = plan::TERMS;
constexpr float NORM_EPS = 1e-8f;   // eps of F.cosine_similarity (sdf_utils.py:35 leaves the default)

struct Box {
  float lo[4], hi[4];
};

// ---- (a) the batch ----------------------------------------------------------------------------------------------------------------
template <int P>
__global__ void __launch_bounds__(BLOCK)
    batch_kernel(int64_t M, int64_t n_surf, int64_t n_off, const float* __restrict__ cloud_points,
                 const float* __restrict__ cloud_normals, const int64_t* __restrict__ indices, const float* __restrict__ uniforms,
                 Box box, float* __restrict__ points, float* __restrict__ normals) {
  const int64_t r = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (r < n_surf) {
    int64_t i = indices[r];
    i = i < 0 ? 0 : (i > M - 1 ? M - 1 : i);      // never outside the cloud, whatever the index says
#pragma unroll
    for (int c = 0; c < P; c++) points[r * P + c] = cloud_points[i * P + c];
#pragma unroll
    for (int c = 0; c < 3; c++) normals[r * 3 + c] = cloud_normals[i * 3 + c];
  } else if (r < n_surf + n_off) {
    const int64_t j = r - n_surf;
#pragma unroll
    for (int c = 0; c < P; c++) points[r * P + c] = box.lo[c] + uniforms[j * P + c] * (box.hi[c] - box.lo[c]);
  }
}

// ---- (b) the loss tail --------------------------------------------------------------------------------------------------------------
struct LossArgs {
  // scale * weights[k] / (rows of term k's mean), 0 for an empty mean: what a row's derivative of term k is multiplied with
  float coef[TERMS];
  float sharpness;
  float two_c2;    // 2 c^2 of the eikonal clamp; <= 0: no clamp
  int want_grad;
};

__device__ __forceinline__ float sign0(float x) { return (float)((x > 0.0f) - (x < 0.0f)); }

// sums over the workgroup of the four accumulators, in a fixed order; every thread calls it, once per kernel
__device__ __forceinline__ void block_sums(double (*red)[BLOCK], int tid, const double* acc) {
  for (int k = 0; k < TERMS; k++) red[k][tid] = acc[k];
  __syncthreads();
  for (int s = BLOCK / 2; s > 0; s >>= 1) {
    if (tid < s)
      for (int k = 0; k < TERMS; k++) red[k][tid] += red[k][tid + s];
    __syncthreads();
  }
}

template <int P>
__global__ void __launch_bounds__(BLOCK)
    loss_kernel(int64_t n_surf, int64_t N, int64_t stride, const float* __restrict__ sdf, const float* __restrict__ gradients,
                const float* __restrict__ normals, LossArgs a, double* __restrict__ partials, float* __restrict__ grad_sdf,
                float* __restrict__ grad_gradients) {
  __shared__ double red[TERMS][BLOCK];
  const int tid = (int)threadIdx.x;
  double acc[TERMS] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t r = (int64_t)blockIdx.x * BLOCK + tid; r < N; r += stride) {
    const float s = sdf[r];
    const float gx = gradients[r * P], gy = gradients[r * P + 1], gz = gradients[r * P + 2];
    const float len = sqrtf(gx * gx + gy * gy + gz * gz);
    // 0: eikonal, in absolute value, under the Gaussian of the SDF value
    const float e = len - 1.0f;
    const float w = a.two_c2 > 0.0f ? expf(-(s * s) / a.two_c2) : 1.0f;
    acc[0] += (double)(w * fabsf(e));
    const float ke = len > 0.0f ? a.coef[0] * w * sign0(e) / len : 0.0f;
    float dx = ke * gx, dy = ke * gy, dz = ke * gz, ds;
    if (r < n_surf) {
      // 1: alignment with the normal; 2: |s|
      const float nx = normals[r * 3], ny = normals[r * 3 + 1], nz = normals[r * 3 + 2];
      const float nlen = sqrtf(nx * nx + ny * ny + nz * nz);
      const float ga = fmaxf(len, NORM_EPS), nb = fmaxf(nlen, NORM_EPS);
      const float ux = nx / nb, uy = ny / nb, uz = nz / nb;
      const float c = (gx / ga) * ux + (gy / ga) * uy + (gz / ga) * uz;
      acc[1] += (double)(1.0f - c);
      acc[2] += (double)fabsf(s);
      // d cos / d g = u / a - cos g / (a |g|); the second part is d |g| / d g, 0 at g = 0
      const float back = len > 0.0f ? c / (ga * len) : 0.0f;
      dx -= a.coef[1] * (ux / ga - back * gx);
      dy -= a.coef[1] * (uy / ga - back * gy);
      dz -= a.coef[1] * (uz / ga - back * gz);
      ds = a.coef[2] * sign0(s);
    } else {
      // 3: off the surface the SDF is not to be near zero
      const float ex = expf(-(a.sharpness * fabsf(s)));
      acc[3] += (double)ex;
      ds = -(a.coef[3] * a.sharpness * sign0(s) * ex);
    }
    if (a.want_grad) {
      grad_sdf[r] = ds;
      grad_gradients[r * P] = dx;
      grad_gradients[r * P + 1] = dy;
      grad_gradients[r * P + 2] = dz;
      if (P == 4) grad_gradients[r * P + 3] = 0.0f;
    }
  }
  block_sums(red, tid, acc);
  if (tid < TERMS) partials[(int64_t)blockIdx.x * TERMS + tid] = red[tid][0];
}

struct FinishArgs {
  double count[TERMS];       // rows of the mean; 0: an empty mean, which is 0
  double weight[TERMS];      // scale * weights[k]
};

// terms[k] = (sum of the partials of term k: thread t takes t, t + BLOCK, ... and then the tree) / count;  loss += sum weight terms
__global__ void __launch_bounds__(BLOCK)
    finish_kernel(const double* __restrict__ partials, int groups, FinishArgs f, float* __restrict__ terms, float* __restrict__ loss) {
  __shared__ double red[TERMS][BLOCK];
  const int tid = (int)threadIdx.x;
  double acc[TERMS] = {0.0, 0.0, 0.0, 0.0};
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

}  // namespace

extern "C" {

int psdf_sdf_fit_plan(int64_t n_surf, int64_t n_off, int64_t* out) {
  if (!out) return PSDF_ERR_ARG;
  const plan::Plan p = plan::plan(n_surf, n_off);
  if (p.status != plan::PLAN_OK) return p.status;
  out[0] = p.loss_grid;
  out[1] = p.workspace_bytes;
  out[2] = plan::ROWS_PER_PASS;
  out[3] = p.batch_grid;
  return PSDF_OK;
}

int psdf_sdf_fit_batch(int P, int64_t M, int64_t n_surf, int64_t n_off, const float* cloud_points, const float* cloud_normals,
                       const int64_t* indices, const float* uniforms, const float* lo, const float* hi, float* points,
                       float* normals, void* stream) {
  const plan::Plan p = plan::plan(n_surf, n_off);
  if (p.status != plan::PLAN_OK) return p.status;
  if (n_surf + n_off == 0) return PSDF_OK;
  if (P != 3 && P != 4) return PSDF_ERR_ARG;
  if (M < 0 || !points) return PSDF_ERR_ARG;
  if (n_surf > 0 && (M < 1 || !cloud_points || !cloud_normals || !indices || !normals)) return PSDF_ERR_ARG;
  if (n_off > 0 && (!uniforms || !lo || !hi)) return PSDF_ERR_ARG;
  if (M > plan::MAX_ROWS) return PSDF_ERR_UNSUPPORTED;
  Box box{};
  for (int c = 0; c < P && n_off > 0; c++) box.lo[c] = lo[c], box.hi[c] = hi[c];
  const dim3 grid((unsigned)p.batch_grid), block(BLOCK);
  if (P == 3)
    hipLaunchKernelGGL(batch_kernel<3>, grid, block, 0, (hipStream_t)stream, M, n_surf, n_off, cloud_points, cloud_normals, indices,
                       uniforms, box, points, normals);
  else
    hipLaunchKernelGGL(batch_kernel<4>, grid, block, 0, (hipStream_t)stream, M, n_surf, n_off, cloud_points, cloud_normals, indices,
                       uniforms, box, points, normals);
  PSDF_LAUNCH_CHECK();
  return PSDF_OK;
}

int psdf_sdf_fit_loss(int P, int64_t n_surf, int64_t n_off, const float* sdf, const float* gradients, const float* normals,
                      const float* weights, float sharpness, float eik_clamp, float scale, double* workspace, float* terms,
                      float* loss, float* grad_sdf, float* grad_gradients, void* stream) {
  const plan::Plan p = plan::plan(n_surf, n_off);
  if (p.status != plan::PLAN_OK) return p.status;
  const int64_t N = n_surf + n_off;
  if (N == 0) return PSDF_OK;
  if (P != 3 && P != 4) return PSDF_ERR_ARG;
  if (!sdf || !gradients || !weights || !workspace || !terms || (n_surf > 0 && !normals)) return PSDF_ERR_ARG;
  if ((grad_sdf == nullptr) != (grad_gradients == nullptr)) return PSDF_ERR_ARG;
  if (!(sharpness == sharpness) || !(scale == scale) || !(eik_clamp == eik_clamp)) return PSDF_ERR_ARG;
  const double count[TERMS] = {(double)N, (double)n_surf, (double)n_surf, (double)n_off};
  LossArgs a{};
  FinishArgs f{};
  for (int k = 0; k < TERMS; k++) {
    if (!(weights[k] == weights[k])) return PSDF_ERR_ARG;
    f.count[k] = count[k];
    f.weight[k] = (double)scale * (double)weights[k];
    a.coef[k] = count[k] > 0.0 ? (float)(f.weight[k] / count[k]) : 0.0f;
  }
  a.sharpness = sharpness;
  a.two_c2 = eik_clamp > 0.0f ? (float)(2.0 * (double)eik_clamp * (double)eik_clamp) : 0.0f;
  a.want_grad = grad_sdf != nullptr;
  const dim3 grid((unsigned)p.loss_grid), block(BLOCK);
  const int64_t stride = (int64_t)p.loss_grid * BLOCK;   // rows of one pass of the grid
  if (P == 3)
    hipLaunchKernelGGL(loss_kernel<3>, grid, block, 0, (hipStream_t)stream, n_surf, N, stride, sdf, gradients, normals, a, workspace, grad_sdf,
                       grad_gradients);
  else
    hipLaunchKernelGGL(loss_kernel<4>, grid, block, 0, (hipStream_t)stream, n_surf, N, stride, sdf, gradients, normals, a, workspace, grad_sdf,
                       grad_gradients);
  PSDF_LAUNCH_CHECK();
  hipLaunchKernelGGL(finish_kernel, dim3(1), block, 0, (hipStream_t)stream, (const double*)workspace, p.loss_grid, f, terms, loss);
  PSDF_LAUNCH_CHECK();
  return PSDF_OK;
}

}  // extern "C"
