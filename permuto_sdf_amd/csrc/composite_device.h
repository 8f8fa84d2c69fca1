// The ONE definition of what the compositing kernels share (volume_rendering.hip, neus.hip, composite_fused.hip,
// frame_composite.hip): the ray-range accessor of a packed sample container, the transmittance step of a 64-sample chunk and the
// forward sweep of a ray around it, the suffix step of the fused backwards, the two opacities with their backwards -- the
// section-point opacity of VolumeRenderingNeus.compute_weights (permuto_sdf_py/volume_rendering/volume_rendering_modules.py:
// 129-163), the NeRF opacity 1 - exp(-softplus(raw) dt) (models.py:520, volume_rendering_modules.py:72-86), the mid-point rule
// of sdf2alpha -- and F.normalize.  Everything is __forceinline__ and the library is built with -ffp-contract=off: a kernel
// that calls a helper rounds exactly as if the expressions stood in its body, in the order they are written here.
#pragma once
#include "psdf_common.h"

namespace {
using namespace psdf;

__device__ __forceinline__ float sigm(float x) { return 1.0f / (1.0f + expf(-x)); }

struct Section {   // everything the backward needs again
  float tc, pre_a, pre_b, ic, en, ep, pc, nc, p, c, q;
};

__device__ __forceinline__ Section section(float sdf, v3 dir, v3 grad, float dt, float inv_s, float r) {
  Section s;
  s.tc = (dir.x * grad.x + dir.y * grad.y) + dir.z * grad.z;            // (dirs * gradients).sum(-1)
  s.pre_a = -s.tc * 0.5f + 0.5f;
  s.pre_b = -s.tc;
  s.ic = -(fmaxf(s.pre_a, 0.f) * (1.0f - r) + fmaxf(s.pre_b, 0.f) * r); // always non-positive
  const float half = s.ic * dt * 0.5f;
  s.en = sdf + half;
  s.ep = sdf - half;
  s.pc = sigm(s.ep * inv_s);
  s.nc = sigm(s.en * inv_s);
  s.p = s.pc - s.nc;
  s.c = s.pc;
  s.q = (s.p + 1e-5f) / (s.c + 1e-5f);
  return s;
}

// torch.clip(q, 0, 1) of the opacity: a NaN stays a NaN (fminf / fmaxf return the bound instead, which turned a NaN sdf into
// alpha = 0, a transparent sample).  For finite inputs with dt >= 0 no bound is ever active from below: ic <= 0 gives
// en <= ep, so nc <= pc up to the monotonicity of expf, p >= -(a few ulp) and q = (p + 1e-5) / (pc + 1e-5) lies in (0, 1].
// Hence the `gq = 0` arm of section_backward (q outside [0, 1]) is taken by a NaN q alone, where it changes nothing:
// g_p = 0 / NaN is NaN all the same, as in torch's backward of clip followed by the division.
__device__ __forceinline__ float clip01(float q) { return q < 0.0f ? 0.0f : (q > 1.0f ? 1.0f : q); }

// Backward of alpha = clip01(section(..).q) for an upstream g_alpha: g_sdf, g_tc (dL/d tc: g_gradients = g_tc * dir) and this
// sample's term of dL/d inv_s.
struct SectionGrad {
  float g_sdf, g_tc, g_inv_s;
};
__device__ __forceinline__ SectionGrad section_backward(const Section& s, float g_alpha, float dt, float inv_s, float r) {
  // clip(q, 0, 1) passes the gradient inside the closed interval (torch.clamp): the 0 arm is reached by a NaN q alone (clip01)
  const float gq = (s.q >= 0.0f && s.q <= 1.0f) ? g_alpha : 0.0f;
  const float den = s.c + 1e-5f;
  const float g_p = gq / den;
  const float g_c = -gq * (s.p + 1e-5f) / (den * den);
  const float g_up = (g_p + g_c) * (s.pc * (1.0f - s.pc));              // through sigmoid(ep * inv_s)
  const float g_un = -g_p * (s.nc * (1.0f - s.nc));                     // through sigmoid(en * inv_s)
  const float g_ep = g_up * inv_s, g_en = g_un * inv_s;
  const float g_ic = (g_en - g_ep) * (dt * 0.5f);
  SectionGrad g;
  g.g_inv_s = g_up * s.ep + g_un * s.en;
  g.g_sdf = g_ep + g_en;
  // ic = -(relu(pre_a) (1-r) + relu(pre_b) r);  pre_a = -tc/2 + 1/2;  pre_b = -tc
  g.g_tc = g_ic * ((s.pre_a > 0.f ? 0.5f * (1.0f - r) : 0.f) + (s.pre_b > 0.f ? r : 0.f));
  return g;
}

// NeRF opacity: density = softplus(raw) with torch's threshold, alpha = 1 - exp(-density dt); e = exp(-density dt) is what the
// backward needs again
__device__ __forceinline__ float softplus20(float x) { return x > 20.0f ? x : log1pf(expf(x)); }
struct NerfAlpha {
  float a, e;
};
__device__ __forceinline__ NerfAlpha nerf_alpha(float raw, float dt) {
  NerfAlpha r;
  r.e = expf(-softplus20(raw) * dt);
  r.a = 1.0f - r.e;
  return r;
}
// -> dL/d raw
__device__ __forceinline__ float nerf_alpha_backward(float g_alpha, float e, float raw, float dt) {
  const float g_dens = g_alpha * e * dt;                                 // alpha = 1 - exp(-dens dt)
  return g_dens * (raw > 20.0f ? 1.0f : sigm(raw));                      // softplus' = sigmoid
}

// sdf2alpha (VolumeRenderingGPU.cuh:490): the opacity of the interval between two neighbouring samples of a ray by the NeuS
// mid-point rule, in the reference's mix of float and double
__device__ __forceinline__ float sigmoidf(float x) { return (float)(1.0 / (1.0 + (double)expf(-x))); }
__device__ __forceinline__ float sdf2alpha_midpoint(float prev, float next, float dt, float inv_s) {
  const float mid = (float)((double)(prev + next) * 0.5);
  float cosv = (next - prev) / fmaxf(dt, 1e-6f);
  cosv = clampf(cosv, -1e3f, 0.0f);
  const float half = (float)((double)(cosv * dt) * 0.5);
  const float prev_cdf = sigmoidf((mid - half) * inv_s);
  const float next_cdf = sigmoidf((mid + half) * inv_s);
  return (float)(((double)(prev_cdf - next_cdf) + 1e-6) / ((double)prev_cdf + 1e-6));
}

// F.normalize(x, dim=-1) (eps 1e-12) and its backward
struct Nrm {
  v3 y;
  float norm, denom;
};
__device__ __forceinline__ Nrm normalize_eps(v3 x) {
  Nrm r;
  r.norm = sqrtf(dot3(x, x));
  r.denom = fmaxf(r.norm, 1e-12f);
  r.y = v3{x.x / r.denom, x.y / r.denom, x.z / r.denom};
  return r;
}
// gradient of y = x / max(|x|, eps) for an upstream gy
__device__ __forceinline__ v3 normalize_bwd(const Nrm& n, v3 gy) {
  const float inv = 1.0f / n.denom;
  v3 g = inv * gy;
  if (n.norm > 1e-12f) {   // the clamp passes the gradient of the norm only above eps
    const float s = dot3(gy, n.y) * inv;
    g = g - s * n.y;
  }
  return g;
}

struct RayIndex {
  const int* __restrict__ start_end;  // [R,2]
  int equal;                          // rays_have_equal_nr_of_samples
  int fixed;                          // fixed_nr_of_samples_per_ray
  int max_nr_samples;
  __device__ __forceinline__ void get(int ray, int& s, int& e) const {
    if (equal) {
      s = ray * fixed;
      e = s + fixed;
    } else {
      s = start_end[2 * ray];
      e = start_end[2 * ray + 1];
    }
  }
  // the reference skips rays whose reservation overflowed the pool, and empty rays
  __device__ __forceinline__ bool valid(int s, int e) const { return !(e > max_nr_samples || e == s); }
};

#define RAY_LOOP(ray, nr_rays) \
  for (int ray = blockIdx.x * (PSDF_BLOCK / 64) + (threadIdx.x >> 6); ray < nr_rays; ray += gridDim.x * (PSDF_BLOCK / 64))

static inline unsigned ray_grid(int nr_rays) {
  unsigned b = psdf_blocks(nr_rays, PSDF_BLOCK / 64);
  return b < 16384u ? (b ? b : 1u) : 16384u;
}

// ------------------------------------------------------------------------------------------- transmittance, forward
// what the transmittance product is fed for a sample of opacity a (1 - alpha + 1e-7)
__device__ __forceinline__ float one_minus(float a) { return (1.0f - a) + 1e-7f; }

// T of the 64 samples of a chunk from their factors: exclusive product scan over the lanes times the product of the chunks
// before.  After a ray's last chunk `carry` is its background transmittance.
struct Transmittance {
  float carry = 1.f;
  __device__ __forceinline__ float step(float factor, int lane) {
    const float incl = wave_incl_scan_mul(factor);
    float excl = __shfl_up(incl, 1, 64);
    if (lane == 0) excl = 1.f;
    const float T = carry * excl;
    carry = carry * __shfl(incl, 63, 64);
    return T;
  }
};

// One 64-sample chunk of the forward sweep of a ray of n samples that starts at s: a = opacity(m) of sample m and its factor
// 1 - a + 1e-7 into the product (the last sample's factor never enters: the bg transmittance is T of the last sample, as in
// cumprod_fwd_kernel).  Lanes past the ray's end (`in` false) evaluate its last sample again, so every lane of the scan holds
// finite work and no load is out of range.
struct Sample {
  int64_t m;   // index into the pool
  float a, T;
  bool in;     // this lane holds a sample of the ray
};
template <class Opacity>
__device__ __forceinline__ Sample sweep_chunk(Transmittance& tr, int s, int n, int base, int lane, Opacity&& opacity) {
  const int i = base + lane;
  Sample c;
  c.in = i < n;
  c.m = s + (c.in ? i : n - 1);
  c.a = opacity(c.m);
  c.T = tr.step((i < n - 1) ? one_minus(c.a) : 1.f, lane);
  return c;
}
// the whole ray, any length: per_sample(m, a, T) for every sample -> the background transmittance
template <class Opacity, class PerSample>
__device__ __forceinline__ float sweep(int s, int n, int lane, Opacity&& opacity, PerSample&& per_sample) {
  Transmittance tr;
  for (int base = 0; base < n; base += 64) {
    const Sample c = sweep_chunk(tr, s, n, base, lane, opacity);
    if (c.in) per_sample(c.m, c.a, c.T);
  }
  return tr.carry;
}

// ------------------------------------------------------------------------------------------ transmittance, backward
// inclusive SUFFIX sum over the 64 lanes (mirror image of wave_incl_scan_add: the same tree, so the same roundings as the
// separate cumsum kernel's scan over the reversed ray)
__device__ __forceinline__ float wave_incl_suffix_add(float v) {
  const int l = lane_id();
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float t = __shfl_down(v, o, 64);
    if (l + o < 64) v += t;
  }
  return v;
}

// Sweep 2 of the fused backwards, one chunk at a time FROM THE RAY'S END: v = g_T T of the chunk's samples -> cs[i + 1], the
// sum of v over all samples behind sample i (cumsum_kernel, inverse), and from it dL/d (1 - alpha + 1e-7) of sample i =
// (cs[i + 1] + gb) / max(om, 1e-6) with gb = g_bg bg (cumprod_bwd_kernel); gb == NULL: no background term.
struct SuffixStep {
  float tail = 0.f;                  // sum of v over the chunks behind the current one
  __device__ __forceinline__ float g_one_minus(float v, float a, const float* gb, int i, int n, int lane) {
    const float suf = wave_incl_suffix_add(v) + tail;               // cs[i] = sum_{j >= i} v[j]
    float cs_next = __shfl_down(suf, 1, 64);                        // cs[i + 1]
    if (lane == 63) cs_next = tail;
    tail = __shfl(suf, 0, 64);
    float g_om = 0.f;
    if (i < n - 1) {
      const float om = fmaxf(one_minus(a), 1e-6f);
      g_om = cs_next / om;
      if (gb) g_om += *gb / om;
    }
    return g_om;
  }
};

// A ray longer than the caller declared (max_per_ray): the register-held chunks of the fused backwards would silently drop its
// tail.  Fail loudly instead: every gradient of the ray becomes NaN (the C ABI has no other error channel out of a kernel).
__device__ __forceinline__ float poison() { return __int_as_float(0x7fc00000); }
template <class Store>
__device__ __forceinline__ void poison_ray(int s, int n, int lane, Store&& store) {
  for (int i = lane; i < n; i += 64) store((int64_t)s + i, poison());
}

}  // namespace
