// Every GELU evaluator of the MLP kernels, once: the erf polynomial, the one-exponential rational fit, their packed forms and
// their value-and-derivative forms, with the shared vector typedefs and the two packed helpers they are written in.  Device
// only; knows nothing of the MLP plans.  WHICH evaluator a kernel takes stays at its call site (RATIONAL = (NT0 == 3) in
// mlp_bwd_split.hip, GELU_SPLIT in mlp.hip, scalar or packed); a coefficient or an error bound is changed or reviewed here.
// Forms that agree only "up to a rounding" (the forwards' max(z, 0) - |z| tail against the backwards' z cdf) are separate
// functions on purpose: unifying them would change results.
#pragma once
#include "psdf_common.h"

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 h2v_t __attribute__((ext_vector_type(2)));

namespace {

// packed fp32 arithmetic on PAIRS (v_pk_fma_f32 / v_pk_mul_f32: two lanes' worth of FMA per instruction on gfx950)
__device__ __forceinline__ f32x2 pk_fma(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f32x2 splat2(float v) { return f32x2{v, v}; }

// ------------------------------------------------------------------------------------------------ erf
// erf with < 1 ulp error, branch-free (both ranges evaluated, then selected): a ~20-instruction VALU
// sequence instead of the two-branch library erff, which matters because 96 GELUs per lane sit between
// the MFMA chains of every tile.  Polynomials: the widely used single-precision minimax pair
// (|x| <= 0.927734375: odd polynomial in x; above: 1 - exp(p(|x|))).
__device__ __forceinline__ float erf_fast(float a) {
  const float t = fabsf(a);
  const float s = a * a;
  float r = fmaf(-1.72853470e-5f, t, 3.83197126e-4f);
  float u = fmaf(-3.88396438e-3f, t, 2.42546219e-2f);
  r = fmaf(r, s, u);
  r = fmaf(r, t, -1.06777877e-1f);
  r = fmaf(r, t, -6.34846687e-1f);
  r = fmaf(r, t, -1.28717512e-1f);
  r = fmaf(r, t, -t);
  const float hi = copysignf(1.0f - __expf(r), a);
  float q = -5.96761703e-4f;
  q = fmaf(q, s, 4.99119423e-3f);
  q = fmaf(q, s, -2.67681349e-2f);
  q = fmaf(q, s, 1.12819925e-1f);
  q = fmaf(q, s, -3.76125336e-1f);
  q = fmaf(q, s, 1.28379166e-1f);
  const float lo = fmaf(q, a, a);
  return t > 0.927734375f ? hi : lo;
}

// The same erf on PAIRS of values with packed fp32 arithmetic -- identical operations in identical order, so the results are
// bit-identical to erf_fast; only the Horner chains (13 of the ~20 instructions) are paired, abs / exp / sign / select stay
// per element.
__device__ __forceinline__ f32x2 erf_fast2(f32x2 a) {
  const f32x2 t = {fabsf(a.x), fabsf(a.y)};
  const f32x2 s = a * a;
  f32x2 r = pk_fma(splat2(-1.72853470e-5f), t, splat2(3.83197126e-4f));
  const f32x2 u = pk_fma(splat2(-3.88396438e-3f), t, splat2(2.42546219e-2f));
  r = pk_fma(r, s, u);
  r = pk_fma(r, t, splat2(-1.06777877e-1f));
  r = pk_fma(r, t, splat2(-6.34846687e-1f));
  r = pk_fma(r, t, splat2(-1.28717512e-1f));
  r = pk_fma(r, t, -t);
  const f32x2 hi = {copysignf(1.0f - __expf(r.x), a.x), copysignf(1.0f - __expf(r.y), a.y)};
  f32x2 q = splat2(-5.96761703e-4f);
  q = pk_fma(q, s, splat2(4.99119423e-3f));
  q = pk_fma(q, s, splat2(-2.67681349e-2f));
  q = pk_fma(q, s, splat2(1.12819925e-1f));
  q = pk_fma(q, s, splat2(-3.76125336e-1f));
  q = pk_fma(q, s, splat2(1.28379166e-1f));
  const f32x2 lo = pk_fma(q, a, a);
  return f32x2{t.x > 0.927734375f ? hi.x : lo.x, t.y > 0.927734375f ? hi.y : lo.y};
}

// ------------------------------------------------------------------------------------ value only (the forwards)
// torch.nn.GELU() default (erf form), 0.5 x (1 + erf(x / sqrt 2)), on a pair: the fp32 forwards (mlp.hip, fused.hip)
__device__ __forceinline__ f32x2 gelu_exact2(f32x2 x) {
  return (splat2(0.5f) * x) * (splat2(1.0f) + erf_fast2(x * splat2(0.70710678118654752440f)));
}

// gelu from ONE exponential and ONE reciprocal (tools/gelu_fit_rational.py): Phi(-|z|) = t P6(t) exp(-z^2/2) with
// t = 1 / (1 + 0.39 |z|), gelu(z) = max(z, 0) - |z| Phi(-|z|).  14 instructions against ~26 for the erf form; error
// against float64 1.8e-7 |z| (torch's fp32 formula 0.5 z (1 + erf(z / sqrt 2)) itself: 1.1e-7 |z|) -- both are rounding
// noise of an fp32 evaluation, and the GPU tests hold the kernels to a multiple of torch's own fp32 error.
// One element per instruction: the form to use beside bf16 MFMAs (packed fp32 arithmetic does not hide in the shadow of
// the matrix pipe, plain VALU does: tools/mfma_valu_overlap.hip).  The split-bf16 forward is VALU bound (gelu + operand
// splitting against 156 MFMAs per tile), so it takes this evaluator: 0.799 -> 0.759 ms for the forward of the bench.
__device__ __forceinline__ float gelu_rational(float z) {
  const float E = __builtin_amdgcn_exp2f(z * z * -0.72134752044448170368f);
  const float t = __builtin_amdgcn_rcpf(fmaf(fabsf(z), 0.39f, 1.0f));
  float q = 5.384693295e-02f;
  q = fmaf(q, t, -2.582434118e-01f);
  q = fmaf(q, t, 3.751679361e-01f);
  q = fmaf(q, t, -1.663514599e-02f);
  q = fmaf(q, t, 1.944366544e-01f);
  q = fmaf(q, t, 1.514270604e-01f);
  const float tail = q * t * E;
  return fmaf(-fabsf(z), tail, fmaxf(z, 0.f));
}

// Two elements per instruction where the instruction set has a packed form (round 5): the two-piece fp16 forward issues 66
// MFMAs per tile where the bf16 one issues 156, so it is bound by the NUMBER of VALU instructions rather than by what hides
// beside the matrix pipe -- 9.5 instead of 14 instructions per element.  Same operations in the same order, fused where the
// scalar form is fused: bit-identical results.  |z| rides as a source modifier of the scalar fmas that need it.
// At four waves per SIMD (mlp_fwd_split_wg_kernel) the forward is bound by vector-ALU issue and the shorter tail below pays:
// 0.2691 -> 0.2495 ms for the forward of the bench step with the tail and the build flag alone, 0.2460 with the operand
// trims of mlp.hip / mlp_device.h (profiles/mlp_fwd_issue_trims_ab.txt); at two waves per SIMD it had measured neutral.
__device__ __forceinline__ f32x2 gelu_rational2(f32x2 z) {
  const f32x2 e = (z * z) * f32x2{-0.72134752044448170368f, -0.72134752044448170368f};
  const f32x2 E = {__builtin_amdgcn_exp2f(e.x), __builtin_amdgcn_exp2f(e.y)};
  const f32x2 t = {__builtin_amdgcn_rcpf(fmaf(fabsf(z.x), 0.39f, 1.0f)), __builtin_amdgcn_rcpf(fmaf(fabsf(z.y), 0.39f, 1.0f))};
  f32x2 q = {5.384693295e-02f, 5.384693295e-02f};
#define PSDF_H2(C) q = __builtin_elementwise_fma(q, t, f32x2{C, C});
  PSDF_H2(-2.582434118e-01f) PSDF_H2(3.751679361e-01f) PSDF_H2(-1.663514599e-02f) PSDF_H2(1.944366544e-01f) PSDF_H2(1.514270604e-01f)
#undef PSDF_H2
  const f32x2 tail = (q * t) * E;
  // the tail, one element per instruction on purpose: max(z, 0) as v_med3_f32 z, 0, FLT_MAX (fmaxf is TWO v_max_f32, a
  // canonicalisation first; with +inf as the bound the compiler folds the median back into that pair) and -|z| as the source
  // modifiers of a scalar v_fma_f32 (v_pk_fma_f32 takes no |.|: packed, -|z| costs a v_or_b32 per element -- which is what the
  // SLP vectoriser makes of the two fmas, so the forwards' file is built with -fno-slp-vectorize, build.py).  Same values for
  // every finite z; three instructions per pair shorter.
  const float mx = __builtin_amdgcn_fmed3f(z.x, 0.f, __FLT_MAX__), my = __builtin_amdgcn_fmed3f(z.y, 0.f, __FLT_MAX__);
  return f32x2{__builtin_fmaf(-__builtin_fabsf(z.x), tail.x, mx), __builtin_fmaf(-__builtin_fabsf(z.y), tail.y, my)};
}

// ------------------------------------------------------------ value and derivative (the backwards' recompute)
// gelu and its derivative Phi(z) + z phi(z) by torch's formula 0.5 z (1 + erf(z / sqrt 2)): one erf (itself one exp) and one
// more exp.  The fp32 wide backward (mlp_wide.hip) and mlp_bwd_split_kernel<4, ...> (see gelu_rational_both) use it.
__device__ __forceinline__ void gelu_erf(float z, float& hval, float& gprime) {
  const float cdf = fmaf(0.5f, erf_fast(z * 0.70710678118654752440f), 0.5f);
  const float pdf = 0.3989422804014327f * __expf(-0.5f * z * z);
  hval = z * cdf;
  gprime = fmaf(z, pdf, cdf);
}

// tools/gelu_fit_rational.py: gelu AND gelu' from ONE exponential and ONE reciprocal (the recompute needs both):
//   E = exp(-z^2/2), t = 1/(1 + p|z|), Phi(-|z|) = t P6(t) E, cdf = z < 0 ? Phi(-|z|) : 1 - Phi(-|z|),
//   gelu = z cdf, gelu' = cdf + z E / sqrt(2 pi).  17 instructions against ~30; error against float64: gelu 1.8e-7 |z|
//   (the fp32 formula 0.5 z (1 + erf(z / sqrt 2)) itself: 1.1e-7 |z|), gelu' 1.9e-7.
// Measured in mlp_bwd_split_kernel on the headline batch (profiles/r02_mlp_bwd_prototype_timings.txt): rational 1.37 ms,
// erf 1.47 ms, a pure-polynomial evaluator (tools/gelu_fit.py, gone) 1.47 ms for the double-staged instantiation (zero scratch
// in all three).  The widest instantiation (K0 > 48) is at the register limit and the rational form's extra live values spill
// there (44 B scratch; a spill reload waits for the LDS-DMA in flight), so mlp_bwd_split_kernel<4, ...> keeps gelu_erf.
__device__ __forceinline__ void gelu_rational_both(float z, float& hval, float& gprime) {
  const float E = __builtin_amdgcn_exp2f(z * z * -0.72134752044448170368f);
  const float t = __builtin_amdgcn_rcpf(fmaf(fabsf(z), 0.39f, 1.0f));
  float q = 5.384693295e-02f;
  q = fmaf(q, t, -2.582434118e-01f);
  q = fmaf(q, t, 3.751679361e-01f);
  q = fmaf(q, t, -1.663514599e-02f);
  q = fmaf(q, t, 1.944366544e-01f);
  q = fmaf(q, t, 1.514270604e-01f);
  const float tail = q * t * E;
  const float cdf = z < 0.f ? tail : 1.0f - tail;
  hval = z * cdf;
  gprime = fmaf(z, E * 0.3989422804014327f, cdf);
}

// The same fit for the four values of an MFMA result as TWO PAIRS in packed fp32 arithmetic, statement by statement: a
// dependent v_pk_fma_f32 needs a wait state after the one that feeds it, and the Horner chain of a single pair is nothing but
// such dependences (117 s_nop per tile in mlp_bwd_split_f16_kernel) -- two chains side by side fill them.  The split-fp16
// backwards (mlp_bwd_split_f16.hip, mlp_wide.hip) use it.  (The forwards evaluate the same fit as max(z, 0) - |z| Phi(-|z|),
// gelu_rational above: equal up to the last bit or two of an fp32 evaluation.)
__device__ __forceinline__ void gelu_rational4(const f32x4& z, f32x4& h, f32x4& gp) {
  const f32x2 za = {z[0], z[1]}, zb = {z[2], z[3]};
  const f32x2 ea = (za * za) * splat2(-0.72134752044448170368f), eb = (zb * zb) * splat2(-0.72134752044448170368f);
  const f32x2 Ea = {__builtin_amdgcn_exp2f(ea.x), __builtin_amdgcn_exp2f(ea.y)};
  const f32x2 Eb = {__builtin_amdgcn_exp2f(eb.x), __builtin_amdgcn_exp2f(eb.y)};
  // 1 + p |z|: two scalar fmas whose |.| is a source modifier (no instruction), instead of two v_and + one packed fma -- the
  // results only feed v_rcp_f32, which is scalar anyway; same fused arithmetic, bit-identical
  const f32x2 da = {__builtin_fmaf(__builtin_fabsf(za.x), 0.39f, 1.0f), __builtin_fmaf(__builtin_fabsf(za.y), 0.39f, 1.0f)};
  const f32x2 db = {__builtin_fmaf(__builtin_fabsf(zb.x), 0.39f, 1.0f), __builtin_fmaf(__builtin_fabsf(zb.y), 0.39f, 1.0f)};
  const f32x2 ta = {__builtin_amdgcn_rcpf(da.x), __builtin_amdgcn_rcpf(da.y)};
  const f32x2 tb = {__builtin_amdgcn_rcpf(db.x), __builtin_amdgcn_rcpf(db.y)};
  f32x2 qa = splat2(5.384693295e-02f), qb = splat2(5.384693295e-02f);
#define PSDF_H4(C) qa = pk_fma(qa, ta, splat2(C)); qb = pk_fma(qb, tb, splat2(C));
  PSDF_H4(-2.582434118e-01f) PSDF_H4(3.751679361e-01f) PSDF_H4(-1.663514599e-02f) PSDF_H4(1.944366544e-01f) PSDF_H4(1.514270604e-01f)
#undef PSDF_H4
  const f32x2 la = (qa * ta) * Ea, lb = (qb * tb) * Eb;
  // cdf = 1/2 + sign(z) (1/2 - Phi(-|z|)): one v_bfi_b32 per value instead of a compare and a select (1/2 - l >= 0 always);
  // differs from `z < 0 ? l : 1 - l` by at most one rounding of the sum (6e-8)
  const f32x2 ma = splat2(0.5f) - la, mb = splat2(0.5f) - lb;
  const f32x2 ca = f32x2{__builtin_copysignf(ma.x, za.x), __builtin_copysignf(ma.y, za.y)} + splat2(0.5f);
  const f32x2 cb = f32x2{__builtin_copysignf(mb.x, zb.x), __builtin_copysignf(mb.y, zb.y)} + splat2(0.5f);
  const f32x2 ha = za * ca, hb = zb * cb;
  const f32x2 ga = pk_fma(za, Ea * splat2(0.3989422804014327f), ca), gb = pk_fma(zb, Eb * splat2(0.3989422804014327f), cb);
  h = f32x4{ha.x, ha.y, hb.x, hb.y};
  gp = f32x4{ga.x, ga.y, gb.x, gb.y};
}

// The erf form on a pair in packed fp32 arithmetic (the fp32 backwards, mlp_bwd.hip): the same operations in the same order as
// gelu_exact2 for the value and as gelu_erf's Phi(x) + x phi(x) for the derivative.  erf_terms2: what the two forms below share.
__device__ __forceinline__ void erf_terms2(f32x2 x, f32x2& one_erf, f32x2& pdf) {
  one_erf = splat2(1.0f) + erf_fast2(x * splat2(0.70710678118654752440f));
  const f32x2 e = (splat2(-0.5f) * x) * x;
  pdf = splat2(0.3989422804014327f) * f32x2{__expf(e.x), __expf(e.y)};
}
// x -> (gelu, gelu') with one erf and one exp
__device__ __forceinline__ void gelu_erf2(f32x2 x, f32x2& h, f32x2& g1) {
  f32x2 one_erf, pdf;
  erf_terms2(x, one_erf, pdf);
  h = (splat2(0.5f) * x) * one_erf;
  g1 = pk_fma(x, pdf, splat2(0.5f) * one_erf);   // Phi + x phi
}
// x -> (gelu, gelu', gelu''): the double backward
__device__ __forceinline__ void gelu_erf2_dd(f32x2 x, f32x2& h, f32x2& g1, f32x2& g2) {
  f32x2 one_erf, pdf;
  erf_terms2(x, one_erf, pdf);
  h = (splat2(0.5f) * x) * one_erf;
  g1 = pk_fma(x, pdf, splat2(0.5f) * one_erf);   // Phi + x phi
  g2 = pdf * (splat2(2.0f) - x * x);             // 2 phi + x phi' = phi (2 - x^2)
}

}  // namespace
