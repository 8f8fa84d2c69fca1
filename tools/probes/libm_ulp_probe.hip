// Worst observed error, in fp32 ulps of the float64 result, of the device expf / log1pf / __expf / acosf over the argument
// ranges the compositing kernels and the loss tails use (csrc/neus.hip, composite_device.h, csrc/volume_rendering.hip).  The
// figures feed ULP_EXPF, ULP_LOG1PF and ULP_FAST_EXPF of oracle/composite_float64.py and ULP_ACOSF of oracle/tails_float64.py
// (worst observed, rounded up to a whole ulp, plus one).
//   hipcc -O3 -ffp-contract=off --offload-arch=gfx950 tools/probes/libm_ulp_probe.hip -o tools/probes/libm_ulp_probe
// Every fp32 value of each range is visited when the range holds fewer than 2^26 of them, else 2^26 evenly spaced bit patterns.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

__device__ __forceinline__ float fn(int which, float x) {
  return which == 0 ? expf(x) : which == 1 ? log1pf(x) : which == 2 ? __expf(x) : acosf(x);
}

__global__ void eval(int which, uint32_t lo_bits, uint32_t step, uint32_t count, float* out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  out[i] = fn(which, __uint_as_float(lo_bits + i * step));
}

static float bits(uint32_t b) {
  float f;
  memcpy(&f, &b, 4);
  return f;
}
static uint32_t as_bits(float f) {
  uint32_t b;
  memcpy(&b, &f, 4);
  return b;
}

// fp32 values of one sign between a and b (|a| < |b|): consecutive bit patterns
static void run(const char* name, int which, float a, float b) {
  const uint32_t lo = as_bits(a), hi = as_bits(b);
  uint64_t span = (uint64_t)hi - lo + 1;
  uint32_t step = 1;
  while (span / step > (1u << 26)) step++;
  const uint32_t count = (uint32_t)(span / step);
  float* d = nullptr;
  if (hipMalloc(&d, (size_t)count * 4) != hipSuccess) {
    printf("%s: allocation failed\n", name);
    return;
  }
  hipLaunchKernelGGL(eval, dim3((count + 255) / 256), dim3(256), 0, 0, which, lo, step, count, d);
  float* h = new float[count];
  if (hipMemcpy(h, d, (size_t)count * 4, hipMemcpyDeviceToHost) != hipSuccess) {
    printf("%s: copy failed\n", name);
    return;
  }
  double worst = 0.0;
  float worst_x = 0.f;
  for (uint32_t i = 0; i < count; i++) {
    const float x = bits(lo + i * step);
    const double ref = which == 1 ? log1p((double)x) : which == 3 ? acos((double)x) : exp((double)x);
    if (!(ref >= 1.1754943508222875e-38) || !(ref < 3.4e38)) continue;   // normal results only: below that the bar is absolute
    int e;
    frexp(ref, &e);
    const double ulp = ldexp(1.0, e - 24);
    const double err = fabs((double)h[i] - ref) / ulp;
    if (err > worst) {
      worst = err;
      worst_x = x;
    }
  }
  printf("%-8s on [%g, %g]: %u arguments (every %u-th fp32 value), worst error %.3f ulp at x = %.9g\n", name, a, b, count, step,
         worst, worst_x);
  delete[] h;
  (void)hipFree(d);
}

int main() {
  // expf: sigmoid arguments are +-(sdf +- ic dt / 2) inv_s, up to ~1e5 in magnitude (expf saturates past +-88); the density
  // activation's expf(raw) on [-30, 20]; exp(-density dt)
  run("expf", 0, 1e-8f, 88.7f);
  run("expf", 0, -1e-8f, -87.3f);
  // log1pf(expf(x)) for x in [-30, 20]: arguments from 1e-13 to 4.9e8
  run("log1pf", 1, 1e-14f, 5e8f);
  // __expf(-sigma dt) of volume_render_nerf: the early-out at T < 1e-4 keeps the products that matter above -20
  run("__expf", 2, -1e-8f, -20.0f);
  run("__expf", 2, -20.0f, -87.3f);
  // acosf(clamp(n(a) . n(b), -1 + 1e-6, 1 - 1e-6)) of curvature_loss_kernel: the fp32 clamp edges are the last arguments
  run("acosf", 3, 1e-30f, 1.0f - 1e-6f);
  run("acosf", 3, -1e-30f, -1.0f + 1e-6f);
  return 0;
}
