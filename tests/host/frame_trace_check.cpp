// Stand-alone check of the resolve kernel of permuto_sdf_amd/csrc/frame_trace.hip on the CPU: the file itself is compiled as C++
// against tests/host/hip_on_host/hip/hip_runtime.h (a launch runs on the CPU, thread after thread), driven through its entry
// point and compared with a float64 transcription.  tests/test_frame_trace_host.py builds it with
// -fsanitize=address,undefined -fno-sanitize-recover=all and runs it: the planes and the dense arrays are of exactly their size,
// so an index out of bounds is a sanitizer report; pixels outside the chunk must keep their canary.
//
// What a valid ray (slot >= 0) must hold, u = 2^-24:
//   rgb           the bits of its dense row; weights_sum exactly 1
//   normals       n = g / max(|g|, eps), eps the fp32 value of 1e-12.  |g|^2 is three products and two sums of non-negative terms
//                 (at most 3u relative), the root halves that and rounds once (2.5u on |g|), the quotient rounds once more:
//                 3.5u |n_c| <= 3.5u to first order.  bar 4u per component.  (A gradient so small that its squares underflow
//                 meets eps in the denominator on both sides: n = g / eps, far below the bar.)
//   normals_cam   normalize(R n) of the kernel's OWN fp32 normal n: three products and two sums per entry c (at most 4u A_c,
//                 A_c = sum_j |R_cj| |n_j|), then the normalisation as above: bar |e|_2 / |c| + 4u
//   depth         ((px - ox) dx + (py - oy) dy) + (pz - oz) dz: every term carries the rounding of its difference (u), of its
//                 product (u) and of at most two sums (2u): 4u S to first order, S = sum_i |(p_i - o_i) d_i|.  bar 5u S (the
//                 fifth u is room for the second-order terms).
// Every other ray of the chunk holds exactly 0 in all five planes.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>
// cross-lane operations and launch geometry that csrc/composite_device.h names in helpers the resolve kernel never calls
template <class T> T __shfl(T v, int, int) { return v; }
template <class T> T __shfl_down(T v, int, int) { return v; }
inline thread_local dim3 gridDim;

#include "frame_trace.hip"

using std::vector;

static int failures = 0;
static const float CANARY = -77.25f;
static const double U = 1.0 / 16777216.0;
static double worst_n = 0.0, worst_c = 0.0, worst_d = 0.0;

static void fail(const char* what, long a = 0, long b = 0) {
  failures++;
  fprintf(stderr, "FAILED: %s (%ld, %ld)\n", what, a, b);
}

static uint32_t lcg_state = 12345u;
static float uni() {   // uniform in [0, 1), 24 bits
  lcg_state = lcg_state * 1664525u + 1013904223u;
  return (float)(lcg_state >> 8) / 16777216.0f;
}
static float sym(float s) { return s * (2.0f * uni() - 1.0f); }

// a rotation that is no permutation: 50 degrees about (1, 2, 3) / sqrt(14), float64 rounded to float32
static void rotation(float* R) {
  const double n = std::sqrt(14.0), a[3] = {1.0 / n, 2.0 / n, 3.0 / n};
  const double K[9] = {0.0, -a[2], a[1], a[2], 0.0, -a[0], -a[1], a[0], 0.0};
  const double th = 50.0 * M_PI / 180.0, s = std::sin(th), c1 = 1.0 - std::cos(th);
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) {
      double kk = 0.0;
      for (int j = 0; j < 3; j++) kk += K[3 * r + j] * K[3 * j + c];
      R[3 * r + c] = (float)((r == c ? 1.0 : 0.0) + s * K[3 * r + c] + c1 * kk);
    }
}

static bool same_bits(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

static void run(int H, int W, long first, int R, bool with_cam, const char* label) {
  const long HW = (long)H * W;
  // about half of the rays valid, in ray order; the first valid ray has a zero gradient, the second one of length 1e-20
  vector<int> slot(R);
  int M = 0;
  for (int i = 0; i < R; i++) slot[i] = uni() < 0.5f ? M++ : -1;
  if (R >= 8 && M < 2) return fail("the pattern holds fewer than two valid rays", R, M);
  vector<float> o(3 * (size_t)R), d(3 * (size_t)R), pos(3 * (size_t)M), grad(3 * (size_t)M), rgb(3 * (size_t)M);
  for (int i = 0; i < R; i++) {
    float dd[3] = {sym(1.f), sym(1.f), 0.2f + uni()};
    const float n = sqrtf(dd[0] * dd[0] + dd[1] * dd[1] + dd[2] * dd[2]);
    for (int k = 0; k < 3; k++) o[3 * i + k] = sym(1.5f), d[3 * i + k] = dd[k] / n;
  }
  for (int m = 0; m < M; m++)
    for (int k = 0; k < 3; k++) pos[3 * m + k] = sym(0.5f), grad[3 * m + k] = sym(2.0f), rgb[3 * m + k] = uni();
  if (M >= 2) {
    grad[0] = grad[1] = grad[2] = 0.f;
    grad[3] = 1e-20f, grad[4] = 0.f, grad[5] = 0.f;
  }
  float rot[9];
  rotation(rot);
  vector<float> img(3 * HW, CANARY), nimg(3 * HW, CANARY), cimg(3 * HW, CANARY), wimg(HW, CANARY), dimg(HW, CANARY);
  const int status = psdf_trace_frame_resolve(R, M, slot.data(), o.data(), d.data(), M ? pos.data() : nullptr, M ? grad.data() : nullptr,
                                              M ? rgb.data() : nullptr, with_cam ? rot : nullptr, H, W, first, img.data(), nimg.data(),
                                              with_cam ? cimg.data() : nullptr, wimg.data(), dimg.data(), nullptr);
  if (status != 0) return fail(label, status);
  // a second call on the same inputs: the same bits
  vector<float> img2(3 * HW, CANARY), nimg2(3 * HW, CANARY), cimg2(3 * HW, CANARY), wimg2(HW, CANARY), dimg2(HW, CANARY);
  if (psdf_trace_frame_resolve(R, M, slot.data(), o.data(), d.data(), M ? pos.data() : nullptr, M ? grad.data() : nullptr,
                               M ? rgb.data() : nullptr, with_cam ? rot : nullptr, H, W, first, img2.data(), nimg2.data(),
                               with_cam ? cimg2.data() : nullptr, wimg2.data(), dimg2.data(), nullptr) != 0)
    return fail(label, -1);
  if (std::memcmp(img.data(), img2.data(), 12 * HW) || std::memcmp(nimg.data(), nimg2.data(), 12 * HW) ||
      std::memcmp(cimg.data(), cimg2.data(), 12 * HW) || std::memcmp(wimg.data(), wimg2.data(), 4 * HW) ||
      std::memcmp(dimg.data(), dimg2.data(), 4 * HW))
    fail("two runs differ", first, R);
  const double eps = (double)1e-12f;
  for (long p = 0; p < HW; p++) {
    const bool inside = p >= first && p < first + R;
    if (!inside || !with_cam)
      for (int k = 0; k < 3; k++)
        if (cimg[k * HW + p] != CANARY) fail("a camera normal outside the chunk, or an unasked one, was written", p, k);
    if (!inside) {
      for (int k = 0; k < 3; k++)
        if (img[k * HW + p] != CANARY || nimg[k * HW + p] != CANARY) fail("a canary outside the chunk was written", p, k);
      if (wimg[p] != CANARY || dimg[p] != CANARY) fail("a canary outside the chunk was written", p, 3);
      continue;
    }
    const int i = (int)(p - first), s = slot[i];
    if (s < 0) {
      bool zero = wimg[p] == 0.f && dimg[p] == 0.f;
      for (int k = 0; k < 3; k++) zero = zero && img[k * HW + p] == 0.f && nimg[k * HW + p] == 0.f && (!with_cam || cimg[k * HW + p] == 0.f);
      if (!zero) fail("an invalid ray is not all zero", p);
      continue;
    }
    if (wimg[p] != 1.f) fail("a valid ray's weight is not 1", p);
    double g[3], gn = 0.0, S = 0.0, depth = 0.0;
    for (int k = 0; k < 3; k++) {
      if (!same_bits(img[k * HW + p], rgb[3 * s + k])) fail("a colour is not the dense row's bits", p, k);
      g[k] = grad[3 * s + k];
      gn += g[k] * g[k];
      const double t = ((double)pos[3 * s + k] - (double)o[3 * i + k]) * (double)d[3 * i + k];
      depth += t;
      S += std::fabs(t);
    }
    gn = std::sqrt(gn);
    for (int k = 0; k < 3; k++) {
      const double err = std::fabs((double)nimg[k * HW + p] - g[k] / std::max(gn, eps));
      worst_n = std::max(worst_n, err / (4 * U));
      if (!(err <= 4 * U)) fail("a normal misses its bar", p, k);
    }
    if (s == 0 && M >= 2)
      for (int k = 0; k < 3; k++)
        if (nimg[k * HW + p] != 0.f || (with_cam && cimg[k * HW + p] != 0.f)) fail("a zero gradient has a normal", p, k);
    {
      const double err = std::fabs((double)dimg[p] - depth), bar = 5 * U * S;
      worst_d = std::max(worst_d, err / bar);
      if (!(err <= bar)) fail("a depth misses its bar", p);
    }
    if (with_cam) {
      double c[3], e2 = 0.0, cn = 0.0;
      for (int r = 0; r < 3; r++) {
        double A = 0.0;
        c[r] = 0.0;
        for (int j = 0; j < 3; j++) c[r] += (double)rot[3 * r + j] * (double)nimg[j * HW + p], A += std::fabs((double)rot[3 * r + j] * (double)nimg[j * HW + p]);
        e2 += (4 * U * A) * (4 * U * A);
        cn += c[r] * c[r];
      }
      cn = std::sqrt(cn);
      const double bar = std::sqrt(e2) / std::max(cn, 1e-300) + 4 * U;
      for (int r = 0; r < 3; r++) {
        const double err = std::fabs((double)cimg[r * HW + p] - c[r] / std::max(cn, 1e-300));
        worst_c = std::max(worst_c, err / bar);
        if (!(err <= bar)) fail("a camera normal misses its bar", p, r);
      }
    }
  }
  printf("%-34s %d x %d, pixels [%ld, %ld), %d valid: ok\n", label, H, W, first, first + R, M);
}

int main() {
  run(7, 13, 0, 7 * 13, true, "a whole frame, no multiple of 64");
  run(40, 48, 77, 333, true, "an unaligned chunk across rows");
  run(40, 48, 77, 333, false, "the same without camera normals");
  run(7, 13, 90, 1, true, "the last pixel");
  // a chunk without a valid ray comes without the dense arrays
  {
    const int H = 7, W = 13, R = 40, first = 20;
    vector<int> slot(R, -1);
    vector<float> o(3 * R, 1.f), d(3 * R, 1.f), img(3 * H * W, CANARY), nimg(3 * H * W, CANARY), wimg(H * W, CANARY), dimg(H * W, CANARY);
    if (psdf_trace_frame_resolve(R, 0, slot.data(), o.data(), d.data(), nullptr, nullptr, nullptr, nullptr, H, W, first, img.data(),
                                 nimg.data(), nullptr, wimg.data(), dimg.data(), nullptr) != 0)
      fail("no valid ray");
    for (int p = 0; p < H * W; p++) {
      const float want = (p >= first && p < first + R) ? 0.f : CANARY;
      if (wimg[p] != want || dimg[p] != want || img[p] != want || img[2 * H * W + p] != want || nimg[H * W + p] != want) fail("no valid ray: planes", p);
    }
  }
  // an empty chunk returns before any pointer check; the refusals
  if (psdf_trace_frame_resolve(0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, nullptr, nullptr, nullptr,
                               nullptr, nullptr, nullptr) != 0)
    fail("empty chunk");
  {
    int slot[4] = {-1, -1, -1, -1};
    float ray[12] = {0}, plane[3 * 91];
    auto call = [&](int R, int M, const int* s, const float* dense, int H, int W, long first, float* out, float* cam, const float* rot) {
      return psdf_trace_frame_resolve(R, M, s, ray, ray, dense, dense, dense, rot, H, W, first, out, out, cam, out, out, nullptr);
    };
    if (call(4, 0, slot, nullptr, 7, 13, 88, plane, nullptr, nullptr) != -1) fail("a range past the frame is accepted");
    if (call(4, 0, slot, nullptr, 0, 13, 0, plane, nullptr, nullptr) != -1) fail("H = 0 is accepted");
    if (call(4, 0, slot, nullptr, 7, -1, 0, plane, nullptr, nullptr) != -1) fail("W < 1 is accepted");
    if (call(4, 0, slot, nullptr, 7, 13, -1, plane, nullptr, nullptr) != -1) fail("a negative first pixel is accepted");
    if (call(-1, 0, slot, nullptr, 7, 13, 0, plane, nullptr, nullptr) != -1) fail("nr_rays < 0 is accepted");
    if (call(4, 5, slot, ray, 7, 13, 0, plane, nullptr, nullptr) != -1) fail("more valid rays than rays are accepted");
    if (call(4, 1, slot, nullptr, 7, 13, 0, plane, nullptr, nullptr) != -1) fail("valid rays without dense arrays are accepted");
    if (call(4, 0, nullptr, nullptr, 7, 13, 0, plane, nullptr, nullptr) != -1) fail("a NULL slot is accepted");
    if (call(4, 0, slot, nullptr, 7, 13, 0, nullptr, nullptr, nullptr) != -1) fail("a NULL plane is accepted");
    if (call(4, 0, slot, nullptr, 7, 13, 0, plane, plane, nullptr) != -1) fail("camera normals without the rotation are accepted");
    if (call(4, 0, slot, nullptr, 65536, 32768, 0, plane, nullptr, nullptr) != -2) fail("a frame of 2^31 pixels is accepted");
  }
  printf("worst error / bar: normals %.3f, camera normals %.3f, depth %.3f\n", worst_n, worst_c, worst_d);
  if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
  else printf("frame_trace_check: all checks passed\n");
  return failures;
}
