// Stand-alone check of permuto_sdf_amd/csrc/colorcal.hip on the CPU: the file itself is compiled as C++ against
// tests/host/hip_on_host/hip/hip_runtime.h (launches run on the calling thread), driven the way permuto_sdf_amd/nerf_train.py
// drives it and compared with brute-force float64 written as plain loops.  tests/test_colorcal_host.py builds it with
// -fsanitize=address,undefined -fno-sanitize-recover=all and runs it: every buffer has exactly the extent include/psdf.h states,
// so an index out of bounds in a kernel is a sanitizer report here, not a fault on a device.  It says nothing about speed, and
// nothing about what the device compiler makes of the source.
//
// The forward and the fold use no cross-lane operation and run for real, on the containers of tests/colorcal_float64.py (the
// cases of the GPU file).  The backward sums a ray with a butterfly over the 16 lanes of a row; the stand-in header does not model
// lanes (its __shfl_xor returns the caller's own value), so that kernel is compiled here and NEVER RUN:
// psdf_colorcal_sigmoid_backward is called with empty batches and bad arguments only, which return before any launch.
//
// Bars (u = 2^-24), as derived in tests/colorcal_float64.py: forward E_z = (2 |raw w| + |z|) u through s (1 - s), plus
// s ((1 - s) 4 u + 2 u) for 1 / (1 + expf(-z)) (the host's expf is well inside the device's 2 ulps); the fold B k u sum |terms|.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <random>

inline thread_local dim3 gridDim;
template <class T> T __shfl_down(T v, int, int) { return v; }
template <class T> T __shfl(T v, int, int) { return v; }

#include "colorcal.hip"

using std::vector;

static std::mt19937 rng(23);
static int failures = 0;
static const double U = std::ldexp(1.0, -24);
static const int I = 4, FIXED = 0;
static const int PATTERN[] = {1, 0, 2, 1, -1, 2, 0, I, 1, 2, 1};

static void fail(const char* label, const char* what, long at, double got, double want, double bar) {
  if (failures < 20) fprintf(stderr, "%s: %s[%ld] = %.9g, expected %.9g (bar %.3g)\n", label, what, at, got, want, bar);
  failures++;
}

struct Container {
  const char* label;
  vector<int> start_end;     // [R, 2]; empty in the equal-count form
  int R, equal, fixed;
  int64_t M;
};

static Container packed(const char* label, const vector<int>& starts, const vector<int>& counts, int64_t M) {
  Container c{label, {}, (int)counts.size(), 0, 0, M};
  for (size_t r = 0; r < counts.size(); r++) {
    c.start_end.push_back(starts[r]);
    c.start_end.push_back(starts[r] + counts[r]);
  }
  return c;
}

static void range_of(const Container& c, int r, int& s, int& e) {
  if (c.equal) s = r * c.fixed, e = s + c.fixed;
  else s = c.start_end[2 * r], e = c.start_end[2 * r + 1];
}

static void run_forward(const Container& c, bool zero_tables) {
  std::uniform_real_distribution<double> uni(-6.0, 6.0);
  std::normal_distribution<double> normal(0.0, 0.3);
  const int64_t M = c.M;
  vector<float> raw(3 * M), wd(3 * I), bias(3 * I), rgb(3 * M, 7.f);
  vector<int> img(c.R);
  for (auto& v : raw) v = (float)uni(rng);
  for (auto& v : wd) v = zero_tables ? 0.f : (float)normal(rng);
  for (auto& v : bias) v = zero_tables ? 0.f : (float)normal(rng);
  for (int r = 0; r < c.R; r++) img[r] = PATTERN[r % 11];
  gridDim = dim3((unsigned)plan::ray_grid(c.R));
  hip_on_host::concurrent = false;
  const int status = psdf_colorcal_sigmoid_forward(c.R, c.equal ? nullptr : c.start_end.data(), c.equal, c.fixed, (int)M, M, raw.data(), img.data(),
                                                   I, FIXED, wd.data(), bias.data(), rgb.data(), nullptr);
  if (status != 0) fail(c.label, "forward status", 0, status, 0, 0);
  vector<char> owned(M, 0);
  double worst = 0;
  for (int r = 0; r < c.R; r++) {
    int s, e;
    range_of(c, r, s, e);
    const bool learned = img[r] >= 0 && img[r] < I && img[r] != FIXED;
    for (int m = s; m < e; m++) {
      owned[m] = 1;
      for (int k = 0; k < 3; k++) {
        const float x = raw[k * M + m], got = rgb[3 * m + k];
        if (!learned || zero_tables) {      // the identity: the bits of sigmoid_rows_kernel's expression
          const float want = 1.0f / (1.0f + expf(-x));
          if (memcmp(&got, &want, 4) != 0) fail(c.label, "identity bits", 3 * m + k, got, want, 0);
          continue;
        }
        const double w = 1.0 + (double)wd[3 * img[r] + k], b = bias[3 * img[r] + k], z = x * w + b;
        const double sg = 1.0 / (1.0 + std::exp(-z)), Ez = (2 * std::fabs(x * w) + std::fabs(z)) * U;
        const double bar = sg * ((1.0 - sg) * (std::expm1(Ez) + 4 * U) + 2 * U) + 1e-37;
        if (!(std::fabs(got - sg) <= bar)) fail(c.label, "rgb", 3 * m + k, got, sg, bar);
        worst = std::max(worst, std::fabs(got - sg) / bar);
      }
    }
  }
  for (int64_t m = 0; m < M; m++)
    if (!owned[m] && (rgb[3 * m] != 7.f || rgb[3 * m + 1] != 7.f || rgb[3 * m + 2] != 7.f)) fail(c.label, "a slot no ray owns was written", m, rgb[3 * m], 7, 0);
  printf("forward %-8s %s %3d rays %4ld samples: worst error / bar %.2e\n", c.label, zero_tables ? "zero tables," : "            ", c.R, (long)M, worst);
}

static void run_fold(int R, bool two) {
  std::normal_distribution<double> normal(0.0, 1.0);
  vector<float> a(6 * R), b(two ? 6 * R : 0), g_wd(3 * I, 7.f), g_b(3 * I, 7.f);
  vector<int> img(R);
  for (auto& v : a) v = (float)normal(rng);
  for (auto& v : b) v = (float)normal(rng);
  for (int r = 0; r < R; r++) img[r] = PATTERN[r % 11];
  hip_on_host::concurrent = false;
  const int status = psdf_colorcal_fold(R, img.data(), I, FIXED, a.data(), two ? b.data() : nullptr, g_wd.data(), g_b.data(), nullptr);
  if (status != 0) fail("fold", "status", R, status, 0, 0);
  double worst = 0;
  for (int i = 0; i < I; i++)
    for (int col = 0; col < 6; col++) {
      double sum = 0, mag = 0;
      int k = 0;
      for (int r = 0; r < R; r++) {
        if (img[r] != i || i == FIXED) continue;
        k++;
        sum += (double)a[6 * r + col] + (two ? (double)b[6 * r + col] : 0.0);
        mag += std::fabs(a[6 * r + col]) + (two ? std::fabs(b[6 * r + col]) : 0.0);
      }
      const float got = col < 3 ? g_wd[3 * i + col] : g_b[3 * i + col - 3];
      const double bar = (two ? 2 : 1) * k * U * mag * 1.001;
      if (k == 0 ? got != 0.0f : !(std::fabs(got - sum) <= bar)) fail("fold", "gradient", 6 * i + col, got, sum, bar);
      if (k) worst = std::max(worst, std::fabs(got - sum) / bar);
    }
  printf("fold    %4d rays, %d branch(es): worst error / bar %.2e\n", R, two ? 2 : 1, worst);
}

int main() {
  const Container cases[] = {
      packed("rows", {0, 0, 1, 16, 32, 49, 80, 112, 145, 209, 212}, {0, 1, 15, 16, 17, 31, 32, 33, 64, 3, 0}, 212),
      packed("one", {0}, {1}, 1),
      Container{"equal32", {}, 5, 1, 32, 160},
      packed("gap", {0, 9, 40}, {5, 20, 7}, 50),
  };
  for (const Container& c : cases) {
    run_forward(c, false);
    run_forward(c, true);
  }
  for (int R : {1, 3, 5, 11, 512}) {
    run_fold(R, false);
    run_fold(R, true);
  }
  // empty batches and refusals, before any launch; the backward is never launched here
  {
    float buf[16] = {0};
    int se[2] = {0, 1}, img[1] = {1};
    bool ok = psdf_colorcal_sigmoid_forward(0, nullptr, 0, 0, 0, 5, nullptr, nullptr, 0, 9, nullptr, nullptr, nullptr, nullptr) == 0;
    ok = ok && psdf_colorcal_sigmoid_forward(3, nullptr, 0, 0, 0, 0, nullptr, nullptr, 0, 9, nullptr, nullptr, nullptr, nullptr) == 0;
    ok = ok && psdf_colorcal_sigmoid_backward(0, nullptr, 0, 0, 0, 5, nullptr, nullptr, nullptr, nullptr, 0, 9, nullptr, nullptr, nullptr, nullptr, nullptr) == 0;
    ok = ok && psdf_colorcal_sigmoid_backward(-2, nullptr, 0, 0, 0, -5, nullptr, nullptr, nullptr, nullptr, 0, 9, nullptr, nullptr, nullptr, nullptr, nullptr) == 0;
    ok = ok && psdf_colorcal_fold(0, nullptr, 0, 9, nullptr, nullptr, nullptr, nullptr, nullptr) == 0;
    auto fwd = [&](int64_t M, const float* raw, const int* im, int images, int fixed, const float* w, const float* b, float* out, const int* ranges) {
      return psdf_colorcal_sigmoid_forward(1, ranges, 0, 0, 1, M, raw, im, images, fixed, w, b, out, nullptr);
    };
    ok = ok && fwd(1, nullptr, img, I, 0, buf, buf, buf, se) == -1 && fwd(1, buf, nullptr, I, 0, buf, buf, buf, se) == -1;
    ok = ok && fwd(1, buf, img, I, 0, nullptr, buf, buf, se) == -1 && fwd(1, buf, img, I, 0, buf, nullptr, buf, se) == -1;
    ok = ok && fwd(1, buf, img, I, 0, buf, buf, nullptr, se) == -1 && fwd(1, buf, img, I, 0, buf, buf, buf, nullptr) == -1;
    ok = ok && fwd(-1, buf, img, I, 0, buf, buf, buf, se) == -1 && fwd(1, buf, img, 0, 0, buf, buf, buf, se) == -1;
    ok = ok && fwd(1, buf, img, I, -1, buf, buf, buf, se) == -1 && fwd(1, buf, img, I, I, buf, buf, buf, se) == -1;
    ok = ok && fwd(plan::MAX_SAMPLES + 1, buf, img, I, 0, buf, buf, buf, se) == -2 && fwd(1, buf, img, plan::MAX_IMAGES + 1, 0, buf, buf, buf, se) == -2;
    ok = ok && psdf_colorcal_sigmoid_forward(plan::MAX_RAYS + 1, se, 0, 0, 1, 1, buf, img, I, 0, buf, buf, buf, nullptr) == -2;
    auto bwd = [&](int64_t M, const float* g, const float* y, const float* raw, const int* im, int images, int fixed, float* g_raw, float* g_ray,
                   const int* ranges) {
      return psdf_colorcal_sigmoid_backward(1, ranges, 0, 0, 1, M, g, y, raw, im, images, fixed, buf, buf, g_raw, g_ray, nullptr);
    };
    ok = ok && bwd(1, nullptr, buf, buf, img, I, 0, buf, buf, se) == -1 && bwd(1, buf, nullptr, buf, img, I, 0, buf, buf, se) == -1;
    ok = ok && bwd(1, buf, buf, nullptr, img, I, 0, buf, buf, se) == -1 && bwd(1, buf, buf, buf, nullptr, I, 0, buf, buf, se) == -1;
    ok = ok && bwd(1, buf, buf, buf, img, I, 0, nullptr, buf, se) == -1 && bwd(1, buf, buf, buf, img, I, 0, buf, nullptr, se) == -1;
    ok = ok && bwd(1, buf, buf, buf, img, I, 0, buf, buf, nullptr) == -1 && bwd(0, nullptr, nullptr, nullptr, nullptr, I, 0, nullptr, nullptr, se) == -1;
    ok = ok && bwd(-1, buf, buf, buf, img, I, 0, buf, buf, se) == -1 && bwd(1, buf, buf, buf, img, 0, 0, buf, buf, se) == -1;
    ok = ok && bwd(1, buf, buf, buf, img, I, I, buf, buf, se) == -1 && bwd(plan::MAX_SAMPLES + 1, buf, buf, buf, img, I, 0, buf, buf, se) == -2;
    ok = ok && psdf_colorcal_fold(1, nullptr, I, 0, buf, buf, buf, buf, nullptr) == -1 && psdf_colorcal_fold(1, img, I, 0, nullptr, buf, buf, buf, nullptr) == -1;
    ok = ok && psdf_colorcal_fold(1, img, I, 0, buf, nullptr, nullptr, buf, nullptr) == -1 && psdf_colorcal_fold(1, img, I, 0, buf, nullptr, buf, nullptr, nullptr) == -1;
    ok = ok && psdf_colorcal_fold(1, img, 0, 0, buf, buf, buf, buf, nullptr) == -1 && psdf_colorcal_fold(1, img, I, I, buf, buf, buf, buf, nullptr) == -1;
    ok = ok && psdf_colorcal_fold(1, img, plan::MAX_IMAGES + 1, 0, buf, buf, buf, buf, nullptr) == -2;
    if (!ok) {
      failures++;
      fprintf(stderr, "empty batch / refusals\n");
    }
  }
  if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
  else printf("colorcal_kernels_check: all checks passed\n");
  return failures ? 1 : 0;
}
