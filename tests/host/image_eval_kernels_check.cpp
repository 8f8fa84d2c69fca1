// Stand-alone check of the kernels of permuto_sdf_amd/csrc/image_eval.hip on the CPU: the file itself is compiled as C++ against
// tests/host/hip_on_host/hip/hip_runtime.h (launches run on CPU threads), driven the way permuto_sdf_amd/image_eval.py drives it
// (plan, workspace, the two entries) and compared with brute-force float64: the f x f pooling written as a mean, the window as
// the full two-dimensional sum of w[i] w[j] products, the scores as plain sums.  tests/test_image_eval_host.py builds it with
// -fsanitize=address,undefined -fno-sanitize-recover=all and runs it: every buffer has exactly the extent the plan states, so an
// index out of bounds in a kernel is a sanitizer report here, not a fault on a device.  It says nothing about speed, and nothing
// about what the device compiler makes of the source.
#include <cstdio>
#include <random>

#include "image_eval.hip"

using std::vector;

static std::mt19937 rng(11);
static int failures = 0;

static void must(int status, const char* what) {
  if (status != 0) {
    fprintf(stderr, "%s returned %d\n", what, status);
    exit(2);
  }
}

// a logical (N, C, H, W) tensor of fp32 or uint8 elements in NCHW or NHWC order, in a buffer of exactly its size
struct Tensor {
  int64_t N, C, H, W;
  bool u8, nhwc;
  vector<float> f;
  vector<uint8_t> b;
  int64_t strides[4];
  Tensor(int64_t N_, int64_t C_, int64_t H_, int64_t W_, bool u8_, bool nhwc_) : N(N_), C(C_), H(H_), W(W_), u8(u8_), nhwc(nhwc_) {
    (u8 ? b.resize(N * C * H * W) : f.resize(N * C * H * W));
    if (nhwc) strides[0] = H * W * C, strides[1] = 1, strides[2] = W * C, strides[3] = C;
    else strides[0] = C * H * W, strides[1] = H * W, strides[2] = W, strides[3] = 1;
  }
  int64_t at(int64_t n, int64_t c, int64_t h, int64_t w) const { return n * strides[0] + c * strides[1] + h * strides[2] + w * strides[3]; }
  // v in [0, 1]: stored as the nearest 8-bit level (times `scale` for fp32 tensors: data_range = scale)
  void set(int64_t n, int64_t c, int64_t h, int64_t w, double v, double scale) {
    const double level = std::nearbyint(v * 255.0);
    if (u8) b[at(n, c, h, w)] = (uint8_t)level;
    else f[at(n, c, h, w)] = (float)(level / 255.0 * scale);
  }
  double get(int64_t n, int64_t c, int64_t h, int64_t w) const {
    return u8 ? (double)b[at(n, c, h, w)] / 255.0 : (double)f[at(n, c, h, w)];
  }
  const void* data() const { return u8 ? (const void*)b.data() : (const void*)f.data(); }
};

// the pair of tests/image_eval_reference.py in spirit: smooth pattern, a block of zeros in both, a saturated block, noise
static void fill_pair(Tensor& x, Tensor& y, double scale_x, double scale_y) {
  std::normal_distribution<double> normal(0.0, 1.0);
  for (int64_t n = 0; n < x.N; n++)
    for (int64_t c = 0; c < x.C; c++)
      for (int64_t h = 0; h < x.H; h++)
        for (int64_t w = 0; w < x.W; w++) {
          double base = 0.5 + 0.4 * std::sin((double)w / (5.0 + c) + n) * std::cos((double)h / (7.0 + n));
          if (h < x.H / 3 && w < x.W / 2) base = 0.0;
          if (h >= x.H / 3 && h < x.H / 2 && w >= x.W / 2) base = 1.0;
          const bool inside = base > 0.0 && base < 1.0;
          const double g = std::min(1.0, std::max(0.0, base + (inside ? 0.02 * normal(rng) : 0.0)));
          const double p = std::min(1.0, std::max(0.0, g + (base > 0.0 ? 0.05 * normal(rng) : 0.0)));
          x.set(n, c, h, w, p, scale_x);
          y.set(n, c, h, w, g, scale_y);
        }
}

struct Case {
  const char* label;
  int N, C, H, W;
  bool x_u8, y_u8, x_nhwc, y_nhwc;
  int mask;   // 0: none, 1: uint8 0 / 255, 2: graded fp32
  double data_range;
  int K;
  double sigma;
  bool downsample;
};

static void run(const Case& k) {
  const bool scaled = k.data_range != 1.0;   // unnormalised floats: both images fp32
  Tensor x(k.N, k.C, k.H, k.W, k.x_u8, k.x_nhwc), y(k.N, k.C, k.H, k.W, k.y_u8, k.y_nhwc);
  fill_pair(x, y, scaled ? k.data_range : 1.0, scaled ? k.data_range : 1.0);
  Tensor m(k.N, 1, k.H, k.W, k.mask == 1, false);
  if (k.mask) {
    std::uniform_real_distribution<double> uni(-0.3, 1.3);
    for (int64_t n = 0; n < k.N; n++)
      for (int64_t h = 0; h < k.H; h++)
        for (int64_t w = 0; w < k.W; w++) {
          if (k.mask == 1) m.b[m.at(n, 0, h, w)] = (h <= k.H / 3 && w < k.W / 2 + 2) ? 0 : 255;
          else m.f[m.at(n, 0, h, w)] = (float)std::min(1.0, std::max(0.0, uni(rng)));
        }
  }
  auto value = [&](const Tensor& t, int64_t n, int64_t c, int64_t h, int64_t w) {
    const double mv = k.mask ? m.get(n, 0, h, w) : 1.0;
    return t.get(n, c, h, w) * mv / k.data_range;
  };
  const void* mp = k.mask ? m.data() : nullptr;
  const int64_t* ms = k.mask ? m.strides : nullptr;
  hip_on_host::concurrent = true;   // every kernel of the file synchronises

  // ---- squared difference
  const int64_t sq_per_image = psdf_image_sq_diff_partials(k.H, k.W);
  vector<double> sq_ws(k.N * sq_per_image, -1.0), sq(k.N, -1.0);
  must(psdf_image_sq_diff(x.data(), x.u8, x.strides, y.data(), y.u8, y.strides, mp, k.mask == 1, ms, k.N, k.C, k.H, k.W, k.data_range,
                          sq_ws.data(), sq.data(), nullptr), "sq_diff");
  double worst_sq = 0;
  for (int64_t n = 0; n < k.N; n++) {
    double want = 0;
    for (int64_t c = 0; c < k.C; c++)
      for (int64_t h = 0; h < k.H; h++)
        for (int64_t w = 0; w < k.W; w++) {
          const double d = value(x, n, c, h, w) - value(y, n, c, h, w);
          want += d * d;
        }
    // a sum of non-negative terms: relative error at most (terms) x 2^-53 on either side
    const double bar = 2.0 * (double)(k.C * k.H * k.W) * std::ldexp(1.0, -53) * want;
    const double err = std::fabs(sq[n] - want);
    if (!(err <= bar)) {
      failures++;
      fprintf(stderr, "%s: squared difference of image %d: %.17g, expected %.17g\n", k.label, (int)n, sq[n], want);
    }
    if (bar > 0) worst_sq = std::max(worst_sq, err / bar);
  }

  // ---- SSIM
  int64_t pl[PSDF_IMAGE_EVAL_PLAN_FIELDS];
  must(psdf_image_eval_plan(k.N, k.C, k.H, k.W, k.K, k.downsample, pl), "plan");
  const int f = (int)pl[0], ph = (int)pl[1], pw = (int)pl[2], mh = (int)pl[3], mw = (int)pl[4];
  vector<double> ws(pl[9] / 8, -1.0), score(k.N, -1.0), map((size_t)k.N * k.C * mh * mw, -7.0);
  must(psdf_image_ssim(x.data(), x.u8, x.strides, y.data(), y.u8, y.strides, mp, k.mask == 1, ms, k.N, k.C, k.H, k.W, k.data_range,
                       k.K, k.sigma, 0.01, 0.03, k.downsample, ws.data(), score.data(), map.data(), nullptr), "ssim");
  // the same call without the map gives the same bits
  vector<double> again(k.N, -1.0);
  must(psdf_image_ssim(x.data(), x.u8, x.strides, y.data(), y.u8, y.strides, mp, k.mask == 1, ms, k.N, k.C, k.H, k.W, k.data_range,
                       k.K, k.sigma, 0.01, 0.03, k.downsample, ws.data(), again.data(), nullptr, nullptr), "ssim (no map)");
  vector<double> g(k.K);
  {
    double sum = 0;
    for (int i = 0; i < k.K; i++) sum += g[i] = std::exp(-std::pow(i - (k.K - 1) / 2.0, 2) / (2 * k.sigma * k.sigma));
    for (auto& v : g) v /= sum;
  }
  const double c1 = 0.01 * 0.01, c2 = 0.03 * 0.03, bar = 1e-9;
  double worst = 0;
  vector<double> px((size_t)ph * pw), py((size_t)ph * pw);
  for (int64_t n = 0; n < k.N; n++) {
    double total = 0;
    for (int64_t c = 0; c < k.C; c++) {
      for (int r = 0; r < ph; r++)
        for (int q = 0; q < pw; q++) {
          double sx = 0, sy = 0;
          for (int dy = 0; dy < f; dy++)
            for (int dx = 0; dx < f; dx++) sx += value(x, n, c, r * f + dy, q * f + dx), sy += value(y, n, c, r * f + dy, q * f + dx);
          px[(size_t)r * pw + q] = sx / (f * f), py[(size_t)r * pw + q] = sy / (f * f);
        }
      for (int r = 0; r < mh; r++)
        for (int q = 0; q < mw; q++) {
          double mx = 0, my = 0, exx = 0, eyy = 0, exy = 0;
          for (int i = 0; i < k.K; i++)
            for (int j = 0; j < k.K; j++) {
              const double w = g[i] * g[j], a = px[(size_t)(r + i) * pw + q + j], b = py[(size_t)(r + i) * pw + q + j];
              mx += w * a, my += w * b, exx += w * a * a, eyy += w * b * b, exy += w * a * b;
            }
          const double v = (2 * mx * my + c1) / (mx * mx + my * my + c1) * (2 * (exy - mx * my) + c2) /
                           ((exx - mx * mx) + (eyy - my * my) + c2);
          total += v;
          const double got = map[(((size_t)n * k.C + c) * mh + r) * mw + q];
          const double err = std::fabs(got - v);
          if (!(err <= bar)) {
            if (failures < 20) fprintf(stderr, "%s: map[%d, %d, %d, %d] = %.17g, expected %.17g\n", k.label, (int)n, (int)c, r, q, got, v);
            failures++;
          }
          worst = std::max(worst, err / bar);
        }
    }
    const double want = total / ((double)k.C * mh * mw), err = std::fabs(score[n] - want);
    if (!(err <= bar) || again[n] != score[n]) {
      failures++;
      fprintf(stderr, "%s: score of image %d: %.17g (again %.17g), expected %.17g\n", k.label, (int)n, score[n], again[n], want);
    }
    worst = std::max(worst, err / bar);
  }
  printf("%-34s f %d map %3d x %3d: worst ssim error / bar %.2e, squared difference %.2e\n", k.label, f, mh, mw, worst, worst_sq);
}

int main() {
  namespace plan = psdf::image_eval_plan;
  const int th = plan::TILE_H, tw = plan::TILE_W;
  const Case cases[] = {
      //  label                      N  C  H            W            x_u8   y_u8   x_nhwc y_nhwc mask range  K   sigma down
      {"one map entry", 1, 1, 11, 11, false, false, false, false, 0, 1.0, 11, 1.5, true},
      {"12 x 11, mixed types", 3, 3, 12, 11, true, false, false, true, 1, 1.0, 11, 1.5, true},
      {"tile - 1", 1, 3, th - 1 + 10, tw - 1 + 10, true, true, true, true, 2, 1.0, 11, 1.5, true},
      {"tile", 3, 1, th + 10, tw + 10, false, true, false, false, 0, 1.0, 11, 1.5, true},
      {"tile + 1, data_range 255", 1, 1, th + 1 + 10, tw + 1 + 10, false, false, true, false, 1, 255.0, 11, 1.5, true},
      {"3 tiles + 1", 1, 3, 3 * th + 1 + 10, 3 * tw + 1 + 10, true, false, true, false, 2, 1.0, 11, 1.5, true},
      {"largest window", 1, 1, th + 17, tw + 15, false, false, false, false, 0, 1.0, plan::MAX_KERNEL, 2.0, true},
      {"3 taps", 2, 1, 9, 40, true, true, false, false, 1, 1.0, 3, 0.8, true},
      {"384 x 390: f = 2", 1, 1, 384, 390, true, true, false, false, 1, 1.0, 11, 1.5, true},
      {"pooling switched off", 1, 2, 13, 45, true, false, false, false, 0, 1.0, 3, 0.8, false},
  };
  for (const Case& k : cases) run(k);
  // empty batch and refusals, before any launch
  {
    const int64_t s[4] = {1, 1, 1, 1}, neg[4] = {1, -1, 1, 1};
    float buf[4] = {0, 0, 0, 0};
    double out[2] = {5, 5}, ws[8];
    bool ok = psdf_image_sq_diff(nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, 0, 3, 4, 4, 1.0, nullptr, nullptr, nullptr) == 0;
    ok = ok && psdf_image_ssim(nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, 0, 3, 4, 4, 1.0, 11, 1.5, 0.01, 0.03, 1, nullptr,
                               nullptr, nullptr, nullptr) == 0;
    ok = ok && psdf_image_sq_diff(nullptr, 0, s, buf, 0, s, nullptr, 0, nullptr, 1, 1, 2, 2, 1.0, ws, out, nullptr) == -1;
    ok = ok && psdf_image_sq_diff(buf, 0, neg, buf, 0, s, nullptr, 0, nullptr, 1, 1, 2, 2, 1.0, ws, out, nullptr) == -1;
    ok = ok && psdf_image_sq_diff(buf, 0, s, buf, 0, s, nullptr, 0, nullptr, 1, 1, 2, 2, 0.0, ws, out, nullptr) == -1;
    ok = ok && psdf_image_ssim(buf, 0, s, buf, 0, s, nullptr, 0, nullptr, 1, 1, 2, 2, 1.0, 11, 1.5, 0.01, 0.03, 1, ws, out, nullptr, nullptr) == -1;
    ok = ok && out[0] == 5 && out[1] == 5;
    if (!ok) {
      failures++;
      fprintf(stderr, "empty batch / refusals\n");
    }
  }
  if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
  else printf("image_eval_kernels_check: all checks passed\n");
  return failures ? 1 : 0;
}
