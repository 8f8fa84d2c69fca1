// Stand-alone check of permuto_sdf_amd/csrc/mesh_color.hip on the CPU: the file itself is compiled as C++ against
// tests/host/hip_on_host/hip/hip_runtime.h (launches run on the calling thread), driven the way permuto_sdf_amd/mesh_color.py
// drives it and compared, entry by entry, with a float64 restatement written here as plain loops.
// tests/test_mesh_color_host.py builds it with -fsanitize=address,undefined -fno-sanitize-recover=all and runs it: every buffer
// has exactly the extent include/psdf.h states, so an index out of bounds in a kernel is a sanitizer report here, not a fault
// on a device.  It says nothing about speed, and nothing about what the device compiler makes of the source.
//
// Bars (u = 2^-24).  Unit vectors G / max(|G|, 1e-12): three squares, two adds, a square root, a division -- 6 u relative, taken
// as 8 u of the entry plus 1e-37 (the squares of a 1e-20 gradient are subnormal: the division by the eps is what is checked).
// Camera directions: one more rounding for p - eye, 8 u absolute (|d| <= 1).  SH values, evaluated in float64 from the kernel's
// own fp32 direction: every channel is a polynomial of at most 16 roundings whose intermediate magnitudes stay below 8 for
// |d| <= 1 (the largest: 3.76 x2 y2 + 0.63 x4 + 0.63 y4, 3.17 z2 + 3.70 z4 + 0.32), hence 128 u absolute.  Colours: the host's
// expf is within 1 ulp, 1 + e and the division round once each: s ((1 - s) 4 u + 2 u) + 1e-37 (as tests/host/
// colorcal_kernels_check.cpp), and bit for bit 1.0f / (1.0f + expf(-raw)) evaluated here.  8-bit colours: exact, against the
// ties-to-even rule restated with floor.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <random>

inline thread_local dim3 gridDim;
template <class T> T __shfl_down(T v, int, int) { return v; }
template <class T> T __shfl(T v, int, int) { return v; }

#include "mesh_color.hip"

using std::vector;

static std::mt19937 rng(31);
static int failures = 0;
static const double U = std::ldexp(1.0, -24);
static const float CANARY = 7.0f;
static const int ENC = 51, G = 32, C = ENC + 25 + 3 + G;      // the real net: 111 rows

static void fail(const char* label, const char* what, long at, double got, double want, double bar) {
  if (failures < 20) fprintf(stderr, "%s: %s[%ld] = %.9g, expected %.9g (bar %.3g)\n", label, what, at, got, want, bar);
  failures++;
}

// the 25 values of degree 5 in float64 (PermutoSDFGPU.cuh:275-365)
static void sh25(double x, double y, double z, double* o) {
  const double xy = x * y, xz = x * z, yz = y * z, x2 = x * x, y2 = y * y, z2 = z * z, x4 = x2 * x2, y4 = y2 * y2, z4 = z2 * z2;
  o[0] = 0.28209479177387814;
  o[1] = -0.48860251190291987 * y;
  o[2] = 0.48860251190291987 * z;
  o[3] = -0.48860251190291987 * x;
  o[4] = 1.0925484305920792 * xy;
  o[5] = -1.0925484305920792 * yz;
  o[6] = 0.94617469575755997 * z2 - 0.31539156525251999;
  o[7] = -1.0925484305920792 * xz;
  o[8] = 0.54627421529603959 * x2 - 0.54627421529603959 * y2;
  o[9] = 0.59004358992664352 * y * (-3.0 * x2 + y2);
  o[10] = 2.8906114426405538 * xy * z;
  o[11] = 0.45704579946446572 * y * (1.0 - 5.0 * z2);
  o[12] = 0.3731763325901154 * z * (5.0 * z2 - 3.0);
  o[13] = 0.45704579946446572 * x * (1.0 - 5.0 * z2);
  o[14] = 1.4453057213202769 * z * (x2 - y2);
  o[15] = 0.59004358992664352 * x * (-x2 + 3.0 * y2);
  o[16] = 2.5033429417967046 * xy * (x2 - y2);
  o[17] = 1.7701307697799304 * yz * (-3.0 * x2 + y2);
  o[18] = 0.94617469575756008 * xy * (7.0 * z2 - 1.0);
  o[19] = 0.66904654355728921 * yz * (3.0 - 7.0 * z2);
  o[20] = -3.1735664074561294 * z2 + 3.7024941420321507 * z4 + 0.31735664074561293;
  o[21] = 0.66904654355728921 * xz * (3.0 - 7.0 * z2);
  o[22] = 0.47308734787878004 * (x2 - y2) * (7.0 * z2 - 1.0);
  o[23] = 1.7701307697799304 * xz * (-x2 + 3.0 * y2);
  o[24] = -3.7550144126950569 * x2 * y2 + 0.62583573544917614 * x4 + 0.62583573544917614 * y4;
}

static void unit64(const float* v, double* out) {
  const double x = v[0], y = v[1], z = v[2];
  const double den = std::max(std::sqrt(x * x + y * y + z * z), (double)1e-12f);
  out[0] = x / den, out[1] = y / den, out[2] = z / den;
}

// one call of psdf_mesh_color_inputs on n vertices; the special rows sit at the front, a zero gradient also in the last wave
static void run_inputs(const char* label, int64_t n, int mode, bool want_side_outputs) {
  std::normal_distribution<double> normal(0.0, 1.0);
  std::uniform_real_distribution<double> ball(-0.5, 0.5);
  vector<float> pts(3 * n), grad(3 * n), y((1 + G) * n), x((size_t)C * n, CANARY), dirs(want_side_outputs ? 3 * n : 0, CANARY),
      nrm(want_side_outputs ? 3 * n : 0, CANARY), eye = {0.3f, -0.7f, 1.1f};
  for (auto& v : pts) v = (float)ball(rng);
  for (auto& v : grad) v = (float)(normal(rng) * 1.3);
  for (auto& v : y) v = (float)normal(rng);
  auto set3 = [](vector<float>& t, int64_t i, float a, float b, float c) { t[3 * i] = a, t[3 * i + 1] = b, t[3 * i + 2] = c; };
  set3(grad, 0, 0.f, 0.f, 0.f);                                       // a zero gradient
  if (n > 1) set3(grad, 1, 1e-20f, -2e-20f, 0.5e-20f);                // below the eps
  if (n > 2) set3(pts, 2, eye[0], eye[1], eye[2]);                    // a vertex equal to the eye
  if (n > 3) set3(grad, 3, 0.f, 0.f, -3.f);                           // an axis
  if (n > 64) set3(grad, n - 1, 0.f, 0.f, 0.f);
  hip_on_host::concurrent = false;
  const int status = psdf_mesh_color_inputs(n, pts.data(), grad.data(), y.data(), G, mode, mode ? eye.data() : nullptr, x.data(), C, ENC,
                                            want_side_outputs ? dirs.data() : nullptr, want_side_outputs ? nrm.data() : nullptr, nullptr);
  if (status != 0) fail(label, "status", 0, status, 0, 0);
  double worst_unit = 0, worst_sh = 0;
  for (int64_t i = 0; i < n; i++) {
    double n64[3], d64[3], diff[3], sh64[25];
    unit64(&grad[3 * i], n64);
    float got_n[3], got_d[3];
    for (int k = 0; k < 3; k++) got_n[k] = x[(size_t)(ENC + 25 + k) * n + i];
    for (int k = 0; k < 3; k++) {
      const double bar = 8 * U * std::fabs(n64[k]) + 1e-37;
      if (!(std::fabs(got_n[k] - n64[k]) <= bar)) fail(label, "normal row", 3 * i + k, got_n[k], n64[k], bar);
      worst_unit = std::max(worst_unit, std::fabs(got_n[k] - n64[k]) / bar);
      if (want_side_outputs && memcmp(&nrm[3 * i + k], &got_n[k], 4) != 0) fail(label, "normals output", 3 * i + k, nrm[3 * i + k], got_n[k], 0);
    }
    // the view direction: from the side output where there is one, else the one the mode defines from the normal rows
    if (mode == plan::MODE_NORMAL) {
      for (int k = 0; k < 3; k++) {
        got_d[k] = -got_n[k];
        if (want_side_outputs && memcmp(&dirs[3 * i + k], &got_d[k], 4) != 0) fail(label, "dirs is not -normal", 3 * i + k, dirs[3 * i + k], got_d[k], 0);
      }
    } else {
      float df[3];
      for (int k = 0; k < 3; k++) df[k] = pts[3 * i + k] - eye[k], diff[k] = (double)pts[3 * i + k] - (double)eye[k];
      const double den = std::max(std::sqrt(diff[0] * diff[0] + diff[1] * diff[1] + diff[2] * diff[2]), (double)1e-12f);
      const Nrm same = normalize_eps(v3{df[0], df[1], df[2]});      // without the side output: the expression itself
      got_d[0] = same.y.x, got_d[1] = same.y.y, got_d[2] = same.y.z;
      for (int k = 0; k < 3; k++) {
        d64[k] = diff[k] / den;
        if (want_side_outputs) got_d[k] = dirs[3 * i + k];
        const double bar = 8 * U;
        if (!(std::fabs(got_d[k] - d64[k]) <= bar)) fail(label, "camera direction", 3 * i + k, got_d[k], d64[k], bar);
        worst_unit = std::max(worst_unit, std::fabs(got_d[k] - d64[k]) / bar);
      }
      if (i == 2 && (got_d[0] != 0.f || got_d[1] != 0.f || got_d[2] != 0.f)) fail(label, "vertex at the eye: d", i, got_d[0], 0, 0);
    }
    if ((i == 0 || (n > 64 && i == n - 1)) && (got_n[0] != 0.f || got_n[1] != 0.f || got_n[2] != 0.f)) fail(label, "zero gradient: normal", i, got_n[0], 0, 0);
    sh25(got_d[0], got_d[1], got_d[2], sh64);
    for (int k = 0; k < 25; k++) {
      const float got = x[(size_t)(ENC + k) * n + i];
      const double bar = 128 * U;
      if (!(std::fabs(got - sh64[k]) <= bar)) fail(label, "sh row", 25 * i + k, got, sh64[k], bar);
      worst_sh = std::max(worst_sh, std::fabs(got - sh64[k]) / bar);
    }
    for (int k = 0; k < G; k++) {
      const float got = x[(size_t)(ENC + 28 + k) * n + i], want = y[(size_t)(1 + k) * n + i];
      if (memcmp(&got, &want, 4) != 0) fail(label, "geometry row", G * i + k, got, want, 0);
    }
  }
  // the colour encoding's rows belong to the encode kernel: not touched
  for (size_t j = 0; j < (size_t)ENC * n; j++)
    if (x[j] != CANARY) {
      fail(label, "a row before the SH block was written", (long)j, x[j], CANARY, 0);
      break;
    }
  printf("inputs %-18s n %4ld mode %d: worst error / bar: unit vectors %.2e, sh %.2e\n", label, (long)n, mode, worst_unit, worst_sh);
}

static float sigmoid32(float x) { return 1.0f / (1.0f + expf(-x)); }

static int u8_of(float y) {      // clamp(rint(y * 255), 0, 255), ties to even, without rint
  const float v = (float)((double)y * 255.0);      // the fp32 product: the float64 product of two floats is exact, rounded once
  double r = std::floor((double)v);
  const double f = (double)v - r;
  if (f > 0.5 || (f == 0.5 && std::fmod(r, 2.0) == 1.0)) r += 1.0;
  return (int)std::min(std::max(r, 0.0), 255.0);
}

// a raw value whose colour times 255 is exactly k + 0.5 in fp32: walked float by float around logit((k + 0.5) / 255)
static bool tie_raw(int k, float* raw) {
  const double y = (k + 0.5) / 255.0;
  float r = (float)std::log(y / (1.0 - y));
  float lo = r, hi = r;
  for (int step = 0; step < 20000; step++) {
    for (float c : {lo, hi})
      if ((float)((double)sigmoid32(c) * 255.0) == (float)k + 0.5f) {
        *raw = c;
        return true;
      }
    lo = std::nextafterf(lo, -INFINITY), hi = std::nextafterf(hi, INFINITY);
  }
  return false;
}

static void run_finish(const char* label, int64_t n, bool want_rgb, bool want_u8) {
  std::uniform_real_distribution<double> uni(-8.0, 8.0);
  vector<float> raw(3 * n), rgb(want_rgb ? 3 * n : 0, CANARY);
  vector<uint8_t> u8(want_u8 ? 3 * n : 0, 77);
  for (auto& v : raw) v = (float)uni(rng);
  vector<std::pair<int64_t, int>> ties;      // (entry of raw, the 8-bit value ties-to-even gives)
  if (n >= 130) {
    const float special[] = {100.f, -100.f, 88.8f, -88.8f, 0.f, -0.f, 88.72f, -88.72f, 16.7f, -103.9f, 1e-30f, INFINITY, -INFINITY};
    int64_t at = 0;
    for (float s : special) raw[(at % 3) * n + at / 3] = s, at++;
    // (for a small k no fp32 colour need exist whose product with 255 rounds to k + 0.5: a colour's steps times 255 are wider
    // than the interval that rounds there; such a k is passed over, an even and an odd one must be found)
    int found[2] = {0, 0};
    for (int k : {0, 1, 2, 3, 100, 101, 126, 127, 128, 253, 254}) {
      float r;
      if (!tie_raw(k, &r)) continue;
      const int64_t e = (at % 3) * n + at / 3;
      raw[e] = r, at++;
      ties.push_back({e, k % 2 ? k + 1 : k});
      found[k % 2]++;
    }
    if (!found[0] || !found[1]) fail(label, "no raw value lands on a tie: even, odd k found", 0, found[0], found[1], 0);
  }
  hip_on_host::concurrent = false;
  const int status = psdf_mesh_color_finish(n, raw.data(), want_rgb ? rgb.data() : nullptr, want_u8 ? u8.data() : nullptr, nullptr);
  if (status != 0) fail(label, "status", 0, status, 0, 0);
  double worst = 0;
  for (int64_t i = 0; i < n; i++)
    for (int c = 0; c < 3; c++) {
      const float x = raw[c * n + i], same = sigmoid32(x);
      if (want_rgb) {
        const float got = rgb[3 * i + c];
        if (memcmp(&got, &same, 4) != 0) fail(label, "rgb bits", 3 * i + c, got, same, 0);
        const double sg = 1.0 / (1.0 + std::exp(-(double)x)), bar = sg * ((1.0 - sg) * 4 * U + 2 * U) + 1e-37;
        if (!(std::fabs(got - sg) <= bar)) fail(label, "rgb", 3 * i + c, got, sg, bar);
        worst = std::max(worst, std::fabs(got - sg) / bar);
      }
      if (want_u8 && u8[3 * i + c] != u8_of(same)) fail(label, "rgb_u8", 3 * i + c, u8[3 * i + c], u8_of(same), 0);
    }
  if (want_u8)
    for (auto& t : ties) {
      const int64_t c = t.first / n, i = t.first % n;
      if (u8[3 * i + c] != t.second) fail(label, "tie to even", t.first, u8[3 * i + c], t.second, 0);
    }
  if (n >= 130 && want_rgb && want_u8) {
    // +-100 and +-88.8: expf overflows to infinity on one side and is subnormal on the other -- exactly 1 and exactly 0
    const float ends[] = {rgb[0], rgb[1], rgb[2], rgb[3]};
    if (ends[0] != 1.f || ends[1] != 0.f || ends[2] != 1.f || ends[3] != 0.f) fail(label, "the ends of the sigmoid", 0, ends[0], 1, 0);
    if (u8[0] != 255 || u8[1] != 0 || u8[2] != 255 || u8[3] != 0) fail(label, "the ends in 8 bits", 0, u8[0], 255, 0);
  }
  printf("finish %-18s n %4ld%s%s: %zu ties, worst error / bar %.2e\n", label, (long)n, want_rgb ? " rgb" : "", want_u8 ? " u8" : "", ties.size(), worst);
}

int main() {
  for (int mode : {plan::MODE_NORMAL, plan::MODE_CAMERA}) {
    run_inputs("two waves and a bit", 130, mode, true);
    run_inputs("no side outputs", 130, mode, false);
    run_inputs("one vertex", 1, mode, true);
    run_inputs("a workgroup + 1", 257, mode, true);
  }
  run_finish("two waves and a bit", 130, true, true);
  run_finish("rgb alone", 130, true, false);
  run_finish("u8 alone", 130, false, true);
  run_finish("one vertex", 1, true, true);
  run_finish("a workgroup + 1", 257, true, true);
  // n = 0 returns before any pointer or argument is looked at (no launch); refusals, before any launch
  {
    float buf[512] = {0};
    uint8_t bytes[8] = {0};
    int64_t out[plan::FIELDS] = {0};
    bool ok = psdf_mesh_color_inputs(0, nullptr, nullptr, nullptr, -4, 99, nullptr, nullptr, -1, -1, nullptr, nullptr, nullptr) == 0;
    ok = ok && psdf_mesh_color_finish(0, nullptr, nullptr, nullptr, nullptr) == 0;
    auto in = [&](int64_t n, const float* p, const float* gr, const float* y, int g, int mode, const float* eye, float* x, int c, int sh) {
      return psdf_mesh_color_inputs(n, p, gr, y, g, mode, eye, x, c, sh, nullptr, nullptr, nullptr);
    };
    ok = ok && in(-1, buf, buf, buf, 2, 0, buf, buf, 31, 1) == -1 && in(1, buf, buf, buf, -1, 0, buf, buf, 28, 1) == -1;
    ok = ok && in(1, buf, buf, buf, 2, 2, buf, buf, 31, 1) == -1 && in(1, buf, buf, buf, 2, -1, buf, buf, 31, 1) == -1;
    ok = ok && in(1, buf, buf, buf, 2, 0, buf, buf, 31, -1) == -1;
    ok = ok && in(1, buf, buf, buf, 2, 0, buf, buf, 30, 1) == -1 && in(1, buf, buf, buf, 2, 0, buf, buf, 32, 1) == -1;   // rows past C, rows short of C
    ok = ok && in(1, buf, nullptr, buf, 2, 0, buf, buf, 31, 1) == -1 && in(1, buf, buf, nullptr, 2, 0, buf, buf, 31, 1) == -1;
    ok = ok && in(1, buf, buf, buf, 2, 0, buf, nullptr, 31, 1) == -1;
    ok = ok && in(1, nullptr, buf, buf, 2, 1, buf, buf, 31, 1) == -1 && in(1, buf, buf, buf, 2, 1, nullptr, buf, 31, 1) == -1;
    ok = ok && in(1, nullptr, buf, nullptr, 0, 0, nullptr, buf, 29, 1) == 0;        // mode 0 reads neither points nor eye, g = 0 no y_fm
    ok = ok && in(plan::MAX_LAUNCH + 1, buf, buf, buf, 2, 0, buf, buf, 31, 1) == -2;
    ok = ok && in(1, buf, buf, buf, 2, 0, buf, buf, plan::MAX_ROWS + 1, plan::MAX_ROWS + 1 - 30) == -2;
    ok = ok && psdf_mesh_color_finish(-1, buf, buf, bytes, nullptr) == -1 && psdf_mesh_color_finish(1, nullptr, buf, bytes, nullptr) == -1;
    ok = ok && psdf_mesh_color_finish(plan::MAX_LAUNCH + 1, buf, buf, bytes, nullptr) == -2;
    ok = ok && psdf_mesh_color_finish(1, buf, nullptr, nullptr, nullptr) == 0;
    ok = ok && psdf_mesh_color_plan(51, 32, 111, 600, 256, out) == 0 && out[0] == 51 && out[1] == 76 && out[2] == 79 && out[3] == 111 &&
         out[4] == 111 && out[5] == 3 && out[6] == 88;
    ok = ok && psdf_mesh_color_plan(51, 32, 111, 600, 256, nullptr) == -1 && psdf_mesh_color_plan(51, 32, 112, 600, 256, out) == -1;
    ok = ok && psdf_mesh_color_plan(51, 32, 111, 600, 0, out) == -1 && psdf_mesh_color_plan(51, 32, 111, 600, plan::MAX_LAUNCH + 1, out) == -2;
    if (!ok) {
      failures++;
      fprintf(stderr, "empty batch / refusals\n");
    }
  }
  if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
  else printf("mesh_color_kernels_check: all checks passed\n");
  return failures ? 1 : 0;
}
