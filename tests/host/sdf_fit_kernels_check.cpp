// Stand-alone check of the kernels of permuto_sdf_amd/csrc/sdf_fit.hip on the CPU: the file itself is compiled as C++ against
// tests/host/hip_on_host/hip/hip_runtime.h (launches run on CPU threads), driven the way permuto_sdf_amd/sdf_fit.py drives it
// (plan, workspace, the two entries) and compared with brute-force float64 written as plain loops.  tests/test_sdf_fit_host.py
// builds it with -fsanitize=address,undefined -fno-sanitize-recover=all and runs it: every buffer has exactly the extent the
// header states, so an index out of bounds in a kernel is a sanitizer report here, not a fault on a device.  It says nothing
// about speed, and nothing about what the device compiler makes of the source.
//
// Bars.  u = 2^-24.  A term is a mean of fp32 row values, each within 16 u (1 + its size) of its float64 value (fewer than 16
// roundings on any path, none amplified: the rows here keep | |g| - 1 | >= 0.05 or are exact zeros), added in double: 32 u
// (1 + |term|).  An entry of grad_gradients is C_0 w sign g / |g| - C_1 (u / a - cos g / (a |g|)): two parts of size at most
// |C_0| and 2 |C_1| / a, each through fewer than 16 roundings, the cosine's 11 u entering the second with the factor 1 / a:
// 64 u (|C_0| + 2 |C_1| / a).  An entry of grad_sdf is a product of at most four factors and an expf within 2 ulps of an
// argument within u: (8 + sharpness |s|) u |value|.  The per-entry analysis proper is tests/sdf_fit_float64.py.
#include <cstdio>
#include <random>

#include "sdf_fit.hip"

using std::vector;

static std::mt19937 rng(7);
static int failures = 0;
static const double U = std::ldexp(1.0, -24);

static void fail(const char* label, const char* what, long at, double got, double want, double bar) {
  if (failures < 20) fprintf(stderr, "%s: %s[%ld] = %.9g, expected %.9g (bar %.3g)\n", label, what, at, got, want, bar);
  failures++;
}

static double sign0(double x) { return (double)((x > 0) - (x < 0)); }

struct Case {
  const char* label;
  int P;
  int64_t n_surf, n_off;
  float eik_clamp;
  bool with_loss, with_grad;
};

static void run(const Case& k) {
  const int P = k.P;
  const int64_t N = k.n_surf + k.n_off, M = 37;
  std::uniform_real_distribution<double> uni(0.0, 1.0);
  std::normal_distribution<double> normal(0.0, 1.0);
  hip_on_host::concurrent = true;   // the loss kernels synchronise

  // ---- the batch: a cloud of M rows, indices that include -1, M and far outside, a box
  vector<float> cloud_p(M * P), cloud_n(M * 3), uniforms(k.n_off * P), points(N * P, 7.0f), normals(k.n_surf * 3, 7.0f);
  vector<int64_t> indices(k.n_surf);
  for (auto& v : cloud_p) v = (float)(uni(rng) - 0.5);
  for (auto& v : cloud_n) v = (float)normal(rng);
  for (auto& v : uniforms) v = (float)uni(rng);
  for (int64_t r = 0; r < k.n_surf; r++) indices[r] = (int64_t)(uni(rng) * M);
  if (k.n_surf > 0) indices[0] = -1;
  if (k.n_surf > 1) indices[1] = M;
  if (k.n_surf > 2) indices[2] = INT64_MAX;
  if (k.n_surf > 3) indices[3] = INT64_MIN;
  const float lo[4] = {-0.5f, -0.25f, 0.125f, 0.0f}, hi[4] = {0.5f, 0.75f, 0.375f, 1.0f};
  int status = psdf_sdf_fit_batch(P, M, k.n_surf, k.n_off, cloud_p.data(), cloud_n.data(), indices.data(), uniforms.data(), lo, hi,
                                  points.data(), normals.data(), nullptr);
  if (status != 0) fail(k.label, "batch status", 0, status, 0, 0);
  for (int64_t r = 0; r < N && status == 0; r++)
    for (int c = 0; c < P; c++) {
      float want;
      if (r < k.n_surf) {
        const int64_t i = std::min<int64_t>(std::max<int64_t>(indices[r], 0), M - 1);
        want = cloud_p[i * P + c];
        if (c < 3 && normals[r * 3 + c] != cloud_n[i * 3 + c]) fail(k.label, "normals", r * 3 + c, normals[r * 3 + c], cloud_n[i * 3 + c], 0);
      } else {
        want = lo[c] + uniforms[(r - k.n_surf) * P + c] * (hi[c] - lo[c]);
      }
      if (points[r * P + c] != want) fail(k.label, "points", r * P + c, points[r * P + c], want, 0);
    }

  // ---- the loss: |g| in [0.7, 0.95] or [1.05, 1.3], with exact zeros of g and of s among the rows
  vector<float> sdf(N), grad(N * P), nrm(k.n_surf * 3);
  for (int64_t r = 0; r < N; r++) {
    double d[3], len = 0;
    for (double& v : d) v = normal(rng), len += v * v;
    const double want_len = (uni(rng) < 0.5 ? 0.7 : 1.05) + 0.25 * uni(rng);
    for (int c = 0; c < 3; c++) grad[r * P + c] = r % 11 == 5 ? 0.0f : (float)(d[c] / std::sqrt(len) * want_len);
    if (P == 4) grad[r * P + 3] = (float)normal(rng);
    sdf[r] = r % 13 == 7 ? 0.0f : (float)((uni(rng) - 0.5) * (r < k.n_surf ? 0.02 : 1.0));
    if (r < k.n_surf)
      for (int c = 0; c < 3; c++) nrm[r * 3 + c] = (float)(d[c] / std::sqrt(len) + 0.3 * normal(rng));
  }
  const float weights[4] = {5e1f, 1e2f, 3e3f, 1e2f}, sharp = 1e2f, scale = 1.0f / 30000.0f;
  int64_t pl[PSDF_SDF_FIT_PLAN_FIELDS];
  if (psdf_sdf_fit_plan(k.n_surf, k.n_off, pl) != 0) fail(k.label, "plan", 0, -1, 0, 0);
  vector<double> ws(pl[1] / 8, -1.0);
  vector<float> terms(4, 7.0f), again(4, 7.0f), g_sdf(k.with_grad ? N : 0, 7.0f), g_grad(k.with_grad ? N * P : 0, 7.0f);
  float loss = 0.25f;
  status = psdf_sdf_fit_loss(P, k.n_surf, k.n_off, sdf.data(), grad.data(), nrm.data(), weights, sharp, k.eik_clamp, scale, ws.data(),
                             terms.data(), k.with_loss ? &loss : nullptr, k.with_grad ? g_sdf.data() : nullptr,
                             k.with_grad ? g_grad.data() : nullptr, nullptr);
  if (status != 0) fail(k.label, "loss status", 0, status, 0, 0);
  // the same call without loss and gradients gives the same bits
  status = psdf_sdf_fit_loss(P, k.n_surf, k.n_off, sdf.data(), grad.data(), nrm.data(), weights, sharp, k.eik_clamp, scale, ws.data(),
                             again.data(), nullptr, nullptr, nullptr, nullptr);
  if (status != 0 || memcmp(terms.data(), again.data(), 16) != 0) fail(k.label, "terms of a second call", 0, again[0], terms[0], 0);

  const double count[4] = {(double)N, (double)k.n_surf, (double)k.n_surf, (double)k.n_off};
  double C[4], sum[4] = {0, 0, 0, 0}, worst = 0;
  for (int t = 0; t < 4; t++) C[t] = count[t] > 0 ? (double)scale * weights[t] / count[t] : 0.0;
  for (int64_t r = 0; r < N; r++) {
    const double s = sdf[r], g[3] = {grad[r * P], grad[r * P + 1], grad[r * P + 2]};
    const double len = std::sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]), e = len - 1.0;
    const double w = k.eik_clamp > 0 ? std::exp(-(s * s) / (2.0 * (double)k.eik_clamp * k.eik_clamp)) : 1.0;
    sum[0] += w * std::fabs(e);
    double dg[3], ds, a = std::max(len, 1e-8);
    for (int c = 0; c < 3; c++) dg[c] = len > 0 ? C[0] * w * sign0(e) * g[c] / len : 0.0;
    if (r < k.n_surf) {
      const double n[3] = {nrm[r * 3], nrm[r * 3 + 1], nrm[r * 3 + 2]};
      const double b = std::max(std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]), 1e-8);
      const double cs = (g[0] * n[0] + g[1] * n[1] + g[2] * n[2]) / (a * b);
      sum[1] += 1.0 - cs;
      sum[2] += std::fabs(s);
      for (int c = 0; c < 3; c++) dg[c] -= C[1] * (n[c] / (a * b) - (len > 0 ? cs * g[c] / (a * len) : 0.0));
      ds = C[2] * sign0(s);
    } else {
      const double ex = std::exp(-(double)sharp * std::fabs(s));
      sum[3] += ex;
      ds = -C[3] * sharp * sign0(s) * ex;
    }
    if (!k.with_grad) continue;
    const double bar_s = (8.0 + sharp * std::fabs(s)) * U * std::fabs(ds), err_s = std::fabs(g_sdf[r] - ds);
    if (!(err_s <= bar_s)) fail(k.label, "grad_sdf", r, g_sdf[r], ds, bar_s);
    if (bar_s > 0) worst = std::max(worst, err_s / bar_s);
    const double bar_g = 64.0 * U * (std::fabs(C[0]) + (r < k.n_surf ? 2.0 * std::fabs(C[1]) / a : 0.0));
    for (int c = 0; c < 3; c++) {
      const double err = std::fabs(g_grad[r * P + c] - dg[c]);
      if (!(err <= bar_g)) fail(k.label, "grad_gradients", r * P + c, g_grad[r * P + c], dg[c], bar_g);
      worst = std::max(worst, err / bar_g);
    }
    if (P == 4 && g_grad[r * P + 3] != 0.0f) fail(k.label, "grad_gradients (time)", r * P + 3, g_grad[r * P + 3], 0, 0);
  }
  double total = 0;
  for (int t = 0; t < 4; t++) {
    const double want = count[t] > 0 ? sum[t] / count[t] : 0.0, bar = 32.0 * U * (1.0 + std::fabs(want)), err = std::fabs(terms[t] - want);
    if (!(err <= bar)) fail(k.label, "terms", t, terms[t], want, bar);
    worst = std::max(worst, err / bar);
    total += (double)scale * weights[t] * want;
  }
  if (k.with_loss) {
    const double want = 0.25 + total, bar = 64.0 * U * (1.0 + std::fabs(want));
    if (!(std::fabs(loss - want) <= bar)) fail(k.label, "loss", 0, loss, want, bar);
  }
  printf("%-28s P %d rows %6ld + %6ld, %3ld workgroups: worst error / bar %.2e\n", k.label, P, (long)k.n_surf, (long)k.n_off,
         (long)pl[0], worst);
}

int main() {
  namespace plan = psdf::sdf_fit_plan;
  const int64_t pass = plan::ROWS_PER_PASS;
  const Case cases[] = {
      {"off-surface rows only", 3, 0, 5, 0.0f, true, true},
      {"surface rows only", 4, 5, 0, 0.05f, true, true},
      {"one of each", 3, 1, 1, 0.05f, false, true},
      {"no gradients", 4, 63, 65, 0.0f, true, false},
      {"63 + 65", 3, 63, 65, 0.0f, true, true},
      {"257 + 1000", 4, 257, 1000, 0.05f, true, true},
      {"257 + 1000, 3-D", 3, 257, 1000, 0.05f, true, true},
      {"one row past a full pass", 4, 300, pass + 1 - 300, 0.0f, true, true},
  };
  for (const Case& k : cases) run(k);
  // the plan, empty batches and refusals, before any launch
  {
    int64_t pl[PSDF_SDF_FIT_PLAN_FIELDS];
    bool ok = psdf_sdf_fit_plan(3000, 30000, pl) == 0 && pl[0] == 129 && pl[1] == 129 * 4 * 8 && pl[2] == pass && pl[3] == 129;
    ok = ok && psdf_sdf_fit_plan(0, 0, pl) == 0 && pl[0] == 0 && pl[1] == 0 && pl[3] == 0;
    ok = ok && psdf_sdf_fit_plan(1, pass, pl) == 0 && pl[0] == plan::MAX_GRID && pl[3] == plan::MAX_GRID + 1;
    ok = ok && psdf_sdf_fit_plan(-1, 0, pl) == -1 && psdf_sdf_fit_plan(0, 0, nullptr) == -1;
    ok = ok && psdf_sdf_fit_plan((int64_t)1 << 31, 0, pl) == -2 && psdf_sdf_fit_plan((int64_t)1 << 30, (int64_t)1 << 30, pl) == -2;
    float buf[16] = {0}, w[4] = {1, 1, 1, 1}, nan = std::nanf("");
    double ws[8];
    int64_t idx[2] = {0, 0};
    ok = ok && psdf_sdf_fit_batch(3, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0;
    ok = ok && psdf_sdf_fit_loss(9, 0, 0, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0;
    ok = ok && psdf_sdf_fit_batch(5, 2, 1, 1, buf, buf, idx, buf, buf, buf, buf, buf, nullptr) == -1;
    ok = ok && psdf_sdf_fit_batch(3, 0, 1, 1, buf, buf, idx, buf, buf, buf, buf, buf, nullptr) == -1;      // an empty cloud
    ok = ok && psdf_sdf_fit_batch(3, 2, 1, 1, buf, nullptr, idx, buf, buf, buf, buf, buf, nullptr) == -1;
    ok = ok && psdf_sdf_fit_batch(3, 2, 1, 1, buf, buf, idx, buf, nullptr, buf, buf, buf, nullptr) == -1;
    ok = ok && psdf_sdf_fit_batch(3, 2, -1, 1, buf, buf, idx, buf, buf, buf, buf, buf, nullptr) == -1;
    ok = ok && psdf_sdf_fit_batch(3, 2, (int64_t)1 << 31, 1, buf, buf, idx, buf, buf, buf, buf, buf, nullptr) == -2;
    ok = ok && psdf_sdf_fit_loss(2, 1, 1, buf, buf, buf, w, 1, 0, 1, ws, buf, buf, buf, buf, nullptr) == -1;
    ok = ok && psdf_sdf_fit_loss(3, 1, 1, nullptr, buf, buf, w, 1, 0, 1, ws, buf, buf, buf, buf, nullptr) == -1;
    ok = ok && psdf_sdf_fit_loss(3, 1, 1, buf, buf, nullptr, w, 1, 0, 1, ws, buf, buf, buf, buf, nullptr) == -1;
    ok = ok && psdf_sdf_fit_loss(3, 1, 1, buf, buf, buf, nullptr, 1, 0, 1, ws, buf, buf, buf, buf, nullptr) == -1;
    ok = ok && psdf_sdf_fit_loss(3, 1, 1, buf, buf, buf, w, 1, 0, 1, nullptr, buf, buf, buf, buf, nullptr) == -1;
    ok = ok && psdf_sdf_fit_loss(3, 1, 1, buf, buf, buf, w, 1, 0, 1, ws, nullptr, buf, buf, buf, nullptr) == -1;
    ok = ok && psdf_sdf_fit_loss(3, 1, 1, buf, buf, buf, w, 1, 0, 1, ws, buf, buf, buf, nullptr, nullptr) == -1;   // one gradient of two
    ok = ok && psdf_sdf_fit_loss(3, 1, 1, buf, buf, buf, w, nan, 0, 1, ws, buf, buf, buf, buf, nullptr) == -1;
    ok = ok && psdf_sdf_fit_loss(3, 1, 1, buf, buf, buf, w, 1, 0, nan, ws, buf, buf, buf, buf, nullptr) == -1;
    ok = ok && psdf_sdf_fit_loss(3, -1, 1, buf, buf, buf, w, 1, 0, 1, ws, buf, buf, buf, buf, nullptr) == -1;
    ok = ok && psdf_sdf_fit_loss(3, 1, (int64_t)1 << 31, buf, buf, buf, w, 1, 0, 1, ws, buf, buf, buf, buf, nullptr) == -2;
    ok = ok && psdf_sdf_fit_loss(3, 0, 1, buf, buf, nullptr, w, 1, 0, 1, ws, buf, nullptr, nullptr, nullptr, nullptr) == 0;   // no normals needed
    if (!ok) {
      failures++;
      fprintf(stderr, "plan / empty batch / refusals\n");
    }
  }
  if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
  else printf("sdf_fit_kernels_check: all checks passed\n");
  return failures ? 1 : 0;
}
