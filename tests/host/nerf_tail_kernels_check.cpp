// Stand-alone check of the loss tail and the head join of permuto_sdf_amd/csrc/nerf_render.hip on the CPU: the file itself is
// compiled as C++ against tests/host/hip_on_host/hip/hip_runtime.h (launches run on CPU threads), driven the way
// permuto_sdf_amd/nerf_train.py drives it (plan, workspace, the entries) and compared with brute-force float64 written as plain
// loops.  tests/test_nerf_host.py builds it with -fsanitize=address,undefined -fno-sanitize-recover=all and runs it: every buffer
// has exactly the extent the header states, so an index out of bounds in a kernel is a sanitizer report here, not a fault on a
// device.  It says nothing about speed, and nothing about what the device compiler makes of the source.
//
// The file also holds the ray kernels, which sweep a ray with wave shuffles: the stand-in header does not model those (its
// __shfl_up returns the caller's own value), so they are compiled here and NEVER RUN -- psdf_nerf_render_forward / _backward are
// called with empty batches and bad arguments only, which return before any launch.  What the helper headers name beyond the
// stand-in (gridDim, two more shuffles, the device's fast-math builtins of gelu_device.h) is declared below, for this program alone.
//
// Bars (u = 2^-24), as derived in tests/nerf_render_float64.py: a term is a mean of fp32 rows added in double -- the squared error
// 4 u, the cross entropy 8 u (1 + |row|) per row (two logarithms within 2 ulps, 1 - c within u); g_pred 4 u, g_weights_sum 7 u
// relative; gelu 4 u |z|, gelu' |z| pdf (36 u + z^2 u) + 3.5 u (the exponential here is the host's expf, well inside the device's bound).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <random>

inline thread_local dim3 gridDim;
template <class T> T __shfl_down(T v, int, int) { return v; }
template <class T> T __shfl(T v, int, int) { return v; }
#define __expf(x) expf(x)
#define __builtin_amdgcn_exp2f(x) exp2f(x)
#define __builtin_amdgcn_rcpf(x) (1.0f / (x))
#define __builtin_amdgcn_fmed3f(a, b, c) fmaxf(fminf(fmaxf(a, b), c), fminf(a, b))

#include "nerf_render.hip"

using std::vector;

static std::mt19937 rng(11);
static int failures = 0;
static const double U = std::ldexp(1.0, -24);

static void fail(const char* label, const char* what, long at, double got, double want, double bar) {
  if (failures < 20) fprintf(stderr, "%s: %s[%ld] = %.9g, expected %.9g (bar %.3g)\n", label, what, at, got, want, bar);
  failures++;
}

struct LossCase {
  const char* label;
  int64_t R;
  bool with_hit, with_mask, with_loss, with_grad;
};

static void run_loss(const LossCase& k) {
  const int64_t R = k.R;
  std::uniform_real_distribution<double> uni(0.0, 1.0);
  hip_on_host::concurrent = true;   // the loss kernels synchronise
  vector<float> pred(3 * R), gt(3 * R), ws(R), mask(R);
  vector<unsigned char> hit(R);
  const float lo = 1e-3f, hi = (float)(1.0 - 1e-3);
  const float special[] = {lo, hi, std::nextafterf(lo, 0.f), std::nextafterf(lo, 1.f), std::nextafterf(hi, 0.f), std::nextafterf(hi, 2.f),
                           0.f, 1.f, 1.0000004f, 5e-4f, 0.5f};
  for (auto& v : pred) v = (float)uni(rng);
  for (auto& v : gt) v = (float)uni(rng);
  for (int64_t r = 0; r < R; r++) {
    hit[r] = uni(rng) < 0.8;
    ws[r] = r % 3 == 0 ? special[(r / 3) % 11] : (float)uni(rng);
    mask[r] = r % 5 == 0 ? (float)uni(rng) : (uni(rng) < 0.5 ? 1.f : 0.f);
  }
  int64_t pl[PSDF_NERF_RENDER_PLAN_FIELDS];
  if (psdf_nerf_render_plan(R, 64, pl) != 0) fail(k.label, "plan", 0, -1, 0, 0);
  vector<double> work(pl[1] / 8, -1.0);
  vector<float> terms(2, 7.f), again(2, 7.f), g_pred(k.with_grad ? 3 * R : 0, 7.f), g_ws(k.with_grad ? R : 0, 7.f);
  float loss = 0.25f;
  const float weight = 0.1f;
  int status = psdf_nerf_loss(R, pred.data(), gt.data(), k.with_hit ? hit.data() : nullptr, k.with_mask ? ws.data() : nullptr,
                              k.with_mask ? mask.data() : nullptr, weight, work.data(), terms.data(), k.with_loss ? &loss : nullptr,
                              k.with_grad ? g_pred.data() : nullptr, k.with_grad ? g_ws.data() : nullptr, nullptr);
  if (status != 0) fail(k.label, "loss status", 0, status, 0, 0);
  // the same call without loss and gradients gives the same bits
  status = psdf_nerf_loss(R, pred.data(), gt.data(), k.with_hit ? hit.data() : nullptr, k.with_mask ? ws.data() : nullptr,
                          k.with_mask ? mask.data() : nullptr, weight, work.data(), again.data(), nullptr, nullptr, nullptr, nullptr);
  if (status != 0 || memcmp(terms.data(), again.data(), 8) != 0) fail(k.label, "terms of a second call", 0, again[0], terms[0], 0);

  double sum0 = 0, sum1 = 0, bar1 = 0, worst = 0;
  for (int64_t r = 0; r < R; r++) {
    const double h = k.with_hit ? (hit[r] ? 1.0 : 0.0) : 1.0;
    for (int c = 0; c < 3; c++) {
      const double d = (double)gt[3 * r + c] - (double)pred[3 * r + c];
      sum0 += d * d * h;
      if (!k.with_grad) continue;
      const double want = -2.0 * d * h / (3.0 * R), bar = 4 * U * std::fabs(want) + 1e-37, err = std::fabs(g_pred[3 * r + c] - want);
      if (!(err <= bar)) fail(k.label, "g_pred", 3 * r + c, g_pred[3 * r + c], want, bar);
      worst = std::max(worst, err / bar);
    }
    double want_g = 0.0;
    if (k.with_mask) {
      const double w = ws[r], t = mask[r], c = std::min(std::max(w, (double)lo), (double)hi), om = 1.0 - c;
      const double row = -(t * std::log(c) + (1.0 - t) * std::log(om));
      sum1 += row;
      bar1 += 8 * U * (1.0 + std::fabs(row));
      if (w >= lo && w <= hi) want_g = (double)weight * (c - t) / (om * c) / (double)R;
    }
    if (k.with_grad) {
      const double bar = 7 * U * std::fabs(want_g) + 1e-37, err = std::fabs(g_ws[r] - want_g);
      if (!(err <= bar) || (want_g == 0.0 && g_ws[r] != 0.0f)) fail(k.label, "g_weights_sum", r, g_ws[r], want_g, bar);
      worst = std::max(worst, err / bar);
    }
  }
  const double want0 = sum0 / (3.0 * R), want1 = k.with_mask ? sum1 / R : 0.0;
  const double b0 = 4 * U * want0 + U * want0 + 1e-37, b1 = (k.with_mask ? bar1 / R : 0.0) + U * std::fabs(want1) + 1e-37;
  if (!(std::fabs(terms[0] - want0) <= b0)) fail(k.label, "terms", 0, terms[0], want0, b0);
  if (!(std::fabs(terms[1] - want1) <= b1) || (!k.with_mask && terms[1] != 0.0f)) fail(k.label, "terms", 1, terms[1], want1, b1);
  worst = std::max(worst, std::max(std::fabs(terms[0] - want0) / b0, std::fabs(terms[1] - want1) / b1));
  if (k.with_loss) {
    const double want = 0.25 + want0 + (double)weight * want1, bar = b0 + weight * b1 + 4 * U * (0.25 + want0 + weight * std::fabs(want1));
    if (!(std::fabs(loss - want) <= bar)) fail(k.label, "loss", 0, loss, want, bar);
  }
  printf("%-34s %6ld rays, %3ld workgroups: worst error / bar %.2e\n", k.label, (long)R, (long)pl[0], worst);
}

static void run_join(int64_t M) {
  std::normal_distribution<double> normal(0.0, 1.0);
  hip_on_host::concurrent = false;   // no barrier in these kernels: a thread past the end of the samples leaves early
  vector<float> fd(65 * M), sh(M * 16), x2(80 * M, 7.f), g_raw(M), dX2(80 * M), g_fd(65 * M, 7.f);
  for (auto& v : fd) v = (float)(3.0 * normal(rng));
  for (int64_t i = 0; i < (int64_t)fd.size(); i += 17) fd[i] = (i % 2 ? -1.f : 1.f) * (float)(i % 11);      // 0, far tails
  for (auto& v : sh) v = (float)normal(rng);
  for (auto& v : g_raw) v = (float)normal(rng);
  for (auto& v : dX2) v = (float)normal(rng);
  if (psdf_nerf_head_join(M, fd.data(), sh.data(), x2.data(), nullptr) != 0) fail("head join", "status", M, -1, 0, 0);
  if (psdf_nerf_head_join_backward(M, g_raw.data(), dX2.data(), fd.data(), g_fd.data(), nullptr) != 0) fail("head join backward", "status", M, -1, 0, 0);
  double worst = 0;
  for (int64_t m = 0; m < M; m++) {
    for (int r = 0; r < 80; r++) {
      const float got = x2[r * M + m];
      if (r >= 64) {
        if (got != sh[m * 16 + (r - 64)]) fail("head join", "harmonics", r * M + m, got, sh[m * 16 + (r - 64)], 0);
        continue;
      }
      const double z = fd[(1 + r) * M + m], want = 0.5 * z * (1.0 + std::erf(z / std::sqrt(2.0))), bar = 4 * U * std::fabs(z) + 1e-37;
      if (!(std::fabs(got - want) <= bar)) fail("head join", "gelu", r * M + m, got, want, bar);
      worst = std::max(worst, std::fabs(got - want) / bar);
    }
    if (g_fd[m] != g_raw[m]) fail("head join backward", "density row", m, g_fd[m], g_raw[m], 0);
    for (int r = 0; r < 64; r++) {
      const double z = fd[(1 + r) * M + m], pdf = std::exp(-0.5 * z * z) / std::sqrt(2.0 * M_PI);
      const double der = 0.5 * (1.0 + std::erf(z / std::sqrt(2.0))) + z * pdf, g = dX2[r * M + m], want = g * der;
      const double bar = std::fabs(g) * (std::fabs(z) * pdf * (36 * U + z * z * U) + 3.5 * U + U * std::fabs(der)) + U * std::fabs(want) + 1e-37;
      const double err = std::fabs(g_fd[(1 + r) * M + m] - want);
      if (!(err <= bar)) fail("head join backward", "g_fd", (1 + r) * M + m, g_fd[(1 + r) * M + m], want, bar);
      worst = std::max(worst, err / bar);
    }
  }
  printf("head join and its backward         %6ld samples: worst error / bar %.2e\n", (long)M, worst);
}

int main() {
  namespace plan = psdf::nerf_render_plan;
  const int64_t pass = plan::RAYS_PER_PASS;
  const LossCase cases[] = {
      {"one ray", 1, true, true, true, true},
      {"63 rays, no hit mask", 63, false, true, true, true},
      {"257 rays", 257, true, true, true, true},
      {"257 rays, no mask term", 257, true, false, true, true},
      {"257 rays, no gradients", 257, true, true, false, false},
      {"one ray past a full pass", pass + 1, true, true, true, true},
  };
  for (const LossCase& k : cases) run_loss(k);
  for (int64_t M : {1, 63, 64, 65, 1000}) run_join(M);
  // the plan, empty batches and refusals, before any launch
  {
    int64_t pl[PSDF_NERF_RENDER_PLAN_FIELDS];
    bool ok = psdf_nerf_render_plan(512, 64, pl) == 0 && pl[0] == 2 && pl[1] == 2 * 2 * 8 && pl[2] == pass && pl[3] == 1;
    ok = ok && psdf_nerf_render_plan(0, 256, pl) == 0 && pl[0] == 0 && pl[1] == 0 && pl[3] == 4;
    ok = ok && psdf_nerf_render_plan(pass + 1, 65, pl) == 0 && pl[0] == plan::MAX_GRID && pl[3] == 2;
    ok = ok && psdf_nerf_render_plan(-1, 64, pl) == -1 && psdf_nerf_render_plan(1, 0, pl) == -1 && psdf_nerf_render_plan(1, 64, nullptr) == -1;
    ok = ok && psdf_nerf_render_plan(plan::MAX_RAYS + 1, 64, pl) == -2 && psdf_nerf_render_plan(1, 257, pl) == -2;
    float buf[16] = {0}, nan = std::nanf("");
    double ws[8];
    int se[2] = {0, 1};
    unsigned char h[4] = {1, 1, 1, 1};
    // the ray entries: never launched here
    ok = ok && psdf_nerf_render_forward(0, nullptr, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0;
    ok = ok && psdf_nerf_render_backward(-1, nullptr, 0, 0, 0, 999, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr) == 0;
    ok = ok && psdf_nerf_render_forward(1, se, 0, 0, 1, buf, buf, buf, nullptr, nullptr, nullptr, nullptr) == -1;      // no output
    ok = ok && psdf_nerf_render_forward(1, nullptr, 0, 0, 1, buf, buf, buf, buf, buf, buf, nullptr) == -1;            // no ranges
    ok = ok && psdf_nerf_render_forward(1, se, 0, 0, 1, buf, buf, nullptr, buf, buf, buf, nullptr) == -1;             // pred without rgb
    ok = ok && psdf_nerf_render_forward(1, se, 0, 0, 1, nullptr, buf, buf, buf, buf, buf, nullptr) == -1;
    ok = ok && psdf_nerf_render_backward(1, se, 0, 0, 1, 64, nullptr, nullptr, nullptr, buf, buf, buf, 0, buf, buf, nullptr) == -1;   // no upstream
    ok = ok && psdf_nerf_render_backward(1, se, 0, 0, 1, 64, buf, buf, buf, buf, buf, nullptr, 0, buf, buf, nullptr) == -1;          // g_pred without rgb
    ok = ok && psdf_nerf_render_backward(1, se, 0, 0, 1, 64, buf, buf, buf, buf, buf, buf, 0, nullptr, buf, nullptr) == -1;
    ok = ok && psdf_nerf_render_backward(1, se, 0, 0, 1, 0, buf, buf, buf, buf, buf, buf, 0, buf, buf, nullptr) == -1;
    ok = ok && psdf_nerf_render_backward(1, se, 0, 0, 1, 257, buf, buf, buf, buf, buf, buf, 0, buf, buf, nullptr) == -2;
    // the loss
    ok = ok && psdf_nerf_loss(0, nullptr, nullptr, nullptr, nullptr, nullptr, nan, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0;
    ok = ok && psdf_nerf_loss(1, nullptr, buf, h, buf, buf, 0.1f, ws, buf, buf, buf, buf, nullptr) == -1;
    ok = ok && psdf_nerf_loss(1, buf, nullptr, h, buf, buf, 0.1f, ws, buf, buf, buf, buf, nullptr) == -1;
    ok = ok && psdf_nerf_loss(1, buf, buf, h, buf, nullptr, 0.1f, ws, buf, buf, buf, buf, nullptr) == -1;      // weight sum without mask
    ok = ok && psdf_nerf_loss(1, buf, buf, h, nullptr, buf, 0.1f, ws, buf, buf, buf, buf, nullptr) == -1;
    ok = ok && psdf_nerf_loss(1, buf, buf, h, buf, buf, 0.1f, nullptr, buf, buf, buf, buf, nullptr) == -1;
    ok = ok && psdf_nerf_loss(1, buf, buf, h, buf, buf, 0.1f, ws, nullptr, buf, buf, buf, nullptr) == -1;
    ok = ok && psdf_nerf_loss(1, buf, buf, h, buf, buf, nan, ws, buf, buf, buf, buf, nullptr) == -1;
    ok = ok && psdf_nerf_loss(plan::MAX_RAYS + 1, buf, buf, h, buf, buf, 0.1f, ws, buf, buf, buf, buf, nullptr) == -2;
    // the join
    ok = ok && psdf_nerf_head_join(0, nullptr, nullptr, nullptr, nullptr) == 0 && psdf_nerf_head_join_backward(0, nullptr, nullptr, nullptr, nullptr, nullptr) == 0;
    ok = ok && psdf_nerf_head_join(-1, buf, buf, buf, nullptr) == -1 && psdf_nerf_head_join(1, nullptr, buf, buf, nullptr) == -1;
    ok = ok && psdf_nerf_head_join(1, buf, nullptr, buf, nullptr) == -1 && psdf_nerf_head_join(1, buf, buf, nullptr, nullptr) == -1;
    ok = ok && psdf_nerf_head_join((int64_t)1 << 31, buf, buf, buf, nullptr) == -2;
    ok = ok && psdf_nerf_head_join_backward(1, nullptr, buf, buf, buf, nullptr) == -1 && psdf_nerf_head_join_backward(1, buf, nullptr, buf, buf, nullptr) == -1;
    ok = ok && psdf_nerf_head_join_backward(1, buf, buf, nullptr, buf, nullptr) == -1 && psdf_nerf_head_join_backward(1, buf, buf, buf, nullptr, nullptr) == -1;
    ok = ok && psdf_nerf_head_join_backward((int64_t)1 << 31, buf, buf, buf, buf, nullptr) == -2;
    if (!ok) {
      failures++;
      fprintf(stderr, "plan / empty batch / refusals\n");
    }
  }
  if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
  else printf("nerf_tail_kernels_check: all checks passed\n");
  return failures ? 1 : 0;
}
