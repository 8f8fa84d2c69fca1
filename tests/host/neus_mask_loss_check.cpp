// Stand-alone check of the loss tail of permuto_sdf_amd/csrc/neus_render.hip on the CPU: the file itself is compiled as C++ against
// tests/host/hip_on_host/hip/hip_runtime.h (launches run on CPU threads), driven the way permuto_sdf_amd/neus.py drives it (plan,
// workspace, the entry) and compared with brute-force float64 written as plain loops.  tests/test_neus_render_host.py builds it
// with -fsanitize=address,undefined -fno-sanitize-recover=all and runs it: every buffer has exactly the extent the header states,
// so an index out of bounds in a kernel is a sanitizer report here, not a fault on a device.  It says nothing about speed, and
// nothing about what the device compiler makes of the source.
//
// The file also holds the ray kernels, which sweep a ray with wave shuffles: the stand-in header does not model those (its
// __shfl_up returns the caller's own value), so they are compiled here and NEVER RUN -- psdf_neus_render_forward / _backward are
// called with empty batches and bad arguments only, which return before any launch.  What the helper headers name beyond the
// stand-in (gridDim, two more shuffles, the float atomic of the inv_s gradient) is declared below, for this program alone.
//
// Bars (u = 2^-24), as derived in tests/neus_render_float64.py: the colour term is a sum of fp32 rows |d| (1 rounding each) added
// in double and weighted by an fp32 scale: 3 u; the cross entropy 8 u (1 + |row|) per row (two logarithms within 2 ulps, 1 - c
// within u); g_pred 2 u, g_weights_sum 7 u relative; the result is rounded to fp32 and added to the accumulator: 2 u of it.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <random>

inline thread_local dim3 gridDim;
template <class T> T __shfl_down(T v, int, int) { return v; }
template <class T> T __shfl(T v, int, int) { return v; }
inline float atomicAdd(float* p, float v) { const float old = *p; *p = old + v; return old; }

#include "neus_render.hip"

using std::vector;

static std::mt19937 rng(13);
static int failures = 0;
static const double U = std::ldexp(1.0, -24);

static void fail(const char* label, const char* what, long at, double got, double want, double bar) {
  if (failures < 20) fprintf(stderr, "%s: %s[%ld] = %.9g, expected %.9g (bar %.3g)\n", label, what, at, got, want, bar);
  failures++;
}

enum HitMode { HIT_NULL, HIT_ZERO, HIT_MIXED };

static void run_loss(int64_t R, HitMode hm, bool with_grad) {
  char label[64];
  snprintf(label, sizeof label, "R %ld hit %s%s", (long)R, hm == HIT_NULL ? "null" : (hm == HIT_ZERO ? "zero" : "mixed"), with_grad ? "" : ", no gradients");
  std::uniform_real_distribution<double> uni(0.0, 1.0);
  hip_on_host::concurrent = true;   // the loss kernels synchronise
  vector<float> pred(3 * R), gt(3 * R), ws(R), mask(R);
  vector<unsigned char> hit(R);
  const float lo = 1e-3f, hi = (float)(1.0 - 1e-3);
  // 0, one step below / at / above each clip bound, 0.5, 1: against both mask values
  const float special[] = {0.f, std::nextafterf(lo, 0.f), lo, std::nextafterf(lo, 1.f), 0.5f, std::nextafterf(hi, 0.f), hi, std::nextafterf(hi, 2.f), 1.f};
  for (auto& v : pred) v = (float)uni(rng);
  for (auto& v : gt) v = (float)uni(rng);
  for (int64_t r = 0; r < R; r++) {
    if (r % 7 == 0) pred[3 * r + 1] = gt[3 * r + 1];      // the sign's zero arm
    hit[r] = hm == HIT_ZERO ? 0 : (uni(rng) < 0.8);
    ws[r] = special[r % 9];
    mask[r] = (float)((r / 9) % 2);
  }
  int64_t pl[PSDF_NEUS_RENDER_PLAN_FIELDS];
  if (psdf_neus_render_plan(R, 64, pl) != 0) fail(label, "plan", 0, -1, 0, 0);
  if ((R <= pl[3]) != (pl[2] == 0)) fail(label, "workspace of the plan", 0, (double)pl[2], 0, 0);
  vector<double> work(pl[2] / 8, -1.0);
  vector<float> g_pred(with_grad ? 3 * R : 0, 7.f), g_ws(with_grad ? R : 0, 7.f);
  const float base = 0.25f, weight = 0.1f;
  const float scale_rgb = (float)(1.0 / (3.0 * R)), scale_mask = (float)((double)weight / R);
  const unsigned char* h = hm == HIT_NULL ? nullptr : hit.data();
  float loss = base;                 // a nonzero value beforehand: added to, not overwritten
  int status = psdf_neus_mask_loss(R, pred.data(), gt.data(), h, ws.data(), mask.data(), scale_rgb, scale_mask,
                                   work.empty() ? nullptr : work.data(), &loss, with_grad ? g_pred.data() : nullptr,
                                   with_grad ? g_ws.data() : nullptr, nullptr);
  if (status != 0) fail(label, "status", 0, status, 0, 0);
  // a second call (without gradients) gives the same bits
  float again = base;
  status = psdf_neus_mask_loss(R, pred.data(), gt.data(), h, ws.data(), mask.data(), scale_rgb, scale_mask,
                               work.empty() ? nullptr : work.data(), &again, nullptr, nullptr, nullptr);
  if (status != 0 || memcmp(&loss, &again, 4) != 0) fail(label, "loss of a second call", 0, again, loss, 0);

  double sum0 = 0, sum1 = 0, bar1 = 0, worst = 0;
  for (int64_t r = 0; r < R; r++) {
    const double hh = hm == HIT_NULL ? 1.0 : (hit[r] ? 1.0 : 0.0);
    for (int c = 0; c < 3; c++) {
      const double d = (double)pred[3 * r + c] - (double)gt[3 * r + c];
      sum0 += std::fabs(d) * hh;
      if (!with_grad) continue;
      const double want = (d > 0 ? 1.0 : (d < 0 ? -1.0 : 0.0)) * hh / (3.0 * R), bar = 2 * U * std::fabs(want), err = std::fabs(g_pred[3 * r + c] - want);
      if (!(err <= bar)) fail(label, "g_pred", 3 * r + c, g_pred[3 * r + c], want, bar);
      if (bar > 0) worst = std::max(worst, err / bar);
    }
    const double w = ws[r], t = mask[r], c = std::min(std::max(w, (double)lo), (double)hi), om = 1.0 - c;
    const double row = -(t * std::log(c) + (1.0 - t) * std::log(om));
    sum1 += row;
    bar1 += 8 * U * (1.0 + std::fabs(row));
    const bool inside = w >= lo && w <= hi;
    const double want_g = inside ? (double)weight * (c - t) / (om * c) / (double)R : 0.0;
    // the two boundaries: AT a bound the gradient passes, one step outside it is exactly zero
    if (with_grad) {
      const double bar = 7 * U * std::fabs(want_g) + 1e-37, err = std::fabs(g_ws[r] - want_g);
      if (!(err <= bar) || (!inside && g_ws[r] != 0.0f) || (inside && g_ws[r] == 0.0f)) fail(label, "g_weights_sum", r, g_ws[r], want_g, bar);
      worst = std::max(worst, err / bar);
    }
  }
  const double t0 = sum0 / (3.0 * R), t1 = sum1 / R;
  const double want = (double)base + t0 + (double)weight * t1;
  const double bar = 3 * U * t0 + weight * (bar1 / R + 2 * U * std::fabs(t1)) + 2 * U * (base + std::fabs(want)) + 1e-37;
  if (!(std::fabs(loss - want) <= bar)) fail(label, "loss", 0, loss, want, bar);
  if (hm == HIT_ZERO && !(std::fabs(loss - (base + weight * t1)) <= bar)) fail(label, "loss without a hit", 0, loss, base + weight * t1, bar);
  worst = std::max(worst, std::fabs(loss - want) / bar);
  printf("%-40s %3ld workgroup(s), %5ld bytes of workspace: worst error / bar %.2e\n", label, (long)pl[1], (long)pl[2], worst);
}

int main() {
  int64_t pl[PSDF_NEUS_RENDER_PLAN_FIELDS];
  if (psdf_neus_render_plan(1, 64, pl) != 0) return 2;
  const int64_t lim = pl[3];
  for (int64_t R : {(int64_t)1, (int64_t)255, (int64_t)256, (int64_t)257, lim, lim + 1})
    for (HitMode hm : {HIT_NULL, HIT_ZERO, HIT_MIXED}) run_loss(R, hm, true);
  run_loss(257, HIT_MIXED, false);
  run_loss(lim + 1, HIT_MIXED, false);

  // ---- codes: empty batches before any pointer check, NULL required pointers, the ray length beyond the register chunks
  float x = 0.f;
  double wk = 0.0;
  int se[2] = {0, 1};
  if (psdf_neus_mask_loss(0, nullptr, nullptr, nullptr, nullptr, nullptr, 1.f, 1.f, nullptr, nullptr, nullptr, nullptr, nullptr) != 0)
    fail("codes", "empty loss", 0, -1, 0, 0);
  if (psdf_neus_mask_loss(1, nullptr, &x, nullptr, &x, &x, 1.f, 1.f, nullptr, &x, nullptr, nullptr, nullptr) != -1) fail("codes", "pred", 0, 0, -1, 0);
  if (psdf_neus_mask_loss(1, &x, &x, nullptr, nullptr, &x, 1.f, 1.f, nullptr, &x, nullptr, nullptr, nullptr) != -1) fail("codes", "weights_sum", 0, 0, -1, 0);
  if (psdf_neus_mask_loss(1, &x, &x, nullptr, &x, &x, 1.f, 1.f, nullptr, nullptr, nullptr, nullptr, nullptr) != -1) fail("codes", "loss", 0, 0, -1, 0);
  if (psdf_neus_mask_loss(lim + 1, &x, &x, nullptr, &x, &x, 1.f, 1.f, nullptr, &x, nullptr, nullptr, nullptr) != -1) fail("codes", "workspace", 0, 0, -1, 0);
  if (psdf_neus_mask_loss(1, &x, &x, nullptr, &x, &x, std::nanf(""), 1.f, &wk, &x, nullptr, nullptr, nullptr) != -1) fail("codes", "scale", 0, 0, -1, 0);
  if (psdf_neus_mask_loss((int64_t)0x7fffffff / 3 + 1, &x, &x, nullptr, &x, &x, 1.f, 1.f, &wk, &x, nullptr, nullptr, nullptr) != -2) fail("codes", "R", 0, 0, -2, 0);
  if (psdf_neus_render_forward(0, nullptr, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, nullptr, nullptr, nullptr, nullptr) != 0)
    fail("codes", "empty forward", 0, -1, 0, 0);
  if (psdf_neus_render_forward(1, se, 0, 0, 1, &x, &x, &x, &x, &x, &x, 0.f, nullptr, nullptr, nullptr, nullptr) != -1) fail("codes", "no output", 0, 0, -1, 0);
  if (psdf_neus_render_backward(0, nullptr, 0, 0, 0, 999, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, 0, nullptr,
                                nullptr, nullptr, nullptr, nullptr) != 0)
    fail("codes", "empty backward", 0, -1, 0, 0);
  if (psdf_neus_render_backward(1, se, 0, 0, 1, 64, nullptr, nullptr, nullptr, &x, &x, &x, &x, &x, &x, 0.f, 0, &x, nullptr, nullptr, nullptr, nullptr) != -1)
    fail("codes", "no upstream", 0, 0, -1, 0);
  if (psdf_neus_render_backward(1, se, 0, 0, 1, 257, &x, &x, nullptr, &x, &x, &x, &x, &x, &x, 0.f, 0, &x, nullptr, nullptr, nullptr, nullptr) != -2)
    fail("codes", "max_per_ray", 0, 0, -2, 0);

  if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
  else printf("neus_mask_loss_check: all checks passed\n");
  return failures ? 1 : 0;
}
