// Stand-alone check of the ray kernel of permuto_sdf_amd/csrc/frame_rays.hip on the CPU: the file itself is compiled as C++
// against tests/host/hip_on_host/hip/hip_runtime.h (a launch runs on the CPU, thread after thread), driven through its entry
// point and compared with a float64 transcription of the reference's create_rays_from_frame
// (permuto_sdf_py/utils/nerf_utils.py:459-500): K^-1 by float64 inversion, R cam + t - t, normalise.
// tests/test_frame_host.py builds it with -fsanitize=address,undefined -fno-sanitize-recover=all and runs it: the exact-size
// buffers make an index out of bounds a sanitizer report, the padded ones make it a damaged canary.
//
// The bar of every entry is derived from the operand magnitudes, u = 2^-24:
//   pc            (px - cx) / fx: two roundings of a value of magnitude |pc_j|                                 2u |pc_j|
//   R pc          three products (u each) and two sums (u each of a partial sum of at most A_c = sum_j |R_cj| |pc_j|),
//                 on top of the error of pc: at most 5u A_c to first order; 8u A_c leaves room for the second-order terms
//   + t, - t      the sum is rounded at magnitude A_c + |t_c|, the difference at magnitude A_c:        u (2 A_c + |t_c|)
//                 -- counted as 2u |t_c| + 2u A_c, the round trip of the issue plus the share of A_c
//   so            e_c = 10u A_c + 2u |t_c|  on component c of d0
//   normalise     d = d0 / |d0| has the Jacobian (I - d d^T) / |d0|, of norm 1 / |d0|: the error e of d0 moves an entry of d by
//                 at most |e|_2 / |d0|; the squared norm is three products and two sums of positive terms (3u relative), the
//                 reciprocal square root at most 2u (1 / sqrtf here: two roundings; the device's rsqrtf: 1 ulp), the final
//                 product u: (1.5 + 2 + 1) u |d_c| <= 4.5u, counted as 6u
//   bar           |e|_2 / |d0| + 6u
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

static inline float rsqrtf(float x) { return 1.0f / sqrtf(x); }   // the device function; the host's libm has none

#include "frame_rays.hip"

using std::vector;

static int failures = 0;
static const float CANARY = -77.25f;
static const int PAD = 64;   // rows of canary on either side of the outputs

static void fail(const char* what, long a = 0, long b = 0) {
  failures++;
  fprintf(stderr, "FAILED: %s (%ld, %ld)\n", what, a, b);
}

struct Camera {
  int H, W;
  float K[9], T[16];
};

static Camera camera() {
  Camera c{};
  c.H = 41, c.W = 53;
  const float K[9] = {63.6f, 0.f, 24.25f, 0.f, 61.0f, 21.5f, 0.f, 0.f, 1.f};   // fx != fy, cx != W / 2, cy != H / 2
  for (int i = 0; i < 9; i++) c.K[i] = K[i];
  // at distance 1.5 from the origin, looking at it: z = -c / |c|, x = normalize(up x z), y = z x x
  const double dir[3] = {0.3, -0.5, 0.8};
  const double len = std::sqrt(dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2]);
  double pos[3], z[3], x[3], y[3];
  for (int i = 0; i < 3; i++) pos[i] = 1.5 * dir[i] / len, z[i] = -dir[i] / len;
  x[0] = 1.0 * z[2] - 0.0 * z[1], x[1] = 0.0 * z[0] - 0.0 * z[2], x[2] = 0.0 * z[1] - 1.0 * z[0];   // (0, 1, 0) x z
  const double xl = std::sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
  for (int i = 0; i < 3; i++) x[i] /= xl;
  y[0] = z[1] * x[2] - z[2] * x[1], y[1] = z[2] * x[0] - z[0] * x[2], y[2] = z[0] * x[1] - z[1] * x[0];
  for (int r = 0; r < 3; r++) {
    c.T[4 * r] = (float)x[r], c.T[4 * r + 1] = (float)y[r], c.T[4 * r + 2] = (float)z[r], c.T[4 * r + 3] = (float)pos[r];
  }
  c.T[15] = 1.f;
  return c;
}

// float64 inverse of the upper-triangular intrinsic matrix [[fx, s, cx], [0, fy, cy], [0, 0, 1]] by back substitution
static void invert_K(const float* K, double* inv) {
  const double fx = K[0], s = K[1], cx = K[2], fy = K[4], cy = K[5];
  inv[0] = 1.0 / fx, inv[1] = -s / (fx * fy), inv[2] = (s * cy - cx * fy) / (fx * fy);
  inv[3] = 0.0, inv[4] = 1.0 / fy, inv[5] = -cy / fy;
  inv[6] = 0.0, inv[7] = 0.0, inv[8] = 1.0;
}

static void reference(const Camera& c, int pix, double* origin, double* dir, double* bar) {
  const double u = std::ldexp(1.0, -24);
  double inv[9];
  invert_K(c.K, inv);
  const double p[3] = {(double)(pix % c.W) + 0.5, (double)(pix / c.W) + 0.5, 1.0};
  double pc[3], d0[3], e2 = 0.0, n2 = 0.0;
  for (int r = 0; r < 3; r++) pc[r] = inv[3 * r] * p[0] + inv[3 * r + 1] * p[1] + inv[3 * r + 2] * p[2];
  for (int r = 0; r < 3; r++) {
    const double t = c.T[4 * r + 3];
    double pw = 0.0, A = 0.0;
    for (int j = 0; j < 3; j++) pw += (double)c.T[4 * r + j] * pc[j], A += std::fabs((double)c.T[4 * r + j] * pc[j]);
    d0[r] = (pw + t) - t;
    origin[r] = t;
    const double e = 10.0 * u * A + 2.0 * u * std::fabs(t);
    e2 += e * e;
    n2 += d0[r] * d0[r];
  }
  const double n = std::sqrt(n2);
  for (int r = 0; r < 3; r++) dir[r] = d0[r] / n;
  *bar = std::sqrt(e2) / n + 6.0 * u;
}

static double worst_ratio = 0.0, largest_bar = 0.0;

static void run(const Camera& c, long first, int count, const char* label) {
  vector<float> o((size_t)(count + 2 * PAD) * 3, CANARY), d((size_t)(count + 2 * PAD) * 3, CANARY);
  const int status = psdf_frame_rays(c.H, c.W, c.K, c.T, first, count, o.data() + 3 * PAD, d.data() + 3 * PAD, nullptr);
  if (status != 0) return fail(label, status);
  for (size_t i = 0; i < o.size(); i++) {
    const bool inside = i >= (size_t)3 * PAD && i < (size_t)3 * (PAD + count);
    if (!inside && (o[i] != CANARY || d[i] != CANARY)) fail("a canary outside the range was written", first, (long)i);
  }
  // once more into buffers of exactly the range: an index outside is a sanitizer report; the same bits
  vector<float> o2((size_t)count * 3, CANARY), d2((size_t)count * 3, CANARY);
  if (psdf_frame_rays(c.H, c.W, c.K, c.T, first, count, o2.data(), d2.data(), nullptr) != 0) return fail(label, -1);
  for (int i = 0; i < count; i++)
    for (int k = 0; k < 3; k++) {
      const float oo = o[3 * (PAD + i) + k], dd = d[3 * (PAD + i) + k];
      if (std::memcmp(&oo, &o2[3 * i + k], 4) || std::memcmp(&dd, &d2[3 * i + k], 4)) fail("two runs differ", first, i);
    }
  for (int i = 0; i < count; i++) {
    double origin[3], dir[3], bar;
    reference(c, (int)first + i, origin, dir, &bar);
    largest_bar = std::max(largest_bar, bar);
    for (int k = 0; k < 3; k++) {
      if ((double)o2[3 * i + k] != origin[k]) fail("an origin is not the camera's position", first + i, k);
      const double err = std::fabs((double)d2[3 * i + k] - dir[k]);
      worst_ratio = std::max(worst_ratio, err / bar);
      if (!(err <= bar)) fail("a direction misses its bar", first + i, k);
    }
    const double n = std::sqrt((double)d2[3 * i] * d2[3 * i] + (double)d2[3 * i + 1] * d2[3 * i + 1] + (double)d2[3 * i + 2] * d2[3 * i + 2]);
    if (std::fabs(n - 1.0) > 3.0 * bar) fail("a direction is not of unit length", first + i);   // three entries, each within bar
  }
  printf("%-28s pixels [%ld, %ld): ok\n", label, first, first + count);
}

int main() {
  const Camera c = camera();
  const int pixels = c.H * c.W;   // 2173: no multiple of 64, and H != W
  run(c, 0, pixels, "the whole frame");
  run(c, 50, 70, "across two row ends");   // 50 .. 119: the ends of rows 0 and 1 (W = 53)
  run(c, pixels - 1, 1, "the last pixel");
  run(c, 0, 0, "an empty range");
  run(c, 17, 0, "an empty range inside");
  // the centre pixel of a symmetric camera looks along the camera's z axis: a swapped x / y or a row-stride slip moves it
  {
    Camera s = c;
    s.K[2] = 26.5f, s.K[5] = 20.5f;   // the centre of pixel (26, 20)
    float o[3], d[3];
    if (psdf_frame_rays(s.H, s.W, s.K, s.T, 20 * s.W + 26, 1, o, d, nullptr) != 0) fail("centre pixel");
    for (int k = 0; k < 3; k++)
      if (std::fabs((double)d[k] - (double)s.T[4 * k + 2]) > largest_bar)   // (the bars of the runs above: the same geometry)
        fail("the centre pixel does not look along z", k);
  }
  // an empty batch returns before any pointer check; the refusals
  if (psdf_frame_rays(0, 0, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr) != 0) fail("empty batch");
  float one[3];
  if (psdf_frame_rays(c.H, c.W, nullptr, c.T, 0, 1, one, one, nullptr) != -1) fail("a NULL K is accepted");
  if (psdf_frame_rays(c.H, c.W, c.K, c.T, 0, 1, nullptr, one, nullptr) != -1) fail("a NULL output is accepted");
  if (psdf_frame_rays(c.H, c.W, c.K, c.T, pixels, 1, one, one, nullptr) != -1) fail("a range past the frame is accepted");
  if (psdf_frame_rays(c.H, c.W, c.K, c.T, -1, 1, one, one, nullptr) != -1) fail("a negative first pixel is accepted");
  if (psdf_frame_rays(0, c.W, c.K, c.T, 0, 1, one, one, nullptr) != -1) fail("an empty frame is accepted");
  if (psdf_frame_rays(65536, 32768, c.K, c.T, 0, 1, one, one, nullptr) != -2) fail("a frame of 2^31 pixels is accepted");
  // the library's plan entry is the header's
  {
    int64_t out[PSDF_FRAME_PLAN_FIELDS] = {-9, -9, -9};
    if (psdf_frame_plan(1200, 1600, 64, 2097152, out) != 0 || out[0] != 32768 || out[1] != 59 || out[2] != 19456) fail("plan entry");
    if (psdf_frame_plan(1200, 1600, 64, 2097152, nullptr) != -1 || psdf_frame_plan(0, 1600, 64, 2097152, out) != -1) fail("plan refusals");
  }
  printf("largest bar %.3e, worst error / bar %.3f\n", largest_bar, worst_ratio);
  if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
  else printf("frame_rays_check: all checks passed\n");
  return failures;
}
