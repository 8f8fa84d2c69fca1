// Stand-alone check of permuto_sdf_amd/csrc/sdf_slice.hip on the CPU: the file itself is compiled as C++ against
// tests/host/hip_on_host/hip/hip_runtime.h (a launch runs on the CPU, thread after thread), driven through its four entry points.
// tests/test_sdf_slice_host.py builds it with -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all and runs
// it.  Every output lies between two rows of canaries inside its allocation and the allocation is of exactly that size: a write
// next to an output changes a canary, a write further out is a sanitizer report.  csrc/frame_rays.hip is compiled in as well:
// the rays of the cut are the ray kernel's own.
//
//   points    the BITS of every point and flag against ref_point below, a scalar restatement of
//             visualize_sdf_isolines.py:77-92 written the way the reference is (x / width - 0.5, then * 2.0, float32; the rotation
//             in float64, rounded once) and of aabb.py:28-42.  S in {1, 2, 37}, whole layers and the range first = 5, count =
//             S S - 7 of S = 37 (it starts and ends mid-row), rows of 3 and of 4 floats, a rotated plane, a box smaller than
//             the layer.
//   bands     exact decisions: every lo_i and hi_i itself (not in the band), nextafter either side of them, width > distance
//             (overlapping bands: the later one wins), negative values, values above 0.3, a NaN, skipped cells.  A cell in a band
//             holds the band's colour bit for bit; any other cell holds the base colour within its bar, which at every such
//             input below 0.29 lies more than 10 bars away from the colour of the band next to it (from 0.3 on both maps have
//             reached the end of the table and a decision cannot be seen in the colour).
//   colours   per channel against float64 on the same float32 inputs, u = 2^-24.  t = out_lo + scale (clamp(s) - in_lo): a
//             difference, a product, a sum, 3u T with T = |out_lo| + |scale (clamp(s) - in_lo)|; the position t (K - 1) rounds
//             once more: |position error| <= 4u T (K - 1).  table() is continuous and piecewise linear with slope at most D =
//             max_j |b_j - a_j| per unit of position: 4u T (K - 1) D.  f = position - j is exact (Sterbenz: j <= position <
//             2 j for j >= 1; j = 0 subtracts nothing); b - a, f (b - a) and a + ... round once each: 2u D + u M, M the largest
//             control value.  bar = u (4 T (K - 1) D + 2 D + 2 M): the second M is room for second-order terms.
//   cut       begin against float64 on the same float32 rays, 41 x 53 frame, the camera, plane, box and sphere of
//             tests/test_gpu_sdf_slice.py (test 4).  With N = dot(n, z n - o), Dn = dot(n, d):
//               errN = 5u sum |n_i| (|z n_i| + |o_i|)    (z n_i, the difference, the product: 3 roundings; 2 sums)
//               errD = 3u sum |n_i d_i|
//               errt = (errN + |t| errD) / (|Dn| - errD) + u |t|
//               errp_i = |d_i| errt + u |t d_i| + u |p_i|
//               erru = sum |a_i| errp_i + 3u sum |a_i p_i|    (in-plane coordinates)
//               errq_i = errp_i + u |p_i - tr_i|              (the box test)
//             A ray is checked when |Dn| > 2 errD, |t| > errt, each in-plane coordinate is further than erru from -extent and
//             from extent, each |q_i| further than errq_i from half_i, and, where the pixel has a surface, |t - depth| > errt.
//             At most 1 % of the rays may fail that (a cap on the float64 geometry alone, checked before the kernel runs);
//             every checked ray must have the float64 decision, and a ray that takes part its point and t within errp, errt.
//             The frame must hold grazing rays (|Dn| < 0.02), rays that meet the plane behind the camera, rays that miss the
//             box, pixels where the slice wins over the sphere, where the sphere wins and where there is no surface.
//   resolve   in place: rays that take part get the colorize entry's colour of the same value bit for bit, depth = t, weight 1,
//             mask 1; every other pixel of the chunk keeps its bits and gets mask 0; nothing outside the chunk is written.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include <hip/hip_runtime.h>
static inline float rsqrtf(float x) { return 1.0f / sqrtf(x); }   // the device function of the ray kernel; the host's libm has none
// cross-lane operations and launch geometry that csrc/composite_device.h (sdf_slice.hip takes it through frame_device.h) names in
// helpers these kernels never call
template <class T> T __shfl(T v, int, int) { return v; }
template <class T> T __shfl_down(T v, int, int) { return v; }
inline thread_local dim3 gridDim;

#include "frame_rays.hip"
#include "sdf_slice.hip"

using std::vector;

static int failures = 0;
static const double U = 1.0 / 16777216.0;
static double worst_colour = 0.0, worst_point = 0.0, worst_t = 0.0;

static void fail(const char* what, long a = 0, long b = 0) {
  failures++;
  if (failures < 40) fprintf(stderr, "FAILED: %s (%ld, %ld)\n", what, a, b);
}

static uint32_t lcg_state = 97531u;
static float uni() {   // uniform in [0, 1), 24 bits
  lcg_state = lcg_state * 1664525u + 1013904223u;
  return (float)(lcg_state >> 8) / 16777216.0f;
}

template <class T> static bool same_bits(T a, T b) { return std::memcmp(&a, &b, sizeof(T)) == 0; }

template <class T> struct Guarded {
  static constexpr int PAD = 16;
  vector<T> all;
  size_t n;
  T canary;
  Guarded(size_t n_, T canary_) : all(n_ + 2 * PAD, canary_), n(n_), canary(canary_) {}
  T* data() { return all.data() + PAD; }
  T& operator[](size_t i) { return all[PAD + i]; }
  bool intact() const {
    for (int i = 0; i < PAD; i++)
      if (!same_bits(all[i], canary) || !same_bits(all[PAD + n + i], canary)) return false;
    return true;
  }
};
static const float CANARY = -77.25f;
static const unsigned char BCANARY = 0xA5;

// ---------------------------------------------------------------------------------------------------- the plane and the box
// rotation by `deg` about `axis`, float64 rounded to float32, row major
static void rotation(const double* axis, double deg, float* R) {
  const double n = std::sqrt(axis[0] * axis[0] + axis[1] * axis[1] + axis[2] * axis[2]), a[3] = {axis[0] / n, axis[1] / n, axis[2] / n};
  const double K[9] = {0.0, -a[2], a[1], a[2], 0.0, -a[0], -a[1], a[0], 0.0};
  const double th = deg * M_PI / 180.0, s = std::sin(th), c1 = 1.0 - std::cos(th);
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) {
      double kk = 0.0;
      for (int j = 0; j < 3; j++) kk += K[3 * r + j] * K[3 * j + c];
      R[3 * r + c] = (float)((r == c ? 1.0 : 0.0) + s * K[3 * r + c] + c1 * kk);
    }
}

struct HostBox {
  float tr[3], half[3];
};
static HostBox make_box(const double* sizes, const double* trans) {
  HostBox b;
  for (int i = 0; i < 3; i++) b.tr[i] = (float)trans[i], b.half[i] = (float)(sizes[i] / 2);   // aabb.py:15-25
  return b;
}
static bool ref_inside(const HostBox& box, const float* p) {   // aabb.py:28-42
  int valid = 0;
  for (int k = 0; k < 3; k++) {
    const float q = p[k] - box.tr[k];
    valid += (q < box.half[k] && q > -box.half[k]) ? 1 : 0;
  }
  return valid == 3;
}

// visualize_sdf_isolines.py:77-92 for cell (ix, iy)
static void ref_point(int S, int ix, int iy, const float* A, float z, float extent_scale, float* out) {
  float x_coord = (float)ix, y_coord = (float)iy;
  x_coord = x_coord / (float)S - 0.5f;
  y_coord = y_coord / (float)S - 0.5f;
  x_coord = x_coord * 2.0f;
  y_coord = y_coord * 2.0f;
  x_coord = x_coord * extent_scale;
  y_coord = y_coord * extent_scale;
  const double V[3] = {(double)x_coord, (double)y_coord, (double)z};
  for (int c = 0; c < 3; c++) {
    const double xa = V[0] * (double)A[3 * c], ya = V[1] * (double)A[3 * c + 1], za = V[2] * (double)A[3 * c + 2];
    const double sum = xa + ya;
    out[c] = (float)(sum + za);
  }
}

static void check_points(int S, long first, int count, int P, float extent_scale, const char* label) {
  const double axis[3] = {1.0, 2.0, 3.0}, sizes[3] = {0.9, 1.2, 0.7}, trans[3] = {0.05, -0.1, 0.02};
  float A[9];
  rotation(axis, 50.0, A);
  const HostBox box = make_box(sizes, trans);
  const float z = -0.057f, time_val = 0.37f;
  Guarded<float> pts((size_t)P * count, CANARY);
  Guarded<unsigned char> skip(count, BCANARY);
  const int status = psdf_slice_points(S, first, count, P, A, z, extent_scale, box.tr, box.half, P == 4 ? &time_val : nullptr,
                                       pts.data(), skip.data(), nullptr);
  if (status != 0) return fail(label, status, S);
  int inside = 0;
  for (int i = 0; i < count; i++) {
    const long k = first + i;
    float want[3];
    ref_point(S, (int)(k % S), (int)(k / S), A, z, extent_scale, want);
    for (int c = 0; c < 3; c++)
      if (!same_bits(pts[(size_t)P * i + c], want[c])) fail("points: a coordinate differs in bits", k, c);
    if (P == 4 && !same_bits(pts[(size_t)P * i + 3], time_val)) fail("points: column 3 is not the time", k);
    const bool in = ref_inside(box, want);
    inside += in;
    if (skip[i] != (in ? 0 : 1)) fail("points: a flag differs", k);
  }
  if (!pts.intact() || !skip.intact()) fail("points: a canary was written", S, P);
  if (count > 1000 && (inside < count / 16 || count - inside < count / 16)) fail("points: cells inside and outside are not both there", inside);
  printf("%-12s points   S = %2d, cells [%ld, %ld), rows of %d, extent %.2f: %d inside, %d outside: ok\n", label, S, first,
         first + count, P, (double)extent_scale, inside, count - inside);
}

// ---------------------------------------------------------------------------------------------------- colours
static const double PUBU[9][3] = {{255, 247, 251}, {236, 231, 242}, {208, 209, 230}, {166, 189, 219}, {116, 169, 207},
                                  {54, 144, 192},  {5, 112, 176},   {4, 90, 141},    {2, 56, 88}};

struct Style {
  vector<float> table;      // [K, 3]
  int K;
  float base[4];            // in_lo, in_hi, out_lo, scale
  double line[4];           // in_lo, in_hi, out_lo, out_hi
  int n;
  vector<float> lo, hi, rgb;
};

static void lookup64(const Style& st, double t, double* out) {
  t = std::min(std::max(t, 0.0), 1.0);
  const double u = t * (st.K - 1);
  const int j = std::min((int)u, st.K - 2);
  for (int c = 0; c < 3; c++) {
    const double a = st.table[3 * j + c], b = st.table[3 * j + 3 + c];
    out[c] = a + (u - j) * (b - a);
  }
}

static Style make_style(const vector<float>& table, double width, double distance, int n) {
  Style st;
  st.table = table, st.K = (int)table.size() / 3, st.n = n;
  const double base[4] = {0.0, 0.3, 0.2, 1.0}, line[4] = {0.0, 0.2, 0.3, 1.0};
  st.base[0] = (float)base[0], st.base[1] = (float)base[1], st.base[2] = (float)base[2];
  st.base[3] = (float)((base[3] - base[2]) / (base[1] - base[0]));
  for (int k = 0; k < 4; k++) st.line[k] = line[k];
  for (int i = 0; i < n; i++) {
    const double centre = i * distance;
    st.lo.push_back((float)(centre - width / 2));
    st.hi.push_back((float)(centre + width / 2));
    const double clamped = std::min(std::max(centre, line[0]), line[1]);
    double c[3];
    lookup64(st, line[2] + ((line[3] - line[2]) / (line[1] - line[0])) * (clamped - line[0]), c);
    for (int k = 0; k < 3; k++) st.rgb.push_back((float)c[k]);
  }
  return st;
}

static vector<float> pubu_table() {
  vector<float> t;
  for (int j = 0; j < 9; j++)
    for (int c = 0; c < 3; c++) t.push_back((float)(PUBU[j][c] / 255.0));
  return t;
}

// float64 base colour of s (not a NaN) and its bar per channel
static void base64(const Style& st, float s, double* colour, double* bar) {
  const double in_lo = st.base[0], in_hi = st.base[1], out_lo = st.base[2], scale = st.base[3];
  const double c = std::min(std::max((double)s, in_lo), in_hi);
  const double t = out_lo + scale * (c - in_lo), T = std::fabs(out_lo) + std::fabs(scale * (c - in_lo));
  lookup64(st, t, colour);
  for (int ch = 0; ch < 3; ch++) {
    double D = 0.0, M = 0.0;
    for (int j = 0; j < st.K; j++) {
      M = std::max(M, std::fabs((double)st.table[3 * j + ch]));
      if (j + 1 < st.K) D = std::max(D, std::fabs((double)st.table[3 * j + 3 + ch] - (double)st.table[3 * j + ch]));
    }
    bar[ch] = U * (4.0 * T * (st.K - 1) * D + 2.0 * D + 2.0 * M);
  }
}

static int expected_band(const Style& st, float s) {
  int band = -1;
  for (int i = 0; i < st.n; i++)
    if (s > st.lo[i] && s < st.hi[i]) band = i;
  return band;
}

// run colorize over `values` laid out as the cells [first, first + n) of an S x S layer and check every plane
static void check_colorize(const Style& st, const vector<float>& values, const vector<unsigned char>& skipped, int S, long first,
                           int edges, const char* label) {
  const int n = (int)values.size();
  const long cells = (long)S * S;
  vector<float> rgb(3 * cells, CANARY), sdf_img(cells, CANARY), in_img(cells, CANARY);
  const int status = psdf_slice_colorize(S, first, n, values.data(), skipped.data(), st.table.data(), st.K, st.base, st.n,
                                         st.lo.data(), st.hi.data(), st.rgb.data(), rgb.data(), sdf_img.data(), in_img.data(), nullptr);
  if (status != 0) return fail(label, status);
  int in_band = 0, nans = 0, skips = 0, near = 0, bounds_outside = 0;
  for (long k = 0; k < cells; k++) {
    const bool in_range = k >= first && k < first + n;
    if (!in_range) {
      if (rgb[k] != CANARY || rgb[cells + k] != CANARY || rgb[2 * cells + k] != CANARY || sdf_img[k] != CANARY || in_img[k] != CANARY)
        fail("colorize: a cell outside the range was written", k);
      continue;
    }
    const int i = (int)(k - first);
    const float s = values[i];
    const float got[3] = {rgb[k], rgb[cells + k], rgb[2 * cells + k]};
    if (skipped[i]) {
      skips++;
      if (!same_bits(got[0], 0.f) || !same_bits(got[1], 0.f) || !same_bits(got[2], 0.f) || !same_bits(sdf_img[k], 0.f) || !same_bits(in_img[k], 0.f))
        fail("colorize: a skipped cell is not 0 in all three planes", k);
      continue;
    }
    if (!same_bits(sdf_img[k], s) || !same_bits(in_img[k], 1.f)) fail("colorize: the sdf or the inside plane differs", k);
    if (s != s) {
      nans++;
      if (!same_bits(got[0], 0.f) || !same_bits(got[1], 0.f) || !same_bits(got[2], 0.f)) fail("colorize: a NaN has a colour", k);
      continue;
    }
    const int band = expected_band(st, s);
    if (band >= 0) {
      in_band++;
      for (int c = 0; c < 3; c++)
        if (!same_bits(got[c], st.rgb[3 * band + c])) fail("colorize: a cell in a band does not hold the band's colour", k, band);
      continue;
    }
    double want[3], bar[3];
    base64(st, s, want, bar);
    for (int c = 0; c < 3; c++) {
      const double err = std::fabs((double)got[c] - want[c]);
      worst_colour = std::max(worst_colour, err / bar[c]);
      if (!(err <= bar[c])) fail("colorize: a base colour misses its bar", k, c);
    }
    // the value sits on or next to a band's bound: the band's colour must be far from the base colour there.  (From 0.3 on both
    // maps have reached the end of the table: the two colours agree and a decision cannot be seen; the bounds below 0.29 can.)
    if (i < edges && s < 0.29f) {
      int nearest = 0;
      for (int b = 0; b < st.n; b++)
        if (std::fabs((double)s - 0.5 * ((double)st.lo[b] + st.hi[b])) < std::fabs((double)s - 0.5 * ((double)st.lo[nearest] + st.hi[nearest]))) nearest = b;
      double gap = 0.0, b10 = 0.0;
      for (int c = 0; c < 3; c++) gap = std::max(gap, std::fabs(want[c] - (double)st.rgb[3 * nearest + c])), b10 = std::max(b10, 10.0 * bar[c]);
      bounds_outside++;
      near += !(gap > b10);
    }
  }
  printf("%-12s colorize S = %2d, cells [%ld, %ld), K = %d, %d lines: %d in a band, %d NaN, %d skipped%s: ok\n", label, S, first, first + n,
         st.K, st.n, in_band, nans, skips, edges ? ", bounds" : "");
  if (edges && (near > 0 || bounds_outside < 2)) fail("bands: the base colour at the bounds does not tell a wrong decision apart", near, bounds_outside);
}

static void check_bands(double width, double distance, int n, const char* label) {
  const Style st = make_style(pubu_table(), width, distance, n);
  vector<float> v;
  const float inf = std::numeric_limits<float>::infinity();
  for (int i = 0; i < n; i++)
    for (float b : {st.lo[i], st.hi[i]}) {
      v.push_back(b);
      v.push_back(std::nextafterf(b, -inf));
      v.push_back(std::nextafterf(b, inf));
    }
  // the decisions at the bounds themselves, stated outright
  for (int i = 0; i < n; i++) {
    if (expected_band(st, st.lo[i]) == i || expected_band(st, st.hi[i]) == i) fail("bands: a bound is in its own band", i);
    if (expected_band(st, std::nextafterf(st.lo[i], inf)) < i) fail("bands: one float above lo is in no band from i on", i);
  }
  if (width > distance) {   // the centre of band i also lies in band i + 1 when width / 2 > distance: the later band wins
    int later = 0;
    for (int i = 0; i + 1 < n; i++) {
      const float s = (float)(i * distance + 0.75 * distance);      // inside bands i and i + 1
      if (s > st.lo[i] && s < st.hi[i] && s > st.lo[i + 1] && s < st.hi[i + 1]) later += expected_band(st, s) >= i + 1;
      v.push_back(s);
    }
    if (later < n - 2) fail("bands: the overlapping inputs do not overlap", later);
  }
  for (float s : {-0.5f, -0.01f, -1e-30f, 0.31f, 0.45f, 7.0f, -inf, inf}) v.push_back(s);
  v.push_back(std::numeric_limits<float>::quiet_NaN());
  vector<unsigned char> skipped(v.size(), 0);
  for (int k = 0; k < 6; k++) {      // skipped cells: a value in a band, a NaN, an ordinary value
    v.push_back(k % 3 == 0 ? (float)(distance) : (k % 3 == 1 ? std::numeric_limits<float>::quiet_NaN() : 0.1f));
    skipped.push_back(1);
  }
  const int S = (int)std::ceil(std::sqrt((double)v.size() + 3.0));
  check_colorize(st, v, skipped, S, 3, 6 * n, label);
}

static void check_colours(const vector<float>& table, int count, const char* label) {
  const Style st = make_style(table, 0.005, 0.03, 15);
  vector<float> v(count);
  vector<unsigned char> skipped(count, 0);
  for (int i = 0; i < count; i++) v[i] = -0.1f + 0.6f * uni();
  for (int i = 0; i < count; i += 97) skipped[i] = 1;
  const int S = (int)std::ceil(std::sqrt((double)count));
  check_colorize(st, v, skipped, S, 0, 0, label);
}

// ---------------------------------------------------------------------------------------------------- the cut
struct Scene {
  int H = 41, W = 53;
  float K[9], T[16], A[9];
  float z = 0.05f, extent = 0.45f, radius = 0.3f;
  HostBox box;
};
static Scene make_scene() {
  Scene sc;
  const float K[9] = {40.f, 0.f, 26.5f, 0.f, 40.f, 20.5f, 0.f, 0.f, 1.f};
  std::memcpy(sc.K, K, sizeof K);
  const double cam_axis[3] = {1.0, 2.0, 3.0}, plane_axis[3] = {0.1, 1.0, 0.05};
  float R[9];
  rotation(cam_axis, 12.0, R);
  const float t[3] = {0.15f, -0.1f, -1.4f};
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) sc.T[4 * r + c] = R[3 * r + c];
    sc.T[4 * r + 3] = t[r];
  }
  sc.T[12] = sc.T[13] = sc.T[14] = 0.f, sc.T[15] = 1.f;
  rotation(plane_axis, 65.0, sc.A);
  const double sizes[3] = {1.0, 1.0, 0.8}, trans[3] = {0.02, -0.03, 0.05};
  sc.box = make_box(sizes, trans);
  return sc;
}

struct Decision {
  bool checked, take;
  double t, p[3], errt, errp[3], Dn;
  bool in_front, in_box, in_layer, surface;
};

static Decision decide64(const Scene& sc, const float* o, const float* d, float weight, float depth) {
  Decision r{};
  const double z = sc.z, ext = sc.extent;
  double n[3], a0[3], a1[3];
  for (int i = 0; i < 3; i++) a0[i] = sc.A[3 * i], a1[i] = sc.A[3 * i + 1], n[i] = sc.A[3 * i + 2];
  double N = 0, Dn = 0, sN = 0, sD = 0;
  for (int i = 0; i < 3; i++) {
    N += n[i] * (z * n[i] - o[i]);
    Dn += n[i] * d[i];
    sN += std::fabs(n[i]) * (std::fabs(z * n[i]) + std::fabs((double)o[i]));
    sD += std::fabs(n[i] * d[i]);
  }
  const double errN = 5 * U * sN, errD = 3 * U * sD;
  r.Dn = Dn;
  r.surface = weight != 0.f;
  if (!(std::fabs(Dn) > 2 * errD)) return r;      // not checked
  const double t = N / Dn;
  const double errt = (errN + std::fabs(t) * errD) / (std::fabs(Dn) - errD) + U * std::fabs(t);
  r.t = t, r.errt = errt;
  bool ok = std::fabs(t) > errt;
  double u = 0, v = 0, erru = 0, errv = 0, su = 0, sv = 0;
  bool in_box = true;
  for (int i = 0; i < 3; i++) {
    r.p[i] = o[i] + t * d[i];
    r.errp[i] = std::fabs((double)d[i]) * errt + U * std::fabs(t * d[i]) + U * std::fabs(r.p[i]);
    u += a0[i] * r.p[i], v += a1[i] * r.p[i];
    erru += std::fabs(a0[i]) * r.errp[i], errv += std::fabs(a1[i]) * r.errp[i];
    su += std::fabs(a0[i] * r.p[i]), sv += std::fabs(a1[i] * r.p[i]);
    const double q = r.p[i] - sc.box.tr[i], errq = r.errp[i] + U * std::fabs(q);
    ok = ok && std::fabs(std::fabs(q) - sc.box.half[i]) > errq;
    in_box = in_box && q < sc.box.half[i] && q > -(double)sc.box.half[i];
  }
  erru += 3 * U * su, errv += 3 * U * sv;
  ok = ok && std::fabs(u + ext) > erru && std::fabs(u - ext) > erru && std::fabs(v + ext) > errv && std::fabs(v - ext) > errv;
  if (r.surface) ok = ok && std::fabs(t - (double)depth) > errt;
  r.checked = ok;
  r.in_front = t > 0;
  r.in_box = in_box;
  r.in_layer = u >= -ext && u < ext && v >= -ext && v < ext;
  r.take = t > 0 && u >= -ext && u < ext && v >= -ext && v < ext && in_box && (!r.surface || t < (double)depth);
  return r;
}

static void check_cut(int P, long first, int R, const char* label) {
  const Scene sc = make_scene();
  const long HW = (long)sc.H * sc.W;
  vector<float> o_all(3 * HW), d_all(3 * HW);
  if (psdf_frame_rays(sc.H, sc.W, sc.K, sc.T, 0, (int)HW, o_all.data(), d_all.data(), nullptr) != 0) return fail("the rays");
  // the base planes: the analytic depth and coverage of a sphere about the origin, in float64, rounded
  vector<float> weights(HW), depth(HW), rgb(3 * HW);
  for (long p = 0; p < HW; p++) {
    const float *o = &o_all[3 * p], *d = &d_all[3 * p];
    double b = 0, c = -(double)sc.radius * sc.radius;
    for (int i = 0; i < 3; i++) b += (double)o[i] * d[i], c += (double)o[i] * o[i];
    const double disc = b * b - c, t = -b - std::sqrt(std::max(disc, 0.0));
    const bool hit = disc > 0 && t > 0;
    weights[p] = hit ? 1.f : 0.f, depth[p] = hit ? (float)t : 0.f;
    for (int ch = 0; ch < 3; ch++) rgb[ch * HW + p] = 0.25f + 0.125f * ch + (float)(p % 7) * 0.0625f;
  }
  // the cap on the float64 geometry alone, and the rays that must be there
  int unchecked = 0, grazing = 0, behind = 0, miss_box = 0, over_sphere = 0, under_sphere = 0, no_surface = 0;
  vector<Decision> dec(HW);
  for (long p = 0; p < HW; p++) {
    dec[p] = decide64(sc, &o_all[3 * p], &d_all[3 * p], weights[p], depth[p]);
    const Decision& r = dec[p];
    unchecked += !r.checked;
    grazing += std::fabs(r.Dn) < 0.02;
    if (!r.checked) continue;
    behind += !r.in_front;
    miss_box += r.in_front && !r.in_box;
    over_sphere += r.take && r.surface;
    under_sphere += !r.take && r.surface && r.in_front && r.in_box && r.in_layer;
    no_surface += r.take && !r.surface;
  }
  if (first == 0 && R == HW) {
    printf("%-12s cut      float64 geometry: %d of %ld rays unchecked (cap %ld), %d grazing, %d behind the camera, %d miss the box, "
           "%d slice over sphere, %d sphere over slice, %d slice on no surface\n", label, unchecked, HW, HW / 100, grazing, behind, miss_box,
           over_sphere, under_sphere, no_surface);
    if (unchecked * 100 > HW) fail("cut: more than 1 % of the rays are excluded by the float64 geometry", unchecked);
    if (grazing < 20 || behind < 10 || miss_box < 10 || over_sphere < 10 || under_sphere < 10 || no_surface < 10)
      fail("cut: the frame does not hold every kind of ray", grazing, behind);
  }
  // begin
  const float time_val = 0.61f;
  Guarded<float> pts((size_t)P * R, CANARY), t_out(R, CANARY);
  Guarded<unsigned char> skip(R, BCANARY);
  int status = psdf_slice_cut_begin(R, P, sc.A, sc.z, sc.extent, sc.box.tr, sc.box.half, &o_all[3 * first], &d_all[3 * first],
                                    P == 4 ? &time_val : nullptr, sc.H, sc.W, first, weights.data(), depth.data(), pts.data(), skip.data(),
                                    t_out.data(), nullptr);
  if (status != 0) return fail(label, status);
  int taken = 0;
  for (int i = 0; i < R; i++) {
    const Decision& r = dec[first + i];
    if (skip[i] > 1) fail("begin: a flag is no 0 / 1", i);
    if (P == 4 && !same_bits(pts[(size_t)P * i + 3], time_val)) fail("begin: column 3 is not the time", i);
    if (skip[i]) {
      for (int c = 0; c < 3; c++)
        if (!same_bits(pts[(size_t)P * i + c], o_all[3 * (first + i) + c])) fail("begin: a ray that does not take part left its origin", i, c);
      if (!same_bits(t_out[i], 0.f)) fail("begin: a ray that does not take part has a t", i);
    }
    if (!r.checked) continue;
    if ((skip[i] == 0) != r.take) fail("begin: a decision differs from float64", first + i, r.take);
    if (skip[i] || !r.take) continue;
    taken++;
    worst_t = std::max(worst_t, std::fabs((double)t_out[i] - r.t) / r.errt);
    if (!(std::fabs((double)t_out[i] - r.t) <= r.errt)) fail("begin: t misses its bar", first + i);
    for (int c = 0; c < 3; c++) {
      const double err = std::fabs((double)pts[(size_t)P * i + c] - r.p[c]);
      worst_point = std::max(worst_point, err / r.errp[c]);
      if (!(err <= r.errp[c])) fail("begin: a point misses its bar", first + i, c);
    }
  }
  if (!pts.intact() || !t_out.intact() || !skip.intact()) fail("begin: a canary was written", R, P);
  // resolve, with SDF values of every kind; against the colorize entry on the same values
  const Style st = make_style(pubu_table(), 0.005, 0.03, 15);
  vector<float> sdf(R);
  for (int i = 0; i < R; i++) sdf[i] = i % 11 == 0 ? std::numeric_limits<float>::quiet_NaN() : (i % 5 == 0 ? 0.03f * (float)(i % 15) : -0.1f + 0.6f * uni());
  vector<unsigned char> flags(R);
  for (int i = 0; i < R; i++) flags[i] = skip[i];
  const int S = (int)std::ceil(std::sqrt((double)R));
  vector<float> c_rgb(3 * (size_t)S * S, 0.f), c_sdf((size_t)S * S, 0.f), c_in((size_t)S * S, 0.f);
  status = psdf_slice_colorize(S, 0, R, sdf.data(), flags.data(), st.table.data(), st.K, st.base, st.n, st.lo.data(), st.hi.data(),
                               st.rgb.data(), c_rgb.data(), c_sdf.data(), c_in.data(), nullptr);
  if (status != 0) return fail(label, status);
  vector<float> rgb0 = rgb, depth0 = depth, weights0 = weights, mask(HW, CANARY);
  status = psdf_slice_cut_resolve(R, sdf.data(), flags.data(), &t_out[0], st.table.data(), st.K, st.base, st.n, st.lo.data(),
                                  st.hi.data(), st.rgb.data(), sc.H, sc.W, first, rgb.data(), depth.data(), weights.data(), mask.data(), nullptr);
  if (status != 0) return fail(label, status);
  for (long p = 0; p < HW; p++) {
    const bool in_chunk = p >= first && p < first + R;
    const bool sliced = in_chunk && !flags[p - first];
    if (!in_chunk && mask[p] != CANARY) fail("resolve: the mask outside the chunk was written", p);
    if (in_chunk && !same_bits(mask[p], sliced ? 1.f : 0.f)) fail("resolve: the mask differs", p);
    if (!sliced) {
      bool kept = same_bits(depth[p], depth0[p]) && same_bits(weights[p], weights0[p]);
      for (int ch = 0; ch < 3; ch++) kept = kept && same_bits(rgb[ch * HW + p], rgb0[ch * HW + p]);
      if (!kept) fail("resolve: a pixel without the slice changed", p);
      continue;
    }
    const int i = (int)(p - first);
    if (!same_bits(depth[p], t_out[i]) || !same_bits(weights[p], 1.f)) fail("resolve: depth / weight of a slice pixel are not t / 1", p);
    for (int ch = 0; ch < 3; ch++)
      if (!same_bits(rgb[ch * HW + p], c_rgb[(size_t)ch * S * S + i])) fail("resolve: a colour differs from colorize's", p, ch);
  }
  printf("%-12s cut      rows of %d, pixels [%ld, %ld): %d rays take part: ok\n", label, P, first, first + R, taken);
}

static void check_refusals() {
  float f[128] = {0};
  unsigned char b[8] = {0};
  const float tri[3] = {0.5f, 0.5f, 0.5f}, A[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, base[4] = {0.f, 0.3f, 0.2f, 2.6666667f};
  const vector<float> table = pubu_table();
  const float* tb = table.data();
  // empty ranges return before any check
  if (psdf_slice_points(0, 0, 0, 7, nullptr, 0.f, 1.f, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != 0) fail("empty points");
  if (psdf_slice_colorize(0, 0, 0, nullptr, nullptr, nullptr, 0, nullptr, 99, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != 0) fail("empty colorize");
  if (psdf_slice_cut_begin(0, 7, nullptr, 0.f, 1.f, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != 0) fail("empty begin");
  if (psdf_slice_cut_resolve(0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 99, nullptr, nullptr, nullptr, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr) != 0) fail("empty resolve");
  auto points = [&](int S, long first, int count, int stride, const float* time, float* pts) {
    return psdf_slice_points(S, first, count, stride, A, 0.f, 1.f, tri, tri, time, pts, b, nullptr);
  };
  if (points(4, 0, 4, 3, nullptr, f) != 0) fail("a plain call is refused (points)");
  if (points(4, 0, -1, 3, nullptr, f) != -1) fail("a negative count is accepted (points)");
  if (points(4, 0, 4, 5, f, f) != -1 || points(4, 0, 4, 2, f, f) != -1) fail("rows of 5 or 2 are accepted (points)");
  if (points(4, 0, 4, 4, nullptr, f) != -1) fail("rows of 4 without a time are accepted (points)");
  if (points(4, 13, 4, 3, nullptr, f) != -1 || points(4, -1, 4, 3, nullptr, f) != -1) fail("a range outside the layer is accepted");
  if (points(0, 0, 4, 3, nullptr, f) != -1) fail("S = 0 is accepted");
  if (points(4, 0, 4, 3, nullptr, nullptr) != -1) fail("NULL points are accepted");
  if (points(46341, 0, 4, 3, nullptr, f) != -2) fail("a layer of 2^31 cells is accepted");
  if (points(46340, 0, 4, 3, nullptr, f) != 0) fail("the largest layer is refused");
  auto colorize = [&](int S, long first, int count, int K, int lines, const float* lo) {
    return psdf_slice_colorize(S, first, count, f, b, tb, K, base, lines, lo, f, f, f, f, f, nullptr);
  };
  if (colorize(4, 0, 4, 9, 15, f) != 0) fail("a plain call is refused (colorize)");
  if (colorize(4, 0, 4, 9, 33, f) != -1 || colorize(4, 0, 4, 9, -1, f) != -1) fail("33 or -1 lines are accepted");
  if (colorize(4, 0, 4, 9, 32, f) != 0 || colorize(4, 0, 4, 9, 0, nullptr) != 0) fail("32 or 0 lines are refused");
  if (colorize(4, 0, 4, 1, 15, f) != -1) fail("a table of one control point is accepted");
  if (colorize(4, 0, 4, 9, 15, nullptr) != -1) fail("NULL bands are accepted");
  if (colorize(4, 14, 4, 9, 15, f) != -1) fail("a range outside the layer is accepted (colorize)");
  if (colorize(65536, 0, 4, 9, 15, f) != -2) fail("a layer of 2^32 cells is accepted (colorize)");
  auto begin = [&](int R, int stride, int H, int W, long first, const float* time) {
    return psdf_slice_cut_begin(R, stride, A, 0.f, 1.f, tri, tri, f, f, time, H, W, first, f, f, f, b, f, nullptr);
  };
  if (begin(2, 3, 2, 3, 4, nullptr) != 0 || begin(2, 4, 2, 3, 0, f) != 0) fail("a plain call is refused (begin)");
  if (begin(-2, 3, 2, 3, 0, nullptr) != -1 || begin(2, 6, 2, 3, 0, f) != -1 || begin(2, 4, 2, 3, 0, nullptr) != -1) fail("bad arguments are accepted (begin)");
  if (begin(2, 3, 2, 3, 5, nullptr) != -1 || begin(2, 3, 0, 3, 0, nullptr) != -1) fail("a range outside the frame is accepted (begin)");
  if (begin(2, 3, 65536, 32768, 0, nullptr) != -2) fail("a frame of 2^31 pixels is accepted (begin)");
  auto resolve = [&](int R, int H, int W, long first, int K, int lines, float* mask) {
    return psdf_slice_cut_resolve(R, f, b, f, tb, K, base, lines, f, f, f, H, W, first, f, f, f, mask, nullptr);
  };
  b[0] = b[1] = 1;   // (both rays skipped: only the mask is written)
  if (resolve(2, 2, 3, 4, 9, 15, f + 8) != 0) fail("a plain call is refused (resolve)");
  if (resolve(2, 2, 3, 5, 9, 15, f) != -1 || resolve(2, 2, 3, 0, 9, 40, f) != -1 || resolve(2, 2, 3, 0, 0, 15, f) != -1) fail("bad arguments are accepted (resolve)");
  if (resolve(2, 2, 3, 0, 9, 15, nullptr) != -1) fail("a NULL mask is accepted");
  if (resolve(2, 65536, 32768, 0, 9, 15, f) != -2) fail("a frame of 2^31 pixels is accepted (resolve)");
}

int main() {
  for (int P = 3; P <= 4; P++) {
    check_points(1, 0, 1, P, 1.0f, "layer");
    check_points(2, 0, 4, P, 1.0f, "layer");
    check_points(37, 0, 37 * 37, P, 1.0f, "layer");
    check_points(37, 5, 37 * 37 - 7, P, 1.0f, "mid-row");
    check_points(37, 5, 37 * 37 - 7, P, 0.45f, "mid-row");
  }
  check_points(37, 37 * 37 - 1, 1, 3, 1.0f, "last cell");
  check_bands(0.005, 0.03, 15, "defaults");
  check_bands(0.05, 0.03, 15, "overlapping");
  check_bands(0.004, 0.011, 32, "32 lines");
  check_colours(pubu_table(), 4001, "PuBu");
  check_colours({0.9f, 0.1f, 0.5f, 0.0f, 1.0f, 0.5f}, 1000, "K = 2");
  {
    vector<float> t;
    for (int i = 0; i < 3 * 5; i++) t.push_back(uni());
    check_colours(t, 1000, "K = 5");
  }
  const long HW = 41 * 53;
  check_cut(3, 0, (int)HW, "whole frame");
  check_cut(4, 0, (int)HW, "whole frame");
  check_cut(3, 1024, 1024, "a chunk");
  check_cut(4, 2048, (int)(HW - 2048), "last chunk");
  check_refusals();
  printf("worst error / bar: colour %.3f, cut point %.3f, cut t %.3f\n", worst_colour, worst_point, worst_t);
  if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
  else printf("sdf_slice_kernels_check: all checks passed\n");
  return failures ? 1 : 0;
}
