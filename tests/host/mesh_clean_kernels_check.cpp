// Stand-alone check of the kernels of permuto_sdf_amd/csrc/mesh_clean.hip on the CPU: the file itself is compiled as C++ against
// tests/host/hip_on_host/hip/hip_runtime.h (launches run on CPU threads, concurrently: the kernels ballot, and the union-find is
// meant to be raced), driven the way permuto_sdf_amd/mesh_clean.py drives it and compared with brute force.
// tests/test_mesh_clean_host.py builds it with -fsanitize=address,undefined -fno-sanitize-recover=all and runs it under a time
// limit: an index out of bounds in a kernel is a sanitizer report here, a union-find that does not end is a timeout here, neither
// a fault nor a hang on a device.  It says nothing about speed, and nothing about what the device compiler makes of the source.
#include <hip/hip_runtime.h>

// what the stand-in lacks
#define __builtin_amdgcn_readfirstlane(v) (v)
inline int atomicCAS(int32_t* p, int expected, int desired) {
  __atomic_compare_exchange_n(p, &expected, desired, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED);
  return expected;
}
inline int atomicMin(int32_t* p, int v) {
  int old = __atomic_load_n(p, __ATOMIC_RELAXED);
  while (old > v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {
  }
  return old;
}

#include <cstdio>
#include <map>
#include <numeric>
#include <random>

#include "mesh_clean.hip"

using std::vector;

static std::mt19937 rng(11);
static int uniform_int(int a, int b) { return std::uniform_int_distribution<int>(a, b)(rng); }
static double uniform(double a, double b) { return std::uniform_real_distribution<double>(a, b)(rng); }
static int failures = 0;

static void must(int status, const char* what) {
  if (status != 0) {
    fprintf(stderr, "%s returned %d\n", what, status);
    exit(2);
  }
}

static vector<int> ellipse(int ksize) {
  vector<int> hw(ksize, 0);
  const int r = ksize / 2;
  for (int i = 0; i < ksize && r > 0; i++) hw[i] = (int)std::nearbyint(r * std::sqrt((double)(r * r - (i - r) * (i - r)) / (r * r)));
  return hw;
}

// ---- dilation ---------------------------------------------------------------------------------------------------------------
static void check_dilation(const char* label, int n, int H, int W, const vector<uint8_t>& src, int threshold, const vector<int>& hw) {
  const int ww = (W + 31) / 32, r = (int)hw.size() / 2;
  vector<uint8_t> hd((size_t)n * H * W + 1, 0x5a);       // one guard byte
  vector<int32_t> words((size_t)n * H * ww + 1, 0x5a5a5a5a);
  hip_on_host::concurrent = true;
  must(psdf_mesh_clean_row_distance(src.data(), n, H, W, threshold, hd.data(), nullptr), "row_distance");
  must(psdf_mesh_clean_dilate(hd.data(), n, H, W, hw.data(), (int)hw.size(), words.data(), nullptr), "dilate");
  hip_on_host::concurrent = false;
  int bad_hd = 0, bad = 0;
  for (int v = 0; v < n; v++)
    for (int y = 0; y < H; y++) {
      const uint8_t* row = &src[((size_t)v * H + y) * W];
      for (int x = 0; x < W; x++) {
        int d = 255;
        for (int k = 0; k < 255; k++)
          if ((x - k >= 0 && row[x - k] > threshold) || (x + k < W && row[x + k] > threshold)) {
            d = k;
            break;
          }
        bad_hd += hd[((size_t)v * H + y) * W + x] != d;
      }
      for (int x = 0; x < ww * 32; x++) {
        bool want = false;
        for (int k = 0; k <= 2 * r && x < W && !want; k++) {
          const int yy = y + k - r;
          if (yy < 0 || yy >= H) continue;
          const uint8_t* other = &src[((size_t)v * H + yy) * W];
          for (int xx = std::max(0, x - hw[k]); xx <= std::min(W - 1, x + hw[k]) && !want; xx++) want = other[xx] > threshold;
        }
        const bool got = ((uint32_t)words[((size_t)v * H + y) * ww + (x >> 5)] >> (x & 31)) & 1;
        bad += got != want;
      }
    }
  bad += hd.back() != 0x5a || words.back() != 0x5a5a5a5a;
  printf("dilation %-28s %d x %3d x %3d, %3zu rows: %d distances wrong, %d bits wrong\n", label, n, H, W, hw.size(), bad_hd, bad);
  failures += bad + bad_hd;
}

static vector<uint8_t> sparse_masks(int n, int H, int W, double density) {
  vector<uint8_t> m((size_t)n * H * W, 0);
  for (auto& p : m) p = uniform(0, 1) < density ? 255 : uniform_int(0, 128);
  for (int v = 0; v < n; v++) {   // the four corners
    uint8_t* img = &m[(size_t)v * H * W];
    img[0] = img[W - 1] = img[(size_t)(H - 1) * W] = img[(size_t)H * W - 1] = 129;
  }
  return m;
}

// ---- vertex test ------------------------------------------------------------------------------------------------------------
static void check_vertex_test(int nV) {
  const int n = 5, H = 40, W = 70, ww = (W + 31) / 32;
  vector<int32_t> words((size_t)n * H * ww);
  for (auto& w : words) w = (int32_t)rng();
  vector<double> mats(12 * n);
  for (int v = 0; v < n; v++) {   // pinholes on a circle looking at the origin from distance 2.5 (focal 60 px)
    const double a = 1.3 * v, c = std::cos(a), s = std::sin(a);
    const double R[9] = {c, 0, -s, 0, 1, 0, s, 0, c}, t[3] = {0, 0, 2.5}, K[9] = {60, 0, W / 2.0, 0, 60, H / 2.0, 0, 0, 1};
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 4; j++) {
        double acc = 0;
        for (int k = 0; k < 3; k++) acc += K[3 * i + k] * (j < 3 ? R[3 * k + j] : t[k]);
        mats[12 * v + 4 * i + j] = acc;
      }
  }
  vector<float> V(3 * (size_t)nV + 3);
  for (auto& c : V) c = (float)uniform(-1, 1);
  if (nV > 8) {
    V[0] = NAN, V[3] = 1e30f, V[7] = INFINITY;
    V[9] = 0, V[10] = 0, V[11] = -2.5f;   // p2 == 0 in view 0
    V[12] = 0, V[13] = 0, V[14] = -9.f;   // behind view 0
  }
  vector<uint8_t> keep(nV + 1, 0x5a);
  hip_on_host::concurrent = true;
  must(psdf_mesh_clean_inside_masks(V.data(), nV, mats.data(), n, words.data(), H, W, keep.data(), nullptr), "inside_masks");
  hip_on_host::concurrent = false;
  int bad = 0, kept = 0;
  for (int i = 0; i < nV; i++) {
    bool want = true;
    const double x = V[3 * i], y = V[3 * i + 1], z = V[3 * i + 2];
    for (int v = 0; v < n; v++) {
      const double* P = &mats[12 * v];
      const double p0 = ((P[0] * x + P[1] * y) + P[2] * z) + P[3], p1 = ((P[4] * x + P[5] * y) + P[6] * z) + P[7];
      const double p2 = ((P[8] * x + P[9] * y) + P[10] * z) + P[11];
      const double u = p0 / p2, w = p1 / p2;
      if (!std::isfinite(u) || !std::isfinite(w)) continue;
      const double ru = std::nearbyint(u), rv = std::nearbyint(w);
      if (ru < 0 || ru >= W || rv < 0 || rv >= H) continue;
      want = want && (((uint32_t)words[((size_t)v * H + (int)rv) * ww + ((int)ru >> 5)] >> ((int)ru & 31)) & 1);
    }
    bad += keep[i] != (want ? 1 : 0);
    kept += want;
  }
  bad += keep[nV] != 0x5a;
  printf("vertex test: %5d vertices, %d kept, %d wrong\n", nV, kept, bad);
  failures += bad;
}

// ---- filter -----------------------------------------------------------------------------------------------------------------
static void check_filter(int nV, int nF, double keep_share, bool with_extras) {
  vector<float> V(3 * (size_t)nV + 3), NV(3 * (size_t)nV + 3);
  vector<int64_t> edges(2 * (size_t)nV + 2);
  for (auto& c : V) c = (float)uniform(-1, 1);
  for (auto& c : NV) c = (float)uniform(-1, 1);
  for (auto& e : edges) e = rng();
  vector<int32_t> F(3 * (size_t)nF + 3);
  for (auto& i : F) i = nV ? uniform_int(0, nV - 1) : 0;
  vector<uint8_t> keep(nV + 1), face_mask(nF + 1, 1);
  for (auto& k : keep) k = uniform(0, 1) < keep_share;
  if (with_extras)
    for (auto& k : face_mask) k = uniform(0, 1) < 0.7;
  vector<uint8_t> face_keep(nF + 1, 0x5a);
  int32_t flag = 0;
  must(psdf_mesh_clean_face_keep(F.data(), nF, keep.data(), nV, with_extras ? face_mask.data() : nullptr, face_keep.data(), &flag,
                                 nullptr), "face_keep");
  vector<int32_t> vincl(nV + 1), fincl(nF + 1);
  int kv = 0, kf = 0;
  for (int i = 0; i < nV; i++) vincl[i] = kv += keep[i];
  for (int f = 0; f < nF; f++) fincl[f] = kf += face_keep[f];
  vector<float> V_out(3 * (size_t)kv + 1, -7.f), NV_out(3 * (size_t)kv + 1, -7.f);
  vector<int64_t> edges_out(2 * (size_t)kv + 1, -7);
  vector<int32_t> F_out(3 * (size_t)kf + 1, -7), vertex_map(nV + 1, -7);
  must(psdf_mesh_clean_emit_vertices(nV, keep.data(), vincl.data(), V.data(), with_extras ? NV.data() : nullptr,
                                     with_extras ? edges.data() : nullptr, V_out.data(), NV_out.data(), edges_out.data(),
                                     vertex_map.data(), nullptr), "emit_vertices");
  must(psdf_mesh_clean_emit_faces(F.data(), nF, face_keep.data(), fincl.data(), vertex_map.data(), F_out.data(), nullptr), "emit_faces");
  int bad = flag != 0, at = 0, fat = 0;
  for (int i = 0; i < nV; i++) {
    if (!keep[i]) {
      bad += vertex_map[i] != -1;
      continue;
    }
    bad += vertex_map[i] != at;
    for (int k = 0; k < 3; k++) bad += V_out[3 * at + k] != V[3 * i + k] || (with_extras && NV_out[3 * at + k] != NV[3 * i + k]);
    for (int k = 0; k < 2 && with_extras; k++) bad += edges_out[2 * at + k] != edges[2 * i + k];
    at++;
  }
  for (int f = 0; f < nF; f++) {
    const bool want = keep[F[3 * f]] && keep[F[3 * f + 1]] && keep[F[3 * f + 2]] && face_mask[f];
    bad += face_keep[f] != (want ? 1 : 0);
    if (!want) continue;
    for (int k = 0; k < 3 && fat < kf; k++) bad += F_out[3 * fat + k] != vertex_map[F[3 * f + k]];
    fat++;
  }
  bad += at != kv || fat != kf || V_out.back() != -7.f || F_out.back() != -7 || vertex_map[nV] != -7 || face_keep[nF] != 0x5a;
  if (nF > 0 && nV > 0) {   // a face out of range raises the flag and is dropped
    F[1] = nV;
    flag = 0;
    must(psdf_mesh_clean_face_keep(F.data(), nF, keep.data(), nV, nullptr, face_keep.data(), &flag, nullptr), "face_keep");
    bad += flag != 2 || face_keep[0] != 0;
  }
  printf("filter: %5d vertices, %5d faces: %d and %d kept, %d wrong\n", nV, nF, kv, kf, bad);
  failures += bad;
}

// ---- components -------------------------------------------------------------------------------------------------------------
static vector<int32_t> brute_labels(const vector<int32_t>& F, int nF, int nV, bool by_edge) {
  vector<vector<int>> adjacent(nF);
  if (by_edge) {
    std::map<std::pair<int, int>, vector<int>> users;
    for (int f = 0; f < nF; f++)
      for (int e = 0; e < 3; e++) {
        const int a = F[3 * f + e], b = F[3 * f + (e + 1) % 3];
        users[{std::min(a, b), std::max(a, b)}].push_back(f);
      }
    for (const auto& [edge, faces] : users)
      if (faces.size() == 2 && edge.first != edge.second) adjacent[faces[0]].push_back(faces[1]), adjacent[faces[1]].push_back(faces[0]);
  } else {
    vector<vector<int>> at(nV);
    for (int f = 0; f < nF; f++)
      for (int k = 0; k < 3; k++) at[F[3 * f + k]].push_back(f);
    for (const auto& faces : at)
      for (size_t k = 1; k < faces.size(); k++) adjacent[faces[0]].push_back(faces[k]), adjacent[faces[k]].push_back(faces[0]);
  }
  vector<int32_t> label(nF, -1);
  for (int f = 0; f < nF; f++) {   // flood from every unlabelled face in ascending order: the label is the smallest member
    if (label[f] >= 0) continue;
    vector<int> stack{f};
    label[f] = f;
    while (!stack.empty()) {
      const int g = stack.back();
      stack.pop_back();
      for (int h : adjacent[g])
        if (label[h] < 0) label[h] = f, stack.push_back(h);
    }
  }
  return label;
}

static void check_components(const char* label, const vector<int32_t>& F, int nV) {
  const int nF = (int)F.size() / 3;
  for (const bool by_edge : {true, false}) {
    vector<int32_t> labels(nF + 1, -7), sizes(nF + 1, 0);
    int32_t flag = 0;
    hip_on_host::concurrent = true;   // 256 threads race on the parents
    if (by_edge) {
      vector<int64_t> keys(3 * (size_t)nF + 1, -7), slot(3 * (size_t)nF), sorted(3 * (size_t)nF);
      must(psdf_mesh_clean_edge_keys(F.data(), nF, nV, keys.data(), &flag, nullptr), "edge_keys");
      std::iota(slot.begin(), slot.end(), 0);
      std::stable_sort(slot.begin(), slot.end(), [&](int64_t a, int64_t b) { return keys[a] < keys[b]; });
      for (size_t i = 0; i < slot.size(); i++) sorted[i] = keys[slot[i]];
      vector<int32_t> parent(nF + 1);
      std::iota(parent.begin(), parent.end(), 0);
      must(psdf_mesh_clean_link_edges(sorted.data(), slot.data(), nF, parent.data(), &flag, nullptr), "link_edges");
      for (int f = 0; f < nF; f++) failures += parent[f] > f;
      must(psdf_mesh_clean_flatten(parent.data(), nF, labels.data(), sizes.data(), &flag, nullptr), "flatten");
      failures += keys.back() != -7;
    } else {
      vector<int32_t> parent(nV + 1), vertex_label(nV + 1, -7), first_face(nV + 1, INT32_MAX);
      std::iota(parent.begin(), parent.end(), 0);
      must(psdf_mesh_clean_link_vertices(F.data(), nF, nV, parent.data(), &flag, nullptr), "link_vertices");
      for (int v = 0; v < nV; v++) failures += parent[v] > v;
      must(psdf_mesh_clean_flatten(parent.data(), nV, vertex_label.data(), nullptr, &flag, nullptr), "flatten");
      must(psdf_mesh_clean_face_labels(F.data(), nF, nV, vertex_label.data(), first_face.data(), labels.data(), sizes.data(), nullptr),
           "face_labels");
      failures += vertex_label[nV] != -7;
    }
    hip_on_host::concurrent = false;
    const vector<int32_t> want = brute_labels(F, nF, nV, by_edge);
    vector<int32_t> want_sizes(nF, 0);
    for (int f = 0; f < nF; f++) want_sizes[want[f]]++;
    int bad = flag != 0, components = 0;
    for (int f = 0; f < nF; f++) bad += labels[f] != want[f] || sizes[f] != want_sizes[f], components += want_sizes[f] > 0;
    bad += labels[nF] != -7 || sizes[nF] != 0;
    printf("components %-22s %6d faces, %-6s: %5d components, %d wrong\n", label, nF, by_edge ? "edge" : "vertex", components, bad);
    failures += bad;
  }
}

static vector<int32_t> strip(int triangles, bool shuffled) {
  vector<int32_t> order(triangles), F;
  std::iota(order.begin(), order.end(), 0);
  if (shuffled) std::shuffle(order.begin(), order.end(), rng);
  for (int t : order) F.insert(F.end(), {t, t + 1, t + 2});
  return F;
}

int main() {
  for (int ksize : {1, 3, 21, 101}) check_dilation("sparse", 2, 70, 100, sparse_masks(2, 70, 100, 0.002), 128, ellipse(ksize));
  for (auto [H, W] : {std::pair<int, int>{1, 1}, {1, 65}, {7, 31}, {7, 32}, {7, 33}, {70, 64}, {3, 300}})
    check_dilation("edge shapes", 1, H, W, sparse_masks(1, H, W, 0.05), 128, ellipse(5));
  check_dilation("all clear", 1, 9, 70, vector<uint8_t>(9 * 70, 128), 128, ellipse(7));
  check_dilation("all set", 1, 9, 70, vector<uint8_t>(9 * 70, 129), 128, ellipse(7));
  check_dilation("bool-like, threshold 0", 1, 9, 70, sparse_masks(1, 9, 70, 0.02), 0, ellipse(3));
  check_dilation("wider than tall", 1, 20, 600, sparse_masks(1, 20, 600, 0.001), 128, {254, 0, 100});
  check_dilation("tallest element", 1, 12, 40, sparse_masks(1, 12, 40, 0.01), 128, vector<int>(255, 1));
  for (int nV : {0, 1, 63, 64, 65, 1500}) check_vertex_test(nV);
  check_filter(2000, 4000, 0.8, true);
  check_filter(65, 257, 0.5, false);
  check_filter(64, 0, 0.5, true);
  check_filter(0, 0, 0.5, false);
  check_filter(300, 500, 1.0, true);
  check_filter(300, 500, 0.0, true);
  check_components("shuffled strip", strip(6000, true), 6002);
  check_components("ordered strip", strip(1000, false), 1002);
  check_components("reversed strip", [] { auto F = strip(1000, false); vector<int32_t> R; for (int f = 999; f >= 0; f--) R.insert(R.end(), F.begin() + 3 * f, F.begin() + 3 * f + 3); return R; }(), 1002);
  {
    vector<int32_t> fan, disjoint, soup;
    for (int t = 0; t < 300; t++) fan.insert(fan.end(), {0, t + 1, t + 2});
    check_components("fan", fan, 302);
    for (int t = 0; t < 500; t++) disjoint.insert(disjoint.end(), {3 * t, 3 * t + 1, 3 * t + 2});
    check_components("disjoint", disjoint, 1500);
    check_components("bow-tie", {0, 1, 2, 2, 3, 4}, 5);
    check_components("three on an edge", {0, 1, 2, 0, 1, 3, 1, 0, 4}, 5);
    check_components("identical faces", {0, 1, 2, 0, 1, 2, 5, 6, 7}, 8);
    check_components("equal indices", {0, 0, 1, 0, 1, 2, 3, 3, 3, 1, 2, 4}, 5);
    check_components("none", {}, 4);
    for (int nF : {1, 63, 64, 65, 257, 3000}) {
      soup.resize(3 * (size_t)nF);
      for (auto& i : soup) i = uniform_int(0, nF / 2 + 2);
      check_components("index soup", soup, nF / 2 + 3);
    }
  }
  {   // a face out of range raises the flag and touches nothing out of bounds
    vector<int32_t> F{0, 1, 2, 1, 2, 7, -1, 0, 1}, parent{0, 1, 2, 3}, labels(3, 0), sizes(3, 0), first(4, INT32_MAX);
    vector<int64_t> keys(9);
    int32_t flag = 0;
    hip_on_host::concurrent = true;
    must(psdf_mesh_clean_edge_keys(F.data(), 3, 4, keys.data(), &flag, nullptr), "edge_keys");
    failures += flag != 2;
    flag = 0;
    must(psdf_mesh_clean_link_vertices(F.data(), 3, 4, parent.data(), &flag, nullptr), "link_vertices");
    failures += flag != 2;
    must(psdf_mesh_clean_face_labels(F.data(), 3, 4, parent.data(), first.data(), labels.data(), sizes.data(), nullptr), "face_labels");
  }
  {   // a parent array that breaks parent[i] <= i (a cycle) ends at the cap with the flag raised, not in a spin
    vector<int32_t> parent{1, 2, 0, 3}, labels(4, -1);
    int32_t flag = 0;
    must(psdf_mesh_clean_flatten(parent.data(), 4, labels.data(), nullptr, &flag, nullptr), "flatten");
    hip_on_host::concurrent = false;
    failures += flag != 4;
    printf("a broken parent array: flag %d\n", flag);
  }
  if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
  else printf("mesh_clean_kernels_check: all checks passed\n");
  return failures != 0;
}
