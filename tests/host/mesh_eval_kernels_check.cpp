// Stand-alone check of the kernels of permuto_sdf_amd/csrc/mesh_eval.hip on the CPU: the file itself is compiled as C++ against
// tests/host/hip_on_host/hip/hip_runtime.h (launches run on CPU threads), driven the way permuto_sdf_amd/mesh_eval.py drives it
// (plan, keys, sort, ranges, kernels) and compared with brute-force float64.  tests/test_mesh_eval_host.py builds it with
// -fsanitize=address,undefined -fno-sanitize-recover=all and runs it: an index out of bounds in a kernel is a sanitizer report
// here, not a fault on a device.  It says nothing about speed, and nothing about what the device compiler makes of the source.
#include <cstdio>
#include <numeric>
#include <random>

#include "mesh_eval.hip"

using std::vector;

static std::mt19937 rng(5);
static float uniform(float a, float b) { return std::uniform_real_distribution<float>(a, b)(rng); }
static float normal() { return std::normal_distribution<float>(0, 1)(rng); }
static const double U = std::ldexp(1.0, -24);
static int failures = 0;

struct Cloud {
  vector<float> p;
  int64_t n() const { return (int64_t)p.size() / 3; }
  const float* at(int64_t i) const { return &p[3 * i]; }
  void add(float x, float y, float z) { p.insert(p.end(), {x, y, z}); }
};
static bool finite(const float* p) { return std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]); }
static double distance64(const float* a, const float* b) {
  double s = 0;
  for (int k = 0; k < 3; k++) s += ((double)a[k] - b[k]) * ((double)a[k] - b[k]);
  return std::sqrt(s);
}
static void must(int status, const char* what) {
  if (status != 0) {
    fprintf(stderr, "%s returned %d\n", what, status);
    exit(2);
  }
}

struct GridOf {
  float origin_edge[4];
  int dims[3];
  int64_t cells, blocks;
};
// the grid of a cloud's finite points; false when there is none
static bool plan_of(const Cloud& c, double min_edge, GridOf& g) {
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  int64_t count = 0;
  for (int64_t i = 0; i < c.n(); i++)
    if (finite(c.at(i))) {
      count++;
      for (int a = 0; a < 3; a++) lo[a] = std::min(lo[a], (double)c.at(i)[a]), hi[a] = std::max(hi[a], (double)c.at(i)[a]);
    }
  if (!count) return false;
  must(psdf_mesh_eval_grid_plan(lo, hi, count, min_edge, 0, g.origin_edge, g.dims, &g.cells, &g.blocks), "grid_plan");
  return true;
}

struct Sorted {
  vector<float> p;
  vector<int32_t> keys, start;
  vector<int64_t> perm;
};
static Sorted sort_by_key(const Cloud& c, const GridOf& g, int block_log2) {
  Sorted s;
  const int64_t n = c.n();
  vector<int32_t> keys(n);
  must(psdf_mesh_eval_cell_keys(c.p.data(), n, g.origin_edge, g.dims, block_log2, keys.data(), nullptr), "cell_keys");
  s.perm.resize(n);
  std::iota(s.perm.begin(), s.perm.end(), 0);
  std::stable_sort(s.perm.begin(), s.perm.end(), [&](int64_t a, int64_t b) { return keys[a] < keys[b]; });
  s.keys.resize(n);
  s.p.resize(3 * n);
  for (int64_t i = 0; i < n; i++) {
    s.keys[i] = keys[s.perm[i]];
    for (int a = 0; a < 3; a++) s.p[3 * i + a] = c.at(s.perm[i])[a];
  }
  const int64_t count = block_log2 ? g.blocks : g.cells;
  s.start.assign(count + 1, -7);
  must(psdf_mesh_eval_cell_ranges(s.keys.data(), n, count, s.start.data(), nullptr), "cell_ranges");
  return s;
}

static void check_nearest(const char* label, const Cloud& q, const Cloud& r, float max_dist) {
  const int64_t nq = q.n(), nr = r.n();
  vector<float> dist(nq, max_dist);
  vector<int64_t> idx(nq, -1);
  int32_t nr_open = 0;
  GridOf g;
  if (nq && plan_of(r, 0.0, g)) {
    const Sorted rs = sort_by_key(r, g, 0), qs = sort_by_key(q, g, psdf::mesh_eval_plan::QUERY_BLOCK_LOG2);
    vector<float> d(nq, max_dist);
    vector<int32_t> at(nq, -1);
    vector<uint8_t> open(nq, 0);
    hip_on_host::concurrent = true;
    must(psdf_mesh_nn_cooperative(qs.p.data(), nq, qs.start.data(), rs.p.data(), nr, rs.start.data(), g.origin_edge, g.dims,
                                  max_dist, d.data(), at.data(), open.data(), &nr_open, nullptr), "nn_cooperative");
    hip_on_host::concurrent = false;
    must(psdf_mesh_nn_ring(qs.p.data(), nq, rs.p.data(), nr, rs.start.data(), g.origin_edge, g.dims, max_dist, d.data(), at.data(),
                           open.data(), nullptr), "nn_ring");
    for (int64_t i = 0; i < nq; i++) {
      dist[qs.perm[i]] = d[i];
      idx[qs.perm[i]] = at[i] >= 0 ? rs.perm[at[i]] : -1;
    }
  }
  int bad = 0;
  double worst = 0;
  for (int64_t i = 0; i < nq; i++) {
    double best = INFINITY;
    if (finite(q.at(i)))
      for (int64_t j = 0; j < nr; j++)
        if (finite(r.at(j))) best = std::min(best, distance64(q.at(i), r.at(j)));
    if (std::fabs(best - max_dist) <= 8 * U * max_dist) continue;   // a coin toss at the cut-off
    bool ok;
    if (best >= max_dist) {
      ok = idx[i] == -1 && dist[i] == max_dist;
    } else {
      const double err = std::fabs((double)dist[i] - best), bar = 4 * U * best;
      ok = idx[i] >= 0 && idx[i] < nr && err <= bar && distance64(q.at(i), r.at(idx[i])) <= best * (1 + 4 * U);
      if (ok && bar > 0) worst = std::max(worst, err / bar);
    }
    if (!ok && bad++ < 5) fprintf(stderr, "  %s, query %ld: got %.9g (row %ld), float64 %.9g\n", label, (long)i, dist[i], (long)idx[i], best);
  }
  printf("nearest  %-24s %5ld x %5ld: %d wrong, largest error / bar %.3f, %d left to the ring search\n", label, (long)nq, (long)nr,
         bad, worst, nr_open);
  failures += bad;
}

static void check_thinning(const char* label, const Cloud& c, float radius, const vector<int64_t>& order) {
  const int64_t n = c.n();
  vector<uint8_t> mask(n, 1);
  int sweeps = 0;
  GridOf g;
  if (n && plan_of(c, radius, g)) {
    const Sorted s = sort_by_key(c, g, 0);
    vector<int32_t> rank(n), rank_sorted(n);
    for (int64_t k = 0; k < n; k++) rank[order[k]] = (int32_t)k;
    for (int64_t i = 0; i < n; i++) rank_sorted[i] = rank[s.perm[i]];
    vector<uint8_t> state(n, 0);
    hip_on_host::concurrent = true;
    for (int32_t undecided = 1; undecided; sweeps++) {
      undecided = 0;
      must(psdf_mesh_thin_sweep(s.p.data(), rank_sorted.data(), s.keys.data(), n, s.start.data(), g.origin_edge, g.dims, radius,
                                state.data(), &undecided, nullptr), "thin_sweep");
      if (sweeps > 4 * n + 4) must(-99, "thin_sweep (no end)");
    }
    hip_on_host::concurrent = false;
    for (int64_t i = 0; i < n; i++) mask[s.perm[i]] = state[i] == 1;
  }
  vector<uint8_t> want(n, 1);   // the sequential loop
  for (int64_t k = 0; k < n; k++) {
    const int64_t cur = order[k];
    if (!want[cur]) continue;
    for (int64_t j = 0; j < n; j++)
      if (j != cur && distance64(c.at(cur), c.at(j)) <= (double)radius) want[j] = 0;
  }
  int bad = 0, kept = 0;
  for (int64_t i = 0; i < n; i++) bad += mask[i] != want[i], kept += want[i];
  printf("thinning %-24s %5ld points: %d kept, %d wrong, %d sweeps\n", label, (long)n, kept, bad, sweeps);
  failures += bad;
}

static void check_sampling(double density) {
  Cloud V;
  vector<int32_t> F;
  auto triangle = [&](std::initializer_list<float> c) {
    const int first = (int)V.n();
    V.p.insert(V.p.end(), c);
    F.insert(F.end(), {first, first + 1, first + 2});
  };
  const float d = (float)density;
  for (int k = 0; k < 300; k++) {
    const float p[3] = {uniform(-10, 10), uniform(-10, 10), uniform(-10, 10)};
    float e[2][3];
    for (auto& v : e) {
      const float len = uniform(0.5f, 20.f) * d, x = normal(), y = normal(), z = normal(), l = std::sqrt(x * x + y * y + z * z);
      v[0] = len * x / l, v[1] = len * y / l, v[2] = len * z / l;
    }
    triangle({p[0], p[1], p[2], p[0] + e[0][0], p[1] + e[0][1], p[2] + e[0][2], p[0] + e[1][0], p[1] + e[1][1], p[2] + e[1][2]});
  }
  triangle({1, 2, 3, 1, 2, 3, 2, 2, 3});                          // two equal corners
  triangle({0, 0, 0, 1, 1, 1, 2, 2, 2});                          // collinear
  triangle({5, 5, 5, 5 + 0.3f * d, 5, 5, 5, 5 + 0.3f * d, 5});    // smaller than the density
  for (int n : {3, 4, 5, 7}) triangle({0, 0, 0, (float)((n + 0.5) * density), 0, 0, 0, (float)((n + 0.5) * density), 0});
  const int64_t nF = (int64_t)F.size() / 3, nV = V.n();
  vector<int32_t> counts(nF, -5);
  int32_t flag = 0;
  must(psdf_mesh_sample_count(V.p.data(), nV, F.data(), nF, density, counts.data(), &flag, nullptr), "sample_count");
  vector<int64_t> incl(nF);
  int64_t total = 0;
  for (int64_t f = 0; f < nF; f++) incl[f] = total += counts[f];
  vector<float> out(3 * total + 3, -777.f);   // one guard row
  must(psdf_mesh_sample_emit(V.p.data(), nV, F.data(), nF, density, incl.data(), out.data(), nullptr), "sample_emit");
  int bad = 0;
  int64_t at = 0;
  for (int64_t f = 0; f < nF; f++) {
    double p0[3], e1[3], e2[3];
    for (int a = 0; a < 3; a++) {
      p0[a] = V.at(F[3 * f])[a];
      e1[a] = (double)V.at(F[3 * f + 1])[a] - p0[a];
      e2[a] = (double)V.at(F[3 * f + 2])[a] - p0[a];
    }
    const double l1 = std::sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]), l2 = std::sqrt(e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2]);
    const double cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2], cz = e1[0] * e2[1] - e1[1] * e2[0];
    const double A2 = std::sqrt(cx * cx + cy * cy + cz * cz);
    int64_t count = 0;
    if (A2 > 0) {
      const double s = density * std::sqrt(l1 * l2 / A2), n1 = std::floor(l1 / s), n2 = std::floor(l2 / s);
      for (int i = 0; i <= (int)n1; i++)
        for (int j = 0; j <= (int)n2; j++) {
          const double a = (i + 0.5) / std::max(n1, 1e-7), b = (j + 0.5) / std::max(n2, 1e-7);
          if (!(a + b < 1)) continue;
          count++;
          for (int k = 0; k < 3 && at < total; k++) bad += out[3 * at + k] != (float)((e1[k] * a + e2[k] * b) + p0[k]);
          at++;
        }
    }
    bad += count != counts[f];
  }
  bad += out[3 * total] != -777.f || flag != 0;
  printf("sampling: %ld triangles, %ld samples, %d wrong\n", (long)nF, (long)total, bad);
  failures += bad;
}

static Cloud noisy_sphere(int n, float scale, float offset) {
  Cloud c;
  for (int i = 0; i < n; i++) {
    const float x = normal(), y = normal(), z = normal(), l = std::sqrt(x * x + y * y + z * z);
    c.add((x / l * 0.4f + 0.002f * normal()) * scale + offset, (y / l * 0.4f + 0.002f * normal()) * scale + offset,
          (z / l * 0.4f + 0.002f * normal()) * scale + offset);
  }
  return c;
}
static vector<int64_t> shuffled(int64_t n) {
  vector<int64_t> o(n);
  std::iota(o.begin(), o.end(), 0);
  std::shuffle(o.begin(), o.end(), rng);
  return o;
}
static Cloud box_corners(float side) {
  Cloud c;
  for (float x : {0.f, side})
    for (float y : {0.f, side})
      for (float z : {0.f, side}) c.add(x, y, z);
  return c;
}

int main() {
  check_sampling(0.2);
  {
    const Cloud r = noisy_sphere(1500, 500, 0), q = noisy_sphere(1500, 500, 0.3f);
    check_nearest("spheres x 500", q, r, 20.f);
    check_nearest("spheres x 500, cut-off 2", q, r, 2.f);
  }
  {
    const Cloud r = noisy_sphere(65, 1, 0), q = noisy_sphere(63, 1, 0), none;
    Cloud one;
    one.add(1, 2, 3);
    check_nearest("63 x 65", q, r, 0.5f);
    check_nearest("63 x 65, tight cut-off", q, r, 0.03f);
    check_nearest("1 x 1", one, one, 1.f);
    check_nearest("no references", q, none, 1.f);
    check_nearest("no queries", none, r, 1.f);
  }
  {   // one cell with more references than two LDS tiles
    Cloud r = box_corners(10), q;
    for (int i = 0; i < 2 * psdf_mesh_eval_tile_capacity() + 100; i++)
      r.add(5.5f + uniform(-1e-3f, 1e-3f), 5.5f + uniform(-1e-3f, 1e-3f), 5.5f + uniform(-1e-3f, 1e-3f));
    for (int i = 0; i < 300; i++) q.add(5.5f + uniform(-.01f, .01f), 5.5f + uniform(-.01f, .01f), 5.5f + uniform(-.01f, .01f));
    for (int i = 0; i < 300; i++) q.add(uniform(0, 10), uniform(0, 10), uniform(0, 10));
    check_nearest("heavy cell", q, r, 20.f);
  }
  {   // a lattice five cell edges apart: answers several shells out; queries outside the box
    Cloud r, q, outside;
    for (int x = 0; x < 4; x++)
      for (int y = 0; y < 4; y++)
        for (int z = 0; z < 4; z++) r.add(2.f * x, 2.f * y, 2.f * z);
    for (int i = 0; i < 5336; i++) r.add(0, 0, 0);
    for (int i = 0; i < 300; i++) q.add(uniform(0, 6), uniform(0, 6), uniform(0, 6));
    check_nearest("lattice", q, r, 20.f);
    check_nearest("lattice, cut-off 1", q, r, 1.f);
    for (int axis = 0; axis < 3; axis++)
      for (int sign : {-1, 1})
        for (float by : {0.3f, 0.9f, 1.1f, 4.f})
          for (int i = 0; i < 10; i++) {
            float p[3] = {uniform(0, 6), uniform(0, 6), uniform(0, 6)};
            p[axis] = sign > 0 ? 6 + by : -by;
            outside.add(p[0], p[1], p[2]);
          }
    outside.add(1e6f, -1e6f, 3.f);
    outside.add(-40.f, 2.f, 2.f);
    check_nearest("outside, cut-off 1", outside, r, 1.f);
    check_nearest("outside, cut-off 20", outside, r, 20.f);
  }
  {
    Cloud r = noisy_sphere(800, 500, 0), q = noisy_sphere(800, 500, 0.3f), all_nan;
    r.p[3 * 5 + 1] = NAN, r.p[3 * 9 + 2] = INFINITY, q.p[3 * 10] = NAN, q.p[3 * 20 + 2] = -INFINITY;
    all_nan.add(NAN, 0, 0);
    check_nearest("non-finite points", q, r, 20.f);
    check_nearest("every reference NaN", q, all_nan, 20.f);
  }
  {   // points on cell boundaries
    Cloud r = box_corners(10), q;
    for (int i = 0; i < 3000; i++) r.add(uniform(0, 10), uniform(0, 10), uniform(0, 10));
    GridOf g;
    plan_of(r, 0, g);
    const float e = g.origin_edge[3];
    for (int i = 8; i < 1500; i++) r.p[3 * i] = e * (int)uniform(0, 12), r.p[3 * i + 1] = e * (int)uniform(0, 12);
    for (int i = 0; i < 500; i++) q.add(e * (int)uniform(0, 12), e * (int)uniform(0, 12), e * (int)uniform(0, 12));
    check_nearest("cell boundaries", q, r, 20.f);
  }
  for (int n : {1, 2, 63, 64, 65, 257, 2000}) {
    char label[32];
    snprintf(label, sizeof label, "sphere, n = %d", n);
    check_thinning(label, noisy_sphere(n, n > 300 ? 1.f : 0.25f, 0), n > 300 ? 0.05f : 0.02f, shuffled(n));
  }
  for (float radius : {0.008f, 0.064f}) check_thinning("the radius decides the edge", noisy_sphere(1500, 10 * radius, 0), radius, shuffled(1500));
  {
    Cloud same, line, lattice;
    for (int i = 0; i < 257; i++) same.add(0.25f, -1.5f, 3.f);
    check_thinning("identical points", same, 0.02f, shuffled(257));
    for (int i = 0; i < 100; i++) line.add(i * (0.6f * 0.02f), 0, 0);
    vector<int64_t> identity(100);
    std::iota(identity.begin(), identity.end(), 0);
    check_thinning("sorted line", line, 0.02f, identity);
    const float e = 0.125f * (1 + 1.f / 512);
    for (int x = 0; x < 4; x++)
      for (int y = 0; y < 4; y++)
        for (int z = 0; z < 4; z++) {
          lattice.add(0.3f + x * e, -1.7f + y * e, 2.1f + z * e);
          for (int k = 0; k < 4; k++)
            lattice.add(std::clamp(0.3f + x * e + uniform(-.05f, .05f), 0.3f, 0.3f + 3 * e),
                        std::clamp(-1.7f + y * e + uniform(-.05f, .05f), -1.7f, -1.7f + 3 * e),
                        std::clamp(2.1f + z * e + uniform(-.05f, .05f), 2.1f, 2.1f + 3 * e));
        }
    check_thinning("cell boundaries", lattice, 0.125f, shuffled(lattice.n()));
    check_thinning("empty cloud", Cloud(), 0.1f, {});
  }
  if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
  else printf("mesh_eval_kernels_check: all checks passed\n");
  return failures != 0;
}
