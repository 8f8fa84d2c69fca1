// Mesh evaluation for gfx950: the three data-parallel stages of the DTU Chamfer protocol (the reference scores its meshes with
// permuto_sdf_py/experiments/evaluation/DTUeval-python/eval.py) on tensors the mesh extractor leaves on the device.
//
//   (a) surface sampling: a lattice of points on every triangle -- a count pass, the caller's inclusive scan, an emit pass, so the
//       order of the cloud (triangle by triangle, i-major, j-minor) is a function of the inputs alone.  Every decision (n1, n2, the
//       `a + b < 1` predicate) is taken in float64 from the fp32 corners promoted, with IEEE division and square root, and the
//       lattice coordinate is the plain (i + 1/2) / n: the predicate is a knife edge whenever i + j + 1 = n1 = n2, and only the
//       same expression gives the same count as a float64 host evaluation.  The point is rounded to fp32 once.
//   (b) radius thinning: the protocol walks a shuffled cloud in order, a point still alive kills every neighbour within the
//       radius (d <= radius).  The survivors are the lexicographically first maximal independent set of the radius graph under
//       that order, which has a parallel form: per point a state undecided / kept / dropped; a sweep looks, for every undecided
//       point, at its neighbours of lower rank -- one kept: dropped; all dropped: kept; otherwise still undecided.  States only
//       move from undecided to final, so the sweeps run in place: a stale read costs a sweep, never correctness.  The caller
//       repeats sweeps until the device counter of undecided points reads zero (no sweep cap: a sorted line of N points needs
//       about N / 2 sweeps).
//   (c) nearest neighbour with a cut-off: for every query the distance to the nearest reference point and its position in the
//       sorted references, or (max_dist, -1) when nothing is closer than max_dist, strictly.  The references are binned into a
//       uniform grid (mesh_eval_plan.h); the queries are sorted by block of 4 x 4 x 4 cells.  Cooperative pass: a workgroup owns
//       the queries of one block, stages the references of the block's cells and their one-cell halo through LDS in tiles of
//       TILE_CAPACITY points, and every lane tests its query against the staged tile.  A query whose best distance is not proven
//       minimal -- best <= distance from the query to the boundary of the region searched -- is left open and finished by the ring
//       pass, which widens the search shell by shell around the query's cell until the same bound holds.  best starts at
//       max_dist, so the search never looks further than the cut-off.
//       Distances are the difference form: fl(q - r) per component, squares, sums, sqrtf -- |q|^2 + |r|^2 - 2 q.r loses
//       everything at the coordinate scale of a scanned scene.
//
// One device function computes cell coordinates for the binning of references, queries and the thinning grid; it clamps in
// floating point before the integer conversion, so a non-finite coordinate is a defined cell, and the keys kernel gives a point
// with a non-finite coordinate the key `cells` (past every cell): as a reference it is in no cell's range, as a query in no
// block's (its answer is what the caller pre-filled: max_dist, -1).
//
// The entries allocate nothing and never synchronise; sorts and scans are the caller's.
#include "psdf_common.h"
#include "mesh_eval_plan.h"
#include "../../include/psdf.h"

using namespace psdf;
namespace plan = psdf::mesh_eval_plan;

namespace {

struct Grid {
  float ox, oy, oz, edge;
  int nx, ny, nz;
};

// ---- the shared cell function --------------------------------------------------------------------------------------------
__device__ __forceinline__ float cell_coord(float p, float o, float edge) { return (p - o) / edge; }
// clamped in floating point (fmaxf(NaN, 0) = 0), then converted
__device__ __forceinline__ int cell_index(float t, int n) { return (int)fminf(fmaxf(t, 0.f), (float)(n - 1)); }
__device__ __forceinline__ bool finite3(v3 p) { return isfinite(p.x) && isfinite(p.y) && isfinite(p.z); }
__device__ __forceinline__ v3 cell_coords(const Grid& g, v3 p) {
  return mk3(cell_coord(p.x, g.ox, g.edge), cell_coord(p.y, g.oy, g.edge), cell_coord(p.z, g.oz, g.edge));
}
__device__ __forceinline__ int cell_key(const Grid& g, int cx, int cy, int cz) { return (cx * g.ny + cy) * g.nz + cz; }

__device__ __forceinline__ float distance(v3 q, v3 r) {
  const float dx = q.x - r.x, dy = q.y - r.y, dz = q.z - r.z;
  return sqrtf(dx * dx + dy * dy + dz * dz);
}
__device__ __forceinline__ float distance2(v3 q, v3 r) {
  const float dx = q.x - r.x, dy = q.y - r.y, dz = q.z - r.z;
  return dx * dx + dy * dy + dz * dz;
}

// key of every point: its cell (block_log2 = 0) or its block of (1 << block_log2)^3 cells; `sentinel` for a non-finite point
__global__ void __launch_bounds__(PSDF_BLOCK)
    cell_keys_kernel(Grid g, int block_log2, int sentinel, int64_t n, const float* __restrict__ pts, int32_t* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * PSDF_BLOCK + threadIdx.x;
  if (i >= n) return;
  const v3 p = ld3(pts + 3 * i);
  int key = sentinel;
  if (finite3(p)) {
    const v3 t = cell_coords(g, p);
    const int round = (1 << block_log2) - 1;
    const int by = (g.ny + round) >> block_log2, bz = (g.nz + round) >> block_log2;
    key = ((cell_index(t.x, g.nx) >> block_log2) * by + (cell_index(t.y, g.ny) >> block_log2)) * bz +
          (cell_index(t.z, g.nz) >> block_log2);
  }
  keys[i] = key;
}

// start[c] = first position of the sorted keys that holds a key >= c, for c = 0 .. cells: cell c owns [start[c], start[c + 1])
__global__ void __launch_bounds__(PSDF_BLOCK)
    cell_ranges_kernel(int64_t cells, int64_t n, const int32_t* __restrict__ sorted_keys, int32_t* __restrict__ start) {
  const int64_t c = (int64_t)blockIdx.x * PSDF_BLOCK + threadIdx.x;
  if (c > cells) return;
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if ((int64_t)sorted_keys[mid] < c) lo = mid + 1;
    else hi = mid;
  }
  start[c] = (int32_t)lo;
}

// ---- (a) surface sampling ------------------------------------------------------------------------------------------------
constexpr double SAMPLE_MAX_N = 30000.0;   // lattice steps per edge: the count of one triangle stays below 2^31

struct TriLattice {
  double p0[3], e1[3], e2[3];
  double n1, n2;   // < 0: the triangle emits nothing
};

__device__ __forceinline__ bool load_triangle(const float* __restrict__ V, int64_t nV, const int32_t* __restrict__ F, int64_t f,
                                              double density, TriLattice& t, int32_t* overflow) {
  t.n1 = t.n2 = -1.0;
  const int64_t i0 = F[3 * f], i1 = F[3 * f + 1], i2 = F[3 * f + 2];
  if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= nV || i1 >= nV || i2 >= nV) {
    if (overflow) atomicOr(overflow, 2);
    return false;
  }
#pragma unroll
  for (int a = 0; a < 3; a++) {
    t.p0[a] = (double)V[3 * i0 + a];
    t.e1[a] = (double)V[3 * i1 + a] - t.p0[a];
    t.e2[a] = (double)V[3 * i2 + a] - t.p0[a];
  }
  const double l1 = sqrt(t.e1[0] * t.e1[0] + t.e1[1] * t.e1[1] + t.e1[2] * t.e1[2]);
  const double l2 = sqrt(t.e2[0] * t.e2[0] + t.e2[1] * t.e2[1] + t.e2[2] * t.e2[2]);
  const double cx = t.e1[1] * t.e2[2] - t.e1[2] * t.e2[1];
  const double cy = t.e1[2] * t.e2[0] - t.e1[0] * t.e2[2];
  const double cz = t.e1[0] * t.e2[1] - t.e1[1] * t.e2[0];
  const double A2 = sqrt(cx * cx + cy * cy + cz * cz);
  if (!(A2 > 0.0)) return false;
  const double s = density * sqrt(l1 * l2 / A2);
  const double n1 = floor(l1 / s), n2 = floor(l2 / s);
  if (!(n1 >= 0.0) || !(n2 >= 0.0)) return false;   // NaN corners
  if (n1 > SAMPLE_MAX_N || n2 > SAMPLE_MAX_N) {
    if (overflow) atomicOr(overflow, 1);
    return false;
  }
  t.n1 = n1;
  t.n2 = n2;
  return true;
}

__device__ __forceinline__ bool lattice_keeps(double a, int j, double den2) { return a + ((double)j + 0.5) / den2 < 1.0; }

// number of j in 0 .. n2 with a + b_j < 1: the predicate is monotone in j, so an estimate corrected by the predicate itself
__device__ __forceinline__ int row_count(double a, int n2, double den2) {
  double est = floor((1.0 - a) * den2 - 0.5) + 1.0;
  est = est < 0.0 ? 0.0 : (est > (double)n2 + 1.0 ? (double)n2 + 1.0 : est);
  int j = (int)est;
  while (j > 0 && !lattice_keeps(a, j - 1, den2)) j--;
  while (j <= n2 && lattice_keeps(a, j, den2)) j++;
  return j;
}

__global__ void __launch_bounds__(PSDF_BLOCK)
    sample_count_kernel(const float* __restrict__ V, int64_t nV, const int32_t* __restrict__ F, int64_t nF, double density,
                        int32_t* __restrict__ counts, int32_t* __restrict__ overflow) {
  const int64_t f = (int64_t)blockIdx.x * PSDF_BLOCK + threadIdx.x;
  if (f >= nF) return;
  TriLattice t;
  int64_t total = 0;
  if (load_triangle(V, nV, F, f, density, t, overflow)) {
    const int n1 = (int)t.n1, n2 = (int)t.n2;
    const double den1 = fmax(t.n1, 1e-7), den2 = fmax(t.n2, 1e-7);
    for (int i = 0; i <= n1; i++) {
      const int c = row_count(((double)i + 0.5) / den1, n2, den2);
      if (c == 0 && i > 0) break;   // a_i grows with i: the later rows are empty too
      total += c;
    }
  }
  counts[f] = (int32_t)total;
}

__global__ void __launch_bounds__(PSDF_BLOCK)
    sample_emit_kernel(const float* __restrict__ V, int64_t nV, const int32_t* __restrict__ F, int64_t nF, double density,
                       const int64_t* __restrict__ incl, float* __restrict__ samples) {
  const int64_t f = (int64_t)blockIdx.x * PSDF_BLOCK + threadIdx.x;
  if (f >= nF) return;
  const int64_t end = incl[f];
  int64_t at = f > 0 ? incl[f - 1] : 0;
  if (end == at) return;
  TriLattice t;
  if (!load_triangle(V, nV, F, f, density, t, nullptr)) return;
  const int n1 = (int)t.n1, n2 = (int)t.n2;
  const double den1 = fmax(t.n1, 1e-7), den2 = fmax(t.n2, 1e-7);
  for (int i = 0; i <= n1 && at < end; i++) {
    const double a = ((double)i + 0.5) / den1;
    const int c = row_count(a, n2, den2);
    for (int j = 0; j < c && at < end; j++, at++) {   // (at < end: never past the rows the count pass reserved)
      const double b = ((double)j + 0.5) / den2;
#pragma unroll
      for (int k = 0; k < 3; k++) samples[3 * at + k] = (float)((t.e1[k] * a + t.e2[k] * b) + t.p0[k]);
    }
  }
}

// ---- (b) radius thinning ---------------------------------------------------------------------------------------------------
enum : uint8_t { UNDECIDED = 0, KEPT = 1, DROPPED = 2 };

__global__ void __launch_bounds__(PSDF_BLOCK)
    thin_sweep_kernel(Grid g, int64_t n, const float* __restrict__ pts, const int32_t* __restrict__ rank,
                      const int32_t* __restrict__ keys, const int32_t* __restrict__ start, float radius, int sentinel,
                      uint8_t* state, int32_t* __restrict__ undecided) {
  const int64_t i = (int64_t)blockIdx.x * PSDF_BLOCK + threadIdx.x;
  bool open = false;
  if (i < n && state[i] == UNDECIDED) {
    uint8_t result = KEPT;
    if (keys[i] != sentinel) {   // (a non-finite point has no neighbours)
      const v3 p = ld3(pts + 3 * i);
      const int my_rank = rank[i];
      const v3 t = cell_coords(g, p);
      const int cx = cell_index(t.x, g.nx), cy = cell_index(t.y, g.ny), cz = cell_index(t.z, g.nz);
      const int z0 = max(cz - 1, 0), z1 = min(cz + 1, g.nz - 1);
      for (int x = max(cx - 1, 0); x <= min(cx + 1, g.nx - 1) && result != DROPPED; x++)
        for (int y = max(cy - 1, 0); y <= min(cy + 1, g.ny - 1) && result != DROPPED; y++) {
          const int first = start[cell_key(g, x, y, z0)], last = start[cell_key(g, x, y, z1) + 1];   // a run of cells along z
          for (int j = first; j < last; j++) {
            if (rank[j] >= my_rank) continue;
            const uint8_t s = __atomic_load_n(state + j, __ATOMIC_RELAXED);
            if (s == DROPPED) continue;
            if (!(distance(p, ld3(pts + 3 * (int64_t)j)) <= radius)) continue;
            if (s == KEPT) {
              result = DROPPED;
              break;
            }
            result = UNDECIDED;
          }
        }
    }
    if (result != UNDECIDED) __atomic_store_n(state + i, result, __ATOMIC_RELAXED);
    open = result == UNDECIDED;
  }
  const unsigned long long b = __ballot(open);
  if (lane_id() == 0 && b) atomicAdd(undecided, (int)__popcll(b));
}

// ---- (c) nearest neighbour ---------------------------------------------------------------------------------------------------
struct Best {
  float d2;
  int at;
};
__device__ __forceinline__ void consider(Best& b, v3 q, v3 r, int at) {
  const float d2 = distance2(q, r);
  if (d2 < b.d2) {
    b.d2 = d2;
    b.at = at;
  }
}
// Lower bounds (in cells) on the distance from a query to every reference not yet tested, less the slack of the cell function.
// axis_gap: to the faces of the searched cells lo .. hi along one axis; a face on the grid's border is infinitely far: no
// reference lies beyond it.  axis_outside: to the grid itself, for a query outside it along this axis.
__device__ __forceinline__ float cell_slack(float t) { return plan::CELL_SLACK + 1e-6f * fabsf(t); }
__device__ __forceinline__ float axis_gap(float t, int lo, int hi, int n) {
  const float inf = __builtin_huge_valf();
  const float below = lo <= 0 ? inf : t - (float)lo;
  const float above = hi >= n - 1 ? inf : (float)(hi + 1) - t;
  const float nearest = fminf(below, above);
  return nearest == inf ? inf : nearest - cell_slack(t);
}
__device__ __forceinline__ float axis_outside(float t, int n) { return fmaxf(fmaxf(-t, t - (float)n) - cell_slack(t), 0.f); }
// the distance no untested reference can undercut, after the cells [x0, x1] x [y0, y1] x [z0, z1] have been searched
__device__ __forceinline__ float search_bound(const Grid& g, v3 t, int x0, int x1, int y0, int y1, int z0, int z1) {
  const float gap = fminf(fminf(axis_gap(t.x, x0, x1, g.nx), axis_gap(t.y, y0, y1, g.ny)), axis_gap(t.z, z0, z1, g.nz));
  const float outside = fmaxf(fmaxf(axis_outside(t.x, g.nx), axis_outside(t.y, g.ny)), axis_outside(t.z, g.nz));
  return fmaxf(gap, outside) * g.edge;
}
// the answer so far: best distance below the cut-off, or (max_dist, -1)
__device__ __forceinline__ void answer(const Best& b, float max_dist, float& d, int& at) {
  const float s = sqrtf(b.d2);
  const bool hit = b.at >= 0 && s < max_dist;
  d = hit ? s : max_dist;
  at = hit ? b.at : -1;
}

constexpr int NN_BLOCK = 1 << plan::QUERY_BLOCK_LOG2;   // cells per axis of a block
constexpr int NN_SPAN = NN_BLOCK + 2;                  // with the halo
constexpr int NN_RUNS = NN_SPAN * NN_SPAN;             // runs of cells along z

__global__ void __launch_bounds__(PSDF_BLOCK)
    nn_cooperative_kernel(Grid g, int nby, int nbz, const float* __restrict__ queries, const int32_t* __restrict__ qstart,
                          const float* __restrict__ refs, const int32_t* __restrict__ start, float max_dist,
                          float* __restrict__ dist, int32_t* __restrict__ idx, uint8_t* __restrict__ open_flag,
                          int32_t* __restrict__ nr_open) {
  __shared__ float4 tile[plan::TILE_CAPACITY];
  __shared__ int run_first[NN_RUNS];
  __shared__ int run_offset[NN_RUNS + 1];   // exclusive prefix of the run lengths
  const int block = (int)blockIdx.x;
  const int q0 = qstart[block], q1 = qstart[block + 1];
  if (q0 >= q1) return;   // (uniform over the workgroup)
  const int bz = block % nbz, by = (block / nbz) % nby, bx = block / (nbz * nby);
  const int x0 = max(bx * NN_BLOCK - 1, 0), x1 = min(bx * NN_BLOCK + NN_BLOCK, g.nx - 1);
  const int y0 = max(by * NN_BLOCK - 1, 0), y1 = min(by * NN_BLOCK + NN_BLOCK, g.ny - 1);
  const int z0 = max(bz * NN_BLOCK - 1, 0), z1 = min(bz * NN_BLOCK + NN_BLOCK, g.nz - 1);
  const int ny_run = y1 - y0 + 1, nruns = (x1 - x0 + 1) * ny_run;
  const int tid = (int)threadIdx.x;
  if (tid < nruns) {
    const int x = x0 + tid / ny_run, y = y0 + tid % ny_run;
    const int first = start[cell_key(g, x, y, z0)];
    run_first[tid] = first;
    run_offset[tid + 1] = start[cell_key(g, x, y, z1) + 1] - first;
  }
  __syncthreads();
  if (tid == 0) {
    run_offset[0] = 0;
    for (int r = 0; r < nruns; r++) run_offset[r + 1] += run_offset[r];
  }
  __syncthreads();
  const int total = run_offset[nruns];
  for (int qb = q0; qb < q1; qb += PSDF_BLOCK) {
    const int qi = qb + tid;
    const bool live = qi < q1;
    const v3 q = live ? ld3(queries + 3 * (int64_t)qi) : mk3(0.f, 0.f, 0.f);
    Best best{__builtin_huge_valf(), -1};
    for (int base = 0; base < total; base += plan::TILE_CAPACITY) {
      const int count = min(plan::TILE_CAPACITY, total - base);
      __syncthreads();   // the previous tile has been read
      for (int e = tid; e < count; e += PSDF_BLOCK) {
        const int flat = base + e;
        int r = 0;
        while (run_offset[r + 1] <= flat) r++;   // (flat < total = run_offset[nruns])
        const int at = run_first[r] + (flat - run_offset[r]);
        const v3 p = ld3(refs + 3 * (int64_t)at);
        tile[e] = make_float4(p.x, p.y, p.z, __int_as_float(at));
      }
      __syncthreads();
      if (live)
        for (int e = 0; e < count; e++) {
          const float4 r = tile[e];
          consider(best, q, mk3(r.x, r.y, r.z), __float_as_int(r.w));
        }
    }
    bool open = false;
    if (live) {
      float d;
      int at;
      answer(best, max_dist, d, at);
      const v3 t = cell_coords(g, q);
      open = !(d <= search_bound(g, t, x0, x1, y0, y1, z0, z1));
      dist[qi] = d;
      idx[qi] = at;
      open_flag[qi] = open ? 1 : 0;
    }
    const unsigned long long b = __ballot(open);
    if (lane_id() == 0 && b) atomicAdd(nr_open, (int)__popcll(b));
  }
}

// one thread per open query: shells of cells around its own cell (the cooperative pass searched shell 0 and 1 at least)
__global__ void __launch_bounds__(PSDF_BLOCK)
    nn_ring_kernel(Grid g, int64_t nq, const float* __restrict__ queries, const float* __restrict__ refs,
                   const int32_t* __restrict__ start, float max_dist, float* __restrict__ dist, int32_t* __restrict__ idx,
                   const uint8_t* __restrict__ open_flag) {
  const int64_t qi = (int64_t)blockIdx.x * PSDF_BLOCK + threadIdx.x;
  if (qi >= nq || !open_flag[qi]) return;
  const v3 q = ld3(queries + 3 * qi);
  if (!finite3(q)) return;
  Best best{__builtin_huge_valf(), idx[qi]};
  if (best.at >= 0) best.d2 = distance2(q, ld3(refs + 3 * (int64_t)best.at));
  const v3 t = cell_coords(g, q);
  const int cx = cell_index(t.x, g.nx), cy = cell_index(t.y, g.ny), cz = cell_index(t.z, g.nz);
  float d = dist[qi];
  int at = best.at;
  for (int k = 2; k <= plan::MAX_DIM; k++) {   // (k = the grid's longest side at the latest: every gap infinite)
    const int xa = max(cx - k, 0), xb = min(cx + k, g.nx - 1), ya = max(cy - k, 0), yb = min(cy + k, g.ny - 1);
    const int za = max(cz - k, 0), zb = min(cz + k, g.nz - 1);
    for (int x = xa; x <= xb; x++)
      for (int y = ya; y <= yb; y++) {
        const bool rim = abs(x - cx) == k || abs(y - cy) == k;
        if (rim) {   // the whole run along z
          const int last = start[cell_key(g, x, y, zb) + 1];
          for (int j = start[cell_key(g, x, y, za)]; j < last; j++) consider(best, q, ld3(refs + 3 * (int64_t)j), j);
        } else {     // the two caps, where they exist
          if (cz - k >= 0) {
            const int c = cell_key(g, x, y, cz - k), last = start[c + 1];
            for (int j = start[c]; j < last; j++) consider(best, q, ld3(refs + 3 * (int64_t)j), j);
          }
          if (cz + k <= g.nz - 1) {
            const int c = cell_key(g, x, y, cz + k), last = start[c + 1];
            for (int j = start[c]; j < last; j++) consider(best, q, ld3(refs + 3 * (int64_t)j), j);
          }
        }
      }
    answer(best, max_dist, d, at);
    // (a box that covers the grid has an infinite gap)
    if (d <= search_bound(g, t, cx - k, cx + k, cy - k, cy + k, cz - k, cz + k)) break;
  }
  dist[qi] = d;
  idx[qi] = at;
}

inline bool grid_of(const float* origin_edge, const int* dims, Grid& g) {
  if (!origin_edge || !dims) return false;
  g = Grid{origin_edge[0], origin_edge[1], origin_edge[2], origin_edge[3], dims[0], dims[1], dims[2]};
  if (!(g.edge > 0.f) || g.nx < 1 || g.ny < 1 || g.nz < 1 || g.nx > plan::MAX_DIM || g.ny > plan::MAX_DIM || g.nz > plan::MAX_DIM)
    return false;
  return (int64_t)g.nx * g.ny * g.nz <= plan::MAX_CELLS;
}
#define EVAL_GRID(n) dim3(psdf_blocks((n), PSDF_BLOCK)), dim3(PSDF_BLOCK), 0, (hipStream_t)stream

}  // namespace

extern "C" {

int psdf_mesh_eval_tile_capacity(void) { return plan::TILE_CAPACITY; }

int psdf_mesh_eval_grid_plan(const double* lo, const double* hi, int64_t n_points, double min_edge, int64_t cell_budget,
                             float* origin_edge, int* dims, int64_t* cells, int64_t* query_blocks) {
  if (!lo || !hi || !origin_edge || !dims || !cells) return PSDF_ERR_ARG;
  const plan::GridPlan p = plan::grid_plan(lo, hi, n_points, min_edge, cell_budget > 0 ? cell_budget : plan::DEFAULT_CELL_BUDGET);
  if (p.status != plan::PLAN_OK) return p.status;
  for (int a = 0; a < 3; a++) {
    origin_edge[a] = p.origin[a];
    dims[a] = p.dims[a];
  }
  origin_edge[3] = p.edge;
  *cells = p.cells;
  if (query_blocks) *query_blocks = plan::query_blocks(p.dims);
  return PSDF_OK;
}

int psdf_mesh_sample_count(const float* V, int64_t nV, const int32_t* F, int64_t nF, double density, int32_t* counts,
                           int32_t* overflow, void* stream) {
  if (nF < 0 || nV < 0 || !(density > 0.0)) return PSDF_ERR_ARG;
  if (nF == 0) return PSDF_OK;
  if (!V || !F || !counts || !overflow) return PSDF_ERR_ARG;
  if (nF > plan::MAX_POINTS || nV > plan::MAX_POINTS) return PSDF_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(sample_count_kernel, EVAL_GRID(nF), V, nV, F, nF, density, counts, overflow);
  PSDF_LAUNCH_CHECK();
  return PSDF_OK;
}

int psdf_mesh_sample_emit(const float* V, int64_t nV, const int32_t* F, int64_t nF, double density, const int64_t* incl,
                          float* samples, void* stream) {
  if (nF < 0 || nV < 0 || !(density > 0.0)) return PSDF_ERR_ARG;
  if (nF == 0) return PSDF_OK;
  if (!V || !F || !incl || !samples) return PSDF_ERR_ARG;
  if (nF > plan::MAX_POINTS || nV > plan::MAX_POINTS) return PSDF_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(sample_emit_kernel, EVAL_GRID(nF), V, nV, F, nF, density, incl, samples);
  PSDF_LAUNCH_CHECK();
  return PSDF_OK;
}

int psdf_mesh_eval_cell_keys(const float* points, int64_t n, const float* origin_edge, const int* dims, int block_log2,
                             int32_t* keys, void* stream) {
  if (n < 0) return PSDF_ERR_ARG;
  if (n == 0) return PSDF_OK;
  Grid g;
  if (!points || !keys || !grid_of(origin_edge, dims, g) || block_log2 < 0 || block_log2 > 4) return PSDF_ERR_ARG;
  if (n > plan::MAX_POINTS) return PSDF_ERR_UNSUPPORTED;
  const int round = (1 << block_log2) - 1;
  const int64_t sentinel = (int64_t)((g.nx + round) >> block_log2) * ((g.ny + round) >> block_log2) * ((g.nz + round) >> block_log2);
  hipLaunchKernelGGL(cell_keys_kernel, EVAL_GRID(n), g, block_log2, (int)sentinel, n, points, keys);
  PSDF_LAUNCH_CHECK();
  return PSDF_OK;
}

int psdf_mesh_eval_cell_ranges(const int32_t* sorted_keys, int64_t n, int64_t cells, int32_t* start, void* stream) {
  if (n < 0 || cells < 0 || cells > plan::MAX_CELLS) return PSDF_ERR_ARG;
  if (!start || (n > 0 && !sorted_keys)) return PSDF_ERR_ARG;
  if (n > plan::MAX_POINTS) return PSDF_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(cell_ranges_kernel, EVAL_GRID(cells + 1), cells, n, sorted_keys, start);
  PSDF_LAUNCH_CHECK();
  return PSDF_OK;
}

int psdf_mesh_thin_sweep(const float* points, const int32_t* rank, const int32_t* keys, int64_t n, const int32_t* cell_start,
                         const float* origin_edge, const int* dims, float radius, uint8_t* state, int32_t* undecided,
                         void* stream) {
  if (n < 0) return PSDF_ERR_ARG;
  if (n == 0) return PSDF_OK;
  Grid g;
  if (!points || !rank || !keys || !cell_start || !state || !undecided || !grid_of(origin_edge, dims, g)) return PSDF_ERR_ARG;
  // the 27 neighbouring cells hold every point within the radius only if a cell is wider than the radius
  if (!(radius >= 0.f) || !((double)g.edge >= (double)radius * plan::EDGE_MARGIN)) return PSDF_ERR_ARG;
  if (n > plan::MAX_POINTS) return PSDF_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(thin_sweep_kernel, EVAL_GRID(n), g, n, points, rank, keys, cell_start, radius, g.nx * g.ny * g.nz, state,
                     undecided);
  PSDF_LAUNCH_CHECK();
  return PSDF_OK;
}

int psdf_mesh_nn_cooperative(const float* queries, int64_t nq, const int32_t* query_block_start, const float* refs, int64_t nr,
                             const int32_t* cell_start, const float* origin_edge, const int* dims, float max_dist, float* dist,
                             int32_t* idx, uint8_t* open, int32_t* nr_open, void* stream) {
  if (nq < 0 || nr < 0) return PSDF_ERR_ARG;
  if (nq == 0) return PSDF_OK;
  Grid g;
  if (!queries || !query_block_start || !cell_start || !dist || !idx || !open || !nr_open || (nr > 0 && !refs) ||
      !grid_of(origin_edge, dims, g) || !(max_dist >= 0.f))
    return PSDF_ERR_ARG;
  if (nq > plan::MAX_POINTS || nr > plan::MAX_POINTS) return PSDF_ERR_UNSUPPORTED;
  const int nby = plan::blocks_of(g.ny), nbz = plan::blocks_of(g.nz);
  const int64_t blocks = plan::query_blocks(dims);
  hipLaunchKernelGGL(nn_cooperative_kernel, dim3((unsigned)blocks), dim3(PSDF_BLOCK), 0, (hipStream_t)stream, g, nby, nbz, queries,
                     query_block_start, refs, cell_start, max_dist, dist, idx, open, nr_open);
  PSDF_LAUNCH_CHECK();
  return PSDF_OK;
}

int psdf_mesh_nn_ring(const float* queries, int64_t nq, const float* refs, int64_t nr, const int32_t* cell_start,
                      const float* origin_edge, const int* dims, float max_dist, float* dist, int32_t* idx, const uint8_t* open,
                      void* stream) {
  if (nq < 0 || nr < 0) return PSDF_ERR_ARG;
  if (nq == 0) return PSDF_OK;
  Grid g;
  if (!queries || !cell_start || !dist || !idx || !open || (nr > 0 && !refs) || !grid_of(origin_edge, dims, g) ||
      !(max_dist >= 0.f))
    return PSDF_ERR_ARG;
  if (nq > plan::MAX_POINTS || nr > plan::MAX_POINTS) return PSDF_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(nn_ring_kernel, EVAL_GRID(nq), g, nq, queries, refs, cell_start, max_dist, dist, idx, open);
  PSDF_LAUNCH_CHECK();
  return PSDF_OK;
}

}  // extern "C"
