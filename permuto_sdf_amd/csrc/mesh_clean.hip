// Mesh cleaning for gfx950: what the reference does to an extracted mesh between extraction and scoring, on tensors the mesh
// extractor leaves on the device.  permuto_sdf_py/experiments/evaluation/evaluate_chamfer_distance.py:110-167
// (clean_points_by_mask, clean_mesh -- NeuS's protocol for scenes trained without masks) projects every vertex into every training
// view, drops a vertex that falls outside any view's mask dilated by a 101 x 101 ellipse, drops the faces that lost a vertex,
// renumbers, and keeps the largest connected component.
//
//   (a) row distance: hd[y, x] = distance along the row to the nearest set pixel (value > threshold), a byte saturated at 255.
//       One wave per row, 64 pixels per step, one sweep from each side: the ballot of the set pixels gives every lane its nearest
//       set pixel inside the step by a count of leading / trailing zeros, and the nearest one of the steps already swept is a
//       value the whole wave carries.  No per-pixel search.
//   (b) span dilation: the structuring element is a stack of centred row spans (half-width hw[k] in row k - r), so pixel (y, x)
//       is set iff hd[y + dy, x] <= hw[dy + r] for some dy with y + dy inside the image.  A workgroup stages the row distances of
//       its tile and r rows of halo above and below in LDS (mesh_clean_plan.h decides the rows), every lane owns one column and
//       walks the 2 r + 1 rows, and the wave's ballot IS the two packed words of the output: no atomics, padding bits zero.
//       Outside the image nothing is set (cv.dilate's default border): it is staged as "far".  While staging, every wave notes
//       which rows hold, in its 64 columns, a distance within the widest span at all; the walk skips groups of eight rows
//       without one and reads the eight rows of the others in one batch.
//   (c) vertex test: one lane per vertex, the views in the outer loop.  p = ((P0 x + P1 y) + P2 z) + P3 per row in float64,
//       u = p0 / p2, v = p1 / p2 rounded half to even; inside the image the view keeps the vertex iff bit (v, u) of its dilated
//       mask is set, outside it (and for a non-finite u or v) the view keeps it.  The view's matrix is read at a wave-uniform
//       address; a culled vertex's lane idles and the wave leaves the loop when no lane is alive.  One wave per workgroup: the
//       exit is then uniform over the workgroup too.
//   (d) filter: a face survives iff its three vertices do (count), the caller scans, then vertices and faces are written at
//       their ranks, old order preserved.
//   (e) components: 3 nF half-edge keys (min << 32 | max), the caller's sort, and a union of the two faces of every run of
//       exactly two equal keys; or, for vertex connectivity, a union of every face's vertices.  The union-find hooks the larger
//       root under the smaller by compare-and-swap, so parent[i] <= i at all times, every walk descends, and the root of a
//       component is its smallest index whatever the thread order: the labels are deterministic.  Every loop carries a cap
//       (mesh_clean_plan.h) and raises a flag on exceeding it instead of spinning.
//
// The entries allocate nothing and never synchronise; sorts and scans are the caller's.
#include "psdf_common.h"
#include "mesh_clean_plan.h"
#include "../../include/psdf.h"

using namespace psdf;
namespace cplan = psdf::mesh_clean_plan;

namespace {

enum : int32_t { FLAG_BAD_INDEX = 2, FLAG_NO_END = 4 };
static_assert(PSDF_BLOCK == cplan::TILE_COLS && PSDF_BLOCK == cplan::ROWS_PER_GROUP * PSDF_WAVE, "one lane per tile column");

// ---- (a) row distance ------------------------------------------------------------------------------------------------------
constexpr int FAR_LEFT = -(1 << 29);    // "no set pixel yet": further than any saturated distance from every column
constexpr int FAR_RIGHT = INT32_MAX;

__global__ void __launch_bounds__(PSDF_BLOCK)
    row_distance_kernel(const uint8_t* __restrict__ src, int64_t rows, int W, int threshold, uint8_t* __restrict__ hd) {
  const int lane = lane_id();
  const int64_t row = (int64_t)blockIdx.x * cplan::ROWS_PER_GROUP + (threadIdx.x >> 6);
  const bool row_ok = row < rows;   // (a wave past the last row still votes: the steps are uniform over the workgroup)
  const uint8_t* in = src + (row_ok ? row : 0) * W;
  uint8_t* out = hd + (row_ok ? row : 0) * W;
  const int steps = (W + 63) >> 6;
  int last = FAR_LEFT;    // left to right: the nearest set pixel of the steps already swept
  for (int s = 0; s < steps; s++) {
    const int x = (s << 6) + lane;
    const bool ok = row_ok && x < W;
    const bool set = ok && (int)in[x] > threshold;
    const unsigned long long m = __ballot(set);
    const unsigned long long below = m & (~0ull >> (63 - lane));   // bits 0 .. lane
    const int at = below ? (s << 6) + 63 - __builtin_clzll(below) : last;
    const int64_t d = (int64_t)x - at;
    if (ok) out[x] = (uint8_t)(d < cplan::HD_FAR ? d : cplan::HD_FAR);
    if (m) last = (s << 6) + 63 - __builtin_clzll(m);
  }
  int next = FAR_RIGHT;   // right to left, over what the first sweep wrote: a set pixel is a distance of 0
  for (int s = steps - 1; s >= 0; s--) {
    const int x = (s << 6) + lane;
    const bool ok = row_ok && x < W;
    const int left = ok ? (int)out[x] : cplan::HD_FAR;
    const unsigned long long m = __ballot(ok && left == 0);
    const unsigned long long above = m >> lane;                    // bits lane .. 63
    const int at = above ? x + __builtin_ctzll(above) : next;
    const int64_t d = (int64_t)at - x;
    if (ok && d < left) out[x] = (uint8_t)d;
    if (m) next = (s << 6) + __builtin_ctzll(m);
  }
}

// ---- (b) span dilation -----------------------------------------------------------------------------------------------------
struct Spans {
  unsigned long long words[cplan::LDS_ROWS / 8];   // the half-widths, one byte per row of the element, eight to a word
};
constexpr int STAGE_BATCH = 16;

// a value every lane of the wave holds, moved to scalar registers: what is branched on with it is a scalar branch
__device__ __forceinline__ unsigned long long wave_uniform(unsigned long long v) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
  return ((unsigned long long)hi << 32) | lo;
}

__global__ void __launch_bounds__(PSDF_BLOCK)
    dilate_kernel(const uint8_t* __restrict__ hd, int H, int W, int radius, int widest, int tile_rows, int tiles_x, int tiles_y,
                  int words_per_row, Spans spans, int32_t* __restrict__ words) {
  __shared__ uint8_t tile[cplan::LDS_BYTES];
  // bit k & 63 of live[wave][k >> 6]: staged row k holds, in the wave's 64 columns, a distance some row of the element accepts.
  // A mask is mostly far from its object: the walk below skips groups of eight rows without a live one.
  __shared__ unsigned long long live[cplan::ROWS_PER_GROUP][cplan::LIVE_WORDS];
  __shared__ unsigned long long spans_lds[cplan::LDS_ROWS / 8];   // (read at per-lane addresses below: not from the arguments)
  const int tid = (int)threadIdx.x, wave = tid >> 6;
#pragma unroll
  for (int i = 0; i < cplan::LDS_ROWS / 8; i++) {
    const unsigned long long w = spans.words[i];   // a uniform index: scalar loads
    if (tid == i) spans_lds[i] = w;
  }
  int64_t b = blockIdx.x;
  const int tx = (int)(b % tiles_x);
  b /= tiles_x;
  const int ty = (int)(b % tiles_y);
  const int64_t view = b / tiles_y;
  const int x = tx * cplan::TILE_COLS + tid, y0 = ty * tile_rows;
  const uint8_t* image = hd + view * H * W;
  const int staged = tile_rows + 2 * radius;   // <= LDS_ROWS (the plan)
  // STAGE_BATCH loads are issued before the first of them is used: one trip to memory per batch, not per row
  unsigned long long rows = 0;
  for (int k0 = 0; k0 < staged; k0 += STAGE_BATCH) {
    uint8_t d[STAGE_BATCH];
#pragma unroll
    for (int j = 0; j < STAGE_BATCH; j++) {
      const int y = y0 - radius + k0 + j;
      d[j] = (k0 + j < staged && y >= 0 && y < H && x < W) ? image[(int64_t)y * W + x] : (uint8_t)cplan::HD_FAR;
    }
#pragma unroll
    for (int j = 0; j < STAGE_BATCH; j++) {
      const int k = k0 + j;
      if (k >= staged) break;   // (uniform)
      tile[k * cplan::TILE_COLS + tid] = d[j];
      if (__ballot((int)d[j] <= widest)) rows |= 1ull << (k & 63);
      if ((k & 63) == 63 || k == staged - 1) {
        if (lane_id() == 0) live[wave][k >> 6] = rows;
        rows = 0;
      }
    }
  }
  for (int c = ((staged - 1) >> 6) + 1; c < cplan::LIVE_WORDS; c++)
    if (lane_id() == 0) live[wave][c] = 0;   // (read, never used: the rows past the staged ones)
  __syncthreads();
  const int word = (tx * cplan::TILE_COLS + (tid & ~63)) >> 5;   // the wave's first packed word of the row
  const int element_rows = 2 * radius + 1;
  for (int t = 0; t < tile_rows; t++) {
    const int y = y0 + t;   // (y >= H in the last tile: nobody votes, nothing is written)
    const bool mine = y < H && x < W;
    bool hit = false;
    for (int k0 = 0; k0 < element_rows && y < H; k0 += 8) {
      // the live bits of the staged rows t + k0 .. t + k0 + 7 (those past the element's last row are masked off)
      const int s0 = t + k0, c = s0 >> 6, o = s0 & 63;
      unsigned long long any = live[wave][c] >> o;
      if (o > 56 && c + 1 < cplan::LIVE_WORDS) any |= live[wave][c + 1] << (64 - o);
      const int left = element_rows - k0;   // rows of the element in this group, when fewer than eight
      any &= left >= 8 ? 0xffull : (1ull << left) - 1;
      if (!wave_uniform(any)) continue;
      if (!mine || hit) continue;
      const unsigned long long h8 = spans_lds[k0 >> 3];
#pragma unroll
      for (int j = 0; j < 8; j++) {   // eight independent reads; a row past the element repeats the last one and is ignored
        const int s = s0 + (j < left ? j : left - 1);
        const bool in = tile[s * cplan::TILE_COLS + tid] <= (uint8_t)(h8 >> (8 * j));
        hit |= in && j < left;
      }
    }
    const unsigned long long bits = __ballot(hit);
    if (lane_id() == 0 && y < H) {
      int32_t* row = words + (view * H + y) * words_per_row;
      if (word < words_per_row) row[word] = (int32_t)(uint32_t)(bits & 0xffffffffull);
      if (word + 1 < words_per_row) row[word + 1] = (int32_t)(uint32_t)(bits >> 32);
    }
  }
}

// ---- (c) vertex test -------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(PSDF_WAVE)
    inside_masks_kernel(const float* __restrict__ V, int64_t nV, const double* __restrict__ mats, int views,
                        const int32_t* __restrict__ words, int H, int W, int words_per_row, uint8_t* __restrict__ keep) {
  const int64_t i = (int64_t)blockIdx.x * PSDF_WAVE + threadIdx.x;
  bool live = i < nV;
  double x = 0, y = 0, z = 0;
  if (live) x = (double)V[3 * i], y = (double)V[3 * i + 1], z = (double)V[3 * i + 2];
  for (int view = 0; view < views; view++) {
    if (!__ballot(live)) break;
    if (!live) continue;
    const double* P = mats + 12 * (int64_t)view;
    const double p0 = ((P[0] * x + P[1] * y) + P[2] * z) + P[3];
    const double p1 = ((P[4] * x + P[5] * y) + P[6] * z) + P[7];
    const double p2 = ((P[8] * x + P[9] * y) + P[10] * z) + P[11];
    const double u = p0 / p2, v = p1 / p2;
    if (!isfinite(u) || !isfinite(v)) continue;   // outside every image: kept by this view
    const double ru = rint(u), rv = rint(v);      // half to even
    if (!(ru >= 0.0 && ru < (double)W && rv >= 0.0 && rv < (double)H)) continue;
    const int xi = (int)ru, yi = (int)rv;
    const uint32_t w = (uint32_t)words[((int64_t)view * H + yi) * words_per_row + (xi >> 5)];
    live = (w >> (xi & 31)) & 1u;
  }
  if (i < nV) keep[i] = live ? 1 : 0;
}

// ---- (d) filter ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool face_in_range(const int32_t* __restrict__ F, int64_t f, int64_t nV, int& a, int& b, int& c) {
  a = F[3 * f], b = F[3 * f + 1], c = F[3 * f + 2];
  return a >= 0 && b >= 0 && c >= 0 && a < nV && b < nV && c < nV;
}

__global__ void __launch_bounds__(PSDF_BLOCK)
    face_keep_kernel(const int32_t* __restrict__ F, int64_t nF, const uint8_t* __restrict__ keep, int64_t nV,
                     const uint8_t* __restrict__ face_mask, uint8_t* __restrict__ face_keep, int32_t* flag) {
  const int64_t f = (int64_t)blockIdx.x * PSDF_BLOCK + threadIdx.x;
  if (f >= nF) return;
  int a, b, c;
  uint8_t k = 0;
  if (!face_in_range(F, f, nV, a, b, c)) atomicOr(flag, FLAG_BAD_INDEX);
  else k = keep[a] && keep[b] && keep[c] && (!face_mask || face_mask[f]);
  face_keep[f] = k;
}

// incl: the caller's inclusive scan of keep; a kept vertex moves to row incl - 1
__global__ void __launch_bounds__(PSDF_BLOCK)
    emit_vertices_kernel(int64_t nV, const uint8_t* __restrict__ keep, const int32_t* __restrict__ incl, const float* __restrict__ V,
                         const float* __restrict__ NV, const int64_t* __restrict__ edges, float* __restrict__ V_out,
                         float* __restrict__ NV_out, int64_t* __restrict__ edges_out, int32_t* __restrict__ vertex_map) {
  const int64_t i = (int64_t)blockIdx.x * PSDF_BLOCK + threadIdx.x;
  if (i >= nV) return;
  if (!keep[i]) {
    vertex_map[i] = -1;
    return;
  }
  const int64_t at = (int64_t)incl[i] - 1;
  vertex_map[i] = (int32_t)at;
  st3(V_out + 3 * at, ld3(V + 3 * i));
  if (NV) st3(NV_out + 3 * at, ld3(NV + 3 * i));
  if (edges) edges_out[2 * at] = edges[2 * i], edges_out[2 * at + 1] = edges[2 * i + 1];
}

__global__ void __launch_bounds__(PSDF_BLOCK)
    emit_faces_kernel(const int32_t* __restrict__ F, int64_t nF, const uint8_t* __restrict__ face_keep, const int32_t* __restrict__ incl,
                      const int32_t* __restrict__ vertex_map, int32_t* __restrict__ F_out) {
  const int64_t f = (int64_t)blockIdx.x * PSDF_BLOCK + threadIdx.x;
  if (f >= nF || !face_keep[f]) return;   // (a kept face names vertices in range: face_keep_kernel)
  const int64_t at = (int64_t)incl[f] - 1;
#pragma unroll
  for (int k = 0; k < 3; k++) F_out[3 * at + k] = vertex_map[F[3 * f + k]];
}

// ---- (e) components --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int load_parent(const int32_t* parent, int i) { return __atomic_load_n(parent + i, __ATOMIC_RELAXED); }

// the root of i: parents descend, so the walk ends within i + 1 steps; then the path is pointed at the root (atomicMin: a parent
// only ever moves to a smaller member of the same component)
__device__ __forceinline__ int find_root(int32_t* parent, int i, int64_t cap, int32_t* flag) {
  int r = i;
  int64_t it = 0;
  for (; it < cap; it++) {
    const int p = load_parent(parent, r);
    if (p >= r) break;   // p == r: the root (p > r cannot be: the cap below reports a broken structure as well)
    r = p;
  }
  if (it >= cap || load_parent(parent, r) > r) {
    atomicOr(flag, FLAG_NO_END);
    return r;
  }
  for (it = 0; i > r && it < cap; it++) {
    const int p = load_parent(parent, i);
    if (p > r) atomicMin(parent + i, r);
    if (p >= i) break;
    i = p;
  }
  return r;
}

__device__ __forceinline__ void unite(int32_t* parent, int a, int b, int64_t cap, int32_t* flag) {
  for (int64_t it = 0; it < cap; it++) {
    a = find_root(parent, a, cap, flag);
    b = find_root(parent, b, cap, flag);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    if (atomicCAS(parent + a, a, b) == a) return;   // a was still a root: hooked under the smaller root
  }
  atomicOr(flag, FLAG_NO_END);
}

__global__ void __launch_bounds__(PSDF_BLOCK)
    edge_keys_kernel(const int32_t* __restrict__ F, int64_t nF, int64_t nV, int64_t* __restrict__ keys, int32_t* flag) {
  const int64_t f = (int64_t)blockIdx.x * PSDF_BLOCK + threadIdx.x;
  if (f >= nF) return;
  int v[3];
  if (!face_in_range(F, f, nV, v[0], v[1], v[2])) atomicOr(flag, FLAG_BAD_INDEX);
#pragma unroll
  for (int e = 0; e < 3; e++) {
    const int a = v[e], b = v[(e + 1) % 3];
    const int lo = a < b ? a : b, hi = a < b ? b : a;
    keys[3 * f + e] = (int64_t)(((uint64_t)(uint32_t)lo << 32) | (uint32_t)hi);
  }
}

// sorted [n]: the keys in ascending order; slot [n]: where each came from (3 f + e: the face is slot / 3)
__global__ void __launch_bounds__(PSDF_BLOCK)
    link_edges_kernel(const int64_t* __restrict__ sorted, const int64_t* __restrict__ slot, int64_t n, int32_t* parent, int64_t cap,
                      int32_t* flag) {
  const int64_t i = (int64_t)blockIdx.x * PSDF_BLOCK + threadIdx.x;
  if (i + 1 >= n) return;
  const int64_t key = sorted[i];
  if (sorted[i + 1] != key) return;
  if (i > 0 && sorted[i - 1] == key) return;       // not the start of its run
  if (i + 2 < n && sorted[i + 2] == key) return;   // a run of three or more: the edge links nothing
  if ((key >> 32) == (key & 0xffffffffll)) return; // both endpoints equal
  const int64_t fa = slot[i] / 3, fb = slot[i + 1] / 3;
  if (fa < 0 || fb < 0 || fa >= n / 3 || fb >= n / 3) {
    atomicOr(flag, FLAG_BAD_INDEX);
    return;
  }
  unite(parent, (int)fa, (int)fb, cap, flag);
}

__global__ void __launch_bounds__(PSDF_BLOCK)
    link_vertices_kernel(const int32_t* __restrict__ F, int64_t nF, int64_t nV, int32_t* parent, int64_t cap, int32_t* flag) {
  const int64_t f = (int64_t)blockIdx.x * PSDF_BLOCK + threadIdx.x;
  if (f >= nF) return;
  int a, b, c;
  if (!face_in_range(F, f, nV, a, b, c)) {
    atomicOr(flag, FLAG_BAD_INDEX);
    return;
  }
  unite(parent, a, b, cap, flag);
  unite(parent, a, c, cap, flag);
}

// sizes[label] += 1 for every valid thread of the workgroup (all of its threads call this).  A mesh is mostly one component, and
// one atomic per face on that component's counter serialises (16 ms for 1.4 x 10^6 faces, measured): the threads that share
// thread 0's label are counted by ballot into LDS and added once per workgroup; the others add by themselves.
__device__ __forceinline__ void count_label(int32_t* sizes, int label, bool valid) {
  __shared__ int32_t group_label, group_count;
  if (threadIdx.x == 0) group_label = valid ? label : -1, group_count = 0;
  __syncthreads();
  const bool same = valid && label == group_label;
  const unsigned long long votes = __ballot(same);
  if (lane_id() == 0 && votes) atomicAdd(&group_count, (int)__popcll(votes));
  __syncthreads();
  if (threadIdx.x == 0 && group_count > 0) atomicAdd(sizes + group_label, group_count);
  if (valid && !same) atomicAdd(sizes + label, 1);
}

__global__ void __launch_bounds__(PSDF_BLOCK)
    flatten_kernel(int32_t* parent, int64_t n, int64_t cap, int32_t* __restrict__ labels, int32_t* sizes, int32_t* flag) {
  const int64_t i = (int64_t)blockIdx.x * PSDF_BLOCK + threadIdx.x;
  int r = -1;
  if (i < n) labels[i] = r = find_root(parent, (int)i, cap, flag);
  if (sizes) count_label(sizes, r, i < n);   // (sizes is uniform: the whole workgroup calls it or none of it)
}

// vertex connectivity: the smallest face of every vertex component, then every face's label
__global__ void __launch_bounds__(PSDF_BLOCK)
    face_min_kernel(const int32_t* __restrict__ F, int64_t nF, int64_t nV, const int32_t* __restrict__ vertex_label, int32_t* first_face) {
  const int64_t f = (int64_t)blockIdx.x * PSDF_BLOCK + threadIdx.x;
  int a, b, c;
  if (f >= nF || !face_in_range(F, f, nV, a, b, c)) return;
  atomicMin(first_face + vertex_label[a], (int)f);
}

__global__ void __launch_bounds__(PSDF_BLOCK)
    face_labels_kernel(const int32_t* __restrict__ F, int64_t nF, int64_t nV, const int32_t* __restrict__ vertex_label,
                       const int32_t* __restrict__ first_face, int32_t* __restrict__ labels, int32_t* sizes) {
  const int64_t f = (int64_t)blockIdx.x * PSDF_BLOCK + threadIdx.x;
  int a, b, c;
  int label = (int)f;   // (a face out of range: the caller raises on the flag)
  if (f < nF) {
    if (face_in_range(F, f, nV, a, b, c)) label = first_face[vertex_label[a]];
    if (label < 0 || label >= nF) label = (int)f;
    labels[f] = label;
  }
  count_label(sizes, label, f < nF);
}

#define CLEAN_GRID(n) dim3(psdf_blocks((n), PSDF_BLOCK)), dim3(PSDF_BLOCK), 0, (hipStream_t)stream

}  // namespace

extern "C" {

int psdf_mesh_clean_dilate_plan(int64_t n, int64_t H, int64_t W, const int* half_widths, int64_t count, int64_t* out) {
  if (!out) return PSDF_ERR_ARG;
  const cplan::DilatePlan p = cplan::dilate_plan(n, H, W, half_widths, count);
  if (p.status != cplan::PLAN_OK) return p.status;
  out[0] = p.radius, out[1] = p.tile_rows, out[2] = p.staged_rows, out[3] = p.tiles_x, out[4] = p.tiles_y;
  out[5] = p.words_per_row, out[6] = p.workgroups, out[7] = p.row_groups, out[8] = cplan::LDS_BYTES + cplan::LIVE_BYTES;
  return PSDF_OK;
}

int64_t psdf_mesh_clean_union_find_cap(int64_t n) { return cplan::union_find_cap(n); }

int psdf_mesh_clean_row_distance(const uint8_t* masks, int64_t n, int H, int W, int threshold, uint8_t* hd, void* stream) {
  if (n < 0) return PSDF_ERR_ARG;
  if (n == 0) return PSDF_OK;
  const int one = 0;
  const cplan::DilatePlan p = cplan::dilate_plan(n, H, W, &one, 1);
  if (p.status != cplan::PLAN_OK) return p.status;
  if (!masks || !hd || threshold < 0 || threshold > 255) return PSDF_ERR_ARG;
  hipLaunchKernelGGL(row_distance_kernel, dim3((unsigned)p.row_groups), dim3(PSDF_BLOCK), 0, (hipStream_t)stream, masks, n * H, W,
                     threshold, hd);
  PSDF_LAUNCH_CHECK();
  return PSDF_OK;
}

int psdf_mesh_clean_dilate(const uint8_t* hd, int64_t n, int H, int W, const int* half_widths, int count, int32_t* words,
                           void* stream) {
  if (n < 0) return PSDF_ERR_ARG;
  if (n == 0) return PSDF_OK;
  const cplan::DilatePlan p = cplan::dilate_plan(n, H, W, half_widths, count);
  if (p.status != cplan::PLAN_OK) return p.status;
  if (!hd || !words) return PSDF_ERR_ARG;
  Spans spans{};
  int widest = 0;
  for (int k = 0; k < count; k++) {
    spans.words[k >> 3] |= (unsigned long long)half_widths[k] << (8 * (k & 7));
    if (half_widths[k] > widest) widest = half_widths[k];
  }
  hipLaunchKernelGGL(dilate_kernel, dim3((unsigned)p.workgroups), dim3(PSDF_BLOCK), 0, (hipStream_t)stream, hd, H, W, p.radius,
                     widest, p.tile_rows, p.tiles_x, p.tiles_y, p.words_per_row, spans, words);
  PSDF_LAUNCH_CHECK();
  return PSDF_OK;
}

int psdf_mesh_clean_inside_masks(const float* V, int64_t nV, const double* world_mats, int views, const int32_t* words, int H,
                                 int W, uint8_t* keep, void* stream) {
  if (nV < 0 || views < 0) return PSDF_ERR_ARG;
  if (nV == 0) return PSDF_OK;
  if (!V || !keep || (views > 0 && (!world_mats || !words || H < 1 || W < 1))) return PSDF_ERR_ARG;
  if (nV > cplan::MAX_COUNT) return PSDF_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(inside_masks_kernel, dim3(psdf_blocks(nV, PSDF_WAVE)), dim3(PSDF_WAVE), 0, (hipStream_t)stream, V, nV, world_mats,
                     views, words, H, W, (W + 31) / 32, keep);
  PSDF_LAUNCH_CHECK();
  return PSDF_OK;
}

int psdf_mesh_clean_face_keep(const int32_t* F, int64_t nF, const uint8_t* keep, int64_t nV, const uint8_t* face_mask,
                              uint8_t* face_keep, int32_t* flag, void* stream) {
  if (nF < 0 || nV < 0) return PSDF_ERR_ARG;
  if (nF == 0) return PSDF_OK;
  if (!F || !face_keep || !flag || (nV > 0 && !keep)) return PSDF_ERR_ARG;
  if (nF > cplan::MAX_COUNT || nV > cplan::MAX_COUNT) return PSDF_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(face_keep_kernel, CLEAN_GRID(nF), F, nF, keep, nV, face_mask, face_keep, flag);
  PSDF_LAUNCH_CHECK();
  return PSDF_OK;
}

int psdf_mesh_clean_emit_vertices(int64_t nV, const uint8_t* keep, const int32_t* incl, const float* V, const float* NV,
                                  const int64_t* edges, float* V_out, float* NV_out, int64_t* edges_out, int32_t* vertex_map,
                                  void* stream) {
  if (nV < 0) return PSDF_ERR_ARG;
  if (nV == 0) return PSDF_OK;
  if (!keep || !incl || !V || !V_out || !vertex_map || (NV && !NV_out) || (edges && !edges_out)) return PSDF_ERR_ARG;
  if (nV > cplan::MAX_COUNT) return PSDF_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(emit_vertices_kernel, CLEAN_GRID(nV), nV, keep, incl, V, NV, edges, V_out, NV_out, edges_out, vertex_map);
  PSDF_LAUNCH_CHECK();
  return PSDF_OK;
}

int psdf_mesh_clean_emit_faces(const int32_t* F, int64_t nF, const uint8_t* face_keep, const int32_t* incl,
                               const int32_t* vertex_map, int32_t* F_out, void* stream) {
  if (nF < 0) return PSDF_ERR_ARG;
  if (nF == 0) return PSDF_OK;
  if (!F || !face_keep || !incl || !vertex_map || !F_out) return PSDF_ERR_ARG;
  if (nF > cplan::MAX_COUNT) return PSDF_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(emit_faces_kernel, CLEAN_GRID(nF), F, nF, face_keep, incl, vertex_map, F_out);
  PSDF_LAUNCH_CHECK();
  return PSDF_OK;
}

int psdf_mesh_clean_edge_keys(const int32_t* F, int64_t nF, int64_t nV, int64_t* keys, int32_t* flag, void* stream) {
  if (nF < 0 || nV < 0) return PSDF_ERR_ARG;
  if (nF == 0) return PSDF_OK;
  if (!F || !keys || !flag) return PSDF_ERR_ARG;
  if (nF > cplan::MAX_COUNT / 3 || nV > cplan::MAX_COUNT) return PSDF_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(edge_keys_kernel, CLEAN_GRID(nF), F, nF, nV, keys, flag);
  PSDF_LAUNCH_CHECK();
  return PSDF_OK;
}

int psdf_mesh_clean_link_edges(const int64_t* sorted_keys, const int64_t* slot, int64_t nF, int32_t* parent, int32_t* flag,
                               void* stream) {
  if (nF < 0) return PSDF_ERR_ARG;
  if (nF == 0) return PSDF_OK;
  if (!sorted_keys || !slot || !parent || !flag) return PSDF_ERR_ARG;
  if (nF > cplan::MAX_COUNT / 3) return PSDF_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(link_edges_kernel, CLEAN_GRID(3 * nF), sorted_keys, slot, 3 * nF, parent, cplan::union_find_cap(nF), flag);
  PSDF_LAUNCH_CHECK();
  return PSDF_OK;
}

int psdf_mesh_clean_link_vertices(const int32_t* F, int64_t nF, int64_t nV, int32_t* parent, int32_t* flag, void* stream) {
  if (nF < 0 || nV < 0) return PSDF_ERR_ARG;
  if (nF == 0) return PSDF_OK;
  if (!F || !flag || (nV > 0 && !parent)) return PSDF_ERR_ARG;
  if (nF > cplan::MAX_COUNT || nV > cplan::MAX_COUNT) return PSDF_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(link_vertices_kernel, CLEAN_GRID(nF), F, nF, nV, parent, cplan::union_find_cap(nV), flag);
  PSDF_LAUNCH_CHECK();
  return PSDF_OK;
}

int psdf_mesh_clean_flatten(int32_t* parent, int64_t n, int32_t* labels, int32_t* sizes, int32_t* flag, void* stream) {
  if (n < 0) return PSDF_ERR_ARG;
  if (n == 0) return PSDF_OK;
  if (!parent || !labels || !flag) return PSDF_ERR_ARG;
  if (n > cplan::MAX_COUNT) return PSDF_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(flatten_kernel, CLEAN_GRID(n), parent, n, cplan::union_find_cap(n), labels, sizes, flag);
  PSDF_LAUNCH_CHECK();
  return PSDF_OK;
}

int psdf_mesh_clean_face_labels(const int32_t* F, int64_t nF, int64_t nV, const int32_t* vertex_label, int32_t* first_face,
                                int32_t* labels, int32_t* sizes, void* stream) {
  if (nF < 0 || nV < 0) return PSDF_ERR_ARG;
  if (nF == 0) return PSDF_OK;
  if (!F || !labels || !sizes || (nV > 0 && (!vertex_label || !first_face))) return PSDF_ERR_ARG;
  if (nF > cplan::MAX_COUNT || nV > cplan::MAX_COUNT) return PSDF_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(face_min_kernel, CLEAN_GRID(nF), F, nF, nV, vertex_label, first_face);
  PSDF_LAUNCH_CHECK();
  hipLaunchKernelGGL(face_labels_kernel, CLEAN_GRID(nF), F, nF, nV, vertex_label, first_face, labels, sizes);
  PSDF_LAUNCH_CHECK();
  return PSDF_OK;
}

}  // extern "C"
