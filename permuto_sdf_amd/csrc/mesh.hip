// Mesh extraction for gfx950: marching tetrahedra over a scalar field sampled on a regular grid, streamed by slabs of x-planes.
//
// The contract is the algorithm compat/skimage/measure.py freezes (tables: mesh_tables.h), so the two compare index for index:
//   * volume [X, Y, Z] fp32, Z fastest; v = vol - level in fp32; a sample is inside iff v < 0 (NaN and -0.0 are outside);
//   * one vertex on every grid edge whose ends differ in `inside`; an edge is owned by its component-wise lower end and falls
//     into one of seven direction classes d (mesh_tables.h); vertices are welded by edge, never by position, and numbered by
//     (owner's linear index, d) -- which is the (lo, hi) order of the stand-in's sorted edge keys;
//   * position in index coordinates, fp32: t = f_lo / (f_lo - f_hi), p = p_lo + (p_hi - p_lo) * t;
//   * faces by (cell, tetrahedron, triangle), winding from the table.
// No pass orders its output with an atomic counter: counts -> prefix sums (the caller's) -> emission at the scanned offsets, so
// the order is a function of the inputs alone.
//
// Buffers.  Per-point buffers (vol, valid, mask, vincl) hold `nplanes` consecutive x-planes starting at global plane `xbase`;
// a caller that streams keeps two planes of overlap and moves them to the front between slabs.  `vincl` is the INCLUSIVE scan
// of the per-point vertex counts plus the number of vertices of all earlier slabs (global vertex ids); a vertex id is
// vincl - popc(mask) + popc(mask & ((1 << d) - 1)): 5 bytes per grid point.  Faces of cell plane x read mask / vincl of the vertex
// planes x and x + 1, which is why a streaming caller emits the faces one plane behind the vertices.
// Sparse mode: `valid` [same layout, bytes, NULL = all valid] marks the points that were evaluated; an edge exists only between
// two valid points and a cell only if its eight corners are valid -- the value of an invalid point is never read.
//
// Every kernel is one thread per grid point (lanes along z, coalesced): the 2x2x2 neighbourhood of a point is read straight from
// global memory, where the seven neighbours of a wave are the wave's own lines or the next row's (L2 hits).  The passes are
// bandwidth-light next to the field evaluation that feeds them.
#include "psdf_common.h"
#define PSDF_MT_TABLE __device__ static const
#include "mesh_tables.h"
#include "../../include/psdf.h"

using namespace psdf;

namespace {

struct Slab {
  int X, Y, Z;   // global extent
  int xbase;     // global x of the first plane the buffers hold
  int nplanes;
  __device__ __forceinline__ int64_t slot(int x, int y, int z) const { return ((int64_t)(x - xbase) * Y + y) * Z + z; }
};

__device__ __forceinline__ bool ok(const uint8_t* valid, int64_t i) { return valid == nullptr || valid[i] != 0; }

// thread -> (x, y, z) of plane range [a, b); false past the end
__device__ __forceinline__ bool point_of_thread(const Slab& s, int a, int b, int& x, int& y, int& z, int64_t& rel) {
  rel = (int64_t)blockIdx.x * PSDF_BLOCK + threadIdx.x;
  const int64_t plane = (int64_t)s.Y * s.Z;
  if (rel >= (int64_t)(b - a) * plane) return false;
  x = a + (int)(rel / plane);
  const int r = (int)(rel % plane);
  y = r / s.Z;
  z = r % s.Z;
  return true;
}

// 7-bit mask of the owned edges of grid vertex (x, y, z) that cross the level
__global__ void __launch_bounds__(PSDF_BLOCK)
    mesh_classify_vertices_kernel(Slab s, int p0, int p1, const float* __restrict__ vol, const uint8_t* __restrict__ valid,
                                  float level, uint8_t* __restrict__ mask, int32_t* __restrict__ vcount) {
  int x, y, z;
  int64_t rel;
  if (!point_of_thread(s, p0, p1, x, y, z, rel)) return;
  const int64_t i = s.slot(x, y, z);
  unsigned m = 0;
  if (ok(valid, i)) {
    const bool in0 = (vol[i] - level) < 0.f;
#pragma unroll
    for (int d = 0; d < 7; ++d) {
      const int c = PSDF_MT_OFFSET_OF_DIR[d];
      const int dx = c & 1, dy = (c >> 1) & 1, dz = c >> 2;
      if (x + dx < s.X && y + dy < s.Y && z + dz < s.Z) {
        const int64_t j = s.slot(x + dx, y + dy, z + dz);
        if (ok(valid, j) && (((vol[j] - level) < 0.f) != in0)) m |= 1u << d;
      }
    }
  }
  mask[i] = (uint8_t)m;
  vcount[rel] = __popc(m);
}

// inside bits of the eight corners of cell (x, y, z); false when the cell does not exist or has an invalid corner
__device__ __forceinline__ bool cell_bits(const Slab& s, int x, int y, int z, const float* __restrict__ vol,
                                          const uint8_t* __restrict__ valid, float level, unsigned& bits) {
  bits = 0;
  if (x + 1 >= s.X || y + 1 >= s.Y || z + 1 >= s.Z) return false;
  bool all = true;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int64_t j = s.slot(x + (c & 1), y + ((c >> 1) & 1), z + (c >> 2));
    if (!ok(valid, j)) {
      all = false;
    } else if ((vol[j] - level) < 0.f) {
      bits |= 1u << c;
    }
  }
  return all;
}

__device__ __forceinline__ unsigned tet_case(unsigned bits, int t) {
  return ((bits >> PSDF_MT_TETS[t][0]) & 1u) | (((bits >> PSDF_MT_TETS[t][1]) & 1u) << 1) |
         (((bits >> PSDF_MT_TETS[t][2]) & 1u) << 2) | (((bits >> PSDF_MT_TETS[t][3]) & 1u) << 3);
}

__device__ __forceinline__ int cell_triangles(unsigned bits) {
  if (bits == 0u || bits == 255u) return 0;
  int n = 0;
#pragma unroll
  for (int t = 0; t < 6; ++t) n += PSDF_MT_NTRI[tet_case(bits, t)];
  return n;
}

__global__ void __launch_bounds__(PSDF_BLOCK)
    mesh_classify_cells_kernel(Slab s, int c0, int c1, const float* __restrict__ vol, const uint8_t* __restrict__ valid,
                               float level, int32_t* __restrict__ tcount) {
  int x, y, z;
  int64_t rel;
  if (!point_of_thread(s, c0, c1, x, y, z, rel)) return;
  unsigned bits;
  tcount[rel] = cell_bits(s, x, y, z, vol, valid, level, bits) ? cell_triangles(bits) : 0;
}

// np.gradient along one axis (edge_order 1): central difference inside, one-sided at the two borders; fp32
__device__ __forceinline__ float axis_gradient(const float* __restrict__ vol, int64_t i, int64_t stride, int k, int n) {
  if (k == 0) return vol[i + stride] - vol[i];
  if (k == n - 1) return vol[i] - vol[i - stride];
  return (vol[i + stride] - vol[i - stride]) * 0.5f;
}
__device__ __forceinline__ v3 volume_gradient(const Slab& s, const float* __restrict__ vol, int x, int y, int z) {
  const int64_t i = s.slot(x, y, z);
  return mk3(axis_gradient(vol, i, (int64_t)s.Y * s.Z, x, s.X), axis_gradient(vol, i, s.Z, y, s.Y), axis_gradient(vol, i, 1, z, s.Z));
}

template <bool NORMALS>
__global__ void __launch_bounds__(PSDF_BLOCK)
    mesh_emit_vertices_kernel(Slab s, int p0, int p1, const float* __restrict__ vol, float level, const uint8_t* __restrict__ mask,
                              const int32_t* __restrict__ vincl, int64_t v_off, float* __restrict__ verts,
                              int64_t* __restrict__ edges, float* __restrict__ normals) {
  int x, y, z;
  int64_t rel;
  if (!point_of_thread(s, p0, p1, x, y, z, rel)) return;
  const int64_t i = s.slot(x, y, z);
  const unsigned m = mask[i];
  if (m == 0u) return;
  int64_t v = (int64_t)vincl[i] - __popc(m) - v_off;
  const float f_lo = vol[i] - level;
  const int64_t lin = ((int64_t)x * s.Y + y) * s.Z + z;
#pragma unroll
  for (int d = 0; d < 7; ++d) {
    if (!((m >> d) & 1u)) continue;
    const int c = PSDF_MT_OFFSET_OF_DIR[d];
    const int dx = c & 1, dy = (c >> 1) & 1, dz = c >> 2;
    const float f_hi = vol[s.slot(x + dx, y + dy, z + dz)] - level;
    const float t = f_lo / (f_lo - f_hi);
    // p_lo + (p_hi - p_lo) * t with p_hi - p_lo in {0, 1}: the product is exact, one rounding per moving coordinate
    st3(verts + 3 * v, mk3(dx ? (float)x + t : (float)x, dy ? (float)y + t : (float)y, dz ? (float)z + t : (float)z));
    if (edges) {
      edges[2 * v] = lin;
      edges[2 * v + 1] = lin + ((int64_t)dx * s.Y + dy) * s.Z + dz;
    }
    if (NORMALS) {   // the stand-in's normal: volume gradient at the two ends, interpolated with t, normalised, negated
      const v3 g0 = volume_gradient(s, vol, x, y, z), g1 = volume_gradient(s, vol, x + dx, y + dy, z + dz);
      const v3 g = g0 + (g1 - g0) * t;
      const float nrm = fmaxf(sqrtf(dot3(g, g)), 1e-20f);
      st3(normals + 3 * v, mk3(-g.x / nrm, -g.y / nrm, -g.z / nrm));
    }
    ++v;
  }
}

__global__ void __launch_bounds__(PSDF_BLOCK)
    mesh_emit_faces_kernel(Slab s, int c0, int c1, const float* __restrict__ vol, const uint8_t* __restrict__ valid, float level,
                           const uint8_t* __restrict__ mask, const int32_t* __restrict__ vincl,
                           const int32_t* __restrict__ tincl, int32_t* __restrict__ faces) {
  int x, y, z;
  int64_t rel;
  if (!point_of_thread(s, c0, c1, x, y, z, rel)) return;
  unsigned bits;
  if (!cell_bits(s, x, y, z, vol, valid, level, bits)) return;
  const int n = cell_triangles(bits);
  if (n == 0) return;
  int64_t f = (int64_t)tincl[rel] - n;
  for (int t = 0; t < 6; ++t) {
    const unsigned cs = tet_case(bits, t);
    const int nt = PSDF_MT_NTRI[cs];
    for (int k = 0; k < nt; ++k) {
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        const unsigned code = PSDF_MT_TRIS[t][cs][k][e];
        const unsigned lo = code >> 3, hi = code & 7u;
        const int64_t o = s.slot(x + (int)(lo & 1u), y + (int)((lo >> 1) & 1u), z + (int)(lo >> 2));
        const unsigned m = mask[o];
        const unsigned d = PSDF_MT_DIR_OF_OFFSET[hi - lo];
        faces[3 * f + e] = vincl[o] - __popc(m) + __popc(m & ((1u << d) - 1u));
      }
      ++f;
    }
  }
}

// grid points of `count` consecutive linear indices (from `first`, relative to plane x0) of an [., Y, Z] grid with the
// caller's axis coordinates (their bits are the caller's: torch.linspace)
__global__ void __launch_bounds__(PSDF_BLOCK)
    mesh_grid_points_kernel(int Y, int Z, int x0, int64_t first, int64_t count, const float* __restrict__ xs,
                            const float* __restrict__ ys, const float* __restrict__ zs, float* __restrict__ pts) {
  const int64_t i = (int64_t)blockIdx.x * PSDF_BLOCK + threadIdx.x;
  if (i >= count) return;
  const int64_t lin = first + i, plane = (int64_t)Y * Z;
  const int r = (int)(lin % plane);
  st3(pts + 3 * i, mk3(xs[x0 + (int)(lin / plane)], ys[r / Z], zs[r % Z]));
}

// Morton spreading of a 10-bit coordinate (the occupancy grid's order, csrc/sampling.hip)
__device__ __forceinline__ uint32_t spread10(uint32_t v) {
  v = (v | (v << 16)) & 0xFF0000FFu;
  v = (v | (v << 8)) & 0x0F00F00Fu;
  v = (v | (v << 4)) & 0xC30C30C3u;
  v = (v | (v << 2)) & 0x49249249u;
  return v;
}
// voxel coordinate of a world coordinate along one axis (OccupancyGrid's pos_to_idx arithmetic), -1 outside the grid
__device__ __forceinline__ int voxel_of(float p, float tr, float extent, int n) {
  const float g = ((p - tr) / extent + 0.5f) * (float)n;
  return (g >= 0.f && g < (float)n) ? (int)g : -1;
}

// valid[i] = one of the 27 probes p + {-h, 0, h}^3 lies in an occupied voxel; skip[i] = !valid[i] (optional)
__global__ void __launch_bounds__(PSDF_BLOCK)
    mesh_sparse_mask_kernel(int64_t count, int n, float extent, float tx, float ty, float tz, const uint8_t* __restrict__ occ,
                            const float* __restrict__ pts, float h, uint8_t* __restrict__ valid, uint8_t* __restrict__ skip) {
  const int64_t i = (int64_t)blockIdx.x * PSDF_BLOCK + threadIdx.x;
  if (i >= count) return;
  const v3 p = ld3(pts + 3 * i);
  int vx[3], vy[3], vz[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float o = (float)(k - 1) * h;
    vx[k] = voxel_of(p.x + o, tx, extent, n);
    vy[k] = voxel_of(p.y + o, ty, extent, n);
    vz[k] = voxel_of(p.z + o, tz, extent, n);
  }
  bool any = false;
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        if (vx[a] < 0 || vy[b] < 0 || vz[c] < 0) continue;
        const uint32_t vox = spread10((uint32_t)vx[a]) | (spread10((uint32_t)vy[b]) << 1) | (spread10((uint32_t)vz[c]) << 2);
        if (vox < (uint32_t)(n * n * n)) any |= occ[vox] != 0;   // (n not a power of two: Morton indices beyond the array)
      }
  valid[i] = any ? 1 : 0;
  if (skip) skip[i] = any ? 0 : 1;
}

inline bool slab_ok(int X, int Y, int Z, int xbase, int nplanes) {
  return X >= 1 && Y >= 1 && Z >= 1 && xbase >= 0 && nplanes >= 0 && (int64_t)xbase + nplanes <= X;
}
// planes [a, b) lie inside the buffer
inline bool planes_ok(int xbase, int nplanes, int a, int b) { return a >= xbase && b <= xbase + nplanes && a <= b; }
#define MESH_GRID(n) dim3(psdf_blocks((n), PSDF_BLOCK)), dim3(PSDF_BLOCK), 0, (hipStream_t)stream

}  // namespace

extern "C" {

int psdf_mesh_classify(const float* vol, const uint8_t* valid, float level, int X, int Y, int Z, int xbase, int nplanes, int p0,
                       int p1, int c0, int c1, uint8_t* mask, int32_t* vcount, int32_t* tcount, void* stream) {
  if (!slab_ok(X, Y, Z, xbase, nplanes)) return PSDF_ERR_ARG;
  const Slab s{X, Y, Z, xbase, nplanes};
  const int64_t plane = (int64_t)Y * Z;
  if (p1 > p0) {
    // vertex plane p reads value plane p + 1 wherever that exists
    if (!planes_ok(xbase, nplanes, p0, p1 < X ? p1 + 1 : p1) || !vol || !mask || !vcount) return PSDF_ERR_ARG;
    hipLaunchKernelGGL(mesh_classify_vertices_kernel, MESH_GRID((p1 - p0) * plane), s, p0, p1, vol, valid, level, mask, vcount);
    PSDF_LAUNCH_CHECK();
  }
  if (c1 > c0) {
    if (c1 > X - 1 || !planes_ok(xbase, nplanes, c0, c1 + 1) || !vol || !tcount) return PSDF_ERR_ARG;
    hipLaunchKernelGGL(mesh_classify_cells_kernel, MESH_GRID((c1 - c0) * plane), s, c0, c1, vol, valid, level, tcount);
    PSDF_LAUNCH_CHECK();
  }
  return (p1 < p0 || c1 < c0) ? PSDF_ERR_ARG : PSDF_OK;
}

int psdf_mesh_emit_vertices(const float* vol, float level, int X, int Y, int Z, int xbase, int nplanes, int p0, int p1,
                            const uint8_t* mask, const int32_t* vincl, int64_t v_off, float* verts, int64_t* edges,
                            float* normals, void* stream) {
  if (!slab_ok(X, Y, Z, xbase, nplanes) || p1 < p0) return PSDF_ERR_ARG;
  if (p1 == p0) return PSDF_OK;
  if (!planes_ok(xbase, nplanes, p0, p1 < X ? p1 + 1 : p1) || !vol || !mask || !vincl || !verts) return PSDF_ERR_ARG;
  if (normals && !(xbase == 0 && nplanes == X)) return PSDF_ERR_UNSUPPORTED;   // the volume gradient needs the whole volume
  const Slab s{X, Y, Z, xbase, nplanes};
  const int64_t n = (int64_t)(p1 - p0) * Y * Z;
  if (normals)
    hipLaunchKernelGGL(mesh_emit_vertices_kernel<true>, MESH_GRID(n), s, p0, p1, vol, level, mask, vincl, v_off, verts, edges, normals);
  else
    hipLaunchKernelGGL(mesh_emit_vertices_kernel<false>, MESH_GRID(n), s, p0, p1, vol, level, mask, vincl, v_off, verts, edges, normals);
  PSDF_LAUNCH_CHECK();
  return PSDF_OK;
}

int psdf_mesh_emit_faces(const float* vol, const uint8_t* valid, float level, int X, int Y, int Z, int xbase, int nplanes, int c0,
                         int c1, const uint8_t* mask, const int32_t* vincl, const int32_t* tincl, int32_t* faces, void* stream) {
  if (!slab_ok(X, Y, Z, xbase, nplanes) || c1 < c0) return PSDF_ERR_ARG;
  if (c1 == c0) return PSDF_OK;
  if (c1 > X - 1 || !planes_ok(xbase, nplanes, c0, c1 + 1) || !vol || !mask || !vincl || !tincl || !faces) return PSDF_ERR_ARG;
  const Slab s{X, Y, Z, xbase, nplanes};
  hipLaunchKernelGGL(mesh_emit_faces_kernel, MESH_GRID((int64_t)(c1 - c0) * Y * Z), s, c0, c1, vol, valid, level, mask, vincl,
                     tincl, faces);
  PSDF_LAUNCH_CHECK();
  return PSDF_OK;
}

int psdf_mesh_grid_points(int nx, int Y, int Z, int x0, int64_t first, int64_t count, const float* xs, const float* ys,
                          const float* zs, float* points, void* stream) {
  if (count < 0 || first < 0 || Y < 1 || Z < 1 || x0 < 0) return PSDF_ERR_ARG;
  if (count == 0) return PSDF_OK;
  // the last point's plane must be one of xs' nx entries
  if (!xs || !ys || !zs || !points || x0 + (first + count - 1) / ((int64_t)Y * Z) >= nx) return PSDF_ERR_ARG;
  hipLaunchKernelGGL(mesh_grid_points_kernel, MESH_GRID(count), Y, Z, x0, first, count, xs, ys, zs, points);
  PSDF_LAUNCH_CHECK();
  return PSDF_OK;
}

int psdf_mesh_sparse_mask(int64_t count, int nr_voxels_per_dim, float extent, const float* grid_translation,
                          const uint8_t* grid_occupancy, const float* points, float h, uint8_t* valid, uint8_t* skip, void* stream) {
  const int n = nr_voxels_per_dim;
  if (count < 0 || n < 1 || n > 1024 || !(extent > 0.f) || !(h >= 0.f) || !grid_translation) return PSDF_ERR_ARG;
  if (count == 0) return PSDF_OK;
  if (!grid_occupancy || !points || !valid) return PSDF_ERR_ARG;
  hipLaunchKernelGGL(mesh_sparse_mask_kernel, MESH_GRID(count), count, n, extent, grid_translation[0], grid_translation[1],
                     grid_translation[2], grid_occupancy, points, h, valid, skip);
  PSDF_LAUNCH_CHECK();
  return PSDF_OK;
}

}  // extern "C"
