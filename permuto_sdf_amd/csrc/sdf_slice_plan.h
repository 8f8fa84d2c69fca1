// sdf_slice_plan.h -- the host arithmetic behind the launches of sdf_slice.hip, in one place: the limits of a layer and of a
// frame, the range checks of a chunk of cells or pixels, the grid over it, and the two small records that travel in the kernel
// arguments (a map_range and the band table).  No HIP, no device, no state -- a plain C++17 compiler accepts this header, and
// tests/host/sdf_slice_kernels_check.cpp uses it under the address and undefined-behaviour sanitizers.
#pragma once
#include <cstdint>

namespace psdf {
namespace sdf_slice_plan {

constexpr int PLAN_OK = 0, PLAN_ERR_ARG = -1, PLAN_ERR_UNSUPPORTED = -2;

constexpr int BLOCK = 256;                       // threads of every workgroup of the file: one per cell or per ray
constexpr int64_t MAX_CELLS = 0x7fffffffll;      // cell and pixel indices are int32: S S < 2^31, H W < 2^31
constexpr int MAX_LINES = 32;                    // iso-bands of one call: the table is a kernel argument, not device memory
constexpr int MIN_TABLE = 2;                     // control points of a colour table: one segment at least
constexpr int MAX_TABLE = 1 << 16;               // float(K - 1) and the segment index stay exact in float32 far beyond it

// map_range (permuto_sdf_py/utils/common_utils.py:150-154) with its clamp: out_lo + scale * (clamp(x, in_lo, in_hi) - in_lo),
// scale = (out_hi - out_lo) / (in_hi - in_lo) computed by the host in float64 and rounded once
struct MapRange {
  float in_lo, in_hi, out_lo, scale;
};

// line i: sdf in (lo[i], hi[i]), both strict, takes rgb[i]; the last matching line wins
struct Bands {
  int n;
  float lo[MAX_LINES], hi[MAX_LINES], rgb[MAX_LINES][3];
};

// the chunk [first, first + count) of the cells of an S x S layer or of the pixels of an H x W frame (count >= 1)
inline int check_range(int rows, int cols, int64_t first, int64_t count) {
  if (rows < 1 || cols < 1 || count < 1) return PLAN_ERR_ARG;
  const int64_t cells = (int64_t)rows * cols;
  if (cells > MAX_CELLS) return PLAN_ERR_UNSUPPORTED;
  if (first < 0 || first > cells - count) return PLAN_ERR_ARG;
  return PLAN_OK;
}

inline int check_stride(int stride) { return (stride == 3 || stride == 4) ? PLAN_OK : PLAN_ERR_ARG; }

inline int check_lines(int nr_lines) { return (nr_lines >= 0 && nr_lines <= MAX_LINES) ? PLAN_OK : PLAN_ERR_ARG; }

// -> workgroups over count elements (count >= 1, at most MAX_CELLS: the product fits an unsigned)
inline unsigned grid(int64_t count) { return (unsigned)((count + BLOCK - 1) / BLOCK); }

}  // namespace sdf_slice_plan
}  // namespace psdf
