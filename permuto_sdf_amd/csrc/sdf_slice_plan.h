// sdf_slice_plan.h -- the host arithmetic behind the launches of sdf_slice.hip, in one place: the limits of the colour
// arguments, the grid over a chunk of cells or pixels (frame_plan.h checks its range), and the two small records that travel in the kernel
// arguments (a map_range and the band table).  No HIP, no device, no state -- a plain C++17 compiler accepts this header, and
// tests/host/sdf_slice_kernels_check.cpp uses it under the address and undefined-behaviour sanitizers.
#pragma once
#include <cstdint>

namespace psdf {
namespace sdf_slice_plan {

constexpr int PLAN_OK = 0, PLAN_ERR_ARG = -1, PLAN_ERR_UNSUPPORTED = -2;

constexpr int BLOCK = 256;                       // threads of every workgroup of the file: one per cell or per ray
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

inline int check_stride(int stride) { return (stride == 3 || stride == 4) ? PLAN_OK : PLAN_ERR_ARG; }

inline int check_lines(int nr_lines) { return (nr_lines >= 0 && nr_lines <= MAX_LINES) ? PLAN_OK : PLAN_ERR_ARG; }

// -> workgroups over count elements (count >= 1, at most frame_plan::MAX_PIXELS: the quotient fits an unsigned)
inline unsigned grid(int64_t count) { return (unsigned)((count + BLOCK - 1) / BLOCK); }

}  // namespace sdf_slice_plan
}  // namespace psdf
