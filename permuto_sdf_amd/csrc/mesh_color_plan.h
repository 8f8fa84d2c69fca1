// mesh_color_plan.h -- the host arithmetic behind mesh_color.hip and permuto_sdf_amd/mesh_color.py, in one place: the rows of the
// colour network's feature-major input x_fm [C, n] = [colour encoding | SH of the view direction | unit normal | geometry
// features], the chunks a mesh's vertices are streamed in, the limits of a launch.  Integers only: no HIP, no device, no state --
// a plain C++17 compiler accepts this header, and tests/host/mesh_color_plan_check.cpp runs it under the address and
// undefined-behaviour sanitizers.
#pragma once
#include <cstdint>

namespace psdf {
namespace mesh_color_plan {

constexpr int PLAN_OK = 0, PLAN_ERR_ARG = -1, PLAN_ERR_UNSUPPORTED = -2;

constexpr int BLOCK = 256;                    // threads of a workgroup: one vertex per thread
constexpr int SH_DEGREE = 5, SH = SH_DEGREE * SH_DEGREE;      // 25 rows (models.py:352)
constexpr int NORMAL = 3;
constexpr int MODE_NORMAL = 0, MODE_CAMERA = 1;               // view direction: -normal | from an eye position
constexpr int64_t MAX_LAUNCH = 0x7fffffffll;  // vertices of one launch: the grid (n / BLOCK workgroups) stays far inside 2^31
constexpr int MAX_ROWS = 1 << 16;             // of x_fm: no network here is wider, and C * n stays far inside int64
constexpr int FIELDS = 7;                     // of `Plan`, as psdf_mesh_color_plan writes them

// Rows of x_fm.  Every field is the row at which the NEXT block starts, as ManualTrainer._fg_forward names them: the colour
// encoding is rows [0, c_enc), SH [c_enc, c_sh), the unit normal [c_sh, c_normal), the geometry features [c_normal, c_geom),
// and C = c_geom rows in all.
struct Rows {
  int c_enc, c_sh, c_normal, c_geom, C;
};

// rgb_enc_width: output channels of the colour encoding (>= 1); g: geometry features of the SDF net (>= 0; its output has 1 + g
// rows).  PLAN_OK, PLAN_ERR_ARG, or PLAN_ERR_UNSUPPORTED beyond MAX_ROWS
inline int rows(int rgb_enc_width, int g, Rows* r) {
  if (rgb_enc_width < 1 || g < 0 || !r) return PLAN_ERR_ARG;
  const int64_t C = (int64_t)rgb_enc_width + SH + NORMAL + (int64_t)g;
  if (C > MAX_ROWS) return PLAN_ERR_UNSUPPORTED;
  r->c_enc = rgb_enc_width;
  r->c_sh = r->c_enc + SH;
  r->c_normal = r->c_sh + NORMAL;
  r->c_geom = r->c_normal + g;
  r->C = (int)C;
  return PLAN_OK;
}

// n vertices in chunks of `chunk`: the number of chunks and the size of the last one (0, 0 without vertices).  PLAN_ERR_ARG: n
// < 0, chunk < 1; PLAN_ERR_UNSUPPORTED: a chunk beyond MAX_LAUNCH
inline int chunks(int64_t n, int64_t chunk, int64_t* count, int64_t* last) {
  if (n < 0 || chunk < 1 || !count || !last) return PLAN_ERR_ARG;
  if (chunk > MAX_LAUNCH) return PLAN_ERR_UNSUPPORTED;
  *count = n / chunk + (n % chunk != 0);      // (not (n + chunk - 1) / chunk: no sum that could pass 2^63)
  *last = n == 0 ? 0 : n - (*count - 1) * chunk;
  return PLAN_OK;
}

// workgroups of a launch over n vertices (1 <= n <= MAX_LAUNCH); < 0: PLAN_ERR_*
inline int grid(int64_t n) {
  if (n < 1) return PLAN_ERR_ARG;
  if (n > MAX_LAUNCH) return PLAN_ERR_UNSUPPORTED;
  return (int)((n + BLOCK - 1) / BLOCK);
}

// everything a call of MeshColorizer.colors needs: the rows, checked against the width the colour MLP takes (mlp_in = dims[0]),
// and the chunks
struct Plan {
  Rows r;
  int64_t nr_chunks, last_chunk;
};
inline int plan(int rgb_enc_width, int g, int mlp_in, int64_t n, int64_t chunk, Plan* p) {
  if (!p) return PLAN_ERR_ARG;
  int status = rows(rgb_enc_width, g, &p->r);
  if (status != PLAN_OK) return status;
  if (p->r.C != mlp_in) return PLAN_ERR_ARG;
  return chunks(n, chunk, &p->nr_chunks, &p->last_chunk);
}

}  // namespace mesh_color_plan
}  // namespace psdf
