// Which MLP widths have a fused kernel: the ONE table the dispatchers of mlp.hip, mlp_bwd.hip, mlp_wide.hip and the split
// backward files expand, and that psdf_mlp_supported (include/psdf.h) answers from.  Host code only.
//
// A new instantiation is one row here (plus its kernel); the dispatchers, the query and the Python predicates
// (permuto_sdf_amd/mlp.py, which asks psdf_mlp_supported) follow from it.
#pragma once
#include "../../include/psdf.h"

// PSDF_IF(c, ...): the arguments when the table column c is 1, nothing when it is 0 -- a dispatcher instantiates the launchers
// of exactly the rows that have its column
#define PSDF_IF_0(...)
#define PSDF_IF_1(...) __VA_ARGS__
#define PSDF_IF(c, ...) PSDF_IF_##c(__VA_ARGS__)

// ---- single-wave kernels on 16-wide tiles (mlp_bwd.hip): X(ti0, t1, t2, t3, to, final_dot, DW, DX, MASKED, DBL, PLUS)
//   ti0 .. to: tiles of 16 of every width (t3 = 0: two hidden layers); final_dot: outputs <= 4
//   DW     psdf_mlp_backward with parameter gradients (0: the single-wave dW form spills; mlp_wide.hip takes the dW of these)
//   DX     psdf_mlp_backward, data gradient only
//   MASKED psdf_mlp_backward_data_masked
//   DBL    psdf_mlp_double_backward
//   PLUS   psdf_mlp_double_backward_plus
#define PSDF_MLP16_ROWS(X)                                                                                          \
  X(3, 4, 4, 4, 1, true, 1, 1, 1, 1, 0)   /* 33..48 -> 64x3 -> 1..4   (BASELINE SDF net on a 16-level encoding) */  \
  X(4, 4, 4, 4, 1, true, 1, 1, 1, 1, 0)   /* 49..64 -> 64x3 -> 1..4   (24-level encoding) */                        \
  X(2, 4, 4, 4, 1, true, 1, 1, 1, 0, 0)   /* 17..32 -> 64x3 -> 1..4   (small encodings) */                          \
  X(4, 2, 2, 2, 1, true, 1, 1, 1, 1, 0)   /* 49..64 -> 32x3 -> 1..4 */                                              \
  X(3, 2, 2, 2, 1, true, 1, 1, 1, 1, 0)   /* 33..48 -> 32x3 -> 1..4 */                                              \
  X(2, 2, 2, 2, 1, true, 1, 1, 1, 1, 0)   /* 17..32 -> 32x3 -> 1..4 */                                              \
  X(4, 2, 2, 2, 3, false, 1, 1, 0, 1, 1)  /* 52 -> 32x3 -> 33         (reference SDF net, models.py:153-161) */      \
  X(3, 2, 2, 2, 3, false, 1, 1, 0, 1, 1)  /* 36 -> 32x3 -> 33         (same net on a 16-level encoding) */          \
  X(4, 4, 4, 4, 5, false, 0, 1, 0, 0, 0)  /* 52 -> 64x3 -> 65         (background density net, models.py:451-459) */ \
  X(4, 4, 4, 4, 3, false, 0, 1, 0, 0, 0)  /* 52 -> 64x3 -> 33 */                                                    \
  X(3, 4, 4, 4, 3, false, 0, 1, 0, 0, 0)  /* 36 -> 64x3 -> 33 */                                                    \
  X(5, 4, 4, 0, 1, true, 1, 1, 0, 0, 0)   /* 80 -> 64x2 -> 3          (background colour head, models.py:463-469) */

// ---- single-wave forward on 32-wide tiles (mlp.hip, mlp_forward_impl): X(t1, t2, t3, to, final_dot, FWD, SPLIT, F16)
//   FWD    psdf_mlp_forward / psdf_mlp_forward_masked (fp32 MFMAs, or the split-bf16 kernel where SPLIT allows it)
//   SPLIT  the split-bf16 kernel is built (its image can fit SPLIT_LDS_MAX; SplitPlan::ok decides per net)
//   F16    psdf_mlp_forward_f16 (two fp16 pieces per operand; also needs baseline_split_shape)
#define PSDF_MLP32_ROWS(X)                                                                                          \
  X(2, 2, 2, 1, true, 1, 1, 1)    /* 64x3 -> 1..4      (BASELINE SDF net) */                                        \
  X(1, 1, 1, 1, true, 1, 1, 0)    /* 32x3 -> 1..4 */                                                                \
  X(1, 1, 1, 2, false, 1, 1, 0)   /* 32x3 -> 33        (reference SDF net, models.py:153-161) */                    \
  X(2, 2, 2, 3, false, 1, 0, 0)   /* 64x3 -> 65        (background density+feature net, models.py:451-459) */       \
  X(2, 2, 2, 2, false, 1, 0, 0)   /* 64x3 -> 33 */                                                                  \
  X(2, 2, 0, 1, true, 1, 1, 0)    /* 64x2 -> 3         (background colour head, models.py:463-469) */               \
  X(4, 4, 2, 1, true, 1, 0, 0)    /* 128,128,64 -> 3   (colour net, models.py:350) */

// ---- the workgroup-cooperative kernels of mlp_wide.hip (shapes by width, not by tile signature)
// the colour network LipshitzMLP 111 -> 128 -> 128 -> 64 -> 3 (models.py:349-350) and what fits its tiles with one output tile:
// psdf_mlp_forward_wide_f16 and psdf_mlp_backward_wide
inline bool colour_net_shape(int n_layers, const int* d) {
  return n_layers == 4 && d[0] <= 112 && d[1] <= 128 && d[2] <= 128 && d[3] <= 64 && d[4] <= 16 && !(d[1] <= 64 && d[2] <= 64);
}
// the background density / feature net 52 -> 64 x 3 -> 65 (models.py:451-459) and 64 x 3 -> 33: psdf_mlp_forward_wide_f16 and
// psdf_mlp_backward_wide.  Hidden layers of 32 or fewer are not taken: the split-fp16 backward misses its bar there by far
// (errors of percents against float64), and the 32-wide nets have single-wave kernels of their own
inline bool density_net_shape(int n_layers, const int* d) {
  return n_layers == 4 && d[0] <= 64 && d[1] > 32 && d[1] <= 64 && d[2] > 32 && d[2] <= 64 && d[3] > 32 && d[3] <= 64 &&
         d[4] > 16 && d[4] <= 80;
}
// the background colour head 80 -> 64 -> 64 -> 3 (models.py:463-469): psdf_mlp_backward_wide with two hidden layers, for the
// heads its fp32 redo (the single-wave row (5, 4, 4, 0, 1) of mlp_bwd.hip) covers
inline bool colour_head_shape(int n_layers, const int* d) {
  return n_layers == 3 && d[0] > 64 && d[0] <= 80 && d[1] > 48 && d[1] <= 64 && d[2] > 48 && d[2] <= 64 && d[3] <= 4;
}
// every shape psdf_mlp_backward_wide takes
inline bool wide_backward_shape(int n_layers, const int* d) {
  return colour_net_shape(n_layers, d) || density_net_shape(n_layers, d) || colour_head_shape(n_layers, d);
}

// ---- the BASELINE net {K0, 64, 64, 64, out} with 1 <= K0 <= max_k0, 1 <= out <= max_out: the two-piece fp16 image of
// psdf_mlp_pack_f16 and psdf_mlp_forward_f16 (64, 4), the split backward kernels (split_check of mlp_split_layout.h):
// psdf_mlp_backward_split_f16 (64, 1), psdf_mlp_backward_split (52, 1: what its larger image leaves of 160 KB of LDS)
inline bool baseline_split_shape(int n_layers, const int* d, int max_k0, int max_out) {
  return n_layers == 4 && d[0] >= 1 && d[0] <= max_k0 && d[1] == 64 && d[2] == 64 && d[3] == 64 && d[4] >= 1 && d[4] <= max_out;
}
