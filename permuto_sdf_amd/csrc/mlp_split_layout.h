// What the two split backwards of the 64x3 -> 1 SDF net share (mlp_bwd_split.hip: three bf16 pieces per operand;
// mlp_bwd_split_f16.hip: two fp16 pieces): the tile constants, the LDS operand image (parameterised by the number of pieces),
// the gradient image a workgroup leaves, the small register-tile helpers, the pack kernels' weight fetch, and the host-side
// block count and argument check.  The kernels themselves stay in their files.
#pragma once
#include "psdf_common.h"
#include "mlp_dispatch.h"
#include "gelu_device.h"

namespace {

constexpr int HID = 64, NT = 4 /* 16-feature tiles of a hidden layer */;   // NT0 (template) = tiles covering the input: 3 (<= 48) or 4 (<= 64)
constexpr int NWAVES = 4;
// feature that slot j of lane group g holds in k-step s of a chain operand (a D tile pair read as a B operand)
__host__ __device__ inline int kf(int s, int g, int j) { return 32 * s + 16 * (j >> 2) + 4 * g + (j & 3); }

// ------------------------------------------------------------------ LDS image (units: 16-byte lane records)
// every layer: [tile][k-step 2][piece NP][lane 64]; then the fp32 tail
constexpr int TAIL_FLOATS = 3 * HID + HID + 1;  // biases of the three hidden layers, final weights, final bias
template <int NP>
struct SplitImage {
  static constexpr int RECL = NT * 2 * NP * 64;
  static constexpr int OFF_W0 = 0, OFF_W1 = RECL, OFF_W2 = 2 * RECL, OFF_T2 = 3 * RECL, OFF_T1 = 4 * RECL, OFF_T0 = 5 * RECL;
  static constexpr int off_f32(int nt0) { return 5 * RECL + nt0 * 2 * NP * 64; }
  static constexpr size_t aligned(int nt0) { return ((size_t)off_f32(nt0) * 16 + TAIL_FLOATS * 4 + 15) / 16 * 16; }
};
// gradient image (floats): dW1 [64][64 (K0 used)], dW2 [64][64], dW3 [64][64], db1, db2, db3 [64], dW4 [64], db4
constexpr int G_W1 = 0, G_W2 = 4096, G_W3 = 8192, G_B1 = 12288, G_B2 = 12352, G_B3 = 12416, G_W4 = 12480, G_B4 = 12544,
              G_TOTAL = 12545;

// ------------------------------------------------------------------ register tiles
// B operand of k-step s from the D tiles 2s, 2s+1 of an activation
__device__ __forceinline__ void step_operand(const f32x4 (&act)[NT], int s, float (&x)[8]) {
#pragma unroll
  for (int j = 0; j < 4; j++) {
    x[j] = act[2 * s][j];
    x[4 + j] = act[2 * s + 1][j];
  }
}
// a 16-bit operand of eight slots from four packed pairs
template <typename OP>
__device__ __forceinline__ OP halves(uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1) {
  const u32x4 q = {a0, a1, b0, b1};
  return __builtin_bit_cast(OP, q);
}
// 0/1 operand that selects the 16 features of tile 2s+u out of a k-step (the same for every s); ONE = 1.0 in the operand's format
template <typename OP, uint32_t ONE>
__device__ __forceinline__ OP ident_op(int u, int lane) {
  const int c = lane & 15, g = lane >> 4;
  u32x4 q;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int j0 = 2 * i, j1 = 2 * i + 1;
    const uint32_t lo = ((j0 >> 2) == u && 4 * g + (j0 & 3) == c) ? ONE : 0u;
    const uint32_t hi = ((j1 >> 2) == u && 4 * g + (j1 & 3) == c) ? ONE : 0u;
    q[i] = lo | (hi << 16);
  }
  return __builtin_bit_cast(OP, q);
}
__device__ __forceinline__ f32x4 zero4() { return f32x4{0.f, 0.f, 0.f, 0.f}; }
template <int NTILE>
__device__ __forceinline__ void bias_init(f32x4 (&acc)[NTILE], const float* __restrict__ b, int g) {
#pragma unroll
  for (int t = 0; t < NTILE; t++) acc[t] = *reinterpret_cast<const f32x4*>(b + 16 * t + 4 * g);
}
template <int NTILE>
__device__ __forceinline__ void zero_init(f32x4 (&acc)[NTILE]) {
#pragma unroll
  for (int t = 0; t < NTILE; t++) acc[t] = zero4();
}

// ------------------------------------------------------------------ pack kernels: torch-layout parameters -> image
// weight that slot j of lane (c = row & 15, g) holds in k-step s of image im = 0..5 (W0, W1, W2, then the transposed W2, W1,
// W0: the order of OFF_W0 .. OFF_T0); row = 16 tile + c
__device__ __forceinline__ float image_weight(int im, int row, int s, int g, int j, int K0, const float* W0,
                                              const float* W1, const float* W2) {
  const int k0 = 32 * s + 8 * g + j, kc = kf(s, g, j);   // layer 0: natural k order
  switch (im) {
    case 0: return k0 < K0 ? W0[row * K0 + k0] : 0.f;
    case 1: return W1[row * HID + kc];
    case 2: return W2[row * HID + kc];
    case 3: return W2[kc * HID + row];                 // transposed images: row is an INPUT neuron of the layer
    case 4: return W1[kc * HID + row];
    default: return row < K0 ? W0[kc * K0 + row] : 0.f;
  }
}
// (The tail copy of the pack kernels and the scatter of the reduce kernels -- two if-ladders over the segments of TAIL_FLOATS and
// of the gradient image -- are NOT functions here: the compiler simplifies a __device__ function on its own before it inlines it,
// and all four kernels then came out a few instructions different from what they were.  Each file keeps its ladder; a change of
// the tail or of G_* above is made in both.)

// ------------------------------------------------------------------ host
inline int64_t split_blocks(int64_t N) {
  const int64_t ntiles = (N + 15) / 16;
  const int64_t blocks = (ntiles + NWAVES - 1) / NWAVES;   // four tiles in flight per workgroup
  return blocks > 256 ? 256 : blocks;  // one workgroup per CU; each wave walks many tiles
}
// the contract of psdf_mlp_backward (include/psdf.h) for dims = {K0 <= max_k0, 64, 64, 64, 1} with dW / db requested:
// PSDF_ERR_UNSUPPORTED for every other net (the caller then takes the fp32 kernel), PSDF_ERR_ARG for missing arguments
inline int split_check(int n_layers, const int* dims, int max_k0, int64_t N, const float* X, const float* const* weights,
                       const float* const* biases, const float* dY, float* const* dW, float* const* db) {
  if (!dims || !dW || !db || !baseline_split_shape(n_layers, dims, max_k0, 1)) return PSDF_ERR_UNSUPPORTED;
  if (N <= 0 || !X || !weights || !biases || !dY) return PSDF_ERR_ARG;
  for (int l = 0; l < 4; l++)
    if (!weights[l] || !biases[l] || !dW[l] || !db[l]) return PSDF_ERR_ARG;
  return PSDF_OK;
}

}  // namespace
