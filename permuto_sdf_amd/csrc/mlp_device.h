// Device-side building blocks of the fused MLP evaluators (shared by mlp.hip and fused.hip); see mlp.hip for the
// formulation (transposed products, chained D->B operand layout, packed LDS weight image).
#pragma once
#include "psdf_common.h"
#include "gelu_device.h"   // vector typedefs, packed helpers, every GELU evaluator

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int MAXL = 5;  // max number of linear layers
constexpr int WS = 65;   // LDS row stride of a 64-lane weight row (64 + 1 pad float)

struct MlpPlan {
  int n_layers;        // number of linear layers (hidden layers + 1)
  int dims[MAXL + 1];  // true widths: dims[0] = input, dims[n_layers] = output
  int in_steps0;       // ceil(dims[0]/2)
  int tiles[MAXL + 1]; // tiles[i] = ceil(dims[i]/32) for i>=1
  int w_off[MAXL];     // float offsets into the packed buffer
  int b_off[MAXL];
  int total;           // packed floats
  int final_dot;       // 1 when the last layer is evaluated with VALU dot products (out <= 4)
};

__host__ __device__ inline int row_of(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

static int make_plan(int n_layers, const int* dims, MlpPlan& p) {
  if (n_layers < 2 || n_layers > MAXL) return PSDF_ERR_ARG;
  p.n_layers = n_layers;
  for (int i = 0; i <= n_layers; i++) {
    if (dims[i] <= 0) return PSDF_ERR_ARG;
    p.dims[i] = dims[i];
    p.tiles[i] = (dims[i] + 31) / 32;
  }
  p.in_steps0 = (dims[0] + 1) / 2;
  p.final_dot = dims[n_layers] <= 4;
  int off = 0;
  for (int l = 0; l < n_layers; l++) {
    p.w_off[l] = off;
    const bool last = (l == n_layers - 1);
    if (l == 0)
      off += p.tiles[1] * p.in_steps0 * WS;
    else if (last && p.final_dot)
      off += dims[n_layers] * p.tiles[l] * 32;
    else
      off += p.tiles[l + 1] * p.tiles[l] * 16 * 64;  // [to][ti][r/4][lane][r%4]: one ds_read_b128 feeds 4 MFMAs
    p.b_off[l] = off;
    off += (last && p.final_dot) ? 4 : p.tiles[l + 1] * 32;
  }
  p.total = off;
  return PSDF_OK;
}

constexpr size_t MLP_LDS_MAX = 160 * 1024;  // dynamic LDS a single-wave MLP launch may ask for

// the fp32 forward (mlp_fwd_kernel) stages the whole packed image; launch_fwd and psdf_mlp_supported decline beyond MLP_LDS_MAX
inline bool fwd_fits(const MlpPlan& p) { return (size_t)p.total * sizeof(float) <= MLP_LDS_MAX; }

template <int T>
__device__ __forceinline__ void init_bias(f32x16 (&acc)[T], const float* __restrict__ bias_lds, int h) {
#pragma unroll
  for (int to = 0; to < T; to++)
#pragma unroll
    for (int r = 0; r < 16; r++) acc[to][r] = bias_lds[32 * to + row_of(r, h)];
}

template <int T>
__device__ __forceinline__ void apply_gelu(f32x16 (&acc)[T]) {
#pragma unroll
  for (int to = 0; to < T; to++)
#pragma unroll
    for (int r = 0; r < 16; r += 2) {
      const f32x2 y = gelu_exact2(f32x2{acc[to][r], acc[to][r + 1]});
      acc[to][r] = y.x;
      acc[to][r + 1] = y.y;
    }
}

// gelu_rational on every element, one element per instruction: the split-bf16 forward (why: gelu_device.h)
template <int T>
__device__ __forceinline__ void apply_gelu_scalar(f32x16 (&acc)[T]) {
#pragma unroll
  for (int to = 0; to < T; to++)
#pragma unroll
    for (int r = 0; r < 16; r++) acc[to][r] = gelu_rational(acc[to][r]);
}

// gelu_rational2 on pairs: the two-piece fp16 forward (why: gelu_device.h)
template <int T>
__device__ __forceinline__ void apply_gelu_packed(f32x16 (&acc)[T]) {
#pragma unroll
  for (int to = 0; to < T; to++)
#pragma unroll
    for (int r = 0; r < 16; r += 2) {
      const f32x2 y = gelu_rational2(f32x2{acc[to][r], acc[to][r + 1]});
      acc[to][r] = y.x;
      acc[to][r + 1] = y.y;
    }
}

// out^T = W * in^T for register-resident activations (chained layout, see header).
// Weight image of a chain layer: [(to,ti)][rq][lane][j] = A operand of k-step r = 4 rq + j, so one 128-bit LDS read
// per lane (conflict free: consecutive lanes, 16 bytes each) serves four MFMAs.
template <int TI, int TO>
__device__ __forceinline__ void dense_chain(const f32x16 (&in)[TI], f32x16 (&out)[TO], const float* __restrict__ w_lds,
                                            int lane) {
#pragma unroll
  for (int ti = 0; ti < TI; ti++)
#pragma unroll
    for (int rq = 0; rq < 4; rq++) {
      f32x4 a[TO];
#pragma unroll
      for (int to = 0; to < TO; to++)
        a[to] = *reinterpret_cast<const f32x4*>(w_lds + (((to * TI + ti) * 4 + rq) * 64 + lane) * 4);
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const float b = in[ti][4 * rq + j];
#pragma unroll
        for (int to = 0; to < TO; to++) out[to] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[to][j], b, out[to], 0, 0, 0);
      }
    }
}

// ------------------------------------------------------------------------------ split-bf16 operand path
// fp32 MFMAs and VALU work do not overlap on gfx950 (their times add), bf16 MFMAs do and are 16x faster per k
// (tools/mfma_valu_overlap.hip, profiles/r01_mfma_valu_overlap.txt).  So the forward evaluator multiplies fp32
// operands as three bf16 pieces each, a = a1 + a2 + a3 (8 mantissa bits per piece, by truncation, so the sum is
// exact for |a| >= 2^-100 and within 2^-132 below: tests/test_split_bf16_numerics.py), and keeps the six products down to 2^-16 relative size:
//     a b ~= a3 b1 + a2 b2 + a1 b3 + a2 b1 + a1 b2 + a1 b1          (error ~2^-22 |a b|, fp32 accumulation)
// on v_mfma_f32_32x32x16_bf16: 6/16 of the fp32 matrix time, hidden under the GELU.  Same chained-register design:
// D tile of layer l = B operand of layer l+1.  Lane (sample n = lane & 31, half h = lane >> 5) supplies, for k-step s
// of input tile ti = s >> 1, its registers r = 8 (s & 1) + j, j = 0..7, i.e. the neurons 32 ti + row_of(r, h); the
// weight image is permuted to match.  Layer 0 reads features k = 16 s + 8 h + j of the feature-major input.
// Half of the 160 KB of LDS of a CU, so two workgroups fit.  Which forms of the forward (mlp.hip) fit how often per CU, for the
// 68.6 KB image of 36-64-64-64-1 (at most 76.1 KB with 64 inputs and 4 outputs; registers allow four waves per SIMD):
//   W = 4  (mlp_fwd_split_kernel, 256 threads)      twice:  8 waves per CU, TWO per SIMD -- the image, not the registers, limits it
//   W = 8  (mlp_fwd_split_wg_kernel, 512 threads)   twice: 16 waves per CU, four per SIMD
//   W = 16 (mlp_fwd_split_wg_kernel, 1024 threads)  once:  16 waves per CU, four per SIMD (the registers limit it)
// The 32-wide nets (20 KB images) fit the four-wave form four times and more; their registers (up to 161) limit them.
constexpr int SPLIT_LDS_MAX = 80 * 1024;

struct SplitPlan {
  int ok;            // the image fits SPLIT_LDS_MAX (else the fp32 MFMA kernel is used)
  int base;          // float offset of the split image inside the packed buffer (multiple of 4: 16-byte records)
  int ns[MAXL];      // k-steps (16 inputs each) of layer l
  int w_rec[MAXL];   // record offset of layer l's weight image [to][s][piece][lane] (8 bf16 per record)
  int tail_rec;      // record offset of the fp32 tail (biases, final dot weights)
  int b_off[MAXL];   // float offsets inside the tail
  int wf_off;        // final dot weights [o][ti][r][h] (final_dot nets)
  int total_rec;
};

static void make_split_plan(const MlpPlan& p, SplitPlan& sp) {
  sp.base = (p.total + 3) & ~3;
  int rec = 0;
  const int nl = p.n_layers;
  for (int l = 0; l < MAXL; l++) sp.ns[l] = sp.w_rec[l] = sp.b_off[l] = 0;
  for (int l = 0; l < nl; l++) {
    const bool dot = (l == nl - 1) && p.final_dot;
    sp.ns[l] = l == 0 ? (p.dims[0] + 15) / 16 : 2 * p.tiles[l];
    sp.w_rec[l] = rec;
    if (!dot) rec += p.tiles[l + 1] * sp.ns[l] * 3 * 64;
  }
  sp.tail_rec = rec;
  int f = 0;
  for (int l = 0; l < nl; l++) {
    const bool dot = (l == nl - 1) && p.final_dot;
    if (dot) {
      sp.wf_off = f;
      f += p.dims[nl] * p.tiles[l] * 32;
    }
    sp.b_off[l] = f;
    f += dot ? 4 : p.tiles[l + 1] * 32;
  }
  if (!p.final_dot) sp.wf_off = 0;
  sp.total_rec = rec + (f + 3) / 4;
  sp.ok = (nl == 3 || nl == 4) && (size_t)sp.total_rec * 16 <= (size_t)SPLIT_LDS_MAX;
}

// three bf16 pieces of a float (top 16 bits of the running remainder); host + device, used by the pack kernel
__host__ __device__ inline void split3(float x, uint32_t (&piece)[3]) {
  float r = x;
#pragma unroll
  for (int i = 0; i < 3; i++) {
    uint32_t u;
    __builtin_memcpy(&u, &r, 4);
    piece[i] = u >> 16;
    const uint32_t t = u & 0xFFFF0000u;
    float tf;
    __builtin_memcpy(&tf, &t, 4);
    r -= tf;
  }
}

// eight fp32 registers -> three bf16x8 B operands
__device__ __forceinline__ void split8(const float (&x)[8], bf16x8& p1, bf16x8& p2, bf16x8& p3) {
  uint32_t a[8], b[8], c[8];
#pragma unroll
  for (int j = 0; j < 8; j++) {
    a[j] = __float_as_uint(x[j]);
    const float r1 = x[j] - __uint_as_float(a[j] & 0xFFFF0000u);
    b[j] = __float_as_uint(r1);
    const float r2 = r1 - __uint_as_float(b[j] & 0xFFFF0000u);
    c[j] = __float_as_uint(r2);
  }
  u32x4 q1, q2, q3;
#pragma unroll
  for (int i = 0; i < 4; i++) {  // v_perm_b32: {high half of odd element, high half of even element}
    q1[i] = __builtin_amdgcn_perm(a[2 * i + 1], a[2 * i], 0x07060302u);
    q2[i] = __builtin_amdgcn_perm(b[2 * i + 1], b[2 * i], 0x07060302u);
    q3[i] = __builtin_amdgcn_perm(c[2 * i + 1], c[2 * i], 0x07060302u);
  }
  p1 = __builtin_bit_cast(bf16x8, q1);
  p2 = __builtin_bit_cast(bf16x8, q2);
  p3 = __builtin_bit_cast(bf16x8, q3);
}

// bias rows of a D tile: registers 4q..4q+3 of lane half h are the consecutive rows 8q + 4h .. +3 -> one 128-bit read
// (every bias block of the split image starts on a 16-byte boundary)
template <int T>
__device__ __forceinline__ void init_bias4(f32x16 (&acc)[T], const float* __restrict__ bias_lds, int h) {
  const f32x4* __restrict__ b4 = reinterpret_cast<const f32x4*>(bias_lds);
#pragma unroll
  for (int to = 0; to < T; to++)
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const f32x4 v = b4[8 * to + 2 * q + h];
#pragma unroll
      for (int c = 0; c < 4; c++) acc[to][4 * q + c] = v[c];
    }
}

// ---- the same with TWO fp16 pieces per operand (round 3; opt-in, see psdf_mlp_forward_f16): a = a0 + a1, a0 = fp16(a) rounded
// to nearest (v_cvt_pk_f16_f32; the remainder is exact in fp32 and fits 12 bits), a1 = fp16(a - a0) to nearest (round 6; rounds
// 3-5 truncated both pieces, a one-sided error of up to 3 * 2^-23 per operand); products a1 b0 + a0 b1 + a0 b0 on v_mfma_f32_32x32x16_f16.
// Half the MFMAs and about half the splitting work of the three-piece bf16 scheme; gfx950's matrix pipe honours fp16 subnormals
// (attic/prototypes/mlp_fwd_split_f16.hip), so small low pieces keep an absolute precision of 2^-24; values must stay below 65504.
// The image keeps the three-slot record layout (slot 2 unused), so SplitPlan is shared.
// The low piece is fp16(fma(x, 1, -high)): v_fma_mixlo_f16 / v_fma_mixhi_f16 form x - high exactly and round it once, ONE
// instruction per element -- v_cvt_pk_f16_f32 + two fma-mix = three instructions per pair, where converting the high pieces
// back, a packed subtraction and a second packed conversion take five.  x - high is exact in fp32 either way, so the pieces are
// the same bits (tests/test_split_f16_numerics.py states the rounding).  `one` is 1.0f the optimiser cannot see through, and
// the file must be built with -fno-slp-vectorize (build.py: mlp.hip), both for the reasons given at split2 in
// mlp_bwd_split_f16.hip, which is this split on a pair.  Measured at four waves per SIMD, where the forward is bound by
// vector-ALU issue: profiles/mlp_fwd_issue_trims_ab.txt (at two waves per SIMD round 4 had measured it neutral).
// (Two forms of the two-piece split remain: this fma-mix form in the forwards here and in split2 of mlp_bwd_split_f16.hip,
// both in files built without the SLP vectoriser, and wsplit2 in mlp_wide.hip, the subtract-and-convert form on a pair in a
// file built with it; same pieces, different instructions.)
__device__ __forceinline__ void split8h(const float (&x)[8], f16x8& hi, f16x8& lo) {
  u32x4 qh, ql;
  float one = 1.0f;
  asm("" : "+s"(one));
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const h2v_t h2 = __builtin_convertvector(f32x2{x[2 * i], x[2 * i + 1]}, h2v_t);   // v_cvt_pk_f16_f32, nearest even
    h2v_t l2;
    l2[0] = (_Float16)__builtin_fmaf(x[2 * i], one, -(float)h2[0]);
    l2[1] = (_Float16)__builtin_fmaf(x[2 * i + 1], one, -(float)h2[1]);
    qh[i] = __builtin_bit_cast(uint32_t, h2);
    ql[i] = __builtin_bit_cast(uint32_t, l2);
  }
  hi = __builtin_bit_cast(f16x8, qh);
  lo = __builtin_bit_cast(f16x8, ql);
}
// two pieces of a float for the pack kernel: {hi, lo} as 16-bit patterns
__device__ __forceinline__ void split2h_bits(float x, uint32_t (&piece)[3]) {
  const h2v_t h2 = __builtin_convertvector(f32x2{x, 0.f}, h2v_t);
  const float r = x - (float)h2[0];
  const h2v_t l2 = __builtin_convertvector(f32x2{r, 0.f}, h2v_t);
  piece[0] = __builtin_bit_cast(uint32_t, h2) & 0xFFFFu;
  piece[1] = __builtin_bit_cast(uint32_t, l2) & 0xFFFFu;
  piece[2] = 0u;
}

// one k-step (16 inputs) into TO output tiles.  w_s -> record [to = 0][s][piece 0][lane 0]; `to` stride = ns*192 records.
template <int TO, bool F16 = false>
__device__ __forceinline__ void split_mac(f32x16 (&out)[TO], const float (&x)[8], const u32x4* __restrict__ w_s, int ns,
                                          int lane) {
  if constexpr (F16) {
    f16x8 bh, bl;
    split8h(x, bh, bl);
#pragma unroll
    for (int to = 0; to < TO; to++) {
      const u32x4* wt = w_s + to * ns * 192 + lane;
      const f16x8 ah = __builtin_bit_cast(f16x8, wt[0]);
      const f16x8 al = __builtin_bit_cast(f16x8, wt[64]);
      out[to] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, out[to], 0, 0, 0);  // smallest terms first
      out[to] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, out[to], 0, 0, 0);
      out[to] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, out[to], 0, 0, 0);
    }
    return;
  }
  bf16x8 b1, b2, b3;
  split8(x, b1, b2, b3);
#pragma unroll
  for (int to = 0; to < TO; to++) {
    const u32x4* wt = w_s + to * ns * 192 + lane;
    const bf16x8 a1 = __builtin_bit_cast(bf16x8, wt[0]);
    const bf16x8 a2 = __builtin_bit_cast(bf16x8, wt[64]);
    const bf16x8 a3 = __builtin_bit_cast(bf16x8, wt[128]);
    out[to] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3, b1, out[to], 0, 0, 0);  // smallest terms first
    out[to] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, b2, out[to], 0, 0, 0);
    out[to] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b3, out[to], 0, 0, 0);
    out[to] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, b1, out[to], 0, 0, 0);
    out[to] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b2, out[to], 0, 0, 0);
    out[to] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, out[to], 0, 0, 0);
  }
}

template <int TI, int TO, bool F16 = false>
__device__ __forceinline__ void split_chain(const f32x16 (&in)[TI], f32x16 (&out)[TO], const u32x4* __restrict__ w,
                                            int lane) {
#pragma unroll
  for (int s = 0; s < 2 * TI; s++) {
    float x[8];
#pragma unroll
    for (int j = 0; j < 8; j++) x[j] = in[s >> 1][8 * (s & 1) + j];
    split_mac<TO, F16>(out, x, w + s * 192, 2 * TI, lane);
  }
}

}  // namespace
