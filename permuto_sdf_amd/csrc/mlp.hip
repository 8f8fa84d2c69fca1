// Fused small-MLP evaluator for gfx950 (fp32 MFMA, LDS-staged weight tiles).
// Replaces the torch.nn.Sequential(Linear, GELU, ...) evaluators of the reference
// (permuto_sdf_py/models/models.py:153-161 SDF net, :451-470 background nets, :54-129,350 colour net,
// and the BASELINE 64x3 SDF variant).  The reference has no native MLP code; the oracle is torch.nn fp32.
//
// Formulation: everything is computed TRANSPOSED, Z^T[out x samples] = W[out x in] * H^T[in x samples],
// with v_mfma_f32_32x32x2_f32.  One wave owns a tile of 32 samples.
//   A operand (1 VGPR): lane l holds W[32*to + (l&31)][k(l>>5)]         -> read from LDS, pre-packed
//   B operand (1 VGPR): lane l holds H^T[k(l>>5)][sample (l&31)]
//   D (16 VGPRs):       lane l, reg r holds Z^T[32*to + (r&3)+8*(r>>2)+4*(l>>5)][sample (l&31)]
// Because a dot product may visit k in any order as long as A and B agree, the k-step "(tile ti, reg r)"
// is defined as the neuron pair { 32*ti + (r&3)+8*(r>>2) + 4*h : h = 0,1 }: then register r of the previous
// layer's D tile IS the B operand of that k-step.  Activations never leave registers and need no
// cross-lane movement between layers; only the weights are permuted (once, by psdf_mlp_pack).
// The first layer reads its B operand straight from the feature-major encoding output [K0, N]
// (two 128-B segments per wave load); the result is stored feature-major [OUT, N].
#include "psdf_common.h"
#include <type_traits>

#include "mlp_device.h"
#include "mlp_dispatch.h"

namespace {

// ---------------------------------------------------------------------------------------- packing
// One thread per packed float.  W_l is torch layout [dims[l+1]][dims[l]] row major.
struct PackArgs {
  MlpPlan plan;
  const float* W[MAXL];
  const float* b[MAXL];
};

__global__ void mlp_pack_kernel(PackArgs a, float* __restrict__ packed) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  const MlpPlan& p = a.plan;
  if (e >= p.total) return;
  int l = 0;
#pragma unroll
  for (int i = 1; i < MAXL; i++)
    if (i < p.n_layers && e >= p.w_off[i]) l = i;
  const int out_d = p.dims[l + 1], in_d = p.dims[l];
  const bool last = (l == p.n_layers - 1);
  float v = 0.f;
  if (e >= p.b_off[l]) {
    const int row = e - p.b_off[l];
    if (row < out_d) v = a.b[l][row];
  } else {
    const int q = e - p.w_off[l];
    int row, col;
    if (l == 0) {  // [to][s][lane], row stride WS
      const int lane = q % WS, s = (q / WS) % p.in_steps0, to = (q / WS) / p.in_steps0;
      row = (lane < 64) ? 32 * to + (lane & 31) : (1 << 20);
      col = 2 * s + (lane >> 5);
    } else if (last && p.final_dot) {  // [o][ti][r][h]
      const int h = q & 1, r = (q >> 1) & 15, ti = (q >> 5) % p.tiles[l], o = (q >> 5) / p.tiles[l];
      row = o;
      col = 32 * ti + row_of(r, h);
    } else {  // [to][ti][r/4][lane][r%4]: one 128-bit read per lane = the A operands of 4 consecutive k-steps
      const int j = q & 3, lane = (q >> 2) & 63, rq = (q >> 8) & 3, pr = q >> 10;
      const int r = 4 * rq + j, ti = pr % p.tiles[l], to = pr / p.tiles[l];
      row = 32 * to + (lane & 31);
      col = 32 * ti + row_of(r, lane >> 5);
    }
    if (row < out_d && col < in_d) v = a.W[l][(int64_t)row * in_d + col];
  }
  packed[e] = v;
}

// Split-bf16 image (mlp_device.h): one thread per 32-bit word = two bf16 of one piece of one lane record, or one float
// of the tail.
__global__ void mlp_pack_split_kernel(PackArgs a, SplitPlan sp, float* __restrict__ packed, int f16) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  const MlpPlan& p = a.plan;
  if (w >= sp.total_rec * 4) return;
  uint32_t* dst = reinterpret_cast<uint32_t*>(packed + sp.base);
  const int nl = p.n_layers;
  const int rec = w >> 2;
  if (rec >= sp.tail_rec) {
    const int f = w - sp.tail_rec * 4;
    float v = 0.f;
    for (int l = 0; l < nl; l++) {
      const bool dot = (l == nl - 1) && p.final_dot;
      const int nb = dot ? 4 : p.tiles[l + 1] * 32;
      if (f >= sp.b_off[l] && f < sp.b_off[l] + nb) {
        const int row = f - sp.b_off[l];
        if (row < p.dims[l + 1]) v = a.b[l][row];
      }
      if (dot && f >= sp.wf_off && f < sp.wf_off + p.dims[nl] * p.tiles[l] * 32) {
        const int q = f - sp.wf_off;  // [o][ti][r][h]
        const int h = q & 1, r = (q >> 1) & 15, ti = (q >> 5) % p.tiles[l], o = (q >> 5) / p.tiles[l];
        const int col = 32 * ti + row_of(r, h);
        if (col < p.dims[l]) v = a.W[l][(int64_t)o * p.dims[l] + col];
      }
    }
    dst[w] = __float_as_uint(v);
    return;
  }
  int l = 0;
  for (int i = 1; i < nl; i++) {
    const bool dot = (i == nl - 1) && p.final_dot;
    if (!dot && rec >= sp.w_rec[i]) l = i;
  }
  const int local = rec - sp.w_rec[l];
  const int lane = local & 63, piece = (local >> 6) % 3, s = (local / 192) % sp.ns[l], to = (local / 192) / sp.ns[l];
  const int row = 32 * to + (lane & 31), hh = lane >> 5;
  uint32_t out = 0;
  for (int e = 0; e < 2; e++) {
    const int j = 2 * (w & 3) + e;
    const int col = l == 0 ? 16 * s + 8 * hh + j : 32 * (s >> 1) + row_of(8 * (s & 1) + j, hh);
    float v = 0.f;
    if (row < p.dims[l + 1] && col < p.dims[l]) v = a.W[l][(int64_t)row * p.dims[l] + col];
    uint32_t pc[3];
    if (f16) split2h_bits(v, pc);      // two fp16 pieces (slot 2 unused)
    else split3(v, pc);
    out |= pc[piece] << (16 * e);
  }
  dst[w] = out;
}

// Forward of the whole net for one 32-sample tile; fills the hidden pre-activation free result in `hid`.
// T1,T2,T3: hidden widths in tiles of 32 (T3 == 0: only two hidden layers).
template <int T1, int T2, int T3>
struct Net {
  static constexpr int NH = (T3 > 0) ? 3 : 2;
  static constexpr int TL = (T3 > 0) ? T3 : T2;  // tiles of the last hidden layer
};

template <int T1, int T2, int T3, int OUT_T, bool FINAL_DOT>
__global__ void __launch_bounds__(PSDF_BLOCK, 2)
    mlp_fwd_kernel(MlpPlan p, int64_t N, const float* __restrict__ X, const float* __restrict__ packed,
                   const unsigned char* __restrict__ skip, float* __restrict__ Y) {
  extern __shared__ __align__(16) float lds[];
  for (int i = threadIdx.x; i < p.total; i += PSDF_BLOCK) lds[i] = packed[i];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // (scalar: the tile loop is uniform)
  const int h = lane >> 5, sl = lane & 31;
  const int K0 = p.dims[0];
  const int OUT = p.dims[p.n_layers];
  const int64_t ntiles = (N + 31) / 32;
  for (int64_t tile = (int64_t)blockIdx.x * 4 + wave; tile < ntiles; tile += (int64_t)gridDim.x * 4) {
    // compiler-only barrier: keeps the (loop-invariant) LDS weight reads inside the tile loop; without it
    // LICM hoists hundreds of them into VGPRs and the kernel spills
    asm volatile("" ::: "memory");
    const int64_t n = tile * 32 + sl;
    const int64_t nc = n < N ? n : N - 1;
    if (skip && __ballot(n < N && !skip[nc]) == 0) continue;  // every sample of the tile is masked
    // ---- layer 0: B operand from global (feature-major input)
    f32x16 h1[T1];
    init_bias<T1>(h1, lds + p.b_off[0], h);
    {
      const float* __restrict__ w0 = lds + p.w_off[0];
      const int steps = p.in_steps0;
      // all operand loads of a chunk are issued before the first MFMA consumes one (a load -> MFMA -> load chain
      // would expose one HBM latency per k-step)
      constexpr int XC = 16;
      for (int s0 = 0; s0 < steps; s0 += XC) {
        float xb[XC];
#pragma unroll
        for (int i = 0; i < XC; i++) {
          const int k = 2 * (s0 + i) + h;
          xb[i] = (s0 + i < steps && k < K0) ? X[(int64_t)k * N + nc] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < XC; i++) {
          if (s0 + i < steps) {
#pragma unroll
            for (int to = 0; to < T1; to++)
              h1[to] = __builtin_amdgcn_mfma_f32_32x32x2f32(w0[(to * steps + s0 + i) * WS + lane], xb[i], h1[to], 0, 0, 0);
          }
        }
      }
    }
    apply_gelu<T1>(h1);
    f32x16 h2[T2];
    init_bias<T2>(h2, lds + p.b_off[1], h);
    dense_chain<T1, T2>(h1, h2, lds + p.w_off[1], lane);
    apply_gelu<T2>(h2);
    constexpr int TL = (T3 > 0) ? T3 : T2;
    f32x16 hl[TL];
    if constexpr (T3 > 0) {
      init_bias<T3>(hl, lds + p.b_off[2], h);
      dense_chain<T2, T3>(h2, hl, lds + p.w_off[2], lane);
      apply_gelu<T3>(hl);
    } else {
#pragma unroll
      for (int t = 0; t < T2; t++) hl[t] = h2[t];
    }
    const int lf = p.n_layers - 1;
    if constexpr (FINAL_DOT) {
      const float* __restrict__ wf = lds + p.w_off[lf];
      for (int o = 0; o < OUT; o++) {
        float acc = 0.f;
#pragma unroll
        for (int ti = 0; ti < TL; ti++)
#pragma unroll
          for (int r = 0; r < 16; r++) acc = fmaf(wf[((o * TL + ti) * 16 + r) * 2 + h], hl[ti][r], acc);
        acc += __shfl_xor(acc, 32, 64);
        acc += lds[p.b_off[lf] + o];
        if (h == 0 && n < N) Y[(int64_t)o * N + n] = acc;
      }
    } else {
      f32x16 y[OUT_T];
      init_bias<OUT_T>(y, lds + p.b_off[lf], h);
      dense_chain<TL, OUT_T>(hl, y, lds + p.w_off[lf], lane);
      if (n < N) {
#pragma unroll
        for (int to = 0; to < OUT_T; to++)
#pragma unroll
          for (int r = 0; r < 16; r++) {
            const int row = 32 * to + row_of(r, h);
            if (row < OUT) Y[(int64_t)row * N + n] = y[to][r];
          }
      }
    }
  }
}

// The same evaluator on the bf16 matrix pipe with split fp32 operands (mlp_device.h, "split-bf16 operand path").
// CH: k-steps of layer 0 whose loads are issued together (= all of them when the input has <= 64 features).
// activation of the split forwards: packed arithmetic for the two-piece fp16 form (VALU-count bound), one element per
// instruction for the three-piece bf16 form (see gelu_rational / gelu_rational2 in gelu_device.h)
#define GELU_SPLIT(T_, H_)                        \
  do {                                            \
    if constexpr (F16) apply_gelu_packed<T_>(H_); \
    else apply_gelu_scalar<T_>(H_);               \
  } while (0)
// O32: how a lane addresses its layer-0 operands X[row][column].  The row bases X + row N are wave-uniform and stay on the scalar
// unit in both forms; with O32 a load is scalar base + ONE 32-bit per-lane byte offset (global_load_dword v, v_off, s[base:base+1]),
// computed once per tile: the lane's column, plus the h-half's eight rows.  No vector ALU per load.  The largest offset is
// 4 (N - 1) + 32 N, so the form is taken where 36 N fits 32 bits (x_offsets_fit32, per launch); beyond that the lane keeps two
// 64-bit pointers and every load adds the scalar row offset to one of them (what the kernel did for every N before).
__host__ __device__ inline bool x_offsets_fit32(int64_t N) { return (uint64_t)N * 36u <= 0xFFFFFFFFull; }

typedef const __attribute__((address_space(1))) char* xrow_t;   // a row's address: global memory, so that a load stays global_load

template <bool O32>
struct XLane {
  const float* __restrict__ X;   // uniform
  int64_t N;                     // uniform
  uint32_t v0, vh;               // O32: byte offset of the column; the same plus eight rows for the lanes of half 1
  const float* p0;               // !O32: the same two as pointers
  const float* ph;
  __device__ __forceinline__ XLane(const float* __restrict__ X_, int64_t N_, int64_t nc, int h) : X(X_), N(N_) {
    if constexpr (O32) {
      v0 = (uint32_t)nc * 4u;
      vh = v0 + (h ? (uint32_t)N * 32u : 0u);
      p0 = ph = nullptr;
    } else {
      v0 = vh = 0;
      p0 = X + nc;
      ph = p0 + (h ? (int64_t)8 * N : (int64_t)0);
    }
  }
  // A row as a wave-uniform cursor: the address of X[row][0] (O32) or its element offset row N; next() steps one row down.
  using Row = std::conditional_t<O32, xrow_t, int64_t>;
  __device__ __forceinline__ Row row(int r) const {
    if constexpr (O32) return (xrow_t)(X + (int64_t)r * N);
    else return (int64_t)r * N;
  }
  __device__ __forceinline__ Row next(Row r, bool step = true) const {
    if constexpr (O32) return r + (step ? N * 4 : (int64_t)0);
    else return r + (step ? N : (int64_t)0);
  }
  // The lane's column: half = false: X[row][column] in every lane; true: X[row + 8 h][column].  Asked for once per k-step, in the
  // block of its loads: the empty asm makes the 32-bit offset a value of THAT block, so that instruction selection sees
  // scalar base + zero-extended offset and takes the scalar-base form of the load (hoisted out of the block, the extension
  // arrives as a 64-bit vector register and every load gets a 64-bit vector add again).  At most one v_mov_b32 per k-step.
  using Col = std::conditional_t<O32, uint32_t, const float*>;
  __device__ __forceinline__ Col col(bool half) const {
    if constexpr (O32) {
      uint32_t o = half ? vh : v0;
      asm("" : "+v"(o));
      return o;
    } else {
      return half ? ph : p0;
    }
  }
  // The empty asm pins the row address to a scalar register pair the optimiser cannot see through: left alone it re-associates
  // (X + lane offset) + row offset, the 64-bit vector add per load.
  __device__ __forceinline__ float load(Row r, Col c) const {
    if constexpr (O32) {
      asm("" : "+s"(r));
      return *(const __attribute__((address_space(1))) float*)(r + c);
    } else {
      return c[r];
    }
  }
};

template <int T1, int T2, int T3, int OUT_T, bool FINAL_DOT, int CH, bool F16, int W, bool O32>
__device__ __forceinline__ void mlp_fwd_split_tiles(const MlpPlan& p, const SplitPlan& sp, int64_t N, const float* __restrict__ X,
                                                    const unsigned char* __restrict__ skip, float* __restrict__ Y) {
  extern __shared__ __align__(16) u32x4 simg[];
  const float* tail = reinterpret_cast<const float*>(simg + sp.tail_rec);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // (scalar: the tile loop is uniform)
  const int h = lane >> 5, sl = lane & 31;
  const int K0 = p.dims[0];
  const int OUT = p.dims[p.n_layers];
  const int ns0 = sp.ns[0];
  const int64_t ntiles = (N + 31) / 32;
  for (int64_t tile = (int64_t)blockIdx.x * W + wave; tile < ntiles; tile += (int64_t)gridDim.x * W) {
    asm volatile("" ::: "memory");  // keeps the loop-invariant LDS reads inside the tile loop (see mlp_fwd_kernel)
    const int64_t n = tile * 32 + sl;
    const int64_t nc = n < N ? n : N - 1;
    if (skip && __ballot(n < N && !skip[nc]) == 0) continue;
    // ---- layer 0: lane (n, h) reads features 16 s + 8 h + j; CH k-steps of loads in flight before their MFMAs
    f32x16 h1[T1];
    init_bias4<T1>(h1, tail + sp.b_off[0], h);
    const XLane<O32> xl(X, N, nc, h);
    for (int s0 = 0; s0 < ns0; s0 += CH) {
      float xs[CH][8];
#pragma unroll
      for (int i = 0; i < CH; i++) {
        const int sb = 16 * (s0 + i);  // wave-uniform
        const int rem = K0 - sb;       // rows of this k-step inside the input (wave-uniform)
        if (rem >= 16) {               // whole k-step: rows sb + 8 h + j
          auto r = xl.row(sb);
          const auto c = xl.col(true);
#pragma unroll
          for (int j = 0; j < 8; j++, r = xl.next(r)) xs[i][j] = xl.load(r, c);
        } else if (rem > 8) {          // partial, both halves: half 0 whole, half 1 has rows sb + 8 + j for j < rem - 8
          auto r = xl.row(sb);
          const auto c0 = xl.col(false), ch = xl.col(true);
#pragma unroll
          for (int j = 0; j < 8; j++, r = xl.next(r)) {
            const bool both = 8 + j < rem;                    // uniform
            const float v = xl.load(r, both ? ch : c0);       // where half 1 has no row it reads half 0's (inside the input)
            xs[i][j] = (both || h == 0) ? v : 0.f;
          }
        } else if (rem > 0) {          // partial, half 0 alone: rows sb + j for j < rem; every lane reads a row inside the input
          auto r = xl.row(sb);
          const auto c = xl.col(false);
#pragma unroll
          for (int j = 0; j < 8; j++, r = xl.next(r, j < rem)) {   // (the cursor stops on the last row)
            const float v = xl.load(r, c);
            xs[i][j] = (j < rem && h == 0) ? v : 0.f;
          }
        } else {
#pragma unroll
          for (int j = 0; j < 8; j++) xs[i][j] = 0.f;
        }
      }
      // branch-free: a k-step past the end multiplies zeros with the (finite) last weight record -- a guarded MFMA would
      // make the accumulators live across control flow (32 register copies per branch)
#pragma unroll
      for (int i = 0; i < CH; i++) {
        const int s = s0 + i < ns0 ? s0 + i : ns0 - 1;
        split_mac<T1, F16>(h1, xs[i], simg + sp.w_rec[0] + s * 192, ns0, lane);
      }
    }
    GELU_SPLIT(T1, h1);
    f32x16 h2[T2];
    init_bias4<T2>(h2, tail + sp.b_off[1], h);
    split_chain<T1, T2, F16>(h1, h2, simg + sp.w_rec[1], lane);
    GELU_SPLIT(T2, h2);
    constexpr int TL = (T3 > 0) ? T3 : T2;
    f32x16 hl[TL];
    if constexpr (T3 > 0) {
      init_bias4<T3>(hl, tail + sp.b_off[2], h);
      split_chain<T2, T3, F16>(h2, hl, simg + sp.w_rec[2], lane);
      GELU_SPLIT(T3, hl);
    } else {
#pragma unroll
      for (int t = 0; t < T2; t++) hl[t] = h2[t];
    }
    const int lf = p.n_layers - 1;
    if constexpr (FINAL_DOT) {
      const float* __restrict__ wf = tail + sp.wf_off;
      for (int o = 0; o < OUT; o++) {
        float acc = 0.f;
#pragma unroll
        for (int ti = 0; ti < TL; ti++)
#pragma unroll
          for (int r = 0; r < 16; r++) acc = fmaf(wf[((o * TL + ti) * 16 + r) * 2 + h], hl[ti][r], acc);
        acc += __shfl_xor(acc, 32, 64);
        acc += tail[sp.b_off[lf] + o];
        if (h == 0 && n < N) Y[(int64_t)o * N + n] = acc;
      }
    } else {
      f32x16 y[OUT_T];
      init_bias4<OUT_T>(y, tail + sp.b_off[lf], h);
      split_chain<TL, OUT_T, F16>(hl, y, simg + sp.w_rec[lf], lane);
      if (n < N) {
#pragma unroll
        for (int to = 0; to < OUT_T; to++)
#pragma unroll
          for (int r = 0; r < 16; r++) {
            const int row = 32 * to + row_of(r, h);
            if (row < OUT) Y[(int64_t)row * N + n] = y[to][r];
          }
      }
    }
  }
}

// W: waves of the workgroup, which share ONE weight image (the image, not the registers, is what limits the residency of the
// 64-wide nets: see SPLIT_LDS_MAX in mlp_device.h).  Wave w of workgroup b walks the tiles b W + w, + gridDim.x W, ...
template <int T1, int T2, int T3, int OUT_T, bool FINAL_DOT, int CH, bool F16, int W>
__device__ __forceinline__ void mlp_fwd_split_body(const MlpPlan& p, const SplitPlan& sp, int64_t N, const float* __restrict__ X,
                                                   const float* __restrict__ packed, const unsigned char* __restrict__ skip,
                                                   float* __restrict__ Y) {
  extern __shared__ __align__(16) u32x4 simg[];
  {
    const u32x4* __restrict__ src = reinterpret_cast<const u32x4*>(packed + sp.base);
    for (int i = threadIdx.x; i < sp.total_rec; i += W * 64) simg[i] = src[i];
  }
  __syncthreads();
  // one uniform branch per launch (the kernels' signatures and instantiations stay what the dispatch and resource tests pin)
  if (x_offsets_fit32(N)) mlp_fwd_split_tiles<T1, T2, T3, OUT_T, FINAL_DOT, CH, F16, W, true>(p, sp, N, X, skip, Y);
  else mlp_fwd_split_tiles<T1, T2, T3, OUT_T, FINAL_DOT, CH, F16, W, false>(p, sp, N, X, skip, Y);
}

// The four-wave form: every net of the SPLIT column, every batch size.
template <int T1, int T2, int T3, int OUT_T, bool FINAL_DOT, int CH, bool F16 = false>
__global__ void __launch_bounds__(PSDF_BLOCK, 2)
    mlp_fwd_split_kernel(MlpPlan p, SplitPlan sp, int64_t N, const float* __restrict__ X,
                         const float* __restrict__ packed, const unsigned char* __restrict__ skip,
                         float* __restrict__ Y) {
  mlp_fwd_split_body<T1, T2, T3, OUT_T, FINAL_DOT, CH, F16, 4>(p, sp, N, X, packed, skip, Y);
}

// The wide form: W waves on one image, four waves per SIMD (128 registers each: 512 per SIMD lane over four waves) -- W = 8 is
// two workgroups per CU, W = 16 one.  Built for the 64-wide nets only, and for one W (split_wide_built below).
template <int T1, int T2, int T3, int OUT_T, bool FINAL_DOT, int CH, bool F16, int W>
__global__ void __launch_bounds__(W * 64, 4)
    mlp_fwd_split_wg_kernel(MlpPlan p, SplitPlan sp, int64_t N, const float* __restrict__ X,
                            const float* __restrict__ packed, const unsigned char* __restrict__ skip,
                            float* __restrict__ Y) {
  mlp_fwd_split_body<T1, T2, T3, OUT_T, FINAL_DOT, CH, F16, W>(p, sp, N, X, packed, skip, Y);
}

// ---- which workgroup form a launch takes
// The wide form that is built.  W = 8 and W = 16 tie at the bench size (0.2580 / 0.2583 ms, profiles/mlp_fwd_forms_ab.txt); 8 is
// kept because it also holds between the powers of two (24 tiles per CU: 29 us against 36 us; two workgroups per CU overlap
// one's staging and tail with the other's tiles).
constexpr int SPLIT_WIDE_W = 8;
constexpr int SPLIT_WIDE_MIN_TILES_PER_CU = 16;   // the launch policy's threshold, see launch_fwd_split_ch

// The wide form exists where the weight image is what limits the residency and the kernel fits 128 registers without scratch:
// the 64-wide rows of PSDF_MLP32_ROWS with one output tile, <2, 2, 2, 1, true> (both piece forms) and <2, 2, 0, 1, true>.  The
// 32-wide rows have 20 KB images and up to 161 registers; they keep the four-wave form.
template <int T1, int T2, int T3, int OUT_T, bool FINAL_DOT, int W>
constexpr bool split_wide_built = T1 == 2 && T2 == 2 && (T3 == 2 || T3 == 0) && OUT_T == 1 && FINAL_DOT && W == SPLIT_WIDE_W;

int g_fwd_form_forced = 0;   // psdf_mlp_forward_set_form: 0 = by the launch policy
int g_fwd_form_last = 0;     // waves per workgroup of the last split forward launch

int mlp_device_cus() {
  static int cus[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  if (cus[dev] == 0) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cus[dev] = n;
  }
  return cus[dev];
}

// one launch of one form; the grid is ONE resident round (occupancy x CUs, asked once per kernel, device and image size), so the image
// is staged once per resident workgroup and every wave walks tiles for the rest of the launch
template <int W, auto KERN>
int launch_fwd_split_form(const MlpPlan& p, const SplitPlan& sp, int64_t N, const float* X, const float* packed,
                          const unsigned char* skip, float* Y, hipStream_t st) {
  const auto kern = KERN;
  const size_t shmem = (size_t)sp.total_rec * 16;
  if (shmem > 64 * 1024) {   // on every launch: the attribute belongs to the current device's copy of the kernel
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
    if (e != hipSuccess) return (int)e;
  }
  // workgroups per CU of THIS kernel (statics of the instantiation), per device and image size.  Host state like g_last_path:
  // not synchronised, one thread launches at a time.
  struct Round { size_t shmem; int per_cu; };
  static Round rounds[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  Round& r = rounds[dev];
  if (r.shmem != shmem || r.per_cu <= 0) {
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, W * 64, shmem) != hipSuccess || per_cu <= 0) {
      (void)hipGetLastError();
      per_cu = 2;        // what 160 KB of LDS allow a 64-wide net's image, in either form
    }
    r = Round{shmem, per_cu};
  }
  const int round_per_cu = r.per_cu;
  const int64_t ntiles = (N + 31) / 32;
  int64_t blocks = (ntiles + W - 1) / W;
  const int64_t cap = (int64_t)round_per_cu * mlp_device_cus();
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(W * 64), shmem, st, p, sp, N, X, packed, skip, Y);
  PSDF_LAUNCH_CHECK();
  g_fwd_form_last = W;
  return PSDF_OK;
}

// the wide form of W waves where it is built; -2 (and no launch) where it is not: a forced form this net does not have
template <int T1, int T2, int T3, int OUT_T, bool FINAL_DOT, int CH, bool F16, int W>
int launch_fwd_split_wide(const MlpPlan& p, const SplitPlan& sp, int64_t N, const float* X, const float* packed,
                          const unsigned char* skip, float* Y, hipStream_t st) {
  if constexpr (split_wide_built<T1, T2, T3, OUT_T, FINAL_DOT, W>)
    return launch_fwd_split_form<W, mlp_fwd_split_wg_kernel<T1, T2, T3, OUT_T, FINAL_DOT, CH, F16, W>>(p, sp, N, X, packed, skip, Y,
                                                                                                         st);
  else
    return PSDF_ERR_UNSUPPORTED;
}

// Launch policy.  The wide form is taken when every CU gets a full resident round of it, 16 tiles (two 8-wave workgroups);
// below that the four-wave form spreads a small batch (a training step's 49 K samples: 1536 tiles) over all CUs.  Measured on
// MI355X (256 CUs), us per launch, median of 15, forced forms (profiles/mlp_fwd_forms_ab.txt has the other nets; W = 16 was
// built for the measurement; the build had the shorter GELU tail the library has again since the operand trims, not these):
//                      36-64-64-64-1, fp16 pieces        36-64-64-64-1, bf16 pieces
//     N   tiles / CU    W = 4    W = 8   W = 16           W = 4    W = 8   W = 16
//    49 152      6       15.8     15.0     20.2            17.3     18.0     22.3
//    98 304     12       19.8     21.6     20.8            21.8     24.2     23.6
//   131 072     16       24.9     22.4     21.8            29.9     25.5     27.5
//   196 608     24       33.1     29.3     35.8            38.4     35.0     45.4
//   262 144     32       46.4     41.0     39.5            53.0     48.4     47.0
//   524 288     64       81.8     72.2     68.3            93.4     89.8     87.7
// 2 097 152    256      283.3    258.1    257.4           356.4    331.1    330.6
// From 16 tiles per CU on W = 8 is the fastest or within 6 % of it for every net; at 12 and below W = 4 is.
template <int T1, int T2, int T3, int OUT_T, bool FINAL_DOT, int CH, bool F16 = false>
int launch_fwd_split_ch(const MlpPlan& p, const SplitPlan& sp, int64_t N, const float* X, const float* packed,
                     const unsigned char* skip, float* Y, hipStream_t st) {
  constexpr bool WIDE = split_wide_built<T1, T2, T3, OUT_T, FINAL_DOT, SPLIT_WIDE_W>;
  int form = g_fwd_form_forced;
  if (form == 0) {
    const int64_t ntiles = (N + 31) / 32;
    form = WIDE && ntiles >= (int64_t)SPLIT_WIDE_MIN_TILES_PER_CU * mlp_device_cus() ? SPLIT_WIDE_W : 4;
  }
  if (form == 4)
    return launch_fwd_split_form<4, mlp_fwd_split_kernel<T1, T2, T3, OUT_T, FINAL_DOT, CH, F16>>(p, sp, N, X, packed, skip, Y, st);
  if (form == 8) return launch_fwd_split_wide<T1, T2, T3, OUT_T, FINAL_DOT, CH, F16, 8>(p, sp, N, X, packed, skip, Y, st);
  return launch_fwd_split_wide<T1, T2, T3, OUT_T, FINAL_DOT, CH, F16, 16>(p, sp, N, X, packed, skip, Y, st);
}

template <int T1, int T2, int T3, int OUT_T, bool FINAL_DOT>
int launch_fwd_split(const MlpPlan& p, const SplitPlan& sp, int64_t N, const float* X, const float* packed,
                     const unsigned char* skip, float* Y, hipStream_t st, bool f16 = false) {
  if constexpr (T1 == 2 && T2 == 2 && T3 == 2 && OUT_T == 1 && FINAL_DOT) {
    // the two-piece fp16 arithmetic is instantiated for the BASELINE net only (64x3 -> 1..4 outputs, <= 64 inputs)
    if (f16) {
      switch (sp.ns[0]) {
        case 1: return launch_fwd_split_ch<T1, T2, T3, OUT_T, FINAL_DOT, 1, true>(p, sp, N, X, packed, skip, Y, st);
        case 2: return launch_fwd_split_ch<T1, T2, T3, OUT_T, FINAL_DOT, 2, true>(p, sp, N, X, packed, skip, Y, st);
        case 3: return launch_fwd_split_ch<T1, T2, T3, OUT_T, FINAL_DOT, 3, true>(p, sp, N, X, packed, skip, Y, st);
        default: return launch_fwd_split_ch<T1, T2, T3, OUT_T, FINAL_DOT, 4, true>(p, sp, N, X, packed, skip, Y, st);
      }
    }
  } else if (f16) {
    return PSDF_ERR_UNSUPPORTED;
  }
  switch (sp.ns[0]) {  // up to 64 input features: one chunk, no padded k-step
    case 1: return launch_fwd_split_ch<T1, T2, T3, OUT_T, FINAL_DOT, 1>(p, sp, N, X, packed, skip, Y, st);
    case 2: return launch_fwd_split_ch<T1, T2, T3, OUT_T, FINAL_DOT, 2>(p, sp, N, X, packed, skip, Y, st);
    case 3: return launch_fwd_split_ch<T1, T2, T3, OUT_T, FINAL_DOT, 3>(p, sp, N, X, packed, skip, Y, st);
    default: return launch_fwd_split_ch<T1, T2, T3, OUT_T, FINAL_DOT, 4>(p, sp, N, X, packed, skip, Y, st);
  }
}

template <int T1, int T2, int T3, int OUT_T, bool FINAL_DOT>
int launch_fwd(const MlpPlan& p, int64_t N, const float* X, const float* packed, const unsigned char* skip, float* Y,
               hipStream_t st) {
  const size_t shmem = (size_t)p.total * sizeof(float);
  auto kern = mlp_fwd_kernel<T1, T2, T3, OUT_T, FINAL_DOT>;
  if (!fwd_fits(p)) return PSDF_ERR_UNSUPPORTED;
  if (shmem > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
    if (e != hipSuccess) return (int)e;
  }
  const int64_t ntiles = (N + 31) / 32;
  int64_t blocks = (ntiles + 3) / 4;
  const int64_t cap = 256 * 4;  // persistent-ish: the weight staging is amortised over many tiles
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(PSDF_BLOCK), shmem, st, p, N, X, packed, skip, Y);
  PSDF_LAUNCH_CHECK();
  return PSDF_OK;
}


}  // namespace

extern "C" {

// Number of floats of the packed (MFMA-operand ordered) parameter buffer for a net with the given
// layer widths: dims[0]=input .. dims[n_layers]=output.  Returns <0 on argument error.
int64_t psdf_mlp_packed_size(int n_layers, const int* dims) {
  MlpPlan p;
  if (make_plan(n_layers, dims, p) != PSDF_OK) return PSDF_ERR_ARG;
  SplitPlan sp;
  make_split_plan(p, sp);
  return sp.ok ? (int64_t)sp.base + (int64_t)sp.total_rec * 4 : (int64_t)p.total;
}

// weights[l]: device pointer to torch-layout W_l [dims[l+1], dims[l]]; biases[l]: [dims[l+1]].
static int mlp_pack_impl(int n_layers, const int* dims, const float* const* weights, const float* const* biases,
                         float* packed, void* stream, int f16) {
  PackArgs a;
  int rc = make_plan(n_layers, dims, a.plan);
  if (rc != PSDF_OK) return rc;
  // the two-piece fp16 image exists for the net psdf_mlp_forward_f16 is instantiated for
  if (f16 && !baseline_split_shape(n_layers, dims, 64, 4)) return PSDF_ERR_UNSUPPORTED;
  for (int l = 0; l < MAXL; l++) {
    a.W[l] = l < n_layers ? weights[l] : nullptr;
    a.b[l] = l < n_layers ? biases[l] : nullptr;
  }
  hipLaunchKernelGGL(mlp_pack_kernel, dim3(psdf_blocks(a.plan.total, 256)), dim3(256), 0, (hipStream_t)stream, a,
                     packed);
  PSDF_LAUNCH_CHECK();
  SplitPlan sp;
  make_split_plan(a.plan, sp);
  if (sp.ok) {  // second image of the same parameters: bf16 pieces in the operand order of mlp_fwd_split_kernel
    hipLaunchKernelGGL(mlp_pack_split_kernel, dim3(psdf_blocks(sp.total_rec * 4, 256)), dim3(256), 0,
                       (hipStream_t)stream, a, sp, packed, f16);
    PSDF_LAUNCH_CHECK();
  } else if (f16) {
    return PSDF_ERR_UNSUPPORTED;
  }
  return PSDF_OK;
}

int psdf_mlp_pack(int n_layers, const int* dims, const float* const* weights, const float* const* biases,
                  float* packed, void* stream) {
  return mlp_pack_impl(n_layers, dims, weights, biases, packed, stream, 0);
}

// The same buffer with the split image holding TWO fp16 pieces per weight: what psdf_mlp_forward_f16 consumes (and only it).
int psdf_mlp_pack_f16(int n_layers, const int* dims, const float* const* weights, const float* const* biases,
                      float* packed, void* stream) {
  return mlp_pack_impl(n_layers, dims, weights, biases, packed, stream, 1);
}

// X: [dims[0], N] feature-major; Y: [dims[n_layers], N] feature-major.  GELU (erf) after every layer but the last.
static int mlp_forward_impl(int n_layers, const int* dims, int64_t N, const float* X, const float* packed,
                            const unsigned char* skip, float* Y, void* stream, bool f16 = false) {
  MlpPlan p;
  int rc = make_plan(n_layers, dims, p);
  if (rc != PSDF_OK) return rc;
  if (N == 0) return PSDF_OK;
  if (N < 0 || !X || !packed || !Y) return PSDF_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int t1 = p.tiles[1], t2 = p.tiles[2], t3 = (n_layers == 4) ? p.tiles[3] : 0, to = p.tiles[n_layers];
  if (n_layers != 3 && n_layers != 4) return PSDF_ERR_UNSUPPORTED;
  if (f16 && !baseline_split_shape(n_layers, dims, 64, 4)) return PSDF_ERR_UNSUPPORTED;   // (the only net psdf_mlp_pack_f16 packs)
  SplitPlan sp;
  make_split_plan(p, sp);
  // the rows of PSDF_MLP32_ROWS (mlp_dispatch.h); S: the split-bf16 kernel is built for the row
#define CASE(A, B, C, O, D, FWD, S, F16)                                        \
  PSDF_IF(FWD, if (t1 == A && t2 == B && t3 == C && to == O && p.final_dot == D) { \
    if (f16 && !F16) return PSDF_ERR_UNSUPPORTED;                               \
    if constexpr (S) {                                                          \
      if (sp.ok) {                                                              \
        psdf::g_last_path[psdf::PATH_MLP_FWD] = f16 ? 3 : 2;                    \
        return launch_fwd_split<A, B, C, O, D>(p, sp, N, X, packed, skip, Y, st, f16); \
      }                                                                         \
    }                                                                           \
    if (f16) return PSDF_ERR_UNSUPPORTED;                                       \
    psdf::g_last_path[psdf::PATH_MLP_FWD] = 1;                                  \
    return launch_fwd<A, B, C, O, D>(p, N, X, packed, skip, Y, st);             \
  })
  PSDF_MLP32_ROWS(CASE)
#undef CASE
  return PSDF_ERR_UNSUPPORTED;
}


int psdf_mlp_forward(int n_layers, const int* dims, int64_t N, const float* X, const float* packed, float* Y,
                     void* stream) {
  return mlp_forward_impl(n_layers, dims, N, X, packed, nullptr, Y, stream);
}

// The same evaluation with TWO fp16 pieces per fp32 operand (three products) for a buffer made by psdf_mlp_pack_f16: the
// BASELINE net only (dims = {<= 64, 64, 64, 64, <= 4}; -2 otherwise).  Opt-in: max error ~3e-6 of the largest output instead of
// ~1e-6, and inputs / activations / weights must stay below 65504 in magnitude (the three-piece bf16 form has no such limit).
int psdf_mlp_forward_f16(int n_layers, const int* dims, int64_t N, const float* X, const float* packed, float* Y,
                         void* stream) {
  return mlp_forward_impl(n_layers, dims, N, X, packed, nullptr, Y, stream, true);
}

// Same with a per-sample mask: 32-sample tiles whose samples all have skip[n] != 0 are not evaluated (their Y entries
// are left as they are); partially masked tiles are evaluated in full.
int psdf_mlp_forward_masked(int n_layers, const int* dims, int64_t N, const float* X, const float* packed,
                            const unsigned char* skip, float* Y, void* stream) {
  return mlp_forward_impl(n_layers, dims, N, X, packed, skip, Y, stream);
}

// Test and A/B hook: forces the workgroup form of the split forward (waves per workgroup: 4, 8 or 16; 0 = the launch policy
// decides) for the process, until it is called again.  A forward whose net has no kernel of the forced form returns -2 and
// launches nothing.  -1 for any other value.
int psdf_mlp_forward_set_form(int waves) {
  if (waves != 0 && waves != 4 && waves != 8 && waves != 16) return PSDF_ERR_ARG;
  g_fwd_form_forced = waves;
  return PSDF_OK;
}

// Waves per workgroup of the last split forward launch (0: none yet).  psdf_last_path(2) keeps naming the arithmetic.
int psdf_mlp_forward_last_form(void) { return g_fwd_form_last; }

}  // extern "C"
