// Permutohedral-lattice hash encoding for gfx950: forward, backward (lattice + positions) and
// double backward (from positions).  Replaces the CUDA op of the un-vendored package
// `permutohedral_encoding` that the reference imports at permuto_sdf_py/models/models.py:20 and calls
// at models.py:186,370,500,542.  Algorithm and frozen conventions: SURVEY.md App. A / oracle/permuto_oracle.py.
//
// Data layout in HBM
//   positions      [N, P]      fp32 row major (what the callers hand over)
//   lattice_values [L, T, F]   fp32 ("monolithic"; per-level table = T*F*4 B = 2 MiB at T=2^18, F=2)
//   sliced         [Lt*F, N]   fp32 feature-major (Lt = L + ceil(P/F) when points are concatenated):
//                              every store of a wave is one 256-B line, and the consumer (the fused MLP,
//                              mlp.hip) reads its MFMA B-operand rows straight from this layout.
// Launch shape of the forward: grid (one resident round of workgroups, slots).  A slot is a coarse level together with a fine
// one -- slot i holds levels i and L - 1 - i, a thread computes both for its point (encode_fwd_pair_kernel; the plan is
// forward_slots of encode_plan.h) -- or a single level: the middle level of an odd L, the pseudo-levels, every level when
// pairing is off (PSDF_ENC_FWD_PAIRS=0 / psdf_encode_set_forward_pairs(0): encode_fwd_kernel, grid (.., Lt), one thread per
// (point, level)).  blockIdx.x is the fast dispatch dimension, so the chip sweeps one slot at a time: the fine level's 2-MiB
// table stays resident in every XCD's 4-MiB L2 (the gathers are L2 hits, HBM sees positions + outputs only) and the coarse
// level beside it reads a few dozen to a few thousand rows of its own.
#include <cstdio>
#include <cstring>
#include <mutex>
#include <type_traits>
#include <vector>

#include "encode_device.h"
#include "encode_plan.h"

namespace {

// ------------------------------------------------------------------------------------------ forward
// What the per-(point, level) body needs besides the point: the kernels' arguments, bundled inside the kernel (the compiler
// dissolves the struct: every member stays the scalar register it was).
struct FwdArgs {
  int64_t N;
  int L;
  uint32_t capacity;
  EncConv conv;
  const float *lattice, *scale_factor, *shifts, *window;
  float points_scaling;
  int pad_points;
  float* sliced;
  unsigned char* touched;
  int touch_shift, blocks_per_level;
};

// One (point, level) between its gathers and its weighted sum: the P+1 table rows as loaded and their weights bary_r * window.
template <int P, int F>
struct FwdGather {
  float fv[P + 1][F];
  float bw[P + 1];
};

// The levels without gathers (workgroup-uniform): true when `level` was one of them and its rows are written.
template <int P, int F>
__device__ __forceinline__ bool fwd_level_flat(const FwdArgs& A, int level, int64_t n, const float (&pos)[P]) {
  if (level >= A.L) {  // pseudo-levels carrying the scaled input point (zero padded)
    const int e = level - A.L;
#pragma unroll
    for (int f = 0; f < F; f++) {
      const int d = e * F + f;
      float v = 0.f;
#pragma unroll
      for (int i = 0; i < P; i++)
        if (i == d) v = pos[i] * A.points_scaling;
      // channel L*F + d; d >= P exists only in the zero-padded pseudo-level layout (encode_conventions.h)
      if (d < P || A.pad_points) A.sliced[((int64_t)level * F + f) * A.N + n] = v;
    }
    return true;
  }
  if (A.window[level] == 0.f) {  // a level the coarse-to-fine window keeps closed (workgroup-uniform): its channels are
                                 // 0 * (finite rows) = 0, no simplex, no gathers, nothing to mark (its backward contributes nothing either)
#pragma unroll
    for (int f = 0; f < F; f++) A.sliced[((int64_t)level * F + f) * A.N + n] = 0.f;
    return true;
  }
  return false;
}

// An open lattice level, first half: locate the simplex, mark the touched blocks, ISSUE all P+1 gathers.  fwd_level_finish
// consumes them; a caller may start a second level in between.
template <int P, int F, bool PLAIN>
__device__ __forceinline__ void fwd_level_gather(const FwdArgs& A, int level, int64_t n, const float (&pos)[P], FwdGather<P, F>& g) {
  const float w = A.window[level];
  Simplex<P> s;
  compute_simplex<P>(pos, A.shifts + level * P, A.scale_factor + level * P, s, A.conv.tie_later);
  const float* __restrict__ table = A.lattice + (int64_t)level * A.capacity * F;
  // issue all P+1 gathers before consuming them (independent 8-B loads in flight)
  uint32_t row[P + 1];
  vertex_rows<P>(s, A.capacity, row, A.conv.hash_c);
  // Training forward: remember which blocks of table rows this batch reads.  Every lattice-gradient contribution of the
  // backward / double backward at these positions lands on exactly these rows, so the optimiser can skip blocks whose
  // gradient and moments are still exactly zero (optim.hip: adamw_blocks_kernel) -- a superset is all it needs.
  if (!PLAIN && A.touched) {
#pragma unroll
    for (int r = 0; r <= P; r++) A.touched[(int64_t)level * A.blocks_per_level + (row[r] >> A.touch_shift)] = 1;
  }
#pragma unroll
  for (int r = 0; r <= P; r++) {
    // 32-bit byte offset from the level's table (a wave-uniform base): one shift per gather instead of a 64-bit shift-add
    // (a level of the table is below 4 GiB: checked by the launcher)
    const char* tb = reinterpret_cast<const char*>(table);
    if (F == 2) {
      float2 t = *reinterpret_cast<const float2*>(tb + (row[r] * 8u));
      g.fv[r][0] = t.x;
      g.fv[r][F - 1] = t.y;
    } else {
#pragma unroll
      for (int f = 0; f < F; f++) g.fv[r][f] = *reinterpret_cast<const float*>(tb + (row[r] * (uint32_t)(F * 4) + (uint32_t)(f * 4)));
    }
  }
#pragma unroll
  for (int r = 0; r <= P; r++) g.bw[r] = s.bary[r] * w;
}

// Second half: the weighted sum of the gathered rows, and the level's F output rows.
template <int P, int F>
__device__ __forceinline__ void fwd_level_finish(const FwdArgs& A, int level, int64_t n, const FwdGather<P, F>& g) {
  float acc[F];
#pragma unroll
  for (int r = 0; r <= P; r++) {
#pragma unroll
    for (int f = 0; f < F; f++) acc[f] = r == 0 ? g.fv[r][f] * g.bw[r] : acc[f] + g.fv[r][f] * g.bw[r];   // (0 + x: the sign of a zero only)
  }
#pragma unroll
  for (int f = 0; f < F; f++) A.sliced[((int64_t)level * F + f) * A.N + n] = acc[f];
}

// The whole body of one (point, level): what encode_fwd_kernel does per thread, and the pair kernel for a slot's only level.
template <int P, int F, bool PLAIN>
__device__ __forceinline__ void fwd_level(const FwdArgs& A, int level, int64_t n, const float (&pos)[P]) {
  if (fwd_level_flat<P, F>(A, level, n, pos)) return;
  FwdGather<P, F> g;
  fwd_level_gather<P, F, PLAIN>(A, level, n, pos, g);
  fwd_level_finish<P, F>(A, level, n, g);
}

template <int P, int F, bool PLAIN = false>   // PLAIN: no skip mask, no touched-block map (their arguments are ignored)
__global__ void __launch_bounds__(PSDF_BLOCK)
    encode_fwd_kernel(int64_t N, int L, uint32_t capacity, EncConv conv, const float* __restrict__ positions,
                      const float* __restrict__ lattice, const float* __restrict__ scale_factor,
                      const float* __restrict__ shifts, const float* __restrict__ window, float points_scaling,
                      int pad_points, const unsigned char* __restrict__ skip, float* __restrict__ sliced,
                      unsigned char* __restrict__ touched, int touch_shift, int blocks_per_level) {
  // (Round 4 measured an XCD-pinned shape -- a 1-D grid whose workgroup id i lands on XCD i % 8, each XCD taking two or three
  // levels for ALL points so that a table is fetched into one L2 instead of eight: 0.358 -> 0.631 ms at 2 M points, 16 levels
  // (profiles/r04_enc_ab.jsonl).  Eight XCDs streaming eight different tables each touch every position and write every
  // output row with 1/8 of the chip; the level-at-a-time sweep below keeps all 256 CUs on one 2-MiB table.)
  const FwdArgs A{N, L, capacity, conv, lattice, scale_factor, shifts, window, points_scaling, pad_points, sliced, touched,
                  touch_shift, blocks_per_level};
  const int level = blockIdx.y;
  const int64_t ntiles = (N + PSDF_BLOCK - 1) / PSDF_BLOCK;
  // a workgroup walks tiles blockIdx.x, blockIdx.x + gridDim.x, ... of its level (gridDim.x = the number of tiles unless the
  // launcher caps it: then the level's constants are fetched once per workgroup instead of once per tile)
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t n = tile * PSDF_BLOCK + threadIdx.x;
    if (n >= N) continue;
    if (!PLAIN && skip && skip[n]) continue;  // masked point (fixed-shape callers, e.g. converged rays): its columns stay untouched
    float pos[P];
    load_pos<P>(positions, n, pos);
    fwd_level<P, F, PLAIN>(A, level, n, pos);
  }
}

// A loop-invariant scalar, made opaque for one trip of the tile loop.  Left alone the compiler hoists everything derived from
// such a value out of the loop -- a level's pointers into the constants, its table and its output rows, the powers of the hash
// multiplier, every uniform condition as a 64-bit lane mask -- and holds it in scalar registers across the loop: with two levels
// per thread that is more than the 102 a wave may have at 8 waves per SIMD (measured: 24 spilled in <3, 2, PLAIN>, 50 in the
// general form).  Through this the derived values are recomputed per tile on the scalar unit, which has nothing else to do here.
template <class T>
__device__ __forceinline__ T per_tile(T v) {
  asm volatile("" : "+s"(v));
  return v;
}

// The same (point, level) bodies, two levels per thread: slot blockIdx.y of the plan names a level from the coarse end and one
// from the fine end (encode_plan.h: forward_slots).  The position is loaded once, both simplices are located and all 2 (P+1)
// gathers are issued before any is consumed -- the coarse level's gathers hit L1 and its time is vector issue, the fine level's
// go to L2 and its time is waiting for them, so each fills the other's idle resource (profiles/enc_fwd_levels.txt).  Whether a
// slot runs that way is decided once per workgroup: a slot with one level (the middle levels, the pseudo-levels), or with a level
// that the window has closed, runs the plain body level after level.  Outputs are bit-identical to encode_fwd_kernel: the same
// expressions per (point, level), no sum across levels.  One resident round of workgroups per slot walks the tiles, as there.
template <int P, int F, bool PLAIN = false>
__global__ void __launch_bounds__(PSDF_BLOCK)
    encode_fwd_pair_kernel(int64_t N, int L, uint32_t capacity, EncConv conv, const float* __restrict__ positions,
                           const float* __restrict__ lattice, const float* __restrict__ scale_factor,
                           const float* __restrict__ shifts, const float* __restrict__ window, float points_scaling,
                           int pad_points, const unsigned char* __restrict__ skip, float* __restrict__ sliced,
                           unsigned char* __restrict__ touched, int touch_shift, int blocks_per_level,
                           psdf::enc_plan::FwdSlots slots) {
  const FwdArgs A{N, L, capacity, conv, lattice, scale_factor, shifts, window, points_scaling, pad_points, sliced, touched,
                  touch_shift, blocks_per_level};
  const int la = slots.a[blockIdx.y], lb = slots.b[blockIdx.y];   // lb == FWD_SLOT_NONE: a single level
  const bool two = lb != psdf::enc_plan::FWD_SLOT_NONE;
  const bool together = two && la < L && lb < L && window[la] != 0.f && window[lb] != 0.f;
  const uint32_t ntiles = (uint32_t)((N + PSDF_BLOCK - 1) / PSDF_BLOCK);   // (32 bits: the launcher checks; three scalar registers)
  if (together) {
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
      const int64_t n = (int64_t)tile * PSDF_BLOCK + threadIdx.x;
      if (n >= N) continue;
      if (!PLAIN) {   // masked point (fixed-shape callers, e.g. converged rays): its columns stay untouched
        const unsigned char* sk = per_tile(skip);
        if (sk && sk[n]) continue;
      }
      float pos[P];
      load_pos<P>(positions, n, pos);
      const int xa = per_tile(la), xb = per_tile(lb);
      FwdArgs B = A;
      B.capacity = per_tile(A.capacity);
      B.conv.hash_c = per_tile(A.conv.hash_c);
      B.conv.tie_later = per_tile(A.conv.tie_later);
      if (!PLAIN) B.touched = per_tile(A.touched);
      // (the coarse level first: 263.5 against 265.0 us with the fine one first, 2 M points x 16 levels, profiles/enc_fwd_pairs_ab.txt)
      FwdGather<P, F> ga, gb;
      fwd_level_gather<P, F, PLAIN>(B, xa, n, pos, ga);
      fwd_level_gather<P, F, PLAIN>(B, xb, n, pos, gb);
      fwd_level_finish<P, F>(A, xa, n, ga);
      fwd_level_finish<P, F>(A, xb, n, gb);
    }
  } else {
    // level after level (a second one only where the window has closed a member of a pair): ONE copy of the plain body
    for (int k = 0; k < (two ? 2 : 1); k++) {
      const int level = k ? lb : la;
      for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t n = (int64_t)tile * PSDF_BLOCK + threadIdx.x;
        if (n >= N) continue;
        if (!PLAIN) {
          const unsigned char* sk = per_tile(skip);
          if (sk && sk[n]) continue;
        }
        float pos[P];
        load_pos<P>(positions, n, pos);
        fwd_level<P, F, PLAIN>(A, per_tile(level), n, pos);
      }
    }
  }
}


// ------------------------------------------------------------------- LDS-privatised scatter-add
// The lattice gradient is a scatter-add of (P+1)*F floats per (point, level).  At coarse levels the whole
// batch lands on a few dozen table rows, and fp32 atomics to one address serialise (measured: 135 ms for
// 2M points x 16 levels with plain global atomics).  Each workgroup therefore owns a direct-mapped cache
// in LDS (tag = table row, F partial sums) that it fills with LDS atomics while it walks its share of the
// points of one level.  A row whose slot is taken by another row bypasses the cache, so the structure is exact
// for any distribution; a workgroup whose hit rate is poor after its first tiles (fine, fully hashed levels)
// switches the cache off for the rest of its walk (vote after its first tile: share of contributions that hit an
// entry which already existed).
// The way out depends on the path.  Plain path (batches below the queue plan's threshold): what bypasses the cache is
// a global float atomic, and `flush` ends the workgroup with one global float atomic per live value.  Queue path: what
// bypasses the cache goes to the level's queues, and so does the cache itself -- at once when it is voted off
// (cache_drain_to_queue), in one reservation round at the end of the walk when it is kept (cache_drain_once).  The queue
// path is thereby left with NO global float atomic except the queue-full fallback of the pushes and drains.
constexpr uint32_t SC_EMPTY = 0xFFFFFFFFu;
constexpr uint32_t Q_NONE = 0xFFFFFFFFu;   // "no contribution" in a thread's list of rows (rows are < capacity <= 2^31)
#if !defined(PSDF_ENC_QSPT)
#define PSDF_ENC_QSPT 2
#endif
constexpr int QUEUE_SPT = PSDF_ENC_QSPT;   // points per thread and super-tile in queue mode (see ScatterCache)

// LDS float accumulation without ds_add_f32.  Measured on this chip (tools/atomic_bench.hip): a wave-wide ds_add_f32
// costs ~197 cycles whatever the access pattern (1 lane per ~3 cycles), while INTEGER LDS atomics run at LDS speed
// (ds_add_u32 10 cycles, ds_cmpst_rtn_b32 12, ds_add_u64 16, plain 8-byte read-modify-write 18).  So a pair of
// floats is added with one 64-bit compare-and-swap: read, add in registers, ds_cmpst_rtn_b64; lanes that lose the
// race (another lane or wave changed the pair) retry up to 3 times, and whatever is still pending after that -- heavy
// same-address contention, where the constant-cost float atomic is the better tool -- falls back to ds_add_f32.
// `hot` remembers that fallback per thread for a few adds so that a contended stream stops paying for doomed attempts.
__device__ __forceinline__ void lds_add_pair(float* p, float a, float b, int& hot) {
  if (hot == 0) {
    unsigned long long* q = reinterpret_cast<unsigned long long*>(p);
    unsigned long long old = *q;
#pragma unroll
    for (int it = 0; it < 4; it++) {  // k lanes of a wave on one pair need k rounds: covers multiplicity <= 4
      const float x = __uint_as_float((uint32_t)old) + a;
      const float y = __uint_as_float((uint32_t)(old >> 32)) + b;
      const unsigned long long want = (unsigned long long)__float_as_uint(x) | ((unsigned long long)__float_as_uint(y) << 32);
      const unsigned long long prev = atomicCAS(q, old, want);
      if (prev == old) return;
      old = prev;
    }
    hot = 8;  // heavily shared pair: use the float atomic for the next few adds, then probe again
  } else {
    hot--;
  }
  atomicAdd(p, a);
  atomicAdd(p + 1, b);
}

// Adjacent lanes are adjacent samples of a ray, and at coarse and medium levels they sit in the same simplex: their
// contributions go to the same rows.  Such runs of equal rows are summed in registers (segmented inclusive scan
// inside each 16-lane DPP row, Hillis-Steele with head flags) and only the LAST lane of a run hands the sum on, so
// that what reaches LDS has a multiplicity of at most 4 per wave -- within reach of the retries of lds_add_pair.
// Returns true on the lanes that own a (partial) run sum.
template <int F>
__device__ __forceinline__ bool combine_runs16(uint32_t key, float (&v)[F]) {
  constexpr int ROW_SHR = 0x110, ROW_SHL = 0x100;
  // key Q_NONE: a lane without a contribution (v = 0).  Such lanes may join each other -- they add zeros and never own a run.
  const int k = (int)key;
  // Every cross-lane move uses bound_ctrl: a lane that would read across the edge of its 16-lane row receives 0 from the
  // instruction itself (otherwise the compiler preloads each destination with a v_mov: 10 per contribution).  The flag is
  // therefore kept INVERTED -- j = 1: "joined to the run of the lane before" -- so that the 0 shifted in means "a run starts
  // here".  (The first lane of a row may read j = 1 against the shifted-in key 0; everything it then adds is a shifted-in 0.)
  const int kprev = __builtin_amdgcn_update_dpp(0, k, ROW_SHR | 1, 0xf, 0xf, true);
  const float joined = (kprev == k) ? 1.0f : 0.0f;
  // The flag is a float 1.0 / 0.0 and the conditional add is ONE fused multiply-add per feature whose shifted operand comes
  // through DPP (v_fmac_f32_dpp: v = shifted(v) * j + v; exact -- a product by 1 or 0 -- instead of v_add_dpp + v_cmp + v_cndmask),
  // the flag update one v_mul_f32_dpp: 3 instructions per step for F = 2, was 7.  (A non-finite contribution now also spoils the
  // lanes of its row that are NOT in its run, 0 x inf; such a step is lost either way.)
  float j = joined;
#define PSDF_SCAN_STEP(D)                                                                                        \
  {                                                                                                              \
    _Pragma("unroll") for (int i = 0; i < F; i++) v[i] = __builtin_fmaf(                                         \
        __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v[i]), ROW_SHR | D, 0xf, 0xf, true)), j, v[i]); \
    j = j * __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(j), ROW_SHR | D, 0xf, 0xf, true));      \
  }
  PSDF_SCAN_STEP(1)
  PSDF_SCAN_STEP(2)
  PSDF_SCAN_STEP(4)
  PSDF_SCAN_STEP(8)
#undef PSDF_SCAN_STEP
  // the lane after: joined to this one (0 shifted in past the end of the row: a run ends with its row)
  const int next_joined = __builtin_amdgcn_update_dpp(0, __float_as_int(joined), ROW_SHL | 1, 0xf, 0xf, true);
  return key != Q_NONE && next_joined == 0;
}

// TOTAL = slots x F.  8192 (48 KiB for F = 2) where the cache is all there is between the contributions and global float
// atomics (small batches); 4096 (24 KiB) in queue mode, where what the cache does not absorb goes to the queues anyway:
// there the binning kernel was held at 3 waves per SIMD by both its LDS and its registers while it spent 48 % of its wave
// cycles waiting (profiles/r02_pmc_sq_encode_bwd.txt) -- half the cache and 2 instead of 4 points per thread and super-tile
// (half the per-thread contribution registers) let more waves in: binning + reduce 0.894 -> 0.828 ms on the bench batch.
template <int F, int TOTAL = 8192>
struct ScatterCache {
  static constexpr int SC_SLOTS = TOTAL / F;  // F=2, TOTAL 8192: 16 KiB tags + 32 KiB sums
  uint32_t* tags;
  float* sums;
  int* stats;  // [0] = hits, [1] = tries, [2] = enabled
  __device__ __forceinline__ void init(float* lds) {
    tags = reinterpret_cast<uint32_t*>(lds);
    sums = lds + SC_SLOTS;
    stats = reinterpret_cast<int*>(lds + SC_SLOTS + SC_SLOTS * F);
    for (int i = threadIdx.x; i < SC_SLOTS; i += blockDim.x) tags[i] = SC_EMPTY;
    for (int i = threadIdx.x; i < SC_SLOTS * F; i += blockDim.x) sums[i] = 0.f;
    if (threadIdx.x == 0) {
      stats[0] = 0;
      stats[1] = 0;
      stats[2] = 1;
    }
    __syncthreads();
  }
  // 0: slot taken by another row (caller adds to HBM / queues); 1: absorbed, claimed an empty slot;
  // 2: absorbed into an entry that already existed (a genuine re-use: what the adaptive vote counts)
  __device__ __forceinline__ int add(uint32_t row, const float* v, int& hot) {
    const uint32_t slot = (row ^ (row >> 12)) & (SC_SLOTS - 1);
    uint32_t old = tags[slot];
    if (old == SC_EMPTY) old = atomicCAS(&tags[slot], SC_EMPTY, row);
    if (old == SC_EMPTY || old == row) {
      static_assert(F % 2 == 0, "pairs");
#pragma unroll
      for (int f = 0; f < F; f += 2) lds_add_pair(&sums[slot * F + f], v[f], v[f + 1], hot);
      return old == row ? 2 : 1;
    }
    return 0;
  }
  __device__ __forceinline__ void flush(float* __restrict__ table_grad) {
    __syncthreads();
    for (int i = threadIdx.x; i < SC_SLOTS; i += blockDim.x) {
      const uint32_t row = tags[i];
      if (row != SC_EMPTY) {
#pragma unroll
        for (int f = 0; f < F; f++) {
          const float v = sums[i * F + f];
          if (v != 0.f) atomicAdd(table_grad + (int64_t)row * F + f, v);
        }
      }
    }
  }
  static constexpr size_t bytes() { return (size_t)(SC_SLOTS + SC_SLOTS * F + 4) * 4; }
};

// ----------------------------------------------------------------------------------------- backward
// grad_lattice[l][row][f] += bary_r * w_l * g[l][f][n]            (LDS-privatised; then fp32 L2 atomics on the plain path,
//                                                                   the queues and encode_bwd_reduce_kernel on the queue path)
// grad_pos[n][i]          += dL/dpos_i  (chain through barycentric -> elevated -> position)
// Launch: grid (B, Lt), workgroup b of level l walks point tiles b, b+B, ...
template <typename SC>
__device__ __forceinline__ bool cache_vote(SC& sc, int hits, int tries) {
  // called by every thread of the workgroup after its first tile; returns the workgroup-uniform decision
  hits = (int)psdf::wave_sum((float)hits);
  tries = (int)psdf::wave_sum((float)tries);
  if (psdf::lane_id() == 0) {
    atomicAdd(&sc.stats[0], hits);
    atomicAdd(&sc.stats[1], tries);
  }
  __syncthreads();
  return sc.stats[0] * 8 >= sc.stats[1];  // keep the cache when >= 1/8 of the first tile hit an existing entry
}

// Binned hand-off to the LDS reduction (large batches, fully hashed levels).  fp32 global atomics are capped at
// ~21 G/s on this chip whatever the placement (tools/atomic_bench.hip) while LDS atomics sustain >= 185 G/s, so
// the contributions of a workgroup that is NOT served by its scatter cache are appended to per-(level, partition)
// queues instead of being added to HBM one atomic at a time: partition p owns table rows [p*RPP, (p+1)*RPP),
// RPP*F floats = 128 KiB = one workgroup's LDS.  Slots are reserved per tile with LDS counters and ONE global
// atomic per (tile, partition); encode_bwd_reduce_kernel then folds every queue into LDS and adds the slice to
// the gradient with plain stores.  A queue that is full falls back to the global atomic (exact either way).
// A queue entry is a (row, F values) pair: one contribution, a run of them summed in registers, or -- from a workgroup that is
// served by its cache -- a drained cache entry, the partial sum of everything that workgroup saw of the row.  The coarse
// levels' queues hold little else.  Capacity: an entry stands for at least one contribution that was not queued itself, so
// no queue receives more entries than its rows have contributions, whatever the caches absorb (encode_plan.h sizes it for
// 1.25 x an even share of all of them).
struct Queues {
  uint16_t* rows;  // [L, NP, cap]      row index inside the partition
  float* vals;     // [L, NP, cap, F]
  int* tails;      // [L, NP]           zeroed per call
  int cap, np, shift;  // rows per partition = 1 << shift
};
using psdf::enc_plan::Q_MAX_PARTS;   // encode_plan.h: the queue plan is sized by it
constexpr int Q_LDS_INTS = 4 * Q_MAX_PARTS + 4;   // q_cnt, q_base, q_off (+1), q_gd; 3 vote words

// Workgroup-collective append of up to NC contributions per thread to the level's partition queues.
// Slots are reserved with an LDS counter per partition and ONE global atomic per (call, partition).
// Addressing (round 5: the binning kernel is VALU bound, profiles/r05_pmc_sq_encode_bwd.txt, and the 64-bit entry offset
// ((level * np + part) * cap + idx) took 12 vector instructions per contribution): the level's slice of the queues is a
// wave-uniform base pointer; the entry offset inside it is 32 bits (queue_plan refuses plans whose level slice exceeds 2^32
// bytes) and comes out of LDS ready made -- next to a partition's reserved tail (q_base[part], for the "queue full" test) sits
// part * cap + tail (q_aux[part], 64 ints further: one ds_read2_b32 fetches both) -- so that a contribution needs two adds.
struct LevelQueues {
  char* rows;   // Q.rows + level * np * cap                [np, cap] uint16
  char* vals;   // Q.vals + level * np * cap * F            [np, cap, F] float
  uint32_t mask;   // rows per partition - 1
};
template <int F>
__device__ __forceinline__ LevelQueues level_queues(const Queues& Q, int level) {
  const int64_t e = (int64_t)level * Q.np * Q.cap;
  return LevelQueues{reinterpret_cast<char*>(Q.rows + e), reinterpret_cast<char*>(Q.vals + e * F), (1u << Q.shift) - 1u};
}
template <int F>
__device__ __forceinline__ void queue_store(const LevelQueues& LQ, uint32_t o, uint32_t row, const float* v) {
  *reinterpret_cast<uint16_t*>(LQ.rows + (o * 2u)) = (uint16_t)(row & LQ.mask);
  if (F == 2) {
    *reinterpret_cast<float2*>(LQ.vals + (o * 8u)) = make_float2(v[0], v[F - 1]);
  } else {
#pragma unroll
    for (int f = 0; f < F; f++) *reinterpret_cast<float*>(LQ.vals + (o * (uint32_t)(F * 4) + (uint32_t)(f * 4))) = v[f];
  }
}

template <int NC, int F>
__device__ __forceinline__ void queue_push(const Queues& Q, int level, int* q_cnt, int* q_base,
                                           const uint32_t (&crow)[NC], const float (&cval)[NC][F],
                                           float* __restrict__ table_grad) {
  int* q_aux = q_base + Q_MAX_PARTS;
  const LevelQueues LQ = level_queues<F>(Q, level);
  if (threadIdx.x < Q.np) q_cnt[threadIdx.x] = 0;
  __syncthreads();
  int slot[NC];
#pragma unroll
  for (int r = 0; r < NC; r++)
    if (crow[r] != Q_NONE) slot[r] = atomicAdd(&q_cnt[crow[r] >> Q.shift], 1);
  __syncthreads();
  if (threadIdx.x < Q.np) {
    const int c = q_cnt[threadIdx.x];
    const int base = c ? atomicAdd(&Q.tails[level * Q.np + threadIdx.x], c) : 0;
    q_base[threadIdx.x] = base;
    q_aux[threadIdx.x] = (int)threadIdx.x * Q.cap + base;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < NC; r++) {
    if (crow[r] == Q_NONE) continue;
    const int part = crow[r] >> Q.shift;
    const int idx = q_base[part] + slot[r];
    if (idx < Q.cap) {
      queue_store<F>(LQ, (uint32_t)(q_aux[part] + slot[r]), crow[r], cval[r]);
    } else {  // queue full: exact fallback
#pragma unroll
      for (int f = 0; f < F; f++) atomicAdd(table_grad + (int64_t)crow[r] * F + f, cval[r][f]);
    }
  }
}

// Same hand-off with COALESCED stores, for workgroups whose scatter cache is switched off (its 48 KiB of LDS are free):
// a direct append makes every lane of a store instruction hit a different partition's queue, and the address
// processing of such scattered 2-/8-byte stores (one lane per cycle per CU) was the limiter of the binning kernel.
// Here the contributions of the super-tile are first laid out in LDS grouped by partition (counting sort: the slot
// inside the group comes from the same LDS counter that reserves the queue segment), then written out linearly, so a
// wave writes 64 consecutive queue entries.
template <int NC>
__device__ __forceinline__ void queue_push_staged(const Queues& Q, int level, int* q_cnt, int* q_base, int* q_off, int* q_gd,
                                                  float* stage, const uint32_t (&crow)[NC],
                                                  const float (&cval)[NC][2], float* __restrict__ table_grad) {
  uint32_t* st_row = reinterpret_cast<uint32_t*>(stage);                 // [NC * PSDF_BLOCK]
  float2* st_val = reinterpret_cast<float2*>(stage + NC * PSDF_BLOCK);   // [NC * PSDF_BLOCK]
  const LevelQueues LQ = level_queues<2>(Q, level);
  if (threadIdx.x < Q.np) q_cnt[threadIdx.x] = 0;
  __syncthreads();
  int slot[NC];
#pragma unroll
  for (int r = 0; r < NC; r++)
    if (crow[r] != Q_NONE) slot[r] = atomicAdd(&q_cnt[crow[r] >> Q.shift], 1);
  __syncthreads();
  if (threadIdx.x < 64) {   // the first wave: segment offsets by a wave scan (np <= 64).  A serial walk over the counters by
    // thread p (p LDS reads in a dependent chain, up to 31 of them, inside a barrier-separated phase) cost 4.5 % of the pair.
    const int lane = threadIdx.x;
    const int c = lane < Q.np ? q_cnt[lane] : 0;
    const int incl = psdf::wave_incl_scan_add_i(c);
    if (lane < Q.np) {
      // staged entry i of partition p goes to queue slot tail_p + (i - off_p): what the write-out loop needs per entry is
      // i + (tail_p - off_p) for the "queue full" test and i + (p * cap + tail_p - off_p) as the offset in the level's slice
      // (q_gd: written here, behind two barriers of this call, and read by the write-out loop of this call only -- so the
      // next call may start while slower waves are still in that loop, no barrier at the end)
      const int base = c ? atomicAdd(&Q.tails[level * Q.np + lane], c) : 0;
      const int off = incl - c;
      q_off[lane] = off;
      q_base[lane] = base - off;
      q_gd[lane] = lane * Q.cap + base - off;
      if (lane == Q.np - 1) q_off[Q.np] = incl;
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < NC; r++)
    if (crow[r] != Q_NONE) {
      const int i = q_off[crow[r] >> Q.shift] + slot[r];
      st_row[i] = crow[r];
      st_val[i] = make_float2(cval[r][0], cval[r][1]);
    }
  __syncthreads();
  const int total = q_off[Q.np];
  for (int i = threadIdx.x; i < total; i += PSDF_BLOCK) {
    const uint32_t row = st_row[i];
    const float2 v = st_val[i];
    const int part = row >> Q.shift;
    const int idx = i + q_base[part];
    if (idx < Q.cap) {
      const float vv[2] = {v.x, v.y};
      queue_store<2>(LQ, (uint32_t)(i + q_gd[part]), row, vv);
    } else {  // queue full: exact fallback
      atomicAdd(table_grad + (int64_t)row * 2, v.x);
      atomicAdd(table_grad + (int64_t)row * 2 + 1, v.y);
    }
  }
}

// The scatter cache was switched off: hand its live entries to the queues too (instead of flushing them with one
// global atomic each at the end) and empty it.
template <int F, typename SC>
__device__ __forceinline__ void cache_drain_to_queue(SC& sc, const Queues& Q, int level, int* q_cnt,
                                                     int* q_base, float* __restrict__ table_grad) {
  for (int base = 0; base < SC::SC_SLOTS; base += PSDF_BLOCK) {
    const int i = base + threadIdx.x;
    uint32_t crow[1];
    float cval[1][F];
    const uint32_t tag = sc.tags[i];
    static_assert(SC_EMPTY == Q_NONE, "an empty slot is 'no contribution'");
    crow[0] = tag;
#pragma unroll
    for (int f = 0; f < F; f++) cval[0][f] = sc.sums[i * F + f];
    queue_push<1, F>(Q, level, q_cnt, q_base, crow, cval, table_grad);
    sc.tags[i] = SC_EMPTY;
  }
  __syncthreads();
}

// The scatter cache was KEPT to the end of the walk (coarse and medium levels): its live entries leave through the queues as
// well, in ONE reservation round for the whole cache.  (cache_drain_to_queue above pushes 256 slots at a time -- SC_SLOTS / 256
// rounds of three barriers and a returning global atomic per partition: fine once, behind the first tile of a workgroup that goes
// on working, a serial tail at the end of one.)  Two walks over the tags, nothing kept in registers between them:
//   count    every thread counts its tagged slots into the per-partition LDS counters
//   reserve  thread p reserves partition p's segment with one atomic on Q.tails and clears the counter again
//   write    the second walk takes each entry's place in the segment from the same counters and writes it
// A tagged slot holds at least one contribution that was therefore NOT queued, so a partition's queue never receives more
// entries than the level has contributions to that partition's rows -- what queue_plan sizes it for, with its 25 % margin,
// whether a cache absorbs anything or not.  Past the end of a queue: the float atomic, as everywhere.
// drained (profile build): where the workgroup adds the number of entries it handed over.
template <int F, typename SC>
__device__ __forceinline__ void cache_drain_once(const SC& sc, const Queues& Q, int level, int* q_cnt, int* q_base,
                                                 float* __restrict__ table_grad, int* drained) {
  int* q_aux = q_base + Q_MAX_PARTS;
  const LevelQueues LQ = level_queues<F>(Q, level);
  // (the last readers of q_cnt are behind a barrier of the last queue_push; q_base / q_aux, which a slow wave may still be
  // reading there, are written behind the two barriers below)
  if (threadIdx.x < Q.np) q_cnt[threadIdx.x] = 0;
  __syncthreads();   // also: every add of the walk has landed in the cache
  for (int i = threadIdx.x; i < SC::SC_SLOTS; i += PSDF_BLOCK) {
    const uint32_t row = sc.tags[i];
    if (row != SC_EMPTY) atomicAdd(&q_cnt[row >> Q.shift], 1);
  }
  __syncthreads();
  if (threadIdx.x < Q.np) {
    const int c = q_cnt[threadIdx.x];
    const int base = c ? atomicAdd(&Q.tails[level * Q.np + threadIdx.x], c) : 0;
    q_base[threadIdx.x] = base;
    q_aux[threadIdx.x] = (int)threadIdx.x * Q.cap + base;
    q_cnt[threadIdx.x] = 0;
    if (drained && c) atomicAdd(drained, c);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < SC::SC_SLOTS; i += PSDF_BLOCK) {
    const uint32_t row = sc.tags[i];
    if (row == SC_EMPTY) continue;
    const int part = row >> Q.shift;
    const int slot = atomicAdd(&q_cnt[part], 1);
    float v[F];
#pragma unroll
    for (int f = 0; f < F; f++) v[f] = sc.sums[i * F + f];
    if (q_base[part] + slot < Q.cap) {
      queue_store<F>(LQ, (uint32_t)(q_aux[part] + slot), row, v);
    } else {  // queue full: exact fallback
#pragma unroll
      for (int f = 0; f < F; f++) atomicAdd(table_grad + (int64_t)row * F + f, v[f]);
    }
  }
}

// Queue mode asks for 5 waves per SIMD: left alone the compiler takes 162 VGPRs (3 waves), told so it needs 96 without a
// vector spill, and the kernel waits on LDS / gathers for half of its wave cycles (profiles/r02_pmc_sq_encode_bwd.txt), so the
// extra residents pay: bench batch 0.835 -> 0.79 ms (4 waves: no change; 6 waves spill 13 VGPRs).  The 24-KiB cache of queue
// mode lets 5 workgroups share a CU's LDS.  (P = 4 and F = 4 would spill a few VGPRs at 5 waves: they ask for 4.)
// A queue-mode workgroup ends by handing what is left in its cache to the queues (cache_drain_once: two walks over the tags,
// nothing held in registers between them, so the budget above stands) -- it issues no global float atomic unless a queue is full.
// DBL = true: the DOUBLE backward's lattice scatter through the same machinery (see encode_dbl_bwd_kernel for the maths): the
// coefficient of vertex r is q_r (the directional derivative of its barycentric along u = dd_positions) instead of bary_r, and
// the kernel also writes grad_grad_sliced = sum_r q_r w lattice[row_r] (a gather of the rows it has just computed; skipped
// when the pointer is NULL).  grad_sliced2 (optional): the PLAIN backward's scatter of a second upstream gradient rides along,
// row_r += w (q_r g + bary_r g2) -- a training step scatters both onto the same rows of the same simplices (the double backward
// of the normals and the backward of the features), so one simplex, one run combine, one queue pass and one reduce serve both.
// Workgroups per level (round 5).  The launch is ONE resident round of workgroups, and with an equal share per level the
// coarse levels (everything absorbed by the LDS cache) were done in half the time of the fine ones (everything queued): level
// durations 0.29 .. 0.55 ms inside a 0.57-ms kernel (profiles/r03_enc_profile_levels.txt), closed levels of a coarse-to-fine
// window holding their share for nothing.  With a plan (n > 0) the grid is one-dimensional, workgroup i serves the level whose
// range [first[l], first[l + 1]) holds it, and it reports its duration (100-MHz ticks, tagged with the launch's generation)
// into host-mapped memory; the host re-deals the round in proportion to count x duration at the next call (encode_balance).
struct LevelPlan {
  int n;                    // 0: rectangular grid (blockIdx.y = level)
  uint32_t gen;             // low 8 bits tag the entries of `times`
  uint32_t* times;          // [workgroups] or NULL
  uint16_t first[42];
};
template <int P, int F, bool LATTICE, bool POS, bool QUEUE, bool DBL = false>
#if !defined(PSDF_ENC_QWAVES)
#define PSDF_ENC_QWAVES 5
#endif
__global__ void __launch_bounds__(PSDF_BLOCK, QUEUE ? ((P <= 3 && F == 2) ? PSDF_ENC_QWAVES : 4) : 1)
    encode_bwd_kernel(int64_t N, int L, uint32_t capacity, EncConv conv, const float* __restrict__ positions,
                      const float* __restrict__ lattice, const float* __restrict__ scale_factor,
                      const float* __restrict__ shifts, const float* __restrict__ window, float points_scaling,
                      const float* __restrict__ grad_sliced, float* __restrict__ grad_lattice,
                      float* __restrict__ grad_positions, Queues Q, const float* __restrict__ dd_positions = nullptr,
                      float* __restrict__ grad_grad_sliced = nullptr, int pad_points = 0,
                      const float* __restrict__ grad_sliced2 = nullptr, LevelPlan plan = LevelPlan{}) {
  static_assert(!(DBL && POS), "the double backward has no position output");
  extern __shared__ __align__(16) float lds[];
#if defined(PSDF_ENC_PROFILE)
  const long long psdf_prof_t0 = (long long)wall_clock64();
#endif
  int level = blockIdx.y, bx = blockIdx.x, gx = gridDim.x;
  long long plan_t0 = 0;
  if (plan.n) {
    level = 0;
    for (int l = 1; l < plan.n; l++)
      if ((int)blockIdx.x >= (int)plan.first[l]) level = l;
    bx = (int)blockIdx.x - (int)plan.first[level];
    gx = (int)plan.first[level + 1] - (int)plan.first[level];
    plan_t0 = (long long)wall_clock64();
  }
  // duration of this workgroup, for the host's next deal (at least 1 tick: 0 means "not written")
  auto plan_report = [&]() {
    if (plan.n && plan.times && threadIdx.x == 0) {
      long long dt = (long long)wall_clock64() - plan_t0;
      dt = dt < 1 ? 1 : (dt > 0xFFFFFF ? 0xFFFFFF : dt);
      __hip_atomic_store(plan.times + blockIdx.x, ((plan.gen & 255u) << 24) | (uint32_t)dt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  };
  const int64_t ntiles = (N + PSDF_BLOCK - 1) / PSDF_BLOCK;
  if (level >= L) {
    if (DBL) {   // concatenated-point channels: grad_g = u_d * points_scaling
      const int e = level - L;
      for (int64_t tile = bx; tile < ntiles; tile += gx) {
        const int64_t n = tile * PSDF_BLOCK + threadIdx.x;
        if (n >= N) continue;
        float u[P];
        load_pos<P>(dd_positions, n, u);
#pragma unroll
        for (int f = 0; f < F; f++) {
          const int d = e * F + f;
          float v = 0.f;
#pragma unroll
          for (int i = 0; i < P; i++)
            if (i == d) v = u[i] * points_scaling;
          if ((d < P || pad_points) && grad_grad_sliced) grad_grad_sliced[((int64_t)level * F + f) * N + n] = v;
        }
      }
    }
    if (POS) {
      const int e = level - L;
      for (int64_t tile = bx; tile < ntiles; tile += gx) {
        const int64_t n = tile * PSDF_BLOCK + threadIdx.x;
        if (n >= N) continue;
#pragma unroll
        for (int f = 0; f < F; f++) {
          const int d = e * F + f;
          if (d < P)
            atomicAdd(grad_positions + n * P + d, grad_sliced[((int64_t)level * F + f) * N + n] * points_scaling);
        }
      }
    }
    plan_report();
    return;
  }
  if (window[level] == 0.f) {   // closed level (workgroup-uniform, before any barrier): every contribution carries the factor 0
    if (DBL && grad_grad_sliced) {
      for (int64_t tile = bx; tile < ntiles; tile += gx) {
        const int64_t n = tile * PSDF_BLOCK + threadIdx.x;
        if (n >= N) continue;
#pragma unroll
        for (int f = 0; f < F; f++) grad_grad_sliced[((int64_t)level * F + f) * N + n] = 0.f;
      }
    }
    plan_report();
    return;
  }
  using SCache = ScatterCache<F, QUEUE ? 4096 : 8192>;
  SCache sc;
  int* q_cnt = reinterpret_cast<int*>(lds + SCache::bytes() / 4);  // [Q_MAX_PARTS]
  int* q_base = q_cnt + Q_MAX_PARTS;                                          // [Q_MAX_PARTS]
  int* q_off = q_base + Q_MAX_PARTS;                                          // [Q_MAX_PARTS + 1]
  int* q_gd = q_off + Q_MAX_PARTS + 1;                                        // [Q_MAX_PARTS]
  int* q_vote = q_gd + Q_MAX_PARTS;                                           // [3]
  if (QUEUE && threadIdx.x < 3) q_vote[threadIdx.x] = 0;   // (a barrier follows in sc.init)
  if (LATTICE) sc.init(lds);
  bool use_cache = LATTICE;
  int hot = 0;  // lds_add_pair: >0 while this thread's adds are contended (go straight to the float atomic)
  int hits = 0, tries = 0, iter = 0;
  const float w = window[level];
  const int64_t tbase = (int64_t)level * capacity * F;
  float sfl[P], shl[P];
#pragma unroll
  for (int i = 0; i < P; i++) {
    sfl[i] = scale_factor[level * P + i];
    shl[i] = shifts[level * P + i];
  }
  // In queue mode a thread handles SPT points per tile, so that one round of slot reservation (3 barriers and a
  // returning global atomic per partition) is amortised over SPT*256 points.
  constexpr int SPT = QUEUE ? QUEUE_SPT : 1;
  constexpr int NC = SPT * (P + 1);
  const int64_t ntiles_w = (N + (int64_t)PSDF_BLOCK * SPT - 1) / ((int64_t)PSDF_BLOCK * SPT);
  for (int64_t tile = bx; tile < ntiles_w; tile += gx, iter++) {
    uint32_t crow[NC];
    float cval[NC][F];
#pragma unroll
    for (int c = 0; c < NC; c++) {
      crow[c] = Q_NONE;   // until the thread's point fills it in; again after the combine where another lane / the cache took it
#pragma unroll
      for (int f = 0; f < F; f++) cval[c][f] = 0.f;
    }
#pragma unroll
    for (int sp = 0; sp < SPT; sp++) {
      const int64_t n = (tile * SPT + sp) * PSDF_BLOCK + threadIdx.x;
      if (n < N) {
        float g[F], g2[F];
#pragma unroll
        for (int f = 0; f < F; f++) {
          g[f] = grad_sliced[((int64_t)level * F + f) * N + n];
          g2[f] = (DBL && grad_sliced2) ? grad_sliced2[((int64_t)level * F + f) * N + n] : 0.f;
        }
        float pos[P];
        load_pos<P>(positions, n, pos);
        Simplex<P> s;
        compute_simplex<P>(pos, shl, sfl, s, conv.tie_later);
        float dbary[P + 2];
#pragma unroll
        for (int k = 0; k <= P + 1; k++) dbary[k] = 0.f;
        float q[P + 2], gg[F];
        if (DBL) {   // q_r = sum_i u_i d bary_r / d pos_i: adjoint of pos -> elevated -> barycentric slots
          float u[P];
          load_pos<P>(dd_positions, n, u);
          float aE[P + 1];
#pragma unroll
          for (int j = 0; j <= P; j++) aE[j] = 0.f;
#pragma unroll
          for (int k = 0; k < P; k++) {
            const float us = u[k] * sfl[k];
#pragma unroll
            for (int j = 0; j <= k; j++) aE[j] = aE[j] + us;
            aE[k + 1] = aE[k + 1] - us * (float)(k + 1);
          }
#pragma unroll
          for (int k = 0; k <= P + 1; k++) q[k] = 0.f;
          const float invp = 1.0f / (P + 1);
#pragma unroll
          for (int i = 0; i <= P; i++) {
            const float t = aE[i] * invp;
#pragma unroll
            for (int k = 0; k <= P + 1; k++) {
              if (k == P - s.rank[i]) q[k] = q[k] + t;
              if (k == P + 1 - s.rank[i]) q[k] = q[k] - t;
            }
          }
          q[0] = q[0] + q[P + 1];
#pragma unroll
          for (int f = 0; f < F; f++) gg[f] = 0.f;
        }
        uint32_t rows[P + 1];
        vertex_rows<P>(s, capacity, rows, conv.hash_c);
#pragma unroll
        for (int r = 0; r <= P; r++) {
          const uint32_t row = rows[r];
          if (DBL && grad_grad_sliced) {
            const float qw = q[r] * w;
#pragma unroll
            for (int f = 0; f < F; f++) gg[f] = gg[f] + qw * lattice[tbase + (int64_t)row * F + f];
          }
          if (LATTICE) {
            const int c = sp * (P + 1) + r;
            const float bw = (DBL ? q[r] : s.bary[r]) * w;
            crow[c] = row;
#pragma unroll
            for (int f = 0; f < F; f++) cval[c][f] = g[f] * bw;
            if (DBL && grad_sliced2) {
              const float bw2 = s.bary[r] * w;
#pragma unroll
              for (int f = 0; f < F; f++) cval[c][f] = cval[c][f] + g2[f] * bw2;
            }
          }
          if (POS) {
#pragma unroll
            for (int f = 0; f < F; f++) dbary[r] = dbary[r] + lattice[tbase + (int64_t)row * F + f] * w * g[f];
          }
        }
        if (DBL && grad_grad_sliced) {
#pragma unroll
          for (int f = 0; f < F; f++) grad_grad_sliced[((int64_t)level * F + f) * N + n] = gg[f];
        }
        if (POS) {
          dbary[P + 1] = dbary[P + 1] + dbary[0];  // adjoint of bary[0] += 1 + bary[P+1]
          float dE[P + 1];
          const float invp = 1.0f / (P + 1);
#pragma unroll
          for (int i = 0; i <= P; i++) {
            float a = 0.f, b = 0.f;
#pragma unroll
            for (int k = 0; k <= P + 1; k++) {
              if (k == P - s.rank[i]) a = dbary[k];
              if (k == P + 1 - s.rank[i]) b = dbary[k];
            }
            dE[i] = (a - b) * invp;
          }
#pragma unroll
          for (int i = 0; i < P; i++) {
            float acc = 0.f;
#pragma unroll
            for (int j = 0; j <= i; j++) acc = acc + dE[j];
            acc = acc - dE[i + 1] * (float)(i + 1);
            atomicAdd(grad_positions + n * P + i, acc * sfl[i]);
          }
        }
      }
    }
    if (LATTICE) {
      // all lanes (also those past the end of the batch) take part in the DPP run combine
#pragma unroll
      for (int c = 0; c < NC; c++) {
        // (also when the cache has been voted off: skipping the combine there was measured, round 3 -- encode backward pair
        // 0.78 -> 0.92 ms, the runs of the mid levels are what keeps their queue traffic down)
        // (also where neighbouring samples do not share rows -- the finest levels: a per-workgroup vote that skips the combine
        // when the first tile merged < 1/16 of its contributions was measured in round 4 and made the pair SLOWER, 0.798 ->
        // 0.835 ms on the bench step, profiles/r04_bench_combine_vote_ab.txt: the scan is cheaper than the vote's bookkeeping)
        const bool own = combine_runs16<F>(crow[c], cval[c]);
        bool absorbed = false;
        if (own && use_cache) {
          const int rc = sc.add(crow[c], cval[c], hot);
          absorbed = rc != 0;
          hits += (rc == 2);
          tries++;
        }
        if (!own || absorbed) crow[c] = Q_NONE;
      }
    }
    if (LATTICE) {
      if (QUEUE) {
        // everything the cache did not absorb goes to the queues (also while the cache is on: rays are spatially
        // coherent, so a mid level can re-use entries AND overflow the 4096 slots)
        uint32_t all = Q_NONE;   // all ones: the AND of the rows is Q_NONE iff every one of them is
#pragma unroll
        for (int c = 0; c < NC; c++) all &= crow[c];
        const bool any = all != Q_NONE;
        // Does any thread of the workgroup hold something for the queues?  With the cache off: yes, no vote.  Otherwise one
        // barrier (__syncthreads_or takes three): a wave that has something sets word iter % 3, everybody reads it behind the
        // barrier; the word of the NEXT super-tile is cleared in front of that barrier -- its last readers (super-tile iter - 2)
        // have arrived at the barrier of iter - 1 by then.
        bool go = !use_cache && iter > 0;
        if (!go) {
          const int vw = iter % 3;
          if (threadIdx.x == 0) q_vote[vw == 2 ? 0 : vw + 1] = 0;
          if (__builtin_amdgcn_ballot_w64(any) != 0ull && psdf::lane_id() == 0) q_vote[vw] = 1;
          __syncthreads();
          go = q_vote[vw] != 0;
        }
        if (go) {
          // cache off (and drained): its LDS is the staging area of the coalesced hand-off
          if constexpr (F == 2 && NC * PSDF_BLOCK * 3 * 4 <= SCache::SC_SLOTS * (1 + F) * 4) {
            if (!use_cache && iter > 0)
              queue_push_staged<NC>(Q, level, q_cnt, q_base, q_off, q_gd, lds, crow, cval, grad_lattice + tbase);
            else
              queue_push<NC, F>(Q, level, q_cnt, q_base, crow, cval, grad_lattice + tbase);
          } else {
            queue_push<NC, F>(Q, level, q_cnt, q_base, crow, cval, grad_lattice + tbase);
          }
        }
      } else {
#pragma unroll
        for (int c = 0; c < NC; c++)
          if (crow[c] != Q_NONE) {
#pragma unroll
            for (int f = 0; f < F; f++) atomicAdd(grad_lattice + tbase + (int64_t)crow[c] * F + f, cval[c][f]);
          }
      }
    }
    if (LATTICE && iter == 0) {
      use_cache = cache_vote(sc, hits, tries);  // re-use rate of the first tile
      if (QUEUE && !use_cache) cache_drain_to_queue<F>(sc, Q, level, q_cnt, q_base, grad_lattice + tbase);
    }
  }
  // The way out of the cache.  Queue mode: through the queues (a cache that was switched off has been drained and its LDS
  // re-used; one that was kept is drained here, in one round).  Plain mode: one global float atomic per live value.
  if (LATTICE) {
    if (QUEUE) {
      if (use_cache) {
#if defined(PSDF_ENC_PROFILE)
        int* const drained = Q.tails + L * Q.np + 192 + level;
#else
        int* const drained = nullptr;
#endif
        cache_drain_once<F>(sc, Q, level, q_cnt, q_base, grad_lattice + tbase, drained);
      }
    } else {
      sc.flush(grad_lattice + tbase);
    }
  }
  plan_report();
  // How the workgroup left (psdf_encode_backward_cache_votes, a debug query): one word per level behind the queue counters,
  // zeroed with them -- low half: workgroups that kept their cache to the end, high half: those that voted it off.
  if (QUEUE && LATTICE && threadIdx.x == 0 && level < 64) atomicAdd(Q.tails + L * Q.np + 128 + level, use_cache ? 1 : 0x10000);
#if defined(PSDF_ENC_PROFILE)
  if (QUEUE && threadIdx.x == 0) {   // per-level duration of the workgroups (wall clock ticks), into the tail of the queue counters
    const long long dt = (long long)wall_clock64() - psdf_prof_t0;
    int* prof = Q.tails + L * Q.np;
    atomicMax(&prof[level], (int)dt);
    atomicAdd(&prof[64 + level], (int)(dt >> 6));
  }
#endif
}

// Position gradient ONLY (no lattice gradient: inference normals, sphere_trace.py; the reference gets them from
// autograd, models.py:236-251).  Same level-major launch shape as the forward, but a thread handles POS_LPB consecutive
// levels and sums their contributions in registers before it touches grad_positions: a quarter of the atomics of the
// general kernel (which also carries the scatter-cache / queue machinery of the lattice gradient) while the 4 tables
// of a group (8 MiB) still mostly live in the L2s.
// PARTIAL (round 4): the level groups do not meet in grad_positions with float atomics; each group stores its sum to its own
// [N, P] slab of a scratch buffer (plain coalesced stores) and encode_bwd_pos_reduce_kernel adds the slabs in group order.
// What it buys is DETERMINISM, not time: the position gradient (the normals of every training step, whose last bits the
// curvature term amplifies) no longer depends on the order in which atomics land.  Measured (profiles/r04_enc_ab.jsonl, 2 M
// points, 16 levels): 0.634 ms against 0.644 ms with atomics -- the 30 M atomics were NOT what makes this kernel 1.8x the
// forward (0.358 ms); 49 152 points x 24 levels: 30.8 against 28.8 us (one more launch).
// LPB = levels per thread: 2 for large batches, 8 for small ones (round 4, profiles/r04_enc_ab_pos_lpb.jsonl).  At 2 M points the
// kernel waits for gathers (70 % of its wave cycles) and the tables of 4 levels (8 MiB) do not fit an XCD's 4-MiB L2 (hit rate
// 48 %, profiles/r04_pmc_encode_bwd_pos.txt): 16 levels 0.623 ms with 4 levels per thread, **0.503 ms with 2** (two tables = one
// L2), 0.524 with 1 (nine more slabs to write and read), 0.749 with 8.  At a training step's 49 152 points x 24 levels nothing
// thrashes and fewer, longer threads win: 28.8 us with 8, 31.0 with 4, 32.9 with 2.
template <int P, int F, bool PARTIAL, int POS_LPB>
__global__ void __launch_bounds__(PSDF_BLOCK)
    encode_bwd_pos_kernel(int64_t N, int L, int Lt, uint32_t capacity, EncConv conv, const float* __restrict__ positions,
                          const float* __restrict__ lattice, const float* __restrict__ scale_factor,
                          const float* __restrict__ shifts, const float* __restrict__ window, float points_scaling,
                          int pad_points, const float* __restrict__ grad_sliced, const unsigned char* __restrict__ skip,
                          float* __restrict__ grad_positions) {
  const int64_t n = (int64_t)blockIdx.x * PSDF_BLOCK + threadIdx.x;
  if (n >= N) return;
  if (skip && skip[n]) return;     // masked sample: its gradient stays as it is
  float pos[P];
  load_pos<P>(positions, n, pos);
  float gp[P];
#pragma unroll
  for (int i = 0; i < P; i++) gp[i] = 0.f;
#pragma unroll
  for (int li = 0; li < POS_LPB; li++) {
    const int level = blockIdx.y * POS_LPB + li;
    if (level >= Lt) break;
    float g[F];
#pragma unroll
    for (int f = 0; f < F; f++)   // rows beyond L*F + P exist only in the padded layout
      g[f] = (level < L || (level - L) * F + f < P || pad_points) ? grad_sliced[((int64_t)level * F + f) * N + n] : 0.f;
    if (level >= L) {  // pseudo-levels: the concatenated, scaled point
      const int e = level - L;
#pragma unroll
      for (int f = 0; f < F; f++) {
        const int d = e * F + f;
#pragma unroll
        for (int i = 0; i < P; i++)
          if (i == d) gp[i] = gp[i] + g[f] * points_scaling;
      }
      continue;
    }
    float sfl[P], shl[P];
#pragma unroll
    for (int i = 0; i < P; i++) {
      sfl[i] = scale_factor[level * P + i];
      shl[i] = shifts[level * P + i];
    }
    const float w = window[level];
    if (w == 0.f) continue;   // closed level: contributes 0
    const int64_t tbase = (int64_t)level * capacity * F;
    Simplex<P> s;
    compute_simplex<P>(pos, shl, sfl, s, conv.tie_later);
    float dbary[P + 2];
#pragma unroll
    for (int k = 0; k <= P + 1; k++) dbary[k] = 0.f;
    uint32_t rows[P + 1];
    vertex_rows<P>(s, capacity, rows, conv.hash_c);
#pragma unroll
    for (int r = 0; r <= P; r++) {
      const uint32_t row = rows[r];
#pragma unroll
      for (int f = 0; f < F; f++) dbary[r] = dbary[r] + lattice[tbase + (int64_t)row * F + f] * w * g[f];
    }
    dbary[P + 1] = dbary[P + 1] + dbary[0];  // adjoint of bary[0] += 1 + bary[P+1]
    float dE[P + 1];
    const float invp = 1.0f / (P + 1);
#pragma unroll
    for (int i = 0; i <= P; i++) {
      float a = 0.f, b = 0.f;
#pragma unroll
      for (int k = 0; k <= P + 1; k++) {
        if (k == P - s.rank[i]) a = dbary[k];
        if (k == P + 1 - s.rank[i]) b = dbary[k];
      }
      dE[i] = (a - b) * invp;
    }
#pragma unroll
    for (int i = 0; i < P; i++) {
      float acc = 0.f;
#pragma unroll
      for (int j = 0; j <= i; j++) acc = acc + dE[j];
      acc = acc - dE[i + 1] * (float)(i + 1);
      gp[i] = gp[i] + acc * sfl[i];
    }
  }
  if (PARTIAL) {   // grad_positions = the scratch slabs [groups][N][P]
#pragma unroll
    for (int i = 0; i < P; i++) grad_positions[((int64_t)blockIdx.y * N + n) * P + i] = gp[i];
  } else {
#pragma unroll
    for (int i = 0; i < P; i++) atomicAdd(grad_positions + n * P + i, gp[i]);
  }
}

// grad_positions[n][i] += sum over the level groups of partial[g][n][i] (in group order: deterministic); one thread per float
__global__ void __launch_bounds__(PSDF_BLOCK)
    encode_bwd_pos_reduce_kernel(int64_t NP, int P, int groups, const float* __restrict__ partial,
                                 const unsigned char* __restrict__ skip, float* __restrict__ grad_positions) {
  const int64_t e = (int64_t)blockIdx.x * PSDF_BLOCK + threadIdx.x;
  if (e >= NP) return;
  if (skip && skip[e / P]) return;     // masked sample: its slabs were not written, its gradient stays as it is
  float s = partial[e];
  for (int g = 1; g < groups; g++) s = s + partial[(int64_t)g * NP + e];
  grad_positions[e] = grad_positions[e] + s;
}

// Four consecutive entries of one queue: what a thread of the reduce kernel loads per step.  Rows stay packed as they lie in
// the queue (two 16-bit rows per register) until they are added.
template <int F>
struct QueueGroup {
  uint32_t r01, r23;
  float v[4 * F];   // entry k, feature f at [k * F + f]: the order in memory
};

// One 8-byte load of the rows and F 16-byte loads of the values.  i0: the group's first entry, a multiple of 4 counted from
// the start of the workspace arrays.  Unconditional, so that the compiler can count the loads in flight (a load under a
// divergent branch makes it wait for ALL outstanding loads before the first use, the prefetched ones included).
template <int F>
__device__ __forceinline__ void queue_group_load(const uint16_t* __restrict__ rows, const float* __restrict__ vals, int i0,
                                                 QueueGroup<F>& G) {
  const uint2 r = *reinterpret_cast<const uint2*>(rows + i0);
  G.r01 = r.x;
  G.r23 = r.y;
  const float4* __restrict__ p = reinterpret_cast<const float4*>(vals + (int64_t)i0 * F);
#pragma unroll
  for (int k = 0; k < F; k++) {
    const float4 t = p[k];
    G.v[4 * k] = t.x;
    G.v[4 * k + 1] = t.y;
    G.v[4 * k + 2] = t.z;
    G.v[4 * k + 3] = t.w;
  }
}

// Adds a group to the LDS slice, entry after entry.  (All four reads, then all four compare-and-swaps, with same-row entries
// merged in registers first, was built and measured: no faster, 55 instead of 44 registers -- profiles/enc_bwd_reduce_ab.txt.)
template <int F>
__device__ __forceinline__ void queue_group_fold(float* tab, const QueueGroup<F>& G, int& hot) {
  const uint32_t r[4] = {G.r01 & 0xFFFFu, G.r01 >> 16, G.r23 & 0xFFFFu, G.r23 >> 16};
#pragma unroll
  for (int k = 0; k < 4; k++) {
#pragma unroll
    for (int f = 0; f < F; f += 2) lds_add_pair(&tab[r[k] * F + f], G.v[k * F + f], G.v[k * F + f + 1], hot);
  }
}

// One workgroup per (partition, level): fold the queue into an LDS image of the partition's table slice (64-bit
// compare-and-swap per feature pair, lds_add_pair), then add the slice to the gradient table (plain read-modify-write:
// this workgroup is the only writer of these rows after the binning kernel has finished).
template <int F>
__global__ void __launch_bounds__(1024)
    encode_bwd_reduce_kernel(uint32_t capacity, Queues Q, float* __restrict__ grad_lattice) {
  extern __shared__ __align__(16) float tab[];  // [rows per partition][F]
  const int part = blockIdx.x, level = blockIdx.y;
  int n = Q.tails[level * Q.np + part];
  if (n == 0) return;
  if (n > Q.cap) n = Q.cap;
  const int rpp = 1 << Q.shift;
  for (int i = threadIdx.x; i < rpp * F; i += blockDim.x) tab[i] = 0.f;
  __syncthreads();
  const int64_t qb = ((int64_t)level * Q.np + part) * Q.cap;
  const uint16_t* __restrict__ rows = Q.rows + qb;
  const float* __restrict__ vals = Q.vals + qb * F;
  const int tid = threadIdx.x, nt = blockDim.x;
  int hot = 0;
  // A thread takes four consecutive entries per step, in groups that are 4-entry aligned in the WORKSPACE (queue_plan aligns
  // the arrays to 256 bytes, but a queue's capacity need not be a multiple of 4, so its first entry need not be aligned):
  // entries [0, head) and [head + 4 nfull, n) are the ragged ends, at most three each, and take the scalar form.
  const bool wide = ((reinterpret_cast<uintptr_t>(Q.rows) & 7) | (reinterpret_cast<uintptr_t>(Q.vals) & 15)) == 0;
  const int lead = (int)((4 - (qb & 3)) & 3);
  const int head = wide ? (lead < n ? lead : n) : n;   // (a workspace that is not 16-byte aligned: everything in the scalar form)
  const int nfull = (n - head) >> 2;
  const int tail0 = head + 4 * nfull;
  for (int i = tid; i < head + (n - tail0); i += nt) {
    const int e = i < head ? i : tail0 + (i - head);
#pragma unroll
    for (int f = 0; f < F; f += 2) lds_add_pair(&tab[(int)rows[e] * F + f], vals[(int64_t)e * F + f], vals[(int64_t)e * F + f + 1], hot);
  }
  if (nfull > 0) {
    // Two groups per thread alternate: the loads of one are issued before the adds of the other.  A thread past the last
    // group loads the last group again and does not add it.
    // Every workgroup starts its walk at another place of its queue (and wraps round): the queues lie a fixed stride apart, and
    // workgroups that all read the same offset of their queues at the same time measured 4 % slower (the order of the
    // additions was never fixed: it depends on which compare-and-swap lands first).
    const int last = nfull - 1;
    const int rot = (int)((((uint32_t)(level * Q.np + part) * 2654435761u) >> 8) % (uint32_t)nfull);
    const auto at = [&](int g) {   // first entry of the g-th group of the walk
      int m = (g < last ? g : last) + rot;
      if (m >= nfull) m -= nfull;
      return head + 4 * m;
    };
    QueueGroup<F> A, B;
    queue_group_load<F>(rows, vals, at(tid), A);
    for (int base = 0; base < nfull; base += 2 * nt) {
      const int g = base + tid;
      queue_group_load<F>(rows, vals, at(g + nt), B);
      if (g < nfull) queue_group_fold<F>(tab, A, hot);
      queue_group_load<F>(rows, vals, at(g + 2 * nt), A);
      if (g + nt < nfull) queue_group_fold<F>(tab, B, hot);
    }
  }
  __syncthreads();
  const int64_t row0 = (int64_t)part << Q.shift;
  int64_t nrows = (int64_t)capacity - row0;
  if (nrows > rpp) nrows = rpp;
  float* __restrict__ out = grad_lattice + ((int64_t)level * capacity + row0) * F;
  // Eight floats per thread and step, their loads issued together (one at a time, the 16 steps of a 64-KiB slice were 16
  // dependent trips to memory at the end of every workgroup).  The loads are unconditional for the same reason as in
  // queue_group_load -- a step past the end reads the slice's last float -- and only sums that changed are stored.
  const int lim = (int)(nrows * F);
  constexpr int EU = 8;
  for (int i0 = tid; i0 < lim; i0 += EU * nt) {
    float t[EU], o[EU];
#pragma unroll
    for (int j = 0; j < EU; j++) {
      const int i = i0 + j * nt;
      t[j] = i < lim ? tab[i] : 0.f;
      o[j] = out[i < lim ? i : lim - 1];
    }
#pragma unroll
    for (int j = 0; j < EU; j++)
      if (t[j] != 0.f) out[i0 + j * nt] = o[j] + t[j];
  }
}

// ---------------------------------------------------------------------------------- double backward
// Inputs: u = dL/d(grad_positions) [N,P], g = grad_sliced [Lt*F,N].  grad_positions is bilinear in
// (g, lattice) for a fixed simplex, so
//   q_r = sum_i u_i * d bary_r / d pos_i        (directional derivative of the barycentrics along u)
//   grad_lattice[l][row_r][f] += q_r * w_l * g[l][f][n]
//   grad_g[l][f][n]            = sum_r q_r * w_l * lattice[l][row_r][f]
// and for the concatenated-point channels grad_g = u_d * points_scaling.
template <int P, int F, bool LATTICE>
__global__ void __launch_bounds__(PSDF_BLOCK)
    encode_dbl_bwd_kernel(int64_t N, int L, uint32_t capacity, EncConv conv, const float* __restrict__ positions,
                          const float* __restrict__ lattice, const float* __restrict__ scale_factor,
                          const float* __restrict__ shifts, const float* __restrict__ window, float points_scaling,
                          int pad_points, const float* __restrict__ dd_positions, const float* __restrict__ grad_sliced,
                          float* __restrict__ grad_lattice, float* __restrict__ grad_grad_sliced) {
  extern __shared__ __align__(16) float lds[];
  const int level = blockIdx.y;
  const int64_t ntiles = (N + PSDF_BLOCK - 1) / PSDF_BLOCK;
  if (level >= L) {
    const int e = level - L;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
      const int64_t n = tile * PSDF_BLOCK + threadIdx.x;
      if (n >= N) continue;
      float u[P];
      load_pos<P>(dd_positions, n, u);
#pragma unroll
      for (int f = 0; f < F; f++) {
        const int d = e * F + f;
        float v = 0.f;
#pragma unroll
        for (int i = 0; i < P; i++)
          if (i == d) v = u[i] * points_scaling;
        if (d < P || pad_points) grad_grad_sliced[((int64_t)level * F + f) * N + n] = v;
      }
    }
    return;
  }
  const float w = window[level];
  if (w == 0.f) {   // closed level: no lattice contribution, gradient w.r.t. the feature gradient 0
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
      const int64_t n = tile * PSDF_BLOCK + threadIdx.x;
      if (n >= N) continue;
#pragma unroll
      for (int f = 0; f < F; f++) grad_grad_sliced[((int64_t)level * F + f) * N + n] = 0.f;
    }
    return;
  }
  ScatterCache<F> sc;
  if (LATTICE) sc.init(lds);
  bool use_cache = LATTICE;
  int hot = 0;  // lds_add_pair: >0 while this thread's adds are contended (go straight to the float atomic)
  int hits = 0, tries = 0, iter = 0;
  const int64_t tbase = (int64_t)level * capacity * F;
  float sfl[P], shl[P];
#pragma unroll
  for (int i = 0; i < P; i++) {
    sfl[i] = scale_factor[level * P + i];
    shl[i] = shifts[level * P + i];
  }
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x, iter++) {
    const int64_t n = tile * PSDF_BLOCK + threadIdx.x;
    if (n < N) {
      float u[P], pos[P];
      load_pos<P>(dd_positions, n, u);
      load_pos<P>(positions, n, pos);
      Simplex<P> s;
      compute_simplex<P>(pos, shl, sfl, s, conv.tie_later);
      // adjoint of pos -> elevated
      float aE[P + 1];
#pragma unroll
      for (int j = 0; j <= P; j++) aE[j] = 0.f;
#pragma unroll
      for (int k = 0; k < P; k++) {
        const float us = u[k] * sfl[k];
#pragma unroll
        for (int j = 0; j <= k; j++) aE[j] = aE[j] + us;
        aE[k + 1] = aE[k + 1] - us * (float)(k + 1);
      }
      // adjoint of elevated -> barycentric slots
      float q[P + 2];
#pragma unroll
      for (int k = 0; k <= P + 1; k++) q[k] = 0.f;
      const float invp = 1.0f / (P + 1);
#pragma unroll
      for (int i = 0; i <= P; i++) {
        const float t = aE[i] * invp;
#pragma unroll
        for (int k = 0; k <= P + 1; k++) {
          if (k == P - s.rank[i]) q[k] = q[k] + t;
          if (k == P + 1 - s.rank[i]) q[k] = q[k] - t;
        }
      }
      q[0] = q[0] + q[P + 1];
      float g[F], gg[F];
#pragma unroll
      for (int f = 0; f < F; f++) {
        g[f] = grad_sliced[((int64_t)level * F + f) * N + n];
        gg[f] = 0.f;
      }
      uint32_t rows[P + 1];
      vertex_rows<P>(s, capacity, rows, conv.hash_c);
#pragma unroll
      for (int r = 0; r <= P; r++) {
        const uint32_t row = rows[r];
        const float qw = q[r] * w;
        if (LATTICE) {
          float v[F];
#pragma unroll
          for (int f = 0; f < F; f++) v[f] = qw * g[f];
          bool absorbed = false;
          if (use_cache) {
            const int rc = sc.add(row, v, hot);
            absorbed = rc != 0;
            hits += (rc == 2);
            tries++;
          }
          if (!absorbed) {
#pragma unroll
            for (int f = 0; f < F; f++) atomicAdd(grad_lattice + tbase + (int64_t)row * F + f, v[f]);
          }
        }
#pragma unroll
        for (int f = 0; f < F; f++) gg[f] = gg[f] + qw * lattice[tbase + (int64_t)row * F + f];
      }
#pragma unroll
      for (int f = 0; f < F; f++) grad_grad_sliced[((int64_t)level * F + f) * N + n] = gg[f];
    }
    if (LATTICE && iter == 0) use_cache = cache_vote(sc, hits, tries);  // re-use rate of the first tile
  }
  if (LATTICE) sc.flush(grad_lattice + tbase);
}

// `concat` = PSDF_ENC_CONCAT_* (encode_conventions.h): both concatenation layouts sweep ceil(P/F) pseudo-levels; the padded
// one also owns the channels L*F + d with d >= P (zeros), the appended one does not have them.
inline int extra_levels(int P, int F, int concat) { return concat ? (P + F - 1) / F : 0; }
inline int pad_points(int concat) { return concat == PSDF_ENC_CONCAT_PSEUDO_LEVELS; }
inline bool concat_ok(int concat) { return concat >= PSDF_ENC_CONCAT_NONE && concat <= PSDF_ENC_CONCAT_APPEND; }

}  // namespace

namespace psdf {
EncConv& enc_conv_state() {
  static EncConv c{(uint32_t)PSDF_ENC_HASH_MULTIPLIER, (uint32_t)PSDF_ENC_RANK_TIE_RAISES_LATER};
  return c;
}
}  // namespace psdf

// ================================================================================== host layer
// Ordinary C++ between the C ABI and the kernels: one list of the supported (P, F) pairs, one bundle of the arguments every
// kernel takes, one function template per launch.  The arithmetic that sizes the launches is in encode_plan.h.
namespace {
namespace plan = psdf::enc_plan;
using plan::env_int;
template <int V>
using int_c = std::integral_constant<int, V>;

// The supported (pos_dim, nr_feat) pairs: fn(int_c<P>, int_c<F>) for the one that matches.
template <class Fn>
int dispatch_pf(int pos_dim, int nr_feat, Fn&& fn) {
  if (pos_dim == 3 && nr_feat == 2) return fn(int_c<3>{}, int_c<2>{});
  if (pos_dim == 4 && nr_feat == 2) return fn(int_c<4>{}, int_c<2>{});
  if (pos_dim == 2 && nr_feat == 2) return fn(int_c<2>{}, int_c<2>{});
  if (pos_dim == 3 && nr_feat == 4) return fn(int_c<3>{}, int_c<4>{});
  return PSDF_ERR_UNSUPPORTED;
}

// What every entry point hands to every kernel.  Host only: the kernels keep their flat parameter lists; launch_enc (and the
// two launches of the position kernel, which take Lt as well) unpack it.
struct EncCall {
  int64_t N;
  int nr_levels, Lt, capacity;   // Lt = nr_levels + the pseudo-levels of the concatenated points
  const float *positions, *lattice, *scale_factor, *shifts, *window;
  float points_scaling;
  int pad;
  hipStream_t stream;
};

// The argument check every entry point shares (false: PSDF_ERR_ARG), and the bundle.
bool enc_call(EncCall& c, int pos_dim, int nr_feat, int64_t N, int nr_levels, int capacity, const float* positions,
              const float* lattice, const float* scale_factor, const float* shifts, const float* window, int concat_points,
              float points_scaling, void* stream) {
  if (N < 0 || nr_levels <= 0 || capacity <= 0 || !positions || !lattice || !concat_ok(concat_points)) return false;
  c = EncCall{N, nr_levels, nr_levels + extra_levels(pos_dim, nr_feat, concat_points), capacity, positions, lattice,
              scale_factor, shifts, window, points_scaling, pad_points(concat_points), (hipStream_t)stream};
  return true;
}

// kern<<<grid, PSDF_BLOCK, shm, stream>>>(N, L, capacity, conventions, positions .. points_scaling, rest...): the head of the
// parameter list of the forward, backward and double-backward kernels.  (A kernel's default arguments do not apply through a
// pointer: `rest` names every remaining parameter.)
template <class Kernel, class... Rest>
void launch_enc(Kernel kern, dim3 grid, size_t shm, const EncCall& c, Rest... rest) {
  hipLaunchKernelGGL(kern, grid, dim3(PSDF_BLOCK), shm, c.stream, c.N, c.nr_levels, (uint32_t)c.capacity, psdf::enc_conv_state(),
                     c.positions, c.lattice, c.scale_factor, c.shifts, c.window, c.points_scaling, rest...);
}

// what an entry point returns after its launches
int launched(int rc) {
  if (rc != PSDF_OK) return rc;
  PSDF_LAUNCH_CHECK();
  return PSDF_OK;
}

int device_cus() {
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

// Plain (cache + atomics) mode of the backward and the double backward: a workgroup sets up and flushes a 48-KiB LDS cache, so
// it should walk several tiles; PSDF_ENC_BWD_WG_PER_LEVEL overrides the per-level workgroup cap (measurement switch).
dim3 plain_grid(const EncCall& c) {
  static const int wg_cap_env = env_int("PSDF_ENC_BWD_WG_PER_LEVEL", 0);
  const unsigned wg_cap = wg_cap_env > 0 ? (unsigned)wg_cap_env : 512u, nb = psdf_blocks(c.N, PSDF_BLOCK);
  return dim3(nb < wg_cap ? nb : wg_cap, c.Lt);
}

// ---------------------------------------------------------------------------------- forward
// The paired form, process-wide: -1 the default rule (encode_plan.h: forward_pairs_default), 0 off (one level per grid row),
// n > 0 that many pairs.  PSDF_ENC_FWD_PAIRS is read once; psdf_encode_set_forward_pairs() replaces it (tests, A/B in one process).
int& fwd_pairs_setting() {
  static int v = env_int("PSDF_ENC_FWD_PAIRS", -1);
  return v;
}

template <int P, int F>
int launch_fwd(int_c<P>, int_c<F>, const EncCall& c, dim3 grid, const unsigned char* skip, float* sliced, unsigned char* touched,
               int touch_shift, const plan::FwdSlots& slots) {
  const int touch_blocks = (c.capacity + (1 << touch_shift) - 1) >> touch_shift;
  // (without a mask and a touched-block map the kernel needs fewer scalar registers: 8 instead of 7 waves per SIMD)
  const bool plain = !skip && !touched;
  if (slots.n > 0) {
    grid.y = (unsigned)slots.n;
    if (plain)
      launch_enc(encode_fwd_pair_kernel<P, F, true>, grid, 0, c, c.pad, skip, sliced, touched, touch_shift, touch_blocks, slots);
    else
      launch_enc(encode_fwd_pair_kernel<P, F, false>, grid, 0, c, c.pad, skip, sliced, touched, touch_shift, touch_blocks, slots);
  } else if (plain) {
    launch_enc(encode_fwd_kernel<P, F, true>, grid, 0, c, c.pad, skip, sliced, touched, touch_shift, touch_blocks);
  } else {
    launch_enc(encode_fwd_kernel<P, F, false>, grid, 0, c, c.pad, skip, sliced, touched, touch_shift, touch_blocks);
  }
  return PSDF_OK;
}

int encode_forward_impl(int pos_dim, int nr_feat, int64_t N, int nr_levels, int capacity, const float* positions,
                        const float* lattice, const float* scale_factor, const float* shifts, const float* window,
                        int concat_points, float points_scaling, const unsigned char* skip, float* sliced, void* stream,
                        unsigned char* touched = nullptr, int touch_shift = 0) {
  EncCall c;
  if (N == 0) return PSDF_OK;
  if (!enc_call(c, pos_dim, nr_feat, N, nr_levels, capacity, positions, lattice, scale_factor, shifts, window, concat_points,
                points_scaling, stream) || !sliced)
    return PSDF_ERR_ARG;
  if ((int64_t)capacity * nr_feat * 4 > 0xffffffffll) return PSDF_ERR_UNSUPPORTED;   // the kernel's 32-bit offsets inside a level
  dim3 grid(psdf_blocks(N, PSDF_BLOCK), c.Lt);
  // one resident round of workgroups per level (8 per CU) that walk the tiles, instead of one workgroup per tile: the level's
  // constants are fetched once per workgroup.  Round 5, 2 M points x 16 levels, forward bracket of the bench step: 0.650 ms
  // uncapped, 0.646 with 1024, 0.636 with 2048 or 4096 (profiles/r05_mlp_pair_ab.txt).  PSDF_ENC_FWD_WGS=0: one tile each.
  static const int fwd_env = env_int("PSDF_ENC_FWD_WGS", -1);
  const int fwd_wgs = fwd_env >= 0 ? fwd_env : device_cus() * 8;
  if (fwd_wgs > 0 && (int)grid.x > fwd_wgs) grid.x = fwd_wgs;
  // grid rows: one per level, or one per slot of the paired form (a level from the coarse end with one from the fine end)
  const int want = fwd_pairs_setting();
  const int pairs = want < 0 ? plan::forward_pairs_default(nr_levels, N) : want;
  // (the paired kernel counts its tiles in 32 bits: 2^40 points and more take the one-level form)
  const bool pairable = pairs > 0 && (N + PSDF_BLOCK - 1) / PSDF_BLOCK <= 0xffffffffll;
  const plan::FwdSlots slots = pairable ? plan::forward_slots(nr_levels, c.Lt, pairs) : plan::FwdSlots{};
  return launched(dispatch_pf(pos_dim, nr_feat, [&](auto p, auto f) {
    return launch_fwd(p, f, c, grid, skip, sliced, touched, touch_shift, slots);
  }));
}

// ---------------------------------------------------------------------------------- position gradient alone
// The level-group kernel + the slab reduction when stream-ordered scratch is available (not while a graph is being captured:
// there the float-atomic form runs), PSDF_ENC_POS_ATOMICS=1 forces the atomic form (A/B).
template <int P, int F, int POS_LPB>
void launch_bwd_pos_lpb(const EncCall& c, const float* grad_sliced, const unsigned char* skip, float* grad_positions, bool capturing,
                        float* caller_slabs = nullptr) {
  static const bool force_atomics = env_int("PSDF_ENC_POS_ATOMICS", 0) != 0;
  const int groups = (c.Lt + POS_LPB - 1) / POS_LPB;
  // The slabs are per-stream scratch that is never handed back: capped (PSDF_ENC_POS_SLAB_MAX_MB, default 256 MiB = 1.7 M points
  // at 24 + 2 levels) -- a multi-million-sample render pass takes the float-atomic form (same time, profiles/r04_enc_ab.jsonl:
  // what the slabs buy is run-to-run identical normals, which matters to the training step's curvature term at its 49 K samples)
  static const size_t slab_cap = (size_t)plan::env_long("PSDF_ENC_POS_SLAB_MAX_MB", 256) << 20;
  const size_t slab_bytes = (size_t)groups * c.N * P * sizeof(float);
  const bool use_slabs = groups > 1 && !force_atomics && !capturing && slab_bytes <= slab_cap;
  // caller_slabs: groups * N * P floats of the caller's (psdf_encode_backward_positions_masked_ws: the slab form whatever the
  // stream's capture state)
  float* slabs = caller_slabs ? (groups > 1 ? caller_slabs : nullptr) : use_slabs ? (float*)psdf::stream_scratch(slab_bytes, c.stream) : nullptr;
  const auto pos_kernel = [&](auto kern, float* out) {
    hipLaunchKernelGGL(kern, dim3(psdf_blocks(c.N, PSDF_BLOCK), groups), dim3(PSDF_BLOCK), 0, c.stream, c.N, c.nr_levels, c.Lt,
                       (uint32_t)c.capacity, psdf::enc_conv_state(), c.positions, c.lattice, c.scale_factor, c.shifts, c.window,
                       c.points_scaling, c.pad, grad_sliced, skip, out);
  };
  if (slabs) {
    pos_kernel(encode_bwd_pos_kernel<P, F, true, POS_LPB>, slabs);
    hipLaunchKernelGGL(encode_bwd_pos_reduce_kernel, dim3(psdf_blocks(c.N * P, PSDF_BLOCK)), dim3(PSDF_BLOCK), 0, c.stream,
                       c.N * P, P, groups, slabs, skip, grad_positions);
  } else {
    pos_kernel(encode_bwd_pos_kernel<P, F, false, POS_LPB>, grad_positions);
  }
}

template <int P, int F>
int launch_bwd_pos(int_c<P>, int_c<F>, const EncCall& c, const float* grad_sliced, const unsigned char* skip, float* grad_positions) {
  // (the capture state is probed once per launch: while a graph is being captured -- the sphere tracer's -- there is no
  // stream-ordered scratch and the float-atomic form runs, as measured in round 2)
  const bool capturing = psdf::stream_scratch(16, c.stream) == nullptr;
  if (capturing)
    launch_bwd_pos_lpb<P, F, 4>(c, grad_sliced, skip, grad_positions, true);
  else if (c.N >= ((int64_t)1 << 17))
    launch_bwd_pos_lpb<P, F, 2>(c, grad_sliced, skip, grad_positions, false);
  else
    launch_bwd_pos_lpb<P, F, 8>(c, grad_sliced, skip, grad_positions, false);
  return PSDF_OK;
}

// ---------------------------------------------------------------------------------- binned lattice gradient
// The plan (bytes == 0: the path does not apply) and the queues it lays out in the caller's workspace.
plan::QueuePlan queue_plan(int pos_dim, int nr_feat, int64_t N, int nr_levels, int capacity) {
  static const int64_t min_n = plan::env_long("PSDF_ENC_QUEUE_MIN_N", (int64_t)1 << 13);
  static const int delta = env_int("PSDF_ENC_QUEUE_SLICE_LOG2_DELTA", 1);   // A/B switch
  return plan::queue_plan(pos_dim, nr_feat, N, nr_levels, capacity, min_n, delta);
}
Queues queue_carve(void* ws, const plan::QueuePlan& p) {
  char* b = (char*)ws;
  return Queues{(uint16_t*)b, (float*)(b + p.rows_bytes), (int*)(b + p.rows_bytes + p.vals_bytes), p.cap, p.np, p.shift};
}
// false: the plain path runs.  Otherwise Q is carved and its counters are zeroed on the stream, together with the 1024 bytes of
// slots behind them (the plan always holds them: per-level cache votes, and the profile build's durations and drain counts).
bool queue_begin(int pos_dim, int nr_feat, const EncCall& c, bool wanted, void* ws, int64_t ws_bytes, Queues& Q, hipError_t& e) {
  const plan::QueuePlan p = (wanted && ws) ? queue_plan(pos_dim, nr_feat, c.N, c.nr_levels, c.capacity) : plan::QueuePlan{};
  if (p.bytes == 0 || ws_bytes < p.bytes) return false;
  Q = queue_carve(ws, p);
  e = hipMemsetAsync(Q.tails, 0, (size_t)c.nr_levels * Q.np * sizeof(int) + plan::Q_SLOT_BYTES, c.stream);
  return true;
}

// The deal of one resident round of binning workgroups over the levels (see LevelPlan; the arithmetic is plan::redeal).  State
// of the previous call per process: the deal it launched with and the host-mapped array its workgroups report their durations
// into (two arrays, used alternately, entries tagged with the call's generation: a call never reads what an older or an
// unfinished launch wrote as if it were the previous one's).  PSDF_ENC_BWD_BALANCE=0: equal shares.
struct EncBalance {
  int levels = 0, total = 0, kind = 0, bucket = -1;
  const void* ident = nullptr;   // the lattice the launches belong to (encodings of one shape have different cost profiles)
  uint32_t gen = 0;
  uint64_t last_use = 0;
  std::vector<int> counts;
  uint32_t* times[2] = {nullptr, nullptr};
  int device = -1;
};
constexpr int BAL_STATES = 16;
std::mutex g_shares_mu;
std::vector<int> g_last_shares;

// returns false when the plan cannot be used (equal shares through the rectangular grid then).  kind: 0 backward, 1 double
// backward.  One state per (lattice, kind, levels, size class of N: quarter octaves, round size) -- a training step alternates between
// several shapes and its sample count moves a little from step to step --, at most BAL_STATES of them (least recently used
// one is re-used).
bool encode_balance(int nr_levels, int64_t N, int total, int64_t super_tiles, LevelPlan& lp, const void* ident, int kind) {
  static const bool off = env_int("PSDF_ENC_BWD_BALANCE", 1) == 0;
  static std::mutex mu;
  static EncBalance states[BAL_STATES];
  static uint64_t tick = 0;
  if (!plan::deal_eligible(off, nr_levels, total, N)) return false;
  std::lock_guard<std::mutex> lock(mu);
  const int bucket = plan::size_bucket(N);
  // (the key holds the device as well: an address re-used on another GPU -- or after a free -- must not inherit a deal measured
  //  elsewhere)
  int device = -1;
  (void)hipGetDevice(&device);
  EncBalance* Bp = nullptr;
  for (auto& st_ : states)
    if (st_.times[0] && st_.ident == ident && st_.device == device && st_.kind == kind && st_.levels == nr_levels && st_.bucket == bucket &&
        st_.total == total)
      Bp = &st_;
  if (!Bp) {
    for (auto& st_ : states)
      if (!Bp || st_.last_use < Bp->last_use) Bp = &st_;
    if (!Bp->times[0]) {
      for (int i = 0; i < 2; i++) {
        void* h = nullptr;
        if (hipHostMalloc(&h, plan::BAL_MAX_WG * sizeof(uint32_t), hipHostMallocMapped) != hipSuccess || !h) {
          (void)hipGetLastError();
          if (i == 1) (void)hipHostFree(Bp->times[0]);
          Bp->times[0] = Bp->times[1] = nullptr;
          return false;
        }
        Bp->times[i] = (uint32_t*)h;
      }
    }
    memset(Bp->times[0], 0, plan::BAL_MAX_WG * sizeof(uint32_t));     // (a launch of the state's previous owner may still write: its
    memset(Bp->times[1], 0, plan::BAL_MAX_WG * sizeof(uint32_t));     // entries carry an older generation tag and are ignored)
    Bp->levels = 0;
  }
  EncBalance& B = *Bp;
  B.last_use = ++tick;
  if (!B.times[0] || !B.times[1]) return false;
  const int cap = (int)(super_tiles < total ? super_tiles : total);       // more workgroups than super-tiles of a level: idle ones
  if (B.levels != nr_levels || (int)B.counts.size() != nr_levels) {
    B.levels = nr_levels;
    B.kind = kind;
    B.ident = ident;
    B.device = device;
    B.bucket = bucket;
    B.total = total;
    B.counts = plan::first_deal(nr_levels, total);
  } else {
    plan::redeal_from_times(B.counts, B.times[B.gen & 1], B.gen, total, cap);
  }
  B.gen++;
  lp.n = nr_levels;
  lp.gen = B.gen;
  lp.times = B.times[B.gen & 1];
  const int at = plan::deal_layout(B.counts, cap, lp.first);
  std::lock_guard<std::mutex> l2(g_shares_mu);
  g_last_shares = B.counts;
  return at <= plan::BAL_MAX_WG;
}

// One resident round of binning workgroups: every workgroup of the launch resident at once and none left over.  The binning
// kernel is a long walk per workgroup (LDS cache warm-up, then tens of super-tiles), so a second, partly filled round of
// workgroups is a tail the size of a whole walk: measured on the bench batch (2 M points; 3 workgroups fit a CU, 768 in all)
// 16 levels x 48 = 768 workgroups 0.96 ms, x 40 1.09, x 56 1.26 (just over one round), x 96 (two rounds) 1.03, x 128 1.10;
// 24 levels x 32 best.  (Those figures are from the 3-workgroups-per-CU state of the kernel; 5 fit now -- 80 per level at 16
// levels -- by the same rule.)
// Returns the workgroups per level of the rectangular grid (the round shared among c.nr_levels).  deal_levels > 0: the round
// is dealt over that many levels by their measured cost instead where encode_balance has a deal -- then deal.n = deal_levels
// and the grid is one-dimensional, deal.first[deal.n] workgroups.  A failed occupancy query: 128 per level, no deal.
template <class Kernel>
unsigned resident_round(Kernel kern, size_t shm, const EncCall& c, int deal_levels, int kind, LevelPlan& deal) {
  int per_cu = 0;
  const bool known = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, PSDF_BLOCK, shm) == hipSuccess && per_cu > 0;
  if (!known) (void)hipGetLastError();
  const int resident = known ? per_cu * device_cus() : 0;
  const int64_t tiles = plan::super_tiles(c.N, PSDF_BLOCK * QUEUE_SPT);
  deal = LevelPlan{};
  if (known && deal_levels > 0 && !encode_balance(deal_levels, c.N, resident, tiles, deal, c.lattice, kind)) deal = LevelPlan{};
  return plan::round_share(resident, c.nr_levels, tiles);
}

template <int F>
constexpr size_t binning_shm() { return ScatterCache<F, 4096>::bytes() + Q_LDS_INTS * sizeof(int); }

// The lattice-only binning kernel of the backward (DBL = false: grad_sliced alone) and of the double backward (with
// dd_positions, grad_grad_sliced and the optional second upstream gradient) over `levels` levels, which are the levels of the
// deal too (the double backward's include the concatenated-point channels; a training step's coarse-to-fine window leaves
// levels closed, whose workgroups return at once).  Returns the rectangular share per level (the profile build prints it).
template <int P, int F, bool DBL>
unsigned launch_binning(const EncCall& c, int levels, const float* grad_sliced, float* grad_lattice, const Queues& Q,
                        const float* dd_positions, float* grad_grad_sliced, const float* grad_sliced2) {
  const auto kern = encode_bwd_kernel<P, F, true, false, true, DBL>;
  LevelPlan deal;
  const unsigned gx = resident_round(kern, binning_shm<F>(), c, levels, DBL ? 1 : 0, deal);
  launch_enc(kern, deal.n ? dim3(deal.first[deal.n]) : dim3(gx, levels), binning_shm<F>(), c, grad_sliced, grad_lattice,
             (float*)nullptr, Q, dd_positions, grad_grad_sliced, DBL ? c.pad : 0, grad_sliced2, deal);
  return gx;
}

// folds every queue into LDS and adds the slices to the gradient
template <int F>
int launch_queue_reduce(const EncCall& c, const Queues& Q, float* grad_lattice) {
  const size_t lds_b = (size_t)(1 << Q.shift) * F * sizeof(float);
  const hipError_t e =
      hipFuncSetAttribute((const void*)encode_bwd_reduce_kernel<F>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_b);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL((encode_bwd_reduce_kernel<F>), dim3(Q.np, c.nr_levels), dim3(1024), lds_b, c.stream, (uint32_t)c.capacity, Q,
                     grad_lattice);
  return PSDF_OK;
}

#if defined(PSDF_ENC_PROFILE)
void enc_profile_report(const EncCall& c, int pos_dim, const Queues& Q, unsigned gx) {
  static int calls = 0;
  if (++calls != 8) return;
  (void)hipStreamSynchronize(c.stream);
  int prof[256];   // [0, 64) longest workgroup, [64, 128) sum of durations / 64, [128, 192) caches kept, [192, 256) entries drained
  (void)hipMemcpy(prof, Q.tails + c.nr_levels * Q.np, sizeof(prof), hipMemcpyDeviceToHost);
  std::vector<int> tails((size_t)c.nr_levels * Q.np);
  (void)hipMemcpy(tails.data(), Q.tails, tails.size() * sizeof(int), hipMemcpyDeviceToHost);
  for (int l = 0; l < c.nr_levels; l++) {
    // the tails count every entry of the level's queues: the contributions pushed during the walk and, apart from them, the
    // cache entries (partial sums of many contributions each) that the workgroups which kept their cache drained at the end
    long long entries = 0;
    for (int q = 0; q < Q.np; q++) entries += tails[(size_t)l * Q.np + q];
    const long long queued = entries - prof[192 + l];
    fprintf(stderr, "[enc-profile] level %2d: max %8d ticks, mean %8.0f ticks, cache kept by %d of %u workgroups, queued %lld of %lld "
            "contributions (%.1f %%), drained %d cache entries\n", l, prof[l], 64.0 * prof[64 + l] / gx, prof[128 + l] & 0xffff, gx, queued,
            (long long)c.N * (pos_dim + 1), 100.0 * queued / ((double)c.N * (pos_dim + 1)), prof[192 + l]);
  }
}
#endif

// ---------------------------------------------------------------------------------- backward
bool pos_fused() {   // A/B: the round-3 form, the position gradient from inside the binning kernel
  static const bool on = env_int("PSDF_ENC_POS_FUSED", 0) != 0;
  return on;
}

// Q: the carved queues when the binned path applies, NULL for the plain (cache + atomics) path.
template <int P, int F>
int launch_bwd(int_c<P> p, int_c<F> f, const EncCall& c, const float* grad_sliced, float* grad_lattice, float* grad_positions,
               const Queues* Q) {
  const float* const no_in = nullptr;
  float* const no_out = nullptr;
  constexpr size_t plain_shm = ScatterCache<F, 8192>::bytes() + Q_LDS_INTS * sizeof(int);
  if (!grad_lattice) return launch_bwd_pos(p, f, c, grad_sliced, nullptr, grad_positions);
  if (!Q) {
    if (grad_positions)
      launch_enc(encode_bwd_kernel<P, F, true, true, false>, plain_grid(c), plain_shm, c, grad_sliced, grad_lattice, grad_positions,
                 Queues{}, no_in, no_out, 0, no_in, LevelPlan{});
    else
      launch_enc(encode_bwd_kernel<P, F, true, false, false>, plain_grid(c), plain_shm, c, grad_sliced, grad_lattice, grad_positions,
                 Queues{}, no_in, no_out, 0, no_in, LevelPlan{});
    return PSDF_OK;
  }
  [[maybe_unused]] unsigned gx;
  if (grad_positions && pos_fused()) {
    const auto kern = encode_bwd_kernel<P, F, true, true, true>;
    LevelPlan none;
    gx = resident_round(kern, binning_shm<F>(), c, 0, 0, none);
    launch_enc(kern, dim3(gx, c.Lt), binning_shm<F>(), c, grad_sliced, grad_lattice, grad_positions, *Q, no_in, no_out, 0, no_in, none);
  } else {
    // large batch, both gradients: the binning kernel for the lattice (its own levels only) and the level-group kernel for the
    // positions -- the fused form adds the position gradient with float atomics from inside the binning kernel: +0.98 ms at
    // 2 M points x 16 levels against 0.63 ms for the separate kernel (round 4)
    gx = launch_binning<P, F, false>(c, c.nr_levels, grad_sliced, grad_lattice, *Q, no_in, no_out, no_in);
    if (grad_positions) launch_bwd_pos(p, f, c, grad_sliced, nullptr, grad_positions);
  }
  const int rc = launch_queue_reduce<F>(c, *Q, grad_lattice);
#if defined(PSDF_ENC_PROFILE)
  if (rc == PSDF_OK) enc_profile_report(c, P, *Q, gx);
#endif
  return rc;
}

// ---------------------------------------------------------------------------------- double backward
template <int P, int F>
int launch_dbl_queue(int_c<P>, int_c<F>, const EncCall& c, const float* dd_positions, const float* grad_sliced, float* grad_lattice,
                     float* grad_grad_sliced, const float* grad_sliced_direct, const Queues& Q) {
  launch_binning<P, F, true>(c, c.Lt, grad_sliced, grad_lattice, Q, dd_positions, grad_grad_sliced, grad_sliced_direct);
  return launch_queue_reduce<F>(c, Q, grad_lattice);
}

template <int P, int F>
int launch_dbl_plain(int_c<P>, int_c<F>, const EncCall& c, const float* dd_positions, const float* grad_sliced, float* grad_lattice,
                     float* grad_grad_sliced) {
  if (grad_lattice)
    launch_enc(encode_dbl_bwd_kernel<P, F, true>, plain_grid(c), ScatterCache<F>::bytes(), c, c.pad, dd_positions, grad_sliced,
               grad_lattice, grad_grad_sliced);
  else
    launch_enc(encode_dbl_bwd_kernel<P, F, false>, plain_grid(c), 0, c, c.pad, dd_positions, grad_sliced, grad_lattice,
               grad_grad_sliced);
  return PSDF_OK;
}

}  // namespace

// ================================================================================== C ABI
extern "C" {

// The conventions in force, by index: 0 hash multiplier, 1 rank tie rule (both RUNTIME values: the defaults of
// encode_conventions.h until psdf_encode_set_conventions() replaces them), 2 sqrt term in scale_factor, 3 inverse-std-dev
// term, 4 default concatenation layout (host-side conventions: scale_factor and the layout are ARGUMENTS of every entry point,
// the values here are the defaults the Python mirror and the oracle read).  Host only (no device needed).
int64_t psdf_encode_convention(int which) {
  switch (which) {
    case 0: return (int64_t)psdf::enc_conv_state().hash_c;
    case 1: return (int64_t)psdf::enc_conv_state().tie_later;
    case 2: return PSDF_ENC_SCALE_SQRT_TERM;
    case 3: return PSDF_ENC_SCALE_INV_STDDEV;
    case 4: return PSDF_ENC_CONCAT_DEFAULT_LAYOUT;
    default: return -1;
  }
}

// Replace the two device-side conventions for this process (every later launch uses them): hash multiplier (any odd or even
// 32-bit value; 0 is rejected) and the rank tie rule (0 / 1).  Not thread-safe against concurrent launches.
int psdf_encode_set_conventions(uint32_t hash_multiplier, int rank_tie_raises_later) {
  if (hash_multiplier == 0u || (rank_tie_raises_later != 0 && rank_tie_raises_later != 1)) return PSDF_ERR_ARG;
  psdf::enc_conv_state() = EncConv{hash_multiplier, (uint32_t)rank_tie_raises_later};
  return PSDF_OK;
}

// The paired form of the forward for this process (every later launch): -1 the default rule, 0 off (one level per grid row), n > 0
// that many coarse-with-fine pairs (clamped to nr_levels / 2 per call).  Results do not depend on it.  Not thread-safe against
// concurrent launches.
int psdf_encode_set_forward_pairs(int pairs) {
  if (pairs < -1) return PSDF_ERR_ARG;
  fwd_pairs_setting() = pairs;
  return PSDF_OK;
}

int psdf_encode_forward(int pos_dim, int nr_feat, int64_t N, int nr_levels, int capacity, const float* positions,
                        const float* lattice, const float* scale_factor, const float* shifts, const float* window,
                        int concat_points, float points_scaling, float* sliced, void* stream) {
  return encode_forward_impl(pos_dim, nr_feat, N, nr_levels, capacity, positions, lattice, scale_factor, shifts, window,
                             concat_points, points_scaling, nullptr, sliced, stream);
}

// Same with a per-point mask: points with skip[n] != 0 are not evaluated and their columns of `sliced` are left as
// they are (fixed-shape callers that keep one slot per ray, e.g. the sphere tracer's converged rays).
int psdf_encode_forward_masked(int pos_dim, int nr_feat, int64_t N, int nr_levels, int capacity, const float* positions,
                               const float* lattice, const float* scale_factor, const float* shifts, const float* window,
                               int concat_points, float points_scaling, const unsigned char* skip, float* sliced,
                               void* stream) {
  return encode_forward_impl(pos_dim, nr_feat, N, nr_levels, capacity, positions, lattice, scale_factor, shifts, window,
                             concat_points, points_scaling, skip, sliced, stream);
}

// Forward that also records the blocks of 2^block_rows_log2 table rows it reads: touched_blocks [nr_levels, ceil(capacity /
// 2^block_rows_log2)] bytes, set to 1 (never cleared here).  See psdf_adamw_step_blocks.
int psdf_encode_forward_mark(int pos_dim, int nr_feat, int64_t N, int nr_levels, int capacity, const float* positions,
                             const float* lattice, const float* scale_factor, const float* shifts, const float* window,
                             int concat_points, float points_scaling, float* sliced, unsigned char* touched_blocks,
                             int block_rows_log2, void* stream) {
  if (!touched_blocks || block_rows_log2 < 0 || block_rows_log2 > 20) return PSDF_ERR_ARG;
  return encode_forward_impl(pos_dim, nr_feat, N, nr_levels, capacity, positions, lattice, scale_factor, shifts, window,
                             concat_points, points_scaling, nullptr, sliced, stream, touched_blocks, block_rows_log2);
}

// Workspace for the binned (queue + LDS reduction) lattice-gradient path; 0 = the path does not apply (small batch,
// table too large for 64 partitions) and psdf_encode_backward_ws behaves exactly like psdf_encode_backward.  Host only.
int64_t psdf_encode_backward_workspace_bytes(int pos_dim, int nr_feat, int64_t N, int nr_levels, int capacity) {
  return queue_plan(pos_dim, nr_feat, N, nr_levels, capacity).bytes;
}

// the deal of the last balanced launch (debug query): counts[0 .. nr_levels), returns nr_levels (0: none yet)
int psdf_encode_backward_level_shares(int* counts, int max_levels) {
  std::lock_guard<std::mutex> lock(g_shares_mu);
  const int n = (int)g_last_shares.size();
  for (int l = 0; l < n && l < max_levels; l++) counts[l] = g_last_shares[l];
  return n;
}

// How the binning workgroups of the last queue-path call that used `workspace` left their scatter caches (debug query; the
// arguments are those of that call): kept[l] workgroups of level l kept the cache to the end of their walk and drained it into
// the queues in one round, voted_off[l] switched it off after their first super-tile.  Waits for `stream`.  Returns the number of
// levels written (at most 64 and max_levels), 0 when the queue plan does not apply to these arguments.
int psdf_encode_backward_cache_votes(int pos_dim, int nr_feat, int64_t N, int nr_levels, int capacity, const void* workspace,
                                     int64_t workspace_bytes, int* kept, int* voted_off, int max_levels, void* stream) {
  const plan::QueuePlan p = queue_plan(pos_dim, nr_feat, N, nr_levels, capacity);
  if (!workspace || !kept || !voted_off || p.bytes == 0 || workspace_bytes < p.bytes) return 0;
  int words[64];
  const int n = nr_levels < 64 ? (nr_levels < max_levels ? nr_levels : max_levels) : (max_levels < 64 ? max_levels : 64);
  if (n <= 0) return 0;
  const Queues Q = queue_carve(const_cast<void*>(workspace), p);
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return 0;
  if (hipMemcpy(words, Q.tails + (size_t)nr_levels * Q.np + 128, (size_t)n * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return 0;
  for (int l = 0; l < n; l++) {
    kept[l] = words[l] & 0xffff;
    voted_off[l] = (int)((uint32_t)words[l] >> 16);
  }
  return n;
}

// grad_lattice / grad_positions must be zero-initialised by the caller (or hold a running sum to add to);
// either may be NULL to skip that gradient.  workspace: device scratch of at least
// psdf_encode_backward_workspace_bytes() bytes (contents undefined on entry and exit) or NULL.
int psdf_encode_backward_ws(int pos_dim, int nr_feat, int64_t N, int nr_levels, int capacity, const float* positions,
                            const float* lattice, const float* scale_factor, const float* shifts, const float* window,
                            int concat_points, float points_scaling, const float* grad_sliced, float* grad_lattice,
                            float* grad_positions, void* workspace, int64_t workspace_bytes, void* stream) {
  EncCall c;
  if (N == 0 || (!grad_lattice && !grad_positions)) return PSDF_OK;
  if (!enc_call(c, pos_dim, nr_feat, N, nr_levels, capacity, positions, lattice, scale_factor, shifts, window, concat_points,
                points_scaling, stream) || !grad_sliced)
    return PSDF_ERR_ARG;
  if (!grad_positions) c.Lt = nr_levels;   // the pseudo-levels of the concatenated points carry a position gradient only
  Queues Q{};
  hipError_t e = hipSuccess;
  const bool use_queue = queue_begin(pos_dim, nr_feat, c, grad_lattice, workspace, workspace_bytes, Q, e);
  if (e != hipSuccess) return (int)e;
  const int rc = dispatch_pf(pos_dim, nr_feat, [&](auto p, auto f) {
    return launch_bwd(p, f, c, grad_sliced, grad_lattice, grad_positions, use_queue ? &Q : nullptr);
  });
  if (rc == PSDF_OK) psdf::g_last_path[psdf::PATH_ENCODE_BWD] = use_queue ? 2 : (grad_lattice ? 1 : 3);
  return launched(rc);
}

int psdf_encode_backward(int pos_dim, int nr_feat, int64_t N, int nr_levels, int capacity, const float* positions,
                         const float* lattice, const float* scale_factor, const float* shifts, const float* window,
                         int concat_points, float points_scaling, const float* grad_sliced, float* grad_lattice,
                         float* grad_positions, void* stream) {
  return psdf_encode_backward_ws(pos_dim, nr_feat, N, nr_levels, capacity, positions, lattice, scale_factor, shifts,
                                 window, concat_points, points_scaling, grad_sliced, grad_lattice, grad_positions,
                                 nullptr, 0, stream);
}

// Position gradient only, with a per-sample mask (masked samples: no gathers, their rows of grad_positions keep their
// contents).  grad_positions is ACCUMULATED INTO, as in psdf_encode_backward.
int psdf_encode_backward_positions_masked(int pos_dim, int nr_feat, int64_t N, int nr_levels, int capacity,
                                          const float* positions, const float* lattice, const float* scale_factor,
                                          const float* shifts, const float* window, int concat_points, float points_scaling,
                                          const float* grad_sliced, const unsigned char* skip, float* grad_positions,
                                          void* stream) {
  EncCall c;
  if (N == 0) return PSDF_OK;
  if (!enc_call(c, pos_dim, nr_feat, N, nr_levels, capacity, positions, lattice, scale_factor, shifts, window, concat_points,
                points_scaling, stream) || !grad_sliced || !grad_positions)
    return PSDF_ERR_ARG;
  return launched(dispatch_pf(pos_dim, nr_feat, [&](auto p, auto f) {
    return launch_bwd_pos(p, f, c, grad_sliced, skip, grad_positions);
  }));
}

// The same with the caller's scratch for the level groups' slabs: the groups never meet in float atomics, so the same inputs
// give the same bits on every call, ALSO while the stream is being captured into a graph (where the entry above has no scratch
// and takes the atomic form) -- what a caller needs whose captured and eager results must agree bit for bit (box_trace.py).
// The levels per thread are those of the entry above outside a capture (8 below 2^17 samples, else 2), hence so are the bits.
// workspace_bytes below psdf_encode_backward_positions_workspace_bytes(): -1.
constexpr int64_t POS_WS_LARGE_N = (int64_t)1 << 17;

int64_t psdf_encode_backward_positions_workspace_bytes(int pos_dim, int nr_feat, int64_t N, int nr_levels, int concat_points) {
  if (N <= 0 || nr_levels <= 0 || pos_dim <= 0 || nr_feat <= 0 || !concat_ok(concat_points)) return 0;
  const int Lt = nr_levels + extra_levels(pos_dim, nr_feat, concat_points), lpb = N >= POS_WS_LARGE_N ? 2 : 8;
  const int groups = (Lt + lpb - 1) / lpb;
  return groups > 1 ? (int64_t)groups * N * pos_dim * (int64_t)sizeof(float) : 0;
}

int psdf_encode_backward_positions_masked_ws(int pos_dim, int nr_feat, int64_t N, int nr_levels, int capacity,
                                             const float* positions, const float* lattice, const float* scale_factor,
                                             const float* shifts, const float* window, int concat_points, float points_scaling,
                                             const float* grad_sliced, const unsigned char* skip, float* grad_positions,
                                             void* workspace, int64_t workspace_bytes, void* stream) {
  EncCall c;
  if (N == 0) return PSDF_OK;
  if (!enc_call(c, pos_dim, nr_feat, N, nr_levels, capacity, positions, lattice, scale_factor, shifts, window, concat_points,
                points_scaling, stream) || !grad_sliced || !grad_positions)
    return PSDF_ERR_ARG;
  const int64_t need = psdf_encode_backward_positions_workspace_bytes(pos_dim, nr_feat, N, nr_levels, concat_points);
  if (need > 0 && (!workspace || workspace_bytes < need)) return PSDF_ERR_ARG;
  return launched(dispatch_pf(pos_dim, nr_feat, [&](auto p, auto f) {
    constexpr int P = decltype(p)::value, F = decltype(f)::value;
    // (one group: a single thread adds to each entry, nothing to order, and no slab is used)
    float* slabs = need > 0 ? (float*)workspace : nullptr;
    if (N >= POS_WS_LARGE_N)
      launch_bwd_pos_lpb<P, F, 2>(c, grad_sliced, skip, grad_positions, slabs == nullptr, slabs);
    else
      launch_bwd_pos_lpb<P, F, 8>(c, grad_sliced, skip, grad_positions, slabs == nullptr, slabs);
    return PSDF_OK;
  }));
}

// grad_lattice must be zero-initialised (or NULL to skip); grad_grad_sliced is fully overwritten.  workspace: device scratch of
// psdf_encode_backward_workspace_bytes() bytes or NULL -- with it, batches large enough for the queue plan send the lattice
// scatter through the binning + reduce kernels of the backward (encode_bwd_kernel<.., DBL = true>) instead of float atomics:
// measured at 49 152 ray samples, 24 levels (a training step) 269 -> ~75 us, at 262 080 samples 1.36 ms -> ~0.2 ms.
int psdf_encode_double_backward_ws(int pos_dim, int nr_feat, int64_t N, int nr_levels, int capacity,
                                   const float* positions, const float* lattice, const float* scale_factor,
                                   const float* shifts, const float* window, int concat_points, float points_scaling,
                                   const float* dd_positions, const float* grad_sliced, float* grad_lattice,
                                   float* grad_grad_sliced, const float* grad_sliced_direct, void* workspace,
                                   int64_t workspace_bytes, void* stream) {
  EncCall c;
  if (N == 0) return PSDF_OK;
  if (!enc_call(c, pos_dim, nr_feat, N, nr_levels, capacity, positions, lattice, scale_factor, shifts, window, concat_points,
                points_scaling, stream) || !dd_positions || !grad_sliced || (!grad_grad_sliced && !grad_lattice) ||
      (grad_sliced_direct && !grad_lattice))
    return PSDF_ERR_ARG;
  Queues Q{};
  hipError_t e = hipSuccess;
  if (queue_begin(pos_dim, nr_feat, c, grad_lattice, workspace, workspace_bytes, Q, e)) {
    if (e != hipSuccess) return (int)e;
    return launched(dispatch_pf(pos_dim, nr_feat, [&](auto p, auto f) {
      return launch_dbl_queue(p, f, c, dd_positions, grad_sliced, grad_lattice, grad_grad_sliced, grad_sliced_direct, Q);
    }));
  }
  // small batches: the plain double-backward kernel (it always writes the gathered output: give it scratch when the caller
  // wants the lattice gradient only), and the direct part as an ordinary backward
  if (grad_sliced_direct) {
    const int rc = psdf_encode_backward_ws(pos_dim, nr_feat, N, nr_levels, capacity, positions, lattice, scale_factor, shifts,
                                           window, concat_points, points_scaling, grad_sliced_direct, grad_lattice, nullptr,
                                           nullptr, 0, stream);
    if (rc != PSDF_OK) return rc;
  }
  if (!grad_grad_sliced) {
    grad_grad_sliced = (float*)psdf::stream_scratch((size_t)c.Lt * nr_feat * N * sizeof(float), c.stream);
    if (!grad_grad_sliced) return PSDF_ERR_UNSUPPORTED;
  }
  return launched(dispatch_pf(pos_dim, nr_feat, [&](auto p, auto f) {
    return launch_dbl_plain(p, f, c, dd_positions, grad_sliced, grad_lattice, grad_grad_sliced);
  }));
}

int psdf_encode_double_backward(int pos_dim, int nr_feat, int64_t N, int nr_levels, int capacity,
                                const float* positions, const float* lattice, const float* scale_factor,
                                const float* shifts, const float* window, int concat_points, float points_scaling,
                                const float* dd_positions, const float* grad_sliced, float* grad_lattice,
                                float* grad_grad_sliced, void* stream) {
  return psdf_encode_double_backward_ws(pos_dim, nr_feat, N, nr_levels, capacity, positions, lattice, scale_factor, shifts,
                                        window, concat_points, points_scaling, dd_positions, grad_sliced, grad_lattice,
                                        grad_grad_sliced, nullptr, nullptr, 0, stream);
}

}  // extern "C"
