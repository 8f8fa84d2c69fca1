// encode_plan.h -- the host arithmetic behind the launches of encode.hip, in one place: the plan of the binned (queue + LDS
// reduction) lattice-gradient path, the size of one resident round of its workgroups, and the deal of that round over the
// levels.  Integers and doubles only: no HIP, no device, no state -- a plain C++17 compiler accepts this header, and
// tests/host/encode_plan_check.cpp runs it under the address and undefined-behaviour sanitizers.  What needs a device, a lock
// or memory that outlives a call (occupancy query, host-mapped arrays, the states of encode_balance) stays in encode.hip.
#pragma once
#include <cstdint>
#include <cstdlib>
#include <vector>

namespace psdf {
namespace enc_plan {

// Environment switches: an integer or the default.  Callers keep the value in a function-local static (read once per process).
inline int env_int(const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; }
inline long long env_long(const char* name, long long dflt) { const char* v = getenv(name); return v ? atoll(v) : dflt; }

// ------------------------------------------------------------------------------------------ queue plan
constexpr int Q_MAX_PARTS = 64;   // partitions of a level's table (the binning kernel keeps four counters per partition in LDS)

constexpr int Q_SLOT_BYTES = 1024;   // behind the tails: one word per level of cache votes; durations and drain counts (profile build)

// bytes == 0: the path does not apply (small batch, table too large for Q_MAX_PARTS partitions, queues past the kernels' 32-bit
// offsets) and every other field is 0.  The workspace is [rows | vals | tails | Q_SLOT_BYTES of per-level slots].
struct QueuePlan {
  int cap, np, shift;   // entries per (level, partition) queue; partitions; rows per partition = 1 << shift
  int64_t rows_bytes, vals_bytes, tails_bytes, bytes;
};

// min_n: PSDF_ENC_QUEUE_MIN_N (default 2^13); slice_delta: PSDF_ENC_QUEUE_SLICE_LOG2_DELTA (default 1, A/B switch).
inline QueuePlan queue_plan(int pos_dim, int nr_feat, int64_t N, int nr_levels, int capacity, int64_t min_n, int slice_delta) {
  // Below ~8 K points the fixed cost of the plan (counter memset, one resident round of binning workgroups, a reduce pass over
  // the whole table: ~27 us for 24 levels x 2^18 rows) exceeds what the plain path (LDS cache + float atomics, ~4.7 ns per point
  // when every level carries a gradient) spends.  Measured, tools/small_batch_enc_bench.py, lattice backward: 1 056 points
  // 10.8 us plain / 27.1 us queued; 49 152 points 232 / 71.5 us; 262 080 points 1206 / 174.5 us.  (Until round 3 the
  // threshold was 2^18 points: every backward of a training step -- ~49 K ray samples -- took the plain path.)
  if (N < min_n) return QueuePlan{};
  // rows per partition: the reduce kernel holds a partition's slice of the table in LDS.  64-KiB slices (two reduce
  // workgroups per CU) instead of the 128 KiB that fit: the coarse levels' queues are nearly empty, so with one workgroup per
  // (level, partition) and 16 partitions only half the CUs had work (16 levels: reduce + binning 0.966 -> 0.905 ms with 32).
  const int base = (nr_feat <= 2) ? 14 : (nr_feat <= 4 ? 13 : 12);   // rows/partition * F * 4 B <= 128 KiB
  int shift = base - (slice_delta < 0 ? 0 : (slice_delta > 3 ? 3 : slice_delta));
  while (shift < base && ((capacity + (1 << shift) - 1) >> shift) > Q_MAX_PARTS) shift++;   // large tables: keep the partition count
  const int rpp = 1 << shift;
  const int np = (capacity + rpp - 1) / rpp;
  if (np > Q_MAX_PARTS || rpp * nr_feat * 4 > 128 * 1024) return QueuePlan{};
  const int64_t contrib = (int64_t)(pos_dim + 1) * N;
  const int64_t cap = (contrib / np) + (contrib / np) / 4 + 4096;
  if (cap > 0x7fffffff) return QueuePlan{};
  // the kernels address a level's slice of the queues with 32-bit byte offsets (queue_store)
  if ((int64_t)np * cap * (nr_feat * 4 > 2 ? nr_feat * 4 : 2) > 0xffffffffll) return QueuePlan{};
  const auto round256 = [](int64_t b) { return (b + 255) & ~(int64_t)255; };
  const int64_t entries = (int64_t)nr_levels * np * cap;
  QueuePlan p{(int)cap, np, shift, round256(entries * 2), round256(entries * nr_feat * 4), round256((int64_t)nr_levels * np * 4), 0};
  p.bytes = p.rows_bytes + p.vals_bytes + p.tails_bytes + Q_SLOT_BYTES;
  return p;
}

// ------------------------------------------------------------------------------------------ one resident round
// The binning kernel walks super-tiles of `tile` points (block size x points per thread).
inline int64_t super_tiles(int64_t N, int tile) { return (N + tile - 1) / tile; }

// Workgroups per level of a rectangular grid: `resident` (workgroups per CU x CUs) shared among nr_levels, never more than a
// level has super-tiles, at least 1.  resident <= 0 (the occupancy query failed): 128 per level under the same clamp.
inline unsigned round_share(int resident, int nr_levels, int64_t tiles) {
  int64_t gx = resident > 0 ? (int64_t)resident / nr_levels : 128;
  if (gx > tiles) gx = tiles;
  return (unsigned)(gx < 1 ? 1 : gx);
}

// ------------------------------------------------------------------------------------------ the level deal
// share_l <- 1/2 share_l + 1/2 total x work_l / sum(work): a level whose workgroups ran longer gets more of the round next time;
// a closed level (its workgroups return at once) falls to the minimum.
constexpr int BAL_MAX_WG = 8192, BAL_MIN_PER_LEVEL = 4, BAL_MAX_LEVELS = 40;

// Size class of N: quarter octaves.
inline int size_bucket(int64_t N) {
  int bucket = 0;
  for (int64_t v = N; v > 1; v >>= 1) bucket += 4;
  const int64_t top = (int64_t)1 << (bucket / 4);
  return bucket + (int)(((N - top) * 4) / top);
}

// (batches below 2^18 points: a training step's 49 152 samples have fewer super-tiles per level than a level's equal share of
// the round, and the measured effect is inside the run-to-run noise, 449 / 447 it/s with against 471 / 438 without: off)
inline bool deal_eligible(bool switched_off, int nr_levels, int total, int64_t N) {
  return !(switched_off || nr_levels > BAL_MAX_LEVELS || total > BAL_MAX_WG || total < nr_levels * BAL_MIN_PER_LEVEL ||
           N < ((int64_t)1 << 18));
}

inline std::vector<int> first_deal(int nr_levels, int total) { return std::vector<int>((size_t)nr_levels, total / nr_levels); }

// work[l] = count_l x mean duration_l.  cap: no level gets more workgroups than it has super-tiles (idle ones).
inline void redeal(std::vector<int>& counts, const double* work, int total, int cap) {
  const int n = (int)counts.size();
  double sum = 0.0;
  for (int l = 0; l < n; l++) sum += work[l];
  if (!(sum > 0.0)) return;
  int used = 0;
  for (int l = 0; l < n; l++) {
    int c = (int)(0.5 * counts[l] + 0.5 * total * work[l] / sum + 0.5);
    c = c < BAL_MIN_PER_LEVEL ? BAL_MIN_PER_LEVEL : (c > cap ? cap : c);
    counts[l] = c;
    used += c;
  }
  // never more than one resident round: take the excess from the largest shares
  while (used > total) {
    int big = 0;
    for (int l = 1; l < n; l++)
      if (counts[l] > counts[big]) big = l;
    if (counts[big] <= BAL_MIN_PER_LEVEL) break;
    counts[big]--;
    used--;
  }
}

// What the previous launch's workgroups reported into times[] (one entry each, in level order: 24-bit duration, tagged with the
// low 8 bits of the launch's generation).  All of them, with that tag: re-deal; otherwise the launch is still running, or
// another shape ran in between: keep the deal (returns false).
inline bool redeal_from_times(std::vector<int>& counts, const volatile uint32_t* times, uint32_t gen, int total, int cap) {
  std::vector<double> work(counts.size(), 0.0);
  int id = 0;
  for (size_t l = 0; l < counts.size(); l++)
    for (int b = 0; b < counts[l]; b++, id++) {
      const uint32_t v = times[id];
      if ((v >> 24) != (gen & 255u) || (v & 0xFFFFFFu) == 0u) return false;
      work[l] += (double)(v & 0xFFFFFFu);
    }
  redeal(counts, work.data(), total, cap);
  return true;
}

// Final clamp to [1, cap] and the prefix layout: workgroups [first[l], first[l + 1]) serve level l.  Returns the grid size.
inline int deal_layout(std::vector<int>& counts, int cap, uint16_t* first) {
  int at = 0;
  for (size_t l = 0; l < counts.size(); l++) {
    if (counts[l] > cap) counts[l] = cap;
    if (counts[l] < 1) counts[l] = 1;
    first[l] = (uint16_t)at;
    at += counts[l];
  }
  first[counts.size()] = (uint16_t)at;
  return at;
}

// ------------------------------------------------------------------------------------------ forward slots
// The paired forward (encode_fwd_pair_kernel) runs one grid row per SLOT: a slot names one level, or two that a thread handles
// together.  Levels are taken as ordered coarse to fine by index (how every caller of this encoding builds its scale list; the
// scale factors live in device memory, so the host cannot sort them -- the order affects speed only, never results): slot
// i < pairs holds (i, L - 1 - i), one level from each end; the middle levels pairs .. L - 1 - pairs and the pseudo-levels
// L .. Lt - 1 follow singly, in index order.  Passed to the kernel by value.
constexpr int FWD_MAX_SLOTS = 42;
constexpr uint8_t FWD_SLOT_NONE = 0xFF;
struct FwdSlots {
  int n;                      // slots = grid rows
  uint8_t a[FWD_MAX_SLOTS];   // the slot's level (the coarse one of a pair)
  uint8_t b[FWD_MAX_SLOTS];   // the fine level of a pair, or FWD_SLOT_NONE
};

// pairs is clamped to [0, L / 2].  n == 0: the plan does not apply (more than FWD_MAX_SLOTS slots, or a level index that does not
// fit the table's bytes) and the caller launches one level per grid row as before.
inline FwdSlots forward_slots(int L, int Lt, int pairs) {
  FwdSlots s{};
  if (L < 1 || Lt < L || Lt >= (int)FWD_SLOT_NONE) return s;
  if (pairs < 0) pairs = 0;
  if (pairs > L / 2) pairs = L / 2;
  if (Lt - pairs > FWD_MAX_SLOTS) return s;
  int at = 0;
  for (int i = 0; i < pairs; i++, at++) {
    s.a[at] = (uint8_t)i;
    s.b[at] = (uint8_t)(L - 1 - i);
  }
  for (int l = pairs; l < Lt; l++) {
    if (l < L && l >= L - pairs) continue;   // the fine member of a pair
    s.a[at] = (uint8_t)l;
    s.b[at] = FWD_SLOT_NONE;
    at++;
  }
  s.n = at;
  return s;
}

// How many levels to pair when nobody said (PSDF_ENC_FWD_PAIRS = -1): every level that has a partner, at every batch size.
// Measured (profiles/enc_fwd_pairs_ab.txt), whole forward, pairs 0 / L/4 / 3L/8 / L/2: 2 M points x 16 levels 307.5 / 280.0 /
// 268.5 / 264.3 us, x 24 levels 457.8 / 417.9 / 399.0 / 391.6 us -- the two half-hashed middle levels together still gain;
// 49 152 points x 24 levels 25.8 / 24.5 / 23.1 / 23.2 us, 1 056 points inside the spread: no gate by N.
inline int forward_pairs_default(int L, int64_t N) {
  (void)N;
  return L / 2;
}

}  // namespace enc_plan
}  // namespace psdf
