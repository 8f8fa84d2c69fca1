// Stand-alone check of permuto_sdf_amd/csrc/encode_plan.h: no HIP, no device, its own main.  tests/test_encode_host_plan.py
// compiles it with -fsanitize=address,undefined -fno-sanitize-recover=all and runs it.  Every expected value below was derived
// by hand from the code the header replaced (queue_plan and encode_balance of csrc/encode.hip); exit status = failed checks.
#include <cstdio>

#include "encode_plan.h"

using namespace psdf::enc_plan;
using Deal = std::vector<int>;

static int failures = 0;

static void check(bool ok, const char* what) {
  if (!ok) {
    failures++;
    fprintf(stderr, "FAILED: %s\n", what);
  }
}
#define CHECK(...) check((__VA_ARGS__), #__VA_ARGS__)

// times[] as the previous launch's workgroups leave it: entry = generation tag << 24 | duration, `per_wg[l]` ticks per workgroup
static std::vector<uint32_t> reported(const Deal& counts, const std::vector<uint32_t>& per_wg, uint32_t gen) {
  std::vector<uint32_t> t;
  for (size_t l = 0; l < counts.size(); l++)
    for (int b = 0; b < counts[l]; b++) t.push_back(((gen & 255u) << 24) | per_wg[l]);
  return t;
}

int main() {
  // size class of N
  CHECK(size_bucket(1 << 18) == 72);
  CHECK(size_bucket(300001) == 72);
  CHECK(size_bucket(327680) == 73);
  CHECK(size_bucket((1 << 19) - 1) == 75);
  CHECK(size_bucket(1 << 21) == 84);

  // eligibility of a launch for the deal
  CHECK(deal_eligible(false, 16, 768, 1 << 18));
  CHECK(!deal_eligible(true, 16, 768, 1 << 18));
  CHECK(!deal_eligible(false, 16, 768, (1 << 18) - 1));
  CHECK(!deal_eligible(false, 41, 768, 1 << 18));
  CHECK(!deal_eligible(false, 16, 63, 1 << 18));
  CHECK(!deal_eligible(false, 16, 8193, 1 << 18));

  // first deal, re-deal, layout
  const Deal equal = first_deal(4, 64);
  CHECK(equal == Deal{16, 16, 16, 16});
  {
    const double work[4] = {1, 1, 1, 5};
    Deal d = equal;
    redeal(d, work, 64, 64);
    CHECK(d == Deal{12, 12, 12, 28});
    uint16_t first[5] = {};
    CHECK(deal_layout(d, 64, first) == 64);
    CHECK(first[0] == 0 && first[1] == 12 && first[2] == 24 && first[3] == 36 && first[4] == 64);
    d = equal;
    redeal(d, work, 64, 20);   // a level has 20 super-tiles only
    CHECK(d == Deal{12, 12, 12, 20});
    const double none[4] = {0, 0, 0, 0};
    redeal(d, none, 64, 64);   // nothing measured: unchanged
    CHECK(d == Deal{12, 12, 12, 20});
  }
  {
    const double work[4] = {1, 1, 1, 997};
    Deal d = equal;
    redeal(d, work, 64, 64);
    CHECK(d == Deal{8, 8, 8, 40});
    redeal(d, work, 64, 64);
    CHECK(d == Deal{4, 4, 4, 52});
    redeal(d, work, 64, 64);   // the minimum share of 4 makes 70: the excess comes off the largest
    CHECK(d == Deal{4, 4, 4, 52});
  }

  // the durations of the previous launch: complete -> re-deal (count x duration = 16, 16, 16, 80: the work 1 : 1 : 1 : 5)
  {
    const uint32_t gen = 0x1ff;   // only the low 8 bits tag the entries
    Deal d = equal;
    std::vector<uint32_t> t = reported(d, {1, 1, 1, 5}, gen);
    CHECK(redeal_from_times(d, t.data(), gen, 64, 64) && d == Deal{12, 12, 12, 28});
    d = equal;
    t[40] = ((gen - 1) & 255u) << 24 | 1u;   // one workgroup of the previous generation: still running, keep the deal
    CHECK(!redeal_from_times(d, t.data(), gen, 64, 64) && d == equal);
    t = reported(d, {1, 1, 1, 5}, gen);
    t[63] &= 0xFF000000u;   // a zero duration: never written
    CHECK(!redeal_from_times(d, t.data(), gen, 64, 64) && d == equal);
  }

  // one resident round: 5 workgroups per CU x 256 CUs over 16 levels; short batches; a failed occupancy query
  CHECK(super_tiles(600001, 512) == 1172 && super_tiles(512, 512) == 1 && super_tiles(513, 512) == 2);
  CHECK(round_share(1280, 16, 4096) == 80 && round_share(1280, 16, 17) == 17 && round_share(8, 16, 4096) == 1);
  CHECK(round_share(0, 16, 4096) == 128 && round_share(0, 16, 17) == 17);

  // queue plan (default switches: at least 2^13 points, slices of half the LDS)
  {
    const QueuePlan a = queue_plan(3, 2, 600001, 8, 1 << 18, 1 << 13, 1);
    CHECK(a.np == 32 && a.cap == 97846 && a.shift == 13);
    const QueuePlan b = queue_plan(3, 4, 600001, 8, 1 << 18, 1 << 13, 1);
    CHECK(b.np == 64 && b.cap == 50971 && b.shift == 12);
    const int64_t entries = (int64_t)8 * 32 * 97846;
    CHECK(a.rows_bytes == ((entries * 2 + 255) & ~(int64_t)255) && a.vals_bytes == ((entries * 8 + 255) & ~(int64_t)255));
    CHECK(a.tails_bytes == 1024 && a.bytes == a.rows_bytes + a.vals_bytes + a.tails_bytes + 1024);
    CHECK(queue_plan(3, 2, 8191, 8, 1 << 18, 1 << 13, 1).bytes == 0);          // small batch
    CHECK(queue_plan(3, 2, 8192, 8, 1 << 18, 1 << 13, 1).bytes > 0);
    CHECK(queue_plan(3, 2, 600001, 8, 1 << 22, 1 << 13, 1).bytes == 0);        // 2^22 rows: more than 64 partitions of 2^14
    CHECK(queue_plan(3, 2, (int64_t)1 << 28, 8, 1 << 18, 1 << 13, 1).bytes == 0);   // queues past 32-bit offsets
  }
  if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
  else printf("encode_plan_check: all checks passed\n");
  return failures;
}
