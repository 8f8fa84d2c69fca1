// Stand-alone check of permuto_sdf_amd/csrc/frame_plan.h: no HIP, no device, its own main.  tests/test_frame_host.py compiles it
// with -fsanitize=address,undefined -fno-sanitize-recover=all and runs it.  The expected values below were derived by hand from
// the rule the header states (the largest multiple of 64 rays with rays * cap <= pool, at most the frame); exit status = failed
// checks.
#include <cstdio>

#include "frame_plan.h"

using namespace psdf::frame_plan;

static int failures = 0;

static void check(bool ok, const char* what) {
  if (!ok) {
    failures++;
    fprintf(stderr, "FAILED: %s\n", what);
  }
}
#define CHECK(...) check((__VA_ARGS__), #__VA_ARGS__)

static bool is(const Plan& p, int64_t rays, int64_t chunks, int64_t last) {
  return p.status == PLAN_OK && p.rays_per_chunk == rays && p.chunks == chunks && p.last_chunk == last &&
         (p.chunks - 1) * p.rays_per_chunk + p.last_chunk == p.pixels;
}

int main() {
  // a DTU view at the reference's pool: 2 097 152 / 64 = 32 768 rays; 1 920 000 = 58 * 32 768 + 19 456
  CHECK(is(plan(1200, 1600, 64, 2097152), 32768, 59, 19456));
  CHECK(plan(1200, 1600, 64, 2097152).pixels == 1920000);
  // a frame smaller than one chunk: one chunk of the whole frame, whatever its size
  CHECK(is(plan(40, 48, 64, 2097152), 1920, 1, 1920));
  CHECK(is(plan(41, 53, 64, 2097152), 2173, 1, 2173));
  CHECK(is(plan(1, 1, 64, 2097152), 1, 1, 1));
  // H W no multiple of 64: 41 * 53 = 2173 = 8 * 256 + 125 at a pool of 256 rays
  CHECK(is(plan(41, 53, 64, 64 * 256), 256, 9, 125));
  // a frame of exactly whole chunks: the last chunk is a full one
  CHECK(is(plan(40, 48, 64, 64 * 320), 320, 6, 320));
  // 40 * 48 = 1920 = 7 * 256 + 128
  CHECK(is(plan(40, 48, 64, 64 * 256), 256, 8, 128));
  // the floor comes before the multiple: 20 000 / 64 = 312.5 -> 312 -> 256; 99 999 / 100 = 999 -> 960
  CHECK(is(plan(40, 48, 64, 20000), 256, 8, 128));
  CHECK(is(plan(100, 100, 100, 99999), 960, 11, 400));
  // a pool of exactly 64 * cap: chunks of one wave's worth of rays; one sample less is refused
  CHECK(is(plan(40, 48, 64, 64 * 64), 64, 30, 64));
  CHECK(is(plan(41, 53, 96, 64 * 96), 64, 34, 61));
  CHECK(plan(40, 48, 64, 64 * 64 - 1).status == PLAN_ERR_ARG);
  // a cap of one sample
  CHECK(is(plan(10, 100, 1, 640), 640, 2, 360));
  // refusals
  CHECK(plan(0, 48, 64, 2097152).status == PLAN_ERR_ARG && plan(40, 0, 64, 2097152).status == PLAN_ERR_ARG);
  CHECK(plan(-1, 48, 64, 2097152).status == PLAN_ERR_ARG && plan(40, -5, 64, 2097152).status == PLAN_ERR_ARG);
  CHECK(plan(40, 48, 0, 2097152).status == PLAN_ERR_ARG && plan(40, 48, -64, 2097152).status == PLAN_ERR_ARG);
  CHECK(plan(40, 48, 64, 0).status == PLAN_ERR_ARG && plan(40, 48, 64, -1).status == PLAN_ERR_ARG);
  CHECK(plan(40, 48, 0x7fffffff, 2097152).status == PLAN_ERR_ARG);   // 64 * cap does not overflow: it is formed in 64 bits
  // H W >= 2^31: 65 536 * 32 768 = 2^31 is refused, one row less is not
  CHECK(plan(65536, 32768, 64, 2097152).status == PLAN_ERR_UNSUPPORTED);
  CHECK(plan(0x7fffffff, 0x7fffffff, 64, 2097152).status == PLAN_ERR_UNSUPPORTED);
  CHECK(is(plan(65535, 32768, 64, 2097152), 32768, 65535, 32768));
  CHECK(is(plan(0x7fffffff, 1, 64, 2097152), 32768, 65536, 32767));
  // a refused plan has every other field zero
  {
    const Plan p = plan(0, 48, 64, 2097152);
    CHECK(p.pixels == 0 && p.rays_per_chunk == 0 && p.chunks == 0 && p.last_chunk == 0);
  }
  // a pool beyond int32
  CHECK(is(plan(1200, 1600, 64, (int64_t)1 << 40), 1920000, 1, 1920000));
  // check_range: the elements [first, first + count) of a rows x cols image.  40 * 48 = 1920
  CHECK(check_range(40, 48, 0, 1920) == PLAN_OK);                       // first = 0 and count = pixels
  CHECK(check_range(40, 48, 77, 333) == PLAN_OK && check_range(7, 7, 0, 49) == PLAN_OK);
  CHECK(check_range(40, 48, 1919, 1) == PLAN_OK);                       // the last element alone
  CHECK(check_range(40, 48, 1919, 2) == PLAN_ERR_ARG);                  // the last element one past the end
  CHECK(check_range(40, 48, 1, 1920) == PLAN_ERR_ARG && check_range(40, 48, 1920, 1) == PLAN_ERR_ARG);
  CHECK(check_range(40, 48, 0, 1921) == PLAN_ERR_ARG);
  CHECK(check_range(40, 48, 0, 0) == PLAN_ERR_ARG && check_range(40, 48, 5, -1) == PLAN_ERR_ARG);   // count = 0 is the caller's case
  CHECK(check_range(40, 48, -1, 10) == PLAN_ERR_ARG);                   // a negative first
  CHECK(check_range(0, 48, 0, 1) == PLAN_ERR_ARG && check_range(40, -3, 0, 1) == PLAN_ERR_ARG);
  // 65 536 * 32 768 = 2^31 elements: unsupported whatever the range; one row less is a frame like any other
  CHECK(check_range(65536, 32768, 0, 1) == PLAN_ERR_UNSUPPORTED && check_range(65536, 32768, -1, 1) == PLAN_ERR_UNSUPPORTED);
  CHECK(check_range(65535, 32768, 2147450879, 1) == PLAN_OK && check_range(65535, 32768, 2147450880, 1) == PLAN_ERR_ARG);
  // the order of the refusals: a bad extent or count before the size, the size before the position
  CHECK(check_range(65536, 32768, 0, 0) == PLAN_ERR_ARG);
  // first + count is never formed: a first near the top of int64 does not overflow
  CHECK(check_range(40, 48, INT64_MAX, 1) == PLAN_ERR_ARG && check_range(40, 48, 0, INT64_MAX) == PLAN_ERR_ARG);
  if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
  else printf("frame_plan_check: all checks passed\n");
  return failures;
}
