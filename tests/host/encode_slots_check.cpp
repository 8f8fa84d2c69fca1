// Stand-alone check of the forward slot plan of permuto_sdf_amd/csrc/encode_plan.h (forward_slots: which levels a grid row of
// the paired encode forward handles): no HIP, no device, its own main.  tests/test_encode_forward_slots.py compiles it with
// -fsanitize=address,undefined -fno-sanitize-recover=all and runs it; exit status = failed checks.
#include <cstdio>

#include "encode_plan.h"

using namespace psdf::enc_plan;

static int failures = 0;

static void check(bool ok, const char* what, int L, int Lt, int pairs) {
  if (!ok) {
    failures++;
    fprintf(stderr, "FAILED (L = %d, Lt = %d, pairs = %d): %s\n", L, Lt, pairs, what);
  }
}
#define CHECK(...) check((__VA_ARGS__), #__VA_ARGS__, L, Lt, pairs)

// every property the plan promises, for one (L, Lt, pairs)
static void check_plan(int L, int Lt, int pairs) {
  const FwdSlots s = forward_slots(L, Lt, pairs);
  const int want_pairs = pairs < 0 ? 0 : (pairs > L / 2 ? L / 2 : pairs);      // clamped
  CHECK(s.n == Lt - want_pairs);
  CHECK(s.n >= 1 && s.n <= FWD_MAX_SLOTS);
  std::vector<int> seen((size_t)Lt, 0);
  int two = 0;
  for (int i = 0; i < s.n; i++) {
    CHECK(s.a[i] < Lt);
    if (s.a[i] < Lt) seen[s.a[i]]++;
    if (s.b[i] != FWD_SLOT_NONE) {
      two++;
      CHECK(s.b[i] < Lt);
      if (s.b[i] < Lt) seen[s.b[i]]++;
      // one member from each end, the i-th coarsest with the i-th finest; never a pseudo-level
      CHECK(i < want_pairs && s.a[i] == i && s.b[i] == L - 1 - i);
      CHECK(s.a[i] < s.b[i] && s.b[i] < L);
      CHECK(2 * (int)s.a[i] < L - 1 && 2 * (int)s.b[i] > L - 1);
    } else {
      CHECK(i >= want_pairs);
      if (i > want_pairs) CHECK(s.a[i] > s.a[i - 1]);                          // the singles follow in index order
    }
  }
  CHECK(two == want_pairs);
  for (int l = 0; l < Lt; l++) CHECK(seen[(size_t)l] == 1);                      // every level in exactly one slot
  for (int i = s.n; i < FWD_MAX_SLOTS; i++) CHECK(s.a[i] == 0 && s.b[i] == 0);   // the rest of the table is zero-initialised
  if (want_pairs == 0)
    for (int i = 0; i < s.n; i++) CHECK(s.a[i] == i && s.b[i] == FWD_SLOT_NONE);  // one level per slot in index order
}

int main() {
  // L = 1, even and odd L, with 0, 1 or 2 pseudo-levels, every number of pairs and a few past the clamp
  const int levels[] = {1, 2, 3, 4, 5, 7, 8, 15, 16, 24, 25, 32, 40};
  for (int L : levels)
    for (int extra = 0; extra <= 2; extra++)
      for (int pairs = -2; pairs <= L / 2 + 3; pairs++)
        if (L + extra - (pairs < 0 ? 0 : (pairs > L / 2 ? L / 2 : pairs)) <= FWD_MAX_SLOTS) check_plan(L, L + extra, pairs);
  {
    // the bench's shape written out: 16 levels + 2 pseudo-levels, 8 pairs -> 10 slots
    const int L = 16, Lt = 18, pairs = 8;
    const FwdSlots s = forward_slots(L, Lt, pairs);
    CHECK(s.n == 10);
    CHECK(s.a[0] == 0 && s.b[0] == 15 && s.a[7] == 7 && s.b[7] == 8);
    CHECK(s.a[8] == 16 && s.b[8] == FWD_SLOT_NONE && s.a[9] == 17 && s.b[9] == FWD_SLOT_NONE);
  }
  {
    // odd L: the middle level stays single, between the pairs and the pseudo-levels
    const int L = 5, Lt = 7, pairs = 9;
    const FwdSlots s = forward_slots(L, Lt, pairs);
    CHECK(s.n == 5);
    CHECK(s.a[0] == 0 && s.b[0] == 4 && s.a[1] == 1 && s.b[1] == 3);
    CHECK(s.a[2] == 2 && s.b[2] == FWD_SLOT_NONE && s.a[3] == 5 && s.a[4] == 6);
  }
  {
    // plans that do not apply: more slots than the table holds, or no levels at all
    int L = 43, Lt = 43, pairs = 0;
    CHECK(forward_slots(L, Lt, pairs).n == 0);
    pairs = 1;
    CHECK(forward_slots(L, Lt, pairs).n == 42);          // 43 levels, one pair: 42 slots fit
    L = 42, Lt = 44, pairs = 1;
    CHECK(forward_slots(L, Lt, pairs).n == 0);
    pairs = 2;
    CHECK(forward_slots(L, Lt, pairs).n == 42);
    L = 0, Lt = 0, pairs = 0;
    CHECK(forward_slots(L, Lt, pairs).n == 0);
    L = 4, Lt = 3, pairs = 1;
    CHECK(forward_slots(L, Lt, pairs).n == 0);
    L = 300, Lt = 300, pairs = 150;
    CHECK(forward_slots(L, Lt, pairs).n == 0);           // level indices are bytes
  }
  {
    // the default rule pairs every level that has a partner
    const int L = 16, Lt = 18, pairs = forward_pairs_default(16, 1 << 21);
    CHECK(pairs == 8);
    CHECK(forward_pairs_default(24, 49152) == 12 && forward_pairs_default(5, 1) == 2 && forward_pairs_default(1, 1) == 0);
  }
  if (failures == 0) printf("all checks passed\n");
  return failures;
}
