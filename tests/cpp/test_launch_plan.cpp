// test_launch_plan.cpp -- plan_launches (pmdfc_amd/csrc/launch_plan.h) over
// every input the engine can produce, against the launch table of DESIGN.md
// 4 written out as rows of data.  Host only, no HIP: tests/test_launch_plan.py
// builds it with the sanitizers and runs it.  Prints "OK <plans checked>".
#include <cstdio>

#include "../../pmdfc_amd/csrc/launch_plan.h"

using namespace pmdfc;

static_assert(kCpSbb == 3 && kParkedGrid == 3072 && kParkedGridRamp == 4096 && kFinalGrid == 256 &&
                  kFinalGridRamp == 1024 && kMixedSmallGrid == 256 && kSplitGroups == 512 && kSplitGroupsRamp == 1024,
              "the defaults (built without A/B macros)");

constexpr int kAny = -1;
constexpr uint32_t kPad = 1024, kTeam = 77;  // the knobs passed through

struct Row {
  // the inputs the row covers (kAny: both)
  int mixed, upsert, fast, wide, cp, small;
  // the first pass: the insert-only variant, its gate, grid = 2^p1 >> shift, whether it takes the LDS pad
  FirstPass first;
  uint32_t first_gate, first_shift;
  bool pad;
  // ... the mixed variant, its gate, whether on the small grid (min(2^p1, 256)) or on 2^p1
  MixedPass mixed_pass;
  uint32_t mixed_gate;
  bool small_grid;
  // k_apply_fb when the fb hint is set, and its gate
  bool fb;
  uint32_t fb_gate;
  ParkedPass parked;
  FinalPass fin;
  int probe;  // kAny: iff upsert
};

using F = FirstPass;
using M = MixedPass;
using P = ParkedPass;
using L = FinalPass;
static const Row kRows[] = {
    // insert-only, not upsert, fast_apply
    {0, 0, 1, 0, 1, 0, F::kFastCp, 0, 3, false, M::kNone, 0, false, true, 0, P::kInsert, L::kInsert, 0},
    {0, 0, 1, 1, 0, 0, F::kWide, 0, 0, false, M::kNone, 0, false, true, 0, P::kInsert, L::kInsert, 0},
    {0, 0, 1, 0, 0, 0, F::kFast, 0, 0, true, M::kNone, 0, false, true, 0, P::kInsert, L::kInsert, 0},
    // insert-only, upsert, fast_apply
    {0, 1, 1, 0, 0, 0, F::kFastUps, 0, 0, false, M::kNone, 0, false, true, 0, P::kInsert, L::kInsert, 0},
    {0, 1, 1, 1, 0, 0, F::kFastUpsWide, 0, 0, false, M::kNone, 0, false, true, 0, P::kInsert, L::kInsert, 0},
    // insert-only, fast_apply off: the probe iff upsert
    {0, kAny, 0, kAny, 0, 0, F::kGeneral, 0, 0, false, M::kNone, 0, false, false, 0, P::kInsert, L::kInsert, kAny},
    // mixed, not upsert (gated): lean or general under gate 2, never cp, then the mixed variant under gate 1
    {1, 0, 1, 0, 0, 0, F::kFast, 2, 0, true, M::kApply, 1, false, true, 2, P::kGated, L::kMixed, 0},
    {1, 0, 1, 1, 0, 0, F::kWide, 2, 0, false, M::kApply, 1, false, true, 2, P::kGated, L::kMixed, 0},
    {1, 0, 1, 0, 0, 1, F::kFast, 2, 0, true, M::kLoop, 1, true, true, 2, P::kGated, L::kMixed, 0},
    {1, 0, 1, 1, 0, 1, F::kWide, 2, 0, false, M::kLoop, 1, true, true, 2, P::kGated, L::kMixed, 0},
    {1, 0, 0, kAny, 0, 0, F::kGeneral, 2, 0, false, M::kApply, 1, false, false, 0, P::kGated, L::kMixed, 0},
    {1, 0, 0, kAny, 0, 1, F::kGeneral, 2, 0, false, M::kLoop, 1, true, false, 0, P::kGated, L::kMixed, 0},
    // mixed, upsert (ungated): the mixed variant alone, the probe always
    {1, 1, kAny, kAny, 0, 0, F::kNone, 0, 0, false, M::kApply, 0, false, false, 0, P::kMixed, L::kMixed, 1},
};

static bool covers(int want, bool have) { return want == kAny || (want != 0) == have; }
static uint32_t umin(uint32_t a, uint32_t b) { return a < b ? a : b; }

static int bad = 0;
#define CHECK(c)                                                                                          \
  do {                                                                                                    \
    if (!(c)) {                                                                                           \
      ++bad;                                                                                              \
      printf("FAIL %s: mixed %d upsert %d fast %d wide %d cp %d fb %d small %d ramp %d p1 %u\n", #c, in.mixed, \
             in.upsert, in.fast_apply, in.wide, in.cp, in.fb, in.mixed_small, in.ramp, in.p1);            \
    }                                                                                                     \
  } while (0)

static void check(const PlanIn& in) {
  const LaunchPlan p = plan_launches(in);
  const Row* r = nullptr;
  int hits = 0;
  for (const Row& x : kRows)
    if (covers(x.mixed, in.mixed) && covers(x.upsert, in.upsert) && covers(x.fast, in.fast_apply) &&
        covers(x.wide, in.wide) && covers(x.cp, in.cp) && covers(x.small, in.mixed_small)) {
      r = &x;
      ++hits;
    }
  CHECK(hits == 1);
  if (hits != 1) return;
  const uint32_t B = 1u << in.p1;
  CHECK(p.first == r->first);
  CHECK(p.first_gate == r->first_gate);
  CHECK(r->first == F::kNone || p.first_grid == B >> r->first_shift);
  CHECK(p.first_lds == (r->pad ? kPad : 0u));
  CHECK(p.mixed == r->mixed_pass);
  CHECK(p.mixed_gate == r->mixed_gate);
  CHECK(r->mixed_pass == M::kNone || p.mixed_grid == (r->small_grid ? umin(B, 256) : B));
  CHECK(p.fb == (r->fb && in.fb));
  CHECK(!p.fb || p.fb_gate == r->fb_gate);
  CHECK(p.fb_class == in.fb);
  CHECK(p.split_grid == (in.ramp ? 1024u : 512u));
  CHECK(p.team_max == kTeam);
  CHECK(p.parked == r->parked);
  CHECK(p.parked_grid == umin(B, in.ramp ? 4096 : 3072));
  CHECK(p.fin == r->fin);
  CHECK(p.final_grid == umin(B, in.ramp ? 1024 : 256));
  CHECK(p.probe == (r->probe == kAny ? in.upsert : r->probe != 0));
  // the invariants
  const bool is_lean = p.first == F::kFastCp || p.first == F::kWide || p.first == F::kFast ||
                       p.first == F::kFastUps || p.first == F::kFastUpsWide;
  CHECK(lean(p.first) == is_lean);
  CHECK(!p.fb || is_lean);  // k_apply_fb only behind a lean kernel
  CHECK(p.first_gate <= 2 && p.mixed_gate <= 2 && p.fb_gate <= 2);
  // a gate-2 launch is paired with a gate-1 launch of the same pass
  CHECK((p.first_gate == 2) == (p.mixed != M::kNone && p.mixed_gate == 1));
  CHECK(p.first_gate != 1 && p.mixed_gate != 2);
  CHECK((p.parked == P::kGated) == (p.first_gate == 2));
  CHECK(!p.fb || p.fb_gate == p.first_gate);  // it follows its lean kernel's variant
  CHECK(p.first != F::kFastCp || (p.first_gate == 0 && p.mixed == M::kNone));  // cp never with a gate
  CHECK(p.first != F::kNone || p.mixed != M::kNone);
}

int main() {
  const uint32_t p1s[] = {0, 3, 8, 12, 14};
  unsigned long plans = 0;
  for (int bits = 0; bits < 256; ++bits)
    for (uint32_t p1 : p1s) {
      PlanIn in{};
      in.mixed = bits & 1;
      in.upsert = bits & 2;
      in.fast_apply = bits & 4;
      in.wide = bits & 8;
      in.cp = bits & 16;
      in.fb = bits & 32;
      in.mixed_small = bits & 64;
      in.ramp = bits & 128;
      in.gated = in.mixed && !in.upsert;
      in.p1 = p1;
      in.fast_lds_pad = kPad;
      in.split_team_max = kTeam;
      // only what the engine can produce
      if (in.cp && (in.mixed || in.upsert || in.wide || !in.fast_apply || p1 <= kCpSbb)) continue;
      if (in.mixed_small && !in.gated) continue;
      check(in);
      ++plans;
    }
  if (bad) {
    printf("%d checks failed\n", bad);
    return 1;
  }
  printf("OK %lu\n", plans);
  return 0;
}
