// launch_plan.h -- which kernels the bucket passes of one general insert /
// mixed batch launch, in order, under which gate and on which grid: decided
// ONCE per batch by plan_launches from plain values (the batch's kind, the
// process knobs, the table's hints).  bucket.hip's launchers switch over the
// result.  No HIP, no environment: tests/cpp/test_launch_plan.cpp walks it.
#pragma once
#include <cstdint>

namespace pmdfc {

constexpr uint32_t kCpSbb = 3;  // coarse partition: 8 directory buckets per partition bucket

// the grids after the first pass (A/B builds override the macros); _RAMP:
// while the table ramps (p1 < p1max) or is small for the batch
#ifndef PMDFC_PARKED_GRID
#define PMDFC_PARKED_GRID 3072  // (3 waves per SIMD since round 6: 2048 13.13-13.15 Gops/s against 13.22; 1024 12.25-12.30 in round 4)
#endif
#ifndef PMDFC_PARKED_GRID_RAMP
#define PMDFC_PARKED_GRID_RAMP 4096
#endif
#ifndef PMDFC_FINAL_GRID
#define PMDFC_FINAL_GRID 256  // (1024 as above)
#endif
#ifndef PMDFC_FINAL_GRID_RAMP
#define PMDFC_FINAL_GRID_RAMP 1024
#endif
#ifndef PMDFC_MIXED_SMALL_GRID
#define PMDFC_MIXED_SMALL_GRID 256  // the mixed first pass's grid when the host expects it gated off
#endif
#ifndef PMDFC_SPLIT_GROUPS
#define PMDFC_SPLIT_GROUPS 512  // (1024: two dispatch rounds at 2 waves/SIMD, 12.41-12.44 against 12.56 Gops/s)
#endif
#ifndef PMDFC_SPLIT_GROUPS_RAMP
#define PMDFC_SPLIT_GROUPS_RAMP 1024
#endif
constexpr uint32_t kParkedGrid = PMDFC_PARKED_GRID, kParkedGridRamp = PMDFC_PARKED_GRID_RAMP;  // k_apply_parked waves
constexpr uint32_t kFinalGrid = PMDFC_FINAL_GRID, kFinalGridRamp = PMDFC_FINAL_GRID_RAMP;      // k_bucket waves
constexpr uint32_t kMixedSmallGrid = PMDFC_MIXED_SMALL_GRID;
constexpr uint32_t kSplitGroups = PMDFC_SPLIT_GROUPS, kSplitGroupsRamp = PMDFC_SPLIT_GROUPS_RAMP;  // k_split workgroups

struct PlanIn {
  bool mixed, upsert;  // a mixed batch (else insert-only); last-writer-wins Insert (PMDFC_CFG_UPSERT)
  bool gated;          // mixed and not upsert: both apply variants are launched and ctl->pget picks one
  bool fast_apply;     // the process knobs
  uint32_t fast_lds_pad, split_team_max;
  // the table's hints
  bool wide;         // more segments per bucket than the narrow lean pass's sub-directories hold
  bool cp;           // partitioned coarsely (insert-only, not upsert, not wide, lean, p1 > kCpSbb)
  bool fb;           // declines are expected: k_apply_fb takes them (else the parked pass does)
  bool mixed_small;  // gated: the mixed first pass is expected to exit, so it loops on a small grid
  bool ramp;         // the larger grids after the first pass
  uint32_t p1;       // directory bucket bits
};

// the first pass's insert-only variant (none for an ungated mixed batch): k_apply_fast_cp, k_apply_wide,
// k_apply_fast, k_apply_fast_ups<false>, <true>, k_apply<false>; all but the last are the lean ones
enum class FirstPass : uint8_t { kNone, kFastCp, kWide, kFast, kFastUps, kFastUpsWide, kGeneral };
constexpr bool lean(FirstPass f) { return f != FirstPass::kNone && f != FirstPass::kGeneral; }
// ... and its mixed variant (none for an insert-only batch): k_apply<true>, k_apply_mloop
enum class MixedPass : uint8_t { kNone, kApply, kLoop };
enum class ParkedPass : uint8_t { kInsert, kMixed, kGated };  // k_apply_parked<false>, <true>, k_apply_parked_gated
enum class FinalPass : uint8_t { kInsert, kMixed };           // k_bucket<false>, <true>

// The launches in order: [k_upsert_probe] .. k_part .. first, mixed, [k_apply_fb], k_split, parked, final.
// A gate (BucketArgs::gate): 0 runs always, 1 iff k_mixed_get left a Get pending, 2 iff not.  Grids in workgroups.
struct LaunchPlan {
  bool probe;  // k_upsert_probe runs before the batch and the first pass is given its result (upos)
  FirstPass first;
  uint32_t first_gate, first_grid, first_lds;
  MixedPass mixed;
  uint32_t mixed_gate, mixed_grid;
  bool fb, fb_class;  // k_apply_fb (a wave per bucket) behind the lean `first`; fb_class: the engine opens
  uint32_t fb_gate;   // its timing class, with or without the launch
  uint32_t split_grid, team_max;  // k_split
  ParkedPass parked;  // kGated: one launch, the insert-only body under gate 2, the mixed one under gate 1
  FinalPass fin;      // (ungated: whatever either variant left)
  uint32_t parked_grid, final_grid;
};

constexpr LaunchPlan plan_launches(const PlanIn& in) {
  LaunchPlan p{};
  const uint32_t B = 1u << in.p1;
  const auto capped = [B](uint32_t grid) { return B < grid ? B : grid; };
  if (in.mixed && !in.gated) {  // every Get goes through the ordered runs: the mixed variant alone
    p.probe = true;
    p.mixed = MixedPass::kApply;
    p.mixed_grid = B;
  } else {
    p.first_gate = p.fb_gate = in.gated ? 2u : 0u;
    p.first = !in.fast_apply ? FirstPass::kGeneral
              : in.upsert    ? (in.wide ? FirstPass::kFastUpsWide : FirstPass::kFastUps)
              : in.cp        ? FirstPass::kFastCp
              : in.wide      ? FirstPass::kWide
                             : FirstPass::kFast;
    p.first_grid = p.first == FirstPass::kFastCp ? B >> kCpSbb : B;
    p.probe = in.upsert && !in.fast_apply;  // (the lean upsert passes probe each window themselves)
    p.first_lds = p.first == FirstPass::kFast ? in.fast_lds_pad : 0u;
    p.fb = in.fb && lean(p.first);  // (k_apply_fb reads the flags a lean kernel wrote)
    if (in.gated) {
      p.mixed = in.mixed_small ? MixedPass::kLoop : MixedPass::kApply;
      p.mixed_gate = 1;
      p.mixed_grid = in.mixed_small ? capped(kMixedSmallGrid) : B;
    }
  }
  p.fb_class = in.fb;
  p.split_grid = in.ramp ? kSplitGroupsRamp : kSplitGroups;
  p.team_max = in.split_team_max;
  p.parked = in.gated ? ParkedPass::kGated : in.mixed ? ParkedPass::kMixed : ParkedPass::kInsert;
  p.parked_grid = capped(in.ramp ? kParkedGridRamp : kParkedGrid);
  p.fin = in.mixed ? FinalPass::kMixed : FinalPass::kInsert;
  p.final_grid = capped(in.ramp ? kFinalGridRamp : kFinalGrid);
  return p;
}

}  // namespace pmdfc
