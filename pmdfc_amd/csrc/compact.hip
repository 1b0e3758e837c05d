// compact.hip -- device side of pmdfc_cceh_compact (gfx950, wave64; the rule:
// DESIGN.md 4.9, the host side: compact_host.hip).
//
// The table has been gathered into a version-1 pairs region (k_image_gather).
// k_compact_merge runs one ROUND of sibling merges inside it: one wave per
// original canonical index i.  Wave i leaves after a few loads unless i is a
// live left child at a depth above the initial one, its pair is not known to
// drop, the next live segment is its sibling as an earlier round left it, and
// the two hold at most fill_limit entries.  The pairs of a round are disjoint
// and wave i alone writes ld[i], ld[next[i]], cnt[i], next[i], refused[i] and
// image segment i, so a round needs no atomics but one counter add per merge.
// The one word another wave may read while it changes is ld[j] of a left
// child j that merges in this round: the word carries the round that made the
// segment, and a sibling made in the running round is left for the next one,
// whichever of the two values the reader sees -- every round merges exactly
// the pairs the table showed when it began.
//
// A merging wave works in two phases.  A: child 0's 1,024 occupancy bits from
// 16 ballots, one 64-bit word in each of the lanes 0..15; child 1 walked from
// the slot after its highest empty one (every cluster, the wrapping one too,
// from its true start), 64 slots per step: the 16-B loads and hash64 are
// lane-parallel, the first-free claim of each entry's 32-slot window on the
// bitmap is wave-uniform and in walk order (serial by design: at most 1,024
// scalar steps per pair, the pairs of a round in parallel), every entry's
// destination goes to LDS (2 KiB).  Nothing is written to memory.  B, only if
// no entry found its window full: child 1's pairs are stored at their
// destinations in image segment i -- child 0 is the parent's image as it
// stands and is never copied -- and the rows are updated.
#include <hip/hip_runtime.h>

#include "cceh_device.h"
#include "cceh_kernels.h"

namespace pmdfc {

namespace {

// lane `src`'s (wave-uniform) 64-bit word
__device__ __forceinline__ uint64_t lane_word(uint64_t v, uint32_t src) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)src);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)src);
  return (uint64_t)lo | ((uint64_t)hi << 32);
}

__global__ __launch_bounds__(64) void k_compact_merge(CompactArgs a) {
  __shared__ uint16_t s_dst[kSlots];
  const uint32_t i = blockIdx.x, lane = threadIdx.x;
  if (i >= a.nseg) return;
  const uint32_t L = a.ld[i] & 0xFFu;
  if (L == kCompactDead || L <= a.d0 || L > kMaxDepth || a.refused[i]) return;
  if (a.pos[i] & ((2u << (kMaxDepth - L)) - 1u)) return;  // a right child
  const uint32_t j = a.next[i];
  if (j >= a.nseg) return;
  const uint32_t lj = a.ld[j];
  if ((lj & 0xFFu) != L || (lj >> 8) >= a.round) return;  // no leaf of depth L, or one this round is making
  const uint32_t c0 = a.cnt[i], c1 = a.cnt[j];
  if (c0 + c1 > a.fill_limit) return;
  ulonglong2* seg0 = a.img + (size_t)i * kSlots;
  const ulonglong2* seg1 = a.img + (size_t)j * kSlots;

  // ---- A. the bitmaps: lane g < 16 holds the word of slots [64 g, 64 g + 64)
  uint64_t occ = 0, emp1 = 0;
  for (uint32_t g = 0; g < 16; ++g) {
    const uint64_t m0 = __ballot(seg0[g * 64u + lane].x != kInvalid);
    const uint64_t m1 = __ballot(seg1[g * 64u + lane].x == kInvalid);
    if (lane == g) {
      occ = m0;
      emp1 = m1;
    }
  }
  // the walk starts after child 1's highest empty slot (slot 0 if it has none)
  uint32_t start = 0;
  const uint64_t has = __ballot(emp1 != 0);
  if (has) {
    const uint32_t g = 63u - (uint32_t)__builtin_clzll(has);
    start = (g * 64u + 64u - (uint32_t)__builtin_clzll(lane_word(emp1, g))) & (kSlots - 1u);
  }
  bool drop = false;
  for (uint32_t k = 0; k < 16 && !drop; ++k) {
    const ulonglong2 p = seg1[(start + k * 64u + lane) & (kSlots - 1u)];
    const uint32_t w = ((uint32_t)hash64(p.x) & 0xFFu) * 4u;
    uint64_t m = __ballot(p.x != kInvalid);
    uint32_t dst = 0xFFFFu;
    while (m) {
      const uint32_t b = (uint32_t)__builtin_ctzll(m);
      m &= m - 1;
      const uint32_t wb = (uint32_t)__builtin_amdgcn_readlane((int)w, (int)b);
      // the 32 window bits from wb on, cyclically (wb is a multiple of 4)
      const uint32_t x = wb >> 6, sh = wb & 63u;
      const uint64_t lo = lane_word(occ, x), hi = lane_word(occ, (x + 1u) & 15u);
      const uint32_t fr = ~(uint32_t)(sh ? (lo >> sh) | (hi << (64u - sh)) : lo);
      if (!fr) {
        drop = true;
        break;
      }
      const uint32_t d = (wb + (uint32_t)__builtin_ctz(fr)) & (kSlots - 1u);
      if (lane == (d >> 6)) occ |= 1ULL << (d & 63u);
      if (lane == b) dst = d;
    }
    s_dst[k * 64u + lane] = (uint16_t)dst;
  }
  if (drop) {  // (wave-uniform) the pair is refused: both children as they were
    if (lane == 0) a.refused[i] = 1u;
    return;
  }

  // ---- B. child 1's entries to their slots of the parent, then the rows
  // (every lane reads back the s_dst word it wrote itself)
  for (uint32_t k = 0; k < 16; ++k) {
    const ulonglong2 p = seg1[(start + k * 64u + lane) & (kSlots - 1u)];
    const uint32_t dst = s_dst[k * 64u + lane];
    if (dst < kSlots && p.x != kInvalid) seg0[dst] = p;
  }
  if (lane == 0) {
    a.ld[i] = (L - 1u) | (a.round << 8);
    a.ld[j] = kCompactDead;
    a.cnt[i] = c0 + c1;
    a.next[i] = a.next[j];
    atomicAdd(a.merged, 1u);
  }
}

}  // namespace

void launch_compact_merge(const CompactArgs& a, hipStream_t s) {
  if (a.nseg) hipLaunchKernelGGL(k_compact_merge, dim3(a.nseg), dim3(64), 0, s, a);
}

}  // namespace pmdfc
