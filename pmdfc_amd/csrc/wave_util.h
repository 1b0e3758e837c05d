// wave_util.h -- what the kernels of the batched Insert / mixed path (part.hip,
// bucket.hip) share below the bucket pass: the chunk geometry and the rop
// word's bits, the debug stamps (the stamp slots of every pass are named
// under "debug stamps") and the wave helpers (waitcnt, shuffles, the
// exclusive scan, the wave sorts).
#pragma once
#include "cceh_device.h"
#include "cceh_kernels.h"

namespace pmdfc {

constexpr int kCW = (int)kChunkWave;  // ops per wave chunk (LDS, register sort)
constexpr int kPer = kCW / 64;        // chunk slots per lane

constexpr uint32_t kGetBit = 0x80000000u;
constexpr uint32_t kOpMask = (1u << 22) - 1;

// ------------------------------------------------------------ debug stamps
//
// PMDFC_STAMPS=1: a wave stores wall_clock64() into its row of the batch's
// stamp set as it passes each phase (pmdfc_cceh_read_stamps; phase_stamps.py
// turns the rows into phase lengths).  row: null when stamps are off; writer:
// the one lane that stores.
__device__ __forceinline__ void stamp(uint64_t* row, uint32_t slot, bool writer) {
  if (row && writer) row[slot] = wall_clock64();
}
// k_part, 8 slots per block: start, tile counted, runs reserved, end
enum : uint32_t { kPsStart, kPsCounted, kPsReserved, kPsEnd };
// k_split, 8 slots per split: descriptors built, cluster starts known, replay
// done, parent pairs reloaded, stores issued, start, the replay taken (a
// value: 1 clusters, 2 generic), wrap unit replayed
enum : uint32_t { kSsHashed, kSsClusters, kSsReplayed, kSsReloaded, kSsStored, kSsStart, kSsPath, kSsWrapUnit };
// Bucket passes, 16 slots per directory bucket.  First pass: start, chunk
// loaded, round 0 ordered into runs (fast_claim: 0, no sort), its claims
// written, its ops binned by segment, in batch order, its runs applied
// (fast_claim: decisions final), end.  Final pass, 8-13: start, loaded, round
// 0 ordered, written, split, end.  14, 15: a first-pass run's claim loop and
// end (last writer).  fast_claim keeps its own three in 10-12, which a final
// pass of the same bucket overwrites: dependency masks built, rounds |
// dependent inserts << 16 (a value), dependent inserts resolved.
enum : uint32_t {
  kBsStart, kBsLoaded, kBsOrdered, kBsWritten, kBsBinned, kBsBatchOrder, kBsRunsDone, kBsEnd,
  kBsFinStart, kBsFinLoaded, kBsFinOrdered, kBsFinWritten, kBsFinSplit, kBsFinEnd, kBsRunClaimed, kBsRunEnd,
  kBsFcMasks = 10, kBsFcRounds = 11, kBsFcResolved = 12,
};

// ------------------------------------------------------------------ helpers

// s_waitcnt vmcnt(N) with the other counters left alone (gfx9 encoding)
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  __builtin_amdgcn_s_waitcnt((N & 15) | ((N >> 4) << 14) | (7 << 4) | (15 << 8));
}

__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int m) {
  const int lo = __shfl_xor((int)(uint32_t)v, m);
  const int hi = __shfl_xor((int)(uint32_t)(v >> 32), m);
  return ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
}

__device__ __forceinline__ uint32_t wave_excl_scan(uint32_t v, uint32_t* total) {
  const uint32_t lane = __lane_id() & 63u;
  uint32_t incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = (uint32_t)__shfl_up((int)incl, o);
    if (lane >= (uint32_t)o) incl += t;
  }
  *total = (uint32_t)__shfl((int)incl, 63);
  return incl - v;
}

// Ascending bitonic sort by one wave of keys held in registers: position
// KP*lane + q in v[q], n a power of two <= 64*KP, positions >= n hold ~0
// (they only meet each other, so every lane runs the same network).  Partner
// distances j < KP stay in the lane, larger ones are cross-lane shuffles
// (j/KP <= 32).
__device__ __forceinline__ uint32_t shfl_xor_key(uint32_t v, int m) { return (uint32_t)__shfl_xor((int)v, m); }
__device__ __forceinline__ uint64_t shfl_xor_key(uint64_t v, int m) { return shfl_xor64(v, m); }
template <class T, int KP>
__device__ __forceinline__ void wave_sort_regs(T (&v)[KP], uint32_t n) {
  const uint32_t lane = __lane_id() & 63u;
  const auto lo = [](T x, T y) { return x < y ? x : y; };
  const auto hi = [](T x, T y) { return x < y ? y : x; };
  for (uint32_t k = 2; k <= n; k <<= 1) {
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      if (j >= (uint32_t)KP) {
        const int m = (int)(j / KP);
#pragma unroll
        for (int q = 0; q < KP; ++q) {
          const uint32_t e = KP * lane + q;
          const T pv = shfl_xor_key(v[q], m);
          const bool up = (e & k) == 0, lower = (e & j) == 0;
          v[q] = (lower == up) ? lo(v[q], pv) : hi(v[q], pv);
        }
      } else {
        // in-lane partners: dispatch on j so every register index is static
        // (a runtime v[q + j] would put v[] in scratch memory)
#pragma unroll
        for (int jj = KP / 2; jj >= 1; jj >>= 1) {
          if ((int)j != jj) continue;
#pragma unroll
          for (int q = 0; q < KP; ++q) {
            if (q & jj) continue;
            const uint32_t e = KP * lane + q;
            const bool up = (e & k) == 0;
            const T x = v[q], y = v[q + jj];
            v[q] = up ? lo(x, y) : hi(x, y);
            v[q + jj] = up ? hi(x, y) : lo(x, y);
          }
        }
      }
    }
  }
}
template <int KP>
__device__ __forceinline__ void wave_sort32(uint32_t (&v)[KP], uint32_t n) {
  wave_sort_regs<uint32_t, KP>(v, n);
}
// s[0..nvalid) in LDS, padded with ~0 to n (a power of two <= kCW), sorted in
// place: s[0..n) holds the result
__device__ __forceinline__ void wave_sort8(uint64_t* s, uint32_t n, uint32_t nvalid) {
  const uint32_t lane = __lane_id() & 63u;
  uint64_t v[kPer];
#pragma unroll
  for (int q = 0; q < kPer; ++q) v[q] = (kPer * lane + q < nvalid) ? s[kPer * lane + q] : ~0ULL;
  wave_sort_regs<uint64_t, kPer>(v, n);
#pragma unroll
  for (int q = 0; q < kPer; ++q)
    if (kPer * lane + q < n) s[kPer * lane + q] = v[q];
  __builtin_amdgcn_wave_barrier();
}

// Positions < n of a 32-bit key array in LDS, sorted in place by one wave
// (KP keys per lane; p2 = n rounded up to a power of two, <= 64 * KP).
template <int KP>
__device__ __forceinline__ void wave_sort32_lds(uint32_t* buf, uint32_t n, uint32_t p2) {
  const uint32_t lane = __lane_id() & 63u;
  uint32_t v[KP];
#pragma unroll
  for (int q = 0; q < KP; ++q) v[q] = KP * lane + q < n ? buf[KP * lane + q] : ~0u;
  __builtin_amdgcn_wave_barrier();
  wave_sort32<KP>(v, p2);
#pragma unroll
  for (int q = 0; q < KP; ++q)
    if (KP * lane + q < n) buf[KP * lane + q] = v[q];
  __builtin_amdgcn_wave_barrier();
}

}  // namespace pmdfc
