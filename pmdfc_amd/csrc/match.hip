// match.hip -- EraseMatching: every stored key k with (k & mask) == (p & mask)
// for one of n patterns p leaves the table, in one scan.
//
// The contract is the serial rule of Erase (erase.hip): with L the distinct
// matching keys in arena order and slot order, the table afterwards is the
// table before with Erase(L[0]), Erase(L[1]), ... applied.  Erase touches one
// segment's pairs and occupancy row and nothing else, so segments commute and
// one wave per segment is the whole schedule: k_erase_matching walks arena ids
// [0, min(ctl->nsegs, max_segs)) -- k_cbf_scan's walk (cbf.hip): every id below
// nsegs is live or retired empty, ids from nsegs on are never read -- and the
// wave that visits a segment is the only one that writes it in the launch.
//
// Per segment: the 1,024 keys in 16 loads of 64 (the next segment's issued
// before this one is judged), each live key tested against the pattern set.
//   no match            nothing is written: an absent pattern is a pure read;
//   every live key      the segment is cleared, {INVALID, 0} over the live slots
//   matches             and the occupancy row zeroed (erasing everything leaves
//                       nothing: the rule's result without its 1,024 shifts);
//   otherwise           the matching keys are listed in slot order in LDS and
//                       erase_key (erase_device.h) runs per listed key -- the
//                       list and not the slots is walked, because a shift moves
//                       entries back behind the point a slot walk has reached; a
//                       key stored twice is listed twice and its second erase
//                       probes and misses -- then the segment is read again
//                       (through L2) and must hold no match, else the guard
//                       bit is set.
// The pattern set: n == 1 is one compare; n > 1 an open-addressing table of the
// masked patterns in LDS (2,048 words for at most 1,024 patterns), built once
// per workgroup, its used slots marked in a bitmap of their own since 0 and ~0
// are patterns like any other.  An empty slot (key INVALID) is never tested.
#include "cceh_device.h"
#include "cceh_kernels.h"
#include "erase_device.h"

#include <algorithm>
#include <atomic>

namespace pmdfc {

constexpr uint32_t kMatchSetSlots = 2048;  // >= 2 * PMDFC_MATCH_MAX

__device__ __forceinline__ uint32_t match_set_slot(uint64_t v) {
  return (uint32_t)((v * 0x9E3779B97F4A7C15ULL) >> 53);  // the top 11 bits: kMatchSetSlots
}

__device__ __forceinline__ uint64_t ld_key(const ulonglong2* p) {
  return __builtin_nontemporal_load(reinterpret_cast<const unsigned long long*>(p));
}

// The pattern set of one workgroup: built by all 256 threads (n > 1), asked by any.
struct MatchSet {
  uint64_t* set;
  uint32_t* used;
  uint32_t n;
  uint64_t mask, p0;
  __device__ __forceinline__ void build(const MatchArgs& a) {
    n = a.n;
    mask = a.mask;
    p0 = a.patterns[0] & mask;
    if (n > 1) {
      if (threadIdx.x < kMatchSetSlots / 32) used[threadIdx.x] = 0u;
      __syncthreads();
      for (uint32_t i = threadIdx.x; i < n; i += 256u) {
        const uint64_t v = a.patterns[i] & mask;
        // the first slot this thread marks is its own (a repeated pattern takes a second one)
        for (uint32_t h = match_set_slot(v);; h = (h + 1u) & (kMatchSetSlots - 1)) {
          const uint32_t bit = 1u << (h & 31u);
          if (!(atomicOr(&used[h >> 5], bit) & bit)) {
            set[h] = v;
            break;
          }
        }
      }
      __syncthreads();
    }
  }
  __device__ __forceinline__ bool matches(uint64_t key) const {
    if (key == kInvalid) return false;
    const uint64_t v = key & mask;
    if (n == 1) return v == p0;
    for (uint32_t h = match_set_slot(v); (used[h >> 5] >> (h & 31u)) & 1u; h = (h + 1u) & (kMatchSetSlots - 1))
      if (set[h] == v) return true;  // (ends: at most half of the slots are used)
    return false;
  }
};

__global__ __launch_bounds__(256) void k_erase_matching(MatchArgs a) {
  __shared__ uint64_t set[kMatchSetSlots];
  __shared__ uint32_t used[kMatchSetSlots / 32];
  __shared__ uint64_t lists[4][kSlots];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wib = threadIdx.x >> 6;
  const uint32_t wave = blockIdx.x * 4u + wib;
  const uint32_t nwaves = gridDim.x * 4u;
  const uint32_t nsegs = min(a.ctl->nsegs, a.max_segs);
  MatchSet ms{set, used};
  ms.build(a);
  auto matches = [&](uint64_t key) -> bool { return ms.matches(key); };
  if (blockIdx.x == 0 && threadIdx.x == 0) a.out[3] = nsegs;
  uint64_t* list = lists[wib];
  unsigned long long removed = 0;
  uint32_t changed = 0, cleared = 0;
  bool trip = false;
  uint64_t k[16], nx[16];
  if (wave < nsegs) {
#pragma unroll
    for (uint32_t r = 0; r < 16; ++r) k[r] = ld_key(a.pairs + (size_t)wave * kSlots + r * 64u + lane);
  }
  for (uint32_t sid = wave; sid < nsegs; sid += nwaves) {
    // the next segment's loads fly while this one is judged
    const uint32_t nsid = sid + nwaves;
    if (nsid < nsegs) {
#pragma unroll
      for (uint32_t r = 0; r < 16; ++r) nx[r] = ld_key(a.pairs + (size_t)nsid * kSlots + r * 64u + lane);
    }
    uint32_t mbits = 0, nlive = 0, nmatch = 0;  // mbits: bit r, this lane's slot r * 64 + lane matches
#pragma unroll
    for (uint32_t r = 0; r < 16; ++r) {
      const bool m = matches(k[r]);
      if (m) mbits |= 1u << r;
      nlive += (uint32_t)__popcll(__ballot(k[r] != kInvalid));
      nmatch += (uint32_t)__popcll(__ballot(m));
    }
    if (nmatch) {
      ulonglong2* sp = a.pairs + (size_t)sid * kSlots;
      uint32_t* row = a.occ + (size_t)sid * 32u;
      ++changed;
      if (nmatch == nlive) {
#pragma unroll
        for (uint32_t r = 0; r < 16; ++r)
          if (k[r] != kInvalid) sp[r * 64u + lane] = make_ulonglong2(kInvalid, 0ULL);
        if (lane < 32u) row[lane] = 0u;
        removed += nmatch;
        ++cleared;
      } else {
        uint32_t cnt = 0;
#pragma unroll
        for (uint32_t r = 0; r < 16; ++r) {
          const bool m = (mbits >> r) & 1u;
          const uint64_t bal = __ballot(m);
          if (m) list[cnt + (uint32_t)__popcll(bal & ((1ULL << lane) - 1ULL))] = k[r];
          cnt += (uint32_t)__popcll(bal);
        }
        // this wave's lanes read what its other lanes listed
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        __builtin_amdgcn_wave_barrier();
        for (uint32_t i = 0; i < cnt; ++i) removed += erase_key(sp, row, list[i], lane, trip);
        // no match may be left: the segment as it is now, through L2
        // (cannot fail: every matching key was listed and erase_key removes every copy)
        bool left = false;
#pragma unroll
        for (uint32_t r = 0; r < 16; ++r) left |= matches(ld_pair_l2(sp + r * 64u + lane).x);
        if (__ballot(left)) trip = true;
        __builtin_amdgcn_wave_barrier();  // the next changed segment rewrites the list
      }
    }
    if (nsid < nsegs) {
#pragma unroll
      for (uint32_t r = 0; r < 16; ++r) k[r] = nx[r];
    }
  }
  if (lane == 0) {
    if (removed) atomicAdd(a.out, removed);
    if (changed) atomicAdd(a.out + 1, (unsigned long long)changed);
    if (cleared) atomicAdd(a.out + 2, (unsigned long long)cleared);
    if (trip) atomicOr(&a.ctl->err, kErrEraseGuard);
  }
}

#ifdef PMDFC_MATCH_TEAM
// The other ownership shape (A/B builds, -DPMDFC_MATCH_TEAM: measured in
// DESIGN.md 4.10 and not kept): a workgroup of four waves per segment.  Each
// wave loads and classifies a quarter (slots [256 w, 256 w + 256), 4 loads of
// 64), the counts meet in LDS, and the writing of a partly matching segment
// is handed to wave 0: it alone runs erase_key over the one list, which the
// four waves wrote in slot order; a cleared segment is written a quarter per
// wave (nothing is read back there).  Then every wave re-checks its quarter.
__global__ __launch_bounds__(256) void k_erase_matching_team(MatchArgs a) {
  __shared__ uint64_t set[kMatchSetSlots];
  __shared__ uint32_t used[kMatchSetSlots / 32];
  __shared__ uint64_t list[kSlots];
  __shared__ uint32_t cnts[2][4][2];  // by step parity and wave: live, matching
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wib = threadIdx.x >> 6;
  const uint32_t nsegs = min(a.ctl->nsegs, a.max_segs);
  MatchSet ms{set, used};
  ms.build(a);
  if (blockIdx.x == 0 && threadIdx.x == 0) a.out[3] = nsegs;
  unsigned long long removed = 0;
  uint32_t changed = 0, cleared = 0, par = 0;
  bool trip = false;
  uint64_t k[4], nx[4];
  if (blockIdx.x < nsegs) {
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) k[q] = ld_key(a.pairs + (size_t)blockIdx.x * kSlots + wib * 256u + q * 64u + lane);
  }
  for (uint32_t sid = blockIdx.x; sid < nsegs; sid += gridDim.x, par ^= 1u) {
    const uint32_t nsid = sid + gridDim.x;
    if (nsid < nsegs) {
#pragma unroll
      for (uint32_t q = 0; q < 4; ++q) nx[q] = ld_key(a.pairs + (size_t)nsid * kSlots + wib * 256u + q * 64u + lane);
    }
    uint32_t mbits = 0, live = 0, mine = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
      const bool m = ms.matches(k[q]);
      if (m) mbits |= 1u << q;
      live += (uint32_t)__popcll(__ballot(k[q] != kInvalid));
      mine += (uint32_t)__popcll(__ballot(m));
    }
    if (lane == 0) {
      cnts[par][wib][0] = live;
      cnts[par][wib][1] = mine;
    }
    __syncthreads();
    uint32_t nlive = 0, nmatch = 0, base = 0;
#pragma unroll
    for (uint32_t w = 0; w < 4; ++w) {
      nlive += cnts[par][w][0];
      nmatch += cnts[par][w][1];
      if (w < wib) base += cnts[par][w][1];
    }
    if (nmatch) {  // (uniform over the workgroup)
      ulonglong2* sp = a.pairs + (size_t)sid * kSlots;
      uint32_t* row = a.occ + (size_t)sid * 32u;
      if (nmatch == nlive) {
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q)
          if (k[q] != kInvalid) sp[wib * 256u + q * 64u + lane] = make_ulonglong2(kInvalid, 0ULL);
        if (threadIdx.x < 32u) row[threadIdx.x] = 0u;
        if (wib == 0) {
          removed += nmatch;
          ++changed;
          ++cleared;
        }
      } else {
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) {
          const bool m = (mbits >> q) & 1u;
          const uint64_t bal = __ballot(m);
          if (m) list[base + (uint32_t)__popcll(bal & ((1ULL << lane) - 1ULL))] = k[q];
          base += (uint32_t)__popcll(bal);
        }
        __syncthreads();
        if (wib == 0) {
          for (uint32_t i = 0; i < nmatch; ++i) removed += erase_key(sp, row, list[i], lane, trip);
          ++changed;
        }
        __syncthreads();  // wave 0's stores are drained (erase_key's fence): every wave reads its quarter again
        bool left = false;
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) left |= ms.matches(ld_pair_l2(sp + wib * 256u + q * 64u + lane).x);
        if (__ballot(left)) trip = true;
      }
    }
    if (nsid < nsegs) {
#pragma unroll
      for (uint32_t q = 0; q < 4; ++q) k[q] = nx[q];
    }
  }
  if (lane == 0) {
    if (removed) atomicAdd(a.out, removed);
    if (changed) atomicAdd(a.out + 1, (unsigned long long)changed);
    if (cleared) atomicAdd(a.out + 2, (unsigned long long)cleared);
    if (trip) atomicOr(&a.ctl->err, kErrEraseGuard);
  }
}
#define MATCH_KERNEL k_erase_matching_team
#define MATCH_SEGS_PER_BLOCK 1
#else
#define MATCH_KERNEL k_erase_matching
#define MATCH_SEGS_PER_BLOCK 4
#endif

// The loop's grid: the workgroups that are resident at once on the current
// device (the kernel's registers and LDS decide how many per CU), asked of the
// runtime once per device; 512 if it does not say.
static uint32_t match_blocks() {
  static std::atomic<uint32_t> cached[64];  // (zero-initialised; threads that meet an empty entry store the same value)
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  uint32_t b = cached[dev].load(std::memory_order_relaxed);
  if (!b) {
    int per_cu = 0, cus = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, MATCH_KERNEL, 256, 0) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || per_cu < 1 || cus < 1) {
      (void)hipGetLastError();
      b = 512;
    } else {
      b = (uint32_t)per_cu * (uint32_t)cus;
    }
    cached[dev].store(b, std::memory_order_relaxed);
  }
  return b;
}

void launch_erase_matching(const MatchArgs& a, hipStream_t s) {
  const uint64_t blocks = std::min<uint64_t>(std::max<uint64_t>((a.max_segs + MATCH_SEGS_PER_BLOCK - 1) / MATCH_SEGS_PER_BLOCK, 1), match_blocks());
  hipLaunchKernelGGL(MATCH_KERNEL, dim3((unsigned)blocks), dim3(256), 0, s, a);
}

}  // namespace pmdfc
