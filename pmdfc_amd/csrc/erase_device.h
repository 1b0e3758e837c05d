// erase_device.h -- Erase(key) on one segment by one whole wave: the serial
// rule of DESIGN.md 4.8 (stated at the head of erase.hip), the one copy of its
// code.  k_erase_apply (erase.hip) calls it per op of a run, k_erase_matching
// (match.hip) per listed key of a segment.
#pragma once
#include "cceh_device.h"

namespace pmdfc {

// Every copy of `key` leaves the segment at sp (occupancy row `row`); returns
// the copies removed.  The calling wave owns the segment and its row for the
// launch; it reads back what it wrote, so pairs are loaded through L2
// (ld_pair_l2) and its stores are drained before the next probe (of this key
// or the caller's next).  A tripped guard sets trip (-> kErrEraseGuard).
__device__ __forceinline__ uint32_t erase_key(ulonglong2* sp, uint32_t* row, uint64_t key, uint32_t lane,
                                              bool& trip) {
  const bool lo = lane < kWindow;
  const uint32_t w = (uint32_t)(hash64(key) & 0xFF) * 4u;
  uint32_t copies = 0;
  for (;; ++copies) {
    // 1. the window in probe order, up to its first empty slot
    ulonglong2 pr = make_ulonglong2(kInvalid, 0ULL);
    if (lo) pr = ld_pair_l2(sp + ((w + lane) & (kSlots - 1)));
    const uint32_t em = (uint32_t)__ballot(lo && pr.x == kInvalid);
    uint32_t mm = (uint32_t)__ballot(lo && pr.x == key);
    if (em) mm &= (1u << __builtin_ctz(em)) - 1u;
    if (!mm) break;
    if (copies >= kWindow) {  // (cannot happen: a window holds 32 copies at most)
      trip = true;
      break;
    }
    // 2. the first match
    uint32_t p = (w + (uint32_t)__builtin_ctz(mm)) & (kSlots - 1);
    // 3. backward shift: lane l looks at slot p + l
    for (uint32_t step = 0;; ++step) {
      const bool in = lane >= 1u && lo;
      const uint32_t slot = (p + lane) & (kSlots - 1);
      ulonglong2 c = make_ulonglong2(kInvalid, 0ULL);
      if (in) c = ld_pair_l2(sp + slot);
      const uint32_t ce = (uint32_t)__ballot(in && c.x == kInvalid);
      const uint32_t home = (uint32_t)(hash64(c.x) & 0xFF) * 4u;
      uint32_t ok = (uint32_t)__ballot(in && c.x != kInvalid && ((slot - home) & (kSlots - 1)) >= lane);
      if (ce) ok &= (1u << __builtin_ctz(ce)) - 1u;
      if (!ok || step >= kSlots) {
        if (ok) trip = true;  // (cannot happen: the hole advances, an entry moves back 31 slots at most)
        if (lane == 0) {
          sp[p] = make_ulonglong2(kInvalid, 0ULL);
          atomicAnd(&row[p >> 5], ~(1u << (p & 31u)));
        }
        break;
      }
      const uint32_t l = (uint32_t)__builtin_ctz(ok);
      if (lane == l) sp[p] = c;
      p = (p + l) & (kSlots - 1);
    }
    // the next probe (of this key or the caller's next) reads these slots
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  }
  return copies;
}

}  // namespace pmdfc
