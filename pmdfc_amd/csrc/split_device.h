// split_device.h -- a segment split on the device (cluster replay below): one
// wave per split (wave_split) or a team of four (split_team<4>).  k_split
// (bucket.hip) runs the requested splits of a round; the final pass
// (bucket_pass.h grow_and_split) splits inline.
#pragma once
#include "wave_util.h"

namespace pmdfc {

// ---------------------------------------------------------------- splitting
//
// Segment::Split (non-INPLACE, CCEH_hybrid.cpp:47-66): walk the parent in slot
// order 0..1023; each entry goes to child (hash bit 63-L) at the first free
// slot of its own 32-slot window, or is dropped if that window is full.
//
// Cluster decomposition (exact).  Inserts never free a slot, and
// slots are freed only by Erase, which restores this before it returns
// (erase.hip): an entry at parent slot s with window start w has every slot
// of [w, s] occupied, so it lies in one CLUSTER (maximal run of occupied
// parent slots).  Replaying in slot order, every entry lands in [w, s]: all
// entries before it landed at or before their own slots.  So clusters replay
// independently, each by one lane with its two child bitmaps in registers.
// The one exception is the cluster that wraps past slot 1023: the reference
// walks its head [0, b] first, so its tail entries can be pushed past 1023
// into wrapped slots <= 30 (or dropped); that cluster, plus every cluster
// starting at <= 30, is one unit replayed by one lane in slot order.  A fully
// occupied parent or a wrap unit wider than 128 slots takes the slower
// generic replay (wave_replay).  The other clusters are replayed as a sweep
// over positions (no drops are possible outside the wrap unit; see the
// comment at the sweep).
constexpr uint32_t kSplitScratch = 2080;  // u32 words per splitting wave

__device__ __forceinline__ uint32_t occ_end(const uint32_t* s_occ, uint32_t a) {
  uint32_t w = a >> 5;
  uint32_t bits = ~s_occ[w] & (~0u << (a & 31u));
  while (bits == 0) {
    if (++w == 32) return kSlots;
    bits = ~s_occ[w];
  }
  return w * 32u + (uint32_t)__builtin_ctz(bits);
}

__device__ __forceinline__ uint32_t ext32(uint64_t lo, uint64_t hi, uint32_t r) {
  if (r >= 128) return 0;
  if (r >= 64) return (uint32_t)(hi >> (r - 64));
  return (uint32_t)((lo >> r) | (r ? (hi << (64 - r)) : 0ULL));
}

// Replay parent slots [x, y) for ONE child c into a 128-bit map relative to
// origin o (the unit's first slot): only the child's entries are visited
// (a bit walk over the occupancy / child-1 words), in slot order.
__device__ __forceinline__ void unit_range(const uint16_t* s_inf, const uint32_t* s_occ, const uint32_t* s_ch1,
                                           uint16_t* s_dst, uint64_t& lo, uint64_t& hi, uint32_t c, uint32_t o,
                                           uint32_t x, uint32_t y, uint32_t* loss, bool* bad) {
  for (uint32_t wd = x >> 5; wd * 32u < y; ++wd) {
    const uint32_t ch = s_ch1[wd];
    uint32_t b = c ? ch : (s_occ[wd] & ~ch);
    if (wd == (x >> 5)) b &= ~0u << (x & 31u);
    if (y - wd * 32u < 32u) b &= (1u << (y - wd * 32u)) - 1u;
    while (b) {
      const uint32_t s = wd * 32u + (uint32_t)__builtin_ctz(b);
      b &= b - 1u;
      const uint32_t e = s_inf[s];
      const uint32_t rw = ((e & 0xFFu) * 4u - o) & (kSlots - 1);
      const uint32_t fr = ~ext32(lo, hi, rw);
      if (fr == 0) {
        ++*loss;  // window full: Insert4split drops the entry (CCEH_hybrid.cpp:24-27)
        continue;
      }
      const uint32_t q = rw + (uint32_t)__builtin_ctz(fr);
      if (q >= 128) {
        *bad = true;
        continue;
      }
      if (q < 64) lo |= 1ULL << q;
      else hi |= 1ULL << (q - 64);
      s_dst[s] = (uint16_t)((c << 10) | ((o + q) & (kSlots - 1)));
    }
  }
}

__device__ __forceinline__ void unit_flush(uint32_t* s_cb, uint64_t lo, uint64_t hi, uint32_t c,
                                           uint32_t o) {
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const uint64_t src = m < 2 ? lo : hi;
    const uint32_t chunk = (uint32_t)(src >> (32 * (m & 1)));
    if (!chunk) continue;
    const uint32_t slot = (o + 32u * m) & (kSlots - 1);
    const uint32_t wi = slot >> 5, sh = slot & 31u;
    atomicOr(&s_cb[c * 32u + wi], chunk << sh);
    if (sh) atomicOr(&s_cb[c * 32u + ((wi + 1u) & 31u)], chunk >> (32u - sh));
  }
}

// Generic replay (wave_replay) for the rare parents the cluster path does not
// take; reads the slot descriptors from s_inf, leaves the placements in s_dst
// and the child bitmaps in s_cb.  Returns this lane's dropped entries.
__device__ inline __noinline__ uint32_t split_slow(const uint16_t* s_inf, uint16_t* s_dst, uint32_t* s_cb,
                                            uint32_t* s_rep) {
  const uint32_t lane = __lane_id() & 63u;
  uint32_t inf[16], dest[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const uint32_t e = s_inf[j * 64 + lane];
    inf[j] = ((e & 0x8000u) ? 0x80000000u : 0u) | (e & 0x1FFu);
  }
  s_rep[lane] = 0;
  __builtin_amdgcn_wave_barrier();
  const uint32_t loss = wave_replay(inf, dest, s_rep, s_rep + 64, s_rep + 128);
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int j = 0; j < 16; ++j) s_dst[j * 64 + lane] = dest[j] == 0xFFFFFFFFu ? 0xFFFF : (uint16_t)dest[j];
  s_cb[lane] = s_rep[lane];
  __builtin_amdgcn_wave_barrier();
  return loss;
}

// Split `seg` (local depth L) into seg (child 0, the parent's storage) and c1
// with a team of NW waves (1, or 4 of one workgroup: k_split when the split
// list is short -- a split is then a chain of dependent phases, and four waves
// quarter its loads and stores).  Wave v of the team loads, hashes and later
// stores the slot groups [v * 16 / NW, (v + 1) * 16 / NW) (group g = slots
// 64g..64g+63); the replay in between (cluster sweep / wave_replay) is wave
// 0's.  Returns dropped entries (the team's total, on every wave); *bad_out
// is set if an internal assumption failed (reported as a sticky device
// error).  NW = 4 needs every wave of the workgroup (barriers).
// drops != null (mixed batches): each dropped entry is logged as {key, trig},
// trig = the batch position of the insert whose full window split `seg`.
template <int NW>
__device__ __forceinline__ uint32_t split_team(ulonglong2* __restrict__ pairs, uint32_t* __restrict__ occ,
                                               uint8_t* __restrict__ ldep, uint32_t seg, uint32_t c1, uint32_t L,
                                               uint32_t* scr, bool* bad_out, uint64_t* srow, ulonglong2* drops,
                                               uint32_t* drop_n, uint32_t trig, uint32_t v) {
  static_assert(NW == 1 || NW == 4, "team of 1 or 4 waves");
  constexpr int G = 16 / NW;  // slot groups per wave
  const auto team_barrier = [] {
    if constexpr (NW == 1) __builtin_amdgcn_wave_barrier();
    else __syncthreads();
  };
  const uint32_t lane = __lane_id() & 63u;
  uint16_t* s_inf = reinterpret_cast<uint16_t*>(scr);          // 1024 x u16
  uint16_t* s_dst = reinterpret_cast<uint16_t*>(scr + 512);    // 1024 x u16
  uint32_t* s_occ = scr + 1024;                                // 32 words
  uint32_t* s_cb = scr + 1056;                                 // 64 words: child bitmaps
  uint32_t* s_ch1 = scr + 1120;                                // 32 words: parent slots of child 1
  uint32_t* s_tm = scr + 1152;                                 // team words: [0] far | bad, [1] loss
  uint32_t* s_rep = scr + 1376;                                // 3 x 64 words (fallback)
  uint32_t* s_E = scr + 1568;                                  // 2 x 256 words: per child and home line,
                                                               // the entries' slots relative to 4 * line
  ulonglong2* sp = pairs + (size_t)seg * kSlots;
  ulonglong2* s1 = pairs + (size_t)c1 * kSlots;
  const int g0 = (int)v * G;
  // keys only: the pairs are re-read (L2-hot) after placement, before the
  // first store, so nothing is live across the replay
  uint64_t pk[G];
#ifndef PMDFC_SPLIT_NT
#define PMDFC_SPLIT_NT 0  // (A/B builds) 1: the first read of the parent with non-temporal loads
#endif
#pragma unroll
  for (int j = 0; j < G; ++j) {
    // a plain load: the parent's lines stay in L2 for the reload below (a
    // non-temporal first read let them go: the reload then came from HBM,
    // ~14 us of a ~35 us split in the heaviest batches)
    if constexpr (PMDFC_SPLIT_NT)
      pk[j] = __builtin_nontemporal_load(reinterpret_cast<const uint64_t*>(sp + (g0 + j) * 64 + lane));
    else
      pk[j] = reinterpret_cast<const uint64_t*>(sp + (g0 + j) * 64 + lane)[0];
  }
  for (uint32_t t = v * 64u + lane; t < 512u; t += 64u * NW) s_E[t] = 0;
  if (v == 0) {
    s_cb[lane] = 0;
    if (lane < 2) s_tm[lane] = 0;
  }
  team_barrier();
  bool far = false;  // an entry more than 31 slots past its window start (cannot happen)
#pragma unroll
  for (int j = 0; j < G; ++j) {
    const int g = g0 + j;
    const bool valid = pk[j] != kInvalid;
    const uint64_t kh = hash64(pk[j]);
    if (valid) {
      const uint32_t sl = (uint32_t)g * 64u + lane, hl = (uint32_t)(kh & 0xFF);
      const uint32_t rel = (sl - 4u * hl) & (kSlots - 1);
      far |= rel > 31u;
      atomicOr(&s_E[((uint32_t)((kh >> (63 - L)) & 1u) << 8) | hl], 1u << (rel & 31u));
    }
    // bit 15 valid, bit 8 child (hash bit 63-L, CCEH_hybrid.cpp:52-55), bits 0-7 home line
    s_inf[g * 64 + lane] = (uint16_t)((valid ? 0x8000u : 0u) | ((uint32_t)((kh >> (63 - L)) & 1u) << 8) |
                                      (uint32_t)(kh & 0xFF));
    s_dst[g * 64 + lane] = 0xFFFF;
    const uint64_t m = __ballot(valid);
    const uint64_t m1 = __ballot(valid && ((kh >> (63 - L)) & 1u));
    if (lane == 0) {
      s_occ[2 * g] = (uint32_t)m;
      s_ch1[2 * g] = (uint32_t)m1;
    }
    if (lane == 1) {
      s_occ[2 * g + 1] = (uint32_t)(m >> 32);
      s_ch1[2 * g + 1] = (uint32_t)(m1 >> 32);
    }
  }
  if (NW > 1 && __ballot(far) && lane == 0) atomicOr(&s_tm[0], 1u);
  team_barrier();
  stamp(srow, kSsHashed, lane == 0 && v == 0);
  uint32_t loss = 0;
  if (v == 0) {
    bool bad = far || (NW > 1 && (s_tm[0] & 1u));
    // ---- clusters.  Lane l replays child c = l >> 5 for the clusters that
    // START in slots [32w, 32w + 32), w = l & 31 (so a long cluster costs one
    // lane per child, and both children run in parallel).
    const uint32_t c = lane >> 5, wl = lane & 31u;
    const uint32_t ow = s_occ[wl];
    const uint32_t pw = wl ? s_occ[wl - 1] : 0u;
    const uint32_t stw = ow & ~((ow << 1) | (pw >> 31));  // cluster starts in my word
    const bool all_full = __ballot(ow != ~0u) == 0;
    const bool cyclic = !all_full && (s_occ[0] & 1u) && (s_occ[31] >> 31);
    // the cluster holding slot 1023 starts at the last start overall
    const uint64_t nzw = __ballot(lane < 32 && stw != 0);
    const int tl = nzw ? 63 - __builtin_clzll(nzw) : 0;
    const uint32_t tail = (uint32_t)__shfl((int)(tl * 32 + (stw ? 31 - __builtin_clz(stw) : 0)), tl);
    const uint32_t head_end = cyclic ? occ_end(s_occ, 0) : 0u;
    stamp(srow, kSsClusters, lane == 0);
    bool wide = false;  // a unit outgrew the 128-bit window
    if (!all_full) {
      if (cyclic && wl == 0) {
        // the wrap unit in the reference's slot order: head, clusters starting
        // at <= 30, then the tail (which may push entries into wrapped slots)
        uint64_t lo = 0, hi = 0;
        unit_range(s_inf, s_occ, s_ch1, s_dst, lo, hi, c, tail, 0, head_end, &loss, &wide);
        uint32_t mb = stw & ~1u;
        while (mb) {
          const uint32_t a0 = (uint32_t)__builtin_ctz(mb);
          mb &= mb - 1;
          if (a0 <= 30u) unit_range(s_inf, s_occ, s_ch1, s_dst, lo, hi, c, tail, a0, occ_end(s_occ, a0), &loss, &wide);
        }
        unit_range(s_inf, s_occ, s_ch1, s_dst, lo, hi, c, tail, tail, kSlots, &loss, &wide);
        unit_flush(s_cb, lo, hi, c, tail);
      }
      stamp(srow, kSsWrapUnit, lane == 0);
      // The other clusters: a sweep over positions, each 32-slot word by its
      // own lane.  Outside the wrap unit an entry at parent slot s with window
      // start w lands at some x in [w, s] of its child (the slots [w, s) hold at
      // most s - w earlier entries of it), so nothing is dropped, and replayed
      // in slot order the child's position x goes to the waiting entry with the
      // smallest s among those with w <= x (an earlier entry that could take x
      // would have, when x was still free).  So: M's bit k = the entry at slot
      // x + k is waiting; at x = 4h the entries of home line h join (s_E, bits
      // relative to 4h, all within 32); x takes M's lowest bit.
      // Words in parallel: the number waiting, P, follows P -> max(P + A - 4, 0)
      // over a home line with A arrivals, and these maps compose as
      // P -> max(P + alpha, beta), so a 32-lane scan gives P at every word
      // start.  P = 0 means nothing waits (M = 0): a lane replays from the last
      // word start at or before its own where P = 0 (usually its own or the
      // one before), recording only its own word's placements.
      {
        const uint32_t* Ec = s_E + c * 256u;
        uint32_t U = 0, T = kSlots;  // [U, T): the positions outside the wrap unit
        if (cyclic) {
          const uint32_t o0 = s_occ[0];
          const uint32_t st0 = o0 & ~(o0 << 1) & 0x7FFFFFFEu;  // cluster starts 1..30
          U = max(head_end, st0 ? occ_end(s_occ, 31u - (uint32_t)__builtin_clz(st0)) : 0u);
          T = tail;
        }
        const uint4* E4 = reinterpret_cast<const uint4*>(Ec);
        const auto line8 = [&](uint32_t vv, uint32_t (&e)[8]) {  // the 8 home lines of word vv
          const uint4 p = E4[2u * vv], q = E4[2u * vv + 1u];
          e[0] = p.x, e[1] = p.y, e[2] = p.z, e[3] = p.w, e[4] = q.x, e[5] = q.y, e[6] = q.z, e[7] = q.w;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const uint32_t x = vv * 32u + 4u * (uint32_t)j;
            if (x < U || x >= T) e[j] = 0u;  // the wrap unit's (replayed above)
          }
        };
        uint32_t e8[8];
        line8(wl, e8);
        int sa = 0, sb = 0;  // my word's map
        uint32_t anyw = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int a1 = __builtin_popcount(e8[j]) - 4;
          sa += a1;
          sb = max(sb + a1, 0);
          anyw |= e8[j];
        }
        // inclusive scan (composition) over my child's words 0..wl
        for (int o = 1; o < 32; o <<= 1) {
          const int pa = __shfl_up(sa, o, 32), pb = __shfl_up(sb, o, 32);
          if (wl >= (uint32_t)o) {
            sb = max(pb + sa, sb);
            sa += pa;
          }
        }
        const int pend = max(sa, sb);  // waiting after my word
        int pst = __shfl_up(pend, 1, 32);
        if (wl == 0) pst = 0;
        const uint32_t zb = (uint32_t)(__ballot(pst == 0) >> (32u * c)) & (wl == 31u ? ~0u : (2u << wl) - 1u);
        const uint32_t w0 = 31u - (uint32_t)__builtin_clz(zb);
        uint32_t M = 0;
        for (uint32_t vv = pst > 0 ? w0 : wl; vv < wl; ++vv) {  // catch up, recording nothing
          uint32_t ev[8];
          line8(vv, ev);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            M |= ev[j];
#pragma unroll
            for (int t = 0; t < 4; ++t) M = (M & (M - 1u)) >> 1;
          }
        }
        if (pst > 0 || anyw) {
          const uint32_t base = wl * 32u;
          uint32_t occw = 0;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            M |= e8[j];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
              if (M) {
                const uint32_t x = base + 4u * (uint32_t)j + (uint32_t)t;
                s_dst[(x + (uint32_t)__builtin_ctz(M)) & (kSlots - 1)] = (uint16_t)((c << 10) | x);
                occw |= 1u << (4 * j + t);
                M &= M - 1u;
              }
              M >>= 1;
            }
          }
          if (occw) atomicOr(&s_cb[c * 32u + wl], occw);
        }
        bad |= __builtin_popcount(M) != pend;  // cannot happen: the replay agrees with the scan
      }
      __builtin_amdgcn_wave_barrier();
    }
    const bool fast = !all_full && __ballot(wide) == 0;
    if (srow && lane == 0) srow[kSsPath] = fast ? 1 : 2;
    if (!fast) {
      // a full parent or a unit wider than 128 slots: the generic replay
      // rewrites every placement and both child bitmaps
      loss = split_slow(s_inf, s_dst, s_cb, s_rep);
    }
    for (int o = 32; o > 0; o >>= 1) loss += (uint32_t)__shfl_down((int)loss, o);
    loss = (uint32_t)__shfl((int)loss, 0);
    bad = __ballot(bad) != 0;
    if (NW > 1 && lane == 0) {
      s_tm[1] = loss;
      if (bad) s_tm[0] |= 2u;
    }
    if (NW == 1) *bad_out = bad;
  }
  stamp(srow, kSsReplayed, lane == 0 && v == 0);
  // every child slot is written exactly once: an entry or INVALID.  Child 0
  // is the parent's storage, so every parent pair is reloaded (L2-hot) into
  // registers before the first store (of any wave of the team); the stores
  // go group by group.
  __asm__ volatile("" ::: "memory");  // no reload hoisted across the replay
  team_barrier();
  ulonglong2 r[G];
#ifndef PMDFC_SPLIT_RELOAD
#define PMDFC_SPLIT_RELOAD 0  // (A/B builds) 1: the reload with plain loads instead of non-temporal ones
#endif
#pragma unroll
  for (int j = 0; j < G; ++j) {
    if constexpr (PMDFC_SPLIT_RELOAD) r[j] = sp[(g0 + j) * 64 + lane];
    else r[j] = ld_pair_l2(sp + (g0 + j) * 64 + lane);
  }
  wait_vmcnt<0>();  // every parent pair is in registers: no store waits below
  if constexpr (NW > 1) {
    team_barrier();  // (another wave's stores may land in my groups)
    loss = s_tm[1];
    *bad_out = (s_tm[0] & 2u) != 0;
  }
  stamp(srow, kSsReloaded, lane == 0 && v == 0);
#pragma unroll
  for (int j = 0; j < G; ++j) {
    const uint32_t slot = (uint32_t)(g0 + j) * 64u + lane;
    const uint32_t d = s_dst[slot];
    if (d != 0xFFFFu) ((d >> 10) ? s1 : sp)[d & 1023u] = r[j];
#pragma unroll
    for (int c = 0; c < 2; ++c)
      if (!((s_cb[c * 32u + (slot >> 5)] >> (slot & 31u)) & 1u)) (c ? s1 : sp)[slot] = make_ulonglong2(kInvalid, 0ULL);
  }
  if (drops && loss) {
    // a valid parent entry with no placement was dropped (rare path)
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const uint32_t slot = (uint32_t)(g0 + j) * 64u + lane;
      if (s_dst[slot] == 0xFFFFu && r[j].x != kInvalid) {
        const uint32_t k = atomicAdd(drop_n, 1u);
        if (k < kDropLog) drops[k] = make_ulonglong2(r[j].x, trig);
      }
    }
  }
  if (v == 0) {
    const uint32_t bw = s_cb[lane];  // lanes 0-31 child-0 words, 32-63 child-1 words
    if (lane < 32) occ[(size_t)seg * 32u + lane] = bw;
    else occ[(size_t)c1 * 32u + (lane - 32)] = bw;
    if (lane == 0) {
      ldep[seg] = (uint8_t)(L + 1);
      ldep[c1] = (uint8_t)(L + 1);
    }
  }
  stamp(srow, kSsStored, lane == 0 && v == 0);  // the stores may still be in flight (callers wait when they re-read)
  if constexpr (NW > 1) team_barrier();  // (the scratch is reused by the team's next split)
  return loss;
}

__device__ __forceinline__ uint32_t wave_split(ulonglong2* __restrict__ pairs, uint32_t* __restrict__ occ,
                                               uint8_t* __restrict__ ldep, uint32_t seg, uint32_t c1, uint32_t L,
                                               uint32_t* scr, bool* bad_out, uint64_t* srow,
                                               ulonglong2* drops = nullptr, uint32_t* drop_n = nullptr,
                                               uint32_t trig = 0) {
  return split_team<1>(pairs, occ, ldep, seg, c1, L, scr, bad_out, srow, drops, drop_n, trig, 0u);
}

}  // namespace pmdfc
