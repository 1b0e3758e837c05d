// apply_fast.h -- the lean first apply pass of an insert-only batch (step 2 of
// a batch's launch sequence, bucket.hip): apply_fast, the device side of
// k_apply_fast and its coarse-partition, wide and last-writer-wins variants
// (the kernels themselves are in bucket.hip; the parallel claims are
// bucket_pass.h fast_claim).
#pragma once
#include "bucket_pass.h"

namespace pmdfc {

// ---------------------------------------------------- lean first apply pass
//
// k_apply_fast: the first pass of an insert-only batch for the common bucket
// -- at most 64 records per sub-region (32 prefetched), no overflow, at most
// kFC inserts, a sub-directory of <= kFastBins entries -- with the parallel
// claims of fast_claim (see there for the rule and why it is exact), in a
// kernel of its own sized for OCCUPANCY: the pass is a chain of dependent
// memory round trips (records + header + fixed sub-directory slot, then each
// insert's two occupancy words, then the claims' stores) with ~6 % VALU busy,
// so its time is waves in flight.  Dense insert slots (the records compacted
// through LDS, kFP per lane), the sub-directory in a register (a shuffle per
// lookup), occupancy words straight from memory and claimed bits OR-ed back
// with global atomics (no bitmap rows in LDS), no key array (the rare
// UNSPLITTABLE check that needs a key claimed in this pass hands the bucket
// back): ~4.9 KB of LDS and no general path in the kernel, so 8 waves per SIMD
// instead of 4.  A bucket it does not take -- or whose claims hit a case
// fast_claim hands back -- is listed (nothing written yet) for k_apply_fb,
// bucket_body's general first pass, launched right after.
// The wide variant (k_apply_wide) takes the buckets of large tables -- a
// sub-directory of up to 128 entries (a 2^28-key table at 2^13 buckets has
// 64-128), read from its fixed slot in the first round trip (two entries
// per lane), at most kFCW inserts -- with the bins of fast_claim assigned
// densely to the segments the bucket's inserts touch (at most 64), and
// fewer insert slots per lane: 6.7 KB of LDS, 6 waves per SIMD.
template <bool WIDE>
struct FastCfg {
  static constexpr int FP = WIDE ? 2 : 3;               // dense insert slots per lane
  static constexpr uint32_t FC = 64u * (uint32_t)FP;    // inserts per bucket on the fast path
  static constexpr uint32_t NB = WIDE ? 64u : kFastBins; // segments (bins) per bucket
  static constexpr uint32_t MaxDb = WIDE ? 7u : 5u;     // sub-directory bits it takes
};

template <bool WIDE>
struct FastLds {
  using C = FastCfg<WIDE>;
  union {
    uint32_t sc[FcLayout<C::FC, C::NB>::Words];  // fast_claim's scratch
    struct {
      ulonglong2 kv[C::FC];
      uint32_t op[C::FC];
    } stage;  // record compaction (before the claims)
  };
  uint32_t seen[4];  // WIDE: the segments (first sub-index) the inserts touch
  uint32_t nsplit, nreq, need;
};

// 0: taken; else a bucket the fast path does not take (nothing written yet):
// 2 for a table-wide reason (sub-directory past MaxDb bits, partition overflow)
// UPS: last-writer-wins (PMDFC_CFG_UPSERT): a bucket with two inserts of one
// key goes to the general pass; otherwise each insert's window is probed for
// its key over the occupied prefix (a stored key lies before the window's
// first free slot: slots are freed only by Erase, which restores that before
// it returns, erase.hip) and a stored key is overwritten.
// The coarse-partition first pass (k_apply_fast_cp): k_part partitions into
// 2^(p1 - 3) buckets, each the records of 8 directory buckets, so a tile's run
// per partition bucket is ~8 records (whole 128-B lines, 1/8 of the reserve
// atomics) instead of ~1; the 8 waves of a workgroup -- one per directory
// bucket -- stage their partition bucket's records in LDS once (coalesced,
// kCpPre per sub-region) and each compacts its own from there.  The staging
// overlays the waves' claim scratch (4 workgroups per CU: 8 waves per SIMD).
constexpr uint32_t kCpWaves = 1u << kCpSbb;
constexpr uint32_t kCpPre = 192;  // records staged per sub-region (mean 128 at 1M ops / 1,024 buckets / 8 sub-regions)
// Staged in two stages: records [0, kCpPre1) of every sub-region before
// anything is known, [kCpPre1, kCpPre) once the sub-region counts have
// arrived and only where the record is live -- at the mean of 128 the second
// stage loads ~4 records per sub-region instead of 64 stale ones.
#ifndef PMDFC_CP_LEAN_STAGE
#define PMDFC_CP_LEAN_STAGE 1  // (A/B builds) 0: all kCpPre records unconditionally
#endif
constexpr uint32_t kCpPre1 = PMDFC_CP_LEAN_STAGE ? 128 : kCpPre;
struct CpLds {
  union {
    FastLds<false> w[kCpWaves];
    struct {
      ulonglong2 kv[kPartSubs * kCpPre];
      uint32_t op[kPartSubs * kCpPre];
      uint16_t idx[kCpWaves][FastCfg<false>::FC];  // each wave's records: staging slots
    } st;
  };
  uint32_t csub[kPartSubs];
};
static_assert(sizeof(CpLds) <= 40 * 1024, "4 workgroups of 8 waves per CU");

// The wide lean pass's bins: bn[j], the first sub-index (< 128) of insert j's
// segment, becomes the rank of that segment among those the bucket's inserts
// touch (seen: 4 LDS words, zeroed).  False: more than nb segments.
__device__ __forceinline__ bool dense_bins(uint32_t* seen, const bool (&pq)[kPer], uint32_t (&bn)[kPer], uint32_t nb) {
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int j = 0; j < kPer; ++j)
    if (pq[j]) atomicOr(&seen[bn[j] >> 5], 1u << (bn[j] & 31u));
  __builtin_amdgcn_wave_barrier();
  const uint32_t s0 = seen[0], s1 = seen[1], s2 = seen[2], s3 = seen[3];
  if (__builtin_popcount(s0) + __builtin_popcount(s1) + __builtin_popcount(s2) + __builtin_popcount(s3) > (int)nb)
    return false;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const uint32_t x = bn[j], q = x >> 5, below = (1u << (x & 31u)) - 1u;
    uint32_t r = __builtin_popcount((q == 0 ? s0 : q == 1 ? s1 : q == 2 ? s2 : s3) & below);
    r += q > 0 ? __builtin_popcount(s0) : 0;
    r += q > 1 ? __builtin_popcount(s1) : 0;
    r += q > 2 ? __builtin_popcount(s2) : 0;
    bn[j] = r;
  }
  return true;
}

// The lean pass in last-writer-wins mode: each insert's window is probed for
// its key over the occupied prefix (a stored key lies before the window's
// first free slot: slots are freed only by Erase, which restores that before
// it returns).  upd[j]: the slot of insert j's key
// (0xFFFF: absent); owin[j]: its window's occupancy bits (window_bits), for
// fast_claim.  False: two inserts of one key, nothing probed (the general
// pass takes the bucket).
__device__ __forceinline__ bool upsert_probe(const BucketArgs& a, const bool (&pq)[kPer], const uint64_t (&rk)[kPer],
                                             const uint32_t (&e8)[kPer], const uint32_t (&home8)[kPer],
                                             uint32_t (&upd)[kPer], uint32_t (&owin)[kPer]) {
  const uint32_t lane = __lane_id() & 63u;
  // two inserts of one key: the general pass (equal keys have equal hashes;
  // a 32-bit hash collision only sends the bucket there too)
  uint32_t hv[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) hv[q] = q < kPer && pq[q] ? (uint32_t)hash64(rk[q]) : 0xFFFFFFFFu;
  wave_sort32<4>(hv, 256);
  bool dup = false;
#pragma unroll
  for (int q = 0; q < 3; ++q) dup |= hv[q] != 0xFFFFFFFFu && hv[q] == hv[q + 1];
  const uint32_t nx = (uint32_t)__shfl_down((int)hv[0], 1);
  dup |= lane < 63u && hv[3] != 0xFFFFFFFFu && hv[3] == nx;
  if (__ballot(dup)) return false;
  // the window's occupancy words, then its occupied prefix, line by line
  // (the loads of all of a lane's inserts in flight together)
  uint32_t nl[kPer];
  WinLd ow[kPer];
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    upd[j] = 0xFFFFu;
    ow[j] = WinLd{};
    if (pq[j]) ow[j] = ld_window_l2(a.occ + (size_t)de_seg(e8[j]) * 32u, home8[j] >> 3);
  }
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const uint32_t win = owin[j] = window_bits(ow[j], home8[j]);
    const uint32_t ff = ~win ? (uint32_t)__builtin_ctz(~win) : 32u;  // first free slot of the window
    nl[j] = pq[j] ? (ff + 3u) >> 2 : 0u;
  }
  for (uint32_t t = 0;; ++t) {
    bool more = false;
#pragma unroll
    for (int j = 0; j < kPer; ++j) more |= t < nl[j] && upd[j] == 0xFFFFu;
    if (!__ballot(more)) break;
    uint64_t kq[kPer][4];
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      if (t >= nl[j] || upd[j] != 0xFFFFu) continue;
      const ulonglong2* ln = a.pairs + (size_t)de_seg(e8[j]) * kSlots + ((home8[j] + t) & 255u) * 4u;
#pragma unroll
      for (int q = 0; q < 4; ++q) kq[j][q] = reinterpret_cast<const uint64_t*>(ln + q)[0];
    }
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      if (t >= nl[j] || upd[j] != 0xFFFFu) continue;
#pragma unroll
      for (int q = 3; q >= 0; --q)
        if (kq[j][q] == rk[j]) upd[j] = ((home8[j] + t) * 4u + (uint32_t)q) & (kSlots - 1);
    }
  }
  return true;
}

template <bool WIDE, bool UPS = false, bool CP = false>
__device__ __forceinline__ uint32_t apply_fast(const BucketArgs& a, FastLds<WIDE>& S, uint32_t w,
                                               CpLds* cpl = nullptr) {
  using C = FastCfg<WIDE>;
  static_assert(!CP || (!WIDE && !UPS), "the coarse-partition pass is the lean insert-only one");
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t pb = w >> a.sbb, sub = w & ((1u << a.sbb) - 1);
  uint64_t* const srow = bucket_stamp_row(a, w);
  stamp(srow, kBsStart, lane == 0);
  first_pass_clears(a, w);
  // one round trip: the first 32 records of each sub-region, the counts, the
  // header, the stat slots, the overflow count and the fixed sub-directory slot
  PreRecs pr;
  constexpr int kCpLd = (int)(kPartSubs * kCpPre / (64 * kCpWaves));  // staging loads per thread
  constexpr int kCpLd1 = (int)(kPartSubs * kCpPre1 / (64 * kCpWaves));  // those of the first stage
  static_assert(kCpLd <= kPre, "the staging loads use the prefetch registers");
  static_assert(kCpLd1 * 64 * kCpWaves == kPartSubs * kCpPre1 && (kCpLd - kCpLd1) * 64 * kCpWaves == kPartSubs * (kCpPre - kCpPre1),
                "whole loads per stage");
  // staging slot (sub-region * kCpPre + record) of this thread's load u: the
  // first stage covers records [0, kCpPre1) of every sub-region, the second
  // [kCpPre1, kCpPre) -- wave v those of sub-region v, one per lane
  const auto cp_slot = [&](int u) -> uint32_t {
    const uint32_t t = (uint32_t)u * 64u * kCpWaves + threadIdx.x;
    if (u < kCpLd1) return (t / kCpPre1) * kCpPre + t % kCpPre1;
    const uint32_t r = t - kPartSubs * kCpPre1;
    return (r / (kCpPre - kCpPre1)) * kCpPre + kCpPre1 + r % (kCpPre - kCpPre1);
  };
  const auto cp_load = [&](int u) {
    const uint32_t s = cp_slot(u);
    const uint64_t j = (uint64_t)pb * a.cap + (uint64_t)(s / kCpPre) * a.capx + min(s % kCpPre, a.capx - 1u);
    pr.op[u] = a.rop[j];
    const ulonglong2 kv = a.rkv[j];
    pr.k[u] = kv.x;
    pr.v[u] = kv.y;
  };
  // (the counts and the other small loads first, the records after them:
  // loads are waited for in issue order, so the second staging stage waits
  // for the counts with the records still in flight)
  const uint64_t wsv = lane < 7u ? a.wstat[(size_t)w * kWStat + lane] : 0ULL;
  const uint32_t* fslot = a.pool + (size_t)w * kFixedSlot;
  const uint32_t spec0 = (a.pfix && (WIDE || lane < 32u)) ? ld_u32_l2(fslot + lane) : 0u;
  const uint32_t spec1 = (WIDE && a.pfix) ? ld_u32_l2(fslot + 64u + lane) : 0u;
  uint64_t hd = a.hdr[w];
  uint32_t novf = *a.ovf;
  uint32_t craw = sub_count_issue(a, pb);
  if constexpr (CP) {
    // the workgroup stages its partition bucket's records; a wave's loads
    // land below.  First stage: unconditional, before anything is known
#pragma unroll
    for (int u = 0; u < kCpLd1; ++u) cp_load(u);
    // (the empty asm statements pin the first use of a small load's value --
    // its wait -- behind the loads above it: the counts' here, the header's
    // and the overflow count's after the second stage)
    asm volatile("" : "+v"(craw));
  } else {
    prefetch_records(a, pb, 0, pr);
  }
  const uint32_t csub = min(craw, a.capx);
  // second staging stage: the counts have arrived, the first stage is in flight
  bool live2 = false;
  if constexpr (CP && kCpLd1 < kCpLd) {
    static_assert(kCpLd - kCpLd1 == 1 && kCpPre - kCpPre1 == 64, "wave v loads the second stage of sub-region v");
    const uint32_t cv = (uint32_t)__builtin_amdgcn_readlane((int)csub, (int)(w & (kCpWaves - 1)));
    live2 = kCpPre1 + lane < cv;
    if (live2) cp_load(kCpLd1);
  }
  if constexpr (CP) {
    uint32_t hl = (uint32_t)hd, hh = (uint32_t)(hd >> 32);
    asm volatile("" : "+v"(hl), "+v"(hh), "+v"(novf));
    hd = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)hh) << 32 | (uint32_t)__builtin_amdgcn_readfirstlane((int)hl);
    novf = (uint32_t)__builtin_amdgcn_readfirstlane((int)novf);
  }
  const uint32_t off = hdr_off(hd), db = hdr_db(hd);
  // the sub-directory, one (two) entries per lane (else loads that wait for the header)
  const bool fixed = a.pfix && off == w * kFixedSlot && db <= kFixedBits;
  uint32_t dv0, dv1 = 0u;
  if (fixed) {
    dv0 = lane < (1u << db) ? spec0 : 0u;
    dv1 = lane + 64u < (1u << db) ? spec1 : 0u;
  } else {
    dv0 = (db <= C::MaxDb && lane < (1u << db)) ? ld_u32_l2(a.pool + off + lane) : 0u;
    if (WIDE) dv1 = (db <= C::MaxDb && lane + 64u < (1u << db)) ? ld_u32_l2(a.pool + off + 64u + lane) : 0u;
  }
  const uint32_t cmax = sub_count_max(csub);
  bool pq[kPer];
  uint64_t rk[kPer], rv[kPer];
  uint32_t rop[kPer];
  if constexpr (CP) {
    // staged records -> LDS; then each wave lists its own (sub-bucket == its
    // bucket) and takes them into insert slots j * 64 + lane; the two
    // workgroup barriers are reached by every wave, declining or not
#pragma unroll
    for (int u = 0; u < kCpLd; ++u) {
      if (u >= kCpLd1 && !live2) continue;  // (a slot nobody wrote is never listed)
      const uint32_t t = cp_slot(u);
      cpl->st.op[t] = pr.op[u];
      cpl->st.kv[t] = make_ulonglong2(pr.k[u], pr.v[u]);
    }
    __syncthreads();
    uint32_t dec = (db > C::MaxDb || novf != 0) ? 2u : cmax > kCpPre ? 2u : 0u;
    uint32_t m = 0;
    if (!dec) {
      const uint64_t lt = (1ULL << lane) - 1;
      const uint32_t v = w & (kCpWaves - 1);
      uint16_t* my = cpl->st.idx[v];
      // sub-region by sub-region, its live records only (cs <= kCpPre here)
      for (uint32_t xs = 0; xs < kPartSubs; ++xs) {
        const uint32_t cs = (uint32_t)__builtin_amdgcn_readlane((int)csub, (int)xs);
        uint32_t r[kCpPre / 64];
#pragma unroll
        for (uint32_t q = 0; q < kCpPre / 64; ++q) {
          const uint32_t i = q * 64u + lane;
          r[q] = i < cs ? cpl->st.op[xs * kCpPre + i] : ~0u;
        }
#pragma unroll
        for (uint32_t q = 0; q < kCpPre / 64; ++q) {
          if (q * 64u >= cs) break;
          const uint32_t i = q * 64u + lane;
          const bool match = i < cs && ((r[q] >> 22) & (kCpWaves - 1)) == v;
          const uint64_t bal = __ballot(match);
          const uint32_t idx = m + (uint32_t)__popcll(bal & lt);
          if (match && idx < C::FC) my[idx] = (uint16_t)(xs * kCpPre + i);
          m += (uint32_t)__popcll(bal);
        }
      }
      if (m > C::FC) dec = 1u;
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int j = 0; j < kPer; ++j) {
        const uint32_t i = (uint32_t)j * 64u + lane;
        pq[j] = !dec && j < C::FP && i < m;
        rk[j] = rv[j] = 0;
        rop[j] = 0;
        if (pq[j]) {
          const uint32_t t = my[i];
          const ulonglong2 kv = cpl->st.kv[t];
          rk[j] = kv.x;
          rv[j] = kv.y;
          rop[j] = cpl->st.op[t];
        }
      }
    }
    __syncthreads();  // (the staging is dead: the waves' claim scratch overlays it)
    if (dec) return dec;
  } else {
    if (db > C::MaxDb || novf != 0) return 2u;
    if (cmax > C::FC) return 1u;
    // compact the bucket's records into insert slots j * 64 + lane, j < FP
    // (in sub-region order: records 0-31 of every sub-region, then 32-63 of
    // those with more, ... -- k_part's sub-regions are ~Poisson(16) at config 2,
    // so ~10 buckets a batch take the second load; a batch of fewer than
    // kPartSubs partition tiles fills fewer sub-regions, more deeply.  The order
    // of the slots does not matter, the claims are decided by op index)
    uint32_t m = 0;
    for (uint32_t half = 0; half * 32u < cmax; ++half) {
      if (half) prefetch_records(a, pb, half, pr);
      m = compact_prefetched(a, pr, half, csub, sub, m, S.stage.kv, S.stage.op, C::FC);
    }
    if (m > C::FC) return 1u;
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const uint32_t i = (uint32_t)j * 64u + lane;
      pq[j] = j < C::FP && i < m;
      rk[j] = rv[j] = 0;
      rop[j] = 0;
      if (pq[j]) {
        const ulonglong2 kv = S.stage.kv[i];
        rk[j] = kv.x;
        rv[j] = kv.y;
        rop[j] = S.stage.op[i];
      }
    }
    __builtin_amdgcn_wave_barrier();  // (staging is dead: the claims' scratch overlays it)
  }
  if (lane == 0) {
    S.nsplit = 0;
    S.nreq = 0;
    S.need = db;
  }
  if (WIDE && lane < 4) S.seen[lane] = 0;
  uint32_t e8[kPer], home8[kPer], x8[kPer], bn[WIDE ? kPer : 1];
  (void)bn;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    home8[j] = x8[j] = 0;
    if (pq[j]) {
      const uint64_t h = hash64(rk[j]);
      home8[j] = (uint32_t)(h & 0xFF);
      x8[j] = sub_index(h, a.sbits, a.p1, db);
    }
    // (every lane: a shuffle reads active lanes only)
    const uint32_t lo = (uint32_t)__shfl((int)dv0, (int)(x8[j] & 63u));
    if (WIDE) {
      const uint32_t hi = (uint32_t)__shfl((int)dv1, (int)(x8[j] & 63u));
      e8[j] = x8[j] < 64u ? lo : hi;
    } else {
      e8[j] = lo;
    }
  }
  // bin: the segment's first sub-index; WIDE: the touched segments numbered
  // densely in sub-index order
  const auto first_sub = [&](int j) -> uint32_t { return first_sub_index(a, db, x8[j], e8[j]); };
  if constexpr (WIDE) {
#pragma unroll
    for (int j = 0; j < kPer; ++j) bn[j] = pq[j] ? first_sub(j) : 0u;
    if (!dense_bins(S.seen, pq, bn, C::NB)) return 1u;  // (nothing written yet)
  }
  uint32_t upd[UPS ? kPer : 1], owin[UPS ? kPer : 1];
  if constexpr (UPS) {
    if (!upsert_probe(a, pq, rk, e8, home8, upd, owin)) return 1u;  // two inserts of one key
  }
  stamp(srow, kBsLoaded, lane == 0);
  WaveStat c;
  const auto bin = [&](int j) -> uint32_t {
    if constexpr (WIDE) return bn[j];
    else return first_sub(j);
  };
  if (!fast_claim<C::FC, C::NB, UPS>(a, w, S.sc, nullptr, a.wl_kv + (size_t)w * kCW, a.wl_op + (size_t)w * kCW,
                                     &S.nsplit, &S.nreq, &S.need, LaneOps{rk, rv, rop, pq, e8, home8, x8}, bin, c, srow,
                                     UPS ? upd : nullptr, UPS ? owin : nullptr))
    return 1u;
  if (lane == 0) a.wl_n[w] = S.nsplit;  // parked inserts (0: done)
  request_tail(a, w, S.nreq, S.need, db);
  c.rounds = c.max_rounds = 1;
  publish_stats(a, w, wsv, c);
  stamp(srow, kBsEnd, lane == 0);
  return 0u;
}

// a bucket the lean pass declined (nothing written): flagged for k_apply_fb,
// or, when none is launched, for k_apply_parked (anydecl: every decliner
// stores the same word, no read-modify-write)
__device__ __forceinline__ void declined(const BucketArgs& a, uint32_t w) {
  a.fbl[w] |= 1u;
  a.ctl->anydecl[a.par] = 1u;
}

}  // namespace pmdfc
