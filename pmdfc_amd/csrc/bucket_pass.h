// bucket_pass.h -- one wave's pass over one directory bucket, for the kernels
// that run one (bucket.hip) and for the lean first pass (apply_fast.h).
//
// bucket_body is the outline of a bucket pass over named phases ("the phases
// of a bucket pass": chunk loaders, entry lookup, the two orderings into
// runs, apply_runs, the claim write-outs, parking, grow_and_split); what the
// first passes share with the lean apply_fast exists once ("what every first
// pass of a batch does"), and so do the parallel claims of the insert-only
// passes (fast_claim: it takes the pass's WaveStat, bitmap rows and stamp
// slots, and bucket_body calls it, so it lives between them).
#pragma once
#include <cstddef>

#include "split_device.h"

namespace pmdfc {

constexpr int kBmLanes = 30;          // lanes with an LDS occupancy bitmap at a time (LDS: 4 waves/SIMD)
constexpr int kRoundGuard = 64;

// k_bucket sort key: [segment:25 @39][op index:22 @17][chunk slot:9 @8][home line:8 @0].
// Ordering is (segment, batch index); the home line rides along so the
// per-run loop needs neither the key nor a hash.
__device__ __forceinline__ uint64_t sk_make(uint32_t seg, uint32_t op, uint32_t i, uint32_t home) {
  return ((uint64_t)seg << 39) | ((uint64_t)op << 17) | ((uint64_t)i << 8) | home;
}
__device__ __forceinline__ uint32_t sk_seg(uint64_t k) { return (uint32_t)(k >> 39); }
__device__ __forceinline__ uint32_t sk_op(uint64_t k) { return (uint32_t)(k >> 17) & kOpMask; }
__device__ __forceinline__ uint32_t sk_item(uint64_t k) { return (uint32_t)(k >> 8) & 511u; }
__device__ __forceinline__ uint32_t sk_home(uint64_t k) { return (uint32_t)k & 0xFFu; }

// ------------------------------------------------------------------ bucket

// a bucket wave's stamp row (debug stamps: wave_util.h), or null
__device__ __forceinline__ uint64_t* bucket_stamp_row(const BucketArgs& a, uint32_t w) {
  return a.stamps ? a.stamps + (size_t)w * 16 : nullptr;
}

constexpr uint32_t kBmWords = kBmLanes * 33;
constexpr uint32_t kUnionWords = kBmWords > kSplitScratch ? kBmWords : kSplitScratch;

// Collect this wave's ops of the batch into LDS (records of its region, read
// coalesced, then its records in the overflow area).  Stores up to kCW;
// returns how many matched.
__device__ __forceinline__ uint32_t collect(const BucketArgs& a, uint32_t pb, uint32_t sub,
                                            uint32_t csub, uint32_t novf, ulonglong2* s_kv,
                                            uint32_t* s_op) {
  const uint32_t lane = __lane_id() & 63u;
  const uint64_t lt = (1ULL << lane) - 1;
  const uint32_t sbm = (1u << a.sbb) - 1;
  uint32_t m = 0;
  for (uint32_t xs = 0; xs < kPartSubs; ++xs) {  // csub: lane xs holds sub-region xs's count
  const uint32_t cnt = (uint32_t)__shfl((int)csub, (int)xs);
  const uint64_t rb = (uint64_t)pb * a.cap + (uint64_t)xs * a.capx;
  for (uint32_t j0 = 0; j0 < cnt; j0 += 128) {
    // plain scalars, all loads issued before any use (a conditionally set
    // ulonglong2[] lands in scratch memory and serializes the loads)
    uint32_t r[2];
    uint64_t kx[2], vx[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const uint32_t j = min(j0 + u * 64 + lane, cnt - 1);
      r[u] = a.rop[rb + j];
      const ulonglong2 kv = a.rkv[rb + j];
      kx[u] = kv.x;
      vx[u] = kv.y;
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const uint32_t j = j0 + u * 64 + lane;
      const bool match = j < cnt && ((r[u] >> 22) & sbm) == sub;
      const uint64_t bal = __ballot(match);
      const uint32_t idx = m + (uint32_t)__popcll(bal & lt);
      if (match && idx < (uint32_t)kCW) {
        s_kv[idx] = make_ulonglong2(kx[u], vx[u]);
        s_op[idx] = r[u];
      }
      m += (uint32_t)__popcll(bal);
    }
  }
  }
  for (uint32_t j0 = 0; j0 < novf; j0 += 64) {
    const uint32_t j = j0 + lane;
    bool match = false;
    uint32_t r = 0;
    if (j < novf && a.robk[j] == pb) {
      r = a.rop[a.ovf_base + j];
      match = ((r >> 22) & sbm) == sub;
    }
    const uint64_t bal = __ballot(match);
    const uint32_t idx = m + (uint32_t)__popcll(bal & lt);
    if (match && idx < (uint32_t)kCW) {
      s_kv[idx] = a.rkv[a.ovf_base + j];
      s_op[idx] = r;
    }
    m += (uint32_t)__popcll(bal);
  }
  __builtin_amdgcn_wave_barrier();
  return m;
}

// ---- big buckets (final pass): more ops than one chunk.  Chunks must follow
// batch order (per segment), and k_part wrote each (tile, bucket) as ONE
// contiguous run in the region plus at most one in the overflow area, where a
// tile is kPartTile consecutive ops.  So one scan finds every tile's runs, and
// the chunks walk the tiles in order: whole tiles while they fit, and a tile
// larger than a chunk through a map of its ops by in-tile index.  Linear in
// the bucket's records.
struct BigLds {
  uint32_t rs[kMaxPartBlocks], re[kMaxPartBlocks];  // region run of each tile
  uint32_t os[kMaxPartBlocks], oe[kMaxPartBlocks];  // overflow run of each tile
  uint16_t map[kPartTile];                          // in-tile op -> record of the tile
};
__device__ __forceinline__ BigLds* big_lds() {
  __shared__ BigLds s;
  return &s;
}

__device__ __forceinline__ uint32_t tile_of(uint32_t rop) { return (rop & kOpMask) / kPartTile; }

__device__ inline void big_index(const BucketArgs& a, BigLds* L, uint32_t pb, uint32_t csub, uint32_t novf,
                          uint32_t ntile) {
  const uint32_t lane = __lane_id() & 63u;
  for (uint32_t t = lane; t < ntile; t += 64) L->rs[t] = L->re[t] = L->os[t] = L->oe[t] = 0;
  __builtin_amdgcn_wave_barrier();
  // tile t's region run lies in sub-region t % kPartSubs (k_part block t);
  // rs/re are offsets inside that sub-region
  for (uint32_t xs = 0; xs < kPartSubs; ++xs) {
    const uint32_t cnt = (uint32_t)__shfl((int)csub, (int)xs);
    const uint64_t rb = (uint64_t)pb * a.cap + (uint64_t)xs * a.capx;
    for (uint32_t j = lane; j < cnt; j += 64) {
      const uint32_t t = tile_of(a.rop[rb + j]);
      if (j == 0 || tile_of(a.rop[rb + j - 1]) != t) L->rs[t] = j;
      if (j + 1 == cnt || tile_of(a.rop[rb + j + 1]) != t) L->re[t] = j + 1;
    }
  }
  for (uint32_t j = lane; j < novf; j += 64) {
    if (a.robk[j] != pb) continue;
    const uint32_t t = tile_of(a.rop[a.ovf_base + j]);
    if (j == 0 || a.robk[j - 1] != pb || tile_of(a.rop[a.ovf_base + j - 1]) != t) L->os[t] = j;
    if (j + 1 == novf || a.robk[j + 1] != pb || tile_of(a.rop[a.ovf_base + j + 1]) != t) L->oe[t] = j + 1;
  }
  __builtin_amdgcn_wave_barrier();
}

// record slot of entry k of tile t's runs (region first, then overflow)
__device__ __forceinline__ uint64_t big_rec(const BucketArgs& a, const BigLds* L, uint64_t rb, uint32_t t,
                                            uint32_t k) {
  const uint32_t rl = L->re[t] - L->rs[t];
  return k < rl ? rb + (uint64_t)(t % kPartSubs) * a.capx + L->rs[t] + k : a.ovf_base + L->os[t] + (k - rl);
}

// Next chunk of a big bucket into s_kv/s_op: ops of tiles [t, ...) in batch
// order, at most C.  (t, mp) is the walk position (mp > 0: inside tile t's map).
__device__ inline uint32_t big_chunk(const BucketArgs& a, BigLds* L, uint32_t pb, uint32_t sub, uint32_t ntile,
                              uint32_t C, uint32_t& t, uint32_t& mp, ulonglong2* s_kv, uint32_t* s_op) {
  const uint32_t lane = __lane_id() & 63u;
  const uint64_t lt = (1ULL << lane) - 1;
  const uint32_t sbm = (1u << a.sbb) - 1;
  const uint64_t rb = (uint64_t)pb * a.cap;
  uint32_t m = 0;
  while (t < ntile) {
    const uint32_t ct = (L->re[t] - L->rs[t]) + (L->oe[t] - L->os[t]);
    if (ct == 0) {
      ++t;
      continue;
    }
    if (mp == 0 && m + ct <= C) {  // the whole tile joins the chunk
      for (uint32_t k0 = 0; k0 < ct; k0 += 64) {
        const uint32_t k = k0 + lane;
        bool match = false;
        uint64_t rs = 0;
        uint32_t r = 0;
        if (k < ct) {
          rs = big_rec(a, L, rb, t, k);
          r = a.rop[rs];
          match = ((r >> 22) & sbm) == sub;
        }
        const uint64_t bal = __ballot(match);
        const uint32_t idx = m + (uint32_t)__popcll(bal & lt);
        if (match) {
          s_kv[idx] = a.rkv[rs];
          s_op[idx] = r;
        }
        m += (uint32_t)__popcll(bal);
      }
      ++t;
      continue;
    }
    if (mp == 0 && m > 0) break;  // a big tile starts its own chunk
    if (mp == 0) {
      for (uint32_t k = lane; k < kPartTile; k += 64) L->map[k] = 0xFFFF;
      __builtin_amdgcn_wave_barrier();
      for (uint32_t k = lane; k < ct; k += 64) {
        const uint32_t r = a.rop[big_rec(a, L, rb, t, k)];
        if (((r >> 22) & sbm) == sub) L->map[(r & kOpMask) % kPartTile] = (uint16_t)k;
      }
      __builtin_amdgcn_wave_barrier();
    }
    // walk the map from mp, taking ops in batch order until the chunk is full
    while (mp < kPartTile && m < C) {
      const uint32_t e = mp + lane < kPartTile ? L->map[mp + lane] : 0xFFFFu;
      const bool v = e != 0xFFFFu;
      const uint64_t bal = __ballot(v);
      const uint32_t room = C - m, nv = (uint32_t)__popcll(bal);
      const uint32_t idx = (uint32_t)__popcll(bal & lt);
      if (v && idx < room) {
        const uint64_t rs = big_rec(a, L, rb, t, e);
        s_kv[m + idx] = a.rkv[rs];
        s_op[m + idx] = a.rop[rs];
      }
      if (nv > room) {
        // stop just past the room-th valid entry of this group
        uint64_t b = bal;
        for (uint32_t q = 0; q + 1 < room; ++q) b &= b - 1;
        mp += (uint32_t)__builtin_ctzll(b) + 1;
        m = C;
      } else {
        mp += 64;
        m += nv;
      }
    }
    if (mp >= kPartTile) {  // tile done (its tail may hold no op of ours)
      mp = 0;
      ++t;
    }
    if (m >= C) break;  // else room is left: go on with the next tiles
  }
  __builtin_amdgcn_wave_barrier();
  return m;
}

// The rare full-window path of a run (out of line: keeps the run loop's
// registers small).  The window may hold the run's deferred inserts: write
// those out first (the store pass writes them again, identically), then test
// whether all 32 window entries carry the new key's full hash.
__device__ inline __noinline__ bool window_all_same(uint32_t mixed, ulonglong2* sp, const uint64_t* s_sk,
                                             const uint16_t* s_pos, const ulonglong2* s_kv,
                                             uint32_t q0, uint32_t q, uint32_t i, uint32_t w0) {
  if (!mixed) {
    for (uint32_t qq = q0; qq < q; ++qq) {
      const uint32_t i2 = sk_item(s_sk[qq]);
      const uint32_t p2 = s_pos[i2];
      if (p2 != 0xFFFFu) sp[p2] = s_kv[i2];
    }
    __builtin_amdgcn_s_waitcnt(0);
  }
  const uint64_t h = hash64(s_kv[i].x);
  for (uint32_t t0 = 0; t0 < kWindow; t0 += 4) {
    ulonglong2 w4[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) w4[t] = ld_pair_l2(sp + ((w0 + t0 + t) & (kSlots - 1)));
    bool same = true;
#pragma unroll
    for (int t = 0; t < 4; ++t) same = same && hash64(w4[t].x) == h;
    if (!same) return false;
  }
  return true;
}

// The same test for the insert-only apply passes, whose pairs live in
// registers until the store pass: a window slot claimed by an earlier op of
// the run holds that op's key (s_pos / s_key), any other slot its key in
// memory.
__device__ inline __noinline__ bool window_all_same_reg(const ulonglong2* sp, const uint64_t* s_sk, const uint16_t* s_pos,
                                                 const uint64_t* s_key, uint32_t q0, uint32_t q, uint32_t i,
                                                 uint32_t w0) {
  const uint64_t h = hash64(s_key[i]);
  for (uint32_t t = 0; t < kWindow; ++t) {
    const uint32_t slot = (w0 + t) & (kSlots - 1);
    bool claimed = false;
    uint64_t k = kInvalid;
    for (uint32_t qq = q0; qq < q; ++qq) {
      const uint32_t i2 = sk_item(s_sk[qq]);
      if (s_pos[i2] == slot) {
        k = s_key[i2];
        claimed = true;
      }
    }
    if (!claimed) k = ld_pair_l2(sp + slot).x;
    if (hash64(k) != h) return false;
  }
  return true;
}

constexpr uint32_t kBigBucket = 0xFFFFFFFFu;  // wl_n of a bucket with more ops than a chunk: the final pass walks its records
constexpr uint32_t kLdsDir = 128;  // k_apply: sub-directories up to this size are read into LDS

// LDS of one bucket wave; the apply pass (no splits) carries no split state,
// which keeps its footprint, and so its occupancy, lower.
template <bool FINAL, bool REG>
struct BucketLds {
  uint32_t u[FINAL ? kUnionWords : kBmWords];  // run phase: per-lane bitmaps; split phase: scratch
  uint64_t sk[kCW];       // sort keys of the pending ops
  ulonglong2 kv[REG ? 1 : kCW];   // {key, value} of each chunk slot (REG: in registers)
  uint64_t key[REG ? kCW : 1];    // REG: the key of each chunk slot
  uint32_t op[REG ? 1 : kCW];     // rop word of each chunk slot (REG: in registers)
  uint16_t pos[kCW];      // insert-only: slot claimed this round, 0xFFFF none
  uint16_t runq[kCW + 1];
  uint8_t L[kCW];         // local depth of the op's segment | Get << 7
  uint8_t pend[kCW];
  uint64_t split[FINAL ? kSplitCap : 1];
  uint32_t dir[FINAL ? 1 : kLdsDir];           // apply pass: the bucket's sub-directory
  uint32_t nsplit, nreq, need;
};
// the REG collect path stages kCW {key, value} pairs across u and sk
using BucketLdsReg = BucketLds<false, true>;
static_assert(offsetof(BucketLdsReg, sk) == sizeof(uint32_t) * kBmWords &&
                  sizeof(uint32_t) * kBmWords + sizeof(uint64_t) * kCW >= sizeof(ulonglong2) * kCW,
              "REG collect staging spans u and sk");

// The per-wave counters of a bucket pass, added to the bucket's stat slots by
// publish_stats (lines and waited are per lane, the others wave-uniform).
struct WaveStat {
  uint32_t lines = 0, waited = 0, splits = 0, loss = 0, runs = 0, rounds = 0;
  uint32_t max_rounds = 0, max_ld = 0, grow = 0, bad = 0;
};

struct RunCtx {  // what one run needs (passed by value: no kernarg copies)
  ulonglong2* pairs;
  uint32_t* occ;
  uint64_t* vout;
  uint8_t* st;
  DevCtl* ctl;
  uint2* req;       // this bucket's split requests (k_apply)
  uint32_t* reqop;  // ... their inserts' batch positions
  uint32_t mixed, max_segments, full, noreq;
  uint64_t* stamp;  // debug: this wave's stamp row (first apply pass), or null
  uint32_t sbits, p1, db;  // geometry of the request's sub-index
  uint32_t upsert;  // last-writer-wins Insert
  const uint16_t* upos;  // upsert, first apply pass: pre-batch key slots by op index, else null
  ulonglong2* wl_kv;  // this bucket's wait list (k_apply parks the rest of a blocked run there)
  uint32_t* wl_op;
  uint32_t pfix, pool_cap;  // final pass: where the sub-directory grows, and the pool's end
};

// Upsert (last-writer-wins, CCEH_hybrid.cpp:153's overwrite clause enabled):
// the slot of `key` in its window if the key is stored there, else -1.  The
// probe walks the occupied prefix of the window (the bitmap marks claims of
// this run too; their slots still read INVALID in memory, which never
// matches), one 64-B line at a time with its 4 pairs loaded together.  No
// stored entry sits past the window's first free slot (slots are
// freed only by Erase, which restores that before it returns, erase.hip), so
// the first free slot ends the probe, as in the reference's claim order.
__device__ __forceinline__ int upsert_find(const ulonglong2* sp, const uint32_t* bm, uint32_t wi0, uint64_t key) {
  for (uint32_t l = 0; l < kLines; ++l) {
    const uint32_t s0 = (wi0 + 4u * l) & (kSlots - 1);  // line aligned: its 4 bits share a word
    const uint32_t occ4 = (bm[s0 >> 5] >> (s0 & 31u)) & 0xFu;
    if (occ4 == 0) return -1;
    ulonglong2 p4[4];
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) p4[q] = ld_pair_l2(sp + s0 + q);
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
      if (!((occ4 >> q) & 1u)) return -1;
      if (p4[q].x == key) return (int)(s0 + q);
    }
  }
  return -1;
}

// a segment's occupancy bitmap, loaded as 8 x uint4, into its 33-word LDS row
__device__ __forceinline__ void put_bitmap_row(uint32_t* row, const uint4 (&v)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    row[4 * j] = v[j].x;
    row[4 * j + 1] = v[j].y;
    row[4 * j + 2] = v[j].z;
    row[4 * j + 3] = v[j].w;
  }
}

// the key of chunk slot i (REG: the insert-only apply passes keep the pairs in
// registers; the runs see the keys only)
template <bool REG, class Lds>
__device__ __forceinline__ uint64_t chunk_key(const Lds& S, uint32_t i) {
  if constexpr (REG) return S.key[i];
  else return S.kv[i].x;
}

// Upsert: the slot that already belongs to `key` as op q of the run [q0, ..)
// comes to it, or -1 -- a claim of this run not yet stored (insert-only
// batches store after the run loop; the earlier claim is dropped, this op
// writes the slot; S.pos keeps the slot each op of the round took in mixed
// batches too), else the key's slot in memory (first pass: the pre-batch
// probe a.upos, no split of this batch having run yet).
template <bool REG, class Lds>
__device__ __forceinline__ int upsert_slot(const RunCtx& a, Lds& S, const ulonglong2* sp, const uint32_t* bm,
                                           uint32_t q0, uint32_t q, uint64_t key, uint32_t op, uint32_t wi0) {
  int upos = -1;
  for (uint32_t qq = q0; qq < q; ++qq) {
    const uint32_t i2 = sk_item(S.sk[qq]);
    if (S.pos[i2] != 0xFFFFu && chunk_key<REG>(S, i2) == key) {
      upos = S.pos[i2];
      S.pos[i2] = 0xFFFF;
    }
  }
  if (upos >= 0) return upos;
  if (!a.upos) return upsert_find(sp, bm, wi0, key);
  const uint32_t u = a.upos[op];
  return u == 0xFFFFu ? -1 : (int)u;
}

// The apply passes' common case: a wave-uniform loop (exit by ballot) with a
// branch-free body that only claims slots (S.pos, the bitmap row bm).  It
// stops a lane at its first full window -- or, in a mixed batch, at its first
// Get -- where apply_run's general loop takes over (go = false, upsert
// batches: from the start, since an insert first looks for its key).
// Returns the first op it did not take; adds the lines its claims probed.
template <bool MIXED, class Lds>
__device__ __forceinline__ uint32_t claim_loop(Lds& S, uint32_t* bm, uint32_t q0, uint32_t q1, bool go,
                                               uint32_t& lines) {
  uint32_t qs = q0;
  uint64_t skn = S.sk[q0];
  for (uint32_t q = q0;; ++q) {
    const bool act = go && q < q1;
    if (__ballot(act) == 0) break;
    if (act) {
      const uint64_t skq = skn;
      skn = S.sk[min(q + 1u, (uint32_t)kCW - 1u)];  // read ahead
      const uint32_t wi0 = sk_home(skq) * 4u;
      const uint32_t wi = wi0 >> 5, wn = (wi + 1u) & 31u;
      const uint32_t lo = bm[wi], hi = bm[wn];
      const uint32_t fr = ~__builtin_amdgcn_alignbit(hi, lo, wi0 & 31u);
      bool ok = fr != 0;
      if constexpr (MIXED) ok = ok && !(S.L[sk_item(skq)] & 0x80u);  // a Get: the general loop
      const uint32_t t = (uint32_t)__builtin_ctz(fr | (ok ? 0u : 1u));
      const uint32_t b = ok ? 1u << ((wi0 + t) & 31u) : 0u;
      const bool in_lo = (wi0 & 31u) + t < 32u;
      bm[wi] = lo | (in_lo ? b : 0u);  // both words written: no divergent branch
      bm[wn] = hi | (in_lo ? 0u : b);
      if (ok) S.pos[sk_item(skq)] = (uint16_t)((wi0 + t) & (kSlots - 1));
      lines += ok ? (t >> 2) + 1 : 0u;
      qs = ok ? q + 1 : qs;
      go = ok;
    }
  }
  return qs;
}

// One segment run (ops q0..q1 of the sorted chunk, one segment), by one lane,
// against an LDS copy of the segment's occupancy bitmap.  A full window stops
// the run: k_apply requests a split (granted at the end of the pass, done by
// k_split) and parks the rest of the run; the final pass splits inline.
template <bool FINAL, bool MIXED>
__device__ __forceinline__ uint2 apply_run(RunCtx a, BucketLds<FINAL, !FINAL && !MIXED>& S, uint32_t q0, uint32_t q1,
                                           bool pre) {
  constexpr bool REG = !FINAL && !MIXED;
  const uint32_t lbase = a.sbits + a.p1;
  uint32_t* const bm = S.u + ((__lane_id() & 63u) % kBmLanes) * 33u;  // this lane's bitmap row
  uint32_t lines = 0, waited = 0;
  const uint64_t sk0 = S.sk[q0];
  const uint32_t seg = sk_seg(sk0);
  const uint32_t L = S.L[sk_item(sk0)] & 31u;
  if (!pre) {  // (the apply pass prefetches the bitmaps of its first kBmLanes runs)
    const uint32_t* og = a.occ + (size_t)seg * 32u;
    uint4 bv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) bv[j] = ld_u4_l2(og + 4 * j);
    put_bitmap_row(bm, bv);
  }
  ulonglong2* sp = a.pairs + (size_t)seg * kSlots;
  bool dirty = false;
  uint32_t qs = q0;
  if constexpr (!FINAL) {
    qs = claim_loop<MIXED>(S, bm, q0, q1, !a.upsert, lines);
    dirty = qs > q0;
    if constexpr (MIXED) {
      // the general loop goes on (a Get, or a full window it inspects): it
      // reads the segment, so the claims made so far are stored first
      if (qs > q0 && qs < q1) {
        for (uint32_t qq = q0; qq < qs; ++qq) {
          const uint64_t sk = S.sk[qq];
          const uint32_t i2 = sk_item(sk);
          sp[S.pos[i2]] = S.kv[i2];
          a.st[sk_op(sk)] = 2;  // PMDFC_ST_INSERTED
          S.pos[i2] = 0xFFFF;
        }
      }
    }
    stamp(a.stamp, kBsRunClaimed, (__lane_id() & 63u) == 0);
  }
  uint64_t nxt = qs < q1 ? S.sk[qs] : 0ULL;
  uint64_t memo_k = kInvalid, memo_v = 0;  // mixed: last Get probe of this run
  uint8_t memo_s = 0;
  for (uint32_t q = qs; q < q1; ++q) {
    const uint64_t skq = nxt;
    if (q + 1 < q1) nxt = S.sk[q + 1];  // prefetch the next op's key
    const uint32_t i = sk_item(skq);
    const uint32_t op = sk_op(skq);
    if (MIXED && (S.L[i] & 0x80u)) {
      // a Get sees the run's earlier inserts only through its own key
      // (others just fill empty slots past or instead of the probe's end),
      // so repeated Gets of one key reuse the last probe until that key
      // is inserted (hot keys of skewed batches)
      const uint64_t key = S.kv[i].x;
      if (key != memo_k) {
        memo_v = 0;
        memo_s = lane_probe(sp, key, hash64(key), &memo_v);
        memo_k = key;
      }
      a.vout[op] = memo_v;
      a.st[op] = memo_s;
      S.pend[i] = 0;
      continue;
    }
    const uint32_t wi0 = sk_home(skq) * 4u;
    const uint32_t wi = wi0 >> 5;
    if (a.upsert) {
      // last-writer-wins: the key's own slot takes the pair if it has one
      const uint64_t key = chunk_key<REG>(S, i);
      const int upos = upsert_slot<REG>(a, S, sp, bm, q0, q, key, op, wi0);
      if (upos >= 0) {
        S.pos[i] = (uint16_t)upos;
        if (MIXED) {
          if (key == memo_k) memo_k = kInvalid;
          sp[upos] = S.kv[i];
        }
        a.st[op] = 11;  // PMDFC_ST_UPDATED
        lines += ((((uint32_t)upos - wi0) & (kSlots - 1)) >> 2) + 1;
        S.pend[i] = 0;
        continue;
      }
    }
    const int pos = window_first_free(bm[wi], bm[(wi + 1) & 31u], wi0);
    if (pos >= 0) {
      bm[(uint32_t)pos >> 5] |= 1u << ((uint32_t)pos & 31u);
      dirty = true;
      if (MIXED) {
        if (S.kv[i].x == memo_k) memo_k = kInvalid;
        sp[pos] = S.kv[i];
        a.st[op] = 2;  // PMDFC_ST_INSERTED (insert-only batches: preset by k_part)
        if (a.upsert) S.pos[i] = (uint16_t)pos;  // a later insert of the key in this run updates it
      } else {
        S.pos[i] = (uint16_t)pos;
      }
      lines += ((((uint32_t)pos - wi0) & (kSlots - 1)) >> 2) + 1;
      S.pend[i] = 0;
      continue;
    }
    // window full.  The reference would split forever if all 32 entries
    // carry this key's full hash: UNSPLITTABLE.
    bool same;
    if constexpr (REG) same = window_all_same_reg(sp, S.sk, S.pos, S.key, q0, q, i, wi0);
    else same = window_all_same(MIXED, sp, S.sk, S.pos, S.kv, q0, q, i, wi0);
    if (same || L + 1 > kMaxDepth) {
      a.st[op] = same ? 4 : 5;  // PMDFC_ST_UNSPLITTABLE / PMDFC_ST_DEPTH_LIMIT
      S.pend[i] = 0;
      continue;
    }
    if (!FINAL) {
      if (a.full) {  // a split round ran out of segment ids or pool
        a.st[op] = 6;  // PMDFC_ST_CAPACITY
        S.pend[i] = 0;
        continue;
      }
      // request the split; park the rest of the run (batch order is
      // restored by the next pass's sort), nothing of it runs ahead
      const uint32_t ri = a.noreq ? kSplitCap : atomicAdd(&S.nreq, 1u);
      if (ri < kSplitCap) {
        const uint32_t x = sub_index(hash64(chunk_key<REG>(S, i)), a.sbits, a.p1, a.db);
        a.req[ri] = make_uint2(seg | (L << 27), x);
        a.reqop[ri] = op;
        atomicMax(&S.need, L + 1 - lbase);
      }
      if constexpr (!REG) {
        const uint32_t k0 = atomicAdd(&S.nsplit, q1 - q);
        for (uint32_t qq = q; qq < q1; ++qq) {
          const uint32_t i2 = sk_item(S.sk[qq]);
          a.wl_kv[k0 + (qq - q)] = S.kv[i2];
          a.wl_op[k0 + (qq - q)] = S.op[i2];
        }
      } else {  // the rest of the run stays pending; its owner lanes park it
        for (uint32_t qq = q; qq < q1; ++qq) S.pend[sk_item(S.sk[qq])] = 2;
      }
      waited += q1 - q;
      break;
    }
    // the final pass grows the sub-directory itself: a split whose growth the
    // pool can no longer take (pool_cur only grows) fails before it takes a
    // child id
    if (const uint32_t nb = L + 1 - lbase; nb > a.db && !(a.pfix && nb <= kFixedBits) &&
        (uint64_t)ld_u32_l2(&a.ctl->pool_cur) + (1ULL << nb) > a.pool_cap) {
      atomicOr(&a.ctl->err, 1u);
      a.st[op] = 6;  // PMDFC_ST_CAPACITY
      S.pend[i] = 0;
      continue;
    }
    const uint32_t si = atomicAdd(&S.nsplit, 1u);
    if (si >= kSplitCap) {
      waited += q1 - q;  // split queue full: the run retries next round
      break;
    }
    const uint32_t c1 = atomicAdd(&a.ctl->nsegs, 1u);
    if (c1 >= a.max_segments) {
      S.split[si] = ~0ULL;
      a.st[op] = 6;  // PMDFC_ST_CAPACITY
      S.pend[i] = 0;
      continue;
    }
    S.split[si] = (uint64_t)i | ((uint64_t)L << 16) | ((uint64_t)c1 << 21);
    atomicMax(&S.need, L + 1 - lbase);
    waited += q1 - q;
    break;  // the rest of the run waits for the split
  }
  if (dirty) {
    uint32_t* o = a.occ + (size_t)seg * 32u;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      *reinterpret_cast<uint4*>(o + 4 * j) = make_uint4(bm[4 * j], bm[4 * j + 1], bm[4 * j + 2], bm[4 * j + 3]);
  }
  stamp(a.stamp, kBsRunEnd, (__lane_id() & 63u) == 0);
  return make_uint2(lines, waited);
}

// Sub-directory growth to `need` bits: a new pool region, new[i] = old[i >> k]
// (CCEH_hybrid.cpp:208-219 at bucket scale).  A fixed slot grows in place
// (no == off, at most kFixedSlot entries): every old entry is read into a
// register before any new one is stored.
__device__ __forceinline__ void grow_subdir(const BucketArgs& a, uint32_t w, uint32_t no, uint32_t need,
                                            uint32_t& off, uint32_t& db) {
  const uint32_t lane = __lane_id() & 63u;
  const uint32_t size = 1u << need, sh = need - db;
  if (size <= 128) {  // (a fixed slot holds up to 128 entries: all read before any store)
    const uint32_t v0 = lane < size ? ld_u32_l2(a.pool + off + (lane >> sh)) : 0u;
    const uint32_t v1 = lane + 64u < size ? ld_u32_l2(a.pool + off + ((lane + 64u) >> sh)) : 0u;
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    if (lane < size) a.pool[no + lane] = v0;
    if (lane + 64u < size) a.pool[no + lane + 64u] = v1;
  } else {  // (never in place)
    for (uint32_t t = lane; t < size; t += 64) a.pool[no + t] = ld_u32_l2(a.pool + off + (t >> sh));
  }
  __builtin_amdgcn_s_waitcnt(0);
  off = no;
  db = need;
  if (lane == 0) a.hdr[w] = hdr_make(no, need);
}

// Directory half of a split (CCEH_hybrid.cpp:243-286): the 2^(db - Lb) entries
// of the parent; the first half keeps child 0 (the parent's id), the second
// half gets child 1.  x: any sub-index of the parent at the current db.
__device__ __forceinline__ void dir_split(const BucketArgs& a, uint32_t off, uint32_t db, uint32_t x,
                                          uint32_t seg, uint32_t c1, uint32_t L) {
  const uint32_t lane = __lane_id() & 63u;
  const uint32_t Lb = L - a.sbits - a.p1;
  const uint32_t span = 1u << (db - Lb);
  const uint32_t xs = x & ~(span - 1u);
  for (uint32_t t = lane; t < span; t += 64) a.pool[off + xs + t] = de_make(t < span / 2 ? seg : c1, L + 1);
}

// Commit the splits granted to this bucket at the end of its last pass
// (k_split already moved the entries): grow the sub-directory if they need
// it, then point the children's directory entries at them.
__device__ __forceinline__ void commit_splits(const BucketArgs& a, uint32_t w, uint32_t& off, uint32_t& db,
                                              WaveStat& c) {
  const uint32_t ng = a.ngrant[w];
  if (!ng) return;
  const uint32_t db0 = db;
  const uint32_t nd = a.need[w];
  if (nd > db) {
    grow_subdir(a, w, a.newoff[w], nd, off, db);
    ++c.grow;
  }
  const uint32_t cb = a.gbase[w];
  const uint2* rq = a.req + (size_t)w * kSplitCap;
  for (uint32_t i = 0; i < ng; ++i) {
    const uint2 r = rq[i];
    const uint32_t L = r.x >> 27;
    dir_split(a, off, db, r.y << (db - db0), r.x & ((1u << 27) - 1), cb + i, L);
    c.max_ld = max(c.max_ld, L + 1);
  }
  __builtin_amdgcn_s_waitcnt(0);
  c.splits += ng;
  if ((__lane_id() & 63u) == 0) a.ngrant[w] = 0;
}

// A bucket's split requests, at the end of the apply pass that made them:
// one atomic on its shard's segment word (cceh_kernels.h: kGShards) and, if
// its sub-directory must grow, one on the shard's pool word reserve its
// offsets among the shard's requested child segments and pool entries; each
// request is then recorded at its segment offset (k_split takes one per
// wave and turns the offsets into global grants).  (The grants used to be a
// prefix sum over all buckets in a single-workgroup kernel between the
// passes, a 12-20 us latency chain per batch with splits; one unsharded word
// serializes the ~8k requests of a split-heavy batch for ~100 us.)
// Wave-uniform call, after the wave's request stores.
__device__ __forceinline__ void request_splits(const BucketArgs& a, uint32_t w, uint32_t nr, uint32_t need) {
  const uint32_t lane = __lane_id() & 63u, x = w % kGShards;
  unsigned long long* sh = reinterpret_cast<unsigned long long*>(a.gsh + ((size_t)a.par * kGShards + x) * kGStride);
  uint64_t old = 0;
  if (lane == 0) old = atomicAdd(sh, (unsigned long long)nr | (1ULL << 32));
  if (lane == 1 && need && !(a.pfix && need <= kFixedBits)) old = atomicAdd(sh + 16, 1ULL << need);  // (else its fixed slot)
  __builtin_amdgcn_s_waitcnt(0);  // (this wave's request stores: read back below from L2)
  const uint32_t rw = lane < nr ? ld_u32_l2(reinterpret_cast<const uint32_t*>(a.req + (size_t)w * kSplitCap + lane)) : 0u;
  const uint64_t os = shfl64(old, 0), op = shfl64(old, 1);
  if (lane == 0) a.ctl->anyreq[a.par] = 1;
  // (a pool offset past 2^32 saturates: it is denied either way)
  if (lane < nr)
    a.gsplit[((size_t)a.par * kGShards + x) * a.gcap + (uint32_t)os + lane] =
        make_uint4(rw, w | (lane << 14) | ((uint32_t)(os >> 32) << 20), (uint32_t)min<uint64_t>(op, 0xFFFFFFFFULL),
                   nr | (need << 8));
}

// The batch's shard words, as prefixes over the shards: requesting buckets,
// splits and pool entries before shard x and the totals.  The per-shard
// prefixes live in lane x (< kGShards) and are read with a cross-lane read
// by the wave-uniform shard index: as arrays indexed at run time they went
// to scratch memory, 144 B per lane stored by every k_split wave (~19 MB of
// writes per launch of 2,048 waves) and reloaded per split.
struct GrantScan {
  uint32_t ce_l, cs_l;  // lane x: requesting buckets / splits before shard x
  uint64_t cp_l;        // lane x: pool entries before shard x
  uint32_t E, S;
  uint64_t P;
  __device__ __forceinline__ uint32_t ce(uint32_t x) const { return (uint32_t)__shfl((int)ce_l, (int)x); }
  __device__ __forceinline__ uint32_t cs(uint32_t x) const { return (uint32_t)__shfl((int)cs_l, (int)x); }
  __device__ __forceinline__ uint64_t cp(uint32_t x) const { return shfl64(cp_l, (int)x); }
};
__device__ __forceinline__ GrantScan grant_scan(const uint64_t* gsh, uint32_t par) {
  const uint32_t lane = __lane_id() & 63u;
  // lanes 0-7: the shards' segment words, lanes 8-15: their pool words
  const uint64_t mine = lane < 2 * kGShards
      ? __builtin_nontemporal_load(gsh + ((size_t)par * kGShards + (lane % kGShards)) * kGStride + (lane / kGShards) * 16)
      : 0ULL;
  GrantScan g;
  uint32_t e = 0, sg = 0;
  uint64_t p = 0;
  g.ce_l = g.cs_l = 0;
  g.cp_l = 0;
#pragma unroll
  for (uint32_t x = 0; x < kGShards; ++x) {
    const uint64_t v = shfl64(mine, (int)x), vp = shfl64(mine, (int)(x + kGShards));
    if (lane == x) {
      g.ce_l = e;
      g.cs_l = sg;
      g.cp_l = p;
    }
    e += (uint32_t)(v >> 32);
    sg += (uint32_t)v;
    p += vp;
  }
  g.E = e;
  g.S = sg;
  g.P = p;
  return g;
}
// split k of the batch (shard-major): its shard, the last x with cs(x) <= k
// (the prefixes are non-decreasing, so that is how many of shards 1..7 have
// cs <= k)
__device__ __forceinline__ uint32_t split_shard(const GrantScan& g, uint32_t k) {
  const uint32_t lane = __lane_id() & 63u;
  return (uint32_t)__popcll(__ballot(lane >= 1u && lane < kGShards && g.cs_l <= k));
}

// ---- parallel claims of the insert-only apply passes (fast_claim)
//
// Serial semantics (CCEH_hybrid.cpp:143-168): a segment's inserts, in batch
// order, each take the first free slot of their 32-slot window; the first one
// that finds its window full splits the segment, and it and every later insert
// of the segment wait for the split.  Two inserts of a segment interact only
// if their windows overlap -- home lines less than 8 apart (cyclic) -- since an
// insert only ever claims inside its own window.  So:
//   * an insert whose claim range -- home slot to the first free slot of its
//     window in the pre-pass bitmap -- meets no other insert's window (no
//     other insert of the segment homed from 7 lines before its home to the
//     line of that slot) is INDEPENDENT: nothing can claim inside that range
//     before it, and its claim is in nobody's window, so it takes that slot
//     whatever the batch order (lane per op, in parallel);
//   * the others (DEPENDENT, ~1/3 at the config-2 load) resolve in rounds, each
//     on its own lane: an insert whose earlier overlapping inserts (smaller op
//     index, same segment) have all resolved takes the first free slot of its
//     window in the pre-pass bitmap plus their claims.  The earliest unresolved
//     insert of every segment resolves in each round, so the rounds end; their
//     number is the longest chain of overlapping inserts (2-3 at config 2);
//   * the segment's split point is the smallest op index whose window is
//     full; inserts after it are parked, the one at it requests the split
//     (decisions taken after the split point are dropped with their insert).
//     If that insert fails instead of splitting (UNSPLITTABLE, DEPTH_LIMIT,
//     CAPACITY: later inserts go on past it), the sorted run loop takes over.
// Nothing is written until every decision is made, so a segment with more than
// kDepMax dependent inserts (tiny or skewed tables) hands the round back to the
// sorted run loop.  Checked against the serial rule on random bitmaps and home
// lines, and by the parity suite (configs 1 and 2 whole-table bit-exact).
constexpr uint32_t kFastBins = 32;  // segments (bins) of a bucket fast_claim handles (the general pass, k_apply_fast)
constexpr uint32_t kDepMax = 32;    // dependent inserts per segment it resolves
// LDS scratch (u32 words) of fast_claim for a dependent list of up to NL
// inserts on up to NB segments (bins) of the bucket (the apply pass's union
// area: NL = kCW; k_apply_fast: kFC; k_apply_wide: kFCW, 64 bins)
template <uint32_t NL, uint32_t NB = kFastBins>
struct FcLayout {
  static_assert(NB <= 64, "one lane per bin");
  static constexpr uint32_t Hm = 0;                      // [bin][8] home lines holding an insert
  static constexpr uint32_t Dm = Hm + NB * 8;            // [bin][8] home lines holding >= 2
  static constexpr uint32_t Cnt = Dm + NB * 8;           // [bin] dependent inserts
  static constexpr uint32_t Dst = Cnt + NB;              // [bin] their first list position
  static constexpr uint32_t Full = Dst + NB;             // [bin] op index of the segment's split (~0 none)
  static constexpr uint32_t Opk = Full + NB;             // dependent list [NL]: op << 8 | home
  static constexpr uint32_t Snap = Opk + NL;             // [NL] window occupancy before the pass
  static constexpr uint32_t Res = Snap + NL;             // [NL] u16 result (kFr*), 0 = unresolved
  static constexpr uint32_t Slot = Res + NL / 2;         // [NL] u8 insert slot (key index)
  static constexpr uint32_t Binp = Slot + NL / 4;        // [NL] u8 bin of the list entry
  static constexpr uint32_t Unres = Binp + NL / 4;       // [bin] entries still unresolved (bit q: entry dst + q)
  static constexpr uint32_t Words = Unres + NB;
};
static_assert(FcLayout<kCW>::Words <= kBmWords + 2 * kCW, "fast_claim scratch spans the bitmap rows and sort keys");
constexpr uint32_t kFrClaim = 0x8000u, kFrFail = 0x4000u, kFrSplit = 0x2000u, kFrPark = 0x1000u;
constexpr uint32_t kFrFull = 0x0800u;  // window full: the segment's split point if it is the first

// every slot of the window starting at wo holds a key of full hash h: the
// pre-pass pairs in memory, or the key of an earlier claim of this pass in the
// segment's dependent list [b0, b0 + n) -- the reference would split forever.
// 0 no, 1 yes, 2 undecided (a slot claimed this pass and no key array: the
// lean pass keeps no keys in LDS and hands such a bucket back)
__device__ __forceinline__ uint32_t fc_all_same(const ulonglong2* sp, uint64_t h, uint32_t wo, const uint16_t* res,
                                             const uint8_t* slot8, const uint64_t* s_key, uint32_t b0, uint32_t n) {
  for (uint32_t t = 0; t < kWindow; ++t) {
    const uint32_t sl = (wo + t) & (kSlots - 1);
    uint64_t k = kInvalid;
    bool claimed = false;
    for (uint32_t q = 0; q < n; ++q) {
      const uint32_t r = res[b0 + q];
      if ((r & kFrClaim) && (r & (kSlots - 1)) == sl) {
        if (!s_key) return 2u;
        k = s_key[slot8[b0 + q]];
        claimed = true;
      }
    }
    if (!claimed) k = ld_pair_l2(sp + sl).x;
    if (hash64(k) != h) return 0u;
  }
  return 1u;
}

// A full window: the insert fails (UNSPLITTABLE, DEPTH_LIMIT, CAPACITY) or
// splits its segment.  Returns kFrFail | status, or kFrSplit (kFrFail | 0:
// undecided, see fc_all_same).
__device__ __forceinline__ uint32_t fc_full(const BucketArgs& a, uint32_t full, uint32_t e, uint64_t key,
                                            uint32_t wo, const uint16_t* res, const uint8_t* slot8,
                                            const uint64_t* s_key, uint32_t b0, uint32_t n) {
  const uint32_t same = fc_all_same(a.pairs + (size_t)de_seg(e) * kSlots, hash64(key), wo, res, slot8, s_key, b0, n);
  if (same == 2u) return kFrFail;
  if (same || de_ld(e) + 1 > kMaxDepth) return kFrFail | (same ? 4u : 5u);  // UNSPLITTABLE / DEPTH_LIMIT
  if (full) return kFrFail | 6u;  // PMDFC_ST_CAPACITY: a split round ran out of ids or pool
  return kFrSplit;
}

// bin(j): insert j's bin, an index (< NB) of its segment within the bucket
// (one bin per segment); the caller defines it.
// UPS (last-writer-wins, the lean pass): upd[j] is the pre-batch slot of
// insert j's key in its window (0xFFFF: absent; the caller probed it, with
// no duplicate key in the bucket) and owin[j] its window's occupancy bits
// (loaded by the caller for that probe).  An insert whose key is
// stored claims nothing: it overwrites its slot (PMDFC_ST_UPDATED) unless its
// segment splits before it in the batch, then it is parked like the others.
// A lane's kPer ops as fast_claim reads them: key, value, rop word, whether
// the slot holds an insert, its directory entry, home line and sub-directory
// index (references: the arrays stay the caller's registers)
struct LaneOps {
  const uint64_t (&rk)[kPer], (&rv)[kPer];
  const uint32_t (&rop)[kPer];
  const bool (&pq)[kPer];
  const uint32_t (&e8)[kPer], (&home8)[kPer], (&x8)[kPer];
};
// fast_claim's scratch (FcLayout) as pointers
template <uint32_t NL, uint32_t NB>
struct FcScr {
  using FL = FcLayout<NL, NB>;
  uint32_t *hm, *dm, *cnt, *dst, *bfull, *opk, *snap, *unres;
  uint16_t* res;
  uint8_t *slot8, *binp;
  __device__ __forceinline__ explicit FcScr(uint32_t* sc)
      : hm(sc + FL::Hm), dm(sc + FL::Dm), cnt(sc + FL::Cnt), dst(sc + FL::Dst), bfull(sc + FL::Full),
        opk(sc + FL::Opk), snap(sc + FL::Snap), unres(sc + FL::Unres), res(reinterpret_cast<uint16_t*>(sc + FL::Res)),
        slot8(reinterpret_cast<uint8_t*>(sc + FL::Slot)), binp(reinterpret_cast<uint8_t*>(sc + FL::Binp)) {}
};

// Step 3 of fast_claim: the ntot dependent inserts resolve in rounds, one list
// entry per lane (the list is usually shorter than a wave): first each
// entry's earlier overlapping entries of its segment as a mask over the
// segment's list, then rounds in which an entry whose mask is resolved
// decides (F.res; a full window lowers F.bfull to its op index).
template <uint32_t NL, uint32_t NB>
__device__ __forceinline__ void fc_resolve(const FcScr<NL, NB>& F, uint32_t ntot, uint64_t* srow) {
  const uint32_t lane = __lane_id() & 63u;
  constexpr int kLp = (int)NL / 64;
  uint32_t dmask[kLp], lres[kLp];
#pragma unroll
  for (int u = 0; u < kLp; ++u) {
    const uint32_t p = (uint32_t)u * 64u + lane;
    dmask[u] = 0;
    lres[u] = 1;  // (no entry: nothing to resolve)
    if (p >= ntot) continue;
    lres[u] = 0;
    const uint32_t v = F.opk[p], xc = F.binp[p], q0 = F.dst[xc], n = F.cnt[xc];
    const uint32_t op = v >> 8, h = v & 0xFFu;
    for (uint32_t q = 0; q < n; q += 4) {  // 4 independent LDS reads in flight
      uint32_t vq[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) vq[t] = q + t < n ? F.opk[q0 + q + t] : 0xFFFFFFFFu;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const uint32_t dl = ((vq[t] & 0xFFu) - h) & 0xFFu;
        if ((vq[t] >> 8) < op && (dl <= 7u || dl >= 249u)) dmask[u] |= 1u << (q + t);
      }
    }
  }
  stamp(srow, kBsFcMasks, lane == 0);
  uint32_t nrounds = 0;
  for (uint32_t round = 0; round <= kDepMax; ++round) {
    ++nrounds;
    bool blocked_any = false;
    uint32_t nr[kLp];
#pragma unroll
    for (int u = 0; u < kLp; ++u) {
      nr[u] = 0;
      const uint32_t p = (uint32_t)u * 64u + lane;
      if (lres[u]) continue;
      const uint32_t xc = F.binp[p];
      if (dmask[u] & F.unres[xc]) {
        blocked_any = true;
        continue;
      }
      const uint32_t v = F.opk[p], wo = (v & 0xFFu) * 4u, q0 = F.dst[xc];
      uint32_t occw = F.snap[p];
      bool park = false;
      for (uint32_t m = dmask[u]; m; m &= m - 1u) {
        const uint32_t rq = F.res[q0 + (uint32_t)__builtin_ctz(m)];
        const uint32_t ds = ((rq & (kSlots - 1)) - wo) & (kSlots - 1);
        park |= (rq & (kFrFull | kFrPark)) != 0;
        if ((rq & kFrClaim) && ds < kWindow) occw |= 1u << ds;
      }
      if (park) {  // behind an earlier full window of its segment: waits with it
        nr[u] = kFrPark;
      } else if (~occw) {
        nr[u] = kFrClaim | ((wo + (uint32_t)__builtin_ctz(~occw)) & (kSlots - 1));
      } else {
        nr[u] = kFrFull;
        atomicMin(&F.bfull[xc], v >> 8);
      }
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int u = 0; u < kLp; ++u) {
      if (!nr[u]) continue;
      const uint32_t p = (uint32_t)u * 64u + lane, xc = F.binp[p];
      F.res[p] = (uint16_t)nr[u];
      atomicAnd(&F.unres[xc], ~(1u << (p - F.dst[xc])));
      lres[u] = nr[u];
    }
    __builtin_amdgcn_wave_barrier();
    if (!__ballot(blocked_any)) break;
  }
  stamp(srow, kBsFcResolved, lane == 0);
  if (srow && lane == 0) srow[kBsFcRounds] = nrounds | ((uint64_t)ntot << 16);
}

// Step 4 of fast_claim: every decision is made (st[j]: kFr* | slot of the
// lane's insert j; pc[j]: it claims a slot).  What precedes its segment's
// split is committed, the rest parked; the insert at the split requests it.
template <bool UPS, uint32_t NL, uint32_t NB, class BinF>
__device__ __forceinline__ void fc_commit(const BucketArgs& a, uint32_t w, const FcScr<NL, NB>& F, const LaneOps& o,
                                          const bool (&pc)[kPer], const uint32_t (&st)[kPer], BinF bin,
                                          ulonglong2* wl_kv, uint32_t* wl_op, uint32_t* s_nsplit, uint32_t* s_nreq,
                                          uint32_t* s_need, WaveStat& c, const uint32_t* upd) {
  const uint32_t lbase = a.sbits + a.p1;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    if (!o.pq[j]) continue;
    const uint32_t op = o.rop[j] & kOpMask, bf = F.bfull[bin(j)];
    const uint32_t r = st[j] & 0xFFFFu;
    const uint32_t seg = de_seg(o.e8[j]);
    if (op >= bf || (r & kFrPark)) {
      if (op == bf) {  // this insert's full window splits the segment
        const uint32_t L = de_ld(o.e8[j]);
        const uint32_t ri = a.mode == 2 ? kSplitCap : atomicAdd(s_nreq, 1u);
        if (ri < kSplitCap) {
          a.req[(size_t)w * kSplitCap + ri] = make_uint2(seg | (L << 27), o.x8[j]);
          a.reqop[(size_t)w * kSplitCap + ri] = op;
          atomicMax(s_need, L + 1 - lbase);
        }
      }
      const uint32_t k = atomicAdd(s_nsplit, 1u);
      wl_kv[k] = make_ulonglong2(o.rk[j], o.rv[j]);
      wl_op[k] = o.rop[j];
      ++c.waited;
    } else if (r & kFrClaim) {
      const uint32_t sl = r & (kSlots - 1);
      a.pairs[(size_t)seg * kSlots + sl] = make_ulonglong2(o.rk[j], o.rv[j]);
      atomicOr(a.occ + (size_t)seg * 32u + (sl >> 5), 1u << (sl & 31u));
      c.lines += (((sl - o.home8[j] * 4u) & (kSlots - 1)) >> 2) + 1u;
    } else if (UPS && !pc[j]) {  // its key is stored: overwrite in place
      const uint32_t sl = upd[j];
      a.pairs[(size_t)seg * kSlots + sl] = make_ulonglong2(o.rk[j], o.rv[j]);
      a.st[op] = 11;  // PMDFC_ST_UPDATED
      c.lines += (((sl - o.home8[j] * 4u) & (kSlots - 1)) >> 2) + 1u;
    }
  }
}

template <uint32_t NL, uint32_t NB, bool UPS = false, class BinF>
__device__ __forceinline__ bool fast_claim(const BucketArgs& a, uint32_t w, uint32_t* sc,
                                           const uint64_t* s_key, ulonglong2* wl_kv, uint32_t* wl_op,
                                           uint32_t* s_nsplit, uint32_t* s_nreq, uint32_t* s_need,
                                           const LaneOps& o, BinF bin, WaveStat& c, uint64_t* srow,
                                           const uint32_t* upd = nullptr, const uint32_t* owin = nullptr) {
  const uint32_t lane = __lane_id() & 63u;
  const uint32_t full = a.ctl->full;
  const FcScr<NL, NB> F(sc);
  uint32_t *const hm = F.hm, *const dm = F.dm, *const cnt = F.cnt, *const dst = F.dst, *const bfull = F.bfull;
  // claimers: the inserts that take a slot (UPS: not those whose key is stored)
  bool pc[kPer];
#pragma unroll
  for (int j = 0; j < kPer; ++j) pc[j] = o.pq[j] && (!UPS || upd[j] == 0xFFFFu);
  // each insert's occupancy window (UPS: upsert_probe loaded it), in flight during the LDS work
  WinLd ow[UPS ? 1 : kPer];
  if constexpr (!UPS) {
#pragma unroll
    for (int j = 0; j < kPer; ++j)
      if (pc[j]) ow[j] = ld_window_l2(a.occ + (size_t)de_seg(o.e8[j]) * 32u, o.home8[j] >> 3);
  }
  // bit t: slot home * 4 + t taken before the pass
  const auto wbits = [&](int j) -> uint32_t {
    if constexpr (UPS) return owin[j];
    else return window_bits(ow[j], o.home8[j]);
  };
#pragma unroll
  for (int t = 0; t < (int)(2 * NB * 8 / 64); ++t) hm[t * 64 + lane] = 0;  // hm and dm
  if (lane < NB) {
    cnt[lane] = 0;
    bfull[lane] = 0xFFFFFFFFu;
  }
  __builtin_amdgcn_wave_barrier();
  // 1. home lines per segment; a line taken twice is marked in dm
  uint32_t st[kPer];  // per insert: result (kFr* | slot or status) | list position << 16 | dependent << 24
#pragma unroll
  for (int j = 0; j < kPer; ++j)
    if (pc[j]) st[j] = atomicOr(&hm[bin(j) * 8u + (o.home8[j] >> 5)], 1u << (o.home8[j] & 31u));
#pragma unroll
  for (int j = 0; j < kPer; ++j)
    if (pc[j] && ((st[j] >> (o.home8[j] & 31u)) & 1u)) atomicOr(&dm[bin(j) * 8u + (o.home8[j] >> 5)], 1u << (o.home8[j] & 31u));
  __builtin_amdgcn_wave_barrier();
  stamp(srow, kBsBinned, lane == 0);
  if (srow && lane == 0) srow[kBsOrdered] = 0;  // (no sort stamp: phase_stamps.py tells the paths apart)
  // 2. independent inserts claim now; dependent ones are counted per segment
  constexpr uint32_t kDep = 1u << 24;
  uint64_t fk = 0;  // first window key of this lane's first independent full window
  int fkj = -1;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    st[j] = 0;
    if (!pc[j]) continue;
    const uint32_t h = o.home8[j], xc = bin(j), base = xc * 8u, l0 = (h - 7u) & 255u;
    const uint32_t wo = h * 4u;
    const uint32_t win = wbits(j);  // bit t: slot wo + t taken
    // lines another insert's window may claim in: its home within 7 lines
    // before this one's, up to the line of this one's claim (the whole window
    // when it is full) -- outside that, neither claim can see the other
    const uint32_t cl = ~win ? (uint32_t)__builtin_ctz(~win) >> 2 : 7u;
    const uint32_t w0 = hm[base + (l0 >> 5)], w1 = hm[base + (((l0 >> 5) + 1u) & 7u)];
    // bit i: line h - 7 + i holds an insert; lines h-7..h+cl but h itself
    const uint32_t nb = __builtin_amdgcn_alignbit(w1, w0, l0 & 31u) & ((0x100u << cl) - 1u) & ~0x80u;
    const bool dup = (dm[base + (h >> 5)] >> (h & 31u)) & 1u;
    if (nb != 0 || dup) {
      const uint32_t r = atomicAdd(&cnt[xc], 1u);
      st[j] = kDep | (r << 16);
    } else if (~win) {
      st[j] = kFrClaim | ((wo + (uint32_t)__builtin_ctz(~win)) & (kSlots - 1));
    } else {
      st[j] = kFrFull;
      atomicMin(&bfull[xc], o.rop[j] & kOpMask);
      if (fkj < 0) {  // the window's first key, for the rarely true UNSPLITTABLE test below
        fk = ld_pair_l2(a.pairs + (size_t)de_seg(o.e8[j]) * kSlots + wo).x;
        fkj = j;
      }
    }
  }
  __builtin_amdgcn_wave_barrier();
  const uint32_t cb = lane < NB ? cnt[lane] : 0u;
  if (__ballot(cb > kDepMax)) return false;  // nothing written outside the scratch yet
  uint32_t ntot;
  const uint32_t ex = wave_excl_scan(cb, &ntot);
  if (lane < NB) dst[lane] = ex;
  uint32_t runs = 0;
  if (lane < NB) {
    uint32_t any = 0;
#pragma unroll
    for (int t = 0; t < 8; ++t) any |= hm[lane * 8u + t];
    runs = (uint32_t)__popcll(__ballot(any != 0));
  }
  __builtin_amdgcn_wave_barrier();
  stamp(srow, kBsBatchOrder, lane == 0);
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    if (!(st[j] & kDep)) continue;
    const uint32_t xc = bin(j), p = dst[xc] + ((st[j] >> 16) & 0xFFu);
    st[j] = kDep | (p << 16);
    F.opk[p] = ((o.rop[j] & kOpMask) << 8) | o.home8[j];
    F.snap[p] = wbits(j);  // the window before the pass
    F.res[p] = 0;
    F.slot8[p] = (uint8_t)((uint32_t)j * 64u + lane);
    F.binp[p] = (uint8_t)xc;
  }
  if (lane < NB) F.unres[lane] = cb >= 32 ? 0xFFFFFFFFu : (1u << cb) - 1u;
  __builtin_amdgcn_wave_barrier();
  // 3. dependent inserts resolve in rounds
  fc_resolve(F, ntot, srow);
  // owners take their dependent results
#pragma unroll
  for (int j = 0; j < kPer; ++j)
    if (st[j] & kDep) st[j] |= F.res[(st[j] >> 16) & 0xFFu];
  // the first full window of a segment splits it -- unless the insert fails
  // instead (UNSPLITTABLE / DEPTH_LIMIT / CAPACITY, rare): then later inserts
  // go on past it, which the sorted run loop handles
  bool fails = false;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    if (!pc[j] || (o.rop[j] & kOpMask) != bfull[bin(j)]) continue;
    const uint32_t xc = bin(j), q0 = (st[j] & kDep) ? dst[xc] : 0u, n = (st[j] & kDep) ? cnt[xc] : 0u;
    if (fkj == j && hash64(fk) != hash64(o.rk[j])) {  // not all one hash: splittable
      fails |= de_ld(o.e8[j]) + 1 > kMaxDepth || full;
      continue;
    }
    fails |= fc_full(a, full, o.e8[j], o.rk[j], o.home8[j] * 4u, F.res, F.slot8, s_key, q0, n) != kFrSplit;
  }
  if (__ballot(fails)) return false;  // still nothing written
  stamp(srow, kBsRunsDone, lane == 0);
  // 4. commit what precedes each segment's split, park the rest
  fc_commit<UPS>(a, w, F, o, pc, st, bin, wl_kv, wl_op, s_nsplit, s_nreq, s_need, c, upd);
  if (lane == 0) c.runs += runs;
  stamp(srow, kBsWritten, lane == 0);
  return true;
}

// The first apply pass of a batch (parity p) resets the previous batch's
// grant shards and final-pass count (parity p ^ 1): every pass that read
// them ran before it on the stream.
__device__ __forceinline__ void clear_other_parity(const BucketArgs& a) {
  const uint32_t lane = __lane_id() & 63u, q = a.par ^ 1u;
  if (lane < 2 * kGShards) a.gsh[((size_t)q * kGShards + (lane % kGShards)) * kGStride + (lane / kGShards) * 16] = 0;
  if (lane == 2 * kGShards) a.ctl->nfin[q] = 0;
  if (lane == 2 * kGShards + 1) a.ctl->anyreq[q] = 0;
  if (lane == 2 * kGShards + 2) a.ctl->anydecl[q] = 0;
}

// ---- what every first pass of a batch does (bucket_body<.., FIRST> in mode
// 0 and apply_fast), one copy each

// The next batch's cursors start at zero, and the previous batch's per-parity
// words are reset.
__device__ __forceinline__ void first_pass_clears(const BucketArgs& a, uint32_t w) {
  const uint32_t lane = __lane_id() & 63u;
  const uint32_t pb = w >> a.sbb, sub = w & ((1u << a.sbb) - 1);
  if (a.clear_next) {
    if (sub == 0 && lane < kPartSubs) a.cursor_next[(lane << (a.p1 - a.sbb)) + pb] = 0;
    if (w == 0 && lane == 0) *a.ovf_next = 0;
  }
  if (w == 0) clear_other_parity(a);
}

// 32 records of each of the partition bucket's kPartSubs sub-regions, one per
// lane and slot: slot u of lane l is record 32 * half + (l & 31) of sub-region
// 2u + l / 32 (clamped to the sub-region: the count decides what is valid).
// Loaded before anything is known about the bucket, so that they share one
// round trip with the header and cursor loads.
constexpr int kPre = 4;  // 4 x 64 = 256 records
static_assert(kPre * 64 == 32 * kPartSubs, "prefetch: 32 records per sub-region");
struct PreRecs {
  uint32_t op[kPre];
  uint64_t k[kPre], v[kPre];
};
__device__ __forceinline__ void prefetch_records(const BucketArgs& a, uint32_t pb, uint32_t half, PreRecs& pr) {
  const uint32_t lane = __lane_id() & 63u;
  const uint64_t rb0 = (uint64_t)pb * a.cap;
#pragma unroll
  for (int u = 0; u < kPre; ++u) {
    const uint32_t jj = (uint32_t)u * 64u + lane;
    const uint64_t j = rb0 + (uint64_t)(jj >> 5) * a.capx + min(half * 32u + (jj & 31u), a.capx - 1u);
    pr.op[u] = a.rop[j];
    const ulonglong2 kv = a.rkv[j];
    pr.k[u] = kv.x;
    pr.v[u] = kv.y;
  }
}
// whether slot u of this lane holds a record of sub-bucket `sub` (csub: below)
__device__ __forceinline__ bool pre_valid(const BucketArgs& a, const PreRecs& pr, int u, uint32_t half, uint32_t csub,
                                          uint32_t sub) {
  const uint32_t jj = (uint32_t)u * 64u + (__lane_id() & 63u);
  const uint32_t cs = (uint32_t)__shfl((int)csub, (int)(jj >> 5));
  return half * 32u + (jj & 31u) < cs && ((pr.op[u] >> 22) & ((1u << a.sbb) - 1)) == sub;
}
// The valid prefetched records appended to kv[] / op[] at m (ballot and
// prefix; nothing stored past `cap`).  Returns the new count, which may
// exceed cap.
__device__ __forceinline__ uint32_t compact_prefetched(const BucketArgs& a, const PreRecs& pr, uint32_t half,
                                                       uint32_t csub, uint32_t sub, uint32_t m, ulonglong2* kv,
                                                       uint32_t* op, uint32_t cap) {
  const uint64_t lt = (1ULL << (__lane_id() & 63u)) - 1;
#pragma unroll
  for (int u = 0; u < kPre; ++u) {
    const bool match = pre_valid(a, pr, u, half, csub, sub);
    const uint64_t bal = __ballot(match);
    const uint32_t idx = m + (uint32_t)__popcll(bal & lt);
    if (match && idx < cap) {
      kv[idx] = make_ulonglong2(pr.k[u], pr.v[u]);
      op[idx] = pr.op[u];
    }
    m += (uint32_t)__popcll(bal);
  }
  return m;
}

// Lane xs (< kPartSubs): the record count of the partition bucket's
// sub-region xs.  The load is issued with the prefetch; sub_count_max, the
// largest of them on every lane, waits for it.
// (sub_count_issue: the load alone, the count not yet clamped to the
// sub-region.  Every lane loads and keeps a count, lane l that of sub-region
// l % kPartSubs: a load under a branch is waited for inside it, ahead of the
// loads issued after it)
__device__ __forceinline__ uint32_t sub_count_issue(const BucketArgs& a, uint32_t pb) {
  const uint32_t lane = __lane_id() & 63u;
  return a.cursor[((lane % kPartSubs) << (a.p1 - a.sbb)) + pb];
}
__device__ __forceinline__ uint32_t sub_count_load(const BucketArgs& a, uint32_t pb) {
  return min(sub_count_issue(a, pb), a.capx);
}
__device__ __forceinline__ uint32_t sub_count_max(uint32_t csub) {
  uint32_t cmax = csub;
#pragma unroll
  for (int o = 4; o > 0; o >>= 1) cmax = max(cmax, (uint32_t)__shfl_xor((int)cmax, o));
  return (uint32_t)__shfl((int)cmax, 0);
}

// The split requests the pass stored (nreq, need: the wave's LDS words) go to
// the bucket's grant shard.  Wave-uniform.
__device__ __forceinline__ void request_tail(const BucketArgs& a, uint32_t w, const uint32_t& nreq,
                                             const uint32_t& need, uint32_t db) {
  __builtin_amdgcn_wave_barrier();
  const uint32_t nr = min(nreq, kSplitCap);
  if (nr) request_splits(a, w, nr, need > db ? need : 0u);
}

// The pass's counters into this bucket's own stat slots (no shared-line
// atomics: one contended device atomic per wave costs more than the wave's
// work).  wsv: the slots' values, lane k holding slot k, loaded at the start
// of the pass.  The lean pass is the case of one round, no split, no growth.
__device__ __forceinline__ void publish_stats(const BucketArgs& a, uint32_t w, uint64_t wsv, WaveStat c) {
  const uint32_t lane = __lane_id() & 63u;
  for (int o = 32; o > 0; o >>= 1) {
    c.lines += (uint32_t)__shfl_down((int)c.lines, o);
    c.waited += (uint32_t)__shfl_down((int)c.waited, o);
  }
  const uint32_t s0 = (uint32_t)__shfl((int)c.lines, 0), s1 = (uint32_t)__shfl((int)c.waited, 0);
  const uint32_t s3 = (uint32_t)__shfl((int)c.loss, 0), s4 = (uint32_t)__shfl((int)c.runs, 0);
  const uint32_t add = lane == 0 ? s0 : lane == 1 ? s1 : lane == 2 ? c.splits : lane == 3 ? s3
                     : lane == 4 ? s4 : lane == 5 ? c.rounds : 0u;
  uint64_t* ws = a.wstat + (size_t)w * kWStat;
  if (lane < 6u && add) ws[lane] = wsv + add;
  if (lane == 3u && s3) atomicAdd(&a.ctl->loss_events, 1u);  // never on the hot path: loss is rare
  // slot 6: max rounds (low 16 bits) | max local depth (bits 16-23) | growths << 32
  if (lane == 6u && (c.max_rounds || c.max_ld || c.grow)) {
    const uint64_t mr = max((uint32_t)(wsv & 0xFFFF), c.max_rounds);
    const uint64_t ml = max((uint32_t)((wsv >> 16) & 0xFF), c.max_ld);
    ws[6] = mr | (ml << 16) | (((wsv >> 32) + c.grow) << 32);
  }
  if (lane == 0 && c.bad) atomicOr(&a.ctl->err, 4u);
}


// ------------------------------------------------- the phases of a bucket pass
//
// bucket_body below is the outline; each phase is a function of the wave's
// LDS (BucketLds), the lane's registers (ChunkRegs, RoundOps) and the pass's
// counters (WaveStat).  REG = !FINAL && !MIXED throughout: the insert-only
// apply passes keep each op's {key, value, rop} in its owner lane's registers
// (chunk slot j*64 + lane); their LDS holds only the keys.

static_assert(kPre == kPer, "the prefetched records fill the chunk registers slot for slot");

// REG: the chunk's ops in registers, slot j of lane l being chunk slot j*64 + l
struct ChunkRegs {
  uint64_t k[kPer], v[kPer];
  uint32_t op[kPer];
  bool ok[kPer];  // the slot holds an op
};

// A round's view of the lane's kPer chunk slots: which are pending, their key
// and rop word, and what the lookup found
struct RoundOps {
  bool pq[kPer];
  uint64_t kk[kPer];
  uint32_t ro[kPer];
  uint32_t e8[kPer], home8[kPer], x8[kPer];  // directory entry, home line, sub-directory index
};

// The chunk slot of a lane's j-th op: strided in the apply pass (a half-full
// chunk leaves whole j-iterations idle, skipped; REG: where the registers
// hold it), blocked for the 64-bit register sort of the other paths
__device__ __forceinline__ uint32_t chunk_slot(bool strided, int j) {
  const uint32_t lane = __lane_id() & 63u;
  return strided ? (uint32_t)j * 64u + lane : kPer * lane + (uint32_t)j;
}

// Apply pass: a sub-directory of up to kLdsDir entries is read once into LDS
// (alongside the record loads) instead of one dependent global load per op.
// Loaded at the start of the pass, written to S.dir at first use: the loads
// (which wait for the header) overlap the record loads' wait and the hashing.
struct LdsDir {
  bool on = false, written = false;
  uint32_t v0 = 0, v1 = 0;  // entries lane and lane + 64
};
__device__ __forceinline__ LdsDir lds_dir_load(const BucketArgs& a, uint32_t off, uint32_t db) {
  const uint32_t lane = __lane_id() & 63u;
  LdsDir d;
  d.on = (1u << db) <= kLdsDir;
  if (d.on) {
    if (lane < (1u << db)) d.v0 = ld_u32_l2(a.pool + off + lane);
    if (lane + 64u < (1u << db)) d.v1 = ld_u32_l2(a.pool + off + lane + 64u);
  }
  return d;
}

// REG: every lane takes chunk slots j*64 + lane of the m ops in kv[] / op[]
__device__ __forceinline__ void take_chunk(const ulonglong2* kv, const uint32_t* op, uint32_t m, ChunkRegs& r) {
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const uint32_t i = (uint32_t)j * 64u + (__lane_id() & 63u);
    r.ok[j] = i < m;
    if (r.ok[j]) {
      const ulonglong2 p = kv[i];
      r.k[j] = p.x;
      r.v[j] = p.y;
      r.op[j] = op[i];
    }
  }
}

// ---- loading a chunk.  Four sources: the batch's records (first pass), the
// bucket's parked list, a chunk the caller pre-loaded (nothing to do), and
// the tile walk of a bucket with more ops than a chunk (big_chunk above).

// First pass: the bucket's records of the batch into the chunk -- the
// prefetched ones if they are all there is (at most 32 per sub-region, no
// overflow), else collected.  Returns their number; past C nothing usable is
// loaded (the final pass takes the bucket).
template <bool REG, class Lds>
__device__ __forceinline__ uint32_t load_records(const BucketArgs& a, Lds& S, uint32_t pb, uint32_t sub,
                                                 const PreRecs& pr, uint32_t csub, uint32_t cmax, uint32_t novf,
                                                 uint32_t C, ChunkRegs& r) {
  const bool prefetched = cmax <= 32u && novf == 0;
  uint32_t m = 0;
  if constexpr (REG) {
    if (prefetched) {
      // the prefetched records stay where they were loaded: chunk slot
      // u*64 + lane (sub-region u*2 + lane/32), holes where the record is
      // another sub-bucket's or past the sub-region's count
#pragma unroll
      for (int u = 0; u < kPre; ++u) {
        r.ok[u] = pre_valid(a, pr, u, 0, csub, sub);
        r.k[u] = pr.k[u];
        r.v[u] = pr.v[u];
        r.op[u] = pr.op[u];
        m += (uint32_t)__popcll(__ballot(r.ok[u]));
      }
    } else {
      // collect compacts into the (still unused) sort scratch and sort
      // keys (contiguous: kCW pairs), the rop words into the key array,
      // then every lane takes chunk slots j*64 + lane into registers
      ulonglong2* stg = reinterpret_cast<ulonglong2*>(S.u);
      uint32_t* sop = reinterpret_cast<uint32_t*>(S.key);
      m = collect(a, pb, sub, csub, novf, stg, sop);
      if (m <= C) take_chunk(stg, sop, m, r);
      __builtin_amdgcn_wave_barrier();
    }
  } else {
    if (prefetched) m = compact_prefetched(a, pr, 0, csub, sub, 0, S.kv, S.op, (uint32_t)kCW);
    else m = collect(a, pb, sub, csub, novf, S.kv, S.op);
  }
  return m;
}

// A later pass: the m ops parked on the bucket's wait list
template <bool REG, class Lds>
__device__ __forceinline__ void load_parked(const ulonglong2* wl_kv, const uint32_t* wl_op, uint32_t m, Lds& S,
                                            ChunkRegs& r) {
  if constexpr (REG) {
    take_chunk(wl_kv, wl_op, m, r);
  } else {
    for (uint32_t i = __lane_id() & 63u; i < m; i += 64) {
      S.kv[i] = wl_kv[i];
      S.op[i] = wl_op[i];
    }
  }
}

// every op of the loaded chunk is pending and has claimed nothing
template <bool REG, class Lds>
__device__ __forceinline__ void mark_pending(Lds& S, uint32_t m, const ChunkRegs& r) {
  const uint32_t lane = __lane_id() & 63u;
  if constexpr (REG) {
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const uint32_t i = (uint32_t)j * 64u + lane;
      S.pend[i] = r.ok[j] ? 1 : 0;
      S.pos[i] = 0xFFFF;
      if (r.ok[j]) S.key[i] = r.k[j];
    }
  } else {
    for (uint32_t i = lane; i < m; i += 64) {
      S.pend[i] = 1;
      S.pos[i] = 0xFFFF;
    }
  }
  __builtin_amdgcn_wave_barrier();
}

// ---- a round

// The lane's ops still pending (o.pq, with key and rop word); returns how many
template <bool REG, class Lds>
__device__ __forceinline__ uint32_t gather_pending(const Lds& S, const ChunkRegs& r, uint32_t m, bool strided,
                                                   RoundOps& o) {
  uint32_t cntp = 0;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const uint32_t i = chunk_slot(strided, j);
    if constexpr (REG) {
      o.pq[j] = r.ok[j] && S.pend[i];
      o.kk[j] = r.k[j];
      o.ro[j] = r.op[j];
    } else {
      o.pq[j] = i < m && S.pend[i];
      if (o.pq[j]) {
        o.kk[j] = S.kv[i].x;
        o.ro[j] = S.op[i];
      }
    }
    cntp += o.pq[j];
  }
  return cntp;
}

// More rounds than the depth bound allows: cannot happen; the pending ops
// fail loudly (CAPACITY, error flag 2) rather than spin
template <class Lds>
__device__ __forceinline__ void fail_pending(const BucketArgs& a, Lds& S, bool strided, const RoundOps& o) {
#pragma unroll
  for (int j = 0; j < kPer; ++j)
    if (o.pq[j]) {
      a.st[o.ro[j] & kOpMask] = 6;
      S.pend[chunk_slot(strided, j)] = 0;
    }
  if ((__lane_id() & 63u) == 0) atomicOr(&a.ctl->err, 2u);
}

// Entry lookup: each pending op's home line, sub-directory index and
// directory entry (from S.dir when the sub-directory is LDS-resident)
template <bool FINAL, class Lds>
__device__ __forceinline__ void lookup_entries(const BucketArgs& a, Lds& S, uint32_t off, uint32_t db, LdsDir& d,
                                               RoundOps& o) {
  const uint32_t lane = __lane_id() & 63u;
#pragma unroll
  for (int j = 0; j < kPer; ++j)
    if (o.pq[j]) {
      const uint64_t h = hash64(o.kk[j]);
      o.home8[j] = (uint32_t)(h & 0xFF);
      o.x8[j] = sub_index(h, a.sbits, a.p1, db);
    }
  if constexpr (!FINAL) {
    if (d.on && !d.written) {
      if (lane < (1u << db)) S.dir[lane] = d.v0;
      if (lane + 64u < (1u << db)) S.dir[lane + 64u] = d.v1;
      __builtin_amdgcn_wave_barrier();
      d.written = true;
    }
  }
#pragma unroll
  for (int j = 0; j < kPer; ++j)
    if (o.pq[j]) {
      if constexpr (!FINAL) o.e8[j] = d.on ? S.dir[o.x8[j]] : ld_u32_l2(a.pool + off + o.x8[j]);
      else o.e8[j] = ld_u32_l2(a.pool + off + o.x8[j]);
    }
}

// The bin of an op on an LDS-resident sub-directory: its segment's first
// sub-directory index (one bin per segment)
__device__ __forceinline__ uint32_t first_sub_index(const BucketArgs& a, uint32_t db, uint32_t x, uint32_t e) {
  return x & ~((1u << (db - (de_ld(e) - (a.sbits + a.p1)))) - 1u);
}

// Ordering on an LDS-resident sub-directory (apply passes), without a 64-bit
// sort: the np pending ops in batch order (32-bit keys op << 8 | slot), then
// a stable counting sort by bin (< kLdsDir).  Leaves the sort keys in S.sk
// run by run, the run bounds in S.runq, the depths in S.L and -- unless the
// sub-directory is wide (128 entries: two bins per lane, the runs load their
// own bitmaps) -- the bitmap of each of the first kBmLanes runs in its row of
// S.u.  Returns the number of runs.  srow: stamped if not null.
template <class Lds>
__device__ __forceinline__ uint32_t order_by_bins(const BucketArgs& a, Lds& S, const RoundOps& o, uint32_t np,
                                                  uint32_t db, bool wide, uint64_t* srow) {
  const uint32_t lane = __lane_id() & 63u;
  uint32_t* hist = S.u;                                  // [128] ops per bin
  uint32_t* cur = S.u + 128;                             // [128] next position of the bin
  uint8_t* xcs = reinterpret_cast<uint8_t*>(S.u + 256);  // [kCW] bin of each slot
  uint32_t* bseg = S.u + 256 + kCW / 4;                  // [128] segment of each bin
  hist[lane] = 0;
  hist[lane + 64] = 0;
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int j = 0; j < kPer; ++j)
    if (o.pq[j]) {
      const uint32_t i = (uint32_t)j * 64u + lane;
      const uint32_t xc = first_sub_index(a, db, o.x8[j], o.e8[j]);
      xcs[i] = (uint8_t)xc;
      bseg[xc] = de_seg(o.e8[j]);
      atomicAdd(&hist[xc], 1u);
      S.sk[i] = sk_make(de_seg(o.e8[j]), o.ro[j] & kOpMask, i, o.home8[j]);  // by slot for now
      S.L[i] = (uint8_t)(de_ld(o.e8[j]) | ((o.ro[j] & kGetBit) ? 0x80u : 0u));
    }
  __builtin_amdgcn_wave_barrier();
  // each non-empty bin's lane fetches its segment's bitmap now; the
  // loads land while the ops are sorted
  const uint32_t hv = hist[lane], hv2 = wide ? hist[lane + 64] : 0u;
  uint4 pbm[8];
  if (hv && !wide) {
    const uint32_t* og = a.occ + (size_t)bseg[lane] * 32u;
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) pbm[jj] = ld_u4_l2(og + 4 * jj);
  }
  stamp(srow, kBsBinned, lane == 0);
  // batch order without a comparison sort: k_part tiles are 4096
  // consecutive ops, and a bucket holds ~0-2 ops per tile, so a
  // counting sort by the op's tile bin (256 bins) leaves only tiny bins
  // to order by op (insertion sort, one lane per bin)
  uint32_t* th = S.u + 448;     // [256] per-bin counts, then offsets
  uint32_t* o32 = S.u + 704;    // [kCW] keys (op << 8 | slot) in batch order
  static_assert(704 + kCW <= kBmWords, "sort scratch");
  {
    const uint32_t lgn = 32u - (uint32_t)__builtin_clz((uint32_t)max<uint64_t>(a.n - 1, 1));
    const uint32_t tsh = max(12u, lgn > 8u ? lgn - 8u : 0u);
#pragma unroll
    for (int t = 0; t < 4; ++t) th[4 * lane + t] = 0;
    __builtin_amdgcn_wave_barrier();
    uint32_t tb[kPer], tr[kPer];
#pragma unroll
    for (int j = 0; j < kPer; ++j)
      if (o.pq[j]) {
        tb[j] = min((o.ro[j] & kOpMask) >> tsh, 255u);
        tr[j] = atomicAdd(&th[tb[j]], 1u);
      }
    __builtin_amdgcn_wave_barrier();
    uint32_t c4[4], s4 = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      c4[t] = th[4 * lane + t];
      s4 += c4[t];
    }
    uint32_t tot;
    uint32_t ex = wave_excl_scan(s4, &tot);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      th[4 * lane + t] = ex;
      ex += c4[t];
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int j = 0; j < kPer; ++j)
      if (o.pq[j]) o32[th[tb[j]] + tr[j]] = ((o.ro[j] & kOpMask) << 8) | ((uint32_t)j * 64u + lane);
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (c4[t] < 2) continue;
      const uint32_t b0 = th[4 * lane + t], b1 = b0 + c4[t];
      for (uint32_t x = b0 + 1; x < b1; ++x) {  // insertion sort by (op, slot)
        const uint32_t v = o32[x];
        uint32_t y = x;
        while (y > b0 && o32[y - 1] > v) {
          o32[y] = o32[y - 1];
          --y;
        }
        o32[y] = v;
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
  stamp(srow, kBsBatchOrder, lane == 0);
  uint32_t rx, nruns;
  {  // bins: exclusive offsets; the non-empty ones are the runs
    uint32_t tot;
    const uint32_t ex = wave_excl_scan(hv + hv2, &tot);  // bins lane, lane + 64 in turn
    cur[lane] = ex;
    cur[lane + 64] = ex + hv;
    rx = wave_excl_scan((hv ? 1u : 0u) + (hv2 ? 1u : 0u), &nruns);
    if (hv) S.runq[rx] = (uint16_t)ex;
    if (hv2) S.runq[rx + (hv ? 1u : 0u)] = (uint16_t)(ex + hv);
    if (lane == 0) S.runq[nruns] = (uint16_t)np;
  }
  __builtin_amdgcn_wave_barrier();
  const uint64_t lt = (1ULL << lane) - 1;
  uint64_t skv[kPer];
  uint32_t dst[kPer];
#pragma unroll
  for (int j = 0; j < kPer; ++j) {  // positions j*64 + lane, in batch order
    const uint32_t q = (uint32_t)j * 64u + lane;
    const bool valid = q < np;
    const uint32_t i = valid ? (o32[q] & 0xFFu) : 0u;
    const uint32_t v = valid ? xcs[i] : 0u;
    uint64_t M = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 7; ++b) {
      if (b == 6 && !wide) break;
      const bool bit = (v >> b) & 1u;
      const uint64_t bb = __ballot(bit);
      M &= bit ? bb : ~bb;
    }
    const uint32_t base = cur[v];
    dst[j] = base + (uint32_t)__popcll(M & lt);
    skv[j] = valid ? S.sk[i] : 0ULL;
    __builtin_amdgcn_wave_barrier();
    if (valid && lane == 63u - (uint32_t)__builtin_clzll(M)) cur[v] = base + (uint32_t)__popcll(M);
    __builtin_amdgcn_wave_barrier();
  }
#pragma unroll
  for (int j = 0; j < kPer; ++j)
    if ((uint32_t)j * 64u + lane < np) S.sk[dst[j]] = skv[j];
  // run rx's bitmap row (the sort scratch above is dead now)
  if (hv && !wide && rx < (uint32_t)kBmLanes) put_bitmap_row(S.u + rx * 33u, pbm);
  __builtin_amdgcn_wave_barrier();
  return nruns;
}

// Ordering by a 64-bit sort of (segment, batch index) keys (wave_sort8) and
// run detection: the same outputs as order_by_bins but the bitmaps.  at: this
// lane's first position among the np pending ops.
template <class Lds>
__device__ __forceinline__ uint32_t order_by_sort(Lds& S, const RoundOps& o, uint32_t at, uint32_t np, bool strided) {
  const uint32_t lane = __lane_id() & 63u;
#pragma unroll
  for (int j = 0; j < kPer; ++j)
    if (o.pq[j]) {
      const uint32_t i = chunk_slot(strided, j);
      S.sk[at++] = sk_make(de_seg(o.e8[j]), o.ro[j] & kOpMask, i, o.home8[j]);
      S.L[i] = (uint8_t)(de_ld(o.e8[j]) | ((o.ro[j] & kGetBit) ? 0x80u : 0u));
    }
  uint32_t p2 = 1;
  while (p2 < np) p2 <<= 1;
  __builtin_amdgcn_wave_barrier();
  if (p2 > 1) wave_sort8(S.sk, p2, np);
  // runs: maximal stretches with one segment
  const uint32_t per_q = (np + 63) / 64;
  uint32_t rc = 0, nruns;
  for (uint32_t j = 0; j < per_q; ++j) {
    const uint32_t q = lane * per_q + j;
    if (q < np && (q == 0 || sk_seg(S.sk[q]) != sk_seg(S.sk[q - 1]))) ++rc;
  }
  uint32_t rat = wave_excl_scan(rc, &nruns);
  for (uint32_t j = 0; j < per_q; ++j) {
    const uint32_t q = lane * per_q + j;
    if (q < np && (q == 0 || sk_seg(S.sk[q]) != sk_seg(S.sk[q - 1]))) S.runq[rat++] = (uint16_t)q;
  }
  if (lane == 0) S.runq[nruns] = (uint16_t)np;
  return nruns;
}

// One lane per run, kBmLanes runs at a time, in batch order inside each run.
// Insert-only batches only DECIDE slots here (S.pos); the pairs are written
// by every lane afterwards.  Mixed batches store at once: a later Get of the
// run must see them.  pre_bm: the first kBmLanes runs' bitmaps are in LDS.
template <bool FINAL, bool MIXED>
__device__ __forceinline__ void apply_runs(const RunCtx& rc, BucketLds<FINAL, !FINAL && !MIXED>& S, uint32_t nruns,
                                           bool pre_bm, WaveStat& c) {
  const uint32_t lane = __lane_id() & 63u;
  for (uint32_t r0 = 0; r0 < nruns; r0 += kBmLanes) {
    const uint32_t r = r0 + lane;
    if (lane >= (uint32_t)kBmLanes || r >= nruns) continue;
    const uint2 cw = apply_run<FINAL, MIXED>(rc, S, S.runq[r], S.runq[r + 1], pre_bm && r < (uint32_t)kBmLanes);
    c.lines += cw.x;
    c.waited += cw.y;
  }
  __builtin_amdgcn_wave_barrier();
}

// ---- the claim write-outs

// REG: each lane writes its own ops' claimed pairs from registers
template <class Lds>
__device__ __forceinline__ void store_claims_reg(const BucketArgs& a, Lds& S, const RoundOps& o, const ChunkRegs& r) {
  const uint32_t lane = __lane_id() & 63u;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    if (!o.pq[j]) continue;
    const uint32_t i = (uint32_t)j * 64u + lane;
    const uint32_t pos = S.pos[i];
    if (pos != 0xFFFFu) {
      a.pairs[(size_t)de_seg(o.e8[j]) * kSlots + pos] = make_ulonglong2(r.k[j], r.v[j]);
      S.pos[i] = 0xFFFF;
      S.pend[i] = 0;  // (the fast claim loop leaves it set)
    }
  }
}
// Mixed apply passes: the claims the run loops left unstored (runs that never
// reached the general loop), with their status
template <class Lds>
__device__ __forceinline__ void store_claims_mixed(const BucketArgs& a, Lds& S, uint32_t np) {
  if (a.upsert) return;
  for (uint32_t q = __lane_id() & 63u; q < np; q += 64) {
    const uint64_t sk = S.sk[q];
    const uint32_t i = sk_item(sk);
    const uint32_t pos = S.pos[i];
    if (pos != 0xFFFFu) {
      a.pairs[(size_t)sk_seg(sk) * kSlots + pos] = S.kv[i];
      a.st[sk_op(sk)] = 2;  // PMDFC_ST_INSERTED
      S.pos[i] = 0xFFFF;
    }
  }
}
// Insert-only final pass: the claimed pairs from LDS, all lanes (loads first,
// then stores)
template <class Lds>
__device__ __forceinline__ void store_claims_lds(const BucketArgs& a, Lds& S, uint32_t np) {
  const uint32_t lane = __lane_id() & 63u;
  for (uint32_t q0 = 0; q0 < np; q0 += 256) {
    uint64_t kq[4], vq[4];
    uint32_t aq[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const uint32_t q = q0 + u * 64 + lane;
      aq[u] = 0xFFFFFFFFu;
      if (q < np) {
        const uint64_t sk = S.sk[q];
        const uint32_t i = sk_item(sk);
        const uint32_t pos = S.pos[i];
        if (pos != 0xFFFFu) {
          aq[u] = sk_seg(sk) * kSlots + pos;
          const ulonglong2 kv = S.kv[i];
          kq[u] = kv.x;
          vq[u] = kv.y;
          S.pos[i] = 0xFFFF;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (aq[u] != 0xFFFFFFFFu) a.pairs[aq[u]] = make_ulonglong2(kq[u], vq[u]);
  }
}

// REG parking: the ops a full window left pending (S.pend 2) go to the
// bucket's wait list, copied by their owner lanes
template <class Lds>
__device__ __forceinline__ void park_pending_reg(Lds& S, const RoundOps& o, const ChunkRegs& r, ulonglong2* wl_kv,
                                                 uint32_t* wl_op) {
  const uint32_t lane = __lane_id() & 63u;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const uint32_t i = (uint32_t)j * 64u + lane;
    if (o.pq[j] && S.pend[i] == 2) {
      const uint32_t k = atomicAdd(&S.nsplit, 1u);
      wl_kv[k] = make_ulonglong2(r.k[j], r.v[j]);
      wl_op[k] = r.op[j];
    }
  }
}

// Final pass only: the round's ns queued splits, inline.  First the
// sub-directory deepens if a child needs more bits (pool exhausted: the
// blocked ops fail with CAPACITY and nothing splits), then each split moves
// its entries (wave_split) and its directory half (dir_split).
__device__ __forceinline__ void grow_and_split(const BucketArgs& a, uint32_t w, BucketLds<true, false>& S, uint32_t ns,
                                               uint32_t& off, uint32_t& db, WaveStat& c, uint64_t* srow) {
  const uint32_t lane = __lane_id() & 63u;
  const uint32_t need = S.need;
  if (need > db) {
    const uint32_t size = 1u << need;
    uint32_t no = 0;
    const bool fx = a.pfix && need <= kFixedBits;  // grows in place in its fixed slot
    if (lane == 0 && !fx) no = atomicAdd(&a.ctl->pool_cur, size);
    no = fx ? w * kFixedSlot : (uint32_t)__shfl((int)no, 0);
    if ((uint64_t)no + size > a.pool_cap) {
      if (lane == 0) atomicOr(&a.ctl->err, 1u);
      for (uint32_t s = lane; s < ns; s += 64) {
        if (S.split[s] == ~0ULL) continue;
        const uint32_t i = (uint32_t)S.split[s] & 0xFFFFu;
        a.st[S.op[i] & kOpMask] = 6;
        S.pend[i] = 0;
      }
      // their child ids are taken: retired empty, so that the arena walks
      // by id find no stale entries under them
      uint32_t nd = 0;
      for (uint32_t s = 0; s < ns; ++s) {
        const uint64_t e = S.split[s];
        if (e == ~0ULL) continue;
        retire_segment(a.pairs, a.occ, a.ldep, (uint32_t)(e >> 21));
        ++nd;
      }
      if (lane == 0 && nd) atomicAdd(&a.ctl->dead, nd);
      __builtin_amdgcn_wave_barrier();
      return;
    }
    grow_subdir(a, w, no, need, off, db);
    ++c.grow;
  }
  for (uint32_t s = 0; s < ns; ++s) {
    const uint64_t e = S.split[s];
    if (e == ~0ULL) continue;  // its child id ran out (CAPACITY)
    const uint32_t i = (uint32_t)e & 0xFFFFu;
    const uint32_t L = (uint32_t)(e >> 16) & 31u;
    const uint32_t c1 = (uint32_t)(e >> 21);
    const uint32_t x = sub_index(hash64(S.kv[i].x), a.sbits, a.p1, db);
    const uint32_t seg = de_seg(ld_u32_l2(a.pool + off + x));
    bool bad = false;
    const uint32_t loss = wave_split(a.pairs, a.occ, a.ldep, seg, c1, L, S.u, &bad, nullptr, a.drops,
                                     &a.ctl->drop_n, S.op[i] & kOpMask);
    dir_split(a, off, db, x, seg, c1, L);
    __builtin_amdgcn_s_waitcnt(0);
    ++c.splits;
    c.loss += loss;
    c.bad += bad;
    c.max_ld = max(c.max_ld, L + 1);
  }
  __builtin_amdgcn_wave_barrier();
  stamp(srow, kBsFinSplit, lane == 0);
}

// One bucket pass of directory bucket w.
// k_apply (FINAL = false, high occupancy, no split code): one round; a run
// blocked by a full window requests a split and parks the rest of the run.
// FIRST takes the bucket's records of the batch, else its parked ops (after
// committing the last split round's splits).
// The final pass (FINAL = true): buckets with parked ops, granted splits or
// too many ops for one chunk; rounds with inline splits until its ops are
// done.  pre_m: the chunk's pre_m ops are already in S.kv / S.op
// (k_mixed_small); kBigBucket: walk the bucket's records (k_medium).
// Returns 0 (a bucket that needs the final pass is listed in fin).
template <bool FINAL, bool MIXED, bool FIRST>
__device__ __forceinline__ uint32_t bucket_body(const BucketArgs& a, const uint32_t w,  // w: directory bucket
                                            BucketLds<FINAL, !FINAL && !MIXED>& S,  // the kernel's LDS
                                            uint32_t pre_m = 0) {
  static_assert(!(FINAL && FIRST), "the final pass is never the first");
  constexpr bool REG = !FINAL && !MIXED;
  const uint32_t lane = __lane_id() & 63u;  // (not threadIdx.x: callers may run several waves per workgroup)
  const uint32_t pb = w >> a.sbb, sub = w & ((1u << a.sbb) - 1);
  uint32_t nw = 0;
  if (!FIRST) {
    nw = (FINAL && pre_m) ? pre_m : a.wl_n[w];
    if (nw == 0 && a.ngrant[w] == 0) return 0u;
    if (!FINAL && nw == kBigBucket) return 0u;  // the final pass takes it (listed by the first pass)
  }
  const bool big = FINAL && nw == kBigBucket;
  ulonglong2* const wl_kv = a.wl_kv + (size_t)w * kCW;
  uint32_t* const wl_op = a.wl_op + (size_t)w * kCW;
  uint64_t* const srow = bucket_stamp_row(a, w);
  if (FIRST) stamp(srow, kBsStart, lane == 0);
  if (FINAL) stamp(srow, kBsFinStart, lane == 0);
  if (FIRST && a.mode == 0) first_pass_clears(a, w);
  // first pass: the first 32 records of each of the bucket's 8 sub-regions
  // and its stat slots are loaded before anything else is known (one round
  // trip with the header and cursor loads instead of three dependent ones)
  const uint32_t csub = sub_count_load(a, pb);
  PreRecs pr;
  if (FIRST) prefetch_records(a, pb, 0, pr);
  const uint64_t wsv = lane < 7u ? a.wstat[(size_t)w * kWStat + lane] : 0ULL;
  uint32_t off, db;
  {
    const uint64_t hd = a.hdr[w];
    off = hdr_off(hd);
    db = hdr_db(hd);
  }
  WaveStat c;
  if (!FIRST) commit_splits(a, w, off, db, c);
  const uint32_t C = a.chunk;
  const uint32_t full = FINAL ? 0u : a.ctl->full;
  LdsDir ldir;
  if constexpr (!FINAL) ldir = lds_dir_load(a, off, db);
  if (lane == 0) {
    S.nsplit = 0;
    S.nreq = 0;
    S.need = db;
  }
  __builtin_amdgcn_wave_barrier();
  const uint32_t cmax = sub_count_max(csub);  // (the prefetch covers 32 of each sub-region)
  const uint32_t novf = *a.ovf;
  const uint32_t ntile = (uint32_t)((a.n + kPartTile - 1) / kPartTile);
  BigLds* BL = nullptr;
  uint32_t bt = 0, bmp = 0;  // big bucket walk position
  if constexpr (FINAL) {
    if (big) {
      BL = big_lds();
      big_index(a, BL, pb, csub, novf, ntile);
    }
  }
  bool first_chunk = true;
  ChunkRegs r;
#pragma unroll
  for (int j = 0; j < kPer; ++j) r.ok[j] = false;
  while (FIRST || nw != 0) {
    // ---- load the chunk
    uint32_t m = 0;
    if (FIRST) {
      m = load_records<REG>(a, S, pb, sub, pr, csub, cmax, novf, C, r);
      if (m > C) {
        if (lane == 0) {
          a.wl_n[w] = kBigBucket;  // too many for one chunk: final pass
          a.fin[(a.par << a.p1) + atomicAdd(&a.ctl->nfin[a.par], 1u)] = w;
        }
        return 0;
      }
    } else if (!big) {
      m = nw;
      if (!(FINAL && pre_m)) load_parked<REG>(wl_kv, wl_op, m, S, r);
      __builtin_amdgcn_wave_barrier();
    } else {
      if constexpr (FINAL) m = big_chunk(a, BL, pb, sub, ntile, C, bt, bmp, S.kv, S.op);
      if (m == 0) break;
    }
    if (first_chunk && (FINAL || FIRST)) stamp(srow, FINAL ? kBsFinLoaded : kBsLoaded, lane == 0);
    mark_pending<REG>(S, m, r);
    uint32_t rounds = 0;
    const bool strided = REG || (!FINAL && ldir.on);
    for (uint32_t round = 0; m > 0; ++round) {
      uint64_t* const srow0 = (first_chunk && round == 0) ? srow : nullptr;  // round 0 of the first chunk is stamped
      // ---- the pending ops and their directory entries
      RoundOps o;
      uint32_t np;
      const uint32_t at = wave_excl_scan(gather_pending<REG>(S, r, m, strided, o), &np);
      if (np == 0) break;
      if (round >= kRoundGuard) {
        fail_pending(a, S, strided, o);
        break;
      }
      ++rounds;
      lookup_entries<FINAL>(a, S, off, db, ldir, o);
      if constexpr (REG) {
        // insert-only passes on a sub-directory of <= 32 entries: claims in
        // parallel (fast_claim); false = a segment with too many interacting
        // ops, nothing done yet: the sorted run loop below takes the round
        if ((1u << db) <= kFastBins && !a.upsert) {
          const auto bin = [&](int j) -> uint32_t { return first_sub_index(a, db, o.x8[j], o.e8[j]); };
          if (fast_claim<kCW, kFastBins>(a, w, S.u, S.key, wl_kv, wl_op, &S.nsplit, &S.nreq, &S.need,
                                         LaneOps{r.k, r.v, r.op, o.pq, o.e8, o.home8, o.x8}, bin, c,
                                         FIRST ? srow0 : nullptr))
            break;  // (an apply pass is one round)
        }
      }
      // ---- order them into runs, one per segment, each in batch order
      const bool wide = db > 6;
      uint32_t nruns;
      if (!FINAL && ldir.on) nruns = order_by_bins(a, S, o, np, db, wide, FIRST ? srow0 : nullptr);
      else nruns = order_by_sort(S, o, at, np, strided);
      if (lane == 0 && FINAL) {
        S.nsplit = 0;
        S.need = db;
      }
      __builtin_amdgcn_wave_barrier();
      if (FINAL || FIRST) stamp(srow0, FINAL ? kBsFinOrdered : kBsOrdered, lane == 0);
      c.runs += lane == 0 ? nruns : 0;
      // ---- apply the runs
      const RunCtx rc{a.pairs, a.occ, a.vout, a.st, a.ctl, a.req + (size_t)w * kSplitCap,
                      a.reqop + (size_t)w * kSplitCap, a.mixed, a.max_segments, full, (uint32_t)(!FINAL && a.mode == 2),
                      (!FINAL && FIRST) ? srow : nullptr,
                      a.sbits, a.p1, db, a.upsert, (FIRST && a.upsert) ? a.upos : nullptr, wl_kv, wl_op, a.pfix,
                      (uint32_t)a.pool_cap};
      apply_runs<FINAL, MIXED>(rc, S, nruns, !FINAL && ldir.on && !wide, c);
      if (!FINAL && FIRST) stamp(srow0, kBsRunsDone, lane == 0);
      // ---- write the claims
      if constexpr (REG) store_claims_reg(a, S, o, r);
      else if constexpr (MIXED && !FINAL) store_claims_mixed(a, S, np);
      else if constexpr (!MIXED) store_claims_lds(a, S, np);
      if (FINAL) __builtin_amdgcn_s_waitcnt(0);  // the next round re-reads the segments
      __builtin_amdgcn_wave_barrier();
      if (FINAL || FIRST) stamp(srow0, FINAL ? kBsFinWritten : kBsWritten, lane == 0);
      // ---- park (apply passes: one round; parked ops wait for the split round)
      if constexpr (REG) park_pending_reg(S, o, r, wl_kv, wl_op);
      if constexpr (!FINAL) {
        break;
      } else {
        // ---- grow and split inline, then the next round
        const uint32_t ns = min(S.nsplit, kSplitCap);
        if (ns == 0) continue;  // every pending op resolved (or failed) this round
        grow_and_split(a, w, S, ns, off, db, c, srow0);
      }
    }
    c.rounds += rounds;
    c.max_rounds = max(c.max_rounds, rounds);
    first_chunk = false;
    if (!big) break;  // one chunk
  }
  // ---- publish: the wait list, the final-pass list, split requests, stats
  if (!FINAL) {
    // the last parked-op pass requests nothing: what it parks is the final pass's
    const uint32_t to_final = (a.mode == 2 && S.nsplit) ? 1u : 0u;
    if (lane == 0) {
      a.wl_n[w] = S.nsplit;  // parked ops (0: done)
      if (to_final) a.fin[(a.par << a.p1) + atomicAdd(&a.ctl->nfin[a.par], 1u)] = w;
    }
    request_tail(a, w, S.nreq, S.need, db);
  }
  publish_stats(a, w, wsv, c);
  if (FIRST) stamp(srow, kBsEnd, lane == 0);
  if (FINAL) stamp(srow, kBsFinEnd, lane == 0);
  return 0;
}

// insert-only and mixed batches get their own kernels: the run loop of an
// insert-only batch carries no Get / immediate-store paths
__device__ __forceinline__ bool gated_off(const BucketArgs& a) {
  if (a.gate == 0) return false;
  const bool pend = __builtin_nontemporal_load(&a.ctl->pget) == a.gate_tag;
  return a.gate == 1 ? !pend : pend;
}

}  // namespace pmdfc
