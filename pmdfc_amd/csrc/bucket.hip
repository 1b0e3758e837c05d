// bucket.hip -- the batched Insert / mixed path.
//
// A batch runs as a fixed launch sequence on the caller's stream, no host
// round trip:
//
// 1. k_part (part.hip): partition of the batch's pending ops into
//    2^(p1 - sbb) partition buckets by the top local hash bits.
// 2. the first apply pass, ONE WAVE PER DIRECTORY BUCKET: k_apply_fast (the
//    lean insert-only pass: parallel claims, fast_claim) or bucket_body's
//    general pass.  A directory bucket owns its sub-directory (cceh_device.h
//    "Bucketed directory") and every segment in it, so the wave applies its
//    ops with no one to coordinate with (CCEH splits are segment-local,
//    CCEH_hybrid.cpp:171-297): each insert takes the first free slot of its
//    32-slot window in batch order (CCEH_hybrid.cpp:143-168); a segment whose
//    window is full requests a split and parks the rest of its ops; the
//    bucket reserves its child ids and grown sub-directory with sharded
//    atomics (request_splits).
// 3. k_split: one wave per requested split (cluster replay: split_device.h),
//    global ids from the shard offsets.
// 4. k_apply_parked: the requesting buckets commit their splits (directory
//    stride update, sub-directory growth, CCEH_hybrid.cpp:208-286) and apply
//    their parked ops.
// 5. k_bucket, the final pass: whatever is still parked, oversized buckets
//    (records walked tile by tile in batch order), rounds with inline splits
//    until nothing is pending (depth is capped at 30, so it terminates).
// Small batches skip the pipeline: k_mixed_tiny (<= 64 ops), k_mixed_small
// (<= 256) and k_part + k_medium (<= 8192) run the final pass's ordered runs
// directly.
//
// Where it all lives: k_part in part.hip; every other kernel of the path
// here, with its launcher; their device code in wave_util.h, split_device.h
// (a split), bucket_pass.h (bucket_body and its phases) and apply_fast.h (the
// lean first pass).
//
// The 20 kernels here stay ONE translation unit, because cut apart some of
// them get different device code (tools/kernel_code_diff.py compares two
// builds; DESIGN.md §1 has the register figures).  The compiler shapes a
// file's internal device functions after the callers it sees in that file:
// * split_slow takes generic pointers (flat accesses) as long as k_split,
//   whose scratch offset is opaque, is among its callers.  k_split compiles
//   the same on its own, but the kernels it would leave behind (k_bucket,
//   k_medium, k_mixed_small, k_mixed_tiny, k_serve) then pass LDS pointers
//   only: split_slow turns to LDS accesses and they all change.
// * window_all_same: its `mixed` argument is a constant in a file without
//   k_bucket<false> / k_medium<false>, its pointers LDS addresses in a file
//   whose callers are all final-pass kernels (the small batches and k_serve
//   cut apart).
// * window_all_same_reg: with k_apply_fb as its one caller the LDS addresses
//   are folded into it, and k_apply_fb changes.
// * the lean kernels call none of the three, but they share fc_all_same with
//   bucket_body's fast_claim; all of them pass it a null key array.  In a
//   file without bucket_body's insert-only first pass (tried: the lean
//   kernels with and without k_apply_fb) that null is known before inlining
//   and the loop of fc_all_same is simplified earlier: the five lean kernels
//   come out differently (k_apply_fast: a v_cndmask per copy of the loop
//   placed elsewhere; k_apply_fast_cp: 22 SGPR spills for 16).  Seen in the
//   optimized IR, whose only differing blocks are that loop's.
// So every family is tied to another one; only k_part shares no such function.
#include <algorithm>

#include "apply_fast.h"
#include "bucket_pass.h"

namespace pmdfc {

template <bool MIXED>
__global__ __launch_bounds__(64, 2) void k_apply(BucketArgs a) {
  if (gated_off(a)) return;
  __shared__ BucketLds<false, !MIXED> S;
  if (MIXED && a.mseen && blockIdx.x == 0 && threadIdx.x == 0)
    __hip_atomic_store(a.mseen, a.gate_tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  bucket_body<false, MIXED, true>(a, blockIdx.x, S);
}
// The mixed first pass on a small grid looping over the buckets: launched
// when the host expects it gated off (PlanIn::mixed_small), so the exit
// of its few waves is cheap; exact on any grid (the loop needs more registers
// than k_apply's one bucket per wave, hence its own kernel)
__global__ __launch_bounds__(64, 2) void k_apply_mloop(BucketArgs a) {
  if (gated_off(a)) return;
  __shared__ BucketLds<false, false> S;
  if (a.mseen && blockIdx.x == 0 && threadIdx.x == 0)
    __hip_atomic_store(a.mseen, a.gate_tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  for (uint32_t w = blockIdx.x; w < (1u << a.p1); w += gridDim.x) {
    bucket_body<false, true, true>(a, w, S);
    __builtin_amdgcn_wave_barrier();
  }
}
// Hand out what k_split granted (wave 0 of the parked pass): a prefix of the
// requests in shard-major order -- all of them unless the arena or the pool
// ran out (plain stores: no other wave of k_apply_parked reads or allocates
// either counter).
__device__ __forceinline__ void handout(const BucketArgs& a) {
  const GrantScan g = grant_scan(a.gsh, a.par);
  const uint32_t seg0 = a.ctl->nsegs, pool0 = a.ctl->pool_cur;
  uint64_t ns = (uint64_t)seg0 + g.S, np = (uint64_t)pool0 + g.P;
  if (ns > a.max_segments || np > a.pool_cap) {
    ns = seg0;
    np = pool0;
    // rare: walk the buckets in shard-major order.  Segment ids are granted
    // as a prefix (a bucket denied for the pool leaves its ids unused);
    // pool regions too, since their offsets only grow (fixed slots take none)
    for (uint32_t k = 0; k < g.S;) {
      const uint32_t x = split_shard(g, k);
      const uint64_t cpx = g.cp(x);  // (every lane active)
      const uint4 el = a.gsplit[((size_t)a.par * kGShards + x) * a.gcap + (k - g.cs(x))];  // (a bucket's first split)
      const uint32_t nr = el.w & 0xFFu, need = el.w >> 8;
      const uint64_t gs = (uint64_t)seg0 + k + nr;
      if (gs > a.max_segments) break;
      ns = gs;
      if (need && !(a.pfix && need <= kFixedBits)) {
        const uint64_t gp = (uint64_t)pool0 + cpx + el.z + (1ULL << need);
        if (gp <= a.pool_cap) np = max(np, gp);
      }
      k += nr;
    }
  }
  if ((__lane_id() & 63u) == 0) {
    a.ctl->nsegs = (uint32_t)ns;
    a.ctl->pool_cur = (uint32_t)np;
    // the launch-time hint: a system-scope vector store into coherent
    // pinned host memory (the host reads it without a sync)
    if (a.hint) __hip_atomic_store(a.hint, (uint32_t)ns, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// the parked-op passes (mode 1 / 2): the same body under its own name, so
// kernel traces tell the two passes apart
// (over the worklist the grants built: the buckets with split requests)
template <bool MIXED>
__device__ __forceinline__ void parked_pass(const BucketArgs& a, BucketLds<false, !MIXED>& S) {
  const bool req = a.ctl->anyreq[a.par] != 0;
  const bool decl = !MIXED && a.ctl->anydecl[a.par] != 0;
  if (!req && !decl) return;  // no bucket requested a split or was declined: nothing is parked
  const uint32_t na = req ? a.ctl->nact[a.par] : 0u;
  if (req && blockIdx.x == 0) handout(a);
  for (uint32_t k = blockIdx.x; k < na; k += gridDim.x) {
    bucket_body<false, MIXED, false>(a, a.act[k], S);
    __builtin_amdgcn_wave_barrier();
  }
  if constexpr (!MIXED) {
    // the buckets the lean first pass declined, when no k_apply_fb ran for
    // them: their first pass here, after the split round -- buckets are
    // independent, and this pass requests no split (mode 2): what a full
    // window blocks goes to the final pass, which splits inline
    if (decl) {
      for (uint32_t w = blockIdx.x; w < (1u << a.p1); w += gridDim.x) {
        const uint32_t f = a.fbl[w];
        if (!(f & 1u)) continue;
        bucket_body<false, false, true>(a, w, S);
        if (threadIdx.x == 0) a.fbl[w] = f + 1u;  // pending bit off, count + 1
        __builtin_amdgcn_wave_barrier();
      }
    }
  }
}
template <bool MIXED>
__global__ __launch_bounds__(64, 3) void k_apply_parked(BucketArgs a) {
  if (gated_off(a)) return;
  __shared__ BucketLds<false, !MIXED> S;
  parked_pass<MIXED>(a, S);
}
// A gated mixed batch's parked pass as ONE launch (round 6; until then the
// insert-only and the mixed variant were both launched and one exited at
// once): the insert-only body unless k_mixed_get / k_part left a Get pending
// (ar: gate 2), else the mixed body (am: gate 1).  Both bodies fit the
// insert-only one's 3 waves per SIMD; the LDS is the larger of the two.
union ParkedLds {
  BucketLds<false, true> r;
  BucketLds<false, false> m;
};
__global__ __launch_bounds__(64, 3) void k_apply_parked_gated(BucketArgs ar, BucketArgs am) {
  __shared__ ParkedLds U;
  if (!gated_off(ar)) parked_pass<false>(ar, U.r);
  else parked_pass<true>(am, U.m);
}
// (over the buckets the earlier passes left to it)
template <bool MIXED>
__global__ __launch_bounds__(64, 1) void k_bucket(BucketArgs a) {
  __shared__ BucketLds<true, false> S;
  const uint32_t nf = a.ctl->nfin[a.par];
  for (uint32_t k = blockIdx.x; k < nf; k += gridDim.x) {
    bucket_body<true, MIXED, false>(a, a.fin[(a.par << a.p1) + k], S);
    __builtin_amdgcn_wave_barrier();
  }
}

// ------------------------------------------------------------- small batches
//
// k_mixed_small: a whole mixed (or insert-only: ops == null) batch of at most
// kCW ops in ONE launch, for the per-op front-end (host/batch_core.cpp: the
// reference's 32 poll threads calling KV::Insert / Get one op at a time,
// server/rdma_svr.cpp:755, batches of ~14-32 ops).  The general pipeline
// costs ~12 dependent launches per batch however small it is; here every
// block ranks the batch's ops by (directory bucket, batch index) itself and
// takes the blockIdx-th distinct bucket (blocks past the last one exit), so
// no partition pass and no grid-wide step is needed: the bucket's ops, in
// batch order, go straight into the final pass's LDS chunk and bucket_body's
// final pass applies them -- one round per split, splits and sub-directory
// growth inline -- with every Get answered in its segment's ordered run.  So
// results are the serial reference's exactly (no early answers, no
// SPLIT_LOST).  The inputs may be host-mapped (pinned) memory: a block reads
// the keys once for the ranking and its own ops' values.
__global__ __launch_bounds__(64, 1) void k_mixed_small(BucketArgs a, const uint8_t* __restrict__ ops,
                                                       const uint64_t* __restrict__ keys,
                                                       const uint64_t* __restrict__ vin) {
  __shared__ BucketLds<true, false> S;
  __shared__ uint32_t s_rank[kCW];  // (bucket << 8 | op) of the valid ops, ascending
  __shared__ uint32_t s_sel[2];     // this block's bucket, its first rank position
  const uint32_t lane = threadIdx.x, n = (uint32_t)a.n;
  static_assert(kCW <= 256, "op index in 8 bits");
  uint32_t v[kPer];
#pragma unroll
  for (int q = 0; q < kPer; ++q) {
    const uint32_t i = kPer * lane + q;  // wave_sort32's layout
    v[q] = ~0u;
    if (i < n) {
      const uint64_t key = keys[i];
      const uint64_t h = hash64(key);
      const uint8_t bad = reserved_key(key) ? 3 : wrong_shard(h, a.sbits, a.shard) ? 8 : 0;
      if (bad) {
        if (blockIdx.x == 0) {
          a.st[i] = bad;  // PMDFC_ST_RESERVED_KEY / PMDFC_ST_WRONG_SHARD
          if (a.vout) a.vout[i] = 0;  // (insert-only batches pass none)
        }
      } else {
        v[q] = (bucket_of(h, a.sbits, a.p1) << 8) | i;
      }
    }
  }
  wave_sort32<kPer>(v, kCW);
  // distinct buckets in ascending order; this block takes the blockIdx-th
  uint32_t starts = 0;
  const uint32_t prev_last = (uint32_t)__shfl_up((int)v[kPer - 1], 1);
#pragma unroll
  for (int q = 0; q < kPer; ++q) {
    const uint32_t pv = q ? v[q - 1] : (lane ? prev_last : ~0u);
    const bool st = v[q] != ~0u && (pv == ~0u || (pv >> 8) != (v[q] >> 8));
    starts |= st ? 1u << q : 0u;
    s_rank[kPer * lane + q] = v[q];
  }
  uint32_t tot;
  const uint32_t rk0 = wave_excl_scan((uint32_t)__builtin_popcount(starts), &tot);
  if (lane == 0) s_sel[0] = ~0u;
  __builtin_amdgcn_wave_barrier();
  if (blockIdx.x >= tot) return;
  {
    uint32_t r = rk0;
#pragma unroll
    for (int q = 0; q < kPer; ++q)
      if ((starts >> q) & 1u) {
        if (r == blockIdx.x) {
          s_sel[0] = v[q] >> 8;
          s_sel[1] = kPer * lane + q;
        }
        ++r;
      }
  }
  __builtin_amdgcn_wave_barrier();
  const uint32_t w = s_sel[0], e0 = s_sel[1];
  // the bucket's ops, in batch order, into the final pass's chunk
  uint32_t m = 0;
  for (uint32_t t0 = 0; e0 + t0 < kCW; t0 += 64) {
    const uint32_t t = t0 + lane;
    const uint32_t e = e0 + t < kCW ? s_rank[e0 + t] : ~0u;
    const bool mine = e != ~0u && (e >> 8) == w;
    const uint64_t bal = __ballot(mine);
    m += (uint32_t)__popcll(bal);
    if (mine) {
      const uint32_t i = e & 0xFFu;
      const bool ins = !ops || ops[i] == 1;  // PMDFC_OP_INSERT
      S.kv[t] = make_ulonglong2(keys[i], ins ? vin[i] : 0ULL);
      S.op[t] = i | (ins ? 0u : kGetBit);
      if (ins && a.vout) a.vout[i] = 0;
    }
    if (bal != ~0ULL) break;  // past the bucket
  }
  __builtin_amdgcn_wave_barrier();
  bucket_body<true, true, false>(a, w, S, m);
}

// k_mixed_tiny: a batch of at most 64 ops (the blocking front-end's usual
// 14-32) by ONE wave, a lane per op in batch order.  An op that is the only
// one of the batch on its segment is applied on its own lane at once: a Get
// probes the window (nothing of this batch changes that segment), an Insert
// takes the first free slot of its window -- exactly what the serial
// reference does, since nothing else of the batch touches the segment and a
// split of another segment never moves it.  The rest -- ops sharing a segment,
// an Insert whose window is full (it splits), every Insert in upsert mode --
// go through the final pass's ordered runs (bucket_body), one directory
// bucket at a time, in batch order within each: the same exact path as
// k_mixed_small.  Common case: key -> header -> sub-directory entry ->
// occupancy words or window line -> store, four dependent round trips in all.
// (the body, also the serving kernel's: lane i holds op i of the n <= 64 in
// registers; results go to a.st[i], a.vout[i])
// hdr_cache (nullable): the directory bucket headers in LDS (the serving
// wave's copy); returns whether the ordered path ran (it may have changed
// headers: the copy is stale then)
__device__ __forceinline__ bool tiny_batch(const BucketArgs& a, BucketLds<true, false>& S, uint32_t n, bool in,
                                           uint64_t key, bool ins, uint64_t val,
                                           const uint64_t* hdr_cache = nullptr) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t h = hash64(key);
  bool live = false;
  if (in) {
    const uint8_t bad = reserved_key(key) ? 3 : wrong_shard(h, a.sbits, a.shard) ? 8 : 0;
    if (bad) {
      a.st[lane] = bad;  // PMDFC_ST_RESERVED_KEY / PMDFC_ST_WRONG_SHARD
      if (a.vout) a.vout[lane] = 0;
    }
    live = !bad;
  }
  const uint32_t w = live ? bucket_of(h, a.sbits, a.p1) : 0u;
  uint32_t e = 0;
  if (live) {
    const uint64_t hd = hdr_cache ? hdr_cache[w] : a.hdr[w];
    e = ld_u32_l2(a.pool + hdr_off(hd) + sub_index(h, a.sbits, a.p1, hdr_db(hd)));
  }
  const uint32_t seg = de_seg(e);
  // another live op of the batch on my segment?
  const uint64_t lv = __ballot(live);
  bool shared = false;
  for (uint64_t m = lv; m; m &= m - 1) {
    const int j = __builtin_ctzll(m);
    const uint32_t sj = (uint32_t)__shfl((int)seg, j);  // (every lane: a shuffle reads active lanes only)
    shared |= (uint32_t)j != lane && sj == seg;
  }
  bool general = live && (shared || (ins && a.upsert));
  if (live && !general) {
    ulonglong2* sp = a.pairs + (size_t)seg * kSlots;
    if (!ins) {
      uint64_t v = 0;
      const uint8_t st = lane_probe(sp, key, h, &v);
      a.vout[lane] = v;
      a.st[lane] = st;
    } else {
      const uint32_t wi0 = (uint32_t)(h & 0xFF) * 4u, wi = wi0 >> 5;
      uint32_t* og = a.occ + (size_t)seg * 32u;
      const uint2 ow = window_words(ld_window_l2(og, wi), wi);
      const uint32_t lo = ow.x, hi = ow.y;
      const int pos = window_first_free(lo, hi, wi0);
      if (pos < 0) {
        general = true;  // full window: the ordered path splits
      } else {
        sp[pos] = make_ulonglong2(key, val);
        const uint32_t pw = (uint32_t)pos >> 5;
        og[pw] = (pw == wi ? lo : hi) | (1u << ((uint32_t)pos & 31u));
        a.st[lane] = 2;  // PMDFC_ST_INSERTED
        if (a.vout) a.vout[lane] = 0;
      }
    }
  }
  // the rest, bucket by bucket, in batch order within each
  const bool any_general = __ballot(general) != 0;
  for (uint64_t gm = __ballot(general); gm;) {
    const uint32_t wb = (uint32_t)__shfl((int)w, __builtin_ctzll(gm));
    const uint64_t mine = __ballot(general && w == wb);
    if (general && w == wb) {
      const uint32_t t = (uint32_t)__popcll(mine & ((1ULL << lane) - 1));
      S.kv[t] = make_ulonglong2(key, val);
      S.op[t] = lane | (ins ? 0u : kGetBit);
      if (ins && a.vout) a.vout[lane] = 0;
    }
    __builtin_amdgcn_s_waitcnt(0);  // (the direct stores land before the bucket's runs read)
    __builtin_amdgcn_wave_barrier();
    bucket_body<true, true, false>(a, wb, S, (uint32_t)__popcll(mine));
    __builtin_amdgcn_wave_barrier();
    gm &= ~mine;
  }
  return any_general;
}

__global__ __launch_bounds__(64, 1) void k_mixed_tiny(BucketArgs a, const uint8_t* __restrict__ ops,
                                                      const uint64_t* __restrict__ keys,
                                                      const uint64_t* __restrict__ vin) {
  __shared__ BucketLds<true, false> S;
  const uint32_t lane = threadIdx.x, n = (uint32_t)a.n;
  const bool in = lane < n;
  const uint64_t key = in ? keys[lane] : kInvalid;
  const bool ins = in && (!ops || ops[lane] == 1);  // PMDFC_OP_INSERT
  const uint64_t val = ins ? vin[lane] : 0ULL;
  tiny_batch(a, S, n, in, key, ins, val);
}

constexpr uint32_t kServeHdrMax = 1024;  // directory buckets the serving wave caches in LDS (8 KB)
constexpr uint64_t kServeWatchdog = 100000000ull;  // wall_clock64 ticks (100 MHz): ~1 s without a heartbeat
constexpr uint64_t kServeIdle = 100000ull;         // ~1 ms without ops: raise ctl->idle (callers on a CPU-
                                                   // quota'd host pause for longer than 100 us at times)

// ------------------------------------------------------------ serving kernel
//
// k_serve: the per-op front-end's device side (host/batch_core.cpp, served
// mode).  The server's caller threads (up to 32 RDMA poll threads calling
// KV::Insert / Get one op at a time, server/rdma_svr.cpp:755-835) publish
// their ops straight into a ring in coherent pinned host memory; ONE
// persistent wave takes the longest published prefix (at most 64 ops)
// in ring order, applies it exactly as k_mixed_tiny does (the serial
// reference, every Get in its ordered run), bumps the attached counting
// bloom filter for the inserts that count (KV::Insert's bf->Insert,
// server/KV.cpp:113-114), and writes each op's {value, status, sequence
// word} into the response ring: the caller that spins on that word reads its
// result without any host thread in between -- no launch, no completion
// event, no wake-up.
// After ~1 ms without ops it raises ctl->idle (and lowers it when ops come
// again): the host then stops it, so a device-wide synchronisation elsewhere
// in the process never waits on an idle wave.  It exits when the host sets
// ctl->stop, or when the host's heartbeat word has not moved for ~1 s (a host
// that died must not leave a spinning wave); either way it clears ctl->alive
// last.
__device__ __forceinline__ uint32_t sys_ld32(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ uint64_t sys_ld64(const uint64_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ void sys_st32(uint32_t* p, uint32_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ void sys_st64(uint64_t* p, uint64_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

__global__ __launch_bounds__(64, 1) void k_serve(ServeArgs sa) {
  __shared__ BucketLds<true, false> S;
  const uint32_t lane = threadIdx.x;
  const uint64_t mask = sa.ring_size - 1;
  // several waves: wave w serves ring w, whose ops all fall in the directory
  // buckets with the top log2(nwaves) bucket bits == w (the host routes each
  // op by its hash): no two waves touch one segment, a sub-directory or a
  // header (splits take their ids and pool regions with atomics)
  if (sa.nwaves > 1) {
    sa.req += (size_t)blockIdx.x * sa.ring_size;
    sa.resp += (size_t)blockIdx.x * sa.ring_size;
    sa.ctl += blockIdx.x;
    sa.head0 = sys_ld64(&sa.ctl->head);
  }
  uint64_t head = sa.head0, chunks = 0, reloads = 0;
  uint64_t hb = sys_ld64(&sa.ctl->heartbeat);
  uint64_t t_hb = (uint64_t)wall_clock64(), t_last = t_hb;
  bool idle_set = false;
  uint64_t tp[5] = {0, 0, 0, 0, 0};  // ticks: read, count BF, apply, answer; empty polls
  const uint64_t t_start = t_hb;
  // head, chunks and the profile every 64 chunks and at exit (the host reads
  // head only to restart a wave that stopped)
  const auto put_prof = [&] {
    const uint64_t life = (uint64_t)wall_clock64() - t_start;
    if (lane < 6)
      sys_st64(&sa.ctl->prof[lane],
               lane == 0 ? tp[0] : lane == 1 ? tp[1] : lane == 2 ? tp[2] : lane == 3 ? tp[3] : lane == 4 ? tp[4] : life);
    if (lane == 6) sys_st64(&sa.ctl->head, head);
    if (lane == 7) sys_st64(&sa.ctl->chunks, chunks);
    if (lane == 8) sys_st64(&sa.ctl->reloads, reloads);
  };
  // results are staged in LDS (no device-memory round trip to read them back)
  __shared__ uint8_t s_st[64];
  __shared__ uint64_t s_vout[64];
  BucketArgs ab = sa.a;
  ab.st = s_st;
  ab.vout = s_vout;
  // the directory bucket headers in LDS (one dependent round trip less per
  // op), reloaded after a chunk whose ordered path may have changed them
  __shared__ uint64_t s_hdr[kServeHdrMax];
  const uint32_t nhdr = 1u << ab.p1;
  const uint64_t* hc = nhdr <= kServeHdrMax ? s_hdr : nullptr;
  const auto load_hdr = [&] {
    for (uint32_t b = lane; b < nhdr; b += 64u) s_hdr[b] = ab.hdr[b];
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
  };
  if (hc) load_hdr();
  bool hdr_stale = false;
  // the request ring through a buffer resource: 16-B loads at system scope
  // (sc0 sc1), both halves of 64 places and the stop word in one round trip
  const __amdgpu_buffer_rsrc_t rq =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<pmdfc_serve_req*>(sa.req), 0, 0x7fffffff, 0x00020000);
  u32x4_t qlo, qhi;
  uint32_t stop;
  const auto poll = [&](uint64_t h) {
    const uint32_t off = (uint32_t)(((h + lane) & mask) * sizeof(pmdfc_serve_req));
    stop = sys_ld32(&sa.ctl->stop);
    qlo = __builtin_amdgcn_raw_buffer_load_b128(rq, off, 0, 0x11);
    qhi = __builtin_amdgcn_raw_buffer_load_b128(rq, off + 16u, 0, 0x11);
  };
  poll(head);
  for (uint32_t idle = 0;;) {
    if (stop) break;
    const uint64_t p = head + lane;
    const uint32_t want = ((uint32_t)p + 1u) & 0x3FFFFFFFu;
    const bool ready = qlo.z == qhi.z && (qlo.z >> 2) == want;  // both halves of place p written
    const uint64_t rb = __ballot(ready);
    const uint32_t n = ~rb ? (uint32_t)__builtin_ctzll(~rb) : 64u;  // the published prefix
    if (n == 0) {
      ++tp[4];
      // idle: back off; every 64 polls check that the host still beats
      if ((++idle & 63u) == 0) {
        const uint64_t h2 = sys_ld64(&sa.ctl->heartbeat), now = (uint64_t)wall_clock64();
        if (h2 != hb) {
          hb = h2;
          t_hb = now;
        } else if (now - t_hb > kServeWatchdog) {
          break;
        }
        if (!idle_set && now - t_last > kServeIdle) {
          idle_set = true;
          if (lane == 0) sys_st32(&sa.ctl->idle, 1u);
        }
      }
      __builtin_amdgcn_s_sleep(4);
      poll(head);
      continue;
    }
    idle = 0;
    const uint64_t c0 = (uint64_t)wall_clock64();
    t_last = c0;
    if (idle_set) {
      idle_set = false;
      if (lane == 0) sys_st32(&sa.ctl->idle, 0u);
    }
    const bool in = lane < n;
    const uint64_t key = in ? ((uint64_t)qlo.y << 32) | qlo.x : kInvalid;
    const uint32_t op = in ? qlo.z & 3u : 0u;
    const bool ins = in && (op & 1u) == PMDFC_SERVE_INSERT;
    const uint64_t val = ins ? ((uint64_t)qhi.y << 32) | qhi.x : 0ULL;
    const uint64_t c1 = c0;
    // the earlier chunks rewrote table lines this CU may hold in its L1 (the
    // headers are read with plain loads): an acquire at agent scope drops them
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    if (hc && hdr_stale) {
      load_hdr();
      ++reloads;
    }
    if (sa.cbf && ins && (op & PMDFC_SERVE_CBF)) cbf_increment(sa.cbf, sa.cbf_m, sa.cbf_k, key);
    __builtin_amdgcn_s_waitcnt(0);
    const uint64_t c2 = (uint64_t)wall_clock64();
    hdr_stale = tiny_batch(ab, S, n, in, key, ins, val, hc);
    // the results in LDS (not the table stores: they complete under the next
    // poll, which the release below waits for anyway; this wave's later loads
    // of the same lines are ordered behind them)
    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0) only (gfx9 encoding)
    __builtin_amdgcn_wave_barrier();
    const uint64_t c3 = (uint64_t)wall_clock64();
    // each answer is ONE 16-B store {value, status | seq << 32} (one bus
    // write per op)
    if (in) {
      const uint8_t st = s_st[lane];
      const uint64_t v = !ins && st == 1 ? s_vout[lane] : 0ULL;
      const u64x2_t w = {v, (uint64_t)st | ((uint64_t)(uint32_t)(p + 1) << 32)};
      __builtin_nontemporal_store(w, reinterpret_cast<u64x2_t*>(sa.resp + (p & mask)));
    }
    head += n;
    ++chunks;
    // the next chunk's poll travels with the answers (the release below waits
    // for both)
    poll(head);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");  // (system scope: the answers leave now)
    const uint64_t c4 = (uint64_t)wall_clock64();
    tp[0] += c1 - c0;
    tp[1] += c2 - c1;
    tp[2] += c3 - c2;
    tp[3] += c4 - c3;
    if ((chunks & 63u) == 0) put_prof();
  }
  put_prof();
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
  if (lane == 0) sys_st32(&sa.ctl->alive, 0u);
}

// k_medium: a mixed / insert batch of at most kPartTile ops after its
// one-block partition: block i takes the i-th partition bucket that received
// ops (blocks past the last exit) and runs each of its directory buckets
// through the final pass with every record walked in batch order (the
// oversized-bucket walk of bucket_body: chunks of whole tiles, here the one
// tile) -- rounds with inline splits, Gets answered in their ordered runs, so
// the serial reference's results exactly.  Two launches per batch instead of
// the general pipeline's ~12; the async front-end's batches of ~1-4k ops.
// The blocks also zero the other parity's cursors for the next batch.
template <bool MIXED>
__global__ __launch_bounds__(64, 1) void k_medium(BucketArgs a, const uint32_t* __restrict__ touched) {
  __shared__ BucketLds<true, false> S;
  const uint32_t lane = threadIdx.x, npb = 1u << (a.p1 - a.sbb);
  for (uint32_t i = blockIdx.x * 64u + lane; i < npb * kPartSubs; i += gridDim.x * 64u) a.cursor_next[i] = 0;
  if (blockIdx.x == 0 && lane == 0) *a.ovf_next = 0;
  const uint32_t nt = touched[0];
  for (uint32_t k = blockIdx.x; k < nt; k += gridDim.x) {
    const uint32_t pb = touched[1 + k];
    for (uint32_t sub = 0; sub < (1u << a.sbb); ++sub) {
      bucket_body<true, MIXED, false>(a, (pb << a.sbb) | sub, S, kBigBucket);
      __builtin_amdgcn_wave_barrier();
    }
  }
}

// ---------------------------------------------------------------- split round

constexpr uint32_t kSplitWaves = 4;      // waves per k_split workgroup

// One wave per requested split, in shard-major order: split k is request i of
// bucket w; its child id is the segment counter at the start of the pass + k
// (the shards' segment offsets are exactly the prefix sums of the requests)
// and the bucket's grown sub-directory, if any, sits at the pool counter + the
// pools of the shards before + its offset in its shard.  A bucket whose
// requests do not fit max_segments / the pool is denied whole (ctl->full: the
// parked pass fails its ops with CAPACITY); both offsets only grow in
// shard-major order, so the grants are a prefix (k_apply_parked then sets the
// counters).  The wave of a bucket's first request also grants it and lists
// it for the parked pass.
__global__ __launch_bounds__(64 * kSplitWaves, 2) void k_split(SplitArgs a) {
  if (a.ctl->anyreq[a.par] == 0) return;
  __shared__ uint32_t s_scr[kSplitWaves][kSplitScratch];
  const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const GrantScan g = grant_scan(a.gsh, a.par);
  const uint32_t seg0 = a.ctl->nsegs, pool0 = a.ctl->pool_cur;
  if (blockIdx.x == 0 && threadIdx.x == 0) a.ctl->nact[a.par] = g.E;
  // a short split list (by default at most one split per workgroup): the
  // workgroup's four waves split together (split_team<4>: a quarter of the
  // loads and stores each), else one wave per split
  const bool team = g.S <= a.team_max;
  uint32_t loss = 0, bad = 0;
  const uint32_t k0 = team ? blockIdx.x : blockIdx.x * kSplitWaves + wv;
  const uint32_t ks = team ? gridDim.x : gridDim.x * kSplitWaves;
  for (uint32_t k = k0; k < g.S; k += ks) {
    const uint32_t x = split_shard(g, k);
    // (the cross-lane reads with every lane active)
    const uint32_t csx = g.cs(x), cex = g.ce(x);
    const uint64_t cpx = g.cp(x);
    const uint4 el = a.gsplit[((size_t)a.par * kGShards + x) * a.gcap + (k - csx)];
    const uint32_t w = el.y & 0x3FFFu, i = (el.y >> 14) & 63u, nr = el.w & 0xFFu, need = el.w >> 8;
    const bool fx = a.pfix && need && need <= kFixedBits;  // grows in its fixed slot: no pool
    const uint64_t gs = (uint64_t)seg0 + k - i, gp = fx ? (uint64_t)w * kFixedSlot : (uint64_t)pool0 + cpx + el.z;
    const bool ok = gs + nr <= a.max_segments && (fx || gp + (need ? 1ULL << need : 0ULL) <= a.pool_cap);
    if (i == 0 && lane == 0 && (!team || wv == 0)) {
      a.gbase[w] = (uint32_t)gs;
      a.ngrant[w] = ok ? nr : 0u;
      a.newoff[w] = (uint32_t)gp;
      a.need[w] = need;
      a.act[cex + (el.y >> 20)] = w;
      if (!ok) a.ctl->full = 1;
    }
    if (!ok) {  // (uniform over a team: one k)
      // denied for the pool with its ids inside the granted prefix (handout
      // counts them): each request's child id is retired empty
      if (gs + nr <= a.max_segments && (!team || wv == 0)) {
        retire_segment(a.pairs, a.occ, a.ldep, seg0 + k);
        if (lane == 0) atomicAdd(&a.ctl->dead, 1u);
      }
      continue;
    }
    bool b = false;
    uint64_t* stp = a.stamps && k < kSplitStamps ? a.stamps + (size_t)k * 8 : nullptr;
    stamp(stp, kSsStart, lane == 0 && (!team || wv == 0));
    const uint32_t trig = a.drops ? a.reqop[(size_t)w * kSplitCap + i] : 0u;
    const uint32_t ps = el.x & ((1u << 27) - 1), pl = el.x >> 27;
    if (team) {
      loss += split_team<4>(a.pairs, a.occ, a.ldep, ps, seg0 + k, pl, &s_scr[0][0], &b, stp, a.drops, &a.ctl->drop_n,
                            trig, wv);
    } else {
      // an opaque scratch offset per iteration: otherwise the split's LDS
      // addresses are hoisted out of the loop into ~60 VGPRs
      uint32_t so = wv * kSplitScratch;
      __asm__ volatile("" : "+v"(so));
      loss += wave_split(a.pairs, a.occ, a.ldep, ps, seg0 + k, pl, &s_scr[0][0] + so, &b, stp, a.drops,
                         &a.ctl->drop_n, trig);
    }
    bad |= b;
  }
  if (lane == 0 && (!team || wv == 0)) {  // (a team's total is on every wave: wave 0 reports it)
    if (loss) {
      atomicAdd(reinterpret_cast<unsigned long long*>(&a.ctl->split_loss), (unsigned long long)loss);
      atomicAdd(&a.ctl->loss_events, 1u);
    }
    if (bad) atomicOr(&a.ctl->err, 4u);
  }
}

// k_split's arguments for the split round of the batch whose passes take `a`
static SplitArgs split_args(const BucketArgs& a, uint64_t* stamps, uint32_t team_max) {
  SplitArgs p;
  p.par = a.par;
  p.pfix = a.pfix;
  p.stamps = stamps;
  p.gsh = a.gsh;
  p.gsplit = a.gsplit;
  p.gcap = a.gcap;
  p.act = a.act;
  p.gbase = a.gbase;
  p.ngrant = a.ngrant;
  p.newoff = a.newoff;
  p.need = a.need;
  p.max_segments = a.max_segments;
  p.pool_cap = a.pool_cap;
  p.pairs = a.pairs;
  p.occ = a.occ;
  p.ldep = a.ldep;
  p.ctl = a.ctl;
  p.reqop = a.reqop;
  p.drops = a.drops;
  p.team_max = team_max;
  return p;
}

__global__ __launch_bounds__(64, 8) void k_apply_fast(BucketArgs a) {
  if (gated_off(a)) return;
  __shared__ FastLds<false> S;
  // a declined bucket is flagged in its own word (bit 0; bits 1+ count the
  // declines for stats): no shared counter, since in a table whose every
  // bucket declines 8,192 atomics on one word would serialize (~88 per us)
  if (apply_fast<false>(a, S, blockIdx.x) != 0 && threadIdx.x == 0) declined(a, blockIdx.x);
}

// the coarse-partition lean first pass: a workgroup of 8 waves per partition
// bucket, wave v taking directory bucket (partition bucket << 3) | v
#ifndef PMDFC_CP_WPE
#define PMDFC_CP_WPE 8  // (A/B builds) minimum waves per SIMD: 8 caps it at 64 VGPRs
#endif
__global__ __launch_bounds__(64 * kCpWaves) __attribute__((amdgpu_waves_per_eu(PMDFC_CP_WPE, 8))) void k_apply_fast_cp(
    BucketArgs a) {
  if (gated_off(a)) return;
  __shared__ CpLds L;
  // (the wave's index through readfirstlane: wave-uniform, so w and every
  // address derived from it live in scalar registers)
  const uint32_t v = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), w = (blockIdx.x << kCpSbb) | v;
  if (apply_fast<false, false, true>(a, L.w[v], w, &L) != 0 && (threadIdx.x & 63u) == 0) declined(a, w);
}

// the lean first pass for large tables (the host picks it from the table's
// segments per bucket, pmdfc_cceh::wide): sub-directories up to 128 entries
__global__ __launch_bounds__(64, 6) void k_apply_wide(BucketArgs a) {
  if (gated_off(a)) return;
  __shared__ FastLds<true> S;
  if (apply_fast<true>(a, S, blockIdx.x) != 0 && threadIdx.x == 0) declined(a, blockIdx.x);
}

// the lean first passes in last-writer-wins mode (insert-only batches)
template <bool WIDE>
__global__ __launch_bounds__(64, 5) void k_apply_fast_ups(BucketArgs a) {
  __shared__ FastLds<WIDE> S;
  if (apply_fast<WIDE, true>(a, S, blockIdx.x) != 0 && threadIdx.x == 0) declined(a, blockIdx.x);
}

// the buckets k_apply_fast / k_apply_wide declined: bucket_body's general
// first pass, the same wave per bucket (the others exit after one load).  At
// config 2 it flags nothing and costs one empty launch.
__global__ __launch_bounds__(64, 2) void k_apply_fb(BucketArgs a) {
  if (gated_off(a)) return;
  const uint32_t w = blockIdx.x, f = a.fbl[w];
  if (!(f & 1u)) return;
  __shared__ BucketLds<false, true> S;
  bucket_body<false, false, true>(a, w, S);
  if (threadIdx.x == 0) a.fbl[w] = f + 1u;  // pending bit off, count + 1
}

// ------------------------------------------------------------- launchers
// The batch's LaunchPlan (launch_plan.h) names each pass's kernel, gate and
// grid; a launcher adds the kernel's workgroup size and the pass's mode.
static BucketArgs pass_args(const BucketLaunch& L, uint32_t mode, uint32_t gate) {
  BucketArgs a = L.a;
  a.mode = mode;
  a.gate = gate;
  return a;
}

void launch_first(const BucketLaunch& L, hipStream_t s) {
  if (!L.a.n) return;
  const LaunchPlan& p = L.plan;
  const BucketArgs ar = pass_args(L, 0, p.first_gate), am = pass_args(L, 0, p.mixed_gate);
  const dim3 g(p.first_grid), gm(p.mixed_grid), b(64);
  switch (p.first) {
    case FirstPass::kNone: break;
    case FirstPass::kFastCp: hipLaunchKernelGGL(k_apply_fast_cp, g, dim3(64 * kCpWaves), 0, s, ar); break;
    case FirstPass::kWide: hipLaunchKernelGGL(k_apply_wide, g, b, 0, s, ar); break;
    case FirstPass::kFast: hipLaunchKernelGGL(k_apply_fast, g, b, p.first_lds, s, ar); break;
    case FirstPass::kFastUps: hipLaunchKernelGGL(k_apply_fast_ups<false>, g, b, 0, s, ar); break;
    case FirstPass::kFastUpsWide: hipLaunchKernelGGL(k_apply_fast_ups<true>, g, b, 0, s, ar); break;
    case FirstPass::kGeneral: hipLaunchKernelGGL(k_apply<false>, g, b, 0, s, ar); break;
  }
  switch (p.mixed) {
    case MixedPass::kNone: break;
    case MixedPass::kApply: hipLaunchKernelGGL(k_apply<true>, gm, b, 0, s, am); break;
    case MixedPass::kLoop: hipLaunchKernelGGL(k_apply_mloop, gm, b, 0, s, am); break;
  }
}

void launch_fallback(const BucketLaunch& L, hipStream_t s) {
  if (!L.a.n || !L.plan.fb) return;
  hipLaunchKernelGGL(k_apply_fb, dim3(1u << L.a.p1), dim3(64), 0, s, pass_args(L, 0, L.plan.fb_gate));
}

void launch_split_round(const BucketLaunch& L, hipStream_t s) {
  if (!L.a.n) return;
  hipLaunchKernelGGL(k_split, dim3(L.plan.split_grid), dim3(64 * kSplitWaves), 0, s,
                     split_args(L.a, L.split_stamps, L.plan.team_max));
}

void launch_parked(const BucketLaunch& L, hipStream_t s) {
  if (!L.a.n) return;
  const dim3 g(L.plan.parked_grid), b(64);
  switch (L.plan.parked) {
    case ParkedPass::kInsert: hipLaunchKernelGGL(k_apply_parked<false>, g, b, 0, s, pass_args(L, 2, 0)); break;
    case ParkedPass::kMixed: hipLaunchKernelGGL(k_apply_parked<true>, g, b, 0, s, pass_args(L, 2, 0)); break;
    case ParkedPass::kGated:  // (both variants as two launches: configs 3 / 4 7.17-7.25 / 6.04-6.06 against 7.31-7.34 / 6.12-6.15)
      hipLaunchKernelGGL(k_apply_parked_gated, g, b, 0, s, pass_args(L, 2, 2), pass_args(L, 2, 1));
      break;
  }
}

void launch_final(const BucketLaunch& L, hipStream_t s) {
  if (!L.a.n) return;
  const dim3 g(L.plan.final_grid), b(64);
  switch (L.plan.fin) {
    case FinalPass::kInsert: hipLaunchKernelGGL(k_bucket<false>, g, b, 0, s, L.a); break;
    case FinalPass::kMixed: hipLaunchKernelGGL(k_bucket<true>, g, b, 0, s, L.a); break;
  }
}

void launch_mixed_small(const BucketArgs& a, const uint8_t* ops, const uint64_t* keys, const uint64_t* vin,
                        hipStream_t s) {
  if (!a.n) return;
  if (a.n <= 64) {
    hipLaunchKernelGGL(k_mixed_tiny, dim3(1), dim3(64), 0, s, a, ops, keys, vin);
    return;
  }
  const uint32_t grid = (uint32_t)std::min<uint64_t>(a.n, 1ULL << a.p1);  // >= the distinct buckets
  hipLaunchKernelGGL(k_mixed_small, dim3(grid), dim3(64), 0, s, a, ops, keys, vin);
}

void launch_serve(const ServeArgs& sa, hipStream_t s) {
  hipLaunchKernelGGL(k_serve, dim3(sa.nwaves), dim3(64), 0, s, sa);
}

void launch_medium(const BucketArgs& a, const uint32_t* touched, hipStream_t s) {
  if (!a.n) return;
  const uint32_t npb = 1u << (a.p1 - a.sbb);
  const dim3 g((uint32_t)std::min<uint64_t>(std::max<uint64_t>(a.n, 64), npb));  // >= the touched buckets
  if (a.mixed) hipLaunchKernelGGL(k_medium<true>, g, dim3(64), 0, s, a, touched);
  else hipLaunchKernelGGL(k_medium<false>, g, dim3(64), 0, s, a, touched);
}

}  // namespace pmdfc
