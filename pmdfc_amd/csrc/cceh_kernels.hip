// cceh_kernels.hip -- hand-written gfx950 kernels of the batched CCEH engine:
// the Get path (one quad per key), the mixed-batch pre-pass, table init and
// small utilities.  The Insert path is in part.hip (the partition) and
// bucket.hip (per-bucket apply / split).
//
// Batch semantics: ops are applied as if run serially in batch
// order on CCEH_hybrid.  A segment's contents depend only on the subsequence
// of ops whose hash falls in its key range, so each segment's ops are applied
// in batch order by one lane, segments in parallel.
#include "cceh_device.h"
#include "cceh_kernels.h"
#include "knobs.h"

#include <algorithm>
#include <cstdlib>

namespace pmdfc {

// ---------------------------------------------------------------- get path
// Pure-Get batch: 4 lanes per key, 64 keys per 256-thread block.
template <bool COUNT>
__global__ __launch_bounds__(256) void k_get(const uint64_t* __restrict__ keys,
                                             uint64_t* __restrict__ vout,
                                             uint8_t* __restrict__ st, uint64_t n, Geo g,
                                             const ulonglong2* __restrict__ pairs,
                                             uint32_t* __restrict__ line_partials) {
  const uint64_t op = ((uint64_t)blockIdx.x * 256u + threadIdx.x) >> 2;
  const uint32_t q = threadIdx.x & 3u;
  uint32_t lines = 0;
  if (op < n) {
    const uint64_t key = keys[op];
    const uint64_t h = hash64(key);
    uint64_t val = 0;
    uint8_t s;
    if (reserved_key(key)) {
      s = 3;  // PMDFC_ST_RESERVED_KEY
    } else if (wrong_shard(h, g.sbits, g.shard)) {
      s = 8;  // PMDFC_ST_WRONG_SHARD
    } else {
      const uint32_t seg = de_seg(dir_entry(g, h));
      s = quad_probe(pairs + (size_t)seg * kSlots, key, h, q, &val, &lines);
    }
    if (q == 0) {
      if (st) {
        vout[op] = val;
        st[op] = s;
      } else {  // routing response record
        reinterpret_cast<ulonglong2*>(vout)[op] = make_ulonglong2(val, (unsigned long long)s);
      }
    }
  }
  if (COUNT) {
    __shared__ uint32_t red[4];
    uint32_t v = (q == 0) ? lines : 0;
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) line_partials[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
  }
}

// Pure-Get batch, U independent keys per quad (ops q, q+Q, q+2Q, ... with Q =
// quads in the grid): the U key loads, directory loads and first window-line
// loads are issued back to back, so each wave keeps U x 16 random lines in
// flight instead of 16.  Most Gets finish on the first line (L ~ 1.02); the
// rest continue one key at a time.
template <int U, bool COUNT>
__global__ __launch_bounds__(256) void k_get_u(const uint64_t* __restrict__ keys,
                                               uint64_t* __restrict__ vout,
                                               uint8_t* __restrict__ st, uint64_t n, Geo g,
                                               const ulonglong2* __restrict__ pairs,
                                               uint32_t* __restrict__ line_partials, uint32_t p2on,
                                               uint32_t rounds) {
  const uint64_t nq = (uint64_t)gridDim.x * 64u;
  const uint64_t q0 = ((uint64_t)blockIdx.x * 256u + threadIdx.x) >> 2;
  const uint32_t q = threadIdx.x & 3u;
  const uint32_t qbase = (threadIdx.x & 63u) & ~3u;
  uint32_t lines = 0;
  // (a capped grid: every quad takes `rounds` x U Gets, U at a time)
  for (uint32_t r = 0; r < rounds; ++r) {
  uint64_t key[U], h[U];
  uint32_t seg[U];
  uint8_t s[U];
  bool live[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const uint64_t op = q0 + ((uint64_t)r * U + (uint64_t)u) * nq;
    live[u] = op < n;
    key[u] = live[u] ? keys[op] : kInvalid;
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    h[u] = hash64(key[u]);
    s[u] = 0;
    if (live[u] && reserved_key(key[u])) {
      s[u] = 3;
      live[u] = false;
    } else if (live[u] && wrong_shard(h[u], g.sbits, g.shard)) {
      s[u] = 8;
      live[u] = false;
    }
    seg[u] = live[u] ? de_seg(dir_entry(g, h[u])) : 0u;
  }
  // An even home line is the first half of a 128-B HBM line: the window's
  // second 64-B line comes with it (same request), so it is loaded too and a
  // Get that runs past its home line continues without a dependent round
  // trip.  (Odd home lines: the second line is in the next 128-B line.)
  ulonglong2 p[U], p2[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const uint32_t l0 = (uint32_t)(h[u] & 0xFF);
    const ulonglong2* sp = pairs + (size_t)seg[u] * kSlots + l0 * 4u + q;
    if (live[u]) p[u] = sp[0];
    p2[u] = live[u] && p2on && !(l0 & 1u) ? sp[4] : make_ulonglong2(kInvalid, 0);
  }
  uint64_t val[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    val[u] = 0;
    if (!live[u]) continue;
    const uint32_t mn = (uint32_t)(__ballot(p[u].x == key[u]) >> qbase) & 0xFu;
    const uint32_t en = (uint32_t)(__ballot(p[u].x == kInvalid) >> qbase) & 0xFu;
    const uint32_t line0 = (uint32_t)(h[u] & 0xFF);
    const bool has2 = p2on && !(line0 & 1u);  // the second line was loaded with the first
    uint32_t m1 = 0, e1 = 0;
    if (!mn && !en && has2) {
      m1 = (uint32_t)(__ballot(p2[u].x == key[u]) >> qbase) & 0xFu;
      e1 = (uint32_t)(__ballot(p2[u].x == kInvalid) >> qbase) & 0xFu;
    }
    if (mn) {
      val[u] = shfl64(p[u].y, (int)(qbase + (uint32_t)__builtin_ctz(mn)));
      s[u] = 1;
      lines += 1;
    } else if (en) {
      lines += 1;
    } else if (m1) {
      val[u] = shfl64(p2[u].y, (int)(qbase + (uint32_t)__builtin_ctz(m1)));
      s[u] = 1;
      lines += 2;
    } else if (e1) {
      lines += 2;
    } else {
      // rare: continue the window from its second (even home: third) line
      const ulonglong2* sp = pairs + (size_t)seg[u] * kSlots;
      uint32_t t = has2 ? 2 : 1;
      for (; t < kLines; ++t) {
        const ulonglong2 pp = sp[((line0 + t) & 255u) * 4u + q];
        const uint32_t m2 = (uint32_t)(__ballot(pp.x == key[u]) >> qbase) & 0xFu;
        const uint32_t e2 = (uint32_t)(__ballot(pp.x == kInvalid) >> qbase) & 0xFu;
        if (m2) {
          val[u] = shfl64(pp.y, (int)(qbase + (uint32_t)__builtin_ctz(m2)));
          s[u] = 1;
          break;
        }
        if (e2) break;
      }
      lines += (t < kLines ? t + 1 : kLines);
    }
  }
  if (q == 0) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint64_t op = q0 + ((uint64_t)r * U + (uint64_t)u) * nq;
      if (op < n) {
        if (st) {
          vout[op] = val[u];
          st[op] = s[u];
        } else {  // routing response record
          reinterpret_cast<ulonglong2*>(vout)[op] = make_ulonglong2(val[u], (unsigned long long)s[u]);
        }
      }
    }
  }
  }
  if (COUNT) {
    __shared__ uint32_t red[4];
    uint32_t v = (q == 0) ? lines : 0;
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) line_partials[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
  }
}

// ------------------------------------------------------------ mixed batches

#ifndef PMDFC_BULK_CLEAR_SHIFT
#define PMDFC_BULK_CLEAR_SHIFT 4  // (A/B builds) the verify pass clears the whole set past (slots >> this) entries
#endif
constexpr uint32_t kBulkClearShift = PMDFC_BULK_CLEAR_SHIFT;
constexpr uint32_t kWrapLine = (kSlots - kWindow) / 4 + 1;  // home lines >= this: the window wraps

// ---- mixed batches, two exact ways to tell a Get whether the batch inserts
// its key (the host picks one per batch, cceh_engine.hip mixed_join_mode):
//   * the INSERT set (k_mixed_prep + k_mixed_get_iset): every insert of the
//     batch puts its key into a device-wide set (a CAS each), and the Gets that
//     need it probe the set -- cheap when the batch inserts little (config 3:
//     5 % inserts);
//   * the JOIN (k_mixed_get + k_mixed_join, round 6): the Gets that need it
//     claim their keys instead, and every insert looks its key up in that much
//     smaller set -- ~500k random CASes fewer in a half-insert batch (config 4).
// Pre-pass of a mixed batch: hash, reserved key / wrong shard, and the batch's
// set of inserted keys (open addressing, load <= 1/2): the first insert of a
// key stores its batch position, a later one flags the key as inserted more
// than once.  The set is empty on entry (the previous mixed batch's verify
// pass cleared the slots it used, islot); each op's early flag starts at 0,
// and thread 0 opens the batch's drop log.  Each block counts its inserts
// (icount) for the verify pass's choice of how to empty the set.
__global__ __launch_bounds__(256) void k_mixed_prep(const MixedArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i == 0) {
    *a.loss0 = a.ctl->loss_events;
    a.ctl->drop_n = 0;  // the batch's drop log starts empty
  }
  __shared__ uint32_t s_ins;
  if (threadIdx.x == 0) s_ins = 0;
  __syncthreads();
  if (i < a.n) {
  const uint64_t key = a.keys[i];
  const uint64_t h = hash64(key);
  uint8_t s = kStPending;
  if (reserved_key(key)) s = 3;
  else if (wrong_shard(h, a.g.sbits, a.g.shard)) s = 8;
  a.st[i] = s;
  a.vout[i] = 0;
  a.early[i] = 0;
  uint32_t my = 0xFFFFFFFFu;
  const bool ins = s == kStPending && a.ops[i] == 1;
  if (ins) {
    for (uint64_t sl = iset_slot(h, a.imask);; sl = (sl + 1) & a.imask) {
      const uint64_t prev = atomicCAS((unsigned long long*)&a.iset[sl], (unsigned long long)kInvalid,
                                      (unsigned long long)key);
      if (prev == kInvalid) {  // the only insert of this key so far: its position
        a.ipos[sl] = (uint32_t)i;
        my = (uint32_t)sl;
        break;
      }
      if (prev == key) {  // inserted more than once in this batch
        a.icnt[sl] = 1u;
        my = (uint32_t)sl;
        break;
      }
    }
  }
  a.islot[i] = my;
  const uint64_t b = __ballot(ins);
  if ((threadIdx.x & 63u) == 0 && b) atomicAdd(&s_ins, (uint32_t)__popcll(b));
  }
  __syncthreads();
  if (threadIdx.x == 0) a.icount[blockIdx.x] = s_ins;  // (k_mixed_get_iset sums them into ctl->ins_total)
}

// ---- Early answers of a mixed batch's Gets, against the pre-batch image
// (k_mixed_get_iset, k_mixed_get).  A Get of a key the batch never inserts
// keeps its pre-batch answer wherever it sits in the batch: inserts of other
// keys only take free slots, and splits move entries without changing what a
// probe returns for a key with one copy.  A miss stays a miss (nothing adds
// the key); a single-copy hit keeps its value unless a split of this batch
// drops it (CCEH_hybrid.cpp:24-27, split_loss) -- k_mixed_verify checks that.
// Keys with several copies (a split may reorder them) stay pending.
//   A single-copy hit whose window does not wrap (home line < kWrapLine) is
// answered WITHOUT asking whether the batch inserts the key again (early 3):
// every slot of a window before a stored entry, in probe order, is occupied
// (an entry is placed at the first free slot, by Insert and by Split's replay
// alike, and slots are freed only by Erase, which restores exactly this before
// it returns, erase.hip), so a new copy lands after the old one;
// and a split replays a non-wrapping window in slot order = probe order,
// placing every entry at the first free slot, so two copies keep their order
// (the later one's slot is past the earlier one's) and a dropped copy drops
// every later copy too.  The pre-batch copy stays the first copy in probe
// order -- the reference's Get -- until a split of the batch drops it;
// k_mixed_verify places those drops through the drop log (and only then looks
// at the batch's inserts of the key).
//   The other Gets -- a hit in a wrapping window (y >= 996: a split can replay
// it out of probe order), a hit under last-writer-wins (an insert overwrites),
// a miss -- depend on whether the batch inserts their key: each mode finds
// that out its own way (below).  A Get left pending is answered by the
// batch's ordered bucket passes; ctl->pget = tag tells them one is left (else
// the insert-only passes run).
//   A 256-thread block takes 256 consecutive ops: their pending Gets are
// compacted in LDS and its 64 quads take them round-robin, up to kMgU each,
// every quad's key, directory and first window-line loads issued back to
// back for kMgU of them at a time (the inserts cost no quad).

// The block's pending Gets, compacted into LDS: s_list[x] the x-th one's
// thread (its op: the block's first + s_list[x]), s_key[x] its key, *s_cnt how
// many.  Every thread of the block, between the barrier after *s_cnt = 0 and
// the one before the list is read: its op is a pending Get of key k0, or not.
__device__ __forceinline__ void list_pending_get(uint8_t* s_list, uint64_t* s_key, uint32_t* s_cnt, bool isget,
                                                 uint64_t k0) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t bal = __ballot(isget);
  uint32_t wb = 0;
  if (lane == 0 && bal) wb = atomicAdd(s_cnt, (uint32_t)__popcll(bal));
  wb = (uint32_t)__shfl((int)wb, 0);
  if (isget) {
    const uint32_t x = wb + (uint32_t)__popcll(bal & ((1ULL << lane) - 1));
    s_list[x] = (uint8_t)threadIdx.x;
    s_key[x] = k0;
  }
}

// Mixed batches read the bucketed directory (pmdfc_cceh::geo has no flat
// copy).  Saying so at compile time drops dir_entry's flat branch, and with it
// a uniform load that a struct's unqualified pointers do not let the compiler
// prove unclobbered by the kernel's own stores.
__device__ __forceinline__ Geo bucketed(Geo g) {
  g.flat = nullptr;
  return g;
}

// A quad's next kMgU Gets, entries quad + 64 (g0 + u) of the ng listed, their
// loads staged kMgU at a time: here op (base: the block's first op) and key
// from LDS, then hash and directory entry (seg); window_lines is the third
// stage.
template <int kMgU>
__device__ __forceinline__ void stage_gets(const uint8_t* s_list, const uint64_t* s_key, uint32_t ng, const MixedArgs& a,
                                           uint64_t base, uint32_t g0, bool (&live)[kMgU], uint64_t (&op)[kMgU],
                                           uint64_t (&key)[kMgU], uint64_t (&h)[kMgU], uint32_t (&seg)[kMgU]) {
  const uint32_t quad = threadIdx.x >> 2;
  const Geo g = bucketed(a.g);
#pragma unroll
  for (int u = 0; u < kMgU; ++u) {
    const uint32_t idx = quad + 64u * (g0 + (uint32_t)u);
    live[u] = idx < ng;
    op[u] = base + (live[u] ? s_list[idx] : 0u);
    key[u] = live[u] ? s_key[idx] : kInvalid;
  }
#pragma unroll
  for (int u = 0; u < kMgU; ++u) {
    h[u] = hash64(key[u]);
    seg[u] = de_seg(live[u] ? dir_entry(g, h[u]) : 0u);
  }
}
// One Get's home line p (l0, in segment seg) and the window's second line p2.
// An even home line's 128-B HBM line holds the second line too (k_get_u):
// loaded with it, so the copy count continues without a dependent round trip
// (odd: p2 stays invalid).
__device__ __forceinline__ void window_lines(const ulonglong2* seg, uint32_t l0, uint32_t q, bool live,
                                             ulonglong2& p, ulonglong2& p2) {
  const ulonglong2* sp = seg + l0 * 4u + q;
  p = live ? sp[0] : make_ulonglong2(kInvalid, 0);
  p2 = live && !(l0 & 1u) ? sp[4] : make_ulonglong2(kInvalid, 0);
}

// Copies of the key in its window, from the lines window_lines loaded (pp,
// pn): what quad_probe_once tells (0, 1, 2 for several; val: the first copy's
// value, on every lane of the quad), but not that probe: past the preloaded
// lines it goes on one line per round trip, not two -- few Gets get there,
// so the loop stays rolled.
struct WindowCopies {
  uint32_t copies;
  uint64_t val;
};
__device__ __forceinline__ WindowCopies window_copies(const ulonglong2* seg, uint64_t key, uint32_t line0,
                                                      uint32_t q, ulonglong2 pp, ulonglong2 pn) {
  const uint32_t qbase = (threadIdx.x & 63u) & ~3u;
  WindowCopies w{0, 0};
  bool have2 = !(line0 & 1u);  // pn holds the second line
#pragma nounroll
  for (uint32_t t = 0;;) {
    const uint32_t mn = (uint32_t)(__ballot(pp.x == key) >> qbase) & 0xFu;
    const uint32_t en = (uint32_t)(__ballot(pp.x == kInvalid) >> qbase) & 0xFu;
    if (mn && w.copies == 0) w.val = shfl64(pp.y, (int)(qbase + (uint32_t)__builtin_ctz(mn)));
    w.copies += (uint32_t)__builtin_popcount(mn);
    if (en || w.copies > 1 || ++t == kLines) break;
    if (have2) pp = pn;
    else pp = seg[((line0 + t) & 255u) * 4u + q];
    have2 = false;
  }
  if (w.copies > 2) w.copies = 2;
  return w;
}

// a non-wrapping single-copy hit stands whatever the batch inserts (above)
__device__ __forceinline__ void answer_unchecked_hit(const MixedArgs& a, uint64_t o, uint64_t val) {
  a.vout[o] = val;
  a.st[o] = 1;
  a.early[o] = 3;
}

// Block 0, every thread: the batch's pending inserts, summed over the blocks'
// counts, for the host's choice of the next batch's mode (a system-scope
// vector store into coherent pinned memory) and, in insert-set mode, for
// k_mixed_verify's choice of how to empty the set (ctl->ins_total).
__device__ __forceinline__ void sum_inserts(const MixedArgs& a, bool total) {
  __shared__ uint32_t s_sum[4];
  const uint32_t nblk = (uint32_t)((a.n + 255) / 256);
  uint32_t c = 0;
#pragma unroll 4
  for (uint32_t j = threadIdx.x; j < nblk; j += 256u) c += a.icount[j];
  for (int o = 32; o > 0; o >>= 1) c += (uint32_t)__shfl_down((int)c, o);
  if ((threadIdx.x & 63u) == 0) s_sum[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t tot = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
    if (total) a.ctl->ins_total = tot;
    if (a.hint_ins) __hip_atomic_store(a.hint_ins, tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// The INSERT set's Gets, after k_mixed_prep set every status and filled the
// set.  The Gets that depend on the batch's inserts of their key probe the
// set: a hit that needs it (a wrapping window, or last-writer-wins) loads its
// first two set slots up front, with its window lines; a miss probes it after
// its window.
//   A key the batch inserts exactly once, absent before the batch: if the
// insert comes after this Get the key is still absent (miss now); if before,
// the Get returns that insert's value if it was stored (resolved after the
// batch, kStLinked).  Anything else (copies before the batch, several
// inserts) stays pending.
template <int kMgU>
__global__ __launch_bounds__(256) void k_mixed_get_iset(const MixedArgs a) {
  __shared__ uint8_t s_list[256];
  __shared__ uint64_t s_key[256];
  __shared__ uint32_t s_cnt;
  const uint64_t base = (uint64_t)blockIdx.x * 256u;  // the block's first op
  if (threadIdx.x == 0) s_cnt = 0;
  __syncthreads();
  {
    // the block's keys are read with its statuses (coalesced, one round trip)
    const uint64_t i = base + threadIdx.x;
    const bool in = i < a.n;
    const uint8_t s0 = in ? a.st[i] : 0, o0 = in ? a.ops[i] : 1;
    const uint64_t k0 = in ? a.keys[i] : kInvalid;
    list_pending_get(s_list, s_key, &s_cnt, s0 == kStPending && o0 != 1, k0);
  }
  if (blockIdx.x == 0) sum_inserts(a, true);  // (block-uniform)
  __syncthreads();
  const uint32_t ng = s_cnt, quad = threadIdx.x >> 2, q = threadIdx.x & 3u;
  bool pending = false;
  for (uint32_t g0 = 0; g0 < 4u && quad + 64u * g0 < ng; g0 += (uint32_t)kMgU) {
  uint64_t op[kMgU], key[kMgU], h[kMgU], iv[kMgU], iv1[kMgU], sl0[kMgU];
  uint32_t seg[kMgU];
  bool live[kMgU], pre[kMgU];
  ulonglong2 p[kMgU], p2[kMgU];
  stage_gets<kMgU>(s_list, s_key, ng, a, base, g0, live, op, key, h, seg);
#pragma unroll
  for (int u = 0; u < kMgU; ++u) {
    sl0[u] = iset_slot(h[u], a.imask);
    const uint32_t l0 = (uint32_t)(h[u] & 0xFF);
    pre[u] = live[u] && (a.ups != 0 || l0 >= kWrapLine);
    iv[u] = pre[u] ? a.iset[sl0[u]] : kInvalid;
    iv1[u] = pre[u] ? a.iset[(sl0[u] + 1) & a.imask] : kInvalid;
    window_lines(a.pairs + (size_t)seg[u] * kSlots, l0, q, live[u], p[u], p2[u]);
  }
#pragma unroll
  for (int u = 0; u < kMgU; ++u) {
    if (!live[u]) continue;  // quad-uniform
    const uint32_t line0 = (uint32_t)(h[u] & 0xFF);
    const WindowCopies w = window_copies(a.pairs + (size_t)seg[u] * kSlots, key[u], line0, q, p[u], p2[u]);
    const uint8_t c = (uint8_t)w.copies;
    const uint64_t o = op[u];
    if (!pre[u]) {
      if (c == 2) {
        pending = true;
        continue;
      }
      if (c == 1) {
        if (q == 0) answer_unchecked_hit(a, o, w.val);
        continue;
      }
      iv[u] = a.iset[sl0[u]];  // a miss: the set after all
      iv1[u] = a.iset[(sl0[u] + 1) & a.imask];
    }
    // the batch's inserted-key set (linear probing from the first slot)
    uint64_t sl = ~0ull;
    for (uint64_t s1 = sl0[u], v = iv[u], t = 0;; ++t) {
      if (v == key[u]) {
        sl = s1;
        break;
      }
      if (v == kInvalid) break;
      s1 = (s1 + 1) & a.imask;
      v = t == 0 ? iv1[u] : a.iset[s1];
    }
    if (sl != ~0ull) {
      if (c != 0 || a.icnt[sl] != 0) {
        pending = true;
      } else if (q == 0) {
        const uint32_t ps = a.ipos[sl];
        if ((uint64_t)ps > o) {
          a.vout[o] = 0;
          a.st[o] = 0;
        } else {
          a.st[o] = kStLinked;
          a.early[o] = 2;
          a.elink[o] = ps;
        }
      }
    } else if (c == 2) {
      pending = true;
    } else if (q == 0) {
      a.vout[o] = c ? w.val : 0;
      a.st[o] = c ? 1 : 0;
      a.early[o] = c;
    }
  }
  }
  if (pending && q == 0) a.ctl->pget = a.tag;  // every writer stores the same word
}

// The JOIN's Gets, in the batch's first kernel (it also sets every op's
// status: reserved key, wrong shard, pending).  The Gets that depend on the
// batch's inserts of their key only mark their key's bit in a small filter
// (one per XCD: kJoinReps replicas, so a hot key's marks spread over 8 words;
// no-return atomics, nothing waits for them) and leave their probe result
// with status kStJoin; k_mixed_join then puts into the key set only the
// inserts whose filter bit is set (the joined keys and the filter's false
// positives: a few thousand CASes per config-4 batch instead of ~500k),
// counting them per key with the first position, and k_part resolves each
// kStJoin Get from the set:
//   * no insert of the key: the probe result stands (early 1 for a hit);
//   * a miss whose key the batch inserts exactly once: before the insert a
//     miss, after it linked to the insert (kStLinked, resolved after the batch:
//     the insert's value if it was stored);
//   * anything else: pending.
__device__ __forceinline__ uint32_t jbit_of(uint64_t h) { return (uint32_t)(h >> 24) & (kJoinBits - 1u); }

template <int kMgU>
__global__ __launch_bounds__(256) void k_mixed_get(const MixedArgs a) {
  __shared__ uint8_t s_list[256];
  __shared__ uint64_t s_key[256];
  __shared__ uint32_t s_cnt, s_ins;
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t base = (uint64_t)blockIdx.x * 256u;  // the block's first op
  if (threadIdx.x == 0) {
    s_cnt = 0;
    s_ins = 0;
    if (blockIdx.x == 0) {
      *a.loss0 = a.ctl->loss_events;
      a.ctl->drop_n = 0;  // the batch's drop log starts empty
    }
  }
  __syncthreads();
  {
    // every op's status (coalesced), and the pending Gets' keys kept in LDS
    const uint64_t i = base + threadIdx.x;
    const bool in = i < a.n;
    const uint8_t o0 = in ? a.ops[i] : 1;
    const uint64_t k0 = in ? a.keys[i] : kInvalid;
    uint8_t s0 = kStPending;
    if (in) {
      const uint64_t h0 = hash64(k0);
      if (reserved_key(k0)) s0 = 3;
      else if (wrong_shard(h0, a.g.sbits, a.g.shard)) s0 = 8;
      a.st[i] = s0;
      a.vout[i] = 0;
      a.early[i] = 0;
      a.islot[i] = 0xFFFFFFFFu;
    }
    list_pending_get(s_list, s_key, &s_cnt, in && s0 == kStPending && o0 != 1, k0);
    const uint64_t bins = __ballot(in && s0 == kStPending && o0 == 1);
    if (lane == 0 && bins) atomicAdd(&s_ins, (uint32_t)__popcll(bins));
  }
  __syncthreads();
  const uint32_t ng = s_cnt, quad = threadIdx.x >> 2, q = threadIdx.x & 3u;
  const uint32_t rep = blockIdx.x & (kJoinReps - 1u);
  bool pending = false, join = false;
  for (uint32_t g0 = 0; g0 < 4u && quad + 64u * g0 < ng; g0 += (uint32_t)kMgU) {
  uint64_t op[kMgU], key[kMgU], h[kMgU];
  uint32_t seg[kMgU];
  bool live[kMgU];
  ulonglong2 p[kMgU], p2[kMgU];
  stage_gets<kMgU>(s_list, s_key, ng, a, base, g0, live, op, key, h, seg);
#pragma unroll
  for (int u = 0; u < kMgU; ++u)
    window_lines(a.pairs + (size_t)seg[u] * kSlots, (uint32_t)(h[u] & 0xFF), q, live[u], p[u], p2[u]);
#pragma unroll
  for (int u = 0; u < kMgU; ++u) {
    if (!live[u]) continue;  // quad-uniform
    const uint32_t line0 = (uint32_t)(h[u] & 0xFF);
    const WindowCopies w = window_copies(a.pairs + (size_t)seg[u] * kSlots, key[u], line0, q, p[u], p2[u]);
    const uint64_t o = op[u];
    if (w.copies > 1) {  // several copies: the ordered passes (st stays pending)
      pending = true;
      continue;
    }
    if (w.copies == 1 && !a.ups && line0 < kWrapLine) {
      if (q == 0) answer_unchecked_hit(a, o, w.val);
      continue;
    }
    // a joining Get: its probe result, its key's filter bit (no return)
    if (q == 0) {
      a.vout[o] = w.copies ? w.val : 0;
      a.early[o] = (uint8_t)w.copies;
      a.st[o] = kStJoin;
      const uint32_t jb = jbit_of(h[u]);
      atomicOr(&a.jbits[(size_t)(jb >> 5) * kJoinReps + rep], 1u << (jb & 31u));
    }
    join = true;
  }
  }
  if (pending && q == 0) a.ctl->pget = a.tag;  // every writer stores the same word
  if (join && q == 0) a.ctl->njoin = a.tag;
  __syncthreads();
  if (threadIdx.x == 0) a.icount[blockIdx.x] = s_ins;  // (k_mixed_join sums them: the host's mode hint)
}

// The inserts' side of the join (see k_mixed_get): a pending insert whose
// key's bit is set in any filter replica (the 8 words of one bit are
// adjacent: one 32-B load) puts its key into the set, counts itself there and
// keeps the first position (ipos starts at ~0: k_mixed_verify leaves every
// slot it empties that way).  Exits at once when no Get of the batch joined.
// Block 0 sums the batch's inserts for the host (the next batch's mode).
__global__ __launch_bounds__(256) void k_mixed_join(const MixedArgs a) {
  static_assert(kJoinReps == 8, "one 32-B filter load per key");
  // the op's loads issued with the control word's (three round trips in all:
  // these, the filter, the set)
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  const bool in = i < a.n;
  const uint8_t o0 = in ? a.ops[i] : 0, st0 = in ? a.st[i] : 0;
  const uint64_t key = in ? a.keys[i] : kInvalid;
  const bool any = a.ctl->njoin == a.tag;
  if (blockIdx.x == 0) sum_inserts(a, false);
  if (!any || !in || o0 != 1 || st0 != kStPending) return;
  const uint64_t h = hash64(key);
  const uint32_t jb = jbit_of(h);
  const uint4* fw = reinterpret_cast<const uint4*>(a.jbits + (size_t)(jb >> 5) * kJoinReps);
  const uint4 f0 = fw[0], f1 = fw[1];
  if (!(((f0.x | f0.y | f0.z | f0.w | f1.x | f1.y | f1.z | f1.w) >> (jb & 31u)) & 1u)) return;
  uint64_t sl = iset_slot(h, a.imask);
  for (;; sl = (sl + 1) & a.imask) {
    const uint64_t prev = atomicCAS((unsigned long long*)&a.iset[sl], (unsigned long long)kInvalid,
                                    (unsigned long long)key);
    if (prev == kInvalid || prev == key) break;
  }
  a.islot[i] = (uint32_t)sl;
  atomicAdd(&a.icnt[sl], 1u);
  atomicMin(&a.ipos[sl], (uint32_t)i);
}

// Upsert batches (PMDFC_CFG_UPSERT): the pre-batch slot of every Insert's key
// in its window (0xFFFF: absent), quad per op, probing to the first empty slot
// like k_get.  The first apply pass takes its UPDATE slots from
// here instead of probing the segment lane by lane; it runs before any split
// of the batch, so these slots are still where the keys are.
__global__ __launch_bounds__(256) void k_upsert_probe(const uint64_t* __restrict__ keys, uint32_t kvs,
                                                      const uint8_t* __restrict__ ops, uint64_t n, Geo g,
                                                      const ulonglong2* __restrict__ pairs,
                                                      uint16_t* __restrict__ upos) {
  const uint64_t op = ((uint64_t)blockIdx.x * 256u + threadIdx.x) >> 2;
  const uint32_t q = threadIdx.x & 3u;
  if (op >= n) return;  // whole quads
  const uint64_t key = keys[op * kvs];
  const uint64_t h = hash64(key);
  const bool live = !reserved_key(key) && (!ops || ops[op] == 1) && !wrong_shard(h, g.sbits, g.shard);
  uint32_t res = 0xFFFFu;
  if (live) {  // quad-uniform
    const ulonglong2* sp = pairs + (size_t)de_seg(dir_entry(g, h)) * kSlots;
    const uint32_t line0 = (uint32_t)(h & 0xFF);
    const uint32_t qbase = (__lane_id() & 63u) & ~3u;
    // a fresh key probes to its window's first empty slot, often several
    // lines: from an even line, the next line is in the same 128-B HBM line
    // and is loaded with it (one round trip per two lines)
    for (uint32_t t = 0; t < kLines;) {
      const uint32_t ln = (line0 + t) & 255u;
      const bool two = !(ln & 1u) && t + 1 < kLines;
      const ulonglong2 p = sp[ln * 4u + q];
      const ulonglong2 pn = two ? sp[ln * 4u + 4u + q] : p;
      const uint32_t mn = (uint32_t)(__ballot(p.x == key) >> qbase) & 0xFu;
      const uint32_t en = (uint32_t)(__ballot(p.x == kInvalid) >> qbase) & 0xFu;
      if (mn) {
        res = ln * 4u + (uint32_t)__builtin_ctz(mn);
        break;
      }
      if (en) break;
      if (two) {
        const uint32_t m2 = (uint32_t)(__ballot(pn.x == key) >> qbase) & 0xFu;
        const uint32_t e2 = (uint32_t)(__ballot(pn.x == kInvalid) >> qbase) & 0xFu;
        if (m2) {
          res = (ln + 1u) * 4u + (uint32_t)__builtin_ctz(m2);
          break;
        }
        if (e2) break;
      }
      t += two ? 2u : 1u;
    }
  }
  if (q == 0) upos[op] = (uint16_t)res;
}

void launch_upsert_probe(const uint64_t* keys, uint32_t kvs, const uint8_t* ops, uint64_t n, Geo g,
                         const ulonglong2* pairs, uint16_t* upos, hipStream_t s) {
  if (n)
    hipLaunchKernelGGL(k_upsert_probe, dim3((unsigned)((n + 63) / 64)), dim3(256), 0, s, keys, kvs, ops, n, g, pairs,
                       upos);
}

// After a mixed batch: if a split dropped entries during it, re-probe the
// early single-copy hits and the Gets linked to their one insert.  A key
// still stored keeps its answer.  A key that is gone was dropped by a split
// of this batch (Insert4split, CCEH_hybrid.cpp:24-27; the batch never adds it
// back): the drop log holds it with the batch position of the insert whose
// full window caused that split.  In the serial order the drop happens inside
// that insert, so a Get after it misses and a Get before it sees the key --
// the reference's answer either way.  (A key has at most one copy here, so it
// is logged at most once.)  Only a log that overflowed (more than kDropLog
// drops in one batch) leaves the position unknown: PMDFC_ST_SPLIT_LOST and
// the sticky error bit 16.  Linked Gets (early == 2) take their insert's
// outcome first.
//   Early hits answered without the set (early == 3: a non-wrapping window,
// so copies of the key stay in probe order and a split drops a SUFFIX of
// them, see k_mixed_get) stand unless the log holds a drop of the key before
// the Get.  Then the key's copies are replayed as a count: the pre-batch
// copy, + 1 for each stored insert of the key before the Get (a wave scans
// the batch), - 1 for each logged drop, a drop at position t coming before
// the insert at t (that insert's full window split the segment); the Get
// sees the first copy: the pre-batch value while the count never reached 0,
// else the value of the insert that refilled it, or a miss.  (More than 64
// such drops of one key before one Get: PMDFC_ST_SPLIT_LOST, error bit 16.)
//   An overflowed log places no drop, but it takes none to see that no copy
// of the key was dropped at all: the batch only adds copies, every copy of a
// key lies in its window, so the window (seg: the key's segment after the
// batch) then holds the pre-batch copy and one more for each stored insert of
// the key anywhere in the batch.  The pre-batch copy is still the first one
// and the early hit stands.  Fewer copies: one of this key's was dropped, at a
// position the log lost -- PMDFC_ST_SPLIT_LOST.  (A key that is present is not
// enough: its pre-batch copy may have been dropped before the Get and an
// insert after the Get may have stored the key again.)
// (A real call: it takes the fields it reads, not the MixedArgs, which would
// have to be spilled to scratch to be passed by reference.)
__device__ __noinline__ bool kept_every_copy(const uint8_t* __restrict__ ops, const uint64_t* __restrict__ keys,
                                             const uint8_t* __restrict__ st, uint64_t n, uint64_t key,
                                             const ulonglong2* __restrict__ seg) {
  const uint32_t lane = __lane_id() & 63u;
  // the window does not wrap (early 3): slots 4 * line .. + 31, one per lane
  const uint64_t at = lane < kWindow ? seg[(uint32_t)(hash64(key) & 0xFF) * 4u + lane].x : kInvalid;
  const uint32_t copies = (uint32_t)__popcll(__ballot(at == key));
  if (copies == 0) return false;
  uint32_t stored = 0;  // the batch's stored inserts of the key, 256 ops per step
  for (uint64_t p0 = 0; p0 < n; p0 += 256) {
    bool ins[4];
    bool any = false;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const uint64_t p = p0 + 64u * (uint32_t)u + lane;
      ins[u] = p < n && ops[p] == 1;
      any |= ins[u];
    }
    if (!__ballot(any)) continue;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const uint64_t p = p0 + 64u * (uint32_t)u + lane;
      stored += (uint32_t)__popcll(__ballot(ins[u] && keys[p] == key && st[p] == 2));
    }
  }
  return copies == 1u + stored;
}

__device__ __noinline__ void replay_unchecked_hit(const uint8_t* __restrict__ ops, const uint64_t* __restrict__ keys,
                                                  const uint64_t* __restrict__ vin, uint8_t* __restrict__ st,
                                                  uint64_t* __restrict__ vout, uint64_t o, uint64_t n,
                                                  DevCtl* __restrict__ ctl, const ulonglong2* __restrict__ drops,
                                                  const ulonglong2* __restrict__ seg) {
  const uint32_t lane = __lane_id() & 63u;
  const uint64_t key = keys[o];
  const uint32_t nd = ctl->drop_n, nl = min(nd, kDropLog);
  if (nd > kDropLog) {  // (wave-uniform) the log is incomplete: no drop can be placed
    if (!kept_every_copy(ops, keys, st, n, key, seg) && lane == 0) {
      st[o] = 10;  // PMDFC_ST_SPLIT_LOST
      vout[o] = 0;
      atomicOr(&ctl->err, 1u << 16);
    }
    return;
  }
  // this key's drops before o, one per lane (at most 64)
  uint32_t dtrig = 0xFFFFFFFFu, cnt = 0;
  for (uint32_t j0 = 0; j0 < nl; j0 += 64) {
    const uint32_t j = j0 + lane;
    const ulonglong2 d = j < nl ? drops[j] : make_ulonglong2(kInvalid, 0);
    const bool mine = d.x == key && d.y < o;
    const uint64_t mm = __ballot(mine);
    uint32_t xi = cnt;  // lane xi keeps the xi-th drop
    for (uint64_t b = mm; b; b &= b - 1, ++xi) {
      const uint32_t tv = (uint32_t)__shfl((int)(uint32_t)d.y, __builtin_ctzll(b));
      if (lane == xi) dtrig = tv;
    }
    cnt += (uint32_t)__popcll(mm);
  }
  if (cnt == 0) return;  // the pre-batch copy outlived the Get: the early hit stands
  if (cnt > 64u) {       // unplaced
    if (lane == 0) {
      st[o] = 10;  // PMDFC_ST_SPLIT_LOST
      vout[o] = 0;
      atomicOr(&ctl->err, 1u << 16);
    }
    return;
  }
  int len = 1;  // copies of the key, the first one's value
  uint64_t first = vout[o];
  bool applied = lane >= cnt;
  bool bad = false;
  const auto drop_to = [&](uint64_t pos) {  // every drop at or before pos
    const bool now = !applied && dtrig <= pos;
    const int k = (int)__popcll(__ballot(now));
    applied |= now;
    len -= k;
    if (len < 0) {
      bad = true;
      len = 0;
    }
  };
  for (uint64_t p0 = 0; p0 < o; p0 += 64) {
    const uint64_t p = p0 + lane;
    const bool ins = p < o && ops[p] == 1 && keys[p] == key && st[p] == 2;  // a stored insert of the key
    for (uint64_t b = __ballot(ins); b; b &= b - 1) {
      const int src = __builtin_ctzll(b);
      const uint64_t pos = p0 + (uint64_t)src;
      drop_to(pos);
      if (len == 0) first = vin[pos];
      ++len;
    }
  }
  drop_to(o);
  if (lane == 0) {
    st[o] = len > 0 ? 1 : 0;
    vout[o] = len > 0 ? first : 0;
    if (bad) atomicOr(&ctl->err, 4u);  // (cannot happen: more drops than copies)
  }
}

__global__ __launch_bounds__(256) void k_mixed_verify(const MixedArgs a) {
  // a thread per op; the rare re-probe (a split of this batch dropped
  // entries) is done by the whole wave, one op at a time
  const uint64_t op = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u;
  // the batch's control words, read ahead of this kernel's own stores: only
  // then are they provably unclobbered and stay scalar loads
  const uint32_t ins_total = a.ctl->ins_total, loss_now = a.ctl->loss_events, loss_was = *a.loss0;
  const uint32_t nd = a.ctl->drop_n, nl = min(nd, kDropLog);
  // the set and the join filter, empty again for the next mixed batch: the
  // slots of this batch's joining Gets (scattered stores), or with many of
  // them the whole set (coalesced stores: 12 B per slot against ~2 scattered
  // stores per key); the filter (1 MiB) whole whenever a Get joined
  // (ipos too, back to ~0: the join's first-position minimum starts there)
  const uint64_t nt = (uint64_t)gridDim.x * 256u;
  if (a.join)
    for (uint64_t x = op; x < kJoinWords; x += nt) a.jbits[x] = 0u;
  if (!a.join && ins_total > (uint32_t)((a.imask + 1) >> kBulkClearShift)) {
    for (uint64_t x = op; x <= a.imask; x += nt) {
      a.iset[x] = kInvalid;
      a.icnt[x] = 0u;
      a.ipos[x] = 0xFFFFFFFFu;
    }
  } else if (op < a.n) {
    const uint32_t sl = a.islot[op];
    if (sl != 0xFFFFFFFFu) {
      a.iset[sl] = kInvalid;
      a.icnt[sl] = 0u;
      a.ipos[sl] = 0xFFFFFFFFu;
    }
  }
  const uint8_t e = op < a.n ? a.early[op] : 0;
  bool hit = e == 1;
  const uint64_t m3 = __ballot(e == 3);
  if (e == 2) {
    const uint32_t p = a.elink[op];
    hit = a.st[p] == 2 || a.st[p] == 11;  // PMDFC_ST_INSERTED, PMDFC_ST_UPDATED (upsert)
    a.vout[op] = hit ? a.vin[p] : 0;
    a.st[op] = hit ? 1 : 0;
  }
  uint64_t m = __ballot(hit);
  if ((!m && !m3) || loss_now == loss_was) return;
  for (uint64_t b = m3; b; b &= b - 1) {
    const uint64_t o = shfl64(op, __builtin_ctzll(b));
    const ulonglong2* seg = nullptr;  // the key's segment: read only behind an overflowed log
    if (nd > kDropLog) seg = a.pairs + (size_t)de_seg(dir_entry(bucketed(a.g), hash64(a.keys[o]))) * kSlots;
    replay_unchecked_hit(a.ops, a.keys, a.vin, a.st, a.vout, o, a.n, a.ctl, a.drops, seg);
  }
  const uint32_t q = lane & 3u;
  while (m) {
    const int src = __builtin_ctzll(m);
    m &= m - 1;
    const uint64_t o = shfl64(op, src);
    const uint64_t key = a.keys[o];
    const uint64_t h = hash64(key);
    uint64_t val = 0;
    uint32_t lines;
    const uint32_t seg = de_seg(dir_entry(bucketed(a.g), h));
    // (every quad probes the same key: a wave-uniform answer)
    if (quad_probe(a.pairs + (size_t)seg * kSlots, key, h, q, &val, &lines) != 0) continue;
    // gone: find the drop in the log, 64 entries per step
    uint32_t trig = 0xFFFFFFFFu;
    bool found = false;
    for (uint32_t j0 = 0; j0 < nl && !found; j0 += 64) {
      const uint32_t j = j0 + lane;
      const ulonglong2 d = j < nl ? a.drops[j] : make_ulonglong2(kInvalid, 0);
      const uint64_t mm = __ballot(d.x == key);
      if (mm) {
        found = true;
        trig = (uint32_t)__shfl((int)(uint32_t)d.y, __builtin_ctzll(mm));
      }
    }
    if (lane != 0) continue;
    if (!found) {
      a.st[o] = 10;  // PMDFC_ST_SPLIT_LOST (drop log overflowed)
      a.vout[o] = 0;
      atomicOr(&a.ctl->err, 1u << 16);
    } else if ((uint64_t)trig < o) {
      a.st[o] = 0;  // dropped before this Get: the reference misses
      a.vout[o] = 0;
    }  // else dropped after it: the a.early hit stands
  }
}

// Fresh table: CCEH(initCap) makes 2^depth segments of local depth `depth`
// (CCEH_hybrid.cpp:79-85).  Bucket b's sub-directory starts at pool offset
// b * 2^db0 with db0 = depth - shard_bits - p1, i.e. the pool begins as the
// flat directory and segment id = directory index.  The same launch zeroes
// the per-bucket words of the passes (z: record cursors, stat slots,
// worklist counts, decline flags, grants, grant shards) and, in block 0, the
// control block with the counters of CCEH(initCap) and the host-mapped
// segment-count hint: one launch per reset instead of eight.
__global__ __launch_bounds__(256) void k_init_segments(ulonglong2* __restrict__ pairs,
                                                       uint32_t* __restrict__ occ,
                                                       uint8_t* __restrict__ ldep,
                                                       uint32_t* __restrict__ pool,
                                                       uint64_t* __restrict__ hdr, uint32_t nseg,
                                                       uint32_t depth, uint32_t p1, uint32_t fixed,
                                                       uint32_t region, InitZero z, DevCtl* __restrict__ ctl,
                                                       uint32_t pool_cur, uint32_t* __restrict__ hint) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  const uint32_t db0 = (uint32_t)__builtin_ctz(nseg) - p1;  // nseg = 2^(depth - sbits)
  if (i < (uint64_t)nseg * kSlots) pairs[i] = make_ulonglong2(kInvalid, 0ULL);
  if (i < (uint64_t)nseg * 32u) occ[i] = 0;
  if (i < nseg) {
    ldep[i] = (uint8_t)depth;
    // bucket b's entries: its fixed slot (cceh_kernels.h kFixedBits) or the pool
    const uint32_t at = fixed ? (uint32_t)(i >> db0) * kFixedSlot + (uint32_t)(i & ((1u << db0) - 1u))
                              : region + (uint32_t)i;
    pool[at] = de_make((uint32_t)i, depth);
  }
  const uint32_t nb = 1u << p1;
  if (i < nb) hdr[i] = hdr_make(fixed ? (uint32_t)i * kFixedSlot : region + ((uint32_t)i << db0), db0);
  zero_batch_words(z, i);
  if (blockIdx.x == 0 && start_ctl(ctl, nseg, depth, pool_cur, hint)) ctl->depth_count[depth] = nseg;
}

// Finer directory buckets (p1 -> p1n bits) once every segment's local depth
// allows it (none spans two new buckets): new bucket w takes the slice of its
// old bucket's sub-directory that its d = p1n - p1 extra hash bits select --
// the same pool entries, nothing moves (the slice has db - d bits, db >= d).
__global__ __launch_bounds__(256) void k_rebucket(const uint64_t* __restrict__ old_hdr, uint64_t* __restrict__ hdr,
                                                  uint32_t p1, uint32_t p1n) {
  const uint32_t w = blockIdx.x * 256u + threadIdx.x;
  if (w >= (1u << p1n)) return;
  const uint32_t d = p1n - p1;
  const uint64_t o = old_hdr[w >> d];
  const uint32_t db = hdr_db(o) - d;
  hdr[w] = hdr_make(hdr_off(o) + ((w & ((1u << d) - 1u)) << db), db);
}

// the smallest local depth over the live segments (ids < ctl->nsegs) -> *out
// (which the caller set to ~0)
__global__ __launch_bounds__(256) void k_min_ldep(const uint8_t* __restrict__ ldep, const DevCtl* __restrict__ ctl,
                                                  uint32_t max_segs, uint32_t* __restrict__ out) {
  const uint32_t n = min(ctl->nsegs, max_segs);
  uint32_t m = 0xFFu;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) m = min(m, (uint32_t)ldep[i]);
  for (int o = 32; o > 0; o >>= 1) m = min(m, (uint32_t)__shfl_xor((int)m, o));
  if ((threadIdx.x & 63u) == 0) atomicMin(out, m);
}

void launch_min_ldep(const uint8_t* ldep, const DevCtl* ctl, uint32_t max_segs, uint32_t* out, hipStream_t s) {
  hipLaunchKernelGGL(k_min_ldep, dim3(64), dim3(256), 0, s, ldep, ctl, max_segs, out);
}

void launch_rebucket(const uint64_t* old_hdr, uint64_t* hdr, uint32_t p1, uint32_t p1n, hipStream_t s) {
  hipLaunchKernelGGL(k_rebucket, dim3(((1u << p1n) + 255) / 256), dim3(256), 0, s, old_hdr, hdr, p1, p1n);
}

// occupied-slot count (CCEH::Utilization numerator, CCEH_hybrid.cpp:412-427)
__global__ __launch_bounds__(256) void k_popcount(const uint32_t* __restrict__ occ, uint64_t nwords,
                                                  unsigned long long* __restrict__ out) {
  uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  uint32_t c = 0;
  for (; i < nwords; i += (uint64_t)gridDim.x * 256u) c += __popc(occ[i]);
  for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(out, (unsigned long long)c);
}

// CCEH::FindAnyway (CCEH_hybrid.cpp:482-496; src/cceh.cpp:457-471): the
// reference walks directory entries 0..capacity-1 and, in each, slots
// 0..1023, returning the first pair whose key matches -- no window, no early
// exit.  Inserts and split replays only ever place a key in the segment its
// hash prefix selects (CCEH_hybrid.cpp:119,54), so the first segment in
// directory order holding the key is that one; inside it the answer is the
// first copy in SLOT order, which differs from Get's probe order when the
// window wraps past slot 1023.  One wave per key: 16 slots per
// lane, one ballot per 64-slot stripe, lowest matching slot wins.
__global__ __launch_bounds__(256) void k_find_anyway(const uint64_t* __restrict__ keys,
                                                     uint64_t* __restrict__ vout, uint8_t* __restrict__ st,
                                                     uint64_t n, Geo g, const ulonglong2* __restrict__ pairs) {
  const uint64_t op = ((uint64_t)blockIdx.x * 256u + threadIdx.x) >> 6;
  const uint32_t lane = threadIdx.x & 63u;
  if (op >= n) return;
  const uint64_t key = keys[op];
  const uint64_t h = hash64(key);
  uint64_t val = 0;
  uint8_t s = 0;  // PMDFC_ST_MISS (NONE)
  if (reserved_key(key)) {
    s = 3;
  } else if (wrong_shard(h, g.sbits, g.shard)) {
    s = 8;
  } else {
    const ulonglong2* sp = pairs + (size_t)de_seg(dir_entry(g, h)) * kSlots;
    ulonglong2 p[kSlots / 64];
#pragma unroll
    for (uint32_t j = 0; j < kSlots / 64; ++j) p[j] = sp[j * 64u + lane];  // stripe j: slots 64j..64j+63
#pragma unroll
    for (uint32_t j = 0; j < kSlots / 64; ++j) {
      const uint64_t m = __ballot(p[j].x == key);
      if (m) {
        val = shfl64(p[j].y, __builtin_ctzll(m));
        s = 1;  // PMDFC_ST_HIT
        break;
      }
    }
  }
  if (lane == 0) {
    vout[op] = val;
    st[op] = s;
  }
}

__global__ __launch_bounds__(256) void k_hash(const uint64_t* __restrict__ keys,
                                              uint64_t* __restrict__ out, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i < n) out[i] = hash64(keys[i]);
}

__global__ __launch_bounds__(256) void k_gen_keys(uint64_t seed, uint64_t start,
                                                  uint64_t* __restrict__ out, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint64_t ctr = start + i + (seed << 40);
  uint64_t k = splitmix64(ctr);
  if (k == 0 || k >= kSentinel) k = 0x5555555555555555ULL + ctr;
  out[i] = k;
}

// owner shard of each key (top sbits of h) for the routing sort
__global__ __launch_bounds__(256) void k_owner(const uint64_t* __restrict__ keys, uint64_t n,
                                               uint32_t sbits, uint32_t* __restrict__ owner,
                                               uint32_t* __restrict__ idx) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  owner[i] = sbits ? (uint32_t)(hash64(keys[i]) >> (64 - sbits)) : 0u;
  idx[i] = (uint32_t)i;
}

__global__ __launch_bounds__(256) void k_bounds(const uint32_t* __restrict__ sorted_owner,
                                                uint64_t n, uint32_t ngroups,
                                                uint64_t* __restrict__ starts) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i > n) return;
  const int64_t lo = (i == 0) ? -1 : (int64_t)sorted_owner[i - 1];
  const int64_t hi = (i == n) ? (int64_t)ngroups : (int64_t)sorted_owner[i];
  for (int64_t g = lo + 1; g <= hi && g <= (int64_t)ngroups; ++g) starts[g] = i;
}

// ------------------------------------------------------------------ launchers
#define GRID(n, per) dim3((unsigned)(((n) + (per)-1) / (per)))

// ---- flat directory for pure-Get batches (one L2 lookup per Get instead of
// header + sub-directory)
__global__ __launch_bounds__(1024) void k_flat_bits(const uint64_t* __restrict__ hdr, uint32_t nb,
                                                    uint32_t p1, uint32_t max_bits, uint32_t* __restrict__ bits) {
  __shared__ uint32_t s_m[16];
  uint32_t m = 0;
  for (uint32_t b = threadIdx.x; b < nb; b += 1024) m = max(m, hdr_db(hdr[b]));
  for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o));
  if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 16; ++w) m = max(m, s_m[w]);
    *bits = p1 + m <= max_bits ? p1 + m : 0xFFu;  // too deep: Gets use hdr/pool
  }
}

__global__ __launch_bounds__(256) void k_flatten(const uint64_t* __restrict__ hdr,
                                                 const uint32_t* __restrict__ pool, uint32_t p1,
                                                 uint32_t* __restrict__ flat, const uint32_t* __restrict__ bits) {
  const uint32_t fb = *bits;
  const uint32_t x = blockIdx.x * 256u + threadIdx.x;
  if (fb > kFlatMaxBits || x >= (1u << fb)) return;
  const uint32_t w = p1 ? x >> (fb - p1) : 0u;
  const uint64_t hd = hdr[w];
  const uint32_t db = hdr_db(hd);
  const uint32_t sub = db ? (x >> (fb - p1 - db)) & ((1u << db) - 1u) : 0u;
  flat[x] = pool[hdr_off(hd) + sub];
}

void launch_flatten(const uint64_t* hdr, const uint32_t* pool, uint32_t p1, uint32_t* flat,
                    uint32_t* bits, uint32_t max_bits, hipStream_t s) {
  hipLaunchKernelGGL(k_flat_bits, dim3(1), dim3(1024), 0, s, hdr, 1u << p1, p1, min(max_bits, kFlatMaxBits),
                     bits);
  hipLaunchKernelGGL(k_flatten, dim3((1u << kFlatMaxBits) / 256), dim3(256), 0, s, hdr, pool, p1, flat,
                     (const uint32_t*)bits);
}

void launch_get(bool count, const uint64_t* keys, uint64_t* vout, uint8_t* st, uint64_t n,
                Geo g, const ulonglong2* pairs, uint32_t* partials, hipStream_t s) {
  if (!n) return;
  const ProcessKnobs& K = process_knobs();
  const int U = K.get_unroll;
  if (U > 1) {
    const uint64_t quads = (n + U - 1) / U;
    // a launch of several batches' Gets (pmdfc_cceh_get_batches) caps its
    // grid (PMDFC_GET_GRID blocks, 0: none) and loops
    const uint64_t want = (quads + 63) / 64, cap = count ? 0 : K.get_grid;  // (COUNT: a partial per block)
    const uint64_t nblk = cap && want > cap ? cap : want;
    const uint32_t rounds = (uint32_t)((want + nblk - 1) / nblk);
    const dim3 grid((unsigned)nblk);
#define LG(UU)                                                                               \
  if (count)                                                                                 \
    hipLaunchKernelGGL((k_get_u<UU, true>), grid, dim3(256), 0, s, keys, vout, st, n, g, pairs, \
                       partials, K.get_p2, rounds);                                          \
  else                                                                                       \
    hipLaunchKernelGGL((k_get_u<UU, false>), grid, dim3(256), 0, s, keys, vout, st, n, g, pairs, \
                       partials, K.get_p2, rounds);
    if (U == 2) {
      LG(2)
    } else {
      LG(4)
    }
#undef LG
    return;
  }
  if (count)
    hipLaunchKernelGGL(k_get<true>, GRID(n, 64), dim3(256), 0, s, keys, vout, st, n, g, pairs, partials);
  else
    hipLaunchKernelGGL(k_get<false>, GRID(n, 64), dim3(256), 0, s, keys, vout, st, n, g, pairs, partials);
}

void launch_mixed_prep(const MixedArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_mixed_prep, GRID(a.n ? a.n : 1, 256), dim3(256), 0, s, a);
}

// Gets per quad issued together: 2 (configs 4 / 3: U=4 3.91 / 5.76, U=2
// 3.95 / 5.96, U=1 3.97 / 5.94 Gops/s); PMDFC_MG_U overrides (A/B)
#define MG(kernel)                                                                       \
  switch (process_knobs().mg_u) {                                                        \
    case 1: hipLaunchKernelGGL(kernel<1>, GRID(a.n, 256), dim3(256), 0, s, a); break;    \
    case 2: hipLaunchKernelGGL(kernel<2>, GRID(a.n, 256), dim3(256), 0, s, a); break;    \
    default: hipLaunchKernelGGL(kernel<4>, GRID(a.n, 256), dim3(256), 0, s, a);          \
  }
void launch_mixed_get_iset(const MixedArgs& a, hipStream_t s) {
  if (a.n) MG(k_mixed_get_iset)
}

void launch_mixed_get(const MixedArgs& a, hipStream_t s) {
  if (a.n) MG(k_mixed_get)
}
#undef MG

void launch_mixed_join(const MixedArgs& a, hipStream_t s) {
  if (a.n) hipLaunchKernelGGL(k_mixed_join, GRID(a.n, 256), dim3(256), 0, s, a);
}

void launch_mixed_verify(const MixedArgs& a, hipStream_t s) {
  if (a.n) hipLaunchKernelGGL(k_mixed_verify, GRID(a.n, 256), dim3(256), 0, s, a);
}

void launch_init_segments(ulonglong2* pairs, uint32_t* occ, uint8_t* ldep, uint32_t* pool,
                          uint64_t* hdr, uint32_t nseg, uint32_t depth, uint32_t p1, uint32_t fixed,
                          uint32_t region, const InitZero& z, DevCtl* ctl, uint32_t pool_cur, uint32_t* hint,
                          hipStream_t s) {
  static_assert(sizeof(DevCtl) % 4 == 0, "DevCtl is zeroed by words");
  uint64_t n = std::max<uint64_t>((uint64_t)nseg * kSlots, 1ULL << p1);
  for (int k = 0; k < kInitZero; ++k) n = std::max<uint64_t>(n, z.n[k]);
  hipLaunchKernelGGL(k_init_segments, GRID(n, 256), dim3(256), 0, s, pairs, occ, ldep, pool, hdr,
                     nseg, depth, p1, fixed, region, z, ctl, pool_cur, hint);
}

void launch_popcount(const uint32_t* occ, uint64_t nwords, unsigned long long* out, hipStream_t s) {
  hipLaunchKernelGGL(k_popcount, dim3(1024), dim3(256), 0, s, occ, nwords, out);
}

void launch_find_anyway(const uint64_t* keys, uint64_t* vout, uint8_t* st, uint64_t n, Geo g,
                        const ulonglong2* pairs, hipStream_t s) {
  if (n) hipLaunchKernelGGL(k_find_anyway, GRID(n, 4), dim3(256), 0, s, keys, vout, st, n, g, pairs);
}

void launch_hash(const uint64_t* keys, uint64_t* out, uint64_t n, hipStream_t s) {
  if (n) hipLaunchKernelGGL(k_hash, GRID(n, 256), dim3(256), 0, s, keys, out, n);
}

void launch_gen_keys(uint64_t seed, uint64_t start, uint64_t* out, uint64_t n, hipStream_t s) {
  if (n) hipLaunchKernelGGL(k_gen_keys, GRID(n, 256), dim3(256), 0, s, seed, start, out, n);
}

void launch_owner(const uint64_t* keys, uint64_t n, uint32_t sbits, uint32_t* owner, uint32_t* idx,
                  hipStream_t s) {
  if (n) hipLaunchKernelGGL(k_owner, GRID(n, 256), dim3(256), 0, s, keys, n, sbits, owner, idx);
}

void launch_bounds(const uint32_t* sorted_owner, uint64_t n, uint32_t ngroups, uint64_t* starts,
                   hipStream_t s) {
  hipLaunchKernelGGL(k_bounds, GRID(n + 1, 256), dim3(256), 0, s, sorted_owner, n, ngroups, starts);
}

}  // namespace pmdfc
