// part.hip -- k_part, step 1 of a batch's launch sequence (bucket.hip):
// partition of the batch's pending ops into 2^(p1 - sbb) partition
// buckets by the top local hash bits.  Each 8192-op tile counts its ops per
// bucket with LDS atomics and reserves one contiguous run per non-empty
// bucket in its XCD's sub-region (blockIdx & 7) of that bucket's record
// region (one global atomic per (tile, bucket), all of a thread's issued
// back to back); a run that does not fit spills into a shared overflow
// area, tagged with its bucket.  Records (SoA): {key, value}, rop = op
// index | sub-bucket << 22 | Get << 31; order inside a bucket is not batch
// order (the passes sort by op index).
#include "cceh_device.h"
#include "cceh_kernels.h"
#include "wave_util.h"

namespace pmdfc {

constexpr int kPartThreads = 1024;
constexpr int kPartPer = (int)kPartTile / kPartThreads;  // ops per thread

// --------------------------------------------------------------- partition

// A joining Get of a mixed batch (kStJoin, cceh_kernels.hip k_mixed_get),
// once k_mixed_join put the batch's inserts of its key into the set (count,
// first position): no insert -- its probe result stands (vout, early 1 for a
// hit); a miss whose key the batch inserts once -- a miss before that insert,
// linked to it after; else pending, for the ordered passes.  The set probe
// loads each slot's key, count and first position together (one round trip:
// the first slot almost always holds the key or is empty).  Returns the Get's
// new status.
__device__ __forceinline__ uint8_t join_resolve(const PartArgs& a, uint64_t p, uint64_t key, uint64_t h) {
  uint64_t sl = iset_slot(h, a.imask);
  const uint8_t c = a.early[p];
  uint32_t ic = 0, ps = 0;
  for (;; sl = (sl + 1) & a.imask) {
    const uint64_t v = a.iset[sl];
    const uint32_t ic1 = a.icnt[sl], ps1 = a.ipos[sl];
    if (v == kInvalid) break;  // no insert of the key
    if (v == key) {
      ic = ic1;
      ps = ps1;
      break;
    }
  }
  uint8_t s;
  if (ic == 0) {
    s = c ? 1 : 0;  // PMDFC_ST_HIT / PMDFC_ST_NOT_FOUND
  } else if (c == 0 && ic == 1) {
    if ((uint64_t)ps > p) {
      s = 0;
    } else {
      s = kStLinked;  // the insert's outcome after the batch (k_mixed_verify)
      a.early[p] = 2;
      a.elink[p] = ps;
    }
  } else {
    s = kStPending;
    a.early[p] = 0;
    a.vout[p] = 0;
    a.ctl->pget = a.tag;  // every writer stores the same word
  }
  a.st[p] = s;
  return s;
}

__global__ __launch_bounds__(kPartThreads) void k_part(PartArgs a) {
  // 64 KB of LDS: a block fits beside a CU's share of the apply pass, which
  // it overlaps in pipelined insert batches (the overflow slot of a run that
  // does not fit its sub-region, rare, goes through global memory: a.povf)
  __shared__ uint32_t s_cnt[1u << kMaxPartBits];  // ops of the tile per bucket
  __shared__ uint32_t s_reg[1u << kMaxPartBits];  // region slot of the bucket's run
  uint64_t* const srow = a.stamps ? a.stamps + (size_t)blockIdx.x * 8 : nullptr;
  stamp(srow, kPsStart, threadIdx.x == 0);
  const uint32_t nb = 1u << a.pbits;
  for (uint32_t i = threadIdx.x; i < nb; i += kPartThreads) s_cnt[i] = 0;
  __syncthreads();
  const uint64_t base = (uint64_t)blockIdx.x * kPartTile;
  uint64_t kk[kPartPer], vv[kPartPer];
  uint32_t bk[kPartPer], rk[kPartPer], ro[kPartPer];
#pragma unroll
  for (int k = 0; k < kPartPer; ++k) {
    const uint64_t p = base + (uint64_t)k * kPartThreads + threadIdx.x;
    kk[k] = p < a.n ? a.keys[p * a.kvs] : kInvalid;
  }
#pragma unroll
  for (int k = 0; k < kPartPer; ++k) {
    const uint64_t p = base + (uint64_t)k * kPartThreads + threadIdx.x;
    bool part = false;
    bk[k] = 0xFFFFFFFFu;
    vv[k] = 0;
    ro[k] = (uint32_t)p;
    if (p < a.n) {
      const uint64_t key = kk[k];
      const uint64_t h = hash64(key);
      if (!a.ops) {
        uint8_t code = 2;  // PMDFC_ST_INSERTED (k_bucket rewrites the rare failures)
        if (reserved_key(key)) code = 3;
        else if (wrong_shard(h, a.sbits, a.shard)) code = 8;
        a.st[p] = code;
        part = code == 2;
      } else {
        if (a.init) {  // (k_mixed_prep's rule)
          const uint8_t code = reserved_key(key) ? 3 : wrong_shard(h, a.sbits, a.shard) ? 8 : kStPending;
          a.st[p] = code;
          a.vout[p] = 0;
          part = code == kStPending;
        } else {
          uint8_t s0 = a.st[p];
          if (s0 == kStJoin) s0 = join_resolve(a, p, key, h);
          part = s0 == kStPending;
        }
        if (part && a.ops[p] != 1) ro[k] |= kGetBit;  // anything but PMDFC_OP_INSERT is a Get
        // inserts: PMDFC_ST_INSERTED unless a pass rewrites it (the
        // insert-only apply passes, which a gated mixed batch may take,
        // never write it)
        else if (part) a.st[p] = 2;
      }
      if (part) {
        const uint32_t b2 = bucket_of(h, a.sbits, a.pbits + a.sbb);  // directory bucket
        bk[k] = b2 >> a.sbb;
        ro[k] |= (b2 & ((1u << a.sbb) - 1)) << 22;
        if (!(ro[k] & kGetBit)) vv[k] = a.vin[p * a.kvs];
        rk[k] = atomicAdd(&s_cnt[bk[k]], 1u);
      }
    }
  }
  __syncthreads();
  stamp(srow, kPsCounted, threadIdx.x == 0);
  if (a.touched) {  // one block (medium batch): the partition buckets that received ops
    __shared__ uint32_t s_nt;
    if (threadIdx.x == 0) s_nt = 0;
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < nb; b += kPartThreads)
      if (s_cnt[b]) a.touched[1 + atomicAdd(&s_nt, 1u)] = b;
    __syncthreads();
    if (threadIdx.x == 0) a.touched[0] = s_nt;
  }
  // one run per non-empty bucket: reserve it in this block's sub-region; the
  // part past the sub-region's capacity goes to the overflow area.  A
  // thread's cursor atomics are issued together (one round trip, not one per
  // bucket)
  {
    constexpr int kRes = (1 << kMaxPartBits) / kPartThreads;
    const uint32_t xs = blockIdx.x & (kPartSubs - 1);
    uint32_t cb[kRes], pos[kRes];
#pragma unroll
    for (int r = 0; r < kRes; ++r) {
      const uint32_t b = threadIdx.x + (uint32_t)r * kPartThreads;
      cb[r] = b < nb ? s_cnt[b] : 0u;
    }
#pragma unroll
    for (int r = 0; r < kRes; ++r) {
      const uint32_t b = threadIdx.x + (uint32_t)r * kPartThreads;
      pos[r] = cb[r] ? atomicAdd(&a.cursor[xs * nb + b], cb[r]) : 0u;  // XCD-private cursor lines
    }
#pragma unroll
    for (int r = 0; r < kRes; ++r) {
      const uint32_t b = threadIdx.x + (uint32_t)r * kPartThreads;
      const uint32_t c = cb[r];
      if (!c) continue;
      const uint32_t fit = pos[r] < a.capx ? min(c, a.capx - pos[r]) : 0u;
      s_reg[b] = b * a.cap + xs * a.capx + pos[r];
      s_cnt[b] = fit;
      if (fit < c) a.povf[(size_t)blockIdx.x * nb + b] = atomicAdd(a.ovf, c - fit);
    }
  }
  __syncthreads();
  stamp(srow, kPsReserved, threadIdx.x == 0);
#pragma unroll
  for (int k = 0; k < kPartPer; ++k) {
    const uint32_t b = bk[k];
    if (b == 0xFFFFFFFFu) continue;
    uint64_t dst;
    const uint32_t fit = s_cnt[b];
    if (rk[k] < fit) {
      dst = (uint64_t)s_reg[b] + rk[k];
    } else {
      const uint32_t o = a.povf[(size_t)blockIdx.x * nb + b] + (rk[k] - fit);
      a.robk[o] = (uint16_t)b;
      dst = a.ovf_base + o;
    }
    a.rkv[dst] = make_ulonglong2(kk[k], vv[k]);
    a.rop[dst] = ro[k];
  }
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();
  stamp(srow, kPsEnd, threadIdx.x == 0);
}

uint32_t part_blocks(uint64_t n) { return (uint32_t)((n + kPartTile - 1) / kPartTile); }

void launch_part(const PartArgs& a, hipStream_t s) {
  if (!a.n) return;
  hipLaunchKernelGGL(k_part, dim3(part_blocks(a.n)), dim3(kPartThreads), 0, s, a);
}

}  // namespace pmdfc
