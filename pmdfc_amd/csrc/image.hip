// image.hip -- device side of pmdfc_cceh_snapshot / pmdfc_cceh_restore
// (gfx950, wave64; the format: image.h).
//
// Snapshot: k_image_count / k_image_scan / k_image_emit put the segments in
// canonical (directory) order on the device, k_image_gather streams each
// 16 KiB segment from its arena id to its canonical slot of the image.
// Restore: k_image_ctl starts the control block and the per-batch words as a
// reset does, k_image_scatter copies canonical segment i to arena id i,
// rebuilds its occupancy words, local depth and directory entries, and checks
// every live key against the segment's hash prefix.
// The copies move 16 B per lane, 1 KiB per wave and step (whole 64-B lines per
// quad), non-temporal on the image side and on the gather's arena side: every
// byte is touched once.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "cceh_device.h"
#include "cceh_kernels.h"

namespace pmdfc {

namespace {

__device__ __forceinline__ void st_pair_nt(ulonglong2* p, ulonglong2 v) {
  u64x2_t w;
  w.x = v.x;
  w.y = v.y;
  __builtin_nontemporal_store(w, reinterpret_cast<u64x2_t*>(p));
}

// The distinct segments of bucket w, in sub-directory order: f(k, entry) for
// the k-th.  A segment of local depth L owns 2^(db - (L - sbits - p1))
// consecutive entries, the first at a multiple of that stride.  (A header or
// entry that a sound table cannot hold ends the walk or steps by one: the walk
// never leaves the pool.)
template <class F>
__device__ __forceinline__ uint32_t walk_bucket(const uint64_t* __restrict__ hdr, const uint32_t* __restrict__ pool,
                                                uint32_t pool_cap, uint32_t p1, uint32_t sbits, uint32_t w, F f) {
  const uint64_t hd = hdr[w];
  const uint32_t db = hdr_db(hd), off = hdr_off(hd);
  if (db > kMaxDepth || (uint64_t)off + (1ULL << db) > pool_cap) return 0;
  uint32_t k = 0;
  for (uint32_t x = 0; x < (1u << db);) {
    const uint32_t e = pool[off + x];
    const uint32_t below = de_ld(e) - sbits - p1;  // the segment's hash bits below the bucket's
    f(k, e);
    ++k;
    x += below <= db ? 1u << (db - below) : 1u;
  }
  return k;
}

__global__ __launch_bounds__(256) void k_image_count(const uint64_t* __restrict__ hdr,
                                                     const uint32_t* __restrict__ pool, uint32_t pool_cap,
                                                     uint32_t p1, uint32_t sbits, uint32_t* __restrict__ cnt) {
  const uint32_t w = blockIdx.x * 256u + threadIdx.x;
  if (w >= (1u << p1)) return;
  cnt[w] = walk_bucket(hdr, pool, pool_cap, p1, sbits, w, [](uint32_t, uint32_t) {});
}

// exclusive scan of cnt[0, nb) (nb <= 2^kMaxP1) by one block of 1024 threads:
// each thread a contiguous run, the run sums scanned in LDS
__global__ __launch_bounds__(1024) void k_image_scan(const uint32_t* __restrict__ cnt, uint32_t nb,
                                                     uint32_t* __restrict__ base, uint32_t* __restrict__ total) {
  __shared__ uint32_t s_sum[1024];
  const uint32_t t = threadIdx.x;
  const uint32_t per = (nb + 1023u) / 1024u;
  const uint32_t lo = min(t * per, nb), hi = min(lo + per, nb);
  uint32_t sum = 0;
  for (uint32_t i = lo; i < hi; ++i) sum += cnt[i];
  s_sum[t] = sum;
  __syncthreads();
  for (uint32_t d = 1; d < 1024u; d <<= 1) {
    const uint32_t v = t >= d ? s_sum[t - d] : 0u;
    __syncthreads();
    s_sum[t] += v;
    __syncthreads();
  }
  uint32_t run = s_sum[t] - sum;
  for (uint32_t i = lo; i < hi; ++i) {
    base[i] = run;
    run += cnt[i];
  }
  if (t == 1023u) *total = s_sum[t];
}

__global__ __launch_bounds__(256) void k_image_emit(const uint64_t* __restrict__ hdr,
                                                    const uint32_t* __restrict__ pool, uint32_t pool_cap,
                                                    uint32_t p1, uint32_t sbits, const uint32_t* __restrict__ base,
                                                    uint32_t nseg, uint32_t* __restrict__ order,
                                                    uint8_t* __restrict__ ld_out) {
  const uint32_t w = blockIdx.x * 256u + threadIdx.x;
  if (w >= (1u << p1)) return;
  const uint32_t b = base[w];
  walk_bucket(hdr, pool, pool_cap, p1, sbits, w, [&](uint32_t k, uint32_t e) {
    if ((uint64_t)b + k < nseg) {
      order[b + k] = e;
      ld_out[b + k] = (uint8_t)de_ld(e);
    }
  });
}

// one workgroup of four waves per segment: four 1-KiB steps per wave, the
// loads of all four issued before the first store
__global__ __launch_bounds__(256) void k_image_gather(const ulonglong2* __restrict__ pairs,
                                                      const uint32_t* __restrict__ order, uint32_t max_segs,
                                                      ulonglong2* __restrict__ out) {
  const uint32_t i = blockIdx.x;
  const uint32_t sid = de_seg(order[i]);
  if (sid >= max_segs) return;  // (no entry of a sound directory)
  const ulonglong2* src = pairs + (size_t)sid * kSlots;
  ulonglong2* dst = out + (size_t)i * kSlots;
  ulonglong2 p[4];
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k) p[k] = ld_pair_l2(src + k * 256u + threadIdx.x);
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k) {
    if (p[k].x == kInvalid) p[k].y = 0;
    st_pair_nt(dst + k * 256u + threadIdx.x, p[k]);
  }
}

__global__ __launch_bounds__(256) void k_image_ctl(InitZero z, DevCtl* __restrict__ ctl, ImageCtl c,
                                                   uint32_t* __restrict__ hint) {
  zero_batch_words(z, (uint64_t)blockIdx.x * 256u + threadIdx.x);
  if (blockIdx.x == 0 && start_ctl(ctl, c.nsegs, c.max_ld, c.pool_cur, hint))
    for (uint32_t d = 0; d < 32; ++d) ctl->depth_count[d] = c.depth_count[d];
}

// One workgroup of four waves per segment i (arena id = canonical index).
// Wave v takes slots [256 k + 64 v, +64) in step k: one ballot of
// key != INVALID is the two occupancy words 8 k + 2 v and 8 k + 2 v + 1.
__global__ __launch_bounds__(256) void k_image_scatter(ScatterArgs a) {
  const uint32_t i = blockIdx.x;
  const uint32_t lane = threadIdx.x & 63u, v = threadIdx.x >> 6;
  const uint2 d = a.desc[i];
  const uint32_t start = d.x, L = d.y;
  const uint32_t Ll = L - a.sbits;         // local hash bits
  const uint32_t top = kMaxDepth - a.sbits;  // start counts 2^-top of the shard's space
  const uint64_t prefix = ((uint64_t)a.shard << Ll) | (start >> (top - Ll));
  const ulonglong2* src = a.img + (size_t)i * kSlots;
  ulonglong2* dst = a.pairs + (size_t)i * kSlots;
  ulonglong2 p[4];
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k) p[k] = ld_pair_l2(src + k * 256u + threadIdx.x);
  uint32_t bad = 0;
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k) {
    const bool live = p[k].x != kInvalid;
    if (!live) p[k].y = 0;
    dst[k * 256u + threadIdx.x] = p[k];
    const uint64_t m = __ballot(live);
    if (lane == 0) {
      uint32_t* o = a.occ + (size_t)i * 32u + k * 8u + v * 2u;
      o[0] = (uint32_t)m;
      o[1] = (uint32_t)(m >> 32);
    }
    // reserved keys are never stored; a live key sits in the segment its
    // top L hash bits select
    bad += live && (p[k].x == kSentinel || (hash64(p[k].x) >> (64u - L)) != prefix) ? 1u : 0u;
  }
  for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor((int)bad, o);
  if (lane == 0 && bad) atomicAdd(a.bad, bad);
  if (threadIdx.x == 0) a.ldep[i] = (uint8_t)L;
  // the segment's 2^(db - (Ll - p1)) entries of its bucket's sub-directory
  const uint32_t w = a.p1 ? start >> (top - a.p1) : 0u;
  const uint64_t hd = a.hdr[w];
  const uint32_t db = hdr_db(hd);
  const uint32_t below = Ll - a.p1;
  const uint32_t first = db ? (start >> (top - a.p1 - db)) & ((1u << db) - 1u) : 0u;
  const uint32_t e = de_make(i, L);
  for (uint32_t j = threadIdx.x; j < (1u << (db - below)); j += 256u) a.pool[hdr_off(hd) + first + j] = e;
}

}  // namespace

void launch_image_count(const uint64_t* hdr, const uint32_t* pool, uint32_t pool_cap, uint32_t p1, uint32_t sbits,
                        uint32_t* cnt, uint32_t* base, uint32_t* total, hipStream_t s) {
  const uint32_t nb = 1u << p1;
  hipLaunchKernelGGL(k_image_count, dim3((nb + 255) / 256), dim3(256), 0, s, hdr, pool, pool_cap, p1, sbits, cnt);
  hipLaunchKernelGGL(k_image_scan, dim3(1), dim3(1024), 0, s, cnt, nb, base, total);
}

void launch_image_emit(const uint64_t* hdr, const uint32_t* pool, uint32_t pool_cap, uint32_t p1, uint32_t sbits,
                       const uint32_t* base, uint32_t nseg, uint32_t* order, uint8_t* ld_out, hipStream_t s) {
  hipLaunchKernelGGL(k_image_emit, dim3(((1u << p1) + 255) / 256), dim3(256), 0, s, hdr, pool, pool_cap, p1, sbits,
                     base, nseg, order, ld_out);
}

void launch_image_gather(const ulonglong2* pairs, const uint32_t* order, uint32_t nseg, uint32_t max_segs,
                         ulonglong2* out, hipStream_t s) {
  if (nseg) hipLaunchKernelGGL(k_image_gather, dim3(nseg), dim3(256), 0, s, pairs, order, max_segs, out);
}

void launch_image_ctl(const InitZero& z, DevCtl* ctl, const ImageCtl& c, uint32_t* hint, hipStream_t s) {
  uint64_t n = 256;
  for (int k = 0; k < kInitZero; ++k) n = std::max<uint64_t>(n, z.n[k]);
  hipLaunchKernelGGL(k_image_ctl, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, z, ctl, c, hint);
}

void launch_image_scatter(const ScatterArgs& a, hipStream_t s) {
  if (a.nseg) hipLaunchKernelGGL(k_image_scatter, dim3(a.nseg), dim3(256), 0, s, a);
}

}  // namespace pmdfc
