// image.hip -- device side of pmdfc_cceh_snapshot / pmdfc_cceh_restore
// (gfx950, wave64; the format: image.h).
//
// Snapshot: k_image_count / k_image_scan / k_image_emit put the segments in
// canonical (directory) order on the device, k_image_gather streams each
// 16 KiB segment from its arena id to its canonical slot of the image.
// Restore: k_image_ctl starts the control block and the per-batch words as a
// reset does, k_image_scatter copies canonical segment i to arena id i,
// rebuilds its occupancy words, local depth and directory entries, and checks
// every live key against the segment's hash prefix (k_image_scatter_sel: the
// same from segment src[i] of a compacted working image, compact.hip).
// The packed image (packed_image.h) and pmdfc_cceh_export_entries leave the
// empty slots out: k_image_live_count / _sums / _scan / _base give every
// canonical segment the number of entries stored before it, from occupancy
// words alone; k_image_pack compacts a segment to that offset by ballot rank
// (into the image, or into dense key and value arrays), k_image_unpack expands
// it again and then does k_image_scatter's work (scatter_segment).
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
// (T: uint32_t for the directory buckets; uint64_t for the block sums of the
// packed image's live counts, any number of them)
template <class T>
__global__ __launch_bounds__(1024) void k_image_scan(const T* __restrict__ cnt, uint32_t nb, T* __restrict__ base,
                                                     T* __restrict__ total) {
  __shared__ T s_sum[1024];
  const uint32_t t = threadIdx.x;
  const uint32_t per = (nb + 1023u) / 1024u;
  const uint32_t lo = min(t * per, nb), hi = min(lo + per, nb);
  T sum = 0;
  for (uint32_t i = lo; i < hi; ++i) sum += cnt[i];
  s_sum[t] = sum;
  __syncthreads();
  for (uint32_t d = 1; d < 1024u; d <<= 1) {
    const T v = t >= d ? s_sum[t - d] : (T)0;
    __syncthreads();
    s_sum[t] += v;
    __syncthreads();
  }
  T run = s_sum[t] - sum;
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

// What a restore does with canonical segment i (arena id = canonical index)
// once its pairs are in registers.  One workgroup of four waves; wave v holds
// slots [256 k + 64 v, +64) in step k, live[k] says whether the lane's slot
// holds an entry: one ballot of it is the two occupancy words 8 k + 2 v and
// 8 k + 2 v + 1.
__device__ __forceinline__ void scatter_segment(const ScatterArgs& a, uint32_t i, ulonglong2 (&p)[4],
                                                const bool (&live)[4]) {
  const uint32_t lane = threadIdx.x & 63u, v = threadIdx.x >> 6;
  const uint2 d = a.desc[i];
  const uint32_t start = d.x, L = d.y;
  const uint32_t Ll = L - a.sbits;         // local hash bits
  const uint32_t top = kMaxDepth - a.sbits;  // start counts 2^-top of the shard's space
  const uint64_t prefix = ((uint64_t)a.shard << Ll) | (start >> (top - Ll));
  ulonglong2* dst = a.pairs + (size_t)i * kSlots;
  uint32_t bad = 0;
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k) {
    if (!live[k]) p[k].y = 0;
    dst[k * 256u + threadIdx.x] = p[k];
    const uint64_t m = __ballot(live[k]);
    if (lane == 0) {
      uint32_t* o = a.occ + (size_t)i * 32u + k * 8u + v * 2u;
      o[0] = (uint32_t)m;
      o[1] = (uint32_t)(m >> 32);
    }
    // reserved keys are never stored; a live key sits in the segment its
    // top L hash bits select
    bad += live[k] && (p[k].x == kInvalid || p[k].x == kSentinel || (hash64(p[k].x) >> (64u - L)) != prefix) ? 1u
                                                                                                              : 0u;
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

// the version-1 image: segment i whole, occupancy is key != INVALID
__global__ __launch_bounds__(256) void k_image_scatter(ScatterArgs a) {
  const uint32_t i = blockIdx.x;
  const ulonglong2* src = a.img + (size_t)i * kSlots;
  ulonglong2 p[4];
  bool live[4];
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k) p[k] = ld_pair_l2(src + k * 256u + threadIdx.x);
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k) live[k] = p[k].x != kInvalid;
  scatter_segment(a, i, p, live);
}

// a compacted working image (compact.hip): canonical segment i is the whole
// segment src[i] of the image
__global__ __launch_bounds__(256) void k_image_scatter_sel(ScatterArgs a) {
  const uint32_t i = blockIdx.x;
  const ulonglong2* src = a.img + (size_t)a.src[i] * kSlots;
  ulonglong2 p[4];
  bool live[4];
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k) p[k] = ld_pair_l2(src + k * 256u + threadIdx.x);
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k) live[k] = p[k].x != kInvalid;
  scatter_segment(a, i, p, live);
}

// ---- the packed image (packed_image.h): count, scan, rank

// entries of the wave's lanes below this one in ballot m
__device__ __forceinline__ uint32_t below_lane(uint64_t m) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// The segment's 16 ballots of 64 slots each (s_m, slot order) -> pre[k] = the
// entries below the 64-slot group 4 k + v that wave v holds in step k; returns
// the segment's entry count.
__device__ __forceinline__ uint32_t group_ranks(const uint64_t* s_m, uint32_t v, uint32_t (&pre)[4]) {
  uint32_t run = 0;
#pragma unroll
  for (uint32_t g = 0; g < 16; ++g) {
    if ((g & 3u) == v) pre[g >> 2] = run;
    run += (uint32_t)__popcll(s_m[g]);
  }
  return run;
}

// cnt[i] = the entries of canonical segment i by its 32 occupancy words: eight
// lanes per segment, 16 B each.  order == nullptr: occ is in canonical order
// (an image's occupancy region); else segment i's words are those of arena id
// de_seg(order[i]).
__global__ __launch_bounds__(256) void k_image_live_count(const uint32_t* __restrict__ occ,
                                                          const uint32_t* __restrict__ order, uint32_t max_segs,
                                                          uint32_t nseg, uint32_t* __restrict__ cnt) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  const uint32_t i = t >> 3, q = t & 7u;
  uint32_t c = 0;
  if (i < nseg) {
    const uint32_t sid = order ? de_seg(order[i]) : i;
    if (!order || sid < max_segs) {  // (no entry of a sound directory fails this)
      const uint4 w = *reinterpret_cast<const uint4*>(occ + (size_t)sid * 32u + q * 4u);
      c = (uint32_t)(__popc(w.x) + __popc(w.y) + __popc(w.z) + __popc(w.w));
    }
  }
  c += __shfl_xor((int)c, 1);
  c += __shfl_xor((int)c, 2);
  c += __shfl_xor((int)c, 4);
  if (i < nseg && q == 0) cnt[i] = c;
}

// One block of 256 threads over kLiveScanBlock = 1024 counts, four per thread:
// c[] the thread's counts, the return value the sum of the block's counts
// before them, total the block's sum (at most 2^20: in 32 bits).
__device__ __forceinline__ uint32_t block_scan4(const uint32_t* __restrict__ cnt, uint32_t n, uint32_t (&c)[4],
                                                uint32_t& total) {
  __shared__ uint32_t s_w[4];
  const uint32_t lane = threadIdx.x & 63u, v = threadIdx.x >> 6;
  const uint32_t i0 = blockIdx.x * kLiveScanBlock + threadIdx.x * 4u;
  uint32_t sum = 0;
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) {
    c[j] = i0 + j < n ? cnt[i0 + j] : 0u;
    sum += c[j];
  }
  uint32_t x = sum;  // inclusive over the wave
  for (uint32_t d = 1; d < 64u; d <<= 1) {
    const uint32_t y = (uint32_t)__shfl_up((int)x, d);
    if (lane >= d) x += y;
  }
  if (lane == 63u) s_w[v] = x;
  __syncthreads();
  uint32_t off = 0;
  total = 0;
#pragma unroll
  for (uint32_t u = 0; u < 4; ++u) {
    if (u < v) off += s_w[u];
    total += s_w[u];
  }
  return off + x - sum;
}

__global__ __launch_bounds__(256) void k_image_live_sums(const uint32_t* __restrict__ cnt, uint32_t n,
                                                         uint64_t* __restrict__ sums) {
  uint32_t c[4], total;
  block_scan4(cnt, n, c, total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// base[i] = offs[block] + the counts before i in its block: 64 bits, nseg x
// 1024 can pass 2^32
__global__ __launch_bounds__(256) void k_image_live_base(const uint32_t* __restrict__ cnt, uint32_t n,
                                                         const uint64_t* __restrict__ offs,
                                                         uint64_t* __restrict__ base) {
  uint32_t c[4], total;
  uint64_t run = offs[blockIdx.x] + block_scan4(cnt, n, c, total);
  const uint32_t i0 = blockIdx.x * kLiveScanBlock + threadIdx.x * 4u;
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) {
    if (i0 + j < n) base[i0 + j] = run;
    run += c[j];
  }
}

// Snapshot (kExport false) and entry export (true).  One workgroup of four
// waves per canonical segment, k_image_gather's load shape.  Per step one
// ballot of key != INVALID is the wave's two occupancy words; the 16 ballots
// of the segment go through LDS, a lane's rank is the entries of the lower
// 64-slot groups plus those of the lower lanes of its own.  The live lanes of
// a wave store one contiguous run at base[i] + rank.  The ballots must count
// what the occupancy words did (cnt[i], an engine invariant): no store lands
// at a rank >= cnt[i], and a segment that disagrees is counted in *bad.
template <bool kExport>
__global__ __launch_bounds__(256) void k_image_pack(PackArgs a) {
  __shared__ uint64_t s_m[16];
  const uint32_t i = blockIdx.x;
  const uint32_t lane = threadIdx.x & 63u, v = threadIdx.x >> 6;
  const uint32_t sid = de_seg(a.order[i]);
  if (sid >= a.max_segs) {  // (no entry of a sound directory)
    if (threadIdx.x == 0) atomicAdd(a.bad, 1u);
    return;
  }
  const ulonglong2* src = a.pairs + (size_t)sid * kSlots;
  ulonglong2 p[4];
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k) p[k] = ld_pair_l2(src + k * 256u + threadIdx.x);
  uint64_t m[4];
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k) {
    m[k] = __ballot(p[k].x != kInvalid);
    if (lane == 0) s_m[k * 4u + v] = m[k];
  }
  __syncthreads();
  uint32_t pre[4];
  const uint32_t n = group_ranks(s_m, v, pre);
  const uint32_t cnt = a.cnt[i];
  const uint64_t base = a.base[i];
  if (threadIdx.x == 0 && n != cnt) atomicAdd(a.bad, 1u);
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k) {
    if (!kExport && lane == 0) {
      uint32_t* o = a.occ_out + (size_t)i * 32u + k * 8u + v * 2u;
      o[0] = (uint32_t)m[k];
      o[1] = (uint32_t)(m[k] >> 32);
    }
    const uint32_t rank = pre[k] + below_lane(m[k]);
    if (p[k].x != kInvalid && rank < cnt) {
      if (kExport) {
        if (a.keys_out) __builtin_nontemporal_store(p[k].x, a.keys_out + base + rank);
        if (a.vals_out) __builtin_nontemporal_store(p[k].y, a.vals_out + base + rank);
      } else {
        st_pair_nt(a.pairs_out + base + rank, p[k]);
      }
    }
  }
}

// Restore from a packed image: segment i's 32 occupancy words come from the
// image, each lane tests its own bit and takes its rank as k_image_pack does;
// live lanes load pairs[base[i] + rank], the others hold {INVALID, 0}.  Then
// scatter_segment.  (The host has compared the sum of the counts with the
// header's live count, which fits the buffer: base[i] + rank < live.  A lane
// that would still read past it holds INVALID in a live slot, which
// scatter_segment counts.)
__global__ __launch_bounds__(256) void k_image_unpack(ScatterArgs a) {
  __shared__ uint64_t s_m[16];
  const uint32_t i = blockIdx.x;
  const uint32_t lane = threadIdx.x & 63u, v = threadIdx.x >> 6;
  if (threadIdx.x < 16u) {
    const uint32_t* w = a.occ_img + (size_t)i * 32u + threadIdx.x * 2u;
    s_m[threadIdx.x] = (uint64_t)w[0] | ((uint64_t)w[1] << 32);
  }
  __syncthreads();
  uint32_t pre[4];
  group_ranks(s_m, v, pre);
  const uint64_t base = a.base[i];
  ulonglong2 p[4];
  bool live[4];
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k) {
    const uint64_t m = s_m[k * 4u + v];
    live[k] = (m >> lane) & 1u;
    const uint64_t idx = base + pre[k] + below_lane(m);
    p[k] = make_ulonglong2(kInvalid, 0);
    if (live[k] && idx < a.live) p[k] = ld_pair_l2(a.img + idx);
  }
  scatter_segment(a, i, p, live);
}

}  // namespace

void launch_image_count(const uint64_t* hdr, const uint32_t* pool, uint32_t pool_cap, uint32_t p1, uint32_t sbits,
                        uint32_t* cnt, uint32_t* base, uint32_t* total, hipStream_t s) {
  const uint32_t nb = 1u << p1;
  hipLaunchKernelGGL(k_image_count, dim3((nb + 255) / 256), dim3(256), 0, s, hdr, pool, pool_cap, p1, sbits, cnt);
  hipLaunchKernelGGL(k_image_scan<uint32_t>, dim3(1), dim3(1024), 0, s, cnt, nb, base, total);
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
  if (!a.nseg) return;
  if (a.occ_img)
    hipLaunchKernelGGL(k_image_unpack, dim3(a.nseg), dim3(256), 0, s, a);
  else if (a.src)
    hipLaunchKernelGGL(k_image_scatter_sel, dim3(a.nseg), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(k_image_scatter, dim3(a.nseg), dim3(256), 0, s, a);
}

void launch_image_live_scan(const uint32_t* occ, const uint32_t* order, uint32_t max_segs, uint32_t nseg,
                            const LiveScan& w, hipStream_t s) {
  const uint32_t nblk = live_scan_blocks(nseg);
  hipLaunchKernelGGL(k_image_live_count, dim3((nseg + 31) / 32), dim3(256), 0, s, occ, order, max_segs, nseg, w.cnt);
  hipLaunchKernelGGL(k_image_live_sums, dim3(nblk), dim3(256), 0, s, w.cnt, nseg, w.sums);
  hipLaunchKernelGGL(k_image_scan<uint64_t>, dim3(1), dim3(1024), 0, s, w.sums, nblk, w.offs, w.offs + nblk);
  hipLaunchKernelGGL(k_image_live_base, dim3(nblk), dim3(256), 0, s, w.cnt, nseg, w.offs, w.base);
}

void launch_image_pack(const PackArgs& a, uint32_t nseg, hipStream_t s) {
  if (!nseg) return;
  if (a.pairs_out)
    hipLaunchKernelGGL(k_image_pack<false>, dim3(nseg), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(k_image_pack<true>, dim3(nseg), dim3(256), 0, s, a);
}

}  // namespace pmdfc
