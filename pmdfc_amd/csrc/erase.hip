// erase.hip -- batched key removal that keeps the probe invariant.
//
// Invariant I: for every stored entry at slot j with window start
// w = (h & 0xFF) * 4, every slot of [w, j] is occupied, cyclically, and
// (j - w) mod 1024 < 32.  Every probe's early exit at the first empty slot,
// the cluster argument of the split replay and the early answers of mixed
// batches rest on it.  Inserts keep it because they never free a slot; Erase
// frees slots and restores it before it returns.
//
// Erase(key), serially: repeat until the probe misses --
//   1. probe the key's 32-slot window in probe order up to the first empty
//      slot; no match: stop;
//   2. p = the first match;
//   3. backward shift: among the slots p+1 .. p+31 (cyclic) up to the first
//      empty one, take the first entry c whose own window start lies at or
//      before p, (c - w_c) mod 1024 >= (c - p) mod 1024; copy pair c to p, set
//      p = c and look again; when there is none, write {INVALID, 0} at p and
//      clear its occupancy bit.
// An entry only moves backwards inside its own window, so I holds after every
// Erase; copies of one key share w and keep their order; an entry at p + 32 or
// later cannot have p in its window, so 31 slots per step are enough; the hole
// advances on every step and an entry moves back at most 31 slots in all, so
// the loop ends (guarded all the same: kErrEraseGuard in error_flags).
//
// A batch equals its ops applied one by one in batch order.  Ops of different
// segments commute (Erase touches one segment's pairs and occupancy row and
// nothing else), so: k_erase_probe finds each op's segment and answers the ops
// that remove nothing (erases only remove: a key absent before the batch is
// absent at its turn); a stable sort by segment id puts each segment's ops
// together in batch order; k_erase_heads lists the runs; k_erase_apply gives
// each run to one wave, which owns the segment for the launch.  A batch that
// repeats one stored key n times gives one wave a run of n ops: slow, correct.
#include "cceh_device.h"
#include "cceh_kernels.h"
#include "erase_device.h"

#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>

namespace pmdfc {

constexpr uint8_t kStErased = 12;  // PMDFC_ST_ERASED

// k_get_u's shape, one key per quad: the statuses of the ops that remove
// nothing are final here; a hit leaves its status to k_erase_apply.
__global__ __launch_bounds__(256) void k_erase_probe(EraseArgs a) {
  const uint64_t op = ((uint64_t)blockIdx.x * 256u + threadIdx.x) >> 2;
  const uint32_t q = threadIdx.x & 3u;
  if (blockIdx.x == 0 && threadIdx.x == 0) *a.cursor = 0;
  if (op >= a.n) return;
  const uint64_t key = a.keys[op];
  const uint64_t h = hash64(key);
  uint32_t seg = a.max_segs;  // past the arena: no work for k_erase_apply
  uint8_t s = 0;              // PMDFC_ST_MISS
  if (reserved_key(key)) {
    s = 3;  // PMDFC_ST_RESERVED_KEY
  } else if (wrong_shard(h, a.g.sbits, a.g.shard)) {
    s = 8;  // PMDFC_ST_WRONG_SHARD
  } else {
    const uint32_t sid = de_seg(dir_entry(a.g, h));
    uint64_t val;
    uint32_t lines;
    if (sid < a.max_segs && quad_probe(a.pairs + (size_t)sid * kSlots, key, h, q, &val, &lines)) seg = sid;
  }
  if (q == 0) {
    a.seg_in[op] = seg;
    a.idx_in[op] = (uint32_t)op;
    if (seg == a.max_segs) a.st[op] = s;
  }
}

// Sorted position j starts a run if its segment is inside the arena and
// differs from its predecessor's; one atomic per wave on the cursor.
__global__ __launch_bounds__(256) void k_erase_heads(const uint32_t* __restrict__ seg, uint64_t n, uint32_t max_segs,
                                                     uint32_t* __restrict__ work, uint32_t* __restrict__ cursor) {
  const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  const uint32_t lane = __lane_id() & 63u;
  bool head = false;
  if (j < n) {
    const uint32_t sg = seg[j];
    head = sg < max_segs && (j == 0 || seg[j - 1] != sg);
  }
  const uint64_t m = __ballot(head);
  if (!m) return;
  const int first = __builtin_ctzll(m);
  uint32_t base = 0;
  if ((int)lane == first) base = atomicAdd(cursor, (uint32_t)__popcll(m));
  base = (uint32_t)__shfl((int)base, first);
  if (head) work[base + (uint32_t)__popcll(m & ((1ULL << lane) - 1))] = (uint32_t)j;
}

// One wave per listed run, the run's ops in batch order, the rule above per
// op with all 64 lanes (erase_key, erase_device.h).  The wave owns the segment
// and its occupancy row; it reads back what it wrote, so pairs are loaded
// through L2 (ld_pair_l2) and its stores are drained before the next probe.
__global__ __launch_bounds__(256) void k_erase_apply(EraseArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = (blockIdx.x * 256u + threadIdx.x) >> 6;
  const uint32_t nwaves = gridDim.x * 4u;
  const uint32_t nruns = *a.cursor;
  bool trip = false;
  for (uint32_t r = wave; r < nruns; r += nwaves) {
    uint32_t j = a.work[r];
    const uint32_t seg = a.seg_out[j];
    ulonglong2* sp = a.pairs + (size_t)seg * kSlots;
    uint32_t* row = a.occ + (size_t)seg * 32u;
    for (; j < a.n && a.seg_out[j] == seg; ++j) {
      const uint32_t op = a.idx_out[j];
      const uint64_t key = a.keys[op];
      const bool erased = erase_key(sp, row, key, lane, trip) != 0;
      if (lane == 0) a.st[op] = erased ? kStErased : (uint8_t)0;
    }
  }
  if (trip && lane == 0) atomicOr(&a.ctl->err, kErrEraseGuard);
}

hipError_t erase_sort_temp_bytes(uint64_t max_batch, uint32_t sort_bits, size_t* bytes) {
  uint32_t* none = nullptr;
  *bytes = 0;
  return rocprim::radix_sort_pairs(nullptr, *bytes, none, none, none, none, (size_t)max_batch, 0u, sort_bits,
                                   (hipStream_t)0);
}

constexpr uint32_t kEraseApplyBlocks = 2048;  // the loop's grid: 8 workgroups of four waves per CU

hipError_t launch_erase(const EraseArgs& a, hipStream_t s) {
  if (!a.n) return hipSuccess;
  hipLaunchKernelGGL(k_erase_probe, dim3((unsigned)((a.n + 63) / 64)), dim3(256), 0, s, a);
  size_t bytes = a.tmp_bytes;
  const hipError_t e = rocprim::radix_sort_pairs(a.tmp, bytes, a.seg_in, a.seg_out, a.idx_in, a.idx_out, (size_t)a.n,
                                                 0u, a.sort_bits, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_erase_heads, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, s,
                     (const uint32_t*)a.seg_out, a.n, a.max_segs, a.work, a.cursor);
  const uint64_t blocks = std::min<uint64_t>((a.n + 3) / 4, kEraseApplyBlocks);
  hipLaunchKernelGGL(k_erase_apply, dim3((unsigned)blocks), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace pmdfc
