// cceh_kernels.h -- launcher declarations for cceh_kernels.hip / bloom.hip
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cceh_device.h"
#include "launch_plan.h"
#include "../../include/pmdfc_cceh.h"

namespace pmdfc {

// st == null: vout receives 16-B {value, status} records (routing responses)
void launch_get(bool count, const uint64_t* keys, uint64_t* vout, uint8_t* st, uint64_t n, Geo g,
                const ulonglong2* pairs, uint32_t* partials, hipStream_t s);
// mixed batches, two exact ways (cceh_kernels.hip): the INSERT set --
// k_mixed_prep (every op's status, the batch's inserted keys in iset, ipos /
// icnt: per slot the key's insert position and a several-inserts flag) then
// k_mixed_get_iset (early answers; the Gets that need it probe the set) --
// or the JOIN -- k_mixed_get (statuses, early answers, the other Gets mark
// their keys' bits in jbits: status kStJoin), then k_mixed_join (the inserts
// whose bit is set put their keys into the set: per slot the count icnt and
// the first position ipos), then k_part resolves the kStJoin Gets.  early: 1 a
// single-copy hit, 2 linked to its insert (elink), 3 a non-wrapping
// single-copy hit.  A Get left pending sets ctl->pget = tag.  hint_ins:
// host-mapped, the batch's insert count (the host's choice of the next mode).
// The five kernels take one argument struct by value; the engine fills it once
// per batch (cceh_engine.hip fill_mixed_launch), the launchers add only the
// kernel or template instance, the grid and the n == 0 return.
struct MixedArgs {
  // the batch
  const uint8_t* ops;
  const uint64_t* keys;
  const uint64_t* vin;   // (the verify pass: a linked Get takes its insert's value)
  uint8_t* st;
  uint64_t* vout;
  uint64_t n;
  // the table view
  Geo g;
  const ulonglong2* pairs;
  // the key set and the join filter
  uint64_t* iset;        // the batch's inserted keys (insert set) or joined keys (join), open addressing
  uint64_t imask;        // its slots - 1
  uint32_t* ipos;        // per set slot: the key's first insert position (~0 in an empty slot)
  uint32_t* icnt;        // per set slot: insert set, 1 if inserted more than once; join, the key's inserts
  uint32_t* islot;       // per op: its insert's set slot (~0: none), what the verify pass empties
  uint32_t* icount;      // per 256-op block: its pending inserts
  uint32_t* jbits;       // the joining Gets' filter (kJoinWords, kJoinReps replicas)
  // the early answers
  uint8_t* early;        // per op: 0 none, 1 / 3 a single-copy hit, 2 linked to its insert
  uint32_t* elink;       // per op: the linked insert's position (early 2)
  // the control words
  DevCtl* ctl;
  uint32_t* loss0;       // ctl->loss_events before the batch
  ulonglong2* drops;     // the drop log (cceh_device.h kDropLog)
  // the scalars
  uint32_t tag;          // the batch's epoch, never 0 (ctl->pget, ctl->njoin)
  uint32_t ups;          // last-writer-wins Insert: every hit depends on the batch's inserts of its key
  uint32_t* hint_ins;    // host-mapped: the batch's insert count, or null
  uint32_t join;         // this batch goes by the join (else by the insert set)
};
void launch_mixed_prep(const MixedArgs& a, hipStream_t s);
void launch_mixed_get_iset(const MixedArgs& a, hipStream_t s);
void launch_mixed_get(const MixedArgs& a, hipStream_t s);
void launch_mixed_join(const MixedArgs& a, hipStream_t s);
// after the batch: linked Gets take their insert's outcome; early hits whose
// key a split of the batch dropped are placed before / after that split's
// insert through the drop log (PMDFC_ST_SPLIT_LOST only if the log overflowed)
void launch_mixed_verify(const MixedArgs& a, hipStream_t s);
// upsert batches: pre-batch slot of each Insert's key (0xFFFF absent); ops may
// be null (insert-only), kvs = u64 words from one key to the next
void launch_upsert_probe(const uint64_t* keys, uint32_t kvs, const uint8_t* ops, uint64_t n, Geo g,
                         const ulonglong2* pairs, uint16_t* upos, hipStream_t s);
// the smallest live local depth -> *out (set to ~0 before)
void launch_min_ldep(const uint8_t* ldep, const DevCtl* ctl, uint32_t max_segs, uint32_t* out, hipStream_t s);
// directory buckets p1 -> p1n bits (every segment's local depth >= sbits + p1n)
void launch_rebucket(const uint64_t* old_hdr, uint64_t* hdr, uint32_t p1, uint32_t p1n, hipStream_t s);
// Fixed sub-directory slots: once the table is at its final bucket resolution
// (p1 == p1max: the bucket numbering never changes again), a sub-directory of
// at most 2^kFixedBits entries lives at pool offset w * kFixedSlot, the pool
// region [0, 2^p1max * kFixedSlot) being reserved for them, and grows there in
// place.  The first apply pass then loads it speculatively with the bucket's
// header and records (one dependent round trip less) and keeps it if the
// header points there.  Everything else is allocated past that region.
// (128 entries: a 2^28-key table at 2^13 buckets has sub-directories of
// 64-128 entries; 2 MiB of pool per 2^14 buckets.)
constexpr uint32_t kFixedBits = 7;
constexpr uint32_t kFixedSlot = 1u << kFixedBits;
// fixed: the initial sub-directories go to their fixed slots (p1 == p1max and
// db0 <= kFixedBits); else to the pool at `region`
// the control block of a fresh table (and the host-mapped hint), in stream order
// word arrays a reset zeroes in k_init_segments' launch (p[k]: n[k] u32 words)
constexpr int kInitZero = 6;
struct InitZero {
  uint32_t* p[kInitZero];
  uint64_t n[kInitZero];
};
void launch_init_segments(ulonglong2* pairs, uint32_t* occ, uint8_t* ldep, uint32_t* pool,
                          uint64_t* hdr, uint32_t nseg, uint32_t depth, uint32_t p1, uint32_t fixed,
                          uint32_t region, const InitZero& z, DevCtl* ctl, uint32_t pool_cur, uint32_t* hint,
                          hipStream_t s);
#ifdef __HIPCC__
// What a fresh table (k_init_segments) and a restored one (k_image_ctl) share.
// Thread i of the grid zeroes word i of each array of z.
__device__ __forceinline__ void zero_batch_words(const InitZero& z, uint64_t i) {
#pragma unroll
  for (int k = 0; k < kInitZero; ++k)
    if (i < z.n[k]) z.p[k][i] = 0;
}
// One whole block of 256 threads: the control block of a table of nsegs
// segments with every counter zero, and the host-mapped segment-count hint.
// True on the one thread that then fills in depth_count[].
__device__ __forceinline__ bool start_ctl(DevCtl* ctl, uint32_t nsegs, uint32_t max_ld, uint32_t pool_cur,
                                          uint32_t* hint) {
  uint32_t* w = reinterpret_cast<uint32_t*>(ctl);
  for (uint32_t j = threadIdx.x; j < sizeof(DevCtl) / 4; j += 256) w[j] = 0;
  __syncthreads();
  if (threadIdx.x != 0) return false;
  ctl->nsegs = nsegs;
  ctl->max_ld = max_ld;
  ctl->pool_cur = pool_cur;
  if (hint) __hip_atomic_store(hint, nsegs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  return true;
}
#endif

// image.hip (pmdfc_cceh_snapshot / pmdfc_cceh_restore, image.h)
// Canonical order on the device, the walk of pmdfc_cceh_dump: cnt[w] = the
// distinct segments of bucket w (an entry is a segment's first when its index
// in the sub-directory is a multiple of the segment's stride); base[] = their
// exclusive scan over the 2^p1 buckets, *total the segment count; then
// order[i] = the directory entry {arena id, local depth} of canonical segment
// i and ld_out[i] its local depth (i < nseg).
void launch_image_count(const uint64_t* hdr, const uint32_t* pool, uint32_t pool_cap, uint32_t p1, uint32_t sbits,
                        uint32_t* cnt, uint32_t* base, uint32_t* total, hipStream_t s);
void launch_image_emit(const uint64_t* hdr, const uint32_t* pool, uint32_t pool_cap, uint32_t p1, uint32_t sbits,
                       const uint32_t* base, uint32_t nseg, uint32_t* order, uint8_t* ld_out, hipStream_t s);
// the 16 KiB of arena segment de_seg(order[i]) -> out + i * 1024, the values
// of empty slots zeroed
void launch_image_gather(const ulonglong2* pairs, const uint32_t* order, uint32_t nseg, uint32_t max_segs,
                         ulonglong2* out, hipStream_t s);
// Restore.  Everything the kernels index with comes from the host, which
// derived it from validated local depths: desc[i] = {segment i's start in the
// shard's hash space in units of 2^-30 of the whole space, local depth}, hdr
// the rebuilt bucket headers (already on the device).
struct ImageCtl {
  uint32_t nsegs, pool_cur, max_ld;
  uint32_t depth_count[32];
};
// the per-batch words zeroed and the control block set, as k_init_segments does
void launch_image_ctl(const InitZero& z, DevCtl* ctl, const ImageCtl& c, uint32_t* hint, hipStream_t s);
struct ScatterArgs {
  const ulonglong2* img;  // nseg x 1024 pairs in canonical order
  const uint2* desc;
  const uint64_t* hdr;
  uint32_t nseg, p1, sbits, shard;
  ulonglong2* pairs;
  uint32_t* occ;
  uint8_t* ldep;
  uint32_t* pool;
  uint32_t* bad;  // += live keys whose hash prefix is not their segment's, and reserved keys
  // A packed image (packed_image.h), else occ_img == nullptr: img is then the
  // `live` dense pairs, occ_img the image's nseg x 32 occupancy words, base[i]
  // the pairs before segment i (launch_image_live_scan over occ_img).
  const uint32_t* occ_img;
  const uint64_t* base;
  uint64_t live;
  // A compacted working image (compact.hip), else src == nullptr: canonical
  // segment i is segment src[i] of img (a version-1 pairs region with gaps).
  const uint32_t* src;
};
// segment i of the image -> arena id i: pairs, occupancy words, local depth,
// its directory entries; the live keys are hashed against the segment's prefix
void launch_image_scatter(const ScatterArgs& a, hipStream_t s);
// The packed image and the entry export: per-segment live counts from the
// occupancy words (the pairs are not read) and their exclusive scan in 64 bits,
// for any nseg: sums per block of kLiveScanBlock counts, a scan of the sums,
// an add-back.  order != nullptr: occ is the engine's, segment i's words those
// of arena id de_seg(order[i]); nullptr: occ is an image's occupancy region.
constexpr uint32_t kLiveScanBlock = 1024;
inline uint32_t live_scan_blocks(uint32_t nseg) { return (nseg + kLiveScanBlock - 1) / kLiveScanBlock; }
struct LiveScan {
  uint64_t* base;  // nseg
  uint64_t* sums;  // live_scan_blocks(nseg)
  uint64_t* offs;  // live_scan_blocks(nseg) + 1: the last is the grand total
  uint32_t* cnt;   // nseg
};
void launch_image_live_scan(const uint32_t* occ, const uint32_t* order, uint32_t max_segs, uint32_t nseg,
                            const LiveScan& w, hipStream_t s);
// Canonical segment i's stored pairs, in slot order, to rank base[i] on:
// into a packed image (pairs_out and occ_out, its occupancy region, written
// from the same ballots), or, pairs_out == nullptr, into the dense arrays
// keys_out / vals_out (either may be nullptr).  *bad += the segments whose
// keys do not count what their occupancy words did.
struct PackArgs {
  const ulonglong2* pairs;
  const uint32_t* order;
  uint32_t max_segs;
  const uint32_t* cnt;
  const uint64_t* base;
  uint32_t* occ_out;
  ulonglong2* pairs_out;
  uint64_t* keys_out;
  uint64_t* vals_out;
  uint32_t* bad;
};
void launch_image_pack(const PackArgs& a, uint32_t nseg, hipStream_t s);
// compact.hip (pmdfc_cceh_compact): one round of sibling
// merges inside a gathered version-1 pairs region.  The rows are indexed by
// the ORIGINAL canonical index and never move; a merged pair lives on in its
// left child's row and image slot, the right child's row is marked dead.
constexpr uint32_t kCompactDead = 0xFFu;  // ld[i] & 0xFF of a segment merged into its left sibling
struct CompactArgs {
  ulonglong2* img;     // nseg x 1024 pairs in canonical order
  uint32_t* ld;        // local depth | the round that made the segment << 8 (0: as gathered)
  const uint32_t* pos; // the segment's start in the hash space, in units of 2^-30 (never changes for a left child)
  uint32_t* cnt;       // live entries (launch_image_live_scan)
  uint32_t* next;      // the next live index (nseg: none)
  uint32_t* refused;   // sticky: the pair (i, next[i]) drops in the replay, its leaves never change
  uint32_t* merged;    // += 1 per pair merged in this round
  uint32_t nseg, d0, fill_limit;
  uint32_t round;      // 1, 2, ...
};
void launch_compact_merge(const CompactArgs& a, hipStream_t s);
// flatten the bucketed directory for pure-Get batches: *bits = p1 + max db
// (the physical depth), flat[x] = the sub-directory entry of index x
void launch_flatten(const uint64_t* hdr, const uint32_t* pool, uint32_t p1, uint32_t* flat,
                    uint32_t* bits, uint32_t max_bits, hipStream_t s);
void launch_popcount(const uint32_t* occ, uint64_t nwords, unsigned long long* out, hipStream_t s);
// CCEH::FindAnyway x n: first copy of each key in slot order (wave per key)
void launch_find_anyway(const uint64_t* keys, uint64_t* vout, uint8_t* st, uint64_t n, Geo g,
                        const ulonglong2* pairs, hipStream_t s);
void launch_hash(const uint64_t* keys, uint64_t* out, uint64_t n, hipStream_t s);
void launch_gen_keys(uint64_t seed, uint64_t start, uint64_t* out, uint64_t n, hipStream_t s);
void launch_owner(const uint64_t* keys, uint64_t n, uint32_t sbits, uint32_t* owner, uint32_t* idx,
                  hipStream_t s);
void launch_bounds(const uint32_t* sorted_owner, uint64_t n, uint32_t ngroups, uint64_t* starts,
                   hipStream_t s);

// part.hip, bucket.hip (insert / mixed path)
constexpr uint32_t kPartTile = 8192;       // ops per partition block (A/B: 4096 32.4 us per 1M, 8192 30.9, 16384 57)
constexpr uint32_t kMaxPartBlocks = 512;   // => max_batch <= 4M
constexpr uint32_t kMaxP1 = 14;            // <= 16384 directory buckets
constexpr uint32_t kServeWavesMax = 64;     // serving waves (PMDFC_SERVE_WAVES_MAX)
constexpr uint32_t kMaxPartBits = 13;      // <= 8192 partition buckets
// A partition bucket's record region is cut into kPartSubs sub-regions, one
// per XCD-sharing class of k_part blocks (blocks b and b + 8 share an XCD,
// MI355X_MICROARCH.md "Workgroup dispatch"): block b writes sub-region b % 8
// only, so every line of a sub-region is dirtied in ONE XCD's L2 and leaves
// it whole, and each region cursor is bumped by 1/8 of the blocks.
constexpr uint32_t kPartSubs = 8;
uint32_t part_blocks(uint64_t n);
constexpr uint32_t kSplitStamps = 8192;
// Split requests are granted through kGShards pairs of counters, one per XCD
// (bucket w -> shard w % 8, the XCD its first-pass wave runs on), each word
// on a 128-B line of its own: {child segments [0,32) | requesting buckets
// [32,64)} and the sub-directory pool entries requested in this batch.  A
// contended single word serializes at ~88 atomics/us, far below the rate of
// a split-heavy batch's ~8k requests.
constexpr uint32_t kGShards = 8;
constexpr uint32_t kGStride = 32;  // u64 words per shard: the segment word at 0, the pool word at 16
constexpr uint32_t kChunkWave = 256;  // ops per k_apply / k_bucket wave chunk (mean load: 128)
constexpr uint32_t kSplitCap = 64;    // split requests per directory bucket and round
// per-bucket cumulative counters: lines, waited, splits, split loss, runs,
// rounds, {max rounds | max local depth << 16 | growths << 32}, spare
constexpr int kWStat = 8;
// partition record buffers (records, cursors, k_part overflow slots):
// pmdfc_cceh_insert_batches partitions groups of up to kRecBufs / 2 batches
// ahead (pipe_group); the per-batch pipeline of the routed loop (pipe_batch)
// reuses a buffer kRecBufs batches later
#ifndef PMDFC_RECBUFS
#define PMDFC_RECBUFS 16  // (A/B builds)
#endif
constexpr uint32_t kRecBufs = PMDFC_RECBUFS;

// The argument structs of part.hip's and bucket.hip's kernels, passed by
// value.  The engine fills them from the batch's BatchPlan (cceh_engine.hip
// plan_batch, then fill_part_launch / fill_bucket_args and the callers that
// patch a batch kind's fields); the launchers add only what the batch's
// LaunchPlan (launch_plan.h) names: the kernel, the grid, mode and gate.

// k_part
struct PartArgs {
  const uint64_t* keys;
  const uint64_t* vin;
  const uint8_t* ops;   // null: insert-only batch (k_part resolves statuses itself)
  uint8_t* st;
  uint64_t n;
  uint32_t kvs;         // u64 words from one op's key (value) to the next: 1 (arrays), or 2 for {key, value} records
  uint32_t sbits, shard;
  uint32_t pbits, sbb;  // partition bucket bits (directory bucket bits - sbb); sbb: sub-bucket bits
  uint32_t cap;         // record slots per partition bucket region
  uint32_t capx;        // ... per sub-region (cap / kPartSubs)
  uint64_t ovf_base;    // first overflow record slot
  ulonglong2* rkv;      // records: {key, value}
  uint32_t* rop;        // records: op index | sub-bucket << 22 | Get << 31
  uint16_t* robk;       // partition bucket of each overflow record
  uint32_t* cursor;     // this batch's cursors, [sub-region][partition bucket] (zero on entry)
  uint32_t* ovf;        // this batch's overflow cursor (zero on entry)
  uint32_t* povf;       // [tile][partition bucket] overflow slot of a run that does not fit its sub-region
  uint64_t* stamps;     // debug: 8 wall-clock stamps per block, or null
  // a medium mixed batch (one partition block, k_medium after): statuses
  // initialized here (k_mixed_prep's rule), Get values zeroed, and the
  // partition buckets that received ops listed ([0] count, then the buckets)
  uint32_t init;
  uint64_t* vout;
  uint32_t* touched;
  // a general mixed batch: its joining Gets (kStJoin) are resolved here from
  // the join's per-slot counts (k_mixed_get, k_mixed_join)
  const uint64_t* iset;
  uint64_t imask;
  const uint32_t* icnt;
  const uint32_t* ipos;
  uint8_t* early;
  uint32_t* elink;
  DevCtl* ctl;
  uint32_t tag;
};
void launch_part(const PartArgs& a, hipStream_t s);

// the apply passes, k_bucket, k_medium, k_mixed_small / k_mixed_tiny, k_serve
struct BucketArgs {
  const ulonglong2* rkv;
  const uint32_t* rop;
  const uint16_t* robk;
  uint64_t n;            // batch size (op indices are < n)
  uint32_t chunk;        // ops per wave chunk (<= kChunkWave)
  uint32_t cap;          // records per partition bucket region
  uint32_t capx;         // ... per sub-region (kPartSubs of them)
  uint64_t ovf_base;
  const uint32_t* cursor;  // this batch's [kPartSubs][partition buckets] cursors, then the overflow cursor
  const uint32_t* ovf;
  uint32_t* cursor_next;   // cleared here for the next batch (clear_next)
  uint32_t* ovf_next;
  uint32_t clear_next;     // the first apply pass zeroes the other parity's cursors (one batch per call);
                           // 0 when the next batch is already being partitioned
  uint64_t* hdr;
  uint32_t* pool;
  uint32_t pool_cap;
  uint32_t p1, sbb, sbits, shard;  // p1: directory bucket bits
  uint32_t pfix;         // p1 == p1max: small sub-directories live (and grow) in their fixed slots (kFixedBits)
  ulonglong2* pairs;
  uint32_t* occ;
  uint8_t* ldep;
  uint64_t* vout;        // mixed only
  uint8_t* st;
  uint32_t mixed;
  uint32_t upsert;       // last-writer-wins Insert (PMDFC_CFG_UPSERT)
  const uint16_t* upos;  // upsert: pre-batch slot of each op's key (k_upsert_probe), first pass only
  uint32_t max_segments;
  DevCtl* ctl;
  uint64_t* wstat;       // per directory bucket: kWStat cumulative counters
  ulonglong2* wl_kv;     // per directory bucket: kChunkWave parked {key, value}
  uint32_t* wl_op;       // ... and their rop words
  uint32_t* wl_n;        // per directory bucket: parked count, or kBigBucket
  uint64_t* stamps;      // debug: 16 wall-clock stamps per wave, or null
  // pipelined split rounds (an apply pass requests and grants -> k_split)
  uint2* req;            // kSplitCap split requests per directory bucket
  uint32_t* reqop;       // ... the batch position of each request's insert
  ulonglong2* drops;     // mixed batches with early answers: the drop log (cceh_device.h kDropLog), else null
  uint32_t* need;        // per bucket: sub-directory bits those requests need (0: none)
  uint32_t* gbase;       // per bucket: first child segment id granted
  uint32_t* ngrant;      // per bucket: requests granted, committed by the owner's next pass
  uint32_t* newoff;      // per bucket: pool offset of the grown sub-directory
  uint64_t* gsh;         // [2][kGShards] grant shard words by batch parity (kGStride apart)
  uint4* gsplit;         // [2][kGShards][gcap] the requested splits by segment offset in their shard:
                         // {request word, w | i << 14 | entry << 20, pool offset, nr | need << 8}
  uint32_t gcap;         // splits per shard (kSplitCap x the shard's buckets)
  uint32_t* act;         // [2^p1] buckets with requests (k_split -> k_apply_parked)
  uint32_t* fbl;         // [2^p1max] per bucket: bit 0 k_apply_fast declined it (-> k_apply_fb), bits 1+ declines so far
  uint32_t* hint;        // device-mapped pinned word: k_apply_parked leaves the segment count after
                         // this batch's grants there (host hint)
  uint32_t mode;         // (launcher) 0 first pass; 2 parked-op pass without split requests, the one
                         // the host sends (the kernels also take 1: a parked-op pass that requests)
  // worklists: the passes after k_apply visit only the buckets that have work
  uint32_t* fin;         // [2][2^p1] by batch parity: k_bucket's worklist (count: ctl->nfin[par])
  uint32_t par;          // this batch's parity
  // gated mixed batches: both apply variants are launched and exactly one
  // runs.  gate 1 (MIXED kernels) runs iff ctl->pget == gate_tag (k_mixed_get
  // left a Get pending), gate 2 (the insert-only kernels) iff not; 0: always.
  // gate: (launcher, from the LaunchPlan); gate_tag: != 0 for a gated batch
  uint32_t gate, gate_tag;
  uint32_t* mseen;       // host-mapped: k_apply<true> stores gate_tag when it runs (PlanIn::mixed_small)
};
// A general batch's bucket passes: the arguments and the launches they go to
struct BucketLaunch {
  BucketArgs a;
  LaunchPlan plan;
  uint64_t* split_stamps;  // debug: 8 stamps for each of the first kSplitStamps splits, or null
};
// The passes in order, each a switch over L.plan (nothing for an empty batch):
// the first pass over the batch's records (mode 0), insert-only and mixed
// variant; k_apply_fb where the plan has it follow a lean first pass; after
// the split round the pass over the parked ops (mode 2); k_bucket
void launch_first(const BucketLaunch& L, hipStream_t s);
void launch_fallback(const BucketLaunch& L, hipStream_t s);
void launch_parked(const BucketLaunch& L, hipStream_t s);
void launch_final(const BucketLaunch& L, hipStream_t s);
// a batch of at most kPartTile ops after its one-block partition (k_part with
// a touched list): every listed partition bucket's directory buckets through
// the final pass, records walked in batch order (k_medium)
void launch_medium(const BucketArgs& a, const uint32_t* touched, hipStream_t s);
// a whole batch of n <= kChunkWave ops in one launch (k_mixed_small, k_mixed_tiny
// up to 64); ops == null: insert-only.  a.st / a.vout are the outputs; inputs
// may be host-mapped
void launch_mixed_small(const BucketArgs& a, const uint8_t* ops, const uint64_t* keys, const uint64_t* vin,
                        hipStream_t s);

// k_split: a fixed grid looping over the splits the first pass requested, in
// shard-major order (their count from the grant shards; a bucket that does not
// fit is denied whole).  Built from the batch's BucketArgs (bucket.hip split_args).
struct SplitArgs {
  uint32_t par;        // the batch's parity: its grant shards
  uint32_t pfix;       // small sub-directories grow in their fixed slots
  uint64_t* stamps;    // BucketLaunch::split_stamps
  const uint64_t* gsh;
  const uint4* gsplit;
  uint32_t gcap;
  uint32_t* act;       // out: the buckets with requests (k_apply_parked's worklist)
  uint32_t* gbase;     // out, per bucket: first child id, grants, pool offset, sub-directory bits
  uint32_t* ngrant;
  uint32_t* newoff;
  uint32_t* need;
  uint32_t max_segments, pool_cap;
  ulonglong2* pairs;
  uint32_t* occ;
  uint8_t* ldep;
  DevCtl* ctl;
  const uint32_t* reqop;  // batch position of each request's insert (drop log)
  ulonglong2* drops;      // the drop log, or null
  uint32_t team_max;      // split lists up to this long go by teams of four waves (PMDFC_SPLIT_TEAM_MAX)
};
// the split round: every split the first pass requested, on the plan's grid
// with its team_max (k_split grants child ids / sub-directory space itself)
void launch_split_round(const BucketLaunch& L, hipStream_t s);

// the persistent serving kernel of the per-op front-end (k_serve, a wave per ring)
struct ServeArgs {
  BucketArgs a;                 // the engine at launch (st / vout: 64-entry device scratch)
  const pmdfc_serve_req* req;   // device mappings of the host rings (wave w: places w * ring_size ...)
  pmdfc_serve_resp* resp;
  pmdfc_serve_ctl* ctl;         // one per wave
  uint64_t ring_size, head0;    // head0: one wave's first place; several waves start at their ctl->head
  uint32_t nwaves;              // 1: one wave from head0; else wave w serves ring w from ctl[w].head
  uint8_t* cbf;                 // counting BF counters, or null
  uint64_t cbf_m;
  uint32_t cbf_k;
};
void launch_serve(const ServeArgs& sa, hipStream_t s);

// ubench.hip
void launch_gather64(const void* buf, uint64_t nlines, const uint32_t* table, uint32_t tmask,
                     uint64_t nops, uint64_t seed, uint64_t* out, hipStream_t s);
int launch_gather(const void* buf, uint64_t nbytes, uint32_t line, uint32_t depth, const uint32_t* table,
                  uint32_t tmask, uint64_t nops, uint64_t seed, uint64_t* out, uint64_t omask, hipStream_t s);
int launch_scatter16(void* buf, uint64_t nbytes, uint32_t depth, uint64_t nops, uint64_t seed, hipStream_t s);

// bloom.hip
void launch_bloom_add(uint64_t* bitmap, uint64_t nbits, uint32_t k, const uint64_t* keys,
                      uint64_t n, hipStream_t s);
void launch_bloom_probe(const uint64_t* bitmap, uint64_t nbits, uint32_t k, const uint64_t* keys,
                        uint8_t* out, uint64_t n, hipStream_t s);
void launch_bloom_get(const uint64_t* bitmap, uint64_t nbits, uint32_t k, const uint64_t* keys,
                      uint64_t* vout, uint8_t* st, uint64_t n, Geo g, const ulonglong2* pairs,
                      hipStream_t s);

// cbf.hip (server counting bloom filter, counting_bloom_filter.h)
constexpr uint64_t kCbfChunk = 4096;  // counter bytes per pack step (counters padded to it)
void launch_cbf_insert(uint8_t* cnt, uint64_t m, uint32_t k, const uint64_t* keys,
                       const uint8_t* ops, uint64_t n, hipStream_t s);
void launch_cbf_query(const uint8_t* cnt, uint64_t m, uint32_t k, const uint64_t* keys,
                      uint8_t* out, uint64_t n, hipStream_t s);
void launch_cbf_delete(uint8_t* cnt, uint64_t m, uint32_t k, const uint64_t* keys, uint8_t* out,
                       uint64_t n, uint32_t* flag, hipStream_t s);
void launch_cbf_pack(const uint8_t* cnt, uint64_t m, uint64_t* bm, hipStream_t s);
// The stored keys of arena segments [0, min(ctl->nsegs, max_segs)) (nsegs read
// on the device): rebuild counts each into cnt, audit queries each; out[0] +=
// the stored keys, audit: out[1] += those whose Query is false.  out is not
// zeroed here; the rebuild takes out == null.
constexpr uint32_t kCbfScanBlocks = 2048;  // the loop's grid: 8 workgroups of four waves per CU
void launch_cbf_scan(bool audit, const ulonglong2* pairs, const DevCtl* ctl, uint64_t max_segs, uint8_t* cnt,
                     uint64_t m, uint32_t k, unsigned long long* out, hipStream_t s);

// erase.hip (batched key removal).  One Erase batch: the
// probe writes the final statuses of the ops that remove nothing and each
// hit's arena segment id into seg_in (max_segs for the others); a stable radix
// sort of {segment id, batch index} over sort_bits bits brings every
// segment's ops together in batch order; the heads of the runs are listed in
// work (their count in *cursor); one wave per run applies its ops in order.
constexpr uint32_t kErrEraseGuard = 1u << 17;  // DevCtl::err: a loop guard of k_erase_apply tripped
struct EraseArgs {
  const uint64_t* keys;  // n
  uint8_t* st;           // n
  uint64_t n;            // <= max_batch
  Geo g;                 // with the flat directory
  ulonglong2* pairs;
  uint32_t* occ;
  DevCtl* ctl;
  uint32_t max_segs;
  // the scratch of the handle, each row max_batch entries
  uint32_t *seg_in, *seg_out;  // per op / sorted: the segment id
  uint32_t *idx_in, *idx_out;  // per op / sorted: the batch index
  uint32_t* work;              // sorted positions of the run heads
  uint32_t* cursor;            // their count
  void* tmp;                   // the sort's temporary storage
  size_t tmp_bytes;
  uint32_t sort_bits;          // ceil_log2(max_segs) + 1
};
// temporary storage of the sort for batches of at most max_batch ops
hipError_t erase_sort_temp_bytes(uint64_t max_batch, uint32_t sort_bits, size_t* bytes);
hipError_t launch_erase(const EraseArgs& a, hipStream_t s);

// match.hip (EraseMatching): one launch over arena ids
// [0, min(ctl->nsegs, max_segs)), a wave per segment; a tripped guard sets
// kErrEraseGuard.  out is not zeroed here.
struct MatchArgs {
  uint64_t mask;
  const uint64_t* patterns;  // n, device memory
  uint32_t n;                // 1 .. PMDFC_MATCH_MAX
  ulonglong2* pairs;
  uint32_t* occ;
  DevCtl* ctl;
  uint32_t max_segs;
  unsigned long long* out;   // [0] += entries removed, [1] += segments changed, [2] += segments cleared, [3] = ids visited
};
void launch_erase_matching(const MatchArgs& a, hipStream_t s);

// trace.hip (replay_KV trace ingestion)
struct TraceLine {
  uint64_t key;  // (inode << 32) + offset
  uint32_t op;   // PMDFC_OP_INSERT (W) / PMDFC_OP_GET (R, or no ops)
  uint32_t pad;
};
uint64_t trace_nl_tiles(uint64_t nbytes);
size_t trace_scan_temp_bytes(uint64_t nlines);
hipError_t launch_trace_newlines(const char* text, uint64_t nbytes, uint64_t* nl, uint64_t* d_nnl,
                                 uint64_t* tile_cnt, uint64_t* tile_off, void* temp,
                                 size_t temp_bytes, hipStream_t s);
hipError_t launch_trace_lines(const char* text, uint64_t nbytes, const uint64_t* nl, uint64_t nnl,
                              uint64_t nlines, TraceLine* lines, uint64_t* pages, uint64_t* cum,
                              unsigned long long* first_bad, uint64_t num_data, uint64_t* info,
                              void* temp, size_t temp_bytes, hipStream_t s);
void launch_trace_expand(const TraceLine* lines, const uint64_t* cum, const uint64_t* pages,
                         uint64_t nlines, uint64_t nout, uint8_t* ops, uint64_t* keys,
                         hipStream_t s);

// extent.hip (Insert_extent / Get_extent, both reference variants)
hipError_t launch_extent_count(bool src, const uint64_t* keys, const uint64_t* cl, const uint64_t* lens,
                               uint64_t n, uint64_t* cnt, uint64_t* cum, hipStream_t s);
void launch_extent_expand(bool src, const uint64_t* keys, const uint64_t* cl, const uint64_t* lens,
                          const uint64_t* vals, uint64_t n, const uint64_t* cum, uint64_t* out_k,
                          uint64_t* out_v, hipStream_t s);
uint32_t extent_targets_per_key(bool src);
void launch_extent_targets(const uint64_t* keys, const uint64_t* cl, uint64_t n, uint32_t per,
                           uint64_t* out, hipStream_t s);
void launch_extent_pick(const uint64_t* v, const uint8_t* st, uint64_t n, uint32_t per, uint64_t* vout,
                        uint8_t* sout, hipStream_t s);

// route.hip (multi-GPU: fixed-capacity owner blocks for equal-split
// all-to-alls, with a per-owner carry so no op is ever dropped)
constexpr uint32_t kRouteTile = 1024;     // ops per routing block
constexpr uint32_t kRouteMaxOwners = 16;  // shard_bits <= 4
constexpr uint32_t kRouteNone = 0xFFFFFFFFu;  // rowpos of a padding row
constexpr uint32_t kCarryWords = 3;       // carried records: key, value, op (width <= 3 used)
struct RouteArgs {
  const uint64_t* keys;
  const uint64_t* vals;  // width >= 2
  const uint8_t* ops;    // width 3
  const uint8_t* keep;   // nullable: ops with keep[i] == 0 stay home (ST_FILTERED)
  uint64_t n;
  uint32_t sbits;
  uint32_t width;        // u64 words per record: key[, value[, op]]
  uint64_t cap;          // record slots per owner block
  uint64_t cc;           // carry slots per owner
  uint32_t base;         // call-global output index of op 0
  uint64_t* send;        // [2^sbits][cap][width]
  uint32_t* rowpos;      // [2^sbits * cap] call-global output index of the row, or kRouteNone
  uint64_t* vals_out;    // nullable, call-global: 0 for ops that are not sent
  uint8_t* st_out;       // call-global: ST_FILTERED / ST_ROUTE_OVERFLOW for ops that are not sent
  uint32_t* tile_cnt;    // [route_tiles(n)][2^sbits]
  const uint32_t* cin;   // [2^sbits] ops carried in (the previous pack's cout)
  uint32_t* cout;        // [2^sbits] ops carried out
  const uint64_t* crec_in;   // [2^sbits][cc][kCarryWords]
  uint64_t* crec_out;
  const uint32_t* cpos_in;   // [2^sbits][cc] call-global output index
  uint32_t* cpos_out;
  uint32_t* ovf;         // ops dropped because the carry was full (sticky count)
  // the local block: owner self_g's rows go to self_dst ([cap][width], the
  // receive buffer's slot for this rank) instead of send (null: send)
  uint32_t self_g;
  uint64_t* self_dst;
};
uint32_t route_tiles(uint64_t n);
void launch_route_pack(const RouteArgs& a, hipStream_t s);
void launch_route_split(const uint64_t* recv, uint64_t rows, uint32_t W, uint64_t* keys, uint64_t* vals,
                        uint8_t* ops, hipStream_t s);
void launch_route_resp(const uint64_t* vals, const uint8_t* st, uint64_t rows, void* resp, hipStream_t s);
// rows [self_lo, self_hi) are read from back_self (the local block's
// responses where the engine wrote them), the others from back
void launch_route_unpack(const void* back, uint32_t W, const uint32_t* rowpos, uint64_t rows, uint64_t* vals_out,
                         uint8_t* st_out, hipStream_t s, const void* back_self = nullptr, uint64_t self_lo = 0,
                         uint64_t self_hi = 0);
void launch_route_carried(const uint32_t* cnt, uint32_t G, uint64_t* out, hipStream_t s);
// Get dedupe within tiles of 4096 Gets (LDS table)
void launch_route_dedupe(const uint64_t* keys, const uint8_t* keep_in, uint64_t n, uint32_t base, uint8_t* keep_out,
                         uint32_t* lead_out, hipStream_t s);
void launch_route_fill(const uint32_t* lead, uint64_t n, uint64_t* vals, uint8_t* st, hipStream_t s);

}  // namespace pmdfc
