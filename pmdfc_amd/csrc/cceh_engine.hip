// cceh_engine.hip -- host side of the MI355X batched CCEH engine: the table's
// part of the C-ABI declared in include/pmdfc_cceh.h.
//
// The engine owns its HBM (segment arena, occupancy bitmaps, local depths,
// bucketed directory, batch workspaces) and drives the kernels of
// cceh_kernels.hip / part.hip / bucket.hip.  Every batched entry point only
// ENQUEUES work on the caller's stream; nothing on the Insert/Get/mixed path
// reads device state back (bucket.hip has the details of every pass):
//   Insert : k_part -> k_apply_fast (first pass; requests and reserves its
//            splits) -> k_split -> k_apply_parked -> k_bucket (final pass)
//   mixed  : k_mixed_prep -> k_mixed_get -> k_part -> the
//            same bucket passes (gated insert-only / mixed variants) ->
//            k_mixed_verify
//   <= 64 ops : k_mixed_tiny; <= 256: k_mixed_small (1 launch)
//   <= 8192   : k_part (one block) -> k_medium (2 launches)
//   Get    : k_get_u (1 launch; k_flatten first after inserts)
// Splits and directory growth are decided and done on the device (per-bucket
// sub-directories), so a batch never needs a host decision; only a table
// still coarser than its bucket resolution syncs once per sub-batch.
//
// This file holds the table alone.  The rest of the C-ABI lives in one host
// file per kernel file; what they may call here is listed in engine_state.h:
//   image_host.hip  (image.hip)   snapshot / restore (synchronous), packed image, entry export
//   route_host.hip  (route.hip)   route_by_shard, the block router, split / respond
//   dist_host.hip   (RCCL)        communicators and the native routed batches
//   filter_host.hip (bloom.hip, cbf.hip)  bloom and counting bloom filters
//   trace_host.hip  (trace.hip)   trace ingestion
//   extent_host.hip (extent.hip)  extent Insert / Get
//   ubench.hip                    the microbenchmarks' wrappers, below their kernels
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/pmdfc_cceh.h"
#include "cceh_device.h"
#include "cceh_kernels.h"
#include "engine_state.h"
#include "host_common.h"
#include "knobs.h"

using namespace pmdfc;

// ------------------------------------------------------------------ helpers

int pmdfc::read_ctl(pmdfc_cceh* t, hipStream_t s) {
  HIPCHK(hipMemcpyAsync(t->hctl, t->ctl, sizeof(DevCtl), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return PMDFC_OK;
}

// the bounds of the *_batches entry points: non-decreasing, no batch past max_batch
static int check_bounds(const uint64_t* bounds, uint32_t nbatches, uint64_t max_batch) {
  for (uint32_t i = 0; i < nbatches; ++i) {
    if (bounds[i + 1] < bounds[i]) return fail(PMDFC_ERR_ARG, "bounds must be non-decreasing");
    if (bounds[i + 1] - bounds[i] > max_batch) return fail(PMDFC_ERR_ARG, "a batch exceeds max_batch");
  }
  return PMDFC_OK;
}

// The per-bucket counters (the slots of every bucket geometry so far) and,
// from them and the control block read_ctl left in hctl, the deepest local
// depth: stats() sums the rest, dump() needs the depth alone.
static int read_wstat(pmdfc_cceh* t, std::vector<uint64_t>& ws, uint32_t& max_ld) {
  ws.resize((size_t)kWStat << t->p1max);
  HIPCHK(hipMemcpy(ws.data(), t->wstat, ws.size() * 8, hipMemcpyDeviceToHost));
  max_ld = t->hctl->max_ld;
  for (size_t i = 6; i < ws.size(); i += kWStat) max_ld = std::max<uint32_t>(max_ld, (uint32_t)((ws[i] >> 16) & 0xFF));
  return PMDFC_OK;
}

// per parity: kPartSubs cursors per partition bucket + the overflow cursor,
// padded to 256 B so both blocks are aligned (one fill kernel per memset)
static size_t cursor_block(uint32_t npb) { return ((size_t)npb * kPartSubs + 1 + 63) & ~(size_t)63; }

// Directory bucket geometry for p1 bits: the partition buckets and their
// record regions (a sub-region holds twice its mean share plus 16).  k_part
// block b writes sub-region b % kPartSubs, so a sub-region takes the records
// of ceil(tiles / kPartSubs) whole tiles: a batch of fewer than kPartSubs
// tiles puts a full tile's share in each (an engine whose max_batch is below
// kPartSubs * kPartTile would otherwise overflow into the shared area, which
// sends every bucket of the batch past the lean first pass).
static uint32_t part_cap(uint32_t max_batch, uint32_t p1, uint32_t sbb) {
  const uint64_t npb = 1ULL << (p1 - sbb);
  const uint64_t tiles = ((uint64_t)max_batch + kPartTile - 1) / kPartTile;
  const uint64_t sub_ops = (tiles + kPartSubs - 1) / kPartSubs * kPartTile;
  const uint64_t per_sub = (sub_ops + npb - 1) / npb;
  return (uint32_t)((2 * per_sub + 16) * kPartSubs);
}

// One debug stamp set (kn.stamps): 16 words per directory bucket (2^p1max
// rows, the bucket passes), then 8 per k_part block of a max_batch batch, then
// 8 for each of the first kSplitStamps splits.
static uint64_t stamp_part_off(const pmdfc_cceh* t) { return 16ULL << t->p1max; }
static uint64_t stamp_split_off(const pmdfc_cceh* t) { return stamp_part_off(t) + 8ULL * part_blocks(t->max_batch); }
static uint64_t stamp_words(const pmdfc_cceh* t) { return stamp_split_off(t) + 8ULL * kSplitStamps; }

// What ONE batch's launches are filled from, chosen by plan_batch before the
// batch's first launch (pipe_group keeps a group's plans until their passes).
struct BatchPlan {
  uint32_t rb = 0;   // record buffer: records, cursors, k_part overflow
  uint32_t par = 0;  // batch parity: the bucket passes' per-batch words (grant shards, worklists)
  uint32_t sbb = 0;  // sub-bucket bits (partition buckets = 2^(p1 - sbb))
  uint32_t cap = 0;  // record slots per partition bucket region
  uint32_t cp = 0;   // the coarse partition (sbb == kCpSbb, k_apply_fast_cp)
  uint32_t wide = 0, fb = 0;   // the lean first pass is the wide one; k_apply_fb is launched
  uint64_t* stamps = nullptr;  // the batch's debug stamp set, or null
};

// Insert-only, non-upsert batches of a table at its bucket resolution whose
// lean pass is the narrow one take the coarse partition (2^(p1 - 3)
// partition buckets of 8 directory buckets: k_part writes runs of ~8 records
// per tile and bucket instead of ~1, k_apply_fast_cp stages them per
// workgroup); the rest the fine one.  The lean pass is the wide one once the
// table has more segments per bucket than the narrow one's 32-entry
// sub-directories hold (about 20: a bucket's deepest segment sits ~1.5 levels
// below the mean).  The count is a hint the device leaves in pinned memory
// (k_apply_parked), read without a sync, so it may lag the batches in flight:
// either variant is exact, and each hands the buckets it cannot take to
// k_apply_fb.  records: the batch has a partition, so it takes the next stamp
// set, in partition order (k_mixed_small and k_serve have none).
static BatchPlan plan_batch(pmdfc_cceh* t, bool insert_only, uint64_t n, bool records = true) {
  BatchPlan b;
  b.rb = t->rb;
  b.par = t->parity;
  const uint32_t spb = __atomic_load_n(t->h_hint, __ATOMIC_RELAXED) >> t->p1;  // segments per bucket
  b.wide = spb > kWideSegs ? 1u : 0u;
  b.fb = spb > kFbSegs ? 1u : 0u;
  // records per (partition bucket, sub-region): a sub-region takes the
  // records of ceil(tiles / kPartSubs) tiles; the staging holds kCpPre, so
  // the mean must stay near 2/3 of it (1M ops at p1 = 13: 128)
  const uint64_t tiles = (n + kPartTile - 1) / kPartTile;
  const uint64_t per_sub = t->p1 > kCpSbb ? (((tiles + kPartSubs - 1) / kPartSubs) * kPartTile) >> (t->p1 - kCpSbb) : ~0ull;
  const bool cp = insert_only && !t->upsert && !b.wide && t->p1 == t->p1max && per_sub <= 128 &&
                  process_knobs().cp && process_knobs().fast_apply;
  b.cp = cp ? 1u : 0u;
  b.sbb = cp ? kCpSbb : (t->p1 > kMaxPartBits ? t->p1 - kMaxPartBits : 0);
  b.cap = part_cap(t->max_batch, t->p1, b.sbb);
  if (records && t->stamps)
    b.stamps = t->stamp_last = t->stamps + (uint64_t)(t->stamp_seq++ % t->kn.stamp_rot) * stamp_words(t);
  return b;
}

// (the batch before zeroed this buffer's cursors at its own geometry's
// positions: a one-batch path of another geometry zeroes the whole block)
static int zero_stale_cursors(pmdfc_cceh* t, const BatchPlan& b, hipStream_t s) {
  if (t->clean_sbb != ~0u && t->clean_sbb != b.sbb)
    HIPCHK(hipMemsetAsync(t->cursor + (size_t)b.rb * t->cblk, 0, t->cblk * sizeof(uint32_t), s));
  return PMDFC_OK;
}

// How each path leaves the handle (finish_batch; every path also invalidates
// the flattened Get directory):
//   flip   the batch parity flips.  Not after k_medium (the final pass, splits
//          inline): it never touches the per-batch words, and only a general
//          batch's first pass clears the other parity's, so a flip would hand
//          the next general batch the stale words of the one before this.
//   next   the record buffer ring advances (the batch had a partition).
//   clean  its first pass (or k_medium) zeroed the next buffer's cursors at its
//          own positions: clean_sbb is its sbb.  Pipelined partitions zero
//          whole blocks instead; pipe_end zeroes the next and sets ~0u.
//   count  batches += 1; a general batch is a sub-batch of a call that counts
//          once itself (insert_ramped, pmdfc_cceh_mixed).
enum BatchPath { kPathSmall, kPathMedium, kPathGeneral, kPathPiped, kPathServe };
static constexpr struct { bool flip, next, clean, count; } kFinish[] = {
    {false, false, false, true},   // kPathSmall
    {false, true, true, true},     // kPathMedium
    {true, true, true, false},     // kPathGeneral (insert_one, mixed_one)
    {true, true, false, true},     // kPathPiped (pipe_batch, pipe_group)
    {false, false, false, false},  // kPathServe
};

static void finish_batch(pmdfc_cceh* t, const BatchPlan& b, BatchPath path) {
  const auto& f = kFinish[path];
  if (f.flip) t->parity = b.par ^ 1u;
  if (f.next) t->rb = (b.rb + 1) % kRecBufs;
  if (f.clean) t->clean_sbb = b.sbb;
  if (f.count) t->batches += 1;
  t->flat_valid = false;
}

// A table created small (CCEH_hybrid(2): 2 segments, so 2 directory buckets)
// gets finer buckets as it deepens.  While p1 < p1max, batches run as
// sub-batches of about 1,024 ops per directory bucket (A/B on CCEH_hybrid(2)
// config 2: 128 -> 5.12-5.15 Gops/s, 512 -> 5.54, 1,024 -> 5.65, 2,048 ->
// 5.48, 4,096 -> 5.27: fewer host round trips against longer final passes
// over oversized buckets) (a sub-batch sequence is
// the same serial op stream), and before each one the host reads the smallest
// live local depth (k_min_ldep) and, once every segment is at least
// sbits + p1' deep, rebuilds the bucket headers for p1' (k_rebucket: the
// sub-directories stay where they are).  The depth is the one an earlier
// call's copy left in pinned memory: the host waits for that copy only (one
// sub-batch back), so the stream keeps a sub-batch queued instead of
// draining.  Local depths only grow, so a value one sub-batch old is still a
// lower bound (init_state seeds it with the initial depth after waiting for
// the last such copy's event, so no copy of an earlier table lands after the
// seed; a reset is otherwise stream-ordered, without a device-wide sync).  A
// table at p1max pays nothing.
static int rebucket_now(pmdfc_cceh* t, hipStream_t s) {
  if (t->p1 >= t->p1max) return PMDFC_OK;
  if (t->minld_pending) HIPCHK(hipEventSynchronize(t->ev_minld));
  const uint32_t minL = __atomic_load_n(&t->h_depth[1], __ATOMIC_ACQUIRE);
  HIPCHK(hipMemsetAsync(t->minld, 0xFF, sizeof(uint32_t), s));
  launch_min_ldep(t->ldep, t->ctl, (uint32_t)t->max_segs, t->minld, s);
  HIPCHK(hipMemcpyAsync(&t->h_depth[1], t->minld, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIPCHK(hipEventRecord(t->ev_minld, s));
  t->minld_pending = true;
  if (minL <= t->sbits || minL > kMaxDepth) return PMDFC_OK;
  const uint32_t target = std::min<uint32_t>(t->p1max, minL - t->sbits);
  if (target <= t->p1) return PMDFC_OK;
  HIPCHK(hipMemcpyAsync(t->hdr_tmp, t->hdr, sizeof(uint64_t) << t->p1, hipMemcpyDeviceToDevice, s));
  launch_rebucket(t->hdr_tmp, t->hdr, t->p1, target, s);
  HIPCHK(hipGetLastError());
  t->p1 = target;
  t->flat_valid = false;
  t->rebuckets += 1;
  return PMDFC_OK;
}

// ops per sub-batch while the table is still coarser than p1max
// (PMDFC_RAMP_OPS per directory bucket, at least PMDFC_RAMP_MIN: tuning knobs)
static uint64_t ramp_batch(const pmdfc_cceh* t, uint64_t n) {
  if (t->p1 >= t->p1max) return n;
  const ProcessKnobs& K = process_knobs();
  return std::min<uint64_t>(n, std::max<uint64_t>(K.ramp_ops << t->p1, K.ramp_min));
}

// empty the mixed batches' key set (32 MB of fills at 1M-op batches, ~20 us)
static int clear_key_set(pmdfc_cceh* t, hipStream_t s) {
  HIPCHK(hipMemsetAsync(t->mx.iset, 0xFF, (t->mx.imask + 1) * sizeof(uint64_t), s));
  HIPCHK(hipMemsetAsync(t->mx.icnt, 0, (t->mx.imask + 1) * sizeof(uint32_t), s));
  HIPCHK(hipMemsetAsync(t->mx.ipos, 0xFF, (t->mx.imask + 1) * sizeof(uint32_t), s));
  HIPCHK(hipMemsetAsync(t->mx.jbits, 0, kJoinWords * sizeof(uint32_t), s));
  return PMDFC_OK;
}

// A mixed batch begins: the set is empty (emptied here if an earlier batch
// stopped between its prep and verify passes) and counts as in use until this
// batch's verify pass is enqueued.
static int open_key_set(pmdfc_cceh* t, hipStream_t s) {
  if (int rc = t->mx.iset_dirty ? clear_key_set(t, s) : PMDFC_OK) return rc;
  t->mx.iset_dirty = true;
  return PMDFC_OK;
}

// The host side of a table that starts over (a reset, or a restore of an
// image): p1 directory bucket bits, every segment at least min_ld deep, no
// batch run yet.
int pmdfc::start_host_state(pmdfc_cceh* t, hipStream_t s, uint32_t p1, uint32_t min_ld) {
  // (no earlier rebucket_now copy may land after the seed below: the event
  // is recorded right after that copy -- a device-wide sync would also wait
  // for every other stream, a serving wave included)
  if (t->minld_pending) HIPCHK(hipEventSynchronize(t->ev_minld));
  __atomic_store_n(&t->h_depth[1], min_ld, __ATOMIC_RELEASE);
  t->minld_pending = false;
  // the mixed batches' key set is empty between batches (each batch's verify
  // pass empties the slots it used), so a reset leaves it alone -- unless it
  // is not known empty (a new engine, or a batch that stopped between its prep
  // and verify passes): then emptied here (a cost the bench's reset at
  // every step must not pay)
  if (t->mx.iset_dirty) {
    if (int rc = clear_key_set(t, s)) return rc;
    t->mx.iset_dirty = false;
  }
  t->p1 = p1;
  t->clean_sbb = ~0u;
  t->batches = 0;
  t->parity = 0;
  t->rb = 0;
  t->flat_valid = false;
  return PMDFC_OK;
}

// the per-batch words a starting table needs zero (the kernel that starts its
// control block zeroes them in the same launch): the record cursors, the stat
// slots, the worklist counts, the decline flags, the grants, the grant shards
InitZero pmdfc::batch_words(const pmdfc_cceh* t) {
  InitZero z{};
  z.p[0] = t->cursor;
  z.n[0] = (uint64_t)kRecBufs * t->cblk;
  z.p[1] = reinterpret_cast<uint32_t*>(t->wstat);
  z.n[1] = (2ULL * kWStat) << t->p1max;
  z.p[2] = t->wl_n;
  z.n[2] = 1ULL << t->p1max;
  z.p[3] = t->fbl;
  z.n[3] = 1ULL << t->p1max;
  z.p[4] = t->ngrant;
  z.n[4] = 1ULL << t->p1max;
  z.p[5] = reinterpret_cast<uint32_t*>(t->gsh);
  z.n[5] = 2ULL * 2 * kGShards * kGStride;
  return z;
}

int pmdfc::init_state(pmdfc_cceh* t, hipStream_t s) {
  const uint32_t n0 = 1u << (t->D0 - t->sbits);
  if (int rc = start_host_state(t, s, t->p1_init, t->D0)) return rc;
  const uint32_t region = kFixedSlot << t->p1max;  // the fixed slots come first in the pool
  const uint32_t db0 = t->D0 - t->sbits - t->p1;
  const uint32_t fixed = (t->p1 == t->p1max && db0 <= kFixedBits) ? 1u : 0u;
  // the segments, the passes' per-bucket words and the control block with
  // the hint, in ONE kernel on s: a reset queues behind the work before it
  // without a host sync (the bench resets the table at every step)
  launch_init_segments(t->pairs, t->occ, t->ldep, t->pool, t->hdr, n0, t->D0, t->p1, fixed, region, batch_words(t),
                       t->ctl, region + (fixed ? 0u : n0), t->d_hint, s);
  return PMDFC_OK;
}

// The view of the plan's record buffer that PartArgs and BucketArgs share:
// the records with their overflow tags, the partition buckets' cursors with
// the overflow cursor after them, and the region sizes.
template <class Args>
static void fill_record_view(const pmdfc_cceh* t, const BatchPlan& b, Args& a) {
  const uint32_t p = b.rb, pbits = t->p1 - b.sbb;
  a.rkv = t->rkv + p * t->nrec;
  a.rop = t->rop + p * t->nrec;
  a.robk = t->robk + (size_t)p * t->max_batch;
  a.cursor = t->cursor + (size_t)p * t->cblk;
  a.ovf = a.cursor + ((size_t)kPartSubs << pbits);
  a.cap = b.cap;
  a.capx = b.cap / kPartSubs;
  a.ovf_base = (uint64_t)b.cap << pbits;
}

// The bucket kernels' arguments for the batch of plan b (A{}: the launchers'
// a.mode / a.gate, the gated mixed batches' gate_tag / mseen and the drop log
// stay zero unless the caller sets them).
static void fill_bucket_args(const pmdfc_cceh* t, const BatchPlan& b, BucketArgs& a, uint64_t n, uint8_t* st,
                             uint64_t* vout, bool mixed) {
  a.n = n;
  fill_record_view(t, b, a);
  a.chunk = (t->kn.chunk == 0 || t->kn.chunk > kChunkWave) ? kChunkWave : t->kn.chunk;
  a.cursor_next = t->cursor + (size_t)((b.rb + 1) % kRecBufs) * t->cblk;
  a.ovf_next = a.cursor_next + (a.ovf - a.cursor);
  a.clear_next = 1;
  a.hdr = t->hdr;
  a.pool = t->pool;
  a.pool_cap = (uint32_t)t->pool_cap;
  a.p1 = t->p1;
  a.sbb = b.sbb;
  a.sbits = t->sbits;
  a.shard = t->shard;
  a.pfix = t->p1 == t->p1max ? 1u : 0u;
  a.pairs = t->pairs;
  a.occ = t->occ;
  a.ldep = t->ldep;
  a.vout = vout;
  a.st = st;
  a.mixed = mixed ? 1u : 0u;
  a.upsert = t->upsert;
  a.upos = t->upos;
  a.max_segments = (uint32_t)t->max_segs;
  a.ctl = t->ctl;
  a.wstat = t->wstat;
  a.wl_kv = t->wl_kv;
  a.wl_op = t->wl_op;
  a.wl_n = t->wl_n;
  a.stamps = b.stamps;
  a.req = t->req;
  a.reqop = t->reqop;
  a.drops = nullptr;  // (mixed batches with early answers set it)
  a.need = t->need;
  a.gbase = t->gbase;
  a.ngrant = t->ngrant;
  a.newoff = t->newoff;
  a.gsh = t->gsh;
  a.gsplit = t->gsplit;
  a.gcap = t->gcap;
  a.act = t->act;
  a.fin = t->fin;
  a.fbl = t->fbl;
  a.par = b.par;
  a.hint = t->d_hint;
}

// The launch plan's inputs but for the hints: the batch's kind (a mixed batch
// is gated unless the table upserts), the process knobs, the bucket bits.
static PlanIn plan_in(const pmdfc_cceh* t, bool mixed) {
  const ProcessKnobs& K = process_knobs();
  PlanIn in{};
  in.mixed = mixed;
  in.upsert = t->upsert != 0;
  in.gated = mixed && !t->upsert;
  in.fast_apply = K.fast_apply;
  in.fast_lds_pad = K.fast_lds_pad;
  in.split_team_max = K.split_team_max;
  in.p1 = t->p1;
  return in;
}

// A general batch's bucket passes: the kernels' arguments and the launch plan
// (launch_plan.h), decided here once.  tag: a gated mixed batch's epoch.
static void fill_bucket_launch(const pmdfc_cceh* t, const BatchPlan& b, BucketLaunch& L, uint64_t n, uint8_t* st,
                               uint64_t* vout, bool mixed, uint32_t tag = 0, bool mixed_small = false) {
  fill_bucket_args(t, b, L.a, n, st, vout, mixed);
  L.split_stamps = b.stamps ? b.stamps + stamp_split_off(t) : nullptr;
  PlanIn in = plan_in(t, mixed);
  in.wide = b.wide;
  in.cp = b.cp;
  in.fb = b.fb;
  in.mixed_small = mixed_small;
  // the larger grids of the passes after the first while the table ramps,
  // or is still small for the batch (more than 32 ops per segment: windows
  // fill within the batch, the final pass has work): the CCEH_hybrid(2)
  // ramp 5.11 -> 5.75 Gops/s with them after p1max too, config 2 (16 ops per
  // segment at its start) 12.56 against 12.41 without (profiles/r05/grids/)
  const uint64_t segs = __atomic_load_n(t->h_hint, __ATOMIC_RELAXED);
  in.ramp = t->p1 < t->p1max || n > 32ull * std::max<uint64_t>(segs, 1);
  L.plan = plan_launches(in);
  L.a.gate_tag = in.gated ? tag : 0u;
  if (!L.plan.probe) L.a.upos = nullptr;  // (the first pass reads it only after k_upsert_probe)
}

// k_part's arguments for the batch of plan b (P{}: the medium batches' init /
// vout / touched and the mixed batches' join group stay zero unless the
// caller sets them); kvs: 1 for key / value arrays, 2 for records
static void fill_part_launch(const pmdfc_cceh* t, const BatchPlan& b, PartArgs& a, const uint8_t* ops,
                             const uint64_t* keys, const uint64_t* vin, uint32_t kvs, uint8_t* st, uint64_t n) {
  a.keys = keys;
  a.vin = vin;
  a.kvs = kvs ? kvs : 1u;
  a.ops = ops;
  a.st = st;
  a.n = n;
  a.sbits = t->sbits;
  a.shard = t->shard;
  a.pbits = t->p1 - b.sbb;
  a.sbb = b.sbb;
  fill_record_view(t, b, a);
  a.povf = t->povf + (size_t)b.rb * part_blocks(t->max_batch) * (1u << kMaxPartBits);
  a.stamps = b.stamps ? b.stamps + stamp_part_off(t) : nullptr;
}

// The mixed pre-pass and verify kernels' arguments for one general mixed batch
// of epoch tag, by the join or by the insert set.
static void fill_mixed_launch(const pmdfc_cceh* t, MixedArgs& a, const uint8_t* ops, const uint64_t* keys,
                              const uint64_t* vin, uint64_t* vout, uint8_t* st, uint64_t n, uint32_t tag, bool join) {
  const pmdfc_cceh::Mixed& m = t->mx;
  a.ops = ops;
  a.keys = keys;
  a.vin = vin;
  a.st = st;
  a.vout = vout;
  a.n = n;
  a.g = t->geo();
  a.pairs = t->pairs;
  a.iset = m.iset;
  a.imask = m.imask;
  a.ipos = m.ipos;
  a.icnt = m.icnt;
  a.islot = m.islot;
  a.icount = m.icount;
  a.jbits = m.jbits;
  a.early = m.early;
  a.elink = m.elink;
  a.ctl = t->ctl;
  a.loss0 = m.loss0;
  a.drops = m.drops;
  a.tag = tag;
  a.ups = t->upsert ? 1u : 0u;
  a.hint_ins = t->d_hint + kHintMixIns;
  a.join = join ? 1u : 0u;
}

// k_part's view of that batch: what resolves its joining Gets
static void fill_part_join(PartArgs& p, const MixedArgs& a) {
  p.iset = a.iset;
  p.imask = a.imask;
  p.icnt = a.icnt;
  p.ipos = a.ipos;
  p.early = a.early;
  p.elink = a.elink;
  p.ctl = a.ctl;
  p.tag = a.tag;
}

// The bucket passes of one insert / mixed batch, all on the stream, as the
// batch's launch plan names them: a first apply pass, ONE split round (a
// batch's grant shards hold one round of requests), the apply pass over the
// parked ops (it commits the round's splits first and requests none), then
// the final pass for whatever is still parked -- ops whose segment needs a
// second split in the same batch, rare enough that one pipelined round
// measured best (an empty round costs ~15 us of launches).
static void run_bucket_passes(pmdfc_cceh* t, const BucketLaunch& B, hipStream_t s) {
  t->timing.begin(PMDFC_K_PROCESS, s);
  launch_first(B, s);
  // the general first pass over the buckets the lean one declined: its own
  // launch (k_apply_fb, requesting splits for the split round) only where
  // declines are expected, a table past the wide pass's 128-entry
  // sub-directories; otherwise the rare declined bucket takes its first pass
  // in k_apply_parked (an empty k_apply_fb launch costs ~3.2 us a batch)
  if (B.plan.fb_class) {
    t->timing.begin(PMDFC_K_FINAL, s);  // (the fallback first pass is timed with the final pass)
    launch_fallback(B, s);
  }
  t->timing.begin(PMDFC_K_SPLIT, s);
  launch_split_round(B, s);
  t->timing.begin(PMDFC_K_PARKED, s);
  launch_parked(B, s);
  t->timing.begin(PMDFC_K_FINAL, s);
  launch_final(B, s);
}

// ------------------------------------------------------------------- C-ABI

// (every pmdfc_* function takes its C linkage from its declaration in
// include/pmdfc_cceh.h)

int pmdfc_abi_version(void) { return PMDFC_ABI_VERSION; }

static thread_local std::string g_err;  // the one error text per thread (host_common.h: last_error, fail)
std::string& pmdfc::last_error() { return g_err; }
const char* pmdfc_last_error(void) { return g_err.c_str(); }

uint32_t pmdfc_depth_for_hybrid(uint64_t init_cap) {
  return (uint32_t)(size_t)std::log2((double)init_cap);  // CCEH_hybrid.cpp:80
}

uint32_t pmdfc_depth_for_src(uint64_t init_cap) {
  return (uint32_t)(size_t)std::log2((double)(init_cap / kSlots));  // src/cceh.cpp:82
}

int pmdfc_cceh_create(const pmdfc_cceh_config_t* cfg, pmdfc_cceh_t** out) {
  if (!cfg || !out) return fail(PMDFC_ERR_ARG, "null argument");
  *out = nullptr;
  if (cfg->initial_depth < 1 || cfg->initial_depth > kMaxDepth)
    return fail(PMDFC_ERR_ARG, "initial_depth must be in [1, 30] (CCEH(initCap) needs initCap >= 2)");
  if (cfg->shard_bits > cfg->initial_depth || cfg->shard_bits > 16)
    return fail(PMDFC_ERR_ARG, "shard_bits must be <= initial_depth (and <= 16)");
  if (cfg->shard_bits && cfg->shard_id >= (1u << cfg->shard_bits))
    return fail(PMDFC_ERR_ARG, "shard_id out of range");
  if (cfg->max_batch == 0) return fail(PMDFC_ERR_ARG, "max_batch must be > 0");
  if (cfg->flags & ~PMDFC_CFG_UPSERT) return fail(PMDFC_ERR_ARG, "unknown flags");
  if ((uint64_t)cfg->max_batch > (uint64_t)kMaxPartBlocks * kPartTile)
    return fail(PMDFC_ERR_ARG, "max_batch must be <= 4194304");
  DevGuard g(cfg->device);
  auto* t = new pmdfc_cceh();
  t->cfg = *cfg;
  t->dev = cfg->device;
  t->D0 = cfg->initial_depth;
  t->sbits = cfg->shard_bits;
  t->shard = cfg->shard_id;
  t->max_batch = cfg->max_batch;
  t->upsert = (cfg->flags & PMDFC_CFG_UPSERT) ? 1u : 0u;
  const uint32_t Dl0 = t->D0 - t->sbits;
  const uint64_t n0 = 1ULL << Dl0;
  // directory buckets: about 128 ops each at max_batch (half a wave chunk),
  // never finer than the initial directory (a segment must not span two);
  // (64-op buckets measured slower: twice the waves, same latency per wave)
  // (floor: a routed engine's max_batch is 2^shard_bits padded owner blocks,
  // ~1.07x the ops it actually receives per batch)
  const uint32_t lgb = cfg->max_batch ? 31u - (uint32_t)__builtin_clz(cfg->max_batch) : 0u;
  const uint32_t p1t = lgb > 7 ? lgb - 7 : 0;
  // never finer than the initial directory at first (a segment must not
  // span two buckets); rebucket_now refines up to p1max as segments deepen
  t->kn = CreateKnobs::read();
  t->p1max = t->kn.p1max >= 0 ? (uint32_t)t->kn.p1max : std::min<uint32_t>(p1t, kMaxP1);
  t->p1_init = std::min<uint32_t>(t->p1max, Dl0);
  t->p1 = t->p1_init;
  uint64_t ms = cfg->max_segments;
  if (ms == 0) {
    size_t fr = 0, tot = 0;
    (void)hipMemGetInfo(&fr, &tot);
    ms = std::min<uint64_t>((uint64_t)(fr * 0.5) / (kSlots * 16 + 160), 1ULL << 22);
  }
  ms = std::max<uint64_t>(ms, n0 + 1);
  if (ms > kMaxSegments) ms = kMaxSegments;  // 26-bit segment ids in directory entries
  t->max_segs = ms;
  // sub-directory pool: the live directory is ~2 entries per segment; every
  // growth leaks the old region (like the reference's directory doubling)
  t->pool_cap = std::min<uint64_t>(std::max<uint64_t>(n0 * 4, 8ULL << ceil_log2(ms)) + 4096 +
                                        ((uint64_t)kFixedSlot << t->p1max), 0xFFFFFFF0ULL);
  // every per-bucket array is sized for p1max
  const uint64_t nb = 1ULL << t->p1max;
  // k_part partitions into at most 2^kMaxPartBits buckets; finer directory
  // buckets share a partition bucket (sub-buckets)
  uint64_t nrec = 0;
  for (uint32_t q = t->p1_init; q <= t->p1max; ++q) {
    const uint32_t sq = q > kMaxPartBits ? q - kMaxPartBits : 0;
    nrec = std::max<uint64_t>(nrec, ((uint64_t)part_cap(t->max_batch, q, sq) << (q - sq)) + t->max_batch);
    if (q > kCpSbb)  // (the coarse partition of plan_batch)
      nrec = std::max<uint64_t>(nrec, ((uint64_t)part_cap(t->max_batch, q, kCpSbb) << (q - kCpSbb)) + t->max_batch);
  }
  t->nrec = nrec;
  {
    const uint32_t sq = t->p1max > kMaxPartBits ? t->p1max - kMaxPartBits : 0;
    t->cblk = cursor_block(1u << (t->p1max - sq));
  }
  hipError_t e;
  // (every allocation is recorded on the handle: destroy frees that list)
#define ALLOC(p, bytes)                                                   \
  do {                                                                    \
    e = hipMalloc(&(p), (bytes));                                         \
    if (e != hipSuccess) {                                                \
      pmdfc_cceh_destroy(t);                                              \
      return fail(PMDFC_ERR_NOMEM, "hipMalloc " #p, e);                   \
    }                                                                     \
    t->dev_allocs.push_back(p);                                           \
  } while (0)
  ALLOC(t->pairs, ms * kSlots * sizeof(ulonglong2));
  ALLOC(t->occ, ms * 32 * sizeof(uint32_t));
  ALLOC(t->ldep, ms);
  {
    // the mixed batches' key set: ONE table at load <= 1/2 even when every op
    // of a batch inserts a distinct key (at least 8192 slots).  Only the
    // joining Gets' filter (jbits) is replicated, kJoinReps times.
    uint64_t isl = 8192;
    while (isl < 2 * (uint64_t)t->max_batch) isl <<= 1;
    t->mx.imask = isl - 1;
    ALLOC(t->mx.iset, isl * sizeof(uint64_t));
    ALLOC(t->mx.ipos, isl * sizeof(uint32_t));
    ALLOC(t->mx.icnt, isl * sizeof(uint32_t));
    ALLOC(t->mx.early, t->max_batch);
    ALLOC(t->mx.islot, t->max_batch * sizeof(uint32_t));
    ALLOC(t->mx.icount, (t->max_batch / 256 + 1) * sizeof(uint32_t));
    ALLOC(t->mx.jbits, kJoinWords * sizeof(uint32_t));
    ALLOC(t->mx.elink, t->max_batch * sizeof(uint32_t));
    ALLOC(t->mx.loss0, 256);
  }
  if (t->upsert) ALLOC(t->upos, (uint64_t)t->max_batch * sizeof(uint16_t));
  ALLOC(t->hdr, nb * sizeof(uint64_t));
  ALLOC(t->pool, t->pool_cap * sizeof(uint32_t));
  ALLOC(t->ctl, sizeof(DevCtl));
  // records, their overflow tags and cursors: kRecBufs sets, so a batch's
  // partition can run while the two batches before it are applied
  ALLOC(t->rkv, kRecBufs * nrec * sizeof(ulonglong2));
  ALLOC(t->rop, kRecBufs * nrec * sizeof(uint32_t));
  ALLOC(t->robk, kRecBufs * (uint64_t)t->max_batch * sizeof(uint16_t));
  ALLOC(t->cursor, kRecBufs * t->cblk * sizeof(uint32_t));
  ALLOC(t->hdr_tmp, nb * sizeof(uint64_t));
  ALLOC(t->minld, sizeof(uint32_t));
  ALLOC(t->wstat, nb * kWStat * sizeof(uint64_t));
  ALLOC(t->wl_kv, nb * kChunkWave * sizeof(ulonglong2));
  ALLOC(t->wl_op, nb * kChunkWave * sizeof(uint32_t));
  ALLOC(t->wl_n, nb * sizeof(uint32_t));
  ALLOC(t->gflat, (sizeof(uint32_t) << kFlatMaxBits));
  ALLOC(t->gflat_bits, sizeof(uint32_t));
  ALLOC(t->req, nb * kSplitCap * sizeof(uint2));
  ALLOC(t->reqop, nb * kSplitCap * sizeof(uint32_t));
  ALLOC(t->mx.drops, (uint64_t)kDropLog * sizeof(ulonglong2));
  // bucket w requests in shard w % 8, at most kSplitCap splits
  t->gcap = (uint32_t)((nb + kGShards - 1) / kGShards) * kSplitCap;
  ALLOC(t->gsh, 2 * kGShards * kGStride * sizeof(uint64_t));
  ALLOC(t->gsplit, 2 * kGShards * (uint64_t)t->gcap * sizeof(uint4));
  ALLOC(t->act, nb * sizeof(uint32_t));
  ALLOC(t->touched, (nb + 1) * sizeof(uint32_t));
  ALLOC(t->povf, kRecBufs * (uint64_t)part_blocks(t->max_batch) * (1u << kMaxPartBits) * sizeof(uint32_t));
  ALLOC(t->need, nb * sizeof(uint32_t));
  ALLOC(t->gbase, nb * sizeof(uint32_t));
  ALLOC(t->ngrant, nb * sizeof(uint32_t));
  ALLOC(t->newoff, nb * sizeof(uint32_t));
  ALLOC(t->fin, 2 * nb * sizeof(uint32_t));
  ALLOC(t->fbl, nb * sizeof(uint32_t));
  ALLOC(t->partials, ((uint64_t)t->max_batch / 64 + 2) * sizeof(uint32_t));
  ALLOC(t->popc, sizeof(unsigned long long));
  ALLOC(t->srv_st, 64);
  ALLOC(t->srv_vout, 64 * sizeof(uint64_t));
  if (t->kn.stamps) {
    const uint64_t bytes = t->kn.stamp_rot * stamp_words(t) * sizeof(uint64_t);
    ALLOC(t->stamps, bytes);
    if ((e = hipMemset(t->stamps, 0, bytes)) != hipSuccess) {
      pmdfc_cceh_destroy(t);
      return fail(PMDFC_ERR_HIP, "hipMemset(t->stamps, 0, bytes)", e);
    }
  }
#undef ALLOC
  {
    // the partition stream at high priority: a batch's k_part is dispatched
    // ahead of the previous batch's remaining bucket waves (PMDFC_PSTREAM_PRIO=0: default priority, A/B)
    int lo = 0, hi = 0;
    if (t->kn.pstream_prio && hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess)
      e = hipStreamCreateWithPriority(&t->pstream, hipStreamNonBlocking, hi);
    else
      e = hipStreamCreateWithFlags(&t->pstream, hipStreamNonBlocking);
  }
  if (e == hipSuccess) e = hipEventCreateWithFlags(&t->ev_in, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&t->ev_minld, hipEventDisableTiming);
  for (int i = 0; i < 2 && e == hipSuccess; ++i) {
    e = hipEventCreateWithFlags(&t->ev_gpart[i], hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&t->ev_gdone[i], hipEventDisableTiming);
  }
  for (int i = 0; i < (int)kRecBufs && e == hipSuccess; ++i) {
    e = hipEventCreateWithFlags(&t->ev_part[i], hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&t->ev_done[i], hipEventDisableTiming);
  }
  if (e == hipSuccess) e = hipHostMalloc((void**)&t->h_depth, 32 * sizeof(uint32_t), hipHostMallocDefault);
  if (e != hipSuccess) {
    pmdfc_cceh_destroy(t);
    return fail(PMDFC_ERR_HIP, "stream/event create", e);
  }
  // (coherent: the device's system-scope store reaches host memory without a
  // fence of the stream)
  if (e == hipSuccess) e = hipHostMalloc((void**)&t->h_hint, 64, hipHostMallocCoherent | hipHostMallocMapped);
  if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&t->d_hint, t->h_hint, 0);
  if (e != hipSuccess) {
    pmdfc_cceh_destroy(t);
    return fail(PMDFC_ERR_HIP, "hint word", e);
  }
  memset(t->h_hint, 0, 64);
  e = hipHostMalloc(&t->hctl, sizeof(DevCtl), hipHostMallocDefault);
  if (e != hipSuccess) {
    pmdfc_cceh_destroy(t);
    return fail(PMDFC_ERR_NOMEM, "hipHostMalloc", e);
  }
  t->mx.iset_dirty = true;  // (fresh allocations: init_state empties the key set)
  int rc = init_state(t, (hipStream_t)0);
  if (rc == PMDFC_OK && hipStreamSynchronize((hipStream_t)0) != hipSuccess) rc = fail(PMDFC_ERR_HIP, "init");
  if (rc) {
    pmdfc_cceh_destroy(t);
    return rc;
  }
  *out = t;
  return PMDFC_OK;
}

int pmdfc_cceh_destroy(pmdfc_cceh_t* t) {
  if (!t) return PMDFC_OK;
  DevGuard g(t->dev);
  (void)hipDeviceSynchronize();
  t->timing.flush_closed();
  for (void* p : t->dev_allocs) (void)hipFree(p);
  if (t->hctl) (void)hipHostFree(t->hctl);
  if (t->h_depth) (void)hipHostFree(t->h_depth);
  if (t->h_hint) (void)hipHostFree(t->h_hint);
  for (hipEvent_t ev : {t->ev_in, t->ev_minld, t->ev_gpart[0], t->ev_gpart[1], t->ev_gdone[0], t->ev_gdone[1]})
    if (ev) (void)hipEventDestroy(ev);
  for (uint32_t i = 0; i < kRecBufs; ++i) {
    if (t->ev_part[i]) (void)hipEventDestroy(t->ev_part[i]);
    if (t->ev_done[i]) (void)hipEventDestroy(t->ev_done[i]);
  }
  if (t->pstream) (void)hipStreamDestroy(t->pstream);
  delete t;
  return PMDFC_OK;
}

int pmdfc_cceh_reset(pmdfc_cceh_t* t, void* stream) {
  if (!t) return fail(PMDFC_ERR_ARG, "null engine");
  std::lock_guard<std::mutex> lk(t->mu);
  DevGuard g(t->dev);
  return init_state(t, (hipStream_t)stream);
}

int pmdfc::do_get(pmdfc_cceh_t* t, const uint64_t* keys, uint64_t* vout, uint8_t* st, uint64_t n,
                  void* stream) {
  if (n == 0) return PMDFC_OK;
  std::lock_guard<std::mutex> lk(t->mu);
  DevGuard g(t->dev);
  hipStream_t s = (hipStream_t)stream;
  const bool count = t->count_lines && n <= t->max_batch;
  if (!t->flat_valid) {  // first Get after inserts: flatten the directory
    launch_flatten(t->hdr, t->pool, t->p1, t->gflat, t->gflat_bits, t->kn.flat_max, s);
    t->flat_valid = true;
  }
  t->timing.begin(PMDFC_K_GET, s);
  launch_get(count, keys, vout, st, n, t->geo_flat(), t->pairs, t->partials, s);
  t->timing.end(s);
  t->last_get_n = n;
  t->last_get_counted = count;
  {
    const int U = process_knobs().get_unroll;  // (as launch_get)
    t->last_get_blocks = ((n + U - 1) / U + 63) / 64;
  }
  HIPCHK(hipGetLastError());
  return PMDFC_OK;
}

int pmdfc_cceh_get(pmdfc_cceh_t* t, const uint64_t* keys, uint64_t* vout, uint8_t* st, uint64_t n,
                   void* stream) {
  if (!t || (n && (!keys || !vout || !st))) return fail(PMDFC_ERR_ARG, "null argument");
  return do_get(t, keys, vout, st, n, stream);
}

// Get batches [bounds[0], bounds[nb]): Get batches change nothing, so
// consecutive ones are one launch over their union -- the same results per op,
// without a kernel boundary (and its ramp and tail) between batches.
int pmdfc_cceh_get_batches(pmdfc_cceh_t* t, const uint64_t* keys, uint64_t* vout, uint8_t* st,
                           const uint64_t* bounds, uint32_t nbatches, void* stream) {
  if (!t || !bounds || (nbatches && (!keys || !vout || !st))) return fail(PMDFC_ERR_ARG, "null argument");
  if (int rc = check_bounds(bounds, nbatches, ~0ull)) return rc;  // (a Get batch may be any size)
  if (nbatches == 0) return PMDFC_OK;
#ifdef PMDFC_GETB_PER_BATCH  // (A/B builds: one launch per batch)
  for (uint32_t i = 0; i < nbatches; ++i)
    if (int rc = do_get(t, keys + bounds[i], vout + bounds[i], st + bounds[i], bounds[i + 1] - bounds[i], stream))
      return rc;
  return PMDFC_OK;
#else
  const uint64_t o = bounds[0];
  return do_get(t, keys + o, vout + o, st + o, bounds[nbatches] - o, stream);
#endif
}

int pmdfc_cceh_find_anyway(pmdfc_cceh_t* t, const uint64_t* keys, uint64_t* vout, uint8_t* st, uint64_t n,
                           void* stream) {
  if (!t || (n && (!keys || !vout || !st))) return fail(PMDFC_ERR_ARG, "null argument");
  if (n == 0) return PMDFC_OK;
  std::lock_guard<std::mutex> lk(t->mu);
  DevGuard g(t->dev);
  launch_find_anyway(keys, vout, st, n, t->geo(), t->pairs, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return PMDFC_OK;
}

// Erase x n (erase.hip): probe, stable sort by segment, run
// heads, one wave per run.  Only the first call waits (it allocates the scratch).
int pmdfc_cceh_erase(pmdfc_cceh_t* t, const uint64_t* keys, uint8_t* st, uint64_t n, void* stream) {
  if (!t || (n && (!keys || !st))) return fail(PMDFC_ERR_ARG, "null argument");
  if (n > t->max_batch) return fail(PMDFC_ERR_ARG, "n > max_batch");
  if (n == 0) return PMDFC_OK;
  std::lock_guard<std::mutex> lk(t->mu);
  DevGuard g(t->dev);
  hipStream_t s = (hipStream_t)stream;
  pmdfc_cceh::Erase& er = t->er;
  if (!er.rows) {
    er.sort_bits = ceil_log2(t->max_segs) + 1;
    HIPCHK(erase_sort_temp_bytes(t->max_batch, er.sort_bits, &er.tmp_bytes));
    void *rows = nullptr, *tmp = nullptr;
    HIPCHK(hipMalloc(&rows, (5ull * t->max_batch + 1) * sizeof(uint32_t)));
    t->dev_allocs.push_back(rows);
    HIPCHK(hipMalloc(&tmp, std::max<size_t>(er.tmp_bytes, 16)));
    t->dev_allocs.push_back(tmp);
    er.cursor = static_cast<uint32_t*>(rows) + 5ull * t->max_batch;
    er.tmp = tmp;
    er.rows = static_cast<uint32_t*>(rows);
  }
  if (!t->flat_valid) {  // (as do_get)
    launch_flatten(t->hdr, t->pool, t->p1, t->gflat, t->gflat_bits, t->kn.flat_max, s);
    t->flat_valid = true;
  }
  EraseArgs a{};
  a.keys = keys;
  a.st = st;
  a.n = n;
  a.g = t->geo_flat();
  a.pairs = t->pairs;
  a.occ = t->occ;
  a.ctl = t->ctl;
  a.max_segs = (uint32_t)t->max_segs;
  const uint64_t mb = t->max_batch;
  a.seg_in = er.rows;
  a.seg_out = er.rows + mb;
  a.idx_in = er.rows + 2 * mb;
  a.idx_out = er.rows + 3 * mb;
  a.work = er.rows + 4 * mb;
  a.cursor = er.cursor;
  a.tmp = er.tmp;
  a.tmp_bytes = er.tmp_bytes;
  a.sort_bits = er.sort_bits;
  HIPCHK(launch_erase(a, s));
  return PMDFC_OK;
}

// EraseMatching (match.hip): one launch, then the four result
// words come back.  Synchronous.
int pmdfc_cceh_erase_matching(pmdfc_cceh_t* t, uint64_t mask, const uint64_t* d_patterns, uint32_t n,
                              pmdfc_erase_matching_result_t* out, void* stream) {
  if (!t || (n && !d_patterns)) return fail(PMDFC_ERR_ARG, "null argument");
  if (n > PMDFC_MATCH_MAX) return fail(PMDFC_ERR_ARG, "n > PMDFC_MATCH_MAX");
  if (out) *out = pmdfc_erase_matching_result_t{};
  if (n == 0) return PMDFC_OK;
  std::lock_guard<std::mutex> lk(t->mu);
  DevGuard g(t->dev);
  hipStream_t s = (hipStream_t)stream;
  if (!t->match_out) {
    void* w = nullptr;
    HIPCHK(hipMalloc(&w, 4 * sizeof(unsigned long long)));
    t->dev_allocs.push_back(w);
    t->match_out = static_cast<unsigned long long*>(w);
  }
  HIPCHK(hipMemsetAsync(t->match_out, 0, 4 * sizeof(unsigned long long), s));
  MatchArgs a{};
  a.mask = mask;
  a.patterns = d_patterns;
  a.n = n;
  a.pairs = t->pairs;
  a.occ = t->occ;
  a.ctl = t->ctl;
  a.max_segs = (uint32_t)t->max_segs;
  a.out = t->match_out;
  launch_erase_matching(a, s);
  HIPCHK(hipGetLastError());
  unsigned long long h[4] = {0, 0, 0, 0};
  HIPCHK(hipMemcpyAsync(h, t->match_out, sizeof(h), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (out) {
    out->removed = h[0];
    out->segments_changed = (uint32_t)h[1];
    out->segments_cleared = (uint32_t)h[2];
    out->segments_scanned = (uint32_t)h[3];
  }
  return PMDFC_OK;
}

int pmdfc_cceh_get_records(pmdfc_cceh_t* t, const uint64_t* keys, uint64_t* resp, uint64_t n, void* stream) {
  if (!t || (n && (!keys || !resp))) return fail(PMDFC_ERR_ARG, "null argument");
  return do_get(t, keys, resp, nullptr, n, stream);
}

// A batch of at most kChunkWave ops takes one launch (k_mixed_small) instead
// of the ~12 of the general pipeline; its results are the serial reference's
// exactly.  PMDFC_SMALL_MAX lowers the cut (0: never; A/B and tests).
static uint64_t small_max() { return process_knobs().small_max; }

static int small_one(pmdfc_cceh_t* t, const uint8_t* ops, const uint64_t* keys, const uint64_t* vin,
                     uint64_t* vout, uint8_t* st, uint64_t n, hipStream_t s) {
  int rc = rebucket_now(t, s);  // (a table coarser than p1max: one sync, as the general path)
  if (rc) return rc;
  const BatchPlan b = plan_batch(t, false, n, false);  // (no records)
  BucketArgs A{};
  fill_bucket_args(t, b, A, n, st, vout, true);
  t->timing.begin(PMDFC_K_PROCESS, s);
  launch_mixed_small(A, ops, keys, vin, s);
  t->timing.end(s);
  finish_batch(t, b, kPathSmall);
  HIPCHK(hipGetLastError());
  return PMDFC_OK;
}

// A batch of at most kPartTile ops at full bucket resolution takes two
// launches: its one-block partition (k_part, statuses initialized there, the
// touched buckets listed) and k_medium, the final pass over every touched
// bucket with its records in batch order.  Exact serial results (no early
// answers).  PMDFC_MEDIUM_MAX lowers the cut (0: never).
static uint64_t medium_max() { return process_knobs().medium_max; }

static int medium_one(pmdfc_cceh_t* t, const uint8_t* ops, const uint64_t* keys, const uint64_t* vin, uint32_t kvs,
                      uint64_t* vout, uint8_t* st, uint64_t n, hipStream_t s) {
  const BatchPlan b = plan_batch(t, false, n);
  if (int rc = zero_stale_cursors(t, b, s)) return rc;
  PartArgs P{};
  fill_part_launch(t, b, P, ops, keys, vin, kvs, st, n);
  P.init = ops ? 1u : 0u;
  P.vout = vout;
  P.touched = t->touched;
  BucketArgs A{};
  fill_bucket_args(t, b, A, n, st, vout, ops != nullptr);
  t->timing.begin(PMDFC_K_PROCESS, s);
  launch_part(P, s);
  launch_medium(A, t->touched, s);
  t->timing.end(s);
  finish_batch(t, b, kPathMedium);
  HIPCHK(hipGetLastError());
  return PMDFC_OK;
}

static int insert_one(pmdfc_cceh_t* t, const uint64_t* keys, const uint64_t* vin, uint32_t kvs, uint8_t* st,
                      uint64_t n, hipStream_t s) {
  const BatchPlan b = plan_batch(t, true, n);
  if (int rc = zero_stale_cursors(t, b, s)) return rc;
  PartArgs P{};
  fill_part_launch(t, b, P, nullptr, keys, vin, kvs, st, n);
  BucketLaunch B{};
  fill_bucket_launch(t, b, B, n, st, nullptr, false);
  t->timing.begin(PMDFC_K_ROUTE, s);
  if (B.plan.probe) launch_upsert_probe(keys, kvs, nullptr, n, t->geo(), t->pairs, t->upos, s);
  launch_part(P, s);
  run_bucket_passes(t, B, s);
  t->timing.end(s);
  finish_batch(t, b, kPathGeneral);
  HIPCHK(hipGetLastError());
  return PMDFC_OK;
}

// one insert batch, as sub-batches while the table is coarser than p1max
static int insert_ramped(pmdfc_cceh_t* t, const uint64_t* keys, const uint64_t* vin, uint32_t kvs, uint8_t* st,
                         uint64_t n, hipStream_t s) {
  for (uint64_t o = 0; o < n;) {
    int rc = rebucket_now(t, s);
    if (rc) return rc;
    const uint64_t m = ramp_batch(t, n - o);
    rc = insert_one(t, keys + o * kvs, vin + o * kvs, kvs, st + o, m, s);
    if (rc) return rc;
    o += m;
  }
  t->batches += 1;
  return PMDFC_OK;
}

int pmdfc::do_insert(pmdfc_cceh_t* t, const uint64_t* keys, const uint64_t* vin, uint32_t kvs, uint8_t* st,
                     uint64_t n, void* stream) {
  if (n == 0) return PMDFC_OK;
  if (n > t->max_batch) return fail(PMDFC_ERR_ARG, "n exceeds max_batch");
  std::lock_guard<std::mutex> lk(t->mu);
  DevGuard g(t->dev);
  if (kvs == 1 && n <= small_max()) return small_one(t, nullptr, keys, vin, nullptr, st, n, (hipStream_t)stream);
  if (n <= medium_max() && t->p1 >= t->p1max)
    return medium_one(t, nullptr, keys, vin, kvs, nullptr, st, n, (hipStream_t)stream);
  return insert_ramped(t, keys, vin, kvs, st, n, (hipStream_t)stream);
}

int pmdfc_cceh_insert(pmdfc_cceh_t* t, const uint64_t* keys, const uint64_t* vin, uint8_t* st,
                      uint64_t n, void* stream) {
  if (!t || (n && (!keys || !vin || !st))) return fail(PMDFC_ERR_ARG, "null argument");
  return do_insert(t, keys, vin, 1, st, n, stream);
}

int pmdfc_cceh_insert_records(pmdfc_cceh_t* t, const uint64_t* records, uint8_t* st, uint64_t n,
                              void* stream) {
  if (!t || (n && (!records || !st))) return fail(PMDFC_ERR_ARG, "null argument");
  return do_insert(t, records, records + 1, 2, st, n, stream);
}

// Pipelined insert batches (t->mu held, table at p1max): batch k of a run
// partitions on the partition stream while the bucket passes of batch k - 1
// (or k - 2) run on the caller's stream.  pipe_begin: the partition stream
// starts after everything already on s; pipe_batch: one batch (input_ready,
// if given: an event the partition waits for first -- the routed loop's
// received rows); pipe_end: the next buffer's cursors zeroed for the
// one-batch entry points.
int pmdfc::pipe_begin(pmdfc_cceh_t* t, hipStream_t s) {
  HIPCHK(hipEventRecord(t->ev_in, s));
  HIPCHK(hipStreamWaitEvent(t->pstream, t->ev_in, 0));
  return PMDFC_OK;
}

int pmdfc::pipe_batch(pmdfc_cceh_t* t, const uint64_t* keys, const uint64_t* vin, uint32_t kvs, uint8_t* st,
                      uint64_t n, hipStream_t s, uint32_t k, hipEvent_t input_ready,
                      hipEvent_t output_free) {
  hipStream_t P = t->pstream;
  const BatchPlan b = plan_batch(t, true, n);
  const uint32_t p = b.rb;
  // record buffer p's records and cursors were last read by the batch
  // kRecBufs back: with three buffers the partition of batch k + 1 may start
  // as soon as batch k - 2 is applied, so it runs under the bucket passes of
  // batch k - 1 or k instead of waiting for their end
  if (k >= kRecBufs) HIPCHK(hipStreamWaitEvent(P, t->ev_done[p], 0));
  if (input_ready) HIPCHK(hipStreamWaitEvent(P, input_ready, 0));
  if (output_free) HIPCHK(hipStreamWaitEvent(P, output_free, 0));  // (the partition writes the statuses)
  HIPCHK(hipMemsetAsync(t->cursor + p * t->cblk, 0, t->cblk * sizeof(uint32_t), P));
  PartArgs PL{};
  fill_part_launch(t, b, PL, nullptr, keys, vin, kvs, st, n);
  BucketLaunch B{};
  fill_bucket_launch(t, b, B, n, st, nullptr, false);
  B.a.clear_next = 0;  // the next batch's cursors may already be in use
  hipEvent_t e0 = t->timing.span_begin(P);
  if (B.plan.probe) {  // the probe reads the table: after the previous batch (ev_done)
    if (k >= 1) HIPCHK(hipStreamWaitEvent(P, t->ev_done[(p + kRecBufs - 1) % kRecBufs], 0));
    launch_upsert_probe(keys, kvs, nullptr, n, t->geo(), t->pairs, t->upos, P);
  }
  launch_part(PL, P);
  t->timing.span_end(PMDFC_K_ROUTE, e0, P);
  HIPCHK(hipEventRecord(t->ev_part[p], P));
  HIPCHK(hipStreamWaitEvent(s, t->ev_part[p], 0));
  run_bucket_passes(t, B, s);
  t->timing.end(s);
  HIPCHK(hipEventRecord(t->ev_done[p], s));
  finish_batch(t, b, kPathPiped);
  return PMDFC_OK;
}

// Groups of G consecutive batches (pmdfc_cceh_insert_batches): the group's
// partitions on the partition stream, then its bucket passes on s behind ONE
// event -- instead of an event record and a cross-stream wait per batch,
// each a packet the engine stream stops at between the passes of consecutive
// batches.  Group g's records reuse group g - 2's buffers (kRecBufs = 2 G_max),
// so its partitions wait for that group's passes only; they run under group
// g - 1's passes.  Each batch keeps the geometry its partition chose.
// (PMDFC_PIPE_GROUP: G; 1 = an event pair per batch)
static int pipe_group(pmdfc_cceh_t* t, const uint64_t* keys, const uint64_t* vin, uint8_t* st,
                      const uint64_t* bounds, const uint32_t* idx, uint32_t m, hipStream_t s, uint32_t gi) {
  hipStream_t P = t->pstream;
  BatchPlan plans[kRecBufs / 2 > 0 ? kRecBufs / 2 : 1];
  if (gi >= 2) HIPCHK(hipStreamWaitEvent(P, t->ev_gdone[gi & 1u], 0));
  hipEvent_t e0 = t->timing.span_begin(P);
  for (uint32_t j = 0; j < m; ++j) {
    const uint64_t o = bounds[idx[j]], n = bounds[idx[j] + 1] - o;
    const BatchPlan& b = plans[j] = plan_batch(t, true, n);
    HIPCHK(hipMemsetAsync(t->cursor + b.rb * t->cblk, 0, t->cblk * sizeof(uint32_t), P));
    PartArgs PL{};
    fill_part_launch(t, b, PL, nullptr, keys + o, vin + o, 1, st + o, n);
    launch_part(PL, P);
    finish_batch(t, b, kPathPiped);  // (the handle moves on; the passes below are filled from the plan alone)
  }
  t->timing.span_end(PMDFC_K_ROUTE, e0, P);
  HIPCHK(hipEventRecord(t->ev_gpart[gi & 1u], P));
  HIPCHK(hipStreamWaitEvent(s, t->ev_gpart[gi & 1u], 0));
  for (uint32_t j = 0; j < m; ++j) {
    const uint64_t o = bounds[idx[j]], n = bounds[idx[j] + 1] - o;
    BucketLaunch B{};
    fill_bucket_launch(t, plans[j], B, n, st + o, nullptr, false);
    B.a.clear_next = 0;  // the next batch's cursors may already be in use
    run_bucket_passes(t, B, s);  // (no probe in B.plan: pmdfc_cceh_insert_batches sends those batches one by one)
    t->timing.end(s);
  }
  HIPCHK(hipEventRecord(t->ev_gdone[gi & 1u], s));
  HIPCHK(hipGetLastError());
  return PMDFC_OK;
}

int pmdfc::pipe_end(pmdfc_cceh_t* t, hipStream_t s) {
  HIPCHK(hipMemsetAsync(t->cursor + t->rb * t->cblk, 0, t->cblk * sizeof(uint32_t), s));
  t->clean_sbb = ~0u;
  HIPCHK(hipGetLastError());
  return PMDFC_OK;
}

int pmdfc_cceh_insert_batches(pmdfc_cceh_t* t, const uint64_t* keys, const uint64_t* vin, uint8_t* st,
                              const uint64_t* bounds, uint32_t nbatches, void* stream) {
  if (!t || !bounds || (nbatches && (!keys || !vin || !st))) return fail(PMDFC_ERR_ARG, "null argument");
  if (int rc = check_bounds(bounds, nbatches, t->max_batch)) return rc;
  if (nbatches == 0) return PMDFC_OK;
  std::lock_guard<std::mutex> lk(t->mu);
  DevGuard g(t->dev);
  hipStream_t s = (hipStream_t)stream;
  // a table still coarser than p1max: its first batches one by one, ramped
  uint32_t i0 = 0;
  for (; i0 < nbatches && t->p1 < t->p1max; ++i0) {
    const int rc = insert_ramped(t, keys + bounds[i0], vin + bounds[i0], 1, st + bounds[i0],
                                 bounds[i0 + 1] - bounds[i0], s);
    if (rc) return rc;
  }
  // the partition stream starts after everything already on the caller's
  // stream (the inputs, and every earlier batch)
  int rc = pipe_begin(t, s);
  if (plan_launches(plan_in(t, false)).probe) {  // (the upsert probe reads the table: batch by batch)
    uint32_t k = 0;
    for (uint32_t i = i0; i < nbatches && rc == PMDFC_OK; ++i) {
      const uint64_t o = bounds[i], n = bounds[i + 1] - bounds[i];
      if (n == 0) continue;
      rc = pipe_batch(t, keys + o, vin + o, 1, st + o, n, s, k++, nullptr);
    }
    return rc ? rc : pipe_end(t, s);
  }
  const uint32_t G = process_knobs().pipe_group;
  uint32_t idx[kRecBufs / 2 > 0 ? kRecBufs / 2 : 1], m = 0, gi = 0;
  for (uint32_t i = i0; i <= nbatches && rc == PMDFC_OK; ++i) {
    if (i < nbatches && bounds[i + 1] > bounds[i]) idx[m++] = i;
    if (m == G || (i == nbatches && m)) {
      rc = pipe_group(t, keys, vin, st, bounds, idx, m, s, gi++);
      m = 0;
    }
  }
  return rc ? rc : pipe_end(t, s);
}

// A mixed batch tells its Gets whether the batch inserts their key through
// the JOIN (the Gets that need it claim their keys, the inserts look them up)
// when the last mixed batch inserted more than 1/8 of its ops, else through
// the INSERT set (every insert claims its key): ~500k random CASes fewer per
// half-insert config-4 batch, while a config-3 batch (5 % inserts) keeps the
// cheaper insert set (cceh_kernels.hip).  The count is a hint the device
// leaves in pinned memory, read without a sync: either mode is exact.
// PMDFC_MIXED_JOIN=0 / 1 forces one (A/B, tests).
static bool mixed_join_mode(const pmdfc_cceh* t) {
  const int force = process_knobs().mixed_join;
  if (force >= 0) return force != 0;
  const uint64_t last = __atomic_load_n(t->h_hint + kHintMixIns, __ATOMIC_RELAXED);
  return t->mx.last_n && last * 8 > t->mx.last_n;
}

// One general mixed batch: plan, fill, the two pre-pass launches in the chosen
// mode's order, partition, bucket passes, verify.
static int mixed_one(pmdfc_cceh_t* t, const uint8_t* ops, const uint64_t* keys, const uint64_t* vin,
                     uint64_t* vout, uint8_t* st, uint64_t n, hipStream_t s) {
  const uint32_t tag = (uint32_t)++t->seq;
  if (int rc = open_key_set(t, s)) return rc;
  const BatchPlan b = plan_batch(t, false, n);
  if (int rc = zero_stale_cursors(t, b, s)) return rc;
  MixedArgs M{};
  fill_mixed_launch(t, M, ops, keys, vin, vout, st, n, tag, mixed_join_mode(t));
  if (M.join) {
    // statuses + early answers + the joining Gets (k_mixed_get), then the
    // inserts' side of the join (k_mixed_join, timed as the pre-pass class);
    // k_part resolves the joining Gets
    t->timing.begin(PMDFC_K_MIXED_GET, s);
    launch_mixed_get(M, s);
    t->timing.begin(PMDFC_K_PREP, s);
    launch_mixed_join(M, s);
  } else {
    t->timing.begin(PMDFC_K_PREP, s);
    launch_mixed_prep(M, s);
    t->timing.begin(PMDFC_K_MIXED_GET, s);
    launch_mixed_get_iset(M, s);
  }
  t->mx.last_n = n;
  PartArgs P{};
  fill_part_launch(t, b, P, ops, keys, vin, 1, st, n);
  fill_part_join(P, M);
  P.vout = vout;
  // when k_mixed_get answered every Get, the insert-only apply passes run
  // (gated by tag; upsert batches always take the mixed ones).  The mixed
  // first pass on a small grid unless a mixed batch of the last 64 ran it (the
  // word may lag the batches in flight: either grid is exact) or PMDFC_MIXED_SMALL=0
  const uint32_t last = __atomic_load_n(t->h_hint + kHintMixed, __ATOMIC_RELAXED);
  const bool mixed_small = !M.ups && !(last != 0 && tag - last < 64u) && process_knobs().mixed_small;
  BucketLaunch B{};
  fill_bucket_launch(t, b, B, n, st, vout, true, tag, mixed_small);
  B.a.mseen = t->d_hint + kHintMixed;
  B.a.drops = M.drops;  // splits log what they drop, for k_mixed_verify
  t->timing.begin(PMDFC_K_ROUTE, s);
  if (B.plan.probe) launch_upsert_probe(keys, 1, ops, n, M.g, M.pairs, t->upos, s);
  launch_part(P, s);
  run_bucket_passes(t, B, s);
  launch_mixed_verify(M, s);
  t->timing.end(s);
  finish_batch(t, b, kPathGeneral);
  HIPCHK(hipGetLastError());
  t->mx.iset_dirty = false;  // (the verify pass that empties the set is enqueued)
  return PMDFC_OK;
}

int pmdfc_cceh_mixed(pmdfc_cceh_t* t, const uint8_t* ops, const uint64_t* keys, const uint64_t* vin,
                     uint64_t* vout, uint8_t* st, uint64_t n, void* stream) {
  if (!t || (n && (!ops || !keys || !vin || !vout || !st))) return fail(PMDFC_ERR_ARG, "null argument");
  if (n == 0) return PMDFC_OK;
  if (n > t->max_batch) return fail(PMDFC_ERR_ARG, "n exceeds max_batch");
  std::lock_guard<std::mutex> lk(t->mu);
  DevGuard g(t->dev);
  hipStream_t s = (hipStream_t)stream;
  if (n <= small_max()) return small_one(t, ops, keys, vin, vout, st, n, s);
  if (n <= medium_max() && t->p1 >= t->p1max) return medium_one(t, ops, keys, vin, 1, vout, st, n, s);
  for (uint64_t o = 0; o < n;) {  // sub-batches while the table is coarser than p1max
    int rc = rebucket_now(t, s);
    if (rc) return rc;
    const uint64_t m = ramp_batch(t, n - o);
    rc = mixed_one(t, ops + o, keys + o, vin + o, vout + o, st + o, m, s);
    if (rc) return rc;
    o += m;
  }
  t->batches += 1;
  return PMDFC_OK;
}

// Batch after batch through the one-batch path.  (Running batch i + 1's
// pre-pass beside batch i -- double-buffered key sets, the pre-pass on a
// stream of its own -- measured slower: DESIGN.md, round 5.)
int pmdfc_cceh_mixed_batches(pmdfc_cceh_t* t, const uint8_t* ops, const uint64_t* keys, const uint64_t* vin,
                             uint64_t* vout, uint8_t* st, const uint64_t* bounds, uint32_t nbatches, void* stream) {
  if (!t || !bounds || (nbatches && (!ops || !keys || !vin || !vout || !st)))
    return fail(PMDFC_ERR_ARG, "null argument");
  if (int rc = check_bounds(bounds, nbatches, t->max_batch)) return rc;
  for (uint32_t i = 0; i < nbatches; ++i) {
    const uint64_t o = bounds[i], n = bounds[i + 1] - bounds[i];
    if (n == 0) continue;
    if (int rc = pmdfc_cceh_mixed(t, ops + o, keys + o, vin + o, vout + o, st + o, n, stream)) return rc;
  }
  return PMDFC_OK;
}

static int serve_start(pmdfc_cceh_t* t, uint32_t nwaves, pmdfc_serve_req* req, pmdfc_serve_resp* resp,
                       pmdfc_serve_ctl* ctl, uint64_t ring_size, uint64_t head0, pmdfc_cbf_t* cbf, void* stream) {
  if (!t || !req || !resp || !ctl || ring_size < 64 || ring_size > (1ull << 25) ||
      (ring_size & (ring_size - 1)))
    return fail(PMDFC_ERR_ARG, "serve_start: rings and a power-of-two ring_size in [64, 2^25]");
  if (cbf && cbf->dev != t->dev) return fail(PMDFC_ERR_ARG, "serve_start: counting BF on another device");
  std::lock_guard<std::mutex> lk(t->mu);
  DevGuard g(t->dev);
  hipStream_t s = (hipStream_t)stream;
  int rc = rebucket_now(t, s);  // (the wave keeps the bucket geometry it starts with)
  if (rc) return rc;
  void *dq = nullptr, *dr = nullptr, *dc = nullptr;
  HIPCHK(hipHostGetDevicePointer(&dq, req, 0));
  HIPCHK(hipHostGetDevicePointer(&dr, resp, 0));
  HIPCHK(hipHostGetDevicePointer(&dc, ctl, 0));
  const BatchPlan b = plan_batch(t, false, 64, false);  // (no records)
  ServeArgs V{};
  fill_bucket_args(t, b, V.a, 64, t->srv_st, t->srv_vout, true);
  V.req = (const pmdfc_serve_req*)dq;
  V.resp = (pmdfc_serve_resp*)dr;
  V.ctl = (pmdfc_serve_ctl*)dc;
  V.ring_size = ring_size;
  V.head0 = head0;
  V.cbf = cbf ? cbf->cnt : nullptr;
  V.cbf_m = cbf ? cbf->nbits : 0;
  V.cbf_k = cbf ? cbf->k : 0;
  V.nwaves = nwaves ? nwaves : 1u;
  launch_serve(V, s);
  HIPCHK(hipGetLastError());
  finish_batch(t, b, kPathServe);
  return PMDFC_OK;
}

int pmdfc_cceh_serve_start(pmdfc_cceh_t* t, pmdfc_serve_req* req, pmdfc_serve_resp* resp, pmdfc_serve_ctl* ctl,
                           uint64_t ring_size, uint64_t head0, pmdfc_cbf_t* cbf, void* stream) {
  return serve_start(t, 1, req, resp, ctl, ring_size, head0, cbf, stream);
}

uint32_t pmdfc_cceh_serve_waves_max(pmdfc_cceh_t* t) {
  if (!t) return 0;
  std::lock_guard<std::mutex> lk(t->mu);
  return std::min<uint32_t>(1u << t->p1, kServeWavesMax);
}

int pmdfc_cceh_serve_start_n(pmdfc_cceh_t* t, uint32_t nwaves, pmdfc_serve_req* req, pmdfc_serve_resp* resp,
                             pmdfc_serve_ctl* ctl, uint64_t ring_size, pmdfc_cbf_t* cbf, void* stream) {
  if (!t || nwaves == 0 || (nwaves & (nwaves - 1)) || nwaves > kServeWavesMax)
    return fail(PMDFC_ERR_ARG, "serve_start_n: nwaves must be a power of two <= 64");
  {
    std::lock_guard<std::mutex> lk(t->mu);
    if (nwaves > (1u << t->p1)) return fail(PMDFC_ERR_ARG, "serve_start_n: more waves than directory buckets");
  }
  return serve_start(t, nwaves, req, resp, ctl, ring_size, 0, cbf, stream);
}

int pmdfc_cceh_mixed_host(pmdfc_cceh_t* t, const uint8_t* ops, const uint64_t* keys,
                          const uint64_t* vin, uint64_t* vout, uint8_t* st, uint64_t n) {
  if (!t) return fail(PMDFC_ERR_ARG, "null engine");
  DevGuard g(t->dev);
  for (uint64_t off = 0; off < n; off += t->max_batch) {
    const uint64_t m = std::min<uint64_t>(t->max_batch, n - off);
    DevTmp d_ops, d_st, d_keys, d_vin, d_vout;  // (freed at the end of the chunk, on every path)
    HIPCHK(hipMalloc(&d_ops.p, m));
    HIPCHK(hipMalloc(&d_st.p, m));
    HIPCHK(hipMalloc(&d_keys.p, m * 8));
    HIPCHK(hipMalloc(&d_vin.p, m * 8));
    HIPCHK(hipMalloc(&d_vout.p, m * 8));
    HIPCHK(hipMemcpy(d_ops.p, ops + off, m, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_keys.p, keys + off, m * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_vin.p, vin + off, m * 8, hipMemcpyHostToDevice));
    if (int rc = pmdfc_cceh_mixed(t, (const uint8_t*)d_ops.p, (const uint64_t*)d_keys.p, (const uint64_t*)d_vin.p,
                                  (uint64_t*)d_vout.p, (uint8_t*)d_st.p, m, nullptr))
      return rc;
    HIPCHK(hipMemcpy(vout + off, d_vout.p, m * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(st + off, d_st.p, m, hipMemcpyDeviceToHost));
  }
  return PMDFC_OK;
}

int pmdfc_cceh_stats(pmdfc_cceh_t* t, pmdfc_cceh_stats_t* out) {
  if (!t || !out) return fail(PMDFC_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> lk(t->mu);
  DevGuard g(t->dev);
  HIPCHK(hipDeviceSynchronize());
  int rc = read_ctl(t, (hipStream_t)0);
  if (rc) return rc;
  const DevCtl& c = *t->hctl;
  std::vector<uint64_t> ws;
  uint32_t max_rounds = 0, max_ld = 0;
  if ((rc = read_wstat(t, ws, max_ld))) return rc;
  uint64_t sum[kWStat] = {0};
  for (size_t i = 0; i < ws.size(); ++i) {
    const int k = (int)(i % kWStat);
    if (k == 6) {
      max_rounds = std::max<uint32_t>(max_rounds, (uint32_t)(ws[i] & 0xFFFF));
      sum[6] += ws[i] >> 32;
    } else {
      sum[k] += ws[i];
    }
  }
  std::vector<uint64_t> hd(1ULL << t->p1);
  HIPCHK(hipMemcpy(hd.data(), t->hdr, hd.size() * 8, hipMemcpyDeviceToHost));
  uint32_t maxdb = 0;
  for (auto v : hd) maxdb = std::max(maxdb, hdr_db(v));
  // the segments in the directory: ids handed out, less the overshoot of a
  // full arena and the ids retired empty when the pool denied their split
  const uint64_t nsegs = std::min<uint64_t>(c.nsegs, t->max_segs) - c.dead;
  out->depth = std::max(t->D0, max_ld);
  out->phys_depth = t->sbits + t->p1 + maxdb;
  out->segments = nsegs;
  out->capacity = nsegs * kSlots;
  out->max_segments = t->max_segs;
  out->splits = sum[2];
  out->doublings = sum[6];
  out->split_loss = sum[3] + c.split_loss;
  out->insert_passes = sum[5];
  out->batches = t->batches;
  out->segment_runs = sum[4];
  out->deferred_ops = sum[1];
  out->bucket_bits = t->p1;
  out->max_rounds = max_rounds;
  out->insert_lines = sum[0];
  out->error_flags = c.err;
  {
    std::vector<uint32_t> fb(1ULL << t->p1max);
    HIPCHK(hipMemcpy(fb.data(), t->fbl, fb.size() * 4, hipMemcpyDeviceToHost));
    uint64_t nd = 0;
    for (auto v : fb) nd += v >> 1;
    out->fast_declined = (uint32_t)std::min<uint64_t>(nd, 0xFFFFFFFFu);
  }
  return PMDFC_OK;
}

int pmdfc_cceh_utilization(pmdfc_cceh_t* t, double* out) {
  if (!t || !out) return fail(PMDFC_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> lk(t->mu);
  DevGuard g(t->dev);
  HIPCHK(hipDeviceSynchronize());
  int rc = read_ctl(t, (hipStream_t)0);
  if (rc) return rc;
  const uint64_t nsegs = std::min<uint64_t>(t->hctl->nsegs, t->max_segs);  // (retired ids are empty)
  HIPCHK(hipMemset(t->popc, 0, sizeof(unsigned long long)));
  launch_popcount(t->occ, nsegs * 32, t->popc, (hipStream_t)0);
  unsigned long long c = 0;
  HIPCHK(hipMemcpy(&c, t->popc, sizeof c, hipMemcpyDeviceToHost));
  *out = (double)c / ((double)(nsegs - t->hctl->dead) * kSlots) * 100.0;
  return PMDFC_OK;
}

int pmdfc_cceh_dump(pmdfc_cceh_t* t, uint32_t* dir_canon, uint32_t* local_depth, uint64_t* prefix,
                    uint64_t* keys, uint64_t* values, uint64_t* nseg_out) {
  if (!t) return fail(PMDFC_ERR_ARG, "null engine");
  std::lock_guard<std::mutex> lk(t->mu);
  DevGuard g(t->dev);
  HIPCHK(hipDeviceSynchronize());
  int rc = read_ctl(t, (hipStream_t)0);
  if (rc) return rc;
  std::vector<uint64_t> ws;
  uint32_t max_ld = 0;
  if ((rc = read_wstat(t, ws, max_ld))) return rc;
  const uint32_t D = std::max(t->D0, max_ld);  // logical global depth
  const uint32_t Dl = D - t->sbits;
  const uint64_t nlog = 1ULL << Dl;
  std::vector<uint64_t> hd(1ULL << t->p1);
  HIPCHK(hipMemcpy(hd.data(), t->hdr, hd.size() * 8, hipMemcpyDeviceToHost));
  std::vector<uint32_t> pl(std::min<uint64_t>(t->hctl->pool_cur, t->pool_cap));
  HIPCHK(hipMemcpy(pl.data(), t->pool, pl.size() * 4, hipMemcpyDeviceToHost));
  const uint32_t nsub = Dl - t->p1;  // logical index bits below the bucket
  std::vector<uint32_t> order;
  uint32_t cur = 0;
  for (uint64_t x = 0; x < nlog; ++x) {
    const uint64_t hb = hd[x >> nsub];
    const uint32_t db = hdr_db(hb);
    const uint64_t sub = (x & ((1ULL << nsub) - 1)) >> (nsub - db);
    const uint32_t e = pl[hdr_off(hb) + sub];
    const uint32_t sid = de_seg(e);
    const uint32_t L = de_ld(e);
    const uint32_t Ll = L - t->sbits;
    if ((x & ((1ULL << (Dl - Ll)) - 1)) == 0) {
      cur = (uint32_t)order.size();
      order.push_back(sid);
      if (local_depth) local_depth[cur] = L;
      if (prefix) prefix[cur] = ((uint64_t)t->shard << Ll) | (x >> (Dl - Ll));
    }
    if (dir_canon) dir_canon[x] = cur;
  }
  if (nseg_out) *nseg_out = order.size();
  if (keys || values) {
    std::vector<ulonglong2> buf(kSlots);
    for (size_t i = 0; i < order.size(); ++i) {
      HIPCHK(hipMemcpy(buf.data(), t->pairs + (size_t)order[i] * kSlots, kSlots * 16,
                       hipMemcpyDeviceToHost));
      for (uint32_t j = 0; j < kSlots; ++j) {
        if (keys) keys[i * kSlots + j] = buf[j].x;
        if (values) values[i * kSlots + j] = buf[j].x == kInvalid ? 0 : buf[j].y;
      }
    }
  }
  return PMDFC_OK;
}

int pmdfc_cceh_timing_enable(pmdfc_cceh_t* t, int on) {
  if (!t) return fail(PMDFC_ERR_ARG, "null engine");
  std::lock_guard<std::mutex> lk(t->mu);
  t->timing.on = (on & 1) != 0;
  t->count_lines = (on & 2) != 0;
  return PMDFC_OK;
}

int pmdfc_cceh_timing_read(pmdfc_cceh_t* t, double* ms_out, uint64_t* launches_out, int reset) {
  if (!t) return fail(PMDFC_ERR_ARG, "null engine");
  std::lock_guard<std::mutex> lk(t->mu);
  DevGuard g(t->dev);
  t->timing.flush_closed();
  for (int i = 0; i < PMDFC_K_COUNT; ++i) {
    if (ms_out) ms_out[i] = t->timing.ms[i];
    if (launches_out) launches_out[i] = t->timing.launches[i];
    if (reset) {
      t->timing.ms[i] = 0;
      t->timing.launches[i] = 0;
    }
  }
  return PMDFC_OK;
}

int pmdfc_cceh_debug_stamps(pmdfc_cceh_t* t, uint64_t* out, uint64_t n, uint32_t* nbuckets) {
  if (!t || !out) return fail(PMDFC_ERR_ARG, "null argument");
  if (!t->stamps) return fail(PMDFC_ERR_STATE, "stamps are off (create with PMDFC_STAMPS=1)");
  std::lock_guard<std::mutex> lk(t->mu);
  DevGuard g(t->dev);
  HIPCHK(hipDeviceSynchronize());
  // the last batch's set, or every set when n holds them all (PMDFC_STAMP_ROT)
  const uint64_t tot = stamp_words(t), all = tot * t->kn.stamp_rot;
  const bool every = t->kn.stamp_rot > 1 && n >= all;
  const uint64_t* src = every || !t->stamp_last ? t->stamps : t->stamp_last;
  HIPCHK(hipMemcpy(out, src, std::min(n, every ? all : tot) * 8, hipMemcpyDeviceToHost));
  if (nbuckets) *nbuckets = 1u << t->p1max;  // (the stamp rows are laid out for p1max)
  return PMDFC_OK;
}

int pmdfc_cceh_last_get_lines(pmdfc_cceh_t* t, uint64_t* lines) {
  if (!t || !lines) return fail(PMDFC_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> lk(t->mu);
  if (!t->last_get_counted) return fail(PMDFC_ERR_STATE, "last get was not counted (enable timing)");
  DevGuard g(t->dev);
  HIPCHK(hipDeviceSynchronize());
  const uint64_t nb = t->last_get_blocks;
  std::vector<uint32_t> p(nb);
  HIPCHK(hipMemcpy(p.data(), t->partials, nb * 4, hipMemcpyDeviceToHost));
  uint64_t sum = 0;
  for (auto v : p) sum += v;
  *lines = sum;
  return PMDFC_OK;
}

int pmdfc_hash64(const uint64_t* keys, uint64_t* out, uint64_t n, void* stream) {
  if (n && (!keys || !out)) return fail(PMDFC_ERR_ARG, "null argument");
  launch_hash(keys, out, n, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return PMDFC_OK;
}

int pmdfc_gen_keys(uint64_t seed, uint64_t start, uint64_t* out, uint64_t n, void* stream) {
  if (n && !out) return fail(PMDFC_ERR_ARG, "null argument");
  launch_gen_keys(seed, start, out, n, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return PMDFC_OK;
}
