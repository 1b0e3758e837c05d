// engine_state.h -- the table's host state (struct pmdfc_cceh) and the few
// engine functions that the sibling host files call.  cceh_engine.hip owns
// both; everything else it defines stays static there.  Host only.
#pragma once
#include <algorithm>
#include <mutex>
#include <vector>

#include "cceh_device.h"
#include "cceh_kernels.h"
#include "host_common.h"
#include "knobs.h"

namespace pmdfc {

// Per-class kernel time from HIP events on the launching stream.  Consecutive
// intervals share their boundary event (begin() closes the open interval), and
// events skip the system-scope fence, so timing perturbs the stream as little
// as possible.
struct Timing {
  bool on = false;
  struct Rec {
    int cls;
    hipEvent_t a, b;
  };
  std::vector<Rec> recs;
  std::vector<hipEvent_t> pool;
  hipEvent_t open = nullptr;
  int open_cls = -1;
  double ms[PMDFC_K_COUNT] = {0};
  uint64_t launches[PMDFC_K_COUNT] = {0};

  hipEvent_t ev() {
    if (!pool.empty()) {
      hipEvent_t e = pool.back();
      pool.pop_back();
      return e;
    }
    hipEvent_t e;
    (void)hipEventCreateWithFlags(&e, hipEventDisableSystemFence);
    return e;
  }
  void begin(int cls, hipStream_t s) {
    if (!on) return;
    hipEvent_t e = ev();
    (void)hipEventRecord(e, s);
    if (open) recs.push_back({open_cls, open, e});
    open = e;
    open_cls = cls;
    if (recs.size() > 4096) flush_closed();
  }
  // an interval on another stream (the partition stream of insert_batches):
  // its own event pair, the open interval is untouched
  hipEvent_t span_begin(hipStream_t s) {
    if (!on) return nullptr;
    hipEvent_t e = ev();
    (void)hipEventRecord(e, s);
    return e;
  }
  void span_end(int cls, hipEvent_t a, hipStream_t s) {
    if (!on || !a) return;
    hipEvent_t e = ev();
    (void)hipEventRecord(e, s);
    recs.push_back({cls, a, e});
    if (recs.size() > 4096) flush_closed();
  }
  void end(hipStream_t s) {
    if (!on || !open) return;
    hipEvent_t e = ev();
    (void)hipEventRecord(e, s);
    recs.push_back({open_cls, open, e});
    open = nullptr;
  }
  void flush_closed() {
    // an event may close one interval and open the next: recycle it once
    std::vector<hipEvent_t> done;
    for (auto& r : recs) {
      (void)hipEventSynchronize(r.b);
      float t = 0;
      (void)hipEventElapsedTime(&t, r.a, r.b);
      ms[r.cls] += t;
      launches[r.cls] += 1;
      done.push_back(r.a);
      done.push_back(r.b);
    }
    recs.clear();
    std::sort(done.begin(), done.end());
    done.erase(std::unique(done.begin(), done.end()), done.end());
    for (auto e : done)
      if (e != open) pool.push_back(e);
  }
  ~Timing() {
    flush_closed();
    if (open) pool.push_back(open);
    for (auto e : pool) (void)hipEventDestroy(e);
  }
};

// segments per directory bucket past which the first pass takes its wide
// variant, and past which k_apply_fb is launched for the buckets it declines
// (sub-directories past 128 entries)
constexpr uint32_t kWideSegs = 20;
constexpr uint32_t kFbSegs = 64;
constexpr uint32_t kHintMixed = 6;  // h_hint word: the tag of the last mixed batch whose mixed passes ran (k_apply<true>)
constexpr uint32_t kHintMixIns = 7;  // h_hint word: the inserts of the last mixed batch (the next batch's mode)

}  // namespace pmdfc

struct pmdfc_cceh {
  pmdfc_cceh_config_t cfg{};
  int dev = 0;
  uint32_t D0 = 1, sbits = 0, shard = 0;
  uint32_t p1 = 0;        // directory bucket bits (grows to p1max as the table deepens: rebucket_now)
  uint32_t p1_init = 0, p1max = 0;
  // (what ONE batch's launches are filled from is a BatchPlan, not kept here)
  uint32_t clean_sbb = ~0u;  // the next record buffer's cursors are zero for a batch of this sbb (~0: all zero)
  size_t cblk = 0;        // cursor block per record buffer, sized for p1max
  uint64_t* hdr_tmp = nullptr;  // re-bucketing: the old headers
  uint32_t* h_depth = nullptr;  // pinned: k_min_ldep's result
  uint32_t* h_hint = nullptr;   // pinned, coherent: the segment count as k_apply_parked last set it (a hint)
  uint32_t* d_hint = nullptr;   // its device mapping
  uint32_t* minld = nullptr;     // device word: the smallest live local depth
  uint64_t rebuckets = 0;
  uint32_t parity = 0;    // batch parity: the bucket passes' per-batch words (grant shards, worklists)
  uint32_t rb = 0;        // record buffer of the next batch (0..kRecBufs-1): records, cursors, k_part overflow
  uint64_t max_segs = 0;
  uint32_t max_batch = 0;
  pmdfc::CreateKnobs kn;         // the environment knobs as this engine's create read them (knobs.h)
  uint32_t upsert = 0;    // PMDFC_CFG_UPSERT: last-writer-wins Insert
  uint16_t* upos = nullptr;  // upsert: pre-batch slot of each op's key (max_batch)

  ulonglong2* pairs = nullptr;
  uint32_t* occ = nullptr;
  uint8_t* ldep = nullptr;
  uint64_t* hdr = nullptr;    // 2^p1 bucket headers (room for 2^p1max)
  uint32_t* pool = nullptr;   // sub-directories
  uint64_t pool_cap = 0;      // entries
  uint64_t seq = 0;             // mixed batch epoch
  // the mixed batches' device state (what fill_mixed_launch hands the kernels)
  struct Mixed {
    uint64_t* iset = nullptr;     // the batch's inserted keys (2^k >= 2 max_batch slots)
    uint64_t imask = 0;
    uint32_t* ipos = nullptr;     // per set slot, the key's insert position (valid if single)
    uint32_t* islot = nullptr;    // per op, its insert's set slot (~0: none) -- the verify pass clears it
    uint32_t* icnt = nullptr;     // per set slot, 1 if the key is inserted more than once
    uint32_t* icount = nullptr;   // per 256-op block, its inserts (k_mixed_prep / k_mixed_get), summed into the host's
                                  // mode hint and, in insert-set mode, ctl->ins_total (k_mixed_get_iset / k_mixed_join)
    uint32_t* jbits = nullptr;    // the joining Gets' filter, one per set replica (kJoinWords)
    uint8_t* early = nullptr;     // per op, 1 early single-copy hit, 2 linked to its insert
    uint32_t* elink = nullptr;    // per op, the linked insert's position (early 2) or the
                                  // pre-batch segment's local depth (early 1)
    uint32_t* loss0 = nullptr;    // ctl->loss_events before the batch
    ulonglong2* drops = nullptr;  // the drop log (kDropLog entries)
    uint64_t last_n = 0;          // the last batch's size (with the pinned insert count: mixed_join_mode)
    bool iset_dirty = false;      // a batch's prep ran without its verify pass (an error return)
  } mx;

  pmdfc::DevCtl* ctl = nullptr;
  pmdfc::DevCtl* hctl = nullptr;  // pinned mirror (stats / dump only)

  // partition records
  ulonglong2* rkv = nullptr;   // records {key, value}
  uint32_t* rop = nullptr;
  uint16_t* robk = nullptr;    // overflow records' bucket
  uint64_t nrec = 0;           // record slots per record buffer
  uint32_t* cursor = nullptr;  // kRecBufs x (the partition buckets' region cursors + 1 overflow cursor)
  uint64_t* wstat = nullptr;   // per directory bucket counters (summed by stats())
  ulonglong2* wl_kv = nullptr; // parked ops per directory bucket (apply -> final pass)
  uint32_t* wl_op = nullptr;
  uint32_t* wl_n = nullptr;
  // split rounds: requests per bucket, grants, the sharded request lists
  uint2* req = nullptr;
  uint32_t* reqop = nullptr;  // batch position of each request's insert (the drop log's trigger)
  uint32_t* need = nullptr;
  uint32_t* gbase = nullptr;
  uint32_t* ngrant = nullptr;
  uint32_t* newoff = nullptr;
  uint64_t* gsh = nullptr;  // [2][kGShards] grant shard words, kGStride apart
  uint4* gsplit = nullptr;  // [2][kGShards][gcap] the requested splits
  uint32_t gcap = 0;
  uint32_t* act = nullptr;  // buckets with requests (k_split -> k_apply_parked)
  uint32_t* touched = nullptr;  // medium batches: partition buckets that received ops ([0]: count)
  uint32_t* povf = nullptr;     // k_part: [parity][tile][partition bucket] overflow slots
  // worklist: final-pass buckets by parity
  uint32_t* fin = nullptr;
  uint32_t* fbl = nullptr;    // [2^p1max] buckets the lean first pass declined (bit 0) and decline counts

  uint32_t* partials = nullptr;
  unsigned long long* popc = nullptr;
  uint8_t* srv_st = nullptr;     // serving wave: a chunk's statuses (64) and Get values (64)
  uint64_t* srv_vout = nullptr;
  uint64_t* stamps = nullptr;  // debug (kn.stamps): [0, 8*nb) k_bucket, then k_part
  // (kn.stamp_rot sets, batch i writing set i % stamp_rot, for a timeline of
  // consecutive pipelined batches; stamp_last: the set of the last batch
  // planned, for pmdfc_cceh_debug_stamps -- plan_batch alone writes both)
  uint64_t* stamp_last = nullptr;
  uint32_t stamp_seq = 0;
  std::vector<void*> dev_allocs;  // every hipMalloc of create (ALLOC), for destroy

  // insert_batches: batch i+1 is partitioned on pstream while batch i is
  // applied on the caller's stream
  hipStream_t pstream = nullptr;
  hipEvent_t ev_in = nullptr, ev_part[pmdfc::kRecBufs] = {}, ev_done[pmdfc::kRecBufs] = {};
  hipEvent_t ev_gpart[2] = {}, ev_gdone[2] = {};  // pipe_group: a group's partitions / passes done
  hipEvent_t ev_minld = nullptr;  // the last rebucket_now depth copy
  bool minld_pending = false;

  uint64_t batches = 0;
  uint64_t last_get_n = 0, last_get_blocks = 0;
  bool last_get_counted = false;
  bool count_lines = false;
  pmdfc::Timing timing;
  std::mutex mu;

  uint32_t* gflat = nullptr;       // flattened directory (pure Gets), 2^kFlatMaxBits entries
  uint32_t* gflat_bits = nullptr;  // its physical depth (device)
  bool flat_valid = false;         // host: no insert since the last flatten

  // Erase batches (erase.hip): five rows of max_batch words (segment ids and
  // batch indices before and after the sort, the run heads), the runs' cursor
  // and the sort's temporary storage; allocated by the first Erase
  struct Erase {
    uint32_t* rows = nullptr;
    uint32_t* cursor = nullptr;
    void* tmp = nullptr;
    size_t tmp_bytes = 0;
    uint32_t sort_bits = 0;
  } er;

  unsigned long long* match_out = nullptr;  // EraseMatching's four result words (allocated by the first call)

  std::vector<float> compact_ms;  // the last Compact's steps (pmdfc_cceh_compact_timing)

  pmdfc::Geo geo() const { return pmdfc::Geo{hdr, pool, p1, sbits, shard, nullptr, nullptr}; }
  pmdfc::Geo geo_flat() const { return pmdfc::Geo{hdr, pool, p1, sbits, shard, gflat, gflat_bits}; }
};

// The counting bloom filter (filter_host.hip).  Its state is here because the
// table reads it in one place: serve_start hands the serving wave the
// filter's counters.
struct pmdfc_cbf {
  int dev = 0;
  uint64_t nbits = 0, nwords = 0, padded = 0;
  uint32_t k = 0;
  uint8_t* cnt = nullptr;   // padded to kCbfChunk, padding stays zero
  uint64_t* bm = nullptr;   // nwords, MSB-first
  uint32_t* flag = nullptr; // delete-batch conflict flag
};

// Who reaches into the table from outside cceh_engine.hip, and why (all of
// these expect t->mu held and the table's device current, except do_insert and
// do_get, which take both themselves):
//   image_host.hip  read_ctl          the live segment count of a snapshot
//                   start_host_state  a restore's bucket bits and host-side batch state
//                   batch_words       the per-batch words launch_image_ctl zeroes
//                   init_state        the reset after a restore that found keys outside their prefix
//   extent_host.hip do_insert, do_get the expanded extent entries, batch by batch
//   dist_host.hip   pipe_begin, pipe_batch, pipe_end
//                                     the routed loop's received inserts through the partition
//                                     pipeline -- the one place outside the engine that takes t->mu
//                                     and drives batches itself
// (filter_host.hip takes t->mu and reads dev, pairs, ctl, max_segs, geo() and
// timing, but calls nothing.)
namespace pmdfc {

int read_ctl(pmdfc_cceh* t, hipStream_t s);
int start_host_state(pmdfc_cceh* t, hipStream_t s, uint32_t p1, uint32_t min_ld);
InitZero batch_words(const pmdfc_cceh* t);
int init_state(pmdfc_cceh* t, hipStream_t s);

int do_insert(pmdfc_cceh* t, const uint64_t* keys, const uint64_t* vin, uint32_t kvs, uint8_t* st, uint64_t n,
              void* stream);
int do_get(pmdfc_cceh* t, const uint64_t* keys, uint64_t* vout, uint8_t* st, uint64_t n, void* stream);

int pipe_begin(pmdfc_cceh* t, hipStream_t s);
int pipe_batch(pmdfc_cceh* t, const uint64_t* keys, const uint64_t* vin, uint32_t kvs, uint8_t* st, uint64_t n,
               hipStream_t s, uint32_t k, hipEvent_t input_ready, hipEvent_t output_free = nullptr);
int pipe_end(pmdfc_cceh* t, hipStream_t s);

}  // namespace pmdfc
