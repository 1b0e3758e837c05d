// dist_host.hip -- communicators and the native routed batches.
//
// The loop of pmdfc_amd.dist.BlockRouter._call_body in C++ with RCCL called
// directly: per batch one pack (route.hip), one equal-split all-to-all of the
// owner blocks, the owner's engine on the received rows, one all-to-all of
// the responses and one unpack.  Two streams joined by events: the
// communicator's (packs and both exchanges) and the caller's (the engine and
// the unpacks), so batch i+1's pack and request exchange and batch i-1's
// response exchange run while batch i is applied.  Buffers: requests and
// responses double-buffered, row positions triple-buffered (pack i+3 waits
// for unpack i).
//
// The router's state and pack come from route_host.h.  route_batches is the
// one place outside the engine that takes the table's lock and drives batches
// itself (pipe_begin / pipe_batch / pipe_end, engine_state.h).
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "engine_state.h"
#include "host_common.h"
#include "route_host.h"

using namespace pmdfc;

struct pmdfc_comm {
  ncclComm_t comm = nullptr;
  int nranks = 1, rank = 0, device = 0;
  hipStream_t cs = nullptr;  // the exchanges' stream
  hipEvent_t ev[14] = {};
  // host-staged transport (pmdfc_comm_create_host): the exchanges go
  // through the caller's functions on pinned host copies instead of RCCL
  pmdfc_host_exchange_fn xchg = nullptr;
  pmdfc_host_allreduce_fn amax = nullptr;
  void* xctx = nullptr;
  uint8_t* hbuf = nullptr;  // [send | recv] staging, 2 * hcap bytes
  size_t hcap = 0;
};

namespace {
int nccl_fail(const char* what, ncclResult_t r) {
  char buf[256];
  snprintf(buf, sizeof buf, "%s: %s", what, ncclGetErrorString(r));
  return fail(PMDFC_ERR_HIP, buf);
}
}  // namespace

#define NCCLCHK(x)                                   \
  do {                                               \
    ncclResult_t r_ = (x);                           \
    if (r_ != ncclSuccess) return nccl_fail(#x, r_); \
  } while (0)

static_assert(sizeof(ncclUniqueId) == PMDFC_COMM_ID_BYTES, "RCCL unique id size");

int pmdfc_comm_id(uint8_t* id_out) {
  if (!id_out) return fail(PMDFC_ERR_ARG, "comm_id: null output");
  ncclUniqueId id;
  NCCLCHK(ncclGetUniqueId(&id));
  memcpy(id_out, &id, sizeof id);
  return PMDFC_OK;
}

int pmdfc_comm_create(const uint8_t* id, int nranks, int rank, int device, pmdfc_comm_t** out) {
  if (!id || !out || nranks < 1 || rank < 0 || rank >= nranks) return fail(PMDFC_ERR_ARG, "comm_create: bad argument");
  *out = nullptr;
  DevGuard g(device);
  auto* c = new pmdfc_comm();
  c->nranks = nranks;
  c->rank = rank;
  c->device = device;
  ncclUniqueId uid;
  memcpy(&uid, id, sizeof uid);
  ncclResult_t nr = ncclCommInitRank(&c->comm, nranks, uid, rank);
  if (nr != ncclSuccess) {
    delete c;
    return nccl_fail("ncclCommInitRank", nr);
  }
  hipError_t e = hipStreamCreateWithFlags(&c->cs, hipStreamNonBlocking);
  for (auto& ev : c->ev)
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
  if (e != hipSuccess) {
    pmdfc_comm_destroy(c);
    return fail(PMDFC_ERR_HIP, "comm_create", e);
  }
  *out = c;
  return PMDFC_OK;
}

int pmdfc_comm_create_host(int nranks, int rank, int device, pmdfc_host_exchange_fn xchg,
                           pmdfc_host_allreduce_fn amax, void* ctx, pmdfc_comm_t** out) {
  if (!out || !xchg || !amax || nranks < 1 || rank < 0 || rank >= nranks)
    return fail(PMDFC_ERR_ARG, "comm_create_host: bad argument");
  *out = nullptr;
  DevGuard g(device);
  auto* c = new pmdfc_comm();
  c->nranks = nranks;
  c->rank = rank;
  c->device = device;
  c->xchg = xchg;
  c->amax = amax;
  c->xctx = ctx;
  hipError_t e = hipStreamCreateWithFlags(&c->cs, hipStreamNonBlocking);
  for (auto& ev : c->ev)
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
  if (e != hipSuccess) {
    pmdfc_comm_destroy(c);
    return fail(PMDFC_ERR_HIP, "comm_create_host", e);
  }
  *out = c;
  return PMDFC_OK;
}

int pmdfc_comm_destroy(pmdfc_comm_t* c) {
  if (!c) return PMDFC_OK;
  DevGuard g(c->device);
  if (c->cs) (void)hipStreamSynchronize(c->cs);
  if (c->hbuf) (void)hipHostFree(c->hbuf);
  if (c->comm) (void)ncclCommDestroy(c->comm);
  for (auto& ev : c->ev)
    if (ev) (void)hipEventDestroy(ev);
  if (c->cs) (void)hipStreamDestroy(c->cs);
  delete c;
  return PMDFC_OK;
}

// width 1: Get, 2: Insert, 3: mixed (ops; the received rows are split into
// the engine's key / value / op arrays, applied by pmdfc_cceh_mixed and
// answered as 16-B responses, as BlockRouter._run_mixed does)
static int route_batches(pmdfc_router_t* r, pmdfc_cceh_t* t, pmdfc_comm_t* c, uint32_t width, const uint8_t* ops,
                         const uint64_t* keys, const uint64_t* values, const uint64_t* bounds, uint64_t nb,
                         uint32_t dedupe, uint64_t* vout, uint8_t* st, void* stream) {
  if (!r || !t || !c || width < 1 || width > 3 || !bounds || !nb || !st || (width != 2 && !vout) ||
      (width >= 2 && !values) || (width == 3 && !ops) || !keys)
    return fail(PMDFC_ERR_ARG, "route_batches: bad argument (width 1: Get, 2: Insert, 3: mixed)");
  if ((int)r->G != c->nranks) return fail(PMDFC_ERR_ARG, "route_batches: 2^shard_bits != communicator ranks");
  if (r->rows > t->max_batch) return fail(PMDFC_ERR_ARG, "route_batches: engine max_batch < router rows");
  if (r->last_width) return fail(PMDFC_ERR_STATE, "route_batches: the router holds another call's carry");
  const uint64_t total = bounds[nb] - bounds[0];
  for (uint64_t i = 0; i < nb; ++i)
    if (bounds[i + 1] < bounds[i] || bounds[i + 1] - bounds[i] > r->cfg.max_batch)
      return fail(PMDFC_ERR_ARG, "route_batches: a batch is empty-negative or past the router's max_batch");
  if (total >= kRouteNone) return fail(PMDFC_ERR_ARG, "route_batches: more than 2^32 - 2 ops");
  DevGuard g(c->device);
  hipStream_t S = (hipStream_t)stream, C = c->cs;
  // PMDFC_ROUTE_DIRECT=0: the pack / exchange / unpack path even on one rank
  // (its per-batch cost, measured where no peer exists; A/B and tests)
  if (process_knobs().route_direct && c->nranks == 1 && r->cfg.cap >= r->cfg.max_batch) {
    // One rank: every op's owner is this rank, its block never moves and
    // holds a whole batch (cap >= max_batch: no carry can form), so the
    // routed call IS the direct call in batch order -- the engine runs on
    // the caller's arrays with call-global outputs (no pack, no exchange, no
    // unpack; a Get-only batch needs no dedupe).  Inserts go through the
    // engine's partition pipeline as pmdfc_cceh_insert_batches.
    const uint64_t o = bounds[0];
    std::vector<uint64_t> rb(nb + 1);  // the bounds from 0: the outputs are call-global
    for (uint64_t i = 0; i <= nb; ++i) rb[i] = bounds[i] - o;
    if (width == 2) return pmdfc_cceh_insert_batches(t, keys + o, values + o, st, rb.data(), (uint32_t)nb, S);
    if (width == 3)
      return pmdfc_cceh_mixed_batches(t, ops + o, keys + o, values + o, vout, st, rb.data(), (uint32_t)nb, S);
    return pmdfc_cceh_get_batches(t, keys + o, vout, st, rb.data(), (uint32_t)nb, S);
  }
  const uint64_t rows = r->rows, cap = r->cfg.cap;
  const bool dd = dedupe && width == 1;
  const size_t req_b = rows * width * 8, resp_b = width == 2 ? rows : rows * 16;
  // call buffers (stream-ordered allocations, freed at the end)
  void* buf = nullptr;
  const size_t off_recv = 2 * req_b, off_rs = 4 * req_b, off_rb = off_rs + 3 * resp_b, off_pos = off_rb + 2 * resp_b;
  const size_t off_keep = off_pos + 3 * rows * 4, off_lead = off_keep + ((r->cfg.max_batch + 255) & ~255ull);
  const size_t off_car = off_lead + (dd ? ((total * 4 + 255) & ~255ull) : 0), off_mix = off_car + 256;
  // mixed: the engine's arrays for one batch of received rows (keys, values,
  // values out, statuses, ops)
  const size_t mix_b = width == 3 ? rows * 26 + 1024 : 0, all_b = off_mix + mix_b;
  HIPCHK(hipMallocAsync(&buf, all_b, S));
  uint8_t* B8 = static_cast<uint8_t*>(buf);
  uint64_t* send[2] = {(uint64_t*)B8, (uint64_t*)(B8 + req_b)};
  uint64_t* recv[2] = {(uint64_t*)(B8 + off_recv), (uint64_t*)(B8 + off_recv + req_b)};
  uint8_t* rsend[3] = {B8 + off_rs, B8 + off_rs + resp_b, B8 + off_rs + 2 * resp_b};  // (read by unpack i: i % 3)
  uint8_t* rback[2] = {B8 + off_rb, B8 + off_rb + resp_b};
  uint32_t* rowpos[3] = {(uint32_t*)(B8 + off_pos), (uint32_t*)(B8 + off_pos + rows * 4),
                         (uint32_t*)(B8 + off_pos + 2 * rows * 4)};
  uint8_t* keep = B8 + off_keep;
  uint32_t* lead = (uint32_t*)(B8 + off_lead);
  uint64_t* car = (uint64_t*)(B8 + off_car);
  uint64_t* mk = (uint64_t*)(B8 + off_mix);
  uint64_t* mv = mk + rows;
  uint64_t* mvo = mv + rows;
  uint8_t* mst = (uint8_t*)(mvo + rows);
  uint8_t* mop = mst + ((rows + 255) & ~255ull);
  hipEvent_t* evPack = c->ev;      // [2]
  hipEvent_t* evReq = c->ev + 2;   // [2]
  hipEvent_t* evRun = c->ev + 4;   // [2]
  hipEvent_t* evResp = c->ev + 6;  // [2]
  hipEvent_t evCar = c->ev[8], evCarDone = c->ev[9];
  hipEvent_t* evFin = c->ev + 10;  // [3]: unpack i done (pack i + 3 reuses its row positions)
  hipEvent_t evJoin = c->ev[13];
  (void)evPack;
  int rc = PMDFC_OK;
  // an all-to-all of equal blocks of `bytes` without the local block (it
  // never moves): grouped point-to-point sends and receives over RCCL
  auto exchange = [&](const void* sb, void* rb, uint64_t bytes) -> int {
    if (c->nranks == 1) return PMDFC_OK;
    if (c->xchg) {  // host-staged: the blocks through pinned host memory and the caller's transport
      const size_t tot = (size_t)c->nranks * bytes;
      if (tot > c->hcap) {
        if (c->hbuf) HIPCHK(hipHostFree(c->hbuf));
        c->hbuf = nullptr;
        HIPCHK(hipHostMalloc((void**)&c->hbuf, 2 * tot, hipHostMallocDefault));
        c->hcap = tot;
      }
      uint8_t* hs = c->hbuf;
      uint8_t* hr = c->hbuf + c->hcap;
      HIPCHK(hipMemcpyAsync(hs, sb, tot, hipMemcpyDeviceToHost, C));
      HIPCHK(hipStreamSynchronize(C));
      if (c->xchg(c->xctx, hs, hr, bytes) != 0) return fail(PMDFC_ERR_HIP, "route_batches: host exchange failed");
      for (int p = 0; p < c->nranks; ++p)  // (the local block never moves)
        if (p != c->rank)
          HIPCHK(hipMemcpyAsync(static_cast<uint8_t*>(rb) + (uint64_t)p * bytes, hr + (uint64_t)p * bytes, bytes,
                                hipMemcpyHostToDevice, C));
      HIPCHK(hipStreamSynchronize(C));  // (the staging is reused by the next exchange)
      return PMDFC_OK;
    }
    NCCLCHK(ncclGroupStart());
    for (int p = 0; p < c->nranks; ++p) {
      if (p == c->rank) continue;
      NCCLCHK(ncclSend(static_cast<const uint8_t*>(sb) + (uint64_t)p * bytes, bytes, ncclUint8, p, c->comm, C));
      NCCLCHK(ncclRecv(static_cast<uint8_t*>(rb) + (uint64_t)p * bytes, bytes, ncclUint8, p, c->comm, C));
    }
    NCCLCHK(ncclGroupEnd());
    return PMDFC_OK;
  };
  // the caller's stream holds the inputs' producers: the exchanges' stream
  // starts after them
  if (hipEventRecord(evJoin, S) != hipSuccess || hipStreamWaitEvent(C, evJoin, 0) != hipSuccess)
    rc = fail(PMDFC_ERR_HIP, "route_batches: join");
  auto pack = [&](uint64_t i) -> int {
    const uint64_t n = i < nb ? bounds[i + 1] - bounds[i] : 0;
    const uint64_t o = i < nb ? bounds[i] - bounds[0] : 0;
    const uint64_t* k = n ? keys + bounds[i] : nullptr;
    const uint64_t* v = n && width >= 2 ? values + bounds[i] : nullptr;
    const uint8_t* op = n && width == 3 ? ops + bounds[i] : nullptr;
    const uint8_t* kp = nullptr;
    if (i >= 3) HIPCHK(hipStreamWaitEvent(C, evFin[i % 3], 0));
    if (dd && n) {
      const int e = pmdfc_router_dedupe(r, k, nullptr, n, (uint32_t)o, keep, lead, C);
      if (e) return e;
      kp = keep;
    }
    // the local block goes straight into its receive slot; only peer blocks travel
    const int e = router_pack(r, k, v, op, kp, n, width, (uint32_t)o, send[i & 1], rowpos[i % 3],
                              width != 2 ? vout : nullptr, st, C, (uint32_t)c->rank,
                              recv[i & 1] + (uint64_t)c->rank * cap * width);
    if (e) return e;
    if ((rc = exchange(send[i & 1], recv[i & 1], cap * width * 8))) return rc;
    HIPCHK(hipEventRecord(evReq[i & 1], C));
    return PMDFC_OK;
  };
  // inserts at p1max go through the engine's pipeline (the partition of
  // batch i + 1 on the engine's partition stream, right after its rows
  // arrive, under batch i's bucket passes); a coarser table ramps batch by
  // batch first
  // (PMDFC_ROUTE_PIPE=1; measured slower on one rank: the partitions ran at
  // ~100 us beside the packs instead of ~40 us inline)
  const bool pipe_inserts = process_knobs().route_pipe;
  uint32_t piped = 0;
  auto run = [&](uint64_t i) -> int {
    int e = PMDFC_OK;
    if (pipe_inserts && width == 2 && t->p1 >= t->p1max) {
      std::lock_guard<std::mutex> lk(t->mu);
      if (piped == 0) e = pipe_begin(t, S);
      // (the statuses buffer's last reader: the unpack of batch i - 3)
      if (!e)
        e = pipe_batch(t, recv[i & 1], recv[i & 1] + 1, 2, rsend[i % 3], rows, S, piped++, evReq[i & 1],
                       i >= 3 ? evFin[i % 3] : nullptr);
    } else {
      if (piped) {  // (cannot happen: a table never gets coarser)
        std::lock_guard<std::mutex> lk(t->mu);
        e = pipe_end(t, S);
        piped = 0;
      }
      HIPCHK(hipStreamWaitEvent(S, evReq[i & 1], 0));
      if (!e && width == 3) {
        launch_route_split(recv[i & 1], rows, 3, mk, mv, mop, S);
        e = pmdfc_cceh_mixed(t, mop, mk, mv, mvo, mst, rows, S);
        if (!e) launch_route_resp(mvo, mst, rows, rsend[i % 3], S);
        if (!e && hipGetLastError() != hipSuccess) e = fail(PMDFC_ERR_HIP, "route_batches: split / respond");
      } else if (!e) {
        e = width == 2 ? pmdfc_cceh_insert_records(t, recv[i & 1], rsend[i % 3], rows, S)
                       : pmdfc_cceh_get_records(t, recv[i & 1], (uint64_t*)rsend[i % 3], rows, S);
      }
    }
    if (e) return e;
    HIPCHK(hipEventRecord(evRun[i & 1], S));
    HIPCHK(hipStreamWaitEvent(C, evRun[i & 1], 0));
    if ((rc = exchange(rsend[i % 3], rback[i & 1], width == 2 ? cap : cap * 16))) return rc;
    HIPCHK(hipEventRecord(evResp[i & 1], C));
    return PMDFC_OK;
  };
  auto finish = [&](uint64_t i) -> int {
    HIPCHK(hipStreamWaitEvent(S, evResp[i & 1], 0));
    // (the local block's responses are read where the engine wrote them)
    launch_route_unpack(rback[i & 1], width == 2 ? 0u : 1u, rowpos[i % 3], rows, width != 2 ? vout : nullptr, st, S,
                        rsend[i % 3], (uint64_t)c->rank * cap, (uint64_t)(c->rank + 1) * cap);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(evFin[i % 3], S));
    return PMDFC_OK;
  };
  if (rc == PMDFC_OK) rc = pack(0);
  uint64_t i = 0, pend = 0;
  bool pending = false;
  while (rc == PMDFC_OK) {
    if (i + 1 < nb && (rc = pack(i + 1))) break;
    if ((rc = run(i))) break;
    if (pending && (rc = finish(pend))) break;
    pending = true;
    pend = i;
    if (++i < nb) continue;
    // drain: every rank exchanges until no rank carries ops (the counts come
    // from the last pack, on the exchanges' stream)
    if (hipEventRecord(evJoin, C) != hipSuccess || hipStreamWaitEvent(S, evJoin, 0) != hipSuccess) {
      rc = fail(PMDFC_ERR_HIP, "route_batches: join");
      break;
    }
    if ((rc = pmdfc_router_carried(r, car, S))) break;
    if (c->nranks > 1) {
      if (hipEventRecord(evCar, S) != hipSuccess || hipStreamWaitEvent(C, evCar, 0) != hipSuccess) {
        rc = fail(PMDFC_ERR_HIP, "route_batches: carried event");
        break;
      }
      if (c->amax) {  // host-staged transport
        uint64_t hv = 0;
        if (hipMemcpyAsync(&hv, car, 8, hipMemcpyDeviceToHost, C) != hipSuccess || hipStreamSynchronize(C) != hipSuccess ||
            c->amax(c->xctx, &hv) != 0 || hipMemcpyAsync(car, &hv, 8, hipMemcpyHostToDevice, C) != hipSuccess ||
            hipStreamSynchronize(C) != hipSuccess) {
          rc = fail(PMDFC_ERR_HIP, "route_batches: host all-reduce failed");
          break;
        }
      } else {
        const ncclResult_t nr = ncclAllReduce(car, car, 1, ncclUint64, ncclMax, c->comm, C);
        if (nr != ncclSuccess) {
          rc = nccl_fail("ncclAllReduce", nr);
          break;
        }
      }
      if (hipEventRecord(evCarDone, C) != hipSuccess || hipStreamWaitEvent(S, evCarDone, 0) != hipSuccess) {
        rc = fail(PMDFC_ERR_HIP, "route_batches: carried event");
        break;
      }
    }
    uint64_t h = 0;
    if (hipMemcpyAsync(&h, car, 8, hipMemcpyDeviceToHost, S) != hipSuccess || hipStreamSynchronize(S) != hipSuccess) {
      rc = fail(PMDFC_ERR_HIP, "route_batches: carried count");
      break;
    }
    if (h == 0) break;
    rc = pack(i);  // a drain exchange (no new ops)
  }
  if (rc == PMDFC_OK && pending) rc = finish(pend);
  if (rc == PMDFC_OK && piped) {
    std::lock_guard<std::mutex> lk(t->mu);
    rc = pipe_end(t, S);
  }
  if (rc == PMDFC_OK && (hipEventRecord(evJoin, C) != hipSuccess || hipStreamWaitEvent(S, evJoin, 0) != hipSuccess))
    rc = fail(PMDFC_ERR_HIP, "route_batches: join");
  if (rc == PMDFC_OK) rc = pmdfc_router_end_call(r);
  if (rc == PMDFC_OK && dd) rc = pmdfc_router_fill(lead, total, vout, st, c->device, S);
  if (rc == PMDFC_OK && hipFreeAsync(buf, S) != hipSuccess) rc = fail(PMDFC_ERR_HIP, "route_batches: free");
  // every failure since buf was allocated leaves here (a failed free is tried once more)
  if (rc != PMDFC_OK) {
    const std::string err = last_error();  // (the reset below must not hide the first error)
    (void)hipStreamSynchronize(C);
    (void)pmdfc_router_reset(r, S);
    (void)hipFreeAsync(buf, S);
    last_error() = err;
  }
  return rc;
}

int pmdfc_route_batches(pmdfc_router_t* r, pmdfc_cceh_t* t, pmdfc_comm_t* c, uint32_t width, const uint64_t* keys,
                        const uint64_t* values, const uint64_t* bounds, uint64_t nb, uint32_t dedupe,
                        uint64_t* vout, uint8_t* st, void* stream) {
  if (width != 1 && width != 2) return fail(PMDFC_ERR_ARG, "route_batches: bad argument (width 1: Get, 2: Insert)");
  return route_batches(r, t, c, width, nullptr, keys, values, bounds, nb, dedupe, vout, st, stream);
}

int pmdfc_route_mixed_batches(pmdfc_router_t* r, pmdfc_cceh_t* t, pmdfc_comm_t* c, const uint8_t* ops,
                              const uint64_t* keys, const uint64_t* values, const uint64_t* bounds, uint64_t nb,
                              uint64_t* vout, uint8_t* st, void* stream) {
  if (!ops) return fail(PMDFC_ERR_ARG, "route_mixed_batches: null ops");
  return route_batches(r, t, c, 3, ops, keys, values, bounds, nb, 0, vout, st, stream);
}
