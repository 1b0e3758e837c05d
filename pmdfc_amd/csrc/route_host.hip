// route_host.hip -- host side of the request routing (kernels: route.hip):
// route_by_shard, the block router and the split / respond helpers.  Nothing
// here touches the table; the routed loop over a communicator is in
// dist_host.hip (route_host.h is what it needs from here).
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include <vector>

#include "cceh_kernels.h"
#include "host_common.h"
#include "route_host.h"

using namespace pmdfc;

int pmdfc_route_by_shard(const uint64_t* keys, uint64_t n, uint32_t shard_bits, uint32_t* perm,
                         uint64_t* h_counts, int device, void* stream) {
  if (shard_bits > 16 || (n && (!keys || !perm || !h_counts))) return fail(PMDFC_ERR_ARG, "bad argument");
  DevGuard g(device);
  hipStream_t s = (hipStream_t)stream;
  const uint32_t G = 1u << shard_bits;
  if (n == 0) {
    for (uint32_t i = 0; i < G; ++i) h_counts[i] = 0;
    return PMDFC_OK;
  }
  {
    // (freed on s at the end of this block, before the final synchronise)
    StreamTmp t_own, t_own2, t_idx, t_starts;
    size_t bytes = 0;
    HIPCHK(t_own.alloc(n * 4, s));
    HIPCHK(t_own2.alloc(n * 4, s));
    HIPCHK(t_idx.alloc(n * 4, s));
    HIPCHK(t_starts.alloc((G + 1) * 8, s));
    uint32_t *own = t_own.as<uint32_t>(), *own2 = t_own2.as<uint32_t>(), *idx = t_idx.as<uint32_t>();
    uint64_t* starts = t_starts.as<uint64_t>();
    if (shard_bits == 0) {
      launch_owner(keys, n, 0, own, perm, s);  // own unused
      h_counts[0] = n;
    } else {
      launch_owner(keys, n, shard_bits, own, idx, s);
      HIPCHK(rocprim::radix_sort_pairs(nullptr, bytes, own, own2, idx, perm, (size_t)n, 0u, shard_bits, s));
      StreamTmp tmp;
      HIPCHK(tmp.alloc(bytes + 16, s));
      HIPCHK(rocprim::radix_sort_pairs(tmp.p, bytes, own, own2, idx, perm, (size_t)n, 0u, shard_bits, s));
      launch_bounds(own2, n, G, starts, s);
      std::vector<uint64_t> st(G + 1);
      HIPCHK(hipMemcpyAsync(st.data(), starts, (G + 1) * 8, hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
      for (uint32_t i = 0; i < G; ++i) h_counts[i] = st[i + 1] - st[i];
    }
  }
  HIPCHK(hipStreamSynchronize(s));
  return PMDFC_OK;
}

int pmdfc_router_create(const pmdfc_router_config* c, pmdfc_router_t** out) {
  if (!c || !out) return fail(PMDFC_ERR_ARG, "router_create: null argument");
  *out = nullptr;
  const uint32_t G = 1u << c->shard_bits;
  if (c->shard_bits > 4 || c->max_batch == 0 || c->cap == 0 || c->flags)
    return fail(PMDFC_ERR_ARG, "router_create: shard_bits <= 4, max_batch > 0, cap > 0, flags 0");
  if (c->cap * G >= 0xFFFFFFFFULL) return fail(PMDFC_ERR_ARG, "router_create: cap * 2^shard_bits < 2^32");
  DevGuard g(c->device);
  auto* r = new pmdfc_router();
  r->cfg = *c;
  if (!r->cfg.carry_cap) r->cfg.carry_cap = c->max_batch;
  r->G = G;
  r->rows = c->cap * G;
  const uint64_t cc = r->cfg.carry_cap;
  hipError_t e = hipSuccess;
  auto A = [&](void** p, size_t bytes) {
    if (e == hipSuccess) e = hipMalloc(p, bytes);
  };
  A((void**)&r->tile_cnt, (size_t)route_tiles(c->max_batch) * G * 4 + 4);
  A((void**)&r->cnt, 2 * G * 4);
  A((void**)&r->ovf, 4);
  A((void**)&r->crec, 2 * G * cc * kCarryWords * 8);
  A((void**)&r->cpos, 2 * G * cc * 4);
  if (e == hipSuccess) e = hipMemset(r->cnt, 0, 2 * G * 4);
  if (e == hipSuccess) e = hipMemset(r->ovf, 0, 4);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    pmdfc_router_destroy(r);
    return fail(PMDFC_ERR_HIP, "router_create", e);
  }
  *out = r;
  return PMDFC_OK;
}

int pmdfc_router_destroy(pmdfc_router_t* r) {
  if (!r) return PMDFC_OK;
  DevGuard g(r->cfg.device);
  for (void* p : {(void*)r->tile_cnt, (void*)r->cnt, (void*)r->ovf, (void*)r->crec, (void*)r->cpos})
    if (p) (void)hipFree(p);
  delete r;
  return PMDFC_OK;
}

uint64_t pmdfc_router_rows(const pmdfc_router_t* r) { return r ? r->rows : 0; }

// (self_dst: owner self_g's block goes there instead of into send -- the
// native loop packs the local block straight into its receive slot)
int pmdfc::router_pack(pmdfc_router_t* r, const uint64_t* keys, const uint64_t* values, const uint8_t* ops,
                       const uint8_t* keep, uint64_t n, uint32_t width, uint32_t base, uint64_t* send,
                       uint32_t* rowpos, uint64_t* values_out, uint8_t* status_out, void* stream, uint32_t self_g,
                       uint64_t* self_dst) {
  if (!r || width < 1 || width > 3 || !send || !rowpos || (n && (!keys || !status_out)) ||
      (width >= 2 && n && !values) || (width == 3 && n && !ops))
    return fail(PMDFC_ERR_ARG, "router_pack: bad argument (width 1..3)");
  if (n > r->cfg.max_batch) return fail(PMDFC_ERR_ARG, "router_pack: n > max_batch");
  if ((uint64_t)base + n >= kRouteNone) return fail(PMDFC_ERR_ARG, "router_pack: base + n >= 2^32 - 1");
  if (r->last_width && r->last_width != width)
    return fail(PMDFC_ERR_STATE, "router_pack: carried records have another width (finish or reset the call)");
  DevGuard g(r->cfg.device);
  const uint64_t cc = r->cfg.carry_cap, G = r->G;
  const uint32_t pi = r->parity, po = pi ^ 1u;
  RouteArgs a{keys, values, ops, keep, n, r->cfg.shard_bits, width, r->cfg.cap, cc, base, send, rowpos,
              values_out, status_out, r->tile_cnt, r->cnt + pi * G, r->cnt + po * G,
              r->crec + pi * G * cc * kCarryWords, r->crec + po * G * cc * kCarryWords, r->cpos + pi * G * cc,
              r->cpos + po * G * cc, r->ovf, self_g, self_dst};
  launch_route_pack(a, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  r->parity = po;
  r->last_width = width;
  return PMDFC_OK;
}

int pmdfc_router_pack(pmdfc_router_t* r, const uint64_t* keys, const uint64_t* values, const uint8_t* ops,
                      const uint8_t* keep, uint64_t n, uint32_t width, uint32_t base, uint64_t* send,
                      uint32_t* rowpos, uint64_t* values_out, uint8_t* status_out, void* stream) {
  return router_pack(r, keys, values, ops, keep, n, width, base, send, rowpos, values_out, status_out, stream, 0,
                     nullptr);
}

int pmdfc_router_unpack(pmdfc_router_t* r, const void* back, uint32_t resp_width, const uint32_t* rowpos,
                        uint64_t* values_out, uint8_t* status_out, void* stream) {
  if (!r || resp_width > 1 || !back || !rowpos || !status_out) return fail(PMDFC_ERR_ARG, "router_unpack: bad argument");
  DevGuard g(r->cfg.device);
  launch_route_unpack(back, resp_width, rowpos, r->rows, values_out, status_out, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return PMDFC_OK;
}

int pmdfc_router_carried(pmdfc_router_t* r, uint64_t* d_out, void* stream) {
  if (!r || !d_out) return fail(PMDFC_ERR_ARG, "router_carried: bad argument");
  DevGuard g(r->cfg.device);
  launch_route_carried(r->cnt + r->parity * r->G, r->G, d_out, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return PMDFC_OK;
}

int pmdfc_router_end_call(pmdfc_router_t* r) {
  if (!r) return fail(PMDFC_ERR_ARG, "router_end_call: null router");
  r->last_width = 0;
  return PMDFC_OK;
}

int pmdfc_router_overflow_count(pmdfc_router_t* r, uint64_t* h_out, void* stream) {
  if (!r || !h_out) return fail(PMDFC_ERR_ARG, "router_overflow_count: bad argument");
  DevGuard g(r->cfg.device);
  uint32_t v = 0;
  HIPCHK(hipMemcpyAsync(&v, r->ovf, 4, hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  *h_out = v;
  return PMDFC_OK;
}

int pmdfc_router_reset(pmdfc_router_t* r, void* stream) {
  if (!r) return fail(PMDFC_ERR_ARG, "router_reset: null router");
  DevGuard g(r->cfg.device);
  HIPCHK(hipMemsetAsync(r->cnt, 0, 2 * r->G * 4, (hipStream_t)stream));
  HIPCHK(hipMemsetAsync(r->ovf, 0, 4, (hipStream_t)stream));
  r->parity = 0;
  r->last_width = 0;
  return PMDFC_OK;
}

int pmdfc_router_dedupe(pmdfc_router_t* r, const uint64_t* keys, const uint8_t* keep_in, uint64_t n, uint32_t base,
                        uint8_t* keep_out, uint32_t* lead_out, void* stream) {
  if (!r || (n && (!keys || !keep_out || !lead_out))) return fail(PMDFC_ERR_ARG, "router_dedupe: bad argument");
  if (n > r->cfg.max_batch) return fail(PMDFC_ERR_ARG, "router_dedupe: n > max_batch");
  if ((uint64_t)base + n >= kRouteNone) return fail(PMDFC_ERR_ARG, "router_dedupe: base + n >= 2^32 - 1");
  if (!n) return PMDFC_OK;
  DevGuard g(r->cfg.device);
  launch_route_dedupe(keys, keep_in, n, base, keep_out, lead_out, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return PMDFC_OK;
}

int pmdfc_router_fill(const uint32_t* lead, uint64_t n, uint64_t* values_out, uint8_t* status_out, int device,
                      void* stream) {
  if (n && (!lead || !status_out)) return fail(PMDFC_ERR_ARG, "router_fill: bad argument");
  DevGuard g(device);
  launch_route_fill(lead, n, values_out, status_out, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return PMDFC_OK;
}

int pmdfc_route_split(const uint64_t* recv, uint64_t rows, uint32_t width, uint64_t* keys, uint64_t* values,
                      uint8_t* ops, int device, void* stream) {
  if (width < 1 || width > 3 || (rows && (!recv || !keys || (width >= 2 && !values) || (width == 3 && !ops))))
    return fail(PMDFC_ERR_ARG, "route_split: bad argument");
  DevGuard g(device);
  launch_route_split(recv, rows, width, keys, values, ops, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return PMDFC_OK;
}

int pmdfc_route_respond(const uint64_t* values, const uint8_t* status, uint64_t rows, uint64_t* resp,
                        int device, void* stream) {
  if (rows && (!values || !status || !resp)) return fail(PMDFC_ERR_ARG, "route_respond: bad argument");
  DevGuard g(device);
  launch_route_resp(values, status, rows, resp, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return PMDFC_OK;
}
