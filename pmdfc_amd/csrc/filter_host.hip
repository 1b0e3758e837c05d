// filter_host.hip -- host side of the bloom filter and the counting bloom
// filter (kernels: bloom.hip, cbf.hip).  Three entry points take the table's
// lock and read its arrays: pmdfc_bloom_probe_then_get, pmdfc_cbf_rebuild and
// pmdfc_cbf_audit.  (struct pmdfc_cbf is in engine_state.h: the serving wave
// reads the counters.)
#include <hip/hip_runtime.h>

#include <mutex>

#include "engine_state.h"
#include "host_common.h"

using namespace pmdfc;

struct pmdfc_bloom {
  int dev = 0;
  uint64_t nbits = 0, nwords = 0;
  uint32_t k = 0;
  uint64_t* bm = nullptr;
};

// ------------------------------------------------------------------- bloom

int pmdfc_bloom_create(uint64_t nbits, uint32_t k, int device, pmdfc_bloom_t** out) {
  if (!out || nbits == 0 || k == 0 || k > 64 || nbits >= (1ULL << 32))
    return fail(PMDFC_ERR_ARG, "bloom: need 0 < nbits < 2^32 (unsigned int index, bloom_filter.c:87) and 0 < k <= 64");
  DevGuard g(device);
  auto* b = new pmdfc_bloom();
  b->dev = device;
  b->nbits = nbits;
  b->nwords = (nbits + 63) / 64;
  b->k = k;
  hipError_t e = hipMalloc(&b->bm, b->nwords * 8);
  if (e != hipSuccess) {
    delete b;
    return fail(PMDFC_ERR_NOMEM, "bloom hipMalloc", e);
  }
  e = hipMemset(b->bm, 0, b->nwords * 8);
  if (e != hipSuccess) {
    (void)hipFree(b->bm);
    delete b;
    return fail(PMDFC_ERR_HIP, "bloom memset", e);
  }
  *out = b;
  return PMDFC_OK;
}

int pmdfc_bloom_destroy(pmdfc_bloom_t* b) {
  if (!b) return PMDFC_OK;
  DevGuard g(b->dev);
  (void)hipDeviceSynchronize();
  (void)hipFree(b->bm);
  delete b;
  return PMDFC_OK;
}

int pmdfc_bloom_clear(pmdfc_bloom_t* b, void* stream) {
  if (!b) return fail(PMDFC_ERR_ARG, "null bloom");
  DevGuard g(b->dev);
  HIPCHK(hipMemsetAsync(b->bm, 0, b->nwords * 8, (hipStream_t)stream));
  return PMDFC_OK;
}

int pmdfc_bloom_add(pmdfc_bloom_t* b, const uint64_t* keys, uint64_t n, void* stream) {
  if (!b || (n && !keys)) return fail(PMDFC_ERR_ARG, "null argument");
  DevGuard g(b->dev);
  launch_bloom_add(b->bm, b->nbits, b->k, keys, n, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return PMDFC_OK;
}

int pmdfc_bloom_probe(pmdfc_bloom_t* b, const uint64_t* keys, uint8_t* out, uint64_t n, void* stream) {
  if (!b || (n && (!keys || !out))) return fail(PMDFC_ERR_ARG, "null argument");
  DevGuard g(b->dev);
  launch_bloom_probe(b->bm, b->nbits, b->k, keys, out, n, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return PMDFC_OK;
}

int pmdfc_bloom_bitmap(pmdfc_bloom_t* b, uint64_t** d_bitmap, uint64_t* nwords) {
  if (!b || !d_bitmap || !nwords) return fail(PMDFC_ERR_ARG, "null argument");
  *d_bitmap = b->bm;
  *nwords = b->nwords;
  return PMDFC_OK;
}

int pmdfc_bloom_set_bitmap_host(pmdfc_bloom_t* b, const uint64_t* host, uint64_t nwords) {
  if (!b || !host || nwords != b->nwords) return fail(PMDFC_ERR_ARG, "bitmap size mismatch");
  DevGuard g(b->dev);
  HIPCHK(hipMemcpy(b->bm, host, nwords * 8, hipMemcpyHostToDevice));
  return PMDFC_OK;
}

int pmdfc_bloom_get_bitmap_host(pmdfc_bloom_t* b, uint64_t* host, uint64_t nwords) {
  if (!b || !host || nwords != b->nwords) return fail(PMDFC_ERR_ARG, "bitmap size mismatch");
  DevGuard g(b->dev);
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(host, b->bm, nwords * 8, hipMemcpyDeviceToHost));
  return PMDFC_OK;
}

int pmdfc_bloom_probe_then_get(pmdfc_bloom_t* b, pmdfc_cceh_t* t, const uint64_t* keys,
                               uint64_t* vout, uint8_t* st, uint64_t n, void* stream) {
  if (!b || !t || (n && (!keys || !vout || !st))) return fail(PMDFC_ERR_ARG, "null argument");
  if (b->dev != t->dev) return fail(PMDFC_ERR_ARG, "bloom and index on different devices");
  std::lock_guard<std::mutex> lk(t->mu);
  DevGuard g(t->dev);
  hipStream_t s = (hipStream_t)stream;
  t->timing.begin(PMDFC_K_BLOOM, s);
  launch_bloom_get(b->bm, b->nbits, b->k, keys, vout, st, n, t->geo(), t->pairs, s);
  t->timing.end(s);
  HIPCHK(hipGetLastError());
  return PMDFC_OK;
}

// ----------------------------------------------------- counting bloom filter

int pmdfc_cbf_create(uint64_t nbits, uint32_t k, int device, pmdfc_cbf_t** out) {
  if (!out || nbits == 0 || nbits >= (1ULL << 31) || k == 0 || k > 64)
    return fail(PMDFC_ERR_ARG, "cbf: need 0 < nbits < 2^31 (int index, counting_bloom_filter.h:252) and 0 < k <= 64");
  DevGuard g(device);
  auto* f = new pmdfc_cbf();
  f->dev = device;
  f->nbits = nbits;
  f->nwords = (nbits + 63) / 64;
  f->padded = (nbits + kCbfChunk - 1) / kCbfChunk * kCbfChunk;
  f->k = k;
  hipError_t e = hipMalloc(&f->cnt, f->padded);
  if (e == hipSuccess) e = hipMalloc(&f->bm, f->nwords * 8);
  if (e == hipSuccess) e = hipMalloc(&f->flag, 256);
  if (e == hipSuccess) e = hipMemset(f->cnt, 0, f->padded);
  if (e == hipSuccess) e = hipMemset(f->bm, 0, f->nwords * 8);
  if (e != hipSuccess) {
    (void)hipFree(f->cnt);
    (void)hipFree(f->bm);
    (void)hipFree(f->flag);
    delete f;
    return fail(PMDFC_ERR_NOMEM, "cbf hipMalloc", e);
  }
  *out = f;
  return PMDFC_OK;
}

int pmdfc_cbf_destroy(pmdfc_cbf_t* f) {
  if (!f) return PMDFC_OK;
  DevGuard g(f->dev);
  (void)hipDeviceSynchronize();
  (void)hipFree(f->cnt);
  (void)hipFree(f->bm);
  (void)hipFree(f->flag);
  delete f;
  return PMDFC_OK;
}

int pmdfc_cbf_clear(pmdfc_cbf_t* f, void* stream) {
  if (!f) return fail(PMDFC_ERR_ARG, "null cbf");
  DevGuard g(f->dev);
  HIPCHK(hipMemsetAsync(f->cnt, 0, f->padded, (hipStream_t)stream));
  HIPCHK(hipMemsetAsync(f->bm, 0, f->nwords * 8, (hipStream_t)stream));
  return PMDFC_OK;
}

int pmdfc_cbf_insert(pmdfc_cbf_t* f, const uint64_t* keys, uint64_t n, void* stream) {
  if (!f || (n && !keys)) return fail(PMDFC_ERR_ARG, "null argument");
  DevGuard g(f->dev);
  launch_cbf_insert(f->cnt, f->nbits, f->k, keys, nullptr, n, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return PMDFC_OK;
}

int pmdfc_cbf_insert_ops(pmdfc_cbf_t* f, const uint8_t* ops, const uint64_t* keys, uint64_t n,
                         void* stream) {
  if (!f || (n && (!keys || !ops))) return fail(PMDFC_ERR_ARG, "null argument");
  DevGuard g(f->dev);
  launch_cbf_insert(f->cnt, f->nbits, f->k, keys, ops, n, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return PMDFC_OK;
}

int pmdfc_cbf_delete(pmdfc_cbf_t* f, const uint64_t* keys, uint8_t* deleted, uint64_t n,
                     void* stream) {
  if (!f || (n && (!keys || !deleted))) return fail(PMDFC_ERR_ARG, "null argument");
  DevGuard g(f->dev);
  launch_cbf_delete(f->cnt, f->nbits, f->k, keys, deleted, n, f->flag, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return PMDFC_OK;
}

int pmdfc_cbf_query(pmdfc_cbf_t* f, const uint64_t* keys, uint8_t* out, uint64_t n, void* stream) {
  if (!f || (n && (!keys || !out))) return fail(PMDFC_ERR_ARG, "null argument");
  DevGuard g(f->dev);
  launch_cbf_query(f->cnt, f->nbits, f->k, keys, out, n, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return PMDFC_OK;
}

int pmdfc_cbf_pack(pmdfc_cbf_t* f, void* stream) {
  if (!f) return fail(PMDFC_ERR_ARG, "null cbf");
  DevGuard g(f->dev);
  launch_cbf_pack(f->cnt, f->nbits, f->bm, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return PMDFC_OK;
}

int pmdfc_cbf_query_bits(pmdfc_cbf_t* f, const uint64_t* keys, uint8_t* out, uint64_t n,
                         void* stream) {
  if (!f || (n && (!keys || !out))) return fail(PMDFC_ERR_ARG, "null argument");
  DevGuard g(f->dev);
  launch_bloom_probe(f->bm, f->nbits, f->k, keys, out, n, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return PMDFC_OK;
}

int pmdfc_cbf_export(pmdfc_cbf_t* f, pmdfc_bloom_t* b, void* stream) {
  if (!f || !b) return fail(PMDFC_ERR_ARG, "null argument");
  if (b->nbits != f->nbits) return fail(PMDFC_ERR_ARG, "cbf and bloom differ in nbits");
  DevGuard g(f->dev);
  HIPCHK(hipMemcpyAsync(b->bm, f->bm, f->nwords * 8, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return PMDFC_OK;
}

int pmdfc_cbf_counters(pmdfc_cbf_t* f, uint8_t** d_counters, uint64_t** d_bitmap, uint64_t* nwords) {
  if (!f || !d_counters || !d_bitmap || !nwords) return fail(PMDFC_ERR_ARG, "null argument");
  *d_counters = f->cnt;
  *d_bitmap = f->bm;
  *nwords = f->nwords;
  return PMDFC_OK;
}

int pmdfc_cbf_get_counters_host(pmdfc_cbf_t* f, uint8_t* host, uint64_t nbits) {
  if (!f || !host || nbits != f->nbits) return fail(PMDFC_ERR_ARG, "counter size mismatch");
  DevGuard g(f->dev);
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(host, f->cnt, nbits, hipMemcpyDeviceToHost));
  return PMDFC_OK;
}

int pmdfc_cbf_get_bitmap_host(pmdfc_cbf_t* f, uint64_t* host, uint64_t nwords) {
  if (!f || !host || nwords != f->nwords) return fail(PMDFC_ERR_ARG, "bitmap size mismatch");
  DevGuard g(f->dev);
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(host, f->bm, nwords * 8, hipMemcpyDeviceToHost));
  return PMDFC_OK;
}

int pmdfc_cbf_rebuild(pmdfc_cbf_t* f, pmdfc_cceh_t* t, uint32_t flags, uint64_t* d_stored, void* stream) {
  if (!f || !t) return fail(PMDFC_ERR_ARG, "null argument");
  if (f->dev != t->dev) return fail(PMDFC_ERR_ARG, "cbf and index on different devices");
  if (flags & ~PMDFC_CBF_KEEP) return fail(PMDFC_ERR_ARG, "cbf_rebuild: unknown flags");
  std::lock_guard<std::mutex> lk(t->mu);
  DevGuard g(t->dev);
  hipStream_t s = (hipStream_t)stream;
  if (!(flags & PMDFC_CBF_KEEP)) {
    HIPCHK(hipMemsetAsync(f->cnt, 0, f->padded, s));
    HIPCHK(hipMemsetAsync(f->bm, 0, f->nwords * 8, s));
  }
  if (d_stored) HIPCHK(hipMemsetAsync(d_stored, 0, sizeof(uint64_t), s));
  launch_cbf_scan(false, t->pairs, t->ctl, t->max_segs, f->cnt, f->nbits, f->k,
                  reinterpret_cast<unsigned long long*>(d_stored), s);
  HIPCHK(hipGetLastError());
  return PMDFC_OK;
}

int pmdfc_cbf_audit(pmdfc_cbf_t* f, pmdfc_cceh_t* t, uint64_t* d_out2, void* stream) {
  if (!f || !t || !d_out2) return fail(PMDFC_ERR_ARG, "null argument");
  if (f->dev != t->dev) return fail(PMDFC_ERR_ARG, "cbf and index on different devices");
  std::lock_guard<std::mutex> lk(t->mu);
  DevGuard g(t->dev);
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipMemsetAsync(d_out2, 0, 2 * sizeof(uint64_t), s));
  launch_cbf_scan(true, t->pairs, t->ctl, t->max_segs, f->cnt, f->nbits, f->k,
                  reinterpret_cast<unsigned long long*>(d_out2), s);
  HIPCHK(hipGetLastError());
  return PMDFC_OK;
}
