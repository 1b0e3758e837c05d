// image_host.hip -- host side of the table images (kernels: image.hip): both
// snapshot formats, both restores and the entry export.  All synchronous,
// under the table's lock; what they call in the engine is listed in
// engine_state.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "engine_state.h"
#include "host_common.h"
#include "image.h"
#include "image_host.h"
#include "packed_image.h"

using namespace pmdfc;

// ---- table image (image.h, image.hip)

int pmdfc_cceh_snapshot(pmdfc_cceh_t* t, void* buf, uint64_t cap_bytes, uint64_t* bytes_out, void* stream) {
  if (!t || !bytes_out) return fail(PMDFC_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> lk(t->mu);
  DevGuard g(t->dev);
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipDeviceSynchronize());
  // canonical order: the segments of each bucket counted, the counts scanned
  const uint32_t nb = 1u << t->p1;
  DevTmp wk;
  HIPCHK(hipMalloc(&wk.p, (2ull * nb + 1) * sizeof(uint32_t)));
  uint32_t* cnt = static_cast<uint32_t*>(wk.p);
  uint32_t *base = cnt + nb, *total = base + nb;
  launch_image_count(t->hdr, t->pool, (uint32_t)t->pool_cap, t->p1, t->sbits, cnt, base, total, s);
  HIPCHK(hipGetLastError());
  uint32_t nseg = 0;
  HIPCHK(hipMemcpyAsync(&nseg, total, sizeof nseg, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (nseg == 0 || nseg > t->max_segs) return fail(PMDFC_ERR_STATE, "snapshot: the directory walk found no sound table");
  const uint64_t need = image::total_bytes(nseg);
  *bytes_out = need;
  if (!buf || cap_bytes < need) return fail(PMDFC_ERR_SIZE, "snapshot: the buffer is smaller than the image");
  if ((uintptr_t)buf & 15u) return fail(PMDFC_ERR_ARG, "snapshot: the buffer must be 16-byte aligned");
  uint8_t* out = static_cast<uint8_t*>(buf);
  DevTmp ord;
  HIPCHK(hipMalloc(&ord.p, (uint64_t)nseg * sizeof(uint32_t)));
  uint32_t* order = static_cast<uint32_t*>(ord.p);
  const uint64_t dbytes = image::depth_bytes(nseg);
  HIPCHK(hipMemsetAsync(out + image::kHeaderBytes, 0, dbytes, s));
  launch_image_emit(t->hdr, t->pool, (uint32_t)t->pool_cap, t->p1, t->sbits, base, nseg, order,
                    out + image::kHeaderBytes, s);
  launch_image_gather(t->pairs, order, nseg, (uint32_t)t->max_segs,
                      reinterpret_cast<ulonglong2*>(out + image::pairs_offset(nseg)), s);
  HIPCHK(hipGetLastError());
  // the live entries from the occupancy words, as Utilization counts them
  if (int rc = read_ctl(t, s)) return rc;
  const uint64_t nsegs = std::min<uint64_t>(t->hctl->nsegs, t->max_segs);
  HIPCHK(hipMemsetAsync(t->popc, 0, sizeof(unsigned long long), s));
  launch_popcount(t->occ, nsegs * 32, t->popc, s);
  unsigned long long live = 0;
  std::vector<uint8_t> ld(dbytes);
  HIPCHK(hipMemcpyAsync(&live, t->popc, sizeof live, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(ld.data(), out + image::kHeaderBytes, dbytes, hipMemcpyDefault, s));
  HIPCHK(hipStreamSynchronize(s));
  image::Header h;
  h.initial_depth = t->D0;
  h.shard_bits = t->sbits;
  h.shard_id = t->shard;
  h.nseg = nseg;
  h.live = live;
  h.total_bytes = need;
  h.min_ld = *std::min_element(ld.begin(), ld.begin() + nseg);
  h.max_ld = *std::max_element(ld.begin(), ld.begin() + nseg);
  h.depth = std::max(t->D0, h.max_ld);
  // (what this call wrote must be what pmdfc_cceh_restore accepts)
  if (int e = image::validate_depths(h, ld.data())) return fail(PMDFC_ERR_STATE, image::error_string(e));
  std::vector<uint8_t> hb(image::kHeaderBytes);
  image::encode_header(h, hb.data());
  HIPCHK(hipMemcpy(out, hb.data(), hb.size(), hipMemcpyDefault));
  return PMDFC_OK;
}

// (image_host.h)
int pmdfc::restore_table(pmdfc_cceh* t, hipStream_t s, const image::Header& h, const std::vector<uint8_t>& ld,
                         ScatterArgs a) {
  const uint32_t nseg = (uint32_t)h.nseg;
  // the directory: the bucket bits rebucket_now would have reached, each
  // bucket's sub-directory as deep as its deepest segment, in its fixed slot
  // or past the reserved region (the rule of k_init_segments and the growth paths)
  const uint32_t p1 = std::min<uint32_t>(t->p1max, h.min_ld - t->sbits);
  const uint32_t top = kMaxDepth - t->sbits;
  std::vector<uint2> desc(nseg);
  std::vector<uint8_t> maxl(1u << p1, 0);
  ImageCtl c{};
  {
    uint32_t pos = 0;  // in units of 2^-30 of the whole hash space
    for (uint32_t i = 0; i < nseg; ++i) {
      const uint32_t L = ld[i];
      const uint32_t w = p1 ? pos >> (top - p1) : 0u;
      maxl[w] = std::max<uint8_t>(maxl[w], (uint8_t)L);
      desc[i] = make_uint2(pos, L);
      c.depth_count[L] += 1;
      pos += 1u << (kMaxDepth - L);
    }
  }
  std::vector<uint64_t> hd(1u << p1);
  const uint64_t region = (uint64_t)kFixedSlot << t->p1max;
  uint64_t cur = region;
  for (uint32_t w = 0; w < hd.size(); ++w) {
    const uint32_t db = maxl[w] - t->sbits - p1;
    if (p1 == t->p1max && db <= kFixedBits) {
      hd[w] = hdr_make(w * kFixedSlot, db);
    } else {
      if (cur + (1ULL << db) > t->pool_cap) return fail(PMDFC_ERR_SIZE, "restore: the sub-directories do not fit the pool");
      hd[w] = hdr_make((uint32_t)cur, db);
      cur += 1ULL << db;
    }
  }
  c.nsegs = nseg;
  c.pool_cur = (uint32_t)cur;
  c.max_ld = h.max_ld;
  DevTmp dv;  // the descriptors, then the prefix check's count
  HIPCHK(hipMalloc(&dv.p, (uint64_t)nseg * sizeof(uint2) + sizeof(uint32_t)));
  uint2* d_desc = static_cast<uint2*>(dv.p);
  uint32_t* d_bad = reinterpret_cast<uint32_t*>(d_desc + nseg);
  // ---- from here the table is the image's
  HIPCHK(hipMemcpy(d_desc, desc.data(), (uint64_t)nseg * sizeof(uint2), hipMemcpyHostToDevice));
  HIPCHK(hipMemset(d_bad, 0, sizeof(uint32_t)));
  HIPCHK(hipMemcpy(t->hdr, hd.data(), hd.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
  if (int rc = start_host_state(t, s, p1, h.min_ld)) return rc;
  launch_image_ctl(batch_words(t), t->ctl, c, t->d_hint, s);
  a.desc = d_desc;
  a.hdr = t->hdr;
  a.nseg = nseg;
  a.p1 = p1;
  a.sbits = t->sbits;
  a.shard = t->shard;
  a.pairs = t->pairs;
  a.occ = t->occ;
  a.ldep = t->ldep;
  a.pool = t->pool;
  a.bad = d_bad;
  launch_image_scatter(a, s);
  HIPCHK(hipGetLastError());
  uint32_t bad = 0;
  HIPCHK(hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (bad) {
    if (int rc = init_state(t, s)) return rc;
    HIPCHK(hipStreamSynchronize(s));
    return fail(PMDFC_ERR_ARG, "restore: live keys outside their segment's hash prefix (the table was reset)");
  }
  return PMDFC_OK;
}

// pmdfc_cceh_restore of a packed image (packed_image.h); hb: its header bytes
static int restore_packed(pmdfc_cceh_t* t, hipStream_t s, const uint8_t* in, uint64_t bytes,
                          const std::vector<uint8_t>& hb) {
  // ---- the table untouched: header, local depths, the occupancy words' count
  image::Header h;
  if (int e = packed::parse_header(hb.data(), bytes, &h)) return fail(PMDFC_ERR_ARG, packed::error_string(e));
  if (h.initial_depth != t->D0 || h.shard_bits != t->sbits || h.shard_id != t->shard)
    return fail(PMDFC_ERR_ARG, "restore: the image's initial_depth / shard_bits / shard_id are not this engine's");
  std::vector<uint8_t> ld(image::depth_bytes(h.nseg));
  HIPCHK(hipMemcpy(ld.data(), in + image::kHeaderBytes, ld.size(), hipMemcpyDefault));
  if (int e = image::validate_depths(h, ld.data())) return fail(PMDFC_ERR_ARG, packed::error_string(e));
  if (h.nseg > t->max_segs) return fail(PMDFC_ERR_SIZE, "restore: the image has more segments than max_segments");
  const uint32_t nseg = (uint32_t)h.nseg;
  // the two paddings the device pass never looks at (each under 4,096 bytes)
  const uint64_t occ_end = packed::occ_offset(nseg) + (uint64_t)nseg * packed::kOccWords * 4;
  const uint64_t pair_end = packed::pairs_offset(nseg) + h.live * 16;
  std::vector<uint8_t> pad((packed::pairs_offset(nseg) - occ_end) + (h.total_bytes - pair_end));
  if (packed::pairs_offset(nseg) > occ_end)
    HIPCHK(hipMemcpy(pad.data(), in + occ_end, packed::pairs_offset(nseg) - occ_end, hipMemcpyDefault));
  if (h.total_bytes > pair_end)
    HIPCHK(hipMemcpy(pad.data() + (packed::pairs_offset(nseg) - occ_end), in + pair_end, h.total_bytes - pair_end,
                     hipMemcpyDefault));
  for (uint8_t b : pad)
    if (b) return fail(PMDFC_ERR_ARG, packed::error_string(packed::kPadding));
  // every segment's offset into the pairs is a prefix sum of popcounts: they
  // must sum to the header's live count, which parse_header fitted to the buffer
  const uint32_t* occ_img = reinterpret_cast<const uint32_t*>(in + packed::occ_offset(nseg));
  LiveWork lw;
  if (int rc = lw.alloc(nseg)) return rc;
  launch_image_live_scan(occ_img, nullptr, 0, nseg, lw.w, s);
  uint64_t live = 0;
  if (int rc = lw.total(nseg, s, &live)) return rc;
  if (live != h.live) return fail(PMDFC_ERR_ARG, packed::error_string(packed::kLive));
  ScatterArgs a{};
  a.img = reinterpret_cast<const ulonglong2*>(in + packed::pairs_offset(nseg));
  a.occ_img = occ_img;
  a.base = lw.w.base;
  a.live = h.live;
  return restore_table(t, s, h, ld, a);
}

int pmdfc_cceh_restore(pmdfc_cceh_t* t, const void* buf, uint64_t bytes, void* stream) {
  if (!t || !buf) return fail(PMDFC_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> lk(t->mu);
  DevGuard g(t->dev);
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipDeviceSynchronize());
  if ((uintptr_t)buf & 15u) return fail(PMDFC_ERR_ARG, "restore: the image must be 16-byte aligned");
  if (bytes < image::kHeaderBytes) return fail(PMDFC_ERR_ARG, image::error_string(image::kShort));
  const uint8_t* in = static_cast<const uint8_t*>(buf);
  // ---- decided on the host, the table untouched: header, local depths, fit
  std::vector<uint8_t> hb(image::kHeaderBytes);
  HIPCHK(hipMemcpy(hb.data(), in, hb.size(), hipMemcpyDefault));
  if (memcmp(hb.data(), packed::kMagic, 8) == 0) return restore_packed(t, s, in, bytes, hb);
  image::Header h;
  if (int e = image::parse_header(hb.data(), bytes, &h)) return fail(PMDFC_ERR_ARG, image::error_string(e));
  if (h.initial_depth != t->D0 || h.shard_bits != t->sbits || h.shard_id != t->shard)
    return fail(PMDFC_ERR_ARG, "restore: the image's initial_depth / shard_bits / shard_id are not this engine's");
  std::vector<uint8_t> ld(image::depth_bytes(h.nseg));
  HIPCHK(hipMemcpy(ld.data(), in + image::kHeaderBytes, ld.size(), hipMemcpyDefault));
  if (int e = image::validate_depths(h, ld.data())) return fail(PMDFC_ERR_ARG, image::error_string(e));
  if (h.nseg > t->max_segs) return fail(PMDFC_ERR_SIZE, "restore: the image has more segments than max_segments");
  ScatterArgs a{};
  a.img = reinterpret_cast<const ulonglong2*>(in + image::pairs_offset(h.nseg));
  return restore_table(t, s, h, ld, a);
}

// ---- packed image and entry export (packed_image.h, image.hip)

// (image_host.h)
int pmdfc::canonical_live(pmdfc_cceh* t, hipStream_t s, Canon& c) {
  const uint32_t nb = 1u << t->p1;
  HIPCHK(hipMalloc(&c.wk.p, (2ull * nb + 1) * sizeof(uint32_t)));
  uint32_t* cnt = static_cast<uint32_t*>(c.wk.p);
  uint32_t *base = cnt + nb, *total = base + nb;
  launch_image_count(t->hdr, t->pool, (uint32_t)t->pool_cap, t->p1, t->sbits, cnt, base, total, s);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(&c.nseg, total, sizeof c.nseg, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (c.nseg == 0 || c.nseg > t->max_segs) return fail(PMDFC_ERR_STATE, "the directory walk found no sound table");
  HIPCHK(hipMalloc(&c.ord.p, (uint64_t)c.nseg * (sizeof(uint32_t) + 1)));
  c.order = static_cast<uint32_t*>(c.ord.p);
  c.ld = reinterpret_cast<uint8_t*>(c.order + c.nseg);
  launch_image_emit(t->hdr, t->pool, (uint32_t)t->pool_cap, t->p1, t->sbits, base, c.nseg, c.order, c.ld, s);
  if (int rc = c.lw.alloc(c.nseg)) return rc;
  HIPCHK(hipMemsetAsync(c.lw.bad, 0, sizeof(uint32_t), s));
  launch_image_live_scan(t->occ, c.order, (uint32_t)t->max_segs, c.nseg, c.lw.w, s);
  if (int rc = c.lw.total(c.nseg, s, &c.live)) return rc;
  if (c.live > (uint64_t)c.nseg * kSlots) return fail(PMDFC_ERR_STATE, "the occupancy words count more than the slots");
  return PMDFC_OK;
}

uint32_t pmdfc_cceh_packed_scan_block(void) { return kLiveScanBlock; }

int pmdfc_cceh_snapshot_packed(pmdfc_cceh_t* t, void* buf, uint64_t cap_bytes, uint64_t* bytes_out, void* stream) {
  if (!t || !bytes_out) return fail(PMDFC_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> lk(t->mu);
  DevGuard g(t->dev);
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipDeviceSynchronize());
  Canon c;
  if (int rc = canonical_live(t, s, c)) return rc;
  const uint32_t nseg = c.nseg;
  const uint64_t need = packed::total_bytes(nseg, c.live);
  *bytes_out = need;
  if (!buf || cap_bytes < need) return fail(PMDFC_ERR_SIZE, "snapshot_packed: the buffer is smaller than the image");
  if ((uintptr_t)buf & 15u) return fail(PMDFC_ERR_ARG, "snapshot_packed: the buffer must be 16-byte aligned");
  uint8_t* out = static_cast<uint8_t*>(buf);
  // the local depths, and the zero padding of the three regions
  const uint64_t dbytes = image::depth_bytes(nseg);
  const uint64_t occ_end = packed::occ_offset(nseg) + (uint64_t)nseg * packed::kOccWords * 4;
  const uint64_t pair_end = packed::pairs_offset(nseg) + c.live * 16;
  HIPCHK(hipMemsetAsync(out + image::kHeaderBytes, 0, dbytes, s));
  HIPCHK(hipMemcpyAsync(out + image::kHeaderBytes, c.ld, nseg, hipMemcpyDefault, s));
  if (packed::pairs_offset(nseg) > occ_end) HIPCHK(hipMemsetAsync(out + occ_end, 0, packed::pairs_offset(nseg) - occ_end, s));
  if (need > pair_end) HIPCHK(hipMemsetAsync(out + pair_end, 0, need - pair_end, s));
  PackArgs a{};
  a.pairs = t->pairs;
  a.order = c.order;
  a.max_segs = (uint32_t)t->max_segs;
  a.cnt = c.lw.w.cnt;
  a.base = c.lw.w.base;
  a.occ_out = reinterpret_cast<uint32_t*>(out + packed::occ_offset(nseg));
  a.pairs_out = reinterpret_cast<ulonglong2*>(out + packed::pairs_offset(nseg));
  a.bad = c.lw.bad;
  launch_image_pack(a, nseg, s);
  HIPCHK(hipGetLastError());
  uint32_t bad = 0;
  std::vector<uint8_t> ld(dbytes, 0);
  HIPCHK(hipMemcpyAsync(&bad, c.lw.bad, sizeof bad, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(ld.data(), c.ld, nseg, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (bad) return fail(PMDFC_ERR_STATE, "snapshot_packed: stored keys and occupancy words disagree");
  image::Header h;
  h.initial_depth = t->D0;
  h.shard_bits = t->sbits;
  h.shard_id = t->shard;
  h.nseg = nseg;
  h.live = c.live;
  h.total_bytes = need;
  h.min_ld = *std::min_element(ld.begin(), ld.begin() + nseg);
  h.max_ld = *std::max_element(ld.begin(), ld.begin() + nseg);
  h.depth = std::max(t->D0, h.max_ld);
  // (what this call wrote must be what pmdfc_cceh_restore accepts)
  if (int e = image::validate_depths(h, ld.data())) return fail(PMDFC_ERR_STATE, packed::error_string(e));
  std::vector<uint8_t> hb(image::kHeaderBytes);
  packed::encode_header(h, hb.data());
  HIPCHK(hipMemcpy(out, hb.data(), hb.size(), hipMemcpyDefault));
  return PMDFC_OK;
}

int pmdfc_cceh_export_entries(pmdfc_cceh_t* t, uint64_t* d_keys, uint64_t* d_values, uint64_t cap_entries,
                              uint64_t* n_out, void* stream) {
  if (!t || !n_out) return fail(PMDFC_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> lk(t->mu);
  DevGuard g(t->dev);
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipDeviceSynchronize());
  Canon c;
  if (int rc = canonical_live(t, s, c)) return rc;
  *n_out = c.live;
  if ((!d_keys && !d_values) || cap_entries < c.live)
    return fail(PMDFC_ERR_SIZE, "export_entries: the arrays are smaller than the stored entries");
  PackArgs a{};
  a.pairs = t->pairs;
  a.order = c.order;
  a.max_segs = (uint32_t)t->max_segs;
  a.cnt = c.lw.w.cnt;
  a.base = c.lw.w.base;
  a.keys_out = d_keys;
  a.vals_out = d_values;
  a.bad = c.lw.bad;
  launch_image_pack(a, c.nseg, s);
  HIPCHK(hipGetLastError());
  uint32_t bad = 0;
  HIPCHK(hipMemcpyAsync(&bad, c.lw.bad, sizeof bad, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (bad) return fail(PMDFC_ERR_STATE, "export_entries: stored keys and occupancy words disagree");
  return PMDFC_OK;
}
