// compact_host.hip -- host side of pmdfc_cceh_compact (kernel: compact.hip;
// DESIGN.md 4.9).  Synchronous, under the table's lock.  Three steps: the
// canonical image gathered on the device (image.hip), the rounds of sibling
// merges inside it, and -- only if a pair merged -- the restore of the table
// from the surviving segments (image_host.hip restore_table).  Until that
// last step the table is not touched.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <new>
#include <vector>

#include "engine_state.h"
#include "host_common.h"
#include "image.h"
#include "image_host.h"

using namespace pmdfc;

namespace {
// HIP events on the call's stream, one per step boundary (pmdfc_cceh_compact_timing)
struct Marks {
  std::vector<hipEvent_t> ev;
  void mark(hipStream_t s) {
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return;
    (void)hipEventRecord(e, s);
    ev.push_back(e);
  }
  // the milliseconds from mark k to mark k + 1 (the caller has synchronised the stream)
  float ms(size_t k) const {
    float t = 0;
    if (k + 1 < ev.size()) (void)hipEventElapsedTime(&t, ev[k], ev[k + 1]);
    return t;
  }
  ~Marks() {
    for (auto e : ev) (void)hipEventDestroy(e);
  }
};
}  // namespace

int pmdfc_cceh_compact(pmdfc_cceh_t* t, uint32_t fill_limit, pmdfc_compact_result_t* out, void* stream) {
  if (!t || !out) return fail(PMDFC_ERR_ARG, "null argument");
  if (fill_limit > kSlots) return fail(PMDFC_ERR_ARG, "compact: fill_limit above 1024");
  if (fill_limit == 0) fill_limit = 512;
  std::lock_guard<std::mutex> lk(t->mu);
  DevGuard g(t->dev);
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipDeviceSynchronize());
  *out = pmdfc_compact_result_t{};
  t->compact_ms.clear();
  Marks mk;
  mk.mark(s);
  Canon c;
  if (int rc = canonical_live(t, s, c)) return rc;
  const uint32_t nseg = c.nseg;
  // ---- the rows, on the host first: depths, starts, live counts
  std::vector<uint8_t> ld8(nseg);
  std::vector<uint32_t> cnt(nseg);
  HIPCHK(hipMemcpyAsync(ld8.data(), c.ld, nseg, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(cnt.data(), c.lw.w.cnt, (uint64_t)nseg * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  // rows[0] ld, [1] pos, [2] next, [3] refused, then the round's merge count
  std::vector<uint32_t> rows;
  try {
    rows.assign(4ull * nseg + 1, 0u);
  } catch (const std::bad_alloc&) {
    return fail(PMDFC_ERR_NOMEM, "compact: out of host memory");
  }
  uint32_t *h_ld = rows.data(), *h_pos = h_ld + nseg, *h_next = h_pos + nseg, *h_ref = h_next + nseg;
  uint32_t max_ld = 0;
  bool any = false;  // a sibling pair within the limit: without one, no round can merge
  {
    uint64_t pos = 0;
    for (uint32_t i = 0; i < nseg; ++i) {
      const uint32_t L = ld8[i];
      if (L < t->D0 || L < 1 || L > kMaxDepth || pos >> kMaxDepth)
        return fail(PMDFC_ERR_STATE, "compact: the directory walk found no sound table");
      h_ld[i] = L;
      h_pos[i] = (uint32_t)pos;
      h_next[i] = i + 1;
      max_ld = std::max(max_ld, L);
      if (i && ld8[i - 1] == L && L > t->D0 && (h_pos[i - 1] & ((2u << (kMaxDepth - L)) - 1u)) == 0 &&
          cnt[i - 1] + cnt[i] <= fill_limit)
        any = true;
      pos += 1ull << (kMaxDepth - L);
    }
  }
  out->segments_before = out->segments_after = nseg;
  out->depth_before = out->depth_after = std::max(t->D0, max_ld);
  if (!any) return PMDFC_OK;
  // ---- the working image and the rows on the device
  DevTmp img, dr;
  const uint64_t row_bytes = (4ull * nseg + 1) * sizeof(uint32_t);
  if (hipMalloc(&img.p, (uint64_t)nseg * image::kSegmentBytes) != hipSuccess || hipMalloc(&dr.p, row_bytes) != hipSuccess) {
    (void)hipGetLastError();
    return fail(PMDFC_ERR_NOMEM, "compact: no device memory for the working image");
  }
  mk.mark(s);  // [0, 1): canonical order, live counts, the host's look at them, the allocations
  launch_image_gather(t->pairs, c.order, nseg, (uint32_t)t->max_segs, static_cast<ulonglong2*>(img.p), s);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(dr.p, rows.data(), row_bytes, hipMemcpyHostToDevice, s));
  mk.mark(s);  // [1, 2): the gather
  CompactArgs a{};
  a.img = static_cast<ulonglong2*>(img.p);
  a.ld = static_cast<uint32_t*>(dr.p);
  a.pos = a.ld + nseg;
  a.next = a.ld + 2ull * nseg;
  a.refused = a.ld + 3ull * nseg;
  a.merged = a.ld + 4ull * nseg;
  a.cnt = c.lw.w.cnt;
  a.nseg = nseg;
  a.d0 = t->D0;
  a.fill_limit = fill_limit;
  // ---- the rounds: each merges the pairs the image showed when it began
  uint64_t merges = 0;
  uint32_t rounds = 0;
  for (uint32_t r = 1; r <= kMaxDepth + 1; ++r) {
    uint32_t m = 0;
    a.round = r;
    HIPCHK(hipMemsetAsync(a.merged, 0, sizeof(uint32_t), s));
    launch_compact_merge(a, s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&m, a.merged, sizeof m, hipMemcpyDeviceToHost, s));
    mk.mark(s);  // [1 + r, 2 + r): round r, the last of them the one that merged nothing
    HIPCHK(hipStreamSynchronize(s));
    if (!m) break;
    merges += m;
    rounds += 1;
  }
  HIPCHK(hipMemcpyAsync(rows.data(), dr.p, row_bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  for (uint32_t i = 0; i < nseg; ++i) out->refused += h_ref[i] ? 1 : 0;
  out->merges = merges;
  out->rounds = rounds;
  const size_t nround = mk.ev.size() - 3;
  auto timing = [&](float restore_ms) {  // (pmdfc_cceh_compact_timing's order)
    t->compact_ms = {mk.ms(0), mk.ms(1), restore_ms};
    for (size_t r = 0; r < nround; ++r) t->compact_ms.push_back(mk.ms(2 + r));
  };
  if (!merges) {
    timing(0.f);
    return PMDFC_OK;
  }
  // ---- the survivors in canonical order, validated as an image's depths are
  std::vector<uint32_t> src;
  src.reserve(nseg - merges);
  for (uint32_t i = 0; i < nseg; ++i)
    if ((h_ld[i] & 0xFFu) != kCompactDead) src.push_back(i);
  if (src.size() != nseg - merges) return fail(PMDFC_ERR_STATE, "compact: the rows and the merge count disagree");
  image::Header h;
  h.initial_depth = t->D0;
  h.shard_bits = t->sbits;
  h.shard_id = t->shard;
  h.nseg = src.size();
  h.total_bytes = image::total_bytes(h.nseg);
  std::vector<uint8_t> ld(image::depth_bytes(h.nseg), 0);
  for (size_t k = 0; k < src.size(); ++k) ld[k] = (uint8_t)(h_ld[src[k]] & 0xFFu);
  h.min_ld = *std::min_element(ld.begin(), ld.begin() + h.nseg);
  h.max_ld = *std::max_element(ld.begin(), ld.begin() + h.nseg);
  h.depth = std::max(t->D0, h.max_ld);
  if (int e = image::validate_depths(h, ld.data())) return fail(PMDFC_ERR_STATE, image::error_string(e));
  DevTmp ds;
  if (hipMalloc(&ds.p, src.size() * sizeof(uint32_t)) != hipSuccess) {
    (void)hipGetLastError();
    return fail(PMDFC_ERR_NOMEM, "compact: no device memory for the survivor list");
  }
  HIPCHK(hipMemcpy(ds.p, src.data(), src.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  ScatterArgs sa{};
  sa.img = a.img;
  sa.src = static_cast<const uint32_t*>(ds.p);
  if (int rc = restore_table(t, s, h, ld, sa)) return rc;
  mk.mark(s);  // the last: the rows read back, the survivors listed, the restore
  HIPCHK(hipStreamSynchronize(s));
  timing(mk.ms(2 + nround));
  out->segments_after = h.nseg;
  out->depth_after = h.depth;
  return PMDFC_OK;
}

int pmdfc_cceh_compact_timing(pmdfc_cceh_t* t, float* ms, uint32_t cap, uint32_t* n_out) {
  if (!t || !n_out) return fail(PMDFC_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> lk(t->mu);
  *n_out = (uint32_t)t->compact_ms.size();
  if (!ms || cap < *n_out) return fail(PMDFC_ERR_SIZE, "compact_timing: the array is smaller than the steps");
  std::copy(t->compact_ms.begin(), t->compact_ms.end(), ms);
  return PMDFC_OK;
}
