// extent_host.hip -- host side of the extent Insert / Get (kernels:
// extent.hip): expand the extents on the device, then the table's own
// do_insert / do_get on the expanded entries (engine_state.h).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "engine_state.h"
#include "host_common.h"

using namespace pmdfc;

// ------------------------------------------------------------------ extents

int pmdfc_cceh_insert_extent(pmdfc_cceh_t* t, int convention, const uint64_t* keys,
                             const uint64_t* cl, const uint64_t* lens, const uint64_t* vals, uint64_t n,
                             uint64_t* n_entries, void* stream) {
  if (!t || (n && (!keys || !lens || !vals)) || (convention != 0 && convention != 1))
    return fail(PMDFC_ERR_ARG, "bad argument");
  if (n_entries) *n_entries = 0;
  if (n == 0) return PMDFC_OK;
  const bool src = convention == 1;
  hipStream_t s = (hipStream_t)stream;
  uint64_t total = 0;
  DevGuard g(t->dev);
  StreamTmp t_cnt, t_cum, t_ok, t_ov, t_st;  // (freed on s, under g, on every return)
  HIPCHK(t_cnt.alloc(n * 8, s));
  HIPCHK(t_cum.alloc(n * 8, s));
  uint64_t *cnt = t_cnt.as<uint64_t>(), *cum = t_cum.as<uint64_t>();
  HIPCHK(launch_extent_count(src, keys, cl, lens, n, cnt, cum, s));
  HIPCHK(hipMemcpyAsync(&total, cum + n - 1, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  HIPCHK(t_ok.alloc(total * 8, s));
  HIPCHK(t_ov.alloc(total * 8, s));
  HIPCHK(t_st.alloc(std::min<uint64_t>(total, t->max_batch), s));
  uint64_t *ok = t_ok.as<uint64_t>(), *ov = t_ov.as<uint64_t>();
  uint8_t* st = t_st.as<uint8_t>();
  launch_extent_expand(src, keys, cl, lens, vals, n, cum, ok, ov, s);
  HIPCHK(hipGetLastError());
  int rc = PMDFC_OK;
  for (uint64_t off = 0; off < total && rc == PMDFC_OK; off += t->max_batch)
    rc = do_insert(t, ok + off, ov + off, 1, st, std::min<uint64_t>(t->max_batch, total - off), s);
  if (n_entries) *n_entries = total;
  return rc;
}

int pmdfc_cceh_get_extent(pmdfc_cceh_t* t, int convention, const uint64_t* keys, const uint64_t* cl,
                          uint64_t* vout, uint8_t* st, uint64_t n, void* stream) {
  if (!t || (n && (!keys || !vout || !st)) || (convention != 0 && convention != 1))
    return fail(PMDFC_ERR_ARG, "bad argument");
  if (n == 0) return PMDFC_OK;
  const uint32_t per = extent_targets_per_key(convention == 1);
  hipStream_t s = (hipStream_t)stream;
  DevGuard g(t->dev);
  StreamTmp t_tk, t_tv, t_ts;  // (freed on s, under g, on every return)
  HIPCHK(t_tk.alloc(n * per * 8, s));
  HIPCHK(t_tv.alloc(n * per * 8, s));
  HIPCHK(t_ts.alloc(n * per, s));
  uint64_t *tk = t_tk.as<uint64_t>(), *tv = t_tv.as<uint64_t>();
  uint8_t* ts = t_ts.as<uint8_t>();
  launch_extent_targets(keys, cl, n, per, tk, s);
  HIPCHK(hipGetLastError());
  int rc = do_get(t, tk, tv, ts, n * per, stream);
  if (rc == PMDFC_OK) {
    launch_extent_pick(tv, ts, n, per, vout, st, s);
    HIPCHK(hipGetLastError());
  }
  return rc;
}
