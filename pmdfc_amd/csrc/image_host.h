// image_host.h -- what image_host.hip shares with compact_host.hip: canonical
// order with live counts on the device, and the restore of a table from local
// depths and segment images in canonical order.  Host only; both expect t->mu
// held and the table's device current.
#pragma once
#include <vector>

#include "engine_state.h"
#include "host_common.h"
#include "image.h"

namespace pmdfc {

// the device scratch of launch_image_live_scan for nseg segments, and a word
// for what a pack counts
struct LiveWork {
  DevTmp mem;
  LiveScan w{};
  uint32_t* bad = nullptr;
  int alloc(uint32_t nseg) {
    const uint64_t nblk = live_scan_blocks(nseg);
    HIPCHK(hipMalloc(&mem.p, (nseg + 2 * nblk + 1) * sizeof(uint64_t) + ((uint64_t)nseg + 1) * sizeof(uint32_t)));
    w.base = static_cast<uint64_t*>(mem.p);
    w.sums = w.base + nseg;
    w.offs = w.sums + nblk;
    w.cnt = reinterpret_cast<uint32_t*>(w.offs + nblk + 1);
    bad = w.cnt + nseg;
    return PMDFC_OK;
  }
  // (after launch_image_live_scan on s) the grand total, read back
  int total(uint32_t nseg, hipStream_t s, uint64_t* out) {
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, w.offs + live_scan_blocks(nseg), sizeof *out, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return PMDFC_OK;
  }
};

// Canonical order on the device for one synchronous call: order[i] the
// directory entry of canonical segment i, ld[i] its local depth, and from the
// engine's occupancy words base[i], the entries stored before segment i, and
// their total.
struct Canon {
  DevTmp wk, ord;
  LiveWork lw;
  uint32_t nseg = 0;
  uint32_t* order = nullptr;
  uint8_t* ld = nullptr;
  uint64_t live = 0;
};
int canonical_live(pmdfc_cceh* t, hipStream_t s, Canon& c);

// The part of a restore that every image kind shares, from a header and local
// depths that validation accepted and nseg <= max_segments: the directory's
// fit (still the table untouched), then the table becomes the image's.  `a`
// arrives with the image's own fields set (img; for a packed image occ_img,
// base, live; for a compacted working image src).
int restore_table(pmdfc_cceh* t, hipStream_t s, const image::Header& h, const std::vector<uint8_t>& ld, ScatterArgs a);

}  // namespace pmdfc
