#!/usr/bin/env python3
"""Time the rebuild of the counting bloom filter from the table.

Builds the config-2 table of bench.py (CCEH_hybrid(65536), 64M unique uniform
keys in 1M-key batches: ~131k segments, 2.15 GB of pairs) and a filter of
m = 1e9 counters, k = 4 (client/rdpma.h:33-35), and measures in one process,
by HIP events on the calls' stream:
  * pmdfc_cbf_rebuild (clear + the scan over the stored keys) and
    pmdfc_cbf_audit;
  * the yardsticks: pmdfc_cbf_clear + pmdfc_cbf_insert over the same 64M keys
    held dense in HBM (what the rebuild would cost if the keys needed no
    finding), and a device-to-device copy of the table's bytes (twice the
    scan's traffic: the scan only reads them).
Every timing is min / median / max over --reps runs, the ratios are of the
medians.  The rebuilt counters are compared with the dense insert's (the key
stream is duplicate-free; equal unless a split dropped an entry).  Prints one
JSON line.  Not part of bench.py; DESIGN.md 4.4 quotes a run.

    python tools/filter_rebuild_bench.py [--keys N] [--batch B] [--init-cap C] [--bits M] [--hashes K] [--reps R]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pmdfc_amd as P  # noqa: E402
from image_bench import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=1 << 26)
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--init-cap", type=int, default=65536)
    ap.add_argument("--bits", type=int, default=1000000000)
    ap.add_argument("--hashes", type=int, default=4)
    ap.add_argument("--reps", type=int, default=15)
    a = ap.parse_args()
    B, NK = a.batch, a.keys
    nb = NK // B
    depth = P.depth_for_hybrid(a.init_cap)
    idx = P.CCEH(depth=depth, max_batch=B, max_segments=int(NK / 512 * 1.25) + (1 << depth) + 1024)
    allk = torch.cat([P.gen_keys(1000, i * B, B) for i in range(nb)])
    idx.InsertBatches(allk, allk, [i * B for i in range(nb + 1)])
    s = idx.stats()
    f = P.CountingBloomFilter(a.hashes, a.bits)
    L = P.load_library()
    stream = f._d.stream
    out = torch.zeros(2, dtype=torch.int64, device="cuda")

    def rebuild():
        rc = L.pmdfc_cbf_rebuild(f._h, idx.handle, 0, out.data_ptr(), stream())
        assert rc == 0, rc

    def audit():
        rc = L.pmdfc_cbf_audit(f._h, idx.handle, out.data_ptr(), stream())
        assert rc == 0, rc

    def dense():
        f.Clear()
        f.Insert(allk)

    dense()  # warm-up
    _, dense_ev = timed(dense, a.reps)
    _, clear_ev = timed(f.Clear, a.reps)  # (part of both: the rebuild clears too)
    dense()
    dense_counters = f.counters()
    dense_sum = int(dense_counters.sum(dtype="int64"))
    rebuild()  # warm-up
    _, rebuild_ev = timed(rebuild, a.reps)
    stored = int(out[0].item())
    same = bool((f.counters() == dense_counters).all())
    _, audit_ev = timed(audit, a.reps)
    audit_out = [int(x) for x in out.tolist()]
    nbytes = s["segments"] * 1024 * 16
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    _, copy_ev = timed(lambda: dst.copy_(src), a.reps)
    res = {
        "keys": NK, "segments": s["segments"], "table_bytes": nbytes, "split_loss": s["split_loss"],
        "bits": a.bits, "hashes": a.hashes, "reps": a.reps,
        "stored": stored, "audit": audit_out, "counter_sum": dense_sum,
        "rebuild_ms": rebuild_ev, "audit_ms": audit_ev, "dense_insert_ms": dense_ev, "clear_ms": clear_ev,
        "d2d_copy_ms": copy_ev,
        "rebuild_vs_dense_insert": round(rebuild_ev["median"] / dense_ev["median"], 3),
        "rebuild_vs_copy": round(rebuild_ev["median"] / copy_ev["median"], 3),
        "rebuilt_equals_dense": same,
        "device": torch.cuda.get_device_name(0),
    }
    print(json.dumps(res))


if __name__ == "__main__":
    main()
