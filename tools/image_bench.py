#!/usr/bin/env python3
"""Time snapshot / restore of the table image against a plain device copy.

Builds the config-2 table of bench.py (CCEH_hybrid(65536), 64M unique uniform
keys in 1M-key batches: ~131k segments, an image of ~2.1 GB) and measures, in
one process:
  * pmdfc_cceh_snapshot into a device buffer and pmdfc_cceh_restore from it.
    Both calls are synchronous, so each is timed twice: wall clock around the
    call (with the sizing copies, the host-side validation and the directory
    plan) and HIP events on the call's stream around it (the same interval as
    the device sees it);
  * a device-to-device copy of the same byte count (torch's copy_, a
    hipMemcpyAsync), by HIP events: the yardstick -- each pass moves the same
    bytes once in and once out;
  * dump() (one blocking copy per segment) and the rebuild by re-inserting
    every key, by wall clock: what the image replaces.
Every timing is given as min / median / max over --reps runs (the ratios: of the
medians).  Prints one JSON line.  Not part of bench.py; DESIGN.md 4.7 quotes a run.

    python tools/image_bench.py [--keys N] [--batch B] [--init-cap C] [--reps R] [--no-dump]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pmdfc_amd as P  # noqa: E402
from pmdfc_amd import image as I  # noqa: E402


def spread(xs):
    xs = sorted(xs)
    return {"min": round(xs[0], 3), "median": round(xs[len(xs) // 2], 3), "max": round(xs[-1], 3)}


def timed(fn, reps):
    """reps runs of fn() on the current stream: (spread of wall ms, spread of event ms)."""
    wall, ev = [], []
    for _ in range(reps):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(a.elapsed_time(b))
    return spread(wall), spread(ev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=1 << 26)
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--init-cap", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--no-dump", action="store_true", help="skip the timing of dump()")
    a = ap.parse_args()
    B, NK = a.batch, a.keys
    nb = NK // B
    depth = P.depth_for_hybrid(a.init_cap)
    idx = P.CCEH(depth=depth, max_batch=B, max_segments=int(NK / 512 * 1.25) + (1 << depth) + 1024)
    allk = torch.cat([P.gen_keys(1000, i * B, B) for i in range(nb)])
    bounds = [i * B for i in range(nb + 1)]

    def rebuild():
        idx.reset()
        idx.InsertBatches(allk, allk, bounds)

    rebuild()  # warm-up
    rebuild_ms, _ = timed(rebuild, 5)
    img = idx.snapshot()
    nbytes = img.numel()
    hdr = img[:I.HEADER_BYTES].cpu().numpy()
    nseg = int(hdr[40:48].view("<u8")[0])
    live = int(hdr[48:56].view("<u8")[0])

    def do_snapshot():
        return idx.snapshot()

    snap_wall, snap_ev = timed(do_snapshot, a.reps)
    rest_wall, rest_ev = timed(lambda: idx.restore(img), a.reps)
    same = bool(torch.equal(idx.snapshot(), img))  # the restored table snapshots to the same bytes
    dst = torch.empty_like(img)
    _, copy_ev = timed(lambda: dst.copy_(img), a.reps)
    res = {
        "keys": NK, "segments": nseg, "live_entries": live, "image_bytes": nbytes, "reps": a.reps,
        "snapshot_ms": snap_ev, "snapshot_wall_ms": snap_wall,
        "restore_ms": rest_ev, "restore_wall_ms": rest_wall,
        "d2d_copy_ms": copy_ev,
        "snapshot_vs_copy": round(snap_ev["median"] / copy_ev["median"], 2),
        "restore_vs_copy": round(rest_ev["median"] / copy_ev["median"], 2),
        "rebuild_by_insert_ms": rebuild_ms,
        "restored_snapshot_identical": same,
        "device": torch.cuda.get_device_name(0),
    }
    if not a.no_dump:
        t0 = time.perf_counter()
        idx.dump()
        res["dump_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
