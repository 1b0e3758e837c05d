#!/usr/bin/env python3
"""Time the packed table image against the version-1 image of the same table.

Builds the config-2 table of bench.py as tools/image_bench.py does
(CCEH_hybrid(65536), 64M unique uniform keys in 1M-key batches: ~131k segments
at half load) and measures, in one process:
  * device to device, by HIP events on the call's stream and by wall clock:
    snapshot() and restore() of the version-1 image, snapshot(packed=True) and
    restore() of the packed image, and a device copy of each byte count.  The
    margin for "not slower" is the min-to-max spread of the version-1 timings;
  * items() (pmdfc_cceh_export_entries) the same way, beside dump() by wall
    clock;
  * through the front-end, by wall clock: KV.save / KV.save(packed=True) and
    KV.load of each kind of file, the files in --dir (/dev/shm: the disk is
    not the subject), with the file sizes.
Every timing is min / median / max over --reps runs (--file-reps for the
front-end).  Prints one JSON line.  Not part of bench.py; DESIGN.md 4.7 quotes
a run.

    python tools/packed_image_bench.py [--keys N] [--batch B] [--init-cap C] [--reps R] [--file-reps F]
                                       [--dir D] [--no-dump] [--no-files]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pmdfc_amd as P  # noqa: E402
from pmdfc_amd import image as I  # noqa: E402
from pmdfc_amd.kv import KV  # noqa: E402
from image_bench import spread, timed  # noqa: E402


def wall(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return spread(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=1 << 26)
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--init-cap", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--file-reps", type=int, default=5)
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--no-dump", action="store_true", help="skip the timing of dump()")
    ap.add_argument("--no-files", action="store_true", help="skip the front-end's Save / Load")
    a = ap.parse_args()
    B, NK = a.batch, a.keys
    nb = NK // B
    depth = P.depth_for_hybrid(a.init_cap)
    max_segs = int(NK / 512 * 1.25) + (1 << depth) + 1024
    idx = P.CCEH(depth=depth, max_batch=B, max_segments=max_segs)
    allk = torch.cat([P.gen_keys(1000, i * B, B) for i in range(nb)])
    idx.InsertBatches(allk, allk, [i * B for i in range(nb + 1)])
    del allk
    img = idx.snapshot()
    pak = idx.snapshot(packed=True)
    hdr = pak[:I.HEADER_BYTES].cpu().numpy()
    nseg = int(hdr[40:48].view("<u8")[0])
    live = int(hdr[48:56].view("<u8")[0])
    assert pak.numel() == I.packed_total_bytes(nseg, live)

    res = {"keys": NK, "segments": nseg, "live_entries": live, "load_factor": round(live / (nseg * 1024), 4),
           "image_bytes": img.numel(), "packed_bytes": pak.numel(),
           "packed_vs_image_bytes": round(pak.numel() / img.numel(), 4), "reps": a.reps,
           "device": torch.cuda.get_device_name(0)}
    # device to device, the two kinds interleaved in one process
    w, e = timed(lambda: idx.snapshot(), a.reps)
    res["snapshot_ms"], res["snapshot_wall_ms"] = e, w
    w, e = timed(lambda: idx.snapshot(packed=True), a.reps)
    res["snapshot_packed_ms"], res["snapshot_packed_wall_ms"] = e, w
    w, e = timed(lambda: idx.restore(img), a.reps)
    res["restore_ms"], res["restore_wall_ms"] = e, w
    w, e = timed(lambda: idx.restore(pak), a.reps)
    res["restore_packed_ms"], res["restore_packed_wall_ms"] = e, w
    res["round_trip_identical"] = bool(torch.equal(idx.snapshot(), img) and torch.equal(idx.snapshot(packed=True), pak))
    for name, src in (("d2d_copy_image_ms", img), ("d2d_copy_packed_ms", pak)):
        dst = torch.empty_like(src)
        _, res[name] = timed(lambda: dst.copy_(src), a.reps)
        del dst
    for kind in ("snapshot", "restore"):
        v1, pk = res[kind + "_ms"], res[kind + "_packed_ms"]
        res[kind + "_packed_vs_v1"] = round(pk["median"] / v1["median"], 3)
        res[kind + "_packed_not_slower"] = bool(pk["median"] <= v1["median"] + (v1["max"] - v1["min"]))
    w, e = timed(lambda: idx.items(), a.reps)
    res["items_ms"], res["items_wall_ms"] = e, w
    if not a.no_dump:
        t0 = time.perf_counter()
        idx.dump()
        res["dump_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    if not a.no_files:
        del pak
        p1, pp = os.path.join(a.dir, "pmdfc_bench.img"), os.path.join(a.dir, "pmdfc_bench.pak")
        try:
            idx.save(p1)
            idx.close()
            del img
            torch.cuda.empty_cache()
            kv = KV(depth=depth, max_batch=B, max_segments=max_segs, serve_waves=1)
            kv.load(p1)
            res["file_reps"] = a.file_reps
            res["kv_save_wall_ms"] = wall(lambda: kv.save(p1), a.file_reps)
            res["kv_save_packed_wall_ms"] = wall(lambda: kv.save(pp, packed=True), a.file_reps)
            res["kv_load_wall_ms"] = wall(lambda: kv.load(p1), a.file_reps)
            res["kv_load_packed_wall_ms"] = wall(lambda: kv.load(pp), a.file_reps)
            res["file_bytes"], res["packed_file_bytes"] = os.path.getsize(p1), os.path.getsize(pp)
            res["kv_save_packed_vs_v1"] = round(res["kv_save_packed_wall_ms"]["median"] / res["kv_save_wall_ms"]["median"], 3)
            res["kv_load_packed_vs_v1"] = round(res["kv_load_packed_wall_ms"]["median"] / res["kv_load_wall_ms"]["median"], 3)
            kv.close()
        finally:
            for p in (p1, pp):
                if os.path.exists(p):
                    os.remove(p)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
