#!/usr/bin/env python3
"""Time one Erase batch against a Get of the same keys and against the rebuild
an operator had to do before Erase existed.

Builds the config-2 table of bench.py (CCEH_hybrid(65536), 64M unique uniform
keys in 1M-key batches: ~131k segments) and measures, in one process, by HIP
events on the call's stream (min / median / max over --reps runs):
  * erase_stored: pmdfc_cceh_erase of one batch of --batch stored keys.  Run i
    takes batch i of the insert stream (uniform keys: a random sample of the
    table); the batch is inserted again after the run, outside the timing, so
    every run meets a table of the same load;
  * erase_absent: pmdfc_cceh_erase of --batch keys the table never held (the
    probe answers all of them; no run reaches the apply kernel);
  * get_stored: pmdfc_cceh_get of the batch erase_stored takes next -- the
    floor, the probe alone;
  * rebuild: what removes the same keys without Erase -- items(), a device-side
    filter of the exported pairs against the batch (torch.isin), reset(),
    InsertBatches of the survivors; timed as a whole and in its parts, over
    --rebuild-reps runs (the table is restored to its full load in between).
The ratios are of the medians.  Prints one JSON line.  Not part of bench.py;
DESIGN.md 4.8 quotes a run.  --only stored|absent restricts the run to one
kind of Erase batch (for a kernel trace of it: the per-kernel split).

    python tools/erase_bench.py [--keys N] [--batch B] [--init-cap C] [--reps R] [--rebuild-reps R2]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pmdfc_amd as P  # noqa: E402


def spread(xs):
    xs = sorted(xs)
    return {"min": round(xs[0], 3), "median": round(xs[len(xs) // 2], 3), "max": round(xs[-1], 3)}


def timed(fn):
    """fn() on the current stream between two events -> (ms, fn's result)."""
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=1 << 26)
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--init-cap", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--rebuild-reps", type=int, default=5)
    ap.add_argument("--only", choices=["stored", "absent"], default=None)
    a = ap.parse_args()
    B, NK = a.batch, a.keys
    nb = NK // B
    depth = P.depth_for_hybrid(a.init_cap)
    idx = P.CCEH(depth=depth, max_batch=B, max_segments=int(NK / 512 * 1.25) + (1 << depth) + 1024)
    allk = torch.cat([P.gen_keys(1000, i * B, B) for i in range(nb)])
    bounds = [i * B for i in range(nb + 1)]
    idx.InsertBatches(allk, allk, bounds)
    s0 = idx.stats()
    res = {"keys": NK, "batch": B, "segments": s0["segments"], "reps": a.reps,
           "device": torch.cuda.get_device_name(0)}

    def batch(i):
        return allk[(i % nb) * B:(i % nb + 1) * B]

    absent = P.gen_keys(2000, 0, B)
    idx.Erase(absent)  # warm-up: the first Erase allocates its scratch
    idx.Get(batch(0))
    if a.only != "absent":
        er, get = [], []
        for i in range(a.reps + 1):  # run 0 warms up
            g_ms, (_, gst) = timed(lambda: idx.Get(batch(i)))
            e_ms, st = timed(lambda: idx.Erase(batch(i)))
            assert bool((gst == P.ST_HIT).all()) and bool((st == P.ST_ERASED).all())
            ist = idx.Insert(batch(i), batch(i))
            assert bool((ist == P.ST_INSERTED).all())
            if i:
                er.append(e_ms)
                get.append(g_ms)
        res["erase_stored_ms"], res["get_stored_ms"] = spread(er), spread(get)
        res["erase_vs_get"] = round(res["erase_stored_ms"]["median"] / res["get_stored_ms"]["median"], 2)
    if a.only != "stored":
        ab = []
        for i in range(a.reps + 1):
            ms, st = timed(lambda: idx.Erase(absent))
            assert bool((st == P.ST_MISS).all())
            if i:
                ab.append(ms)
        res["erase_absent_ms"] = spread(ab)
    if a.only is None:
        parts = {"items": [], "filter": [], "reset_reinsert": [], "total": []}
        for i in range(a.rebuild_reps + 1):
            gone = batch(i)
            t_items, (k, v) = timed(idx.items)

            def keep():
                m = ~torch.isin(k, gone)
                return k[m], v[m]
            t_filter, (k2, v2) = timed(keep)
            n2 = k2.numel()
            b2 = list(range(0, n2, B)) + [n2]

            def again():
                idx.reset()
                idx.InsertBatches(k2, v2, b2)
            t_ins, _ = timed(again)
            # (the table may hold a few entries fewer than NK, of this batch too:
            # Insert4split's drops, stats().split_loss, differ from one rebuild to the next)
            assert 0 <= k.numel() - n2 <= B and B - (k.numel() - n2) <= 1024, (k.numel(), n2)
            if i:
                for name, t in zip(parts, (t_items, t_filter, t_ins, t_items + t_filter + t_ins)):
                    parts[name].append(t)
            del k, v, k2, v2
            idx.Insert(gone, gone)  # back to the full load
        res["rebuild_ms"] = {n: spread(x) for n, x in parts.items()}
        res["rebuild_vs_erase"] = round(res["rebuild_ms"]["total"]["median"] / res["erase_stored_ms"]["median"], 1)
    res["segments_after"] = idx.stats()["segments"]
    res["error_flags"] = idx.stats()["error_flags"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
