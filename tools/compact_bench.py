#!/usr/bin/env python3
"""Time Compact against what an operator had to do for the same effect before
it existed.

Builds the config-2 table of bench.py (CCEH_hybrid(65536), 64M unique uniform
keys in 1M-key batches: ~131k segments), erases a seeded --erase fraction of
the keys, keeps that table as a packed image, and measures in one process, by
HIP events on the call's stream (min / median / max over --reps runs, the
table restored from the image before each):
  * compact: CCEH.Compact(--limit), as a whole and in its steps (canonical
    order and live counts, gather, each round, restore: compact_timing());
  * rebuild: items() -> reset() -> InsertBatches of the survivors, which also
    merges (the table is built anew) -- as a whole and in its parts;
  * save_load: snapshot() then restore() of the version-1 and of the packed
    image on the device (no file), which reclaims retired ids and merges
    nothing.
The segment counts before and after each are reported.  Prints one JSON line.
Not part of bench.py; DESIGN.md 4.9 quotes a run.

    python tools/compact_bench.py [--keys N] [--batch B] [--init-cap C] [--erase F] [--limit L] [--reps R]
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
    ap.add_argument("--erase", type=float, default=0.75)
    ap.add_argument("--limit", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    B, NK = a.batch, a.keys
    nb = NK // B
    depth = P.depth_for_hybrid(a.init_cap)
    idx = P.CCEH(depth=depth, max_batch=B, max_segments=int(NK / 512 * 1.25) + (1 << depth) + 1024)
    allk = torch.cat([P.gen_keys(1000, i * B, B) for i in range(nb)])
    idx.InsertBatches(allk, allk, [i * B for i in range(nb + 1)])
    full = idx.stats()
    g = torch.Generator(device=allk.device)
    g.manual_seed(4242)
    gone = allk[torch.rand(NK, device=allk.device, generator=g) < a.erase]
    t_erase, st = timed(lambda: idx.Erase(gone))
    erased = int((st == P.ST_ERASED).sum())
    del allk, gone, st
    image = idx.snapshot(packed=True).clone()
    s0 = idx.stats()
    live = idx.items()[0].numel()
    res = {"keys": NK, "erased": erased, "live": live, "limit": a.limit, "reps": a.reps,
           "segments_full": full["segments"], "segments_erased": s0["segments"], "depth_erased": s0["depth"],
           "erase_ms": round(t_erase, 1), "device": torch.cuda.get_device_name(0)}

    # ---- Compact
    whole, steps, out = [], [], None
    for i in range(a.reps + 1):  # run 0 warms up
        idx.restore(image)
        ms, out = timed(lambda: idx.Compact(a.limit))
        if i:
            whole.append(ms)
            steps.append(idx.compact_timing())
    assert idx.items()[0].numel() == live
    res["compact"] = out
    res["compact_ms"] = spread(whole)
    res["compact_steps_ms"] = {k: spread([s[k] for s in steps]) for k in ("canonical", "gather", "restore")}
    res["compact_round_ms"] = [spread([s["rounds"][r] for s in steps]) for r in range(len(steps[0]["rounds"]))]
    res["utilization_after_compact"] = round(idx.Utilization(), 2)

    # ---- the rebuild: items -> reset -> InsertBatches
    parts = {"items": [], "reset_reinsert": [], "total": []}
    for i in range(a.reps + 1):
        idx.restore(image)
        t_items, (k, v) = timed(idx.items)
        n = k.numel()
        b2 = list(range(0, n, B)) + [n]

        def again():
            idx.reset()
            idx.InsertBatches(k, v, b2)
        t_ins, _ = timed(again)
        if i:
            for name, t in zip(parts, (t_items, t_ins, t_items + t_ins)):
                parts[name].append(t)
        del k, v
    res["rebuild_ms"] = {n: spread(x) for n, x in parts.items()}
    res["rebuild_segments"] = idx.stats()["segments"]
    res["rebuild_live"] = idx.items()[0].numel()  # (Insert4split's drops: a few fewer than before are possible)
    res["rebuild_vs_compact"] = round(res["rebuild_ms"]["total"]["median"] / res["compact_ms"]["median"], 2)

    # ---- snapshot + restore, both image kinds
    for packed in (False, True):
        ts, tr = [], []
        for i in range(a.reps + 1):
            idx.restore(image)
            t_s, img = timed(lambda: idx.snapshot(packed=packed))
            t_r, _ = timed(lambda: idx.restore(img))
            if i:
                ts.append(t_s)
                tr.append(t_r)
            del img
        name = "save_load_packed" if packed else "save_load_v1"
        res[name + "_ms"] = {"snapshot": spread(ts), "restore": spread(tr),
                             "total": spread([x + y for x, y in zip(ts, tr)])}
        res[name + "_segments"] = idx.stats()["segments"]
    res["error_flags"] = idx.stats()["error_flags"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
