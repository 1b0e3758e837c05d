#!/usr/bin/env python3
"""Time EraseMatching against the scans that are its floor and against what an
operator had to do before it existed.

Builds the config-2 table of bench.py (CCEH_hybrid(65536), 64M unique uniform
keys in 1M-key batches: ~131k segments), keeps its packed image, and measures
in one process, by HIP events around the call (min / median / max over --reps
runs after a warm-up run; the table is restored from the packed image before
every run that removes something):
  * absent:     one pattern no key has under the full mask -- the pure scan --
                beside pmdfc_cbf_audit's scan of the same table and a
                device-to-device copy of the arena's pairs, the two floors of a
                full read;
  * sel64:      (mask, pattern) = (63, 21): 1/64 of the keys, about 8 per
                segment, beside today's way -- items(), the masked compare and
                nonzero in torch, Erase of the list in max_batch pieces, each
                step timed -- and beside Erase of the same list alone;
  * all:        mask 0 (every segment cleared) beside reset();
  * one_of_1024: one stored key under the full mask as 1 pattern and among
                1,024 patterns: the price of the LDS set.
The ratios are of the medians.  Prints one JSON line.  Not part of bench.py;
DESIGN.md 4.10 quotes a run.

    python tools/erase_matching_bench.py [--keys N] [--batch B] [--init-cap C] [--reps R] [--old-reps R2]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pmdfc_amd as P  # noqa: E402

FULL = 0xFFFFFFFFFFFFFFFF


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
    ap.add_argument("--old-reps", type=int, default=5)
    a = ap.parse_args()
    B, NK = a.batch, a.keys
    nb = NK // B
    depth = P.depth_for_hybrid(a.init_cap)
    idx = P.CCEH(depth=depth, max_batch=B, max_segments=int(NK / 512 * 1.25) + (1 << depth) + 1024)
    allk = torch.cat([P.gen_keys(1000, i * B, B) for i in range(nb)])
    idx.InsertBatches(allk, allk, [i * B for i in range(nb + 1)])
    s0 = idx.stats()
    live = idx.items()[0].numel()
    image = idx.snapshot(packed=True)
    res = {"keys": NK, "live": live, "segments": s0["segments"], "reps": a.reps, "device": torch.cuda.get_device_name(0)}

    def runs(fn, reps, restore):
        out, last = [], None
        for i in range(reps + 1):  # run 0 warms up
            if restore and i:
                idx.restore(image)
            ms, last = timed(fn)
            if i:
                out.append(ms)
        return spread(out), last

    def dev(xs):
        return torch.tensor(xs, dtype=torch.int64, device="cuda")

    # ---- the pure scan and its floors
    absent = P.gen_keys(2000, 0, 1)  # (another stream's key: the table never held it)
    res["absent_ms"], r = runs(lambda: idx.EraseMatching(absent, FULL), a.reps, False)
    assert r["removed"] == 0 and r["segments_changed"] == 0, r
    f = P.CountingBloomFilter(4, 1 << 28)
    f.rebuild(idx)
    res["cbf_audit_ms"], _ = runs(lambda: f.audit(idx), a.reps, False)
    f.close()
    pairs = torch.empty(s0["segments"] * 1024 * 2, dtype=torch.int64, device="cuda")
    dst = torch.empty_like(pairs)
    res["d2d_copy_ms"], _ = runs(lambda: dst.copy_(pairs), a.reps, False)
    res["d2d_copy_bytes"] = pairs.numel() * 8
    del pairs, dst
    res["absent_vs_audit"] = round(res["absent_ms"]["median"] / res["cbf_audit_ms"]["median"], 2)
    res["absent_vs_copy"] = round(res["absent_ms"]["median"] / res["d2d_copy_ms"]["median"], 2)

    # ---- 1/64 of the keys
    p64 = dev([21])
    res["sel64_ms"], r = runs(lambda: idx.EraseMatching(p64, 63), a.reps, True)
    res["sel64"] = r
    idx.restore(image)
    parts = {"items": [], "compare_nonzero": [], "erase": [], "total": []}
    alone = []
    for i in range(a.old_reps + 1):
        t_items, (k, _) = timed(idx.items)
        t_cmp, gone = timed(lambda: k[torch.nonzero((k & 63) == 21).squeeze(1)])

        def erase_all():
            for lo in range(0, gone.numel(), B):
                idx.Erase(gone[lo:lo + B])
        t_er, _ = timed(erase_all)
        assert gone.numel() == r["removed"], (gone.numel(), r)
        idx.restore(image)
        t_alone, _ = timed(erase_all)
        idx.restore(image)
        if i:
            for name, t in zip(parts, (t_items, t_cmp, t_er, t_items + t_cmp + t_er)):
                parts[name].append(t)
            alone.append(t_alone)
        del k, gone
    res["old_way_ms"] = {n: spread(x) for n, x in parts.items()}
    res["erase_list_alone_ms"] = spread(alone)
    res["old_way_vs_sel64"] = round(res["old_way_ms"]["total"]["median"] / res["sel64_ms"]["median"], 1)
    res["sel64_vs_erase_list_alone"] = round(res["sel64_ms"]["median"] / res["erase_list_alone_ms"]["median"], 2)

    # ---- everything
    any1 = dev([0x1234])
    res["all_ms"], r = runs(lambda: idx.EraseMatching(any1, 0), a.reps, True)
    assert r["removed"] == live and r["segments_cleared"] == r["segments_changed"], r
    res["all"] = r
    res["reset_ms"], _ = runs(idx.reset, a.reps, True)
    idx.restore(image)

    # ---- one pattern against 1,024 of which one exists
    one = allk[12345:12346].clone()
    many = torch.cat([one, P.gen_keys(3000, 0, 1023)])
    res["one_pattern_ms"], r = runs(lambda: idx.EraseMatching(one, FULL), a.reps, True)
    assert r["removed"] == 1, r
    res["of_1024_patterns_ms"], r = runs(lambda: idx.EraseMatching(many, FULL), a.reps, True)
    assert r["removed"] == 1, r
    res["set_vs_one"] = round(res["of_1024_patterns_ms"]["median"] / res["one_pattern_ms"]["median"], 2)
    res["error_flags"] = idx.stats()["error_flags"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
