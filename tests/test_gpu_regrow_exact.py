"""Shrink and regrow: Compact and EraseMatching inside the churn, op by op
against the serial oracle.

Compact is the one operation that moves a live table
backwards: the depth and the bucket resolution fall, the history counters
restart, segment ids are dense again, and the table ramps and splits its way
back.  A one-sided erase before it leaves local depths 3 and 8 side by side,
a shape growth never produces.  Every insert and mixed path was written for
tables that only grow, so here the regrow scripts of tests/churn_ref.py go
through all of them: after every step the statuses and values, after every
erase, match and compact step the table image, depth, segments, split_loss
and stored entries are the serial oracle's, which follows a Compact by
loading the image of tests/compact_ref.py (oc_load) and an EraseMatching by
erasing the keys of tests/match_ref.py.  The results of the two calls are the
models'.  tests/test_churn_ref.py holds the scripts, the load and the models
to each other on the CPU.  Every comparison is equality.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import churn_ref as CR
import limits_ref as R
from oracle import oracle as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pmdfc_amd as P  # noqa: E402
from pmdfc_amd.kv import KV  # noqa: E402

import test_gpu_churn_exact as T  # noqa: E402
from test_gpu_churn_exact import FULL_BITS, MAX_BATCH, MAX_SEGS, _eq, apply_mixed, check_state, engine  # noqa: E402

REPO = T.REPO
FULL_SIZE = ("regrow", "regrow_upsert", "lopsided")


def check_trace(s, trace):
    """bucket_bits after every step: it never falls except across a compact
    step, and a full-size script is back at the full resolution at the last
    erase before each compact step and at the end -- the lean first pass, the
    two-launch path and the unramped general and pipelined paths ran on a
    table that a Compact had taken down and that split its way back."""
    full = s.name.split("/")[0] in FULL_SIZE
    prev, last_erase = None, None
    for i, kind, b in trace:
        if kind == "compact":
            if full:  # (lopsided's first compact step follows its inserts directly)
                assert (prev if last_erase is None else last_erase) == FULL_BITS, (s.name, i, last_erase, trace)
            last_erase = None
        elif prev is not None:
            assert b >= prev, (s.name, i, trace)
        if kind == "erase":
            last_erase = b
        prev = b
    if full:
        assert prev == FULL_BITS, (s.name, trace)
        assert min(b for _, kind, b in trace if kind == "compact") < FULL_BITS - 1, trace  # (it did come down)


def run(name, cut, path, inserts=False, **kw):
    s = CR.script(name)
    if inserts:
        s = CR.insert_only(s)
    t = engine(s, **kw)
    trace = []
    r, _ = T.replay(t, s, cut, path, trace=trace)
    check_trace(s, trace)
    st = t.stats()
    assert st["error_flags"] == 0 and st["splits"] > 0
    t.close()
    return r


# ---- 1. regrow on every mixed path: ramped sub-batches, k_medium, the general pipeline, the pipelined call

@pytest.mark.parametrize("cut", [1000, 16384])
def test_regrow_whole_steps(cut):
    run("regrow", cut, "Mixed")


def test_regrow_mixed_batches():
    run("regrow", 4096, "MixedBatches")


# ---- 2. the insert-only calls: the lean first pass on a regrown table

def insert_batches(name):
    """The inserts of a script alone: each run of insert steps as one
    InsertBatches call with a batch per 4,096 ops, the other steps between."""
    s = CR.insert_only(CR.script(name))
    r = CR.run_oracle(s)
    t = engine(s)
    i, loss0, trace = 0, 0, []
    while i < len(s.steps):
        step, what = s.steps[i], (s.name, "InsertBatches", f"step {i}")
        if step[0] == "mixed":
            j = i
            while j < len(s.steps) and s.steps[j][0] == "mixed":
                j += 1
            keys = np.concatenate([s.steps[x][2] for x in range(i, j)])
            vals = np.concatenate([s.steps[x][3] for x in range(i, j)])
            st = t.InsertBatches(keys, vals, list(range(0, keys.size, 4096)) + [keys.size])
            _eq(st, np.concatenate([r.results[x][1] for x in range(i, j)]), what + ("status",))
            i = j - 1
        elif step[0] == "erase":
            _eq(t.Erase(step[1]), r.results[i], what + ("erase status",))
            check_state(t, r.post[i], r.marks[i], what, loss0)
        elif step[0] == "match":
            T.match_step(t, s, r, i, what, loss0)
        else:
            loss0 = T.compact_step(t, s, r, i, what, loss0)
        trace.append((i, step[0], t.stats()["bucket_bits"]))
        i += 1
    check_state(t, r.final, r.marks[len(s.steps)], (s.name, "end"), loss0)
    check_trace(s, trace)
    t.close()


def test_regrow_insert_batches():
    insert_batches("regrow")


def test_regrow_insert_calls():
    run("regrow", 8192, "Insert", inserts=True)


# ---- 3. the small cuttings: k_mixed_tiny, k_mixed_small, the ramp of a table that is tiny again

@pytest.mark.parametrize("cut", [23, 65, 256])
def test_regrow_short_small_cuttings(cut):
    run("regrow_short", cut, "Mixed")


# ---- 4. last-writer-wins: k_upsert_probe after a whole and after a partial Compact

@pytest.mark.parametrize("cut", [256, 16384])
def test_regrow_upsert(cut):
    assert CR.script("regrow_upsert").upsert
    run("regrow_upsert", cut, "Mixed")


# ---- 5. a lopsided table: local depths 3 and 8 under one bucket resolution, 32-entry sub-directories

def test_lopsided_mixed():
    r = run("lopsided", 16384, "Mixed")
    s = CR.script("lopsided")
    nothing, shrink = s.steps_of("compact")
    ld = np.asarray(r.post[shrink]["local_depth"], np.int64)
    assert r.results[nothing]["merges"] == 0 and ld.max() - ld.min() >= 4 and r.post[shrink]["depth"] == r.pre[shrink]["depth"]


@pytest.mark.parametrize("inserts", [False, True])
def test_lopsided_insert_calls(inserts):
    """The script as it is (a piece of inserts alone goes through Insert, the
    others through Mixed: k_medium at its limit) and its inserts alone."""
    run("lopsided", 8192, "Insert", inserts=inserts)


def test_lopsided_insert_batches():
    insert_batches("lopsided")


# ---- 6. both modes of the general mixed pre-pass (a process knob: a child each)

CHILD_JOIN = r'''
import json, sys
sys.path.insert(0, "tests")
import test_gpu_regrow_exact as G
G.run("regrow", 16384, "Mixed")
print(json.dumps({"ok": True}))
'''


@pytest.mark.parametrize("mode", ["0", "1"])
def test_regrow_mixed_join_modes(mode):
    e = dict(os.environ)
    e["PMDFC_MIXED_JOIN"] = mode
    r = subprocess.run([sys.executable, "-c", CHILD_JOIN], cwd=REPO, env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (mode, r.stderr[-3000:])
    assert json.loads(r.stdout.strip().splitlines()[-1])["ok"]


# ---- 7. the served front-end: k_serve's ordered path on a table that Compact took down to two segments

def test_served_regrow():
    """One caller thread, blocking runs of 1..200 ops as in test_served_churn,
    with erase_run, erase_matching and compact at the steps and a counting
    filter attached.  The results are the serial oracle's position by position
    and the images are its images at every erase, match and compact step."""
    s = CR.script("regrow_short")
    r = CR.run_oracle(s)
    kv = KV(depth=1, max_batch=4096, max_segments=MAX_SEGS, serve_waves=8)
    f = P.CountingBloomFilter(5, 1 << 20)
    kv.attach_counting_bf(f)
    rng = np.random.default_rng(8)
    loss0, shrunk = 0, None
    for i, step in enumerate(s.steps):
        if step[0] == "mixed":
            n = len(step[1])
            vo, st = np.zeros(n, np.uint64), np.zeros(n, np.uint8)
            for a, b in T._runs(n, rng):
                vo[a:b], st[a:b], _ = kv.ops(step[1][a:b], step[2][a:b], step[3][a:b], run=b - a)
            _eq(st, r.results[i][1], (i, "status"))
            _eq(vo, r.results[i][0], (i, "values"))
            continue
        if step[0] == "erase":
            _eq(kv.erase_run(step[1]), r.results[i], (i, "erase status"))
        elif step[0] == "match":
            got = kv.erase_matching(step[2], step[1])
            assert got == r.results[i], (i, got, r.results[i])
        else:
            got = kv.compact(step[1])
            assert {k: got[k] for k in T.COMPACT_COUNTS} == {k: r.results[i][k] for k in T.COMPACT_COUNTS}, (i, got)
            assert got["merges"] > 0 and kv.stats()["splits"] == 0
            loss0 = r.marks[i]["split_loss"]
            shrunk = (kv.stats()["splits"], kv.phase()["header_reloads"])
        d, ks, m = kv.dump(), kv.stats(), r.marks[i]
        assert R.same_image(d, r.post[i]), (i, step[0])
        R.check_table(d, ks, MAX_SEGS)
        assert (ks["depth"], ks["segments"], ks["split_loss"], ks["error_flags"]) == \
            (m["depth"], m["segments"], m["split_loss"] - loss0, 0), (i, ks, m)
    d, ks, ph = kv.dump(), kv.stats(), kv.phase()
    last = r.marks[len(s.steps)]
    assert R.same_image(d, r.final)
    R.check_table(d, ks, MAX_SEGS)
    assert (ks["depth"], ks["segments"], ks["split_loss"]) == (last["depth"], last["segments"], last["split_loss"] - loss0)
    assert ks["error_flags"] == 0 and ph["failed_ops"] == 0
    assert ph["flood_batches"] == 0  # the table grew back inside the served path
    assert ks["splits"] > shrunk[0] or ph["header_reloads"] > shrunk[1], (shrunk, ks["splits"], ph["header_reloads"])
    assert kv.audit_filter() == (last["live"], 0)  # no stored key is missing from the filter
    kv.attach_counting_bf(None)
    kv.close()
    f.close()


# ---- 8. two shards: each engine compacts its own half, the halves side by side are the oracle's table

def _side_by_side(a, b):
    d = {f: np.concatenate([np.asarray(a[f], np.uint64), np.asarray(b[f], np.uint64)])
         for f in ("local_depth", "prefix", "keys", "values")}
    d["depth"] = max(int(a["depth"]), int(b["depth"]))
    return d


@pytest.mark.parametrize("depth", [1, 2])
def test_two_shards_regrow(depth):
    """Two engines with shard_bits = 1 take regrow_short: every op goes to
    both, its owner (the top hash bit) answers as the oracle does and the other
    engine answers WRONG_SHARD (a reserved key is refused by both).  The oracle
    and the Compact model run unsharded at the engines' initial depth, which
    counts global hash bits: at depth 1 an engine starts as one segment (no
    bucket bits at all after a full Compact), at depth 2 as two.  No pair at
    the initial depth merges, so no merge crosses the shard boundary and the
    two dumps side by side, shard 0 first, are the oracle's image."""
    s = CR.script("regrow_short")
    r = CR.run_oracle(s, depth=depth)
    p1max = FULL_BITS
    ts = [P.CCEH(depth=depth, shard_bits=1, shard_id=k, max_batch=MAX_BATCH, max_segments=MAX_SEGS) for k in (0, 1)]
    base = [0, 0]  # split_loss of each engine before its last restart

    def owned(got, want, keys, k, what):
        mine = ((O.hash64(keys) >> np.uint64(63)) == np.uint64(k)) | (keys >= np.uint64(R.SENTINEL))  # (or reserved)
        _eq(got[mine], np.asarray(want)[mine], what + (k, "owner"))
        assert np.all(got[~mine] == P.ST_WRONG_SHARD), what + (k, "other shard")

    for i, step in enumerate(s.steps):
        what = (s.name, "shards", depth, f"step {i}")
        if step[0] == "mixed":
            for k, t in enumerate(ts):
                vo, st = apply_mixed(t, "Mixed", step[1], step[2], step[3], 4096)
                owned(st, r.results[i][1], step[2], k, what + ("status",))
                mine = (O.hash64(step[2]) >> np.uint64(63)) == np.uint64(k)
                _eq(vo[mine], r.results[i][0][mine], what + (k, "values"))
                assert np.all(vo[~mine] == 0), what
            continue
        res = r.results[i]
        if step[0] == "erase":
            for k, t in enumerate(ts):
                owned(t.Erase(step[1]), res, step[1], k, what + ("erase status",))
        elif step[0] == "match":
            got = [t.EraseMatching(step[2], step[1]) for t in ts]
            assert {f: got[0][f] + got[1][f] for f in res} == res, (what, got, res)
        else:
            before = [t.stats() for t in ts]
            got = [t.Compact(step[1]) for t in ts]
            for f in ("merges", "segments_before", "segments_after", "refused"):
                assert got[0][f] + got[1][f] == res[f], (what, f, got, res)
            assert max(g["depth_after"] for g in got) == res["depth_after"] and max(g["rounds"] for g in got) == res["rounds"]
            for k, t in enumerate(ts):
                after = t.stats()
                if got[k]["merges"] > 0:
                    assert after["splits"] == 0 and after["error_flags"] == 0
                    base[k] += before[k]["split_loss"]
                else:
                    assert after == before[k], (what, k)
        dumps, stats = [t.dump() for t in ts], [t.stats() for t in ts]
        whole, m = _side_by_side(*dumps), r.marks[i]
        for k in (0, 1):  # (check_table wants a whole hash space: the two halves together)
            assert stats[k]["error_flags"] == 0 and stats[k]["segments"] == len(dumps[k]["local_depth"]), (what, k)
        R.check_table(whole, {"segments": stats[0]["segments"] + stats[1]["segments"]}, 2 * MAX_SEGS)
        assert R.same_image(whole, r.post[i]), what
        assert stats[0]["segments"] + stats[1]["segments"] == m["segments"] and max(x["depth"] for x in stats) == m["depth"]
        assert sum(base) + stats[0]["split_loss"] + stats[1]["split_loss"] == m["split_loss"], what
        assert sum(t.items()[0].numel() for t in ts) == m["live"], what
        if step[0] == "compact":
            for k in (0, 1):
                assert stats[k]["bucket_bits"] == min(p1max, int(np.min(dumps[k]["local_depth"])) - 1), (what, k, stats[k])
    dumps = [t.dump() for t in ts]
    last = r.marks[len(s.steps)]
    assert R.same_image(_side_by_side(*dumps), r.final)
    assert sum(t.stats()["segments"] for t in ts) == last["segments"] and all(t.stats()["error_flags"] == 0 for t in ts)
    assert sum(base) + sum(t.stats()["split_loss"] for t in ts) == last["split_loss"]
    assert all(t.stats()["splits"] > 0 for t in ts)  # each half split its way back after its last Compact
    for t in ts:
        t.close()
