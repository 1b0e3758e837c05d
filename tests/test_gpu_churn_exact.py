"""Erase and insert churn across splits, op by op against the serial oracle.

Erase exists for churn: keys leave, fresh keys come, segments
keep splitting and the directory keeps doubling.  DESIGN.md 2 claims that no
other kernel had to change for it, because Invariant I holds between batches.
tests/test_gpu_erase.py compares with a table that cannot split, so its exact
comparisons stop at the first split after an erase.  Here the churn scripts of
tests/churn_ref.py are replayed through every mixed and insert path, and
after every step the statuses and values, after every erase step and at the
end the table image, depth, segments, split_loss and the stored entries are
the serial oracle's (oracle/cceh_oracle.c with oc_erase, which
tests/test_churn_ref.py holds to tests/erase_ref.py at these very states).
Every comparison is equality.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import churn_ref as CR
import erase_ref as E
import limits_ref as R
import scenarios as S
from pmdfc_amd.workload import uniform_keys

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pmdfc_amd as P  # noqa: E402
from pmdfc_amd.kv import KV  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_SEGS, MAX_BATCH = 512, 16384
FULL_BITS = 7  # floor(log2(MAX_BATCH)) - 7: the directory bucket bits of a table at full resolution


def engine(s, **kw):
    cfg = dict(depth=s.depth, max_batch=MAX_BATCH, max_segments=MAX_SEGS, upsert=s.upsert)
    cfg.update(kw)
    return P.CCEH(**cfg)


def _eq(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (what, f"{bad.size} of {got.size} differ, first at {int(bad[0])}: "
                           f"{got[bad[:4]].tolist()} != {want[bad[:4]].tolist()}")


def checked_dump(t, max_segments=MAX_SEGS):
    d, s = t.dump(), t.stats()
    R.check_table(d, s, max_segments)
    assert s["error_flags"] == 0, s["error_flags"]
    return d


def check_state(t, want, mark, what, loss0=0):
    """The engine's table is the oracle's: image, depth, segments, split_loss
    (loss0: the oracle's count when the engine's counters started), entries."""
    d = checked_dump(t)
    assert R.same_image(d, want), (what, "image")
    s = t.stats()
    got = (s["depth"], s["segments"], s["split_loss"])
    assert got == (mark["depth"], mark["segments"], mark["split_loss"] - loss0), (what, got, mark)
    assert t.items()[0].numel() == mark["live"], what


def _pieces(n, cut):
    return [(a, min(n, a + cut)) for a in range(0, n, cut)] if cut else [(0, n)]


def apply_mixed(t, path, ops, keys, vals, cut):
    n = len(ops)
    vo, st = np.zeros(n, np.uint64), np.zeros(n, np.uint8)
    if path == "MixedBatches":  # the whole step in one call, batch bounds every `cut`
        return t.MixedBatches(ops, keys, vals, list(range(0, n, cut)) + [n])
    for a, b in _pieces(n, cut):
        if path == "Insert" and np.all(ops[a:b] == P.OP_INSERT):
            st[a:b] = t.Insert(keys[a:b], vals[a:b])
        else:
            vo[a:b], st[a:b] = t.Mixed(ops[a:b], keys[a:b], vals[a:b])
    return vo, st


COMPACT_COUNTS = ("segments_before", "segments_after", "merges", "refused", "rounds", "depth_before", "depth_after")


def match_step(t, s, r, i, what, loss0=0):
    """Step i of script s, ("match", mask, patterns), through EraseMatching:
    the result's four fields and the table are the model's and the oracle's."""
    got = t.EraseMatching(s.steps[i][2], s.steps[i][1])
    assert got == r.results[i], (what, got, r.results[i])
    check_state(t, r.post[i], r.marks[i], what, loss0)


def compact_step(t, s, r, i, what, loss0=0):
    """Step i of script s, ("compact", fill_limit), through Compact -> the
    loss0 that holds from here on.  The counts are the model's and the table
    is the image the oracle went on from.  After a merge the engine was
    rebuilt as restore() rebuilds one: its history counters restarted, so its
    split_loss counts from the oracle's value at this step, and its bucket
    resolution is what the image's shallowest segment allows.  With no merge
    nothing restarted."""
    res, before = r.results[i], t.stats()
    got = t.Compact(s.steps[i][1])
    assert {k: got[k] for k in COMPACT_COUNTS} == {k: res[k] for k in COMPACT_COUNTS}, (what, got, res)
    after = t.stats()
    if res["merges"] > 0:
        assert after["splits"] == 0 and after["error_flags"] == 0, (what, after)
        loss0 = r.marks[i]["split_loss"]
    else:
        assert after == before, (what, before, after)
    check_state(t, r.post[i], r.marks[i], what, loss0)
    assert after["bucket_bits"] == min(FULL_BITS, int(np.min(r.post[i]["local_depth"]))), (what, after["bucket_bits"])
    return loss0


def replay(t, s, cut, path, first=0, loss0=0, trace=None):
    """Steps first.. of script s on engine t: each mixed step in pieces of
    `cut` ops (0: whole) through `path`, each erase step through Erase in
    pieces of `cut`, a match step through EraseMatching, a compact step
    through Compact.  Everything is compared with run_oracle(s).  Returns the
    oracle's run and the engine's bucket_bits at every erase step; trace, a
    list, receives (step, kind, bucket_bits after it) of every step."""
    r = CR.run_oracle(s)
    bits = []
    for i in range(first, len(s.steps)):
        step, what = s.steps[i], (s.name, path, cut, f"step {i}")
        if step[0] == "mixed":
            vo, st = apply_mixed(t, path, step[1], step[2], step[3], cut)
            _eq(st, r.results[i][1], what + ("status",))
            _eq(vo, r.results[i][0], what + ("values",))
        elif step[0] == "match":
            match_step(t, s, r, i, what, loss0)
        elif step[0] == "compact":
            loss0 = compact_step(t, s, r, i, what, loss0)
        else:
            st = np.concatenate([t.Erase(step[1][a:b]) for a, b in _pieces(len(step[1]), cut)])
            _eq(st, r.results[i], what + ("erase status",))
            check_state(t, r.post[i], r.marks[i], what, loss0)
            bits.append(t.stats()["bucket_bits"])
        if trace is not None:
            trace.append((i, step[0], t.stats()["bucket_bits"]))
    check_state(t, r.final, r.marks[len(s.steps)], (s.name, path, cut, "end"), loss0)
    return r, bits


def at_full_resolution(bits):
    """The two-launch path (k_medium) and the unramped general and pipelined
    paths are taken only by a table at its full bucket resolution, 7 bits at
    max_batch 16,384 (until then a batch runs as ramped sub-batches of the
    general pipeline).  churn and churn_upsert reach it two rounds before
    their end (test_churn_ref.py asserts the oracle's local depths): the whole
    last round, after nine erase steps, ran on those paths."""
    return bits[-2] == bits[-1] == FULL_BITS and bits[0] < FULL_BITS


# ---- 1. churn on every mixed path: k_medium, k_medium at its limit, the general pipeline

@pytest.mark.parametrize("cut", [1000, 8192, 16384])
def test_churn_whole_steps(cut):
    s = CR.script("churn")
    t = engine(s)
    _, bits = replay(t, s, cut, "Mixed")
    assert at_full_resolution(bits), bits
    t.close()


# ---- 2. the small cuttings: k_mixed_tiny, k_mixed_small, the ramp of a tiny table

@pytest.mark.parametrize("cut", [23, 64, 65, 256])
def test_churn_short_small_cuttings(cut):
    s = CR.script("churn_short")
    t = engine(s)
    replay(t, s, cut, "Mixed")
    t.close()


# ---- 3. the pipelined calls

def test_churn_mixed_batches():
    s = CR.script("churn")
    t = engine(s)
    _, bits = replay(t, s, 4096, "MixedBatches")
    assert at_full_resolution(bits), bits
    t.close()


def test_churn_insert_batches():
    """The inserts of churn alone (the oracle runs the projected script): each
    round's insert steps as one InsertBatches call with a batch per 4,096 ops,
    the erase steps between the calls."""
    s = CR.insert_only(CR.script("churn"))
    r = CR.run_oracle(s)
    t = engine(s)
    i, bits = 0, []
    while i < len(s.steps):
        if s.steps[i][0] == "erase":
            _eq(t.Erase(s.steps[i][1]), r.results[i], (s.name, i, "erase status"))
            check_state(t, r.post[i], r.marks[i], (s.name, i))
            bits.append(t.stats()["bucket_bits"])
            i += 1
            continue
        j = i
        while j < len(s.steps) and s.steps[j][0] == "mixed":
            j += 1
        keys = np.concatenate([s.steps[x][2] for x in range(i, j)])
        vals = np.concatenate([s.steps[x][3] for x in range(i, j)])
        st = t.InsertBatches(keys, vals, list(range(0, keys.size, 4096)) + [keys.size])
        _eq(st, np.concatenate([r.results[x][1] for x in range(i, j)]), (s.name, i, "status"))
        i = j
    check_state(t, r.final, r.marks[len(s.steps)], (s.name, "end"))
    assert at_full_resolution(bits), bits  # (the call pipelines only at full resolution)
    t.close()


# ---- 4. last-writer-wins: k_upsert_probe on re-inserted keys

@pytest.mark.parametrize("cut", [256, 16384])
def test_churn_upsert(cut):
    s = CR.script("churn_upsert")
    assert s.upsert
    t = engine(s)
    _, bits = replay(t, s, cut, "Mixed")
    assert at_full_resolution(bits), bits
    t.close()


# ---- 5. a split that drops entries after an erase

@pytest.mark.parametrize("cut", [64, 1000, 0])
def test_loss_after_erase(cut):
    s = CR.script("loss_after_erase")
    t = engine(s)
    r, _ = replay(t, s, cut, "Mixed")  # (ST_SPLIT_LOST is no status of the oracle's, so it cannot appear)
    (e,) = s.erase_steps()
    assert t.stats()["split_loss"] == r.marks[len(s.steps)]["split_loss"] > r.marks[e]["split_loss"]
    t.close()


# ---- 6. UNSPLITTABLE, erased, and UNSPLITTABLE again

@pytest.mark.parametrize("cut", [1, 0])
@pytest.mark.parametrize("path", ["Insert", "Mixed"])
def test_unsplittable(path, cut):
    s = CR.script("unsplittable")
    t = engine(s)
    r, _ = replay(t, s, cut, path)
    assert r.results[-1][1].tolist() == [P.ST_UNSPLITTABLE] and r.results[-4].tolist() == [P.ST_ERASED]
    t.close()


# ---- 7. both modes of the general mixed pre-pass after an erase (a process knob: a child each)

CHILD_JOIN = r'''
import json, sys
sys.path.insert(0, "tests")
import churn_ref as CR
import test_gpu_churn_exact as T
s = CR.script("churn")
t = T.engine(s)
_, bits = T.replay(t, s, 16384, "Mixed")
print(json.dumps({"ok": T.at_full_resolution(bits), "bits": bits}))
'''


@pytest.mark.parametrize("mode", ["0", "1"])
def test_churn_mixed_join_modes(mode):
    e = dict(os.environ)
    e["PMDFC_MIXED_JOIN"] = mode
    r = subprocess.run([sys.executable, "-c", CHILD_JOIN], cwd=REPO, env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (mode, r.stderr[-3000:])
    assert json.loads(r.stdout.strip().splitlines()[-1])["ok"]


# ---- 8. the served front-end: k_serve's ordered path grows the table after an erase

def _runs(n, rng):
    out, o = [], 0
    while o < n:
        r = int(rng.choice([1, 3, 17, 63, 64, 65, 100, 129, 200]))
        out.append((o, min(n, o + r)))
        o += r
    return out


def test_served_churn():
    """One caller thread, blocking runs of 1..200 ops.  The waves own disjoint
    hash prefixes, so whatever order they serve a run in, every op sees its
    own segment's ops in call order: the results are the serial oracle's,
    position by position."""
    s = CR.script("churn_short")
    r = CR.run_oracle(s)
    m_bits, k_hash = 1 << 20, 5
    kv = KV(depth=1, max_batch=4096, max_segments=MAX_SEGS, serve_waves=8)
    f = P.CountingBloomFilter(k_hash, m_bits)
    kv.attach_counting_bf(f)
    rng = np.random.default_rng(8)
    grown, inserts, erased = None, 0, 0
    for i, step in enumerate(s.steps):
        if step[0] == "mixed":
            n = len(step[1])
            vo, st = np.zeros(n, np.uint64), np.zeros(n, np.uint8)
            for a, b in _runs(n, rng):
                vo[a:b], st[a:b], _ = kv.ops(step[1][a:b], step[2][a:b], step[3][a:b], run=b - a)
            _eq(st, r.results[i][1], (i, "status"))
            _eq(vo, r.results[i][0], (i, "values"))
            inserts += int(np.count_nonzero(step[1] == P.OP_INSERT))
        else:
            st = kv.erase_run(step[1])
            _eq(st, r.results[i], (i, "erase status"))
            erased += int(np.count_nonzero(st == P.ST_ERASED))
            assert R.same_image(kv.dump(), r.post[i]), i
            if grown is None:
                grown = (kv.stats()["splits"], kv.phase()["header_reloads"])
    d, ks, ph = kv.dump(), kv.stats(), kv.phase()
    last = r.marks[len(s.steps)]
    assert R.same_image(d, r.final)
    R.check_table(d, ks, MAX_SEGS)
    assert (ks["depth"], ks["segments"], ks["split_loss"]) == (last["depth"], last["segments"], last["split_loss"])
    assert ks["error_flags"] == 0 and ph["failed_ops"] == 0
    # the table grew inside the served path after an erase (no backlog ever reached the flood hand-off)
    assert ph["flood_batches"] == 0
    assert ks["splits"] > grown[0] or ph["header_reloads"] > grown[1], (grown, ks["splits"], ph["header_reloads"])
    # the filter: no stored key is missing; it holds one count too many for every copy but
    # the first of an erased key, which the oracle's dumps give exactly
    stored, missing = kv.audit_filter()
    assert (stored, missing) == (last["live"], 0)
    c = f.counters()
    assert int(c.max()) < 255 and int(c.sum(dtype=np.uint64)) == k_hash * (inserts - erased)
    assert inserts - erased - stored == CR.copies_erased(s, r) + last["split_loss"]
    kv.attach_counting_bf(None)
    kv.close()
    f.close()


# ---- 9. erase under a full arena: ctl->full stays sticky, nothing splits

def test_erase_under_a_full_arena():
    ms = 16
    keys, vals = S.limit_stream(19, ms)
    t = P.CCEH(depth=2, max_batch=MAX_BATCH, max_segments=ms)
    cap = 0
    for a in range(0, keys.size, 8192):
        cap += int(np.count_nonzero(t.Insert(keys[a:a + 8192], vals[a:a + 8192]) == P.ST_CAPACITY))
    assert cap > 1000  # the arena is exhausted: from its dump on, the table that cannot split is the exact model
    pre, nseg = t.dump(), t.stats()["segments"]
    R.check_table(pre, t.stats(), ms)
    m = E.ErasableTable(pre)
    rng = np.random.default_rng(91)
    stored = np.unique(pre["keys"][pre["keys"] != np.uint64(R.INVALID)])
    gone = stored[rng.random(stored.size) < 0.5]
    plan = np.concatenate([gone, uniform_keys(92, 0, 200), gone[:50], np.array([R.INVALID, R.SENTINEL], np.uint64)])
    plan = plan[rng.permutation(plan.size)]
    _eq(t.Erase(plan), m.erase_batch(plan), "erase status")
    d = t.dump()
    R.check_table(d, t.stats(), ms)
    assert R.same_image(d, m.image()) and t.stats()["segments"] == nseg
    # re-inserts of every erased key, 5,000 fresh keys and Gets of stored, erased and absent keys, shuffled, in
    # a general batch; then a small one.  More inserts than the erase freed slots: the model answers CAPACITY
    fresh = uniform_keys(93, 0, 5000 + 100)
    general = (np.concatenate([gone, fresh[:5000]]),
               np.concatenate([stored[rng.integers(0, stored.size, 2000)], uniform_keys(94, 0, 500),
                               fresh[rng.integers(0, 5000, 500)]]))
    small = (fresh[5000:], stored[rng.integers(0, stored.size, 100)])
    for lo, (ins, gets) in enumerate((general, small)):
        mk = np.concatenate([ins, gets])
        ops = np.concatenate([np.full(ins.size, P.OP_INSERT, np.uint8), np.full(gets.size, P.OP_GET, np.uint8)])
        p = rng.permutation(mk.size)
        ops, mk = ops[p], mk[p]
        mv = np.where(ops == P.OP_INSERT, mk ^ np.uint64(0xE7A5E), np.uint64(0)).astype(np.uint64)
        assert mk.size <= MAX_BATCH
        wv, ws = m.mixed(ops, mk, mv)
        if lo == 0:
            assert np.count_nonzero(ws == R.ST_CAPACITY) > 100 and np.count_nonzero(ws == R.ST_INSERTED) > 1000
            assert np.count_nonzero(ws == R.ST_HIT) > 1000 and np.count_nonzero(ws == R.ST_MISS) > 100
        v, st = t.Mixed(ops, mk, mv)
        _eq(st, ws, ("mixed status", lo))
        _eq(v, wv, ("mixed values", lo))
        d, sa = t.dump(), t.stats()
        R.check_table(d, sa, ms)
        assert R.same_image(d, m.image()) and sa["segments"] == nseg, lo
        assert sa["error_flags"] & (1 << 17) == 0 and t.items()[0].numel() == m.live()
    t.close()


# ---- 10. restore in the middle of the churn

def test_restore_mid_churn():
    """After the fifth round an engine of its own starts from the first one's
    packed image; both finish the script, each compared with the oracle (not
    with the other).  restore() restarts the history counters: b's split_loss
    counts from the oracle's value at that point."""
    s = CR.script("churn")
    r = CR.run_oracle(s)
    mid = s.erase_steps()[4]
    a = engine(s)
    for i, step in enumerate(s.steps[:mid + 1]):  # (the head of the script: replay() without its end check)
        if step[0] == "mixed":
            vo, st = a.Mixed(step[1], step[2], step[3])
            _eq(st, r.results[i][1], (i, "status"))
            _eq(vo, r.results[i][0], (i, "values"))
        else:
            _eq(a.Erase(step[1]), r.results[i], (i, "erase status"))
            check_state(a, r.post[i], r.marks[i], i)
    b = engine(s)
    b.restore(a.snapshot(packed=True))
    assert R.same_image(checked_dump(b), r.post[mid])
    for t in (a, b):
        _, bits = replay(t, s, 16384, "Mixed", first=mid + 1, loss0=r.marks[mid]["split_loss"] if t is b else 0)
        assert bits[-2] == bits[-1] == FULL_BITS, bits
    assert b.stats()["segments"] - r.marks[mid]["segments"] > 40  # b split on from the restored image
    a.close()
    b.close()
