"""Crafted split images (scenarios.split_shapes) at every split call site.

split_team (split_device.h) has four mechanisms the uniform streams of the other
files hardly touch: the wrap unit's serial replay, the sweep's catch-up from a
backlog, the generic replay (a full parent, a wrap unit wider than 128 slots)
and the drop log.  Each shape here pins one of them (scenarios.SPLIT_SHAPES),
in segment 0 of CCEH_hybrid(2) and in a depth-4 segment of CCEH_hybrid(16).

Every run is compared bit for bit with the reference's own results
(tests/golden/split_shapes.json) and with the serial oracle: every op's
status and value, the final depth / local depths / keys / values, the dropped
entries, error_flags == 0 and no ST_SPLIT_LOST.

A stream is: n image inserts, n Gets of the image, the trigger insert (its
window is full: the split), n Gets of the image, 120 Gets of absent keys.  No
split happens before the trigger, so the cutting of the image inserts does not
matter (256-op batches); a CUT says which batch the trigger lands in.  Which
kernel a batch takes (cceh_engine.hip pmdfc_cceh_mixed / do_insert):
  n <= 64    k_mixed_tiny, n <= 256 k_mixed_small (one launch, splits inline);
  n <= 8192  k_part + k_medium (splits inline) if the table is at its full
             bucket resolution p1max = log2(max_batch) - 7 (or PMDFC_P1MAX):
             both tables are with max_batch = 500 (p1max = 1);
  else       the general pipeline, whose split round is k_split: both tables
             with max_batch = 4096 (p1max = 5 is deeper than either starts,
             and the untouched segments never deepen);
  tight      PMDFC_P1MAX=1 PMDFC_CHUNK=61: 61-op chunks, so the image, the
             Gets and the split of one batch meet in many rounds of the final
             pass (grow_and_split inline) -- through k_medium, and through the
             general pipeline's k_bucket for a batch padded past 8192 ops.
The tests do not assume this: they read the launch classes of the trigger's
batch from timing_read (`route` and `split` intervals exist only in the
general pipeline; a one-launch or k_medium batch is one `process` interval).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import scenarios as S
from oracle import oracle as O
from pmdfc_amd.workload import uniform_keys

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pmdfc_amd as P  # noqa: E402
from pmdfc_amd.kv import KV  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [b + s for s in S.SPLIT_SHAPE_TABLES for b in S.SPLIT_SHAPES]
GENERIC = ("full_", "wide_wrap")  # kSsPath 2: the generic replay (a full parent, a wrap unit wider than 128 slots)
# kSsPath 1: the cluster path (split_team's `fast`: the parent is not full and no unit outgrew the 128-bit
# window) -- dense_drop's wrap unit is 60 slots wide, dense_drop_wrap's 44
CLUSTER = ("backlog_", "cyclic_heads", "wrap_drop_both", "dense_drop")
kSsPath = 6


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "split_shapes.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def shapes():
    return S.split_shapes(O.hash64)


@pytest.fixture(scope="module")
def serial(shapes):
    """name -> the oracle's (values, statuses, dump, split_loss) of the whole
    stream, computed once; upsert: the same with last-writer-wins inserts."""
    def run(upsert):
        out = {}
        for name, (init_cap, conv, ops, keys, vals) in shapes.items():
            o = O.OracleCCEH(O.OracleCCEH.depth_for_hybrid(init_cap), upsert=upsert)
            ov, ost = o.mixed(ops, keys, vals)
            out[name] = (ov, ost, o.dump(), o.stats()["split_loss"])
        return out
    return {False: run(False), True: run(True)}


@pytest.fixture(scope="module")
def wants(shapes, golden):
    """name -> the reference's result of every Get of the stream, in stream order."""
    return {name: S.split_shape_get_values(golden[name], ops, keys, vals)
            for name, (_, _, ops, keys, vals) in shapes.items()}


def _check_table(t, g, od, loss):
    """The final table against the fixture and the oracle's dump."""
    d = t.dump()
    assert d["depth"] == od["depth"] == g["depth"]
    for f in ("local_depth", "keys", "values"):
        assert np.array_equal(d[f], od[f]), f
    assert S.sha(d["keys"]) == g["keys_sha"] and S.sha(d["values"]) == g["values_sha"]
    assert S.sha(d["local_depth"].astype(np.uint64)) == g["local_depth_sha"]
    s = t.stats()
    assert s["split_loss"] == loss == g["split_loss"]
    assert s["error_flags"] == 0


def _check_ops(out, st, ops, g, ov, ost, want):
    """Every op of a whole stream against the fixture and the oracle."""
    assert not np.any(st == P.ST_SPLIT_LOST)
    bad = np.nonzero((st != ost) | (out != ov))[0]
    assert bad.size == 0, (bad[:8], st[bad[:8]], ost[bad[:8]], out[bad[:8]], ov[bad[:8]])
    gets = ops == S.OP_GET
    assert np.array_equal(out[gets], want)
    assert np.all(st[~gets] == P.ST_INSERTED) and np.array_equal(st[gets] == P.ST_HIT, want != 0)


def _classes(t):
    return {k: c for k, (_, c) in t.timing_read().items() if c}


def _kernel(cls, n):
    """The kernel a batch of n ops took, from its timed launch classes."""
    if cls.get("route") or cls.get("split"):
        assert cls.get("route") == cls.get("split") == cls.get("parked") == 1, cls
        return "general"
    assert cls == {"process": 1}, cls
    return "tiny" if n <= 64 else "small" if n <= 256 else "medium"


# cut -> (max_batch, ops of the trigger's batch before the trigger, after it, the kernel it must take, tight);
# None: up to the stream's end
CUTS = {
    "tiny1": (4096, 0, 0, "tiny", False),
    "tiny64": (4096, 31, 32, "tiny", False),
    "small256": (4096, 127, 128, "small", False),
    "medium": (500, 249, 250, "medium", False),
    "general": (4096, None, None, "general", False),
    "tight_medium": (4096, None, None, "medium", True),
    "tight_general": (1 << 14, None, None, "general", True),
}


@pytest.fixture
def tight(monkeypatch):
    def set_(on):
        for k, v in (("PMDFC_P1MAX", "1"), ("PMDFC_CHUNK", "61"), ("PMDFC_FLAT_MAX", "3")):
            if on:
                monkeypatch.setenv(k, v)
            else:
                monkeypatch.delenv(k, raising=False)
    return set_


@pytest.mark.parametrize("cut", list(CUTS))
@pytest.mark.parametrize("name", NAMES)
def test_mixed_trigger_in_each_kernel(name, cut, shapes, golden, serial, wants, tight):
    """The whole stream through Mixed.  The trigger's batch holds Gets of image
    keys before and after the trigger (general, tight_*: all of them -- the
    batch is the stream from the first Get on, or the whole stream under
    tight_*), so a mixed batch answers them early against the pre-batch image
    and the drop log (28 entries for wide_wrap / wide_wrap_drop) decides which
    of them come before the split."""
    max_batch, before, after, kernel, is_tight = CUTS[cut]
    tight(is_tight)
    init_cap, conv, ops, keys, vals = shapes[name]
    n = S.split_shape_image_size(keys)
    if cut == "tight_general":  # pad past k_medium's 8192 ops with Gets of absent keys
        pad = uniform_keys(902, 0, 8193 - keys.size + 1000)
        keys = np.concatenate([keys, pad])
        ops = np.concatenate([ops, np.zeros(pad.size, np.uint8)])
        vals = np.concatenate([vals, np.zeros(pad.size, np.uint64)])
    N = keys.size
    if is_tight:
        a, b = 0, N
    elif before is None:
        a, b = n, N
    else:  # (the small images: the batch reaches back into the image inserts or ends with the stream)
        a, b = max(0, 2 * n - before), min(N, 2 * n + 1 + after)
    step = min(max(b - a, 64), max_batch)
    bounds = sorted(set(range(0, a, 256)) | {a, b, N} | set(range(b, N, step)))
    t = P.CCEH(init_cap, convention=conv, max_batch=max_batch, max_segments=64)
    t.timing(events=True)
    out = np.zeros(N, np.uint64)
    st = np.zeros(N, np.uint8)
    took = None
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        _classes(t)
        out[lo:hi], st[lo:hi] = t.Mixed(ops[lo:hi], keys[lo:hi], vals[lo:hi])
        if lo <= 2 * n < hi:
            assert (lo, hi) == (a, b)
            took = _kernel(_classes(t), hi - lo)
    assert took == kernel, (took, kernel)
    ov, ost, od, loss = serial[False][name]
    m = ov.size
    assert np.all(out[m:] == 0) and np.all(st[m:] == P.ST_MISS)  # (the padding)
    _check_ops(out[:m], st[:m], ops[:m], golden[name], ov, ost, wants[name])
    _check_table(t, golden[name], od, loss)
    t.close()


# the insert-only entry point: cut -> (max_batch, ops of the trigger's Insert batch, the kernel it must take)
INSERT_CUTS = {"tiny1": (4096, 1, "tiny"), "tiny64": (4096, 64, "tiny"), "small256": (4096, 256, "small"),
               "medium": (500, 500, "medium"), "general": (4096, 300, "general")}


@pytest.mark.parametrize("cut", list(INSERT_CUTS))
@pytest.mark.parametrize("name", NAMES)
def test_insert_trigger_in_each_kernel(name, cut, shapes, golden, serial, wants):
    """Insert batches, then the stream's last Gets through Get.  The trigger
    shares its Insert batch with the image inserts before it (ops of one
    segment: the split its full window causes replays what the batch has
    already placed).  Where the image has fewer keys than the batch needs
    (and in `general`, 300 ops: 59 image inserts, the trigger, the rest),
    inserts of other keys follow the trigger, none of the target segment's
    hash prefix -- the target's segments and the Gets stay the fixture's, the
    other segments are compared with the oracle."""
    max_batch, size, kernel = INSERT_CUTS[cut]
    init_cap, conv, ops, keys, vals = shapes[name]
    _, prefix, L, _, _, _ = S.split_shape_parts(name, O.hash64)
    n = S.split_shape_image_size(keys)
    before = min(59 if cut == "general" else size - 1, n)
    extra = uniform_keys(903, 0, 16 * size)
    extra = extra[O.hash64(extra) >> np.uint64(64 - L) != np.uint64(prefix)][:size - 1 - before]
    ik = np.concatenate([keys[:n], keys[2 * n:2 * n + 1], extra])
    iv = np.concatenate([vals[:n], vals[2 * n:2 * n + 1], extra ^ np.uint64(0x77)])
    a = n - before
    assert ik.size - a == size
    t = P.CCEH(init_cap, convention=conv, max_batch=max_batch, max_segments=64)
    t.timing(events=True)
    o = O.OracleCCEH(t.initial_depth)
    for lo in range(0, a, 256):
        hi = min(a, lo + 256)
        assert np.array_equal(t.Insert(ik[lo:hi], iv[lo:hi]), o.insert(ik[lo:hi], iv[lo:hi]))
    assert o.stats()["splits"] == 0
    _classes(t)
    st = t.Insert(ik[a:], iv[a:])
    assert _kernel(_classes(t), size) == kernel
    ost = o.insert(ik[a:], iv[a:])
    assert np.array_equal(st, ost) and np.all(st == P.ST_INSERTED)
    gk = keys[2 * n + 1:]
    gv, gs = t.Get(gk)
    ov, os_ = o.get(gk)
    assert np.array_equal(gv, ov) and np.array_equal(gs, os_) and not np.any(gs == P.ST_SPLIT_LOST)
    g = golden[name]
    want = wants[name][n:]
    assert np.array_equal(gv, want)  # the reference's answers after the split
    d, od = t.dump(), o.dump()
    assert d["depth"] == od["depth"]
    for f in ("local_depth", "keys", "values"):
        assert np.array_equal(d[f], od[f]), f
    s = t.stats()
    assert s["split_loss"] == o.stats()["split_loss"] == g["split_loss"] and s["error_flags"] == 0
    if not extra.size:
        _check_table(t, g, serial[False][name][2], serial[False][name][3])
    t.close()


@pytest.mark.parametrize("name", NAMES)
def test_upsert_matches_oracle(name, shapes, golden, serial, wants):
    """upsert=True (the claim paths around the shared split differ): the image
    in 256-op batches, then the stream from its first Get on as one mixed
    batch of the general pipeline, against OracleCCEH(upsert=True) -- and,
    the streams holding no key twice, against the same fixture."""
    init_cap, conv, ops, keys, vals = shapes[name]
    n = S.split_shape_image_size(keys)
    t = P.CCEH(init_cap, convention=conv, max_batch=4096, max_segments=64, upsert=True)
    out, st = t.MixedBatches(ops, keys, vals, list(range(0, n, 256)) + [n, keys.size])
    ov, ost, od, loss = serial[True][name]
    _check_ops(out, st, ops, golden[name], ov, ost, wants[name])
    _check_table(t, golden[name], od, loss)
    t.close()


@pytest.mark.parametrize("name", NAMES)
def test_k_split_takes_the_designed_replay(name, shapes, golden, serial, monkeypatch):
    """Under PMDFC_STAMPS=1 k_split writes word kSsPath of stamp row k for the
    k-th split of its launch (bucket.hip k_split: `a.stamps + k * 8`; rows are
    per batch, never cleared, and only k_split writes them -- the inline call
    sites pass no row): 1 for the cluster path, 2 for the generic replay.  The
    image goes in through one-launch batches (no partition, no stamp set), so
    the row is still zero; the trigger's batch is the trigger and 300 Gets of
    absent keys (past k_mixed_small: the general pipeline), the crafted split
    is the only request of its split round (row 0), and a second split of the
    same insert (full_child0, ...) runs inline in the final pass."""
    monkeypatch.setenv("PMDFC_STAMPS", "1")
    init_cap, conv, ops, keys, vals = shapes[name]
    n = S.split_shape_image_size(keys)
    t = P.CCEH(init_cap, convention=conv, max_batch=4096, max_segments=64)
    for lo in range(0, n, 256):
        assert np.all(t.Insert(keys[lo:min(n, lo + 256)], vals[lo:min(n, lo + 256)]) == P.ST_INSERTED)
    assert not t.debug_stamps(4096)[2][:, kSsPath].any()
    pad = uniform_keys(902, 0, 300)
    bk = np.concatenate([keys[2 * n:2 * n + 1], pad])
    bo = np.zeros(301, np.uint8)
    bo[0] = S.OP_INSERT
    t.timing(events=True)
    out, st = t.Mixed(bo, bk, np.concatenate([vals[2 * n:2 * n + 1], np.zeros(300, np.uint64)]))
    assert _kernel(_classes(t), 301) == "general"
    assert st[0] == P.ST_INSERTED and np.all(st[1:] == P.ST_MISS)
    rows = t.debug_stamps(4096)[2]
    assert name.startswith(GENERIC) != name.startswith(CLUSTER)  # every shape says which replay it is designed for
    want = 2 if name.startswith(GENERIC) else 1
    assert int(rows[0, kSsPath]) == want, (name, rows[:2])
    assert not rows[1:, kSsPath].any()  # the only split of its round
    ov, ost, od, loss = serial[False][name]
    _check_table(t, golden[name], od, loss)
    gv, gs = t.Get(keys[2 * n + 1:])
    assert np.array_equal(gv, ov[2 * n + 1:]) and np.array_equal(gs, ost[2 * n + 1:])
    t.close()


@pytest.mark.parametrize("name", NAMES)
def test_served_stream_matches_reference(name, shapes, golden, serial, wants):
    """The served path (k_serve through the ring, one blocking call per op,
    one ring: the ops apply in call order)."""
    init_cap, conv, ops, keys, vals = shapes[name]
    kv = KV(init_cap, convention=conv, max_batch=4096, max_segments=64, serve_waves=1, ring_size=1 << 13)
    out, st, pl = kv.ops(ops, keys, vals, run=0)
    assert np.array_equal(pl, np.arange(pl.size, dtype=np.uint64) + pl[0])
    ov, ost, od, loss = serial[False][name]
    _check_ops(out, st, ops, golden[name], ov, ost, wants[name])
    assert kv.phase()["failed_ops"] == 0
    _check_table(kv, golden[name], od, loss)
    kv.close()


# Team and single-wave splits: k_split gives a split to a team of four waves
# when its round's split list is at most PMDFC_SPLIT_TEAM_MAX long (a process
# knob: one child per setting runs every shape).  The general cutting of
# test_mixed_trigger_in_each_kernel, and the stamp cutting (the trigger with
# Gets of absent keys only) where the split is known to be k_split's.
CHILD = r'''
import json, sys, numpy as np
sys.path.insert(0, "tests")
import scenarios as S
from oracle import oracle as O
from pmdfc_amd.workload import uniform_keys
import pmdfc_amd as P
golden = json.load(open("tests/golden/split_shapes.json"))
res = {}
for name, (init_cap, conv, ops, keys, vals) in S.split_shapes(O.hash64).items():
    n = S.split_shape_image_size(keys)
    g = golden[name]
    o = O.OracleCCEH(O.OracleCCEH.depth_for_hybrid(init_cap))
    ov, ost = o.mixed(ops, keys, vals)
    od = o.dump()
    want = S.split_shape_get_values(g, ops, keys, vals)
    for cut in ("general", "alone"):
        t = P.CCEH(init_cap, convention=conv, max_batch=4096, max_segments=64)
        t.timing(events=True)
        if cut == "general":
            out, st = t.MixedBatches(ops, keys, vals, list(range(0, n, 256)) + [n, keys.size])
        else:
            pad = uniform_keys(902, 0, 300)
            z = np.zeros(300, np.uint64)
            out, st = t.MixedBatches(np.concatenate([ops[:2 * n + 1], z.astype(np.uint8), ops[2 * n + 1:]]),
                                     np.concatenate([keys[:2 * n + 1], pad, keys[2 * n + 1:]]),
                                     np.concatenate([vals[:2 * n + 1], z, vals[2 * n + 1:]]),
                                     list(range(0, n, 256)) + [n, 2 * n, 2 * n + 301, keys.size + 300])
            ok_pad = bool(np.all(st[2 * n + 1:2 * n + 301] == P.ST_MISS))
            keep = np.r_[0:2 * n + 1, 2 * n + 301:keys.size + 300]
            out, st = out[keep], st[keep]
        ok = bool(np.array_equal(st, ost) and np.array_equal(out, ov)) and not bool(np.any(st == P.ST_SPLIT_LOST))
        ok = ok and bool(np.array_equal(out[ops == S.OP_GET], want))
        if cut == "alone":
            ok = ok and ok_pad
        d = t.dump()
        ok = ok and d["depth"] == od["depth"] == g["depth"]
        ok = ok and all(np.array_equal(d[f], od[f]) for f in ("local_depth", "keys", "values"))
        ok = ok and S.sha(d["keys"]) == g["keys_sha"] and S.sha(d["values"]) == g["values_sha"]
        s = t.stats()
        ok = ok and s["split_loss"] == g["split_loss"] == o.stats()["split_loss"] and s["error_flags"] == 0
        ok = ok and t.timing_read()["split"][1] >= 1  # the general pipeline ran
        res[name + "/" + cut] = ok
        t.close()
print(json.dumps(res))
'''


@pytest.mark.parametrize("team_max", ["0", "1000000"])
def test_team_and_single_wave_splits(team_max):
    e = dict(os.environ)
    e["PMDFC_SPLIT_TEAM_MAX"] = team_max
    for k in ("PMDFC_P1MAX", "PMDFC_CHUNK", "PMDFC_FLAT_MAX", "PMDFC_STAMPS"):
        e.pop(k, None)
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=REPO, env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert len(res) == 2 * len(NAMES) and all(res.values()), (team_max, [k for k, v in res.items() if not v])
