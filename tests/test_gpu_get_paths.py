"""Every pure-Get kernel instance launch_get (cceh_kernels.hip) can choose, and
the probe-line count the roofline fraction of the benchmark is computed from.

launch_get picks by three process knobs: k_get (PMDFC_GET_UNROLL=1, built on
quad_probe), k_get_u<2> (the default) or k_get_u<4>, each with or without the
speculative second-line load of even home lines (PMDFC_GET_P2=0), and the
`rounds` loop of k_get_u when PMDFC_GET_GRID caps the grid; with
timing(count_lines=True) the COUNT instances, whose per-block partials
last_get_lines() sums.  The knobs are read once per process, so each variant
is one child process; the child runs one battery and prints one JSON dict of
named booleans, every one of which the parent asserts.

The battery compares everything with the serial oracle (OracleCCEH), by exact
equality -- values, statuses and the line count, which the oracle keeps as
stats()["get_lines"] under the same early-exit rule (oc_get):
  a  the probe-shape table (scenarios.get_probe_shapes: Gets that stop on every
     line of the window, from even, odd and wrapping home lines -- the CPU test
     tests/test_get_shapes.py holds the stream to that): the whole query set,
     then counted, class by class (hits / misses by even / odd home line, the
     wrapping home lines, everything); uncounted again, last_get_lines() raises;
  b  batch sizes around every tail of U x 64 quads per block and of `rounds`;
  c  GetBatches over a union past max_batch, GetRecords, an empty table, and a
     Get on both sides of an insert batch that splits (the flat directory copy
     is rebuilt);
  d  a split table (cap2_ins100k) under both directory forms of dir_entry
     (PMDFC_FLAT_MAX unset / 0 / 3, a create knob);
  e  a sharded pair: ST_WRONG_SHARD exactly for the other shard's keys.
"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import json, os, sys, numpy as np
sys.path.insert(0, "tests")
import scenarios as S
from oracle import oracle as O
import pmdfc_amd as P
from pmdfc_amd.workload import uniform_keys
out = {}

def same(a, b):
    return bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]))

def lines_of(o, k):
    """The oracle's Get of k and the lines it read."""
    a = o.stats()["get_lines"]
    r = o.get(k)
    return r, o.stats()["get_lines"] - a

def counted(t, o, k):
    """A counted Get of k: results and line count equal the oracle's."""
    r, want = lines_of(o, k)
    g = t.Get(k)
    return same(g, r) and t.last_get_lines() == want

# ---- a. the probe-shape table
depth, ins, vals, q = S.get_probe_shapes(O.hash64)
MB = 8192
t = P.CCEH(depth=depth, max_batch=MB, max_segments=64)
o = O.OracleCCEH(depth)
out["a/insert"] = bool(np.array_equal(t.Insert(ins, vals), o.insert(ins, vals)))
ref = o.get(q)
out["a/reserved_in_stream"] = int((ref[1] == P.ST_RESERVED_KEY).sum()) == 2
plain = t.Get(q)
out["a/get"] = same(plain, ref)
home = (O.hash64(q) & np.uint64(0xFF)).astype(np.int64)
hit, miss = ref[1] == P.ST_HIT, ref[1] == P.ST_MISS
classes = {"hit_even": hit & (home % 2 == 0), "hit_odd": hit & (home % 2 == 1),
           "miss_even": miss & (home % 2 == 0), "miss_odd": miss & (home % 2 == 1),
           "wrap": home >= S.GET_SHAPE_WRAP_LINE, "all": np.ones(q.size, bool)}
t.timing(events=False, count_lines=True)
for name, sel in classes.items():
    k = q[sel]
    out[f"a/counted/{name}"] = 0 < k.size <= MB and counted(t, o, k)
    g = t.Get(k)
    out[f"a/counted_equals_plain/{name}"] = bool(np.array_equal(g[0], plain[0][sel]) and np.array_equal(g[1], plain[1][sel]))
t.timing(events=False, count_lines=False)
out["a/plain_again"] = same(t.Get(q), ref)
try:
    t.last_get_lines()
    out["a/uncounted_raises"] = False
except P.PmdfcError:
    out["a/uncounted_raises"] = True

# ---- b. batch sizes (the query set twice over: the largest is past its end)
qq = np.tile(q, 2)
rr = (np.tile(ref[0], 2), np.tile(ref[1], 2))
for n in (1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 513, 4095, 4097):
    g = t.Get(qq[:n])
    out[f"b/n={n}"] = bool(np.array_equal(g[0], rr[0][:n]) and np.array_equal(g[1], rr[1][:n]))
t.timing(events=False, count_lines=True)
for n in (1, 65, 513, 4097):
    out[f"b/counted/n={n}"] = counted(t, o, qq[:n])
t.timing(events=False, count_lines=False)

# ---- c. entry points
q3 = np.tile(q, 3)
g = t.GetBatches(q3, [0, 1, 700, 5000, 5000, q3.size])
out["c/get_batches"] = q3.size > MB and bool(np.array_equal(g[0], np.tile(ref[0], 3)) and np.array_equal(g[1], np.tile(ref[1], 3)))
rec = t.GetRecords(q).cpu().numpy().view(np.uint64).reshape(-1, 2)
out["c/get_records"] = bool(np.array_equal(rec[:, 0], plain[0]) and np.array_equal(rec[:, 1], plain[1].astype(np.uint64)))
out["a/error_flags"] = t.stats()["error_flags"] == 0
t.close()

t = P.CCEH(depth=depth, max_batch=MB, max_segments=64)
o = O.OracleCCEH(depth)
out["c/empty"] = same(t.Get(q), o.get(q))
t.timing(events=False, count_lines=True)
out["c/empty_counted"] = counted(t, o, q)
out["c/empty_error_flags"] = t.stats()["error_flags"] == 0
t.close()

k = uniform_keys(31, 0, 6000)
v = k ^ np.uint64(0x77)
ask = np.concatenate([k, uniform_keys(31, 6000, 2000)])
t = P.CCEH(2, max_batch=MB, max_segments=256)
o = O.OracleCCEH(t.initial_depth)
ok = bool(np.array_equal(t.Insert(k[:1500], v[:1500]), o.insert(k[:1500], v[:1500])))
out["c/resplit/get_before"] = ok and same(t.Get(ask), o.get(ask))
before = t.stats()["splits"]
ok = bool(np.array_equal(t.Insert(k[1500:], v[1500:]), o.insert(k[1500:], v[1500:])))
out["c/resplit/splits"] = ok and t.stats()["splits"] > before and o.stats()["splits"] == t.stats()["splits"]
out["c/resplit/get_after"] = same(t.Get(ask), o.get(ask))
t.timing(events=False, count_lines=True)
out["c/resplit/counted"] = counted(t, o, ask)
out["c/resplit/error_flags"] = t.stats()["error_flags"] == 0
t.close()

# ---- d. a split table, both directory forms
init_cap, conv, ops, keys, vals = S.scenarios(O.hash64)["cap2_ins100k"]
batch = 1 << 14
ik, iv = keys[ops == S.OP_INSERT], vals[ops == S.OP_INSERT]
ask = np.concatenate([ik, uniform_keys(4, ik.size, ik.size)])
ask = ask[np.random.default_rng(5).permutation(ask.size)]
o = O.OracleCCEH(O.OracleCCEH.depth_for_hybrid(init_cap))
ost = o.insert(ik, iv)
want = o.get(ask)
out["d/half_absent"] = int((want[1] == P.ST_MISS).sum()) == ik.size
(w1, l1) = lines_of(o, ask[:batch])
for flat in (None, "0", "3"):
    os.environ.pop("PMDFC_FLAT_MAX", None)
    if flat is not None:
        os.environ["PMDFC_FLAT_MAX"] = flat
    t = P.CCEH(init_cap, convention=conv, max_batch=batch, max_segments=16384)
    st = t.InsertBatches(ik, iv, list(range(0, ik.size, batch)) + [ik.size])
    out[f"d/flat={flat}/insert"] = bool(np.array_equal(st, ost)) and t.stats()["splits"] == o.stats()["splits"]
    out[f"d/flat={flat}/get"] = same(t.Get(ask), want)
    t.timing(events=False, count_lines=True)
    g = t.Get(ask[:batch])
    out[f"d/flat={flat}/counted"] = same(g, w1) and t.last_get_lines() == l1
    out[f"d/flat={flat}/error_flags"] = t.stats()["error_flags"] == 0
    t.close()
os.environ.pop("PMDFC_FLAT_MAX", None)

# ---- e. a sharded pair: each shard holds its half, and is asked for every key
k = uniform_keys(41, 0, 40000)
v = k ^ np.uint64(0x99)
ask = np.concatenate([k, uniform_keys(41, 40000, 20000)])
ask = ask[np.random.default_rng(6).permutation(ask.size)]
D = 4
o = O.OracleCCEH(D)
o.insert(k, v)
want = o.get(ask)
owner = (O.hash64(k) >> np.uint64(63)).astype(np.int64)
aowner = (O.hash64(ask) >> np.uint64(63)).astype(np.int64)
for sh in (0, 1):
    t = P.CCEH(depth=D, shard_bits=1, shard_id=sh, max_batch=1 << 16, max_segments=4096)
    mine = owner == sh
    out[f"e/shard{sh}/insert"] = bool(np.all(t.Insert(k[mine], v[mine]) == P.ST_INSERTED))
    gv, gs = t.Get(ask)
    other = aowner != sh
    out[f"e/shard{sh}/wrong_shard"] = bool(np.array_equal(gs == P.ST_WRONG_SHARD, other) and np.all(gv[other] == 0)
                                           and 0 < int(other.sum()) < ask.size)
    out[f"e/shard{sh}/own"] = bool(np.array_equal(gv[~other], want[0][~other]) and np.array_equal(gs[~other], want[1][~other]))
    out[f"e/shard{sh}/error_flags"] = t.stats()["error_flags"] == 0
    t.close()
print(json.dumps(out))
'''

VARIANTS = {
    "default": {},
    "u1": {"PMDFC_GET_UNROLL": "1"},
    "u2_nop2": {"PMDFC_GET_UNROLL": "2", "PMDFC_GET_P2": "0"},
    "u4": {"PMDFC_GET_UNROLL": "4"},
    "u4_nop2": {"PMDFC_GET_UNROLL": "4", "PMDFC_GET_P2": "0"},
    "u2_grid1": {"PMDFC_GET_UNROLL": "2", "PMDFC_GET_GRID": "1"},
    "u4_grid3": {"PMDFC_GET_UNROLL": "4", "PMDFC_GET_GRID": "3"},
    "u4_nop2_grid1": {"PMDFC_GET_UNROLL": "4", "PMDFC_GET_P2": "0", "PMDFC_GET_GRID": "1"},
}
GET_KNOBS = ("PMDFC_GET_UNROLL", "PMDFC_GET_P2", "PMDFC_GET_GRID", "PMDFC_FLAT_MAX")


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_get_variant_matches_oracle(variant):
    e = dict(os.environ)
    for k in GET_KNOBS:
        e.pop(k, None)
    e.update(VARIANTS[variant])
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=REPO, env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert len(res) == 69, sorted(res)  # (the whole battery ran)
    bad = sorted(k for k, v in res.items() if v is not True)
    assert not bad, (variant, bad)
