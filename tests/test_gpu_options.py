"""The engine's optional pass layouts, each in a child process with its
environment knob set (the engine reads them once per process): results equal
the serial oracle op by op and table by table, as the default layout's do in
test_gpu_parity.py.  The options are off by default because they measured
slower, not because they differ:
  PMDFC_SPLIT_TEAM_MAX=0        every split by one wave (no four-wave teams);
  PMDFC_SPLIT_TEAM_MAX=1000000  every split by a team of four waves;
  PMDFC_PIPE_GROUP=1            the insert pipeline with an event pair per batch.
(The round-5 fused layouts -- split round + parked pass, parked + final pass
-- measured slower and were removed in round 6.)
Further down, each with its own comment: the mixed batches' two modes and Get
unrolls, the routed call forced on one rank, and the remaining knobs of
csrc/knobs.h -- the moved path cuts (PMDFC_SMALL_MAX, PMDFC_MEDIUM_MAX), gated
mixed batches on full grids (PMDFC_MIXED_SMALL), the ramp's sub-batch sizes
(PMDFC_RAMP_OPS / PMDFC_RAMP_MIN), PMDFC_FAST_LDS_PAD, PMDFC_PSTREAM_PRIO,
stamp-set rotation (PMDFC_STAMP_ROT) and routed inserts through the pipeline
(PMDFC_ROUTE_PIPE).  The pure-Get knobs are in test_gpu_get_paths.py;
tests/test_get_shapes.py fails for a knob that no GPU test sets."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import json, sys, numpy as np
sys.path.insert(0, "tests")
import scenarios as S
from oracle import oracle as O
import pmdfc_amd as P
scen = S.scenarios(O.hash64)
out = {}
for name, batch in (("cap2_ins100k", 1 << 14), ("cap256_ins400k", 1 << 16), ("mixed_cap16_60k", 10000),
                    ("split_loss", 1 << 12), ("dup_pairs", 9000)):
    init_cap, conv, ops, keys, vals = scen[name]
    n = keys.size
    t = P.CCEH(init_cap, convention=conv, max_batch=batch, max_segments=16384)
    o = O.OracleCCEH(t.initial_depth)
    ins = ops == S.OP_INSERT
    if ins.all() or (ins[: ins.sum()].all() and name != "mixed_cap16_60k"):
        k, v = keys[ins], vals[ins]
        st = t.InsertBatches(k, v, list(range(0, k.size, batch)) + [k.size])
        ost = o.insert(k, v)
        ok = bool(np.array_equal(st, ost))
        g = keys[~ins]
        if g.size:
            gv, gs = t.Get(g)
            ov, os_ = o.get(g)
            ok = ok and bool(np.array_equal(gv, ov) and np.array_equal(gs, os_))
    else:
        vo, st = t.MixedBatches(ops, keys, vals, list(range(0, n, batch)) + [n])
        ov, ost = o.mixed(ops, keys, vals)
        ok = bool(np.array_equal(st, ost) and np.array_equal(vo, ov))
    d, od = t.dump(), o.dump()
    ok = ok and d["depth"] == od["depth"] and all(np.array_equal(d[f], od[f]) for f in ("local_depth", "keys", "values"))
    ok = ok and t.stats()["error_flags"] == 0
    out[name] = ok
    t.close()
print(json.dumps(out))
'''


@pytest.mark.parametrize("env", [{"PMDFC_SPLIT_TEAM_MAX": "0"}, {"PMDFC_SPLIT_TEAM_MAX": "1000000"},
                                 {"PMDFC_PIPE_GROUP": "1"}])
def test_optional_layouts_match_oracle(env):
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=REPO, env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert all(res.values()), (env, res)


# Mixed batches tell their Gets whether the batch inserts their key in one of
# two exact ways, chosen per batch from the last batch's insert count
# (cceh_engine.hip mixed_join_mode): the insert set, or the Get-side join.
# Each forced for every batch, over the mixed fixture streams at three batch
# cuttings (every op and the final table against the serial oracle), plus a
# stream whose Gets hit wrapping windows of keys the same batch re-inserts
# and misses of keys inserted once or twice in the batch (the join's cases).
MIXED_STREAMS = r'''
import json, sys, numpy as np
sys.path.insert(0, "tests")
import scenarios as S
from oracle import oracle as O
import pmdfc_amd as P
scen = dict(S.scenarios(O.hash64))
rng = np.random.default_rng(77)
base = rng.integers(1, 1 << 62, 40000, dtype=np.uint64)
h = O.hash64(base)
wrap = base[(h & np.uint64(0xFF)) >= np.uint64(249)]
pre = base[:30000]
ops = [np.ones(30000, np.uint8)]
keys = [pre]
for r in range(4):
    k = np.concatenate([rng.choice(pre, 12000), rng.choice(wrap, 3000), base[30000 + r * 2000: 32000 + r * 2000],
                        rng.choice(base[30000:], 3000)])
    o = (rng.random(k.size) < 0.45).astype(np.uint8)
    p = rng.permutation(k.size)
    ops.append(o[p]); keys.append(k[p])
ops = np.concatenate(ops); keys = np.concatenate(keys)
vals = keys ^ np.uint64(0x5555)
scen["join_cases"] = (64, "hybrid", np.where(ops == 1, S.OP_INSERT, S.OP_GET).astype(np.uint8), keys, vals)
out = {}
'''
CHILD_MIXED = MIXED_STREAMS + r'''for name in ("mixed_cap16_60k", "mixed_cap2_30k_ins80", "split_loss_mixed", "dup_wrap", "join_cases"):
    init_cap, conv, ops, keys, vals = scen[name]
    n = keys.size
    for batch in (9000, 20000, 65536):
        t = P.CCEH(init_cap, convention=conv, max_batch=batch, max_segments=16384)
        o = O.OracleCCEH(t.initial_depth)
        vo, st = t.MixedBatches(ops, keys, vals, list(range(0, n, batch)) + [n])
        ov, ost = o.mixed(ops, keys, vals)
        ok = bool(np.array_equal(st, ost) and np.array_equal(vo, ov))
        d, od = t.dump(), o.dump()
        ok = ok and d["depth"] == od["depth"] and all(np.array_equal(d[f], od[f]) for f in ("local_depth", "keys", "values"))
        ok = ok and t.stats()["error_flags"] == 0
        out[f"{name}/{batch}"] = ok
        t.close()
print(json.dumps(out))
'''


@pytest.mark.parametrize("mode", ["0", "1"])
def test_mixed_modes_match_oracle(mode):
    e = dict(os.environ)
    e["PMDFC_MIXED_JOIN"] = mode
    r = subprocess.run([sys.executable, "-c", CHILD_MIXED], cwd=REPO, env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert all(res.values()), (mode, res)


# The Get kernels of both modes have one template instance per unroll
# (PMDFC_MG_U: Gets per quad issued together; 2 is the default the test above
# runs).  The other two, each under both modes: the join's stream and
# dup_wrap, cut into 9,000-op batches -- the smallest that still take the
# general path (PMDFC_MEDIUM_MAX is 8,192) -- with first-writer-wins and with
# last-writer-wins inserts (under upsert every hit asks about the batch's
# inserts of its key).  Every op and the final table against the serial oracle.
CHILD_MIXED_UNROLL = MIXED_STREAMS + r'''for name in ("join_cases", "dup_wrap"):
    init_cap, conv, ops, keys, vals = scen[name]
    n = keys.size
    batch = 9000
    for upsert in (False, True):
        t = P.CCEH(init_cap, convention=conv, max_batch=batch, max_segments=16384, upsert=upsert)
        o = O.OracleCCEH(t.initial_depth, upsert=upsert)
        vo, st = t.MixedBatches(ops, keys, vals, list(range(0, n, batch)) + [n])
        ov, ost = o.mixed(ops, keys, vals)
        ok = bool(np.array_equal(st, ost) and np.array_equal(vo, ov))
        d, od = t.dump(), o.dump()
        ok = ok and d["depth"] == od["depth"] and all(np.array_equal(d[f], od[f]) for f in ("local_depth", "keys", "values"))
        ok = ok and t.stats()["error_flags"] == 0
        out[f"{name}/upsert={upsert}"] = ok
        t.close()
print(json.dumps(out))
'''


@pytest.mark.parametrize("mode", ["0", "1"])
@pytest.mark.parametrize("unroll", ["1", "4"])
def test_mixed_get_unrolls_match_oracle(unroll, mode):
    e = dict(os.environ)
    e["PMDFC_MG_U"] = unroll
    e["PMDFC_MIXED_JOIN"] = mode
    r = subprocess.run([sys.executable, "-c", CHILD_MIXED_UNROLL], cwd=REPO, env=e, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert len(res) == 4 and all(res.values()), (unroll, mode, res)


# The routed call forced through its pack / exchange / unpack on one rank
# (PMDFC_ROUTE_DIRECT=0: on one rank the routed call is otherwise the direct
# call), at the bench's batch geometry: three 1M-op insert batches, then Get
# batches (half stored keys, half absent) with and without the per-tile
# dedupe, then 50/50 mixed batches -- every status and value equal to a
# direct engine fed the same batches.
CHILD_ROUTE = r'''
import json, sys, torch, numpy as np
import pmdfc_amd as P
from pmdfc_amd.dist import BlockRouter
B, nb = 1 << 20, 3
pk = P.BlockPacker(0, B, 0)
idx = P.CCEH(depth=16, max_batch=pk.rows, max_segments=1 << 17, device=0)
comm = P.Comm(0)
r = BlockRouter(idx, pk, comm=comm)
assert r._native()
direct = P.CCEH(depth=16, max_batch=B, max_segments=1 << 17, device=0)
keys = [P.gen_keys(900 + i, 0, B, device=0) for i in range(nb)]
out = {}
st_r = r.insert_batches([(k, k) for k in keys])
out["insert"] = all(bool(torch.equal(a, direct.Insert(k, k))) for a, k in zip(st_r, keys))
q = [torch.cat([k[: B // 2], P.gen_keys(950 + i, 0, B // 2, device=0)]) for i, k in enumerate(keys)]
ok = True
for dd in (True, False):
    r.dedupe_gets = dd
    for (v, s), qq in zip(r.get_batches(q), q):
        vd, sd = direct.Get(qq)
        ok = ok and bool(torch.equal(v, vd) and torch.equal(s, sd))
out["get"] = ok
rng = np.random.default_rng(5)
mb = []
for i in range(nb):
    o = torch.from_numpy((rng.random(B) < 0.5).astype(np.uint8)).to("cuda:0")
    fresh = P.gen_keys(980 + i, 0, B, device=0)
    k = torch.where(o.bool(), fresh, keys[i][torch.randint(0, B, (B,), device="cuda:0")])
    mb.append((k, k ^ 5, o))
ok = True
for (v, s), (k, vv, o) in zip(r.mixed_batches(mb), mb):
    vd, sd = direct.Mixed(o, k, vv)
    ok = ok and bool(torch.equal(v, vd) and torch.equal(s, sd))
out["mixed"] = ok
print(json.dumps(out))
'''


def test_routed_forced_one_rank_bench_geometry():
    e = dict(os.environ)
    e["PMDFC_ROUTE_DIRECT"] = "0"
    r = subprocess.run([sys.executable, "-c", CHILD_ROUTE], cwd=REPO, env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert all(res.values()), res


def _run_child(script, env, *args):
    """One child process with `env` on top of the caller's: its last output
    line, a JSON dict of named booleans."""
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, "-c", script, *map(str, args)], cwd=REPO, env=e, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


# The cuts between the one-launch, the two-launch and the general path moved
# (PMDFC_SMALL_MAX, PMDFC_MEDIUM_MAX: process knobs): the small-batch streams of
# test_gpu_parity.py's test_small_batches_exact, cut the same way -- a batch
# of inserts goes through Insert or through Mixed in turn -- at batch sizes on
# both sides of the moved cut (argv: max_batch, then the batch sizes).  Every
# op and the final table against the serial oracle.
CHILD_SMALL = r'''
import json, sys, numpy as np
sys.path.insert(0, "tests")
import scenarios as S
from oracle import oracle as O
import pmdfc_amd as P
scen = S.scenarios(O.hash64)
max_batch = int(sys.argv[1])
out = {}
for name in ("cap2_ins3k", "mixed_cap2_30k_ins80"):
    init_cap, conv, ops, keys, vals = scen[name]
    n = keys.size
    for batch in map(int, sys.argv[2:]):
        t = P.CCEH(init_cap, convention=conv, max_batch=max_batch, max_segments=8192)
        vo = np.zeros(n, np.uint64)
        st = np.zeros(n, np.uint8)
        for i, off in enumerate(range(0, n, batch)):
            sl = slice(off, off + batch)
            if i % 2 and np.all(ops[sl] == S.OP_INSERT):
                st[sl] = t.Insert(keys[sl], vals[sl])
            else:
                vo[sl], st[sl] = t.Mixed(ops[sl], keys[sl], vals[sl])
        o = O.OracleCCEH(t.initial_depth)
        ov, ost = o.mixed(ops, keys, vals)
        ok = bool(np.array_equal(st, ost) and np.array_equal(vo, ov))
        d, od = t.dump(), o.dump()
        ok = ok and d["depth"] == od["depth"] and all(np.array_equal(d[f], od[f]) for f in ("local_depth", "keys", "values"))
        ok = ok and t.stats()["error_flags"] == 0
        out[f"{name}/{batch}"] = ok
        t.close()
print(json.dumps(out))
'''


@pytest.mark.parametrize("env,max_batch,batches", [
    ({"PMDFC_SMALL_MAX": "0"}, 8192, (23, 256)),    # no batch takes k_mixed_tiny / k_mixed_small
    ({"PMDFC_SMALL_MAX": "64"}, 8192, (64, 65)),    # the cut inside the default range: the last small batch, the first other
    ({"PMDFC_MEDIUM_MAX": "0"}, 1024, (300, 1000)),  # (p1max = 3, reached early) no batch takes k_part + k_medium
], ids=["small_max0", "small_max64", "medium_max0"])
def test_moved_path_cuts_match_oracle(env, max_batch, batches):
    res = _run_child(CHILD_SMALL, env, max_batch, *batches)
    assert len(res) == 4 and all(res.values()), (env, res)


def test_gated_mixed_batches_on_full_grids():
    """PMDFC_MIXED_SMALL=0: the passes of gated mixed batches on full grids,
    over the streams of the mixed-Get unroll test."""
    res = _run_child(CHILD_MIXED_UNROLL, {"PMDFC_MIXED_SMALL": "0"})
    assert len(res) == 4 and all(res.values()), res


# While a table is coarser than its full bucket resolution a batch runs as
# sub-batches of max(PMDFC_RAMP_OPS << p1, PMDFC_RAMP_MIN) ops (ramp_batch).
# CCEH_hybrid(2) starts at p1 = 1; PMDFC_P1MAX=4 (a create knob, set here
# before the create) ends the ramp within the stream: the first 30,000 inserts
# of cap2_ins100k as Insert batches of 10,000, and as one MixedBatches call
# with a last batch of Gets.  (1, 1): sub-batches of 1 << p1 ops; (7, 100):
# 100, 100, 112-op sub-batches.
CHILD_RAMP = r'''
import json, os, sys, numpy as np
sys.path.insert(0, "tests")
import scenarios as S
from oracle import oracle as O
import pmdfc_amd as P
os.environ["PMDFC_P1MAX"] = "4"
init_cap, conv, ops, keys, vals = S.scenarios(O.hash64)["cap2_ins100k"]
n, batch = 30000, 10000
assert np.all(ops[:n] == S.OP_INSERT)
k, v = keys[:n], vals[:n]
out = {}
def table_equal(t, o):
    d, od = t.dump(), o.dump()
    return d["depth"] == od["depth"] and all(np.array_equal(d[f], od[f]) for f in ("local_depth", "keys", "values"))
t = P.CCEH(init_cap, convention=conv, max_batch=batch, max_segments=4096)
out["starts_coarse"] = t.stats()["bucket_bits"] == 1
o = O.OracleCCEH(t.initial_depth)
ok = True
for off in range(0, n, batch):
    ok = ok and bool(np.array_equal(t.Insert(k[off:off + batch], v[off:off + batch]), o.insert(k[off:off + batch], v[off:off + batch])))
out["insert"] = ok and table_equal(t, o)
out["insert/bucket_bits"] = t.stats()["bucket_bits"] == 4
out["insert/error_flags"] = t.stats()["error_flags"] == 0
t.close()
g = np.concatenate([k[:4000], keys[-4000:]])
mo = np.concatenate([ops[:n], np.zeros(g.size, np.uint8)])
mk = np.concatenate([k, g])
mv = np.concatenate([v, np.zeros(g.size, np.uint64)])
t = P.CCEH(init_cap, convention=conv, max_batch=batch, max_segments=4096)
o = O.OracleCCEH(t.initial_depth)
vo, st = t.MixedBatches(mo, mk, mv, [0, 10000, 20000, 30000, mk.size])
ov, ost = o.mixed(mo, mk, mv)
out["mixed"] = bool(np.array_equal(st, ost) and np.array_equal(vo, ov)) and table_equal(t, o)
out["mixed/bucket_bits"] = t.stats()["bucket_bits"] == 4
out["mixed/error_flags"] = t.stats()["error_flags"] == 0
t.close()
print(json.dumps(out))
'''


@pytest.mark.parametrize("ramp_ops,ramp_min", [("1", "1"), ("7", "100")])
def test_ramp_sub_batches_match_oracle(ramp_ops, ramp_min):
    res = _run_child(CHILD_RAMP, {"PMDFC_RAMP_OPS": ramp_ops, "PMDFC_RAMP_MIN": ramp_min})
    assert len(res) == 7 and all(res.values()), (ramp_ops, ramp_min, res)


@pytest.mark.parametrize("env", [{"PMDFC_FAST_LDS_PAD": "4096"}, {"PMDFC_PSTREAM_PRIO": "0"}],
                         ids=["fast_lds_pad", "pstream_prio0"])
def test_launch_shape_knobs_match_oracle(env):
    """Padding LDS onto the lean first pass's waves (lower occupancy) and the
    partition stream at default priority change scheduling, never results."""
    res = _run_child(CHILD, env)
    assert len(res) == 5 and all(res.values()), (env, res)


# PMDFC_STAMPS=1 with PMDFC_STAMP_ROT=3: three stamp sets, batch i writing set
# i % 3.  Five insert batches (20,000 ops: three k_part blocks each, each
# stamping its start in word 0 of its row) leave batch 3 in set 0, batch 4 in
# set 1 and batch 2 in set 2; a buffer of one set reads the last batch's, a
# buffer of all three reads them all.  A set, for depth 10 and max_batch 2^16
# as in test_debug_stamps_follow_the_batch: 16 words for each of the 2^9
# buckets, 8 for each of the 8 partition blocks, 8 for each of 8,192 splits.
CHILD_STAMP_ROT = r'''
import ctypes as C, json, numpy as np
from oracle import oracle as O
import pmdfc_amd as P
from pmdfc_amd.workload import uniform_keys
t = P.CCEH(depth=10, max_batch=1 << 16, max_segments=8192)
o = O.OracleCCEH(10)
keys = uniform_keys(702, 0, 100000)
vals = keys ^ np.uint64(3)
out = {}
ok = True
for off in range(0, keys.size, 20000):
    ok = ok and bool(np.array_equal(t.Insert(keys[off:off + 20000], vals[off:off + 20000]),
                                    o.insert(keys[off:off + 20000], vals[off:off + 20000])))
out["insert"] = ok
ask = np.concatenate([keys, uniform_keys(702, 100000, 5000)])
gv, gs = t.Get(ask)
ov, os_ = o.get(ask)
out["get"] = bool(np.array_equal(gv, ov) and np.array_equal(gs, os_))
d, od = t.dump(), o.dump()
out["table"] = d["depth"] == od["depth"] and all(np.array_equal(d[f], od[f]) for f in ("local_depth", "keys", "values"))
nbk, nblk = 512, 8
tot = 16 * nbk + 8 * nblk + 8 * 8192
L = P.load_library()
def read(words):
    buf = np.zeros(words, np.uint64)
    nb = C.c_uint32()
    rc = L.pmdfc_cceh_debug_stamps(t.handle, buf.ctypes.data, C.c_uint64(buf.size), C.byref(nb))
    return rc, nb.value, buf
rc1, nb1, one = read(tot)
rc3, nb3, three = read(3 * tot)
out["reads"] = rc1 == 0 and rc3 == 0 and nb1 == nbk and nb3 == nbk
sets = three.reshape(3, tot)
part = sets[:, 16 * nbk: 16 * nbk + 8 * nblk].reshape(3, nblk, 8)
out["every_set_written"] = bool(np.all(part[:, :3, 0] > 0) and np.all(part[:, 3:] == 0))
out["rotation"] = bool(part[2, 0, 0] < part[0, 0, 0] < part[1, 0, 0])
out["one_set_is_the_last_batch"] = bool(np.array_equal(one, sets[1]))
out["error_flags"] = t.stats()["error_flags"] == 0
t.close()
print(json.dumps(out))
'''


def test_stamp_rotation():
    res = _run_child(CHILD_STAMP_ROT, {"PMDFC_STAMPS": "1", "PMDFC_STAMP_ROT": "3"})
    assert len(res) == 8 and all(res.values()), res


# PMDFC_ROUTE_PIPE=1 (with PMDFC_ROUTE_DIRECT=0): routed inserts through the
# engine's partition pipeline (pipe_batch, with the exchange's events across
# the streams) -- taken only by a table at its full bucket resolution, so that
# is asserted first: max_batch = the packer's rows, p1max = floor(log2) - 7,
# and depth 12 is deeper.  CHILD_ROUTE's insert and Get sections at B = 2^16;
# 7 insert batches: past the third the pipeline waits for the unpack that last
# read its status buffer, and the record buffers wrap.
CHILD_ROUTE_PIPE = r'''
import json, sys, torch, numpy as np
import pmdfc_amd as P
from pmdfc_amd.dist import BlockRouter
B, nb = 1 << 16, 7
pk = P.BlockPacker(0, B, 0)
idx = P.CCEH(depth=12, max_batch=pk.rows, max_segments=1 << 14, device=0)
comm = P.Comm(0)
r = BlockRouter(idx, pk, comm=comm)
assert r._native()
out = {}
out["full_resolution"] = idx.stats()["bucket_bits"] == int(pk.rows).bit_length() - 1 - 7
direct = P.CCEH(depth=12, max_batch=B, max_segments=1 << 14, device=0)
keys = [P.gen_keys(900 + i, 0, B, device=0) for i in range(nb)]
st_r = r.insert_batches([(k, k) for k in keys])
out["insert"] = len(st_r) == nb and all(bool(torch.equal(a, direct.Insert(k, k))) for a, k in zip(st_r, keys))
q = [torch.cat([k[: B // 2], P.gen_keys(950 + i, 0, B // 2, device=0)]) for i, k in enumerate(keys)]
ok = True
for dd in (True, False):
    r.dedupe_gets = dd
    for (v, s), qq in zip(r.get_batches(q), q):
        vd, sd = direct.Get(qq)
        ok = ok and bool(torch.equal(v, vd) and torch.equal(s, sd))
out["get"] = ok
d, dd = idx.dump(), direct.dump()
out["table"] = d["depth"] == dd["depth"] and all(np.array_equal(d[f], dd[f]) for f in ("local_depth", "keys", "values"))
out["splits"] = idx.stats()["splits"] == direct.stats()["splits"]
out["error_flags"] = idx.stats()["error_flags"] == 0 and direct.stats()["error_flags"] == 0
print(json.dumps(out))
'''


def test_routed_inserts_through_the_pipeline():
    res = _run_child(CHILD_ROUTE_PIPE, {"PMDFC_ROUTE_DIRECT": "0", "PMDFC_ROUTE_PIPE": "1"})
    assert len(res) == 6 and all(res.values()), res
