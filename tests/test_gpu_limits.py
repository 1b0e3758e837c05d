"""Arena and pool exhaustion on every insert path, and deep hash chains.

A production table runs until memory is full, so every one ends up answering
PMDFC_ST_CAPACITY.  run_to_exhaustion drives an engine through a stream that
overfills it and checks after every batch (dump() and stats()):
  (a) exact prefix: until the first batch with a CAPACITY, every op and the
      table equal the serial oracle;
  (b) structure and accounting: limits_ref.check_table, and the stored pairs
      are exactly those answered INSERTED (check_accounting; no split drops
      an entry: split_loss == 0 is asserted, the streams are chosen for it);
  (c) justified failure: an op answered CAPACITY finds its window full in the
      table after the batch (nothing is deleted, so a window that was full
      stays full); a Get of a key the batch never inserts answers as on the
      table before the batch;
  (d) frozen exactness: a batch across which the segment count did not change
      equals limits_ref.FrozenTable -- the serial table that cannot split --
      status by status, value by value and slot by slot.  Every case sees at
      least 3 such batches, one with a CAPACITY in it;
  (e) error flags: bit 1 (sub-directory pool exhausted) stays clear where the
      arena runs out first, bit 2 (round guard) everywhere.
The cases (scenarios.LIMIT_CASES) run it over every way an insert is applied;
the ones that need a process knob run this file as a child process.  Then:
UNSPLITTABLE before CAPACITY, snapshots of exhausted tables, recovery by
reset() and load(), and chains of splits under a long common hash prefix
(scenarios.deep_chain_stream, built with unhash64), inside the pool and past it.
Bit-exact throughout.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import scenarios as S  # (first: it puts the repository root on sys.path for a child process)
import limits_ref as R
from oracle import oracle as O
from pmdfc_amd.workload import uniform_keys

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pmdfc_amd as P  # noqa: E402
from pmdfc_amd import image as I  # noqa: E402
from pmdfc_amd.kv import KV  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONES = lambda n: np.full(n, S.OP_INSERT, np.uint8)  # noqa: E731


def _eq(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.nonzero(a != b)[0]
    assert bad.size == 0, (what, f"{bad.size} of {a.size} differ, first at {int(bad[0])}: "
                           f"{a[bad[:4]].tolist()} != {b[bad[:4]].tolist()}")


def _same_table(got, want, what):
    assert int(got["depth"]) == int(want["depth"]), (what, "depth", got["depth"], want["depth"])
    for f in ("local_depth", "prefix", "keys", "values"):
        _eq(np.asarray(got[f], np.uint64), np.asarray(want[f], np.uint64), (what, f))


def run_to_exhaustion(t, batches, max_segments, upsert=False, arena=True, oracle=None, history=None):
    """Apply batches -- (ops, keys, values), ops None for a pure Insert -- to
    engine t (anything with Insert, Mixed, dump and stats) and check (a)-(e)
    after each.  oracle: the serial oracle in the table's state, or None to
    skip (a).  history: the (keys, values) lists of the pairs stored so far,
    extended here.  Returns the counts a case asserts on and every status."""
    ik, iv = history if history is not None else ([], [])
    before, sb = t.dump(), t.stats()
    info = dict(batches=0, exact=0, frozen=0, frozen_capacity=0, capacity=0, first_capacity=None, status=[])
    for b, (ops, keys, vals) in enumerate(batches):
        if ops is None:
            ops, vo, st = ONES(keys.size), np.zeros(keys.size, np.uint64), t.Insert(keys, vals)
        else:
            vo, st = t.Mixed(ops, keys, vals)
        after, sa = t.dump(), t.stats()
        ins = ops == S.OP_INSERT
        cap = st == P.ST_CAPACITY
        what = f"batch {b}"
        ok_ins = [P.ST_INSERTED, P.ST_CAPACITY, P.ST_UNSPLITTABLE] + ([P.ST_UPDATED] if upsert else [])
        assert np.all(np.isin(st[ins], ok_ins)), (what, np.unique(st[ins]).tolist())
        assert np.all(np.isin(st[~ins], [P.ST_HIT, P.ST_MISS])), (what, np.unique(st[~ins]).tolist())
        assert not np.any(vo[st != P.ST_HIT]), (what, "a value without a HIT")
        # (a) exact prefix
        if oracle is not None and not cap.any():
            ov, ost = oracle.mixed(ops, keys, vals)
            _eq(st, ost, (what, "(a) status"))
            _eq(vo, ov, (what, "(a) values"))
            _same_table(after, oracle.dump(), (what, "(a)"))
            info["exact"] += 1
        else:
            oracle = None
        # (b) structure and accounting
        assert sa["split_loss"] == 0, (what, "split_loss", sa["split_loss"])
        R.check_table(after, sa, max_segments)
        k, v = R.stored_pairs(keys[ins], vals[ins], st[ins])
        ik.append(k)
        iv.append(v)
        R.check_accounting(after, (np.concatenate(ik), np.concatenate(iv)), upsert=upsert)
        # (c) justified failure
        fa = R.FrozenTable(after, upsert=upsert)
        for key in np.unique(keys[cap]).tolist():
            assert fa.insert(key) == R.ST_CAPACITY, (what, "(c) CAPACITY with room in the window", key)
        if not ins.all():
            g = ~ins & ~np.isin(keys, keys[ins])
            gv, gs = R.FrozenTable(before).mixed(ops[g], keys[g], vals[g])
            _eq(st[g], gs, (what, "(c) Get status"))
            _eq(vo[g], gv, (what, "(c) Get value"))
        # (d) frozen exactness
        if sa["segments"] == sb["segments"]:
            fz = R.FrozenTable(before, upsert=upsert)
            zv, zs = fz.mixed(ops, keys, vals)
            _eq(st, zs, (what, "(d) status"))
            _eq(vo, zv, (what, "(d) values"))
            _same_table(after, fz.image(), (what, "(d)"))
            info["frozen"] += 1
            info["frozen_capacity"] += int(cap.any())
        # (e) error flags
        assert sa["error_flags"] & (3 if arena else 2) == 0, (what, "error_flags", sa["error_flags"])
        if cap.any() and info["first_capacity"] is None:
            info["first_capacity"] = b
        info["capacity"] += int(cap.sum())
        info["batches"] += 1
        info["status"].append(st)
        before, sb = after, sa
    info["stats"] = sb
    return info


def _case_stream(c):
    ms = (1 << c["depth"]) + c["extra"]
    keys, vals = (S.limit_upsert_stream if c.get("upsert") else S.limit_stream)(c["seed"], ms)
    if "gets" in c:
        return ms, S.limit_mixed_batches(c["seed"], keys, vals, c["batch"], c["gets"])
    return ms, [(None, keys[a:a + c["batch"]], vals[a:a + c["batch"]]) for a in range(0, keys.size, c["batch"])]


def run_case(name):
    """One row of scenarios.LIMIT_CASES, in this process (its knobs are set by the caller)."""
    c = S.LIMIT_CASES[name]
    ms, batches = _case_stream(c)
    upsert = bool(c.get("upsert"))
    t = P.CCEH(depth=c["depth"], max_batch=c["max_batch"], max_segments=ms, upsert=upsert)
    info = run_to_exhaustion(t, batches, ms, upsert=upsert, oracle=O.OracleCCEH(c["depth"], upsert=upsert))
    st = info.pop("stats")
    info.pop("status")
    assert info["frozen"] >= 3 and info["frozen_capacity"] >= 1, info
    p1max = max(c["max_batch"].bit_length() - 1 - 7, 0)
    if name.startswith(("medium", "mixed_medium")):  # at full bucket resolution: the batches took k_part + k_medium
        assert st["bucket_bits"] == p1max, (st["bucket_bits"], p1max)
    if name == "general2000_ramp":  # below it to the end: every batch ran as ramp sub-batches
        assert st["bucket_bits"] < p1max, (st["bucket_bits"], p1max)
    t.close()
    info["stats"] = {k: st[k] for k in ("segments", "bucket_bits", "max_rounds", "fast_declined", "error_flags", "splits")}
    return info


def _child(name, env):
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), name], cwd=REPO, env=e, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, (name, f"returncode={r.returncode}", r.stdout[-1500:], r.stderr[-3000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("name", list(S.LIMIT_CASES))
def test_exhaustion(name):
    env = S.LIMIT_CASES[name].get("env")
    info = _child(name, env) if env else run_case(name)
    print(name, json.dumps(info))


def _bounds(n, batch):
    return list(range(0, n, batch)) + [n]


class _Pipelined:
    """Insert as one pipelined Insert_batches call over sub-batches of `batch` ops."""

    def __init__(self, t, batch):
        self.t, self.batch, self.dump, self.stats = t, batch, t.dump, t.stats

    def Insert(self, keys, vals):
        return self.t.InsertBatches(keys, vals, _bounds(keys.size, self.batch))


def test_exhaustion_pipelined_insert_batches():
    """Insert_batches partitions the batches that follow the exhausting one
    before it runs.  Each call here pipelines three batches; (a)-(e) are
    checked call by call (the table cannot be read inside a call), so a call
    across which nothing split must equal FrozenTable over its three batches
    in order."""
    c = S.LIMIT_PIPELINED
    ms = (1 << c["depth"]) + c["extra"]
    keys, vals = S.limit_stream(c["seed"], ms)
    t = P.CCEH(depth=c["depth"], max_batch=c["max_batch"], max_segments=ms)
    assert t.stats()["bucket_bits"] == c["depth"]  # full bucket resolution: the call pipelines from its first batch
    call = 3 * c["batch"]
    batches = [(None, keys[a:a + call], vals[a:a + call]) for a in range(0, keys.size, call)]
    info = run_to_exhaustion(_Pipelined(t, c["batch"]), batches, ms, oracle=O.OracleCCEH(c["depth"]))
    assert info["frozen"] >= 3 and info["frozen_capacity"] >= 1, {k: info[k] for k in ("frozen", "frozen_capacity")}
    assert info["first_capacity"] is not None and info["batches"] == len(batches)


class _Served:
    """The served front-end as run_to_exhaustion's engine: one caller, one
    ring, so the ring places are the call order."""

    def __init__(self, kv, mode):
        self.kv, self.mode, self.dump, self.stats = kv, mode, kv.dump, kv.stats

    def Mixed(self, ops, keys, vals):
        if self.mode == "async":
            vo, st, pl = self.kv.ops_async(ops, keys, vals)
        else:  # runs of 1, 7, 64 and 200 ops
            n = ops.size
            vo, st, pl = np.zeros(n, np.uint64), np.zeros(n, np.uint8), np.zeros(n, np.uint64)
            a = 0
            while a < n:
                for r in (1, 7, 64, 200):
                    b = min(n, a + r)
                    if b > a:
                        vo[a:b], st[a:b], pl[a:b] = self.kv.ops(ops[a:b], keys[a:b], vals[a:b], run=b - a)
                    a = b
        assert np.array_equal(pl, pl[0] + np.arange(pl.size, dtype=np.uint64)), "ring places out of call order"
        return vo, st

    def Insert(self, keys, vals):
        return self.Mixed(ONES(keys.size), keys, vals)[1]


@pytest.mark.parametrize("mode", ["burst", "async"])
def test_exhaustion_served_front_end(mode):
    """The served KV front-end over an exhausting stream of Inserts: (a)-(e)
    per chunk; its failure counter counts exactly the CAPACITY answers (the
    stream holds no other failure); an attached counting filter misses no
    stored key."""
    c = S.LIMIT_SERVED
    ms = (1 << c["depth"]) + c["extra"]
    keys, vals = S.limit_stream(c["seed"], ms)
    cfg = dict(ring_size=256) if mode == "burst" else dict(ring_size=1 << 13, flood_ops=1024)
    kv = KV(depth=c["depth"], max_batch=c["max_batch"], max_segments=ms, serve_waves=1, **cfg)
    f = P.CountingBloomFilter(4, 1 << 20)
    kv.attach_counting_bf(f)
    batches = [(None, keys[a:a + c["batch"]], vals[a:a + c["batch"]]) for a in range(0, keys.size, c["batch"])]
    info = run_to_exhaustion(_Served(kv, mode), batches, ms, oracle=O.OracleCCEH(c["depth"]))
    assert info["frozen"] >= 3 and info["frozen_capacity"] >= 1, info
    st = np.concatenate(info["status"])
    assert np.all(np.isin(st, [P.ST_INSERTED, P.ST_CAPACITY]))
    ph = kv.phase()
    assert ph["failed_ops"] == info["capacity"] == int((st == P.ST_CAPACITY).sum()), (ph, info["capacity"])
    if mode == "async":
        assert ph["flood_batches"] > 0
    stored, missing = kv.audit_filter()
    d = kv.dump()
    assert stored == int(np.count_nonzero(d["keys"] != np.uint64(R.INVALID))) == int((st == P.ST_INSERTED).sum())
    assert missing == 0
    kv.close()


def _exhaust(t, keys, vals, batch):
    """The whole stream in Insert batches -> every status."""
    return np.concatenate([t.Insert(keys[a:a + batch], vals[a:a + batch]) for a in range(0, keys.size, batch)])


def test_unsplittable_before_capacity():
    """On an exhausted table a 33rd copy of a key whose 32 copies fill its
    window answers UNSPLITTABLE, another key of that window CAPACITY (the run
    loop tests the all-same window before it looks at the arena), alone in a
    small batch and inside a general one."""
    depth, ms = 2, 6
    k = S.keys_from_hash_fields(2, 2, 77, 2)  # two keys of segment 2, home line 77
    keys, vals = S.limit_stream(12, ms)
    t = P.CCEH(depth=depth, max_batch=16384, max_segments=ms)
    hist = ([np.full(32, k[0], np.uint64)], [np.arange(1, 33, dtype=np.uint64)])
    _eq(t.Insert(hist[0][0], hist[1][0]), np.full(32, P.ST_INSERTED), "32 copies")
    st = _exhaust(t, keys[:15000], vals[:15000], 9000)
    hist[0].append(keys[:15000][st == P.ST_INSERTED])
    hist[1].append(vals[:15000][st == P.ST_INSERTED])
    assert np.any(st == P.ST_CAPACITY)
    f = R.FrozenTable(t.dump())
    assert f.insert(int(k[0]), 33) == R.ST_UNSPLITTABLE and f.insert(int(k[1]), 1) == R.ST_CAPACITY  # (the construction)
    more = uniform_keys(112, 0, 9100)
    mv = more ^ np.uint64(0x33)
    batches = [(None, k, np.array([33, 34], np.uint64)),
               (None, np.concatenate([more[:4000], k, more[4000:9000]]), np.concatenate([mv[:4000], k, mv[4000:9000]])),
               (None, k[::-1].copy(), np.array([35, 36], np.uint64)),
               (None, np.concatenate([more[9000:9100], k]), np.concatenate([mv[9000:9100], k]))]
    info = run_to_exhaustion(t, batches, ms, history=hist)
    assert info["frozen"] == 4 and info["frozen_capacity"] == 4
    assert info["status"][0].tolist() == [P.ST_UNSPLITTABLE, P.ST_CAPACITY]
    assert info["status"][1][4000:4002].tolist() == [P.ST_UNSPLITTABLE, P.ST_CAPACITY]
    assert info["status"][2].tolist() == [P.ST_CAPACITY, P.ST_UNSPLITTABLE]
    assert info["status"][3][-2:].tolist() == [P.ST_UNSPLITTABLE, P.ST_CAPACITY]


def _stored(d):
    live = d["keys"] != np.uint64(R.INVALID)
    return d["keys"][live], d["values"][live]


def _check_snapshot(t, tmp_path, d0, max_segments):
    """save / save(packed) of table t validate and are the canonical image of
    its dump; a fresh engine loads either back to the same dump; items() is
    the stored pairs; Utilization is stored / slots."""
    d, s = t.dump(), t.stats()
    R.check_table(d, s, max_segments)
    for packed in (False, True):
        path = str(tmp_path / f"img{int(packed)}")
        t.save(path, packed=packed)
        raw = open(path, "rb").read()
        h = (I.validate_packed if packed else I.validate)(raw)
        assert h["nseg"] == len(d["local_depth"])
        assert raw == (I.packed_from_dump if packed else I.image_from_dump)(d, d0)
        fresh = P.CCEH(depth=d0, max_batch=4096, max_segments=max(max_segments + 8, 4096))
        fresh.load(path)
        _same_table(fresh.dump(), d, ("load", packed))
        assert fresh.stats()["segments"] == len(d["local_depth"])
        fresh.close()
    sk, sv = _stored(d)
    ik, iv = t.items()
    _eq(ik.cpu().numpy().view(np.uint64), sk, "items keys")
    _eq(iv.cpu().numpy().view(np.uint64), sv, "items values")
    assert t.Utilization() == pytest.approx(100.0 * sk.size / (len(d["local_depth"]) * 1024), rel=1e-12)
    f = P.CountingBloomFilter(4, 1 << 20)
    assert f.rebuild(t) == sk.size
    assert f.audit(t) == (sk.size, 0)
    _same_table(t.dump(), d, "the table after its snapshots")


@pytest.mark.parametrize("depth,extra,max_batch,batch", [(2, 7, 1000, 1000), (6, 7, 65536, 65536)],
                         ids=["medium_d2", "general_d6"])
def test_snapshot_after_exhaustion(tmp_path, depth, extra, max_batch, batch):
    """The segment counter overshoots max_segments when the final pass runs
    out of ids; everything that walks the arena still sees max_segments live
    segments."""
    ms = (1 << depth) + extra
    keys, vals = S.limit_stream(13 if depth == 2 else 15, ms)
    t = P.CCEH(depth=depth, max_batch=max_batch, max_segments=ms)
    st = _exhaust(t, keys, vals, batch)
    assert np.any(st == P.ST_CAPACITY)
    R.check_accounting(t.dump(), R.stored_pairs(keys, vals, st))
    _check_snapshot(t, tmp_path, depth, ms)


def test_recovery_reset_and_load(tmp_path):
    """An exhausted engine is not frozen for good: after reset() it splits
    again (a stream that fits equals the oracle from scratch, flags and
    counters restarted), and after load() of a smaller image too."""
    depth, ms = 2, 11
    keys, vals = S.limit_stream(13, ms)
    t = P.CCEH(depth=depth, max_batch=16384, max_segments=ms)
    st = _exhaust(t, keys, vals, 9000)
    assert np.any(st == P.ST_CAPACITY)
    # a stream that fits: the oracle needs fewer than ms segments for it
    fit_k, fit_v = uniform_keys(31, 0, 3600), uniform_keys(31, 0, 3600) ^ np.uint64(0xF17)
    o = O.OracleCCEH(depth)
    ost = o.insert(fit_k, fit_v)
    assert 4 < o.num_segments < ms and np.all(ost == O.ST_INSERTED) and o.stats()["split_loss"] == 0
    t.reset()
    s0 = t.stats()
    assert s0["segments"] == 4 and s0["error_flags"] == 0 and s0["splits"] == 0
    for batch in (9000, 700, 100):  # general, medium (once at full resolution) and small
        t.reset()
        _eq(_exhaust(t, fit_k, fit_v, batch), ost, ("after reset", batch))
        _same_table(t.dump(), o.dump(), ("after reset", batch))
        assert t.stats()["error_flags"] == 0 and t.stats()["segments"] == o.num_segments
    # load: exhaust again, then restore the image of the first 1,200 inserts and go on
    for batch in (9000, 700, 100):
        st = _exhaust(t, keys, vals, 9000)
        assert np.any(st[-9000:] == P.ST_CAPACITY)
        o = O.OracleCCEH(depth)
        o.insert(fit_k[:1200], fit_v[:1200])
        small = o.num_segments
        path = str(tmp_path / "small.img")
        with open(path, "wb") as fh:
            fh.write(I.image_from_dump(o.dump(), depth))
        t.load(path)
        assert t.stats()["segments"] == small and t.stats()["error_flags"] == 0
        _same_table(t.dump(), o.dump(), "loaded")
        _eq(_exhaust(t, fit_k[1200:], fit_v[1200:], batch), o.insert(fit_k[1200:], fit_v[1200:]), ("after load", batch))
        assert o.num_segments > small, "the stream after the load must split"
        _same_table(t.dump(), o.dump(), ("after load", batch))
        assert t.stats()["error_flags"] == 0


# ---- deep chains: a few segments under a long common hash prefix

DEEP_MAX_BATCH = 1 << 16  # p1max = 9 = DEEP_CHAIN_DEPTH: full bucket resolution from the start


def _deep_max_segments(D, groups=3):
    """The sizing rule of pmdfc_cceh_create: the pool holds
        max(4 * 2^depth, 8 << ceil_log2(max_segments)) + 4096 + (128 << p1max)
    entries, the last term being the buckets' fixed slots (sub-directories of
    up to 7 bits grow there in place).  A chain to local depth D grows its
    bucket's sub-directory a bit at a time to D - p1 bits and leaks every
    region it leaves: fewer than 2^(D - p1 + 1) entries in all.  max_segments
    is the smallest power of two that keeps the leaks of all the groups
    within a quarter of the 8 << ceil_log2(max_segments) term."""
    leak = groups << (D - S.DEEP_CHAIN_DEPTH + 1)
    ms = 2048
    while 8 * ms < 4 * leak:
        ms *= 2
    return ms


_DEEP = {}


def _deep_reference(D, seed):
    """The oracle's answers for the deep-chain stream, once per D."""
    if D not in _DEEP:
        keys, vals, groups = S.deep_chain_stream(D, seed)
        o = O.OracleCCEH(S.DEEP_CHAIN_DEPTH)
        r = dict(keys=keys, vals=vals, groups=groups, st=o.insert(keys, vals))
        rng = np.random.default_rng(seed)
        r["q"] = np.concatenate([keys, uniform_keys(seed + 1, 0, 3000), np.concatenate(groups)])
        r["q"] = r["q"][rng.permutation(r["q"].size)]
        r["get"] = o.get(r["q"])
        # (the oracle's FindAnyway walks all 2^D directory entries for every key: a few keys at D = 22)
        r["qfa"] = np.concatenate([groups[0][:1], groups[-1][32:], uniform_keys(seed + 1, 0, 1),
                                   keys[:max(1, 600 >> max(0, 2 * (D - 12) - 3))]])
        r["findany"] = o.find_anyway(r["qfa"])
        r["dump"] = o.dump()
        # a mixed batch: Gets of stored and absent keys among inserts of fresh keys next to the chains
        near = np.concatenate([S.keys_from_hash_fields(int(O.hash64(g[:1])[0] >> np.uint64(65 - D)), D - 1, 40, 20,
                                                       first=64) for g in groups])
        mk = np.concatenate([r["q"][:6000], near, uniform_keys(seed + 2, 0, 3000)])
        mo = np.concatenate([np.zeros(6000, np.uint8), ONES(near.size + 3000)])
        p = rng.permutation(mk.size)
        r["mixed_in"] = (mo[p], mk[p], np.where(mo[p] == 1, mk[p] ^ np.uint64(0x3D), np.uint64(0)).astype(np.uint64))
        r["mixed"] = o.mixed(*r["mixed_in"])
        r["dump2"] = o.dump()
        assert o.stats()["split_loss"] == 0 and o.depth == D
        _DEEP[D] = r
    return _DEEP[D]


@pytest.mark.parametrize("batch", [64, 4096, 65536])
@pytest.mark.parametrize("D,seed", S.DEEP_CHAIN_CASES)
def test_deep_chains_inside_the_pool(D, seed, batch):
    """Groups of 33 keys with a common hash prefix of D - 1 bits force chains
    of splits to local depth D over a few segments: a directory of depth D
    (D = 22: past the flat directory of pure-Get batches) with about 540
    segments.  Batches of 64, 4,096 and 65,536 ops walk the chain in the
    small, the medium and the general passes.  Everything equals the oracle."""
    r = _deep_reference(D, seed)
    ms = _deep_max_segments(D)
    t = P.CCEH(depth=S.DEEP_CHAIN_DEPTH, max_batch=DEEP_MAX_BATCH, max_segments=ms)
    assert t.stats()["bucket_bits"] == S.DEEP_CHAIN_DEPTH
    _eq(_exhaust(t, r["keys"], r["vals"], batch), r["st"], "insert status")
    s = t.stats()
    assert s["depth"] == D and s["error_flags"] == 0 and s["split_loss"] == 0
    assert s["segments"] == len(r["dump"]["local_depth"])
    _same_table(t.dump(), r["dump"], "table")
    for name, got, want in (("Get", t.Get(r["q"]), r["get"]), ("FindAnyway", t.FindAnyway(r["qfa"]), r["findany"])):
        _eq(got[1], want[1], (name, "status"))
        _eq(got[0], want[0], (name, "values"))
    img = t.snapshot().cpu().numpy().tobytes()
    assert img == I.image_from_dump(r["dump"], S.DEEP_CHAIN_DEPTH)
    t2 = P.CCEH(depth=S.DEEP_CHAIN_DEPTH, max_batch=DEEP_MAX_BATCH, max_segments=ms)
    t2.restore(t.snapshot(packed=True))
    _same_table(t2.dump(), r["dump"], "restored")
    for e in (t, t2):  # the restored table goes on as the original does
        mv, mst = e.Mixed(*r["mixed_in"])
        _eq(mst, r["mixed"][1], "mixed status")
        _eq(mv, r["mixed"][0], "mixed values")
        _same_table(e.dump(), r["dump2"], "table after the mixed batch")
        assert e.stats()["error_flags"] == 0 and e.stats()["split_loss"] == 0
        e.close()


@pytest.mark.parametrize("path", list(S.DEEP_POOL_CASES))
def test_deep_chain_past_the_pool(tmp_path, path):
    """The same chains on a table whose pool is far smaller than they need
    (4,096 + 1,024 entries beyond the fixed slots at 5 bucket bits, where one
    chain to depth 22 leaks over 250,000; 4,096 + 2,048 at 7, where it leaks
    over 60,000): the pool runs out inside a chain.  The blocked inserts answer
    CAPACITY, error flag 1 is set, the arena is not used up; (b), (c) and (d)
    hold, every stored key is still a HIT, and inserts elsewhere still
    succeed.  The triggers are retried three more times: nothing changes.  In
    the general case the chains run out in the first batch's final pass and
    the retries are denied by the split round of two more general batches,
    then by a small batch."""
    c = S.DEEP_POOL_CASES[path]
    batch = c["batch"]
    keys, vals, groups = S.deep_chain_stream(c["D"], c["seed"], c["groups"], c["n_uniform"], c["depth"])
    ms = c["max_segments"]
    t = P.CCEH(depth=c["depth"], max_batch=c["max_batch"], max_segments=ms)
    assert t.stats()["bucket_bits"] == c["depth"]
    last = np.array([g[32] for g in groups], np.uint64)  # each chain's trigger
    T = c["tail"]
    more = uniform_keys(c["seed"] + 5, 0, 3 * T)
    tail = np.concatenate([more[:T], last, more[T:2 * T], last, more[2 * T:], last])
    keys = np.concatenate([keys, tail])
    vals = np.concatenate([vals, tail ^ np.uint64(0x7A11)])
    batches = [(None, keys[a:a + batch], vals[a:a + batch]) for a in range(0, keys.size, batch)]
    hist = ([], [])
    info = run_to_exhaustion(t, batches, ms, arena=False, oracle=O.OracleCCEH(c["depth"]), history=hist)
    st = np.concatenate(info["status"])
    s = info["stats"]
    assert info["capacity"] > 0 and s["error_flags"] & 1 == 1, (info["capacity"], s["error_flags"])
    assert info["frozen"] >= 3 and info["frozen_capacity"] >= 1, {k: info[k] for k in ("frozen", "frozen_capacity")}
    assert np.all(np.isin(keys[st == P.ST_CAPACITY], last)), "only the chains' triggers may fail"
    assert s["segments"] < ms
    assert np.all(st[-tail.size:][~np.isin(tail, last)] == P.ST_INSERTED)  # windows with room still take keys
    ok = st == P.ST_INSERTED
    gv, gs = t.Get(keys)
    assert np.all(gs[ok] == P.ST_HIT) and np.array_equal(gv[ok], vals[ok])
    assert np.all(gs[~ok] == P.ST_MISS)
    _check_snapshot(t, tmp_path, c["depth"], ms)


if __name__ == "__main__":
    print(json.dumps(run_case(sys.argv[1])))
