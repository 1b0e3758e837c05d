"""The coarse-partition lean first pass (k_apply_fast_cp) at the edges of its
two-stage record staging, and the one-load occupancy window (ld_window_l2) at
the end of the occupancy row.

Geometry: a table of max_batch 65,536 whose initial depth is at least 9 is at
its full 2^9 directory buckets from the start, so an insert-only batch takes
the coarse partition when a sub-region's mean share is at most 128 records: 64
partition buckets of 8 directory buckets, k_part tile b (8,192 ops) writing
sub-region b % 8.  The keys are made from their hash (scenarios.unhash64): the
top hash bits are the segment (the top 9 the directory bucket), the low 8 the
home line.

counts   batch 1 has 65,536 ops (8 tiles, so all 8 sub-regions in use).
         Partition bucket X receives 0, 1, 127, 128, 129, 191, 192 and 64
         records from tiles 0-7 (taken: every count the second stage treats
         differently -- nothing, below, at and above its start at 128, its
         last slot and the whole staging); partition bucket Y 193, 0, 1, 127,
         128, 129, 191 and 192 (193 is past the staging: its 8 buckets
         decline).  Batch 2 has 20,000 ops (3 tiles): X 129, 192, 1; Y 193,
         128, 0.  The table starts at depth 12 (8 segments per bucket) and
         every key set is dealt over its segments in turn, the filler over
         those of all other partition buckets (about 128 records per whole
         tile and partition bucket, at most 160): a segment gets at most 17 inserts a batch, so no
         bucket is handed back for another reason (more than 32 dependent
         inserts in a segment, more than 192 inserts in a bucket), and the
         decline count is exact.
wrap     20,000-op batches into a table of depth 9 (one segment per bucket).
         Ten segments each get 32 keys of one home line
         -- 247, 248, ..., 255 and 0 -- which fill that line's 32-slot window
         exactly (across the end of the row for 249-255); then one more key of
         that line, alone in its bucket, whose window is full: it must request
         the split (default mode: the lean pass; upsert mode: the lean
         last-writer-wins pass, whose probe walks the same window), with
         inserts at lines 247 and 0 beside it; then the first keys again
         (default mode: stored twice; upsert mode: ST_UPDATED).  The filler
         keys of every batch are uniform, so ~1/32 of them have a home line in
         248-255 too.

The engine reads PMDFC_CP once per process, so each variant (default and
PMDFC_CP=0, the fine partition) is one child process that runs every scenario
and prints one JSON dict; the children run side by side, once per module.

Compared, for each scenario: every status after each batch, the final table
(dump) and insert_lines with the serial oracle, which keeps no segment_runs or
deferred_ops; those two, with insert_lines again, between the two variants.
fast_declined is path-dependent: in `counts` it is exactly Y's 8 buckets per
batch with the coarse partition and 0 with the fine one (whose buckets hold
~120 records each); in `wrap`, where no sub-region is past the staging, it is
equal between the variants (there a bucket's one segment takes ~39 inserts a
batch, and those with more than 32 dependent ones are handed back either way).
"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import json, sys, zlib, numpy as np
sys.path.insert(0, "tests")
import scenarios as S
from oracle import oracle as O
import pmdfc_amd as P

TILE, NB = 8192, 512
rng = np.random.default_rng(1307)
used = set()

def keys_at(prefix, home, pbits=9):
    """One key per element: top pbits hash bits (9: the directory bucket) and home line given, the rest random."""
    prefix, home = np.asarray(prefix, np.uint64), np.asarray(home, np.uint64)
    mid = rng.integers(0, 1 << (56 - pbits), prefix.size, dtype=np.uint64)
    k = S.unhash64((prefix << np.uint64(64 - pbits)) | (mid << np.uint64(8)) | home)
    assert np.array_equal(O.hash64(k) >> np.uint64(64 - pbits), prefix)
    return k

def fresh(k):
    s = set(k.tolist())
    assert len(s) == k.size and not (s & used)
    used.update(s)
    return k

def crc(*arrs):
    c = 0
    for a in arrs:
        c = zlib.crc32(np.ascontiguousarray(a).tobytes(), c)
    return c

def run(batches, upsert=False, depth=9):
    """Each batch through the engine and the oracle; what the parent compares."""
    t = P.CCEH(depth=depth, max_batch=1 << 16, max_segments=8192, upsert=upsert)
    o = O.OracleCCEH(depth, upsert=upsert)
    r = {"bucket_bits": int(t.stats()["bucket_bits"]), "status_ok": [], "splits": [], "declined": [], "status_crc": 0}
    for k, v in batches:
        st, ost = t.Insert(k, v), o.insert(k, v)
        r["status_ok"].append(bool(np.array_equal(st, ost)))
        r["status_crc"] = crc(st) ^ (r["status_crc"] * 31 & 0xFFFFFFFF)
        r["splits"].append(int(t.stats()["splits"]))
        r["declined"].append(int(t.stats()["fast_declined"]))
        r.setdefault("updated", []).append(int((st == P.ST_UPDATED).sum()))
    d, od = t.dump(), o.dump()
    r["dump_ok"] = bool(d["depth"] == od["depth"] and all(np.array_equal(d[f], od[f]) for f in ("local_depth", "keys", "values")))
    r["dump_crc"] = crc(d["local_depth"], d["keys"], d["values"])
    s, os_ = t.stats(), o.stats()
    r["stats"] = {f: int(s[f]) for f in ("segment_runs", "insert_lines", "deferred_ops", "fast_declined", "splits", "error_flags")}
    r["oracle"] = {"insert_lines": int(os_["insert_lines"]), "splits": int(os_["splits"])}
    t.close()
    return r

def filler(n, buckets):
    return keys_at(rng.choice(buckets, n), rng.integers(0, 256, n))

out = {}

# ---- counts: chosen record counts per (k_part tile, partition bucket)
X, Y = 5, 40
others = rng.permutation(np.array([s for s in range(NB * 8) if s >> 6 not in (X, Y)]))  # segments (top 12 hash bits)
dealt = 0

def deal(segs, n):
    """n keys over segs in turn, any home line."""
    global dealt
    i = (dealt + np.arange(n)) % segs.size
    dealt += n
    return keys_at(segs[i], rng.integers(0, 256, n), 12)

def counted_batch(n, cx, cy):
    tiles = []
    for b in range(-(-n // TILE)):
        size = min(TILE, n - b * TILE)
        part = [deal(X * 64 + np.arange(64), cx[b]), deal(Y * 64 + np.arange(64), cy[b]),
                deal(others, size - cx[b] - cy[b])]
        tiles.append(rng.permutation(np.concatenate(part)))
    k = fresh(np.concatenate(tiles))
    # (what k_part will count: records per tile and partition bucket)
    pb = (O.hash64(k) >> np.uint64(58)).astype(np.int64)
    cnt = np.stack([np.bincount(pb[b * TILE:(b + 1) * TILE], minlength=64) for b in range(len(tiles))])
    assert cnt[:, X].tolist() == list(cx[:len(tiles)]) and cnt[:, Y].tolist() == list(cy[:len(tiles)])
    rest = np.delete(cnt, [X, Y], axis=1)
    assert rest.max() <= 160, rest.max()
    assert np.bincount((O.hash64(k) >> np.uint64(52)).astype(np.int64)).max() <= 17
    return k, k ^ np.uint64(9)

cx1, cy1 = [0, 1, 127, 128, 129, 191, 192, 64], [193, 0, 1, 127, 128, 129, 191, 192]
cx2, cy2 = [129, 192, 1], [193, 128, 0]
out["counts"] = run([counted_batch(8 * TILE, cx1, cy1), counted_batch(20000, cx2, cy2)], depth=12)

# ---- wrap: windows at the end of the occupancy row
HOMES = [247, 248, 249, 250, 251, 252, 253, 254, 255, 0]
SEGS = [3 + 50 * i for i in range(len(HOMES))]
free = np.array([b for b in range(NB) if b not in SEGS])

def wrap_batches():
    B = 20000
    fill = fresh(np.concatenate([keys_at(np.full(32, s), np.full(32, h)) for s, h in zip(SEGS, HOMES)]))
    one = fresh(np.concatenate([keys_at([s, s, s], [h, 247, 0]) for s, h in zip(SEGS, HOMES)]))
    b = []
    for crafted in (fill, one, fill):
        k = rng.permutation(np.concatenate([crafted, fresh(filler(B - crafted.size, free))]))
        b.append((k, k ^ np.uint64(len(b) + 3)))
    return b

wb = wrap_batches()
out["wrap"] = run(wb)
out["wrap_upsert"] = run(wb, upsert=True)
print(json.dumps(out))
'''

ENVS = {"default": {}, "cp0": {"PMDFC_CP": "0"}}
SCENARIOS = ("counts", "wrap", "wrap_upsert")


@pytest.fixture(scope="module")
def res():
    procs = {}
    for name, env in ENVS.items():
        e = dict(os.environ)
        for k in ("PMDFC_CP", "PMDFC_FAST_APPLY", "PMDFC_CHUNK", "PMDFC_P1MAX", "PMDFC_STAMPS"):
            e.pop(k, None)
        e.update(env)
        procs[name] = subprocess.Popen([sys.executable, "-c", CHILD], cwd=REPO, env=e, stdout=subprocess.PIPE,
                                       stderr=subprocess.PIPE, text=True)
    out = {}
    for name, p in procs.items():
        o, err = p.communicate(timeout=600)
        assert p.returncode == 0, (name, err[-3000:])
        out[name] = json.loads(o.strip().splitlines()[-1])
    for name, r in out.items():
        for sc in SCENARIOS:
            print(name, sc, r[sc]["stats"], "declined", r[sc]["declined"], "splits", r[sc]["splits"])
    return out


@pytest.mark.parametrize("scenario", SCENARIOS)
@pytest.mark.parametrize("variant", list(ENVS))
def test_statuses_table_and_lines_equal_the_oracle(res, variant, scenario):
    r = res[variant][scenario]
    assert r["bucket_bits"] == 9  # full resolution from the first batch: the default takes the coarse partition
    assert all(r["status_ok"]), r["status_ok"]
    assert r["dump_ok"]
    assert r["stats"]["error_flags"] == 0
    assert r["stats"]["insert_lines"] == r["oracle"]["insert_lines"]
    assert r["stats"]["splits"] == r["oracle"]["splits"]


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_both_partitions_keep_the_same_books(res, scenario):
    a, b = res["default"][scenario], res["cp0"][scenario]
    assert a["status_crc"] == b["status_crc"] and a["dump_crc"] == b["dump_crc"]
    for f in ("segment_runs", "insert_lines", "deferred_ops", "splits"):
        assert a["stats"][f] == b["stats"][f], (f, a["stats"][f], b["stats"][f])
    if scenario != "counts":  # (no sub-region past the staging: the same buckets decline either way)
        assert a["declined"] == b["declined"], (a["declined"], b["declined"])


def test_a_sub_region_past_the_staging_declines_its_partition_bucket(res):
    """193 records in one sub-region: the 8 buckets of that partition bucket
    decline, in each of the two batches, and no other bucket does (192 is
    taken); the fine partition, which stages per directory bucket, takes all."""
    assert res["default"]["counts"]["declined"] == [8, 16]
    assert res["cp0"]["counts"]["declined"] == [0, 0]
    assert res["default"]["counts"]["splits"] == [0, 0]  # (at most 34 keys per 1,024-slot segment)


@pytest.mark.parametrize("scenario", ("wrap", "wrap_upsert"))
@pytest.mark.parametrize("variant", list(ENVS))
def test_a_window_full_across_the_row_end_requests_the_split(res, variant, scenario):
    """Batch 1 fills ten windows exactly and splits nothing; in batch 2 the one
    more key of each of those home lines finds its window full and splits its
    segment -- exactly those ten (the uniform filler, ~39 keys per segment and
    batch, fills no window)."""
    r = res[variant][scenario]
    assert r["splits"][0] == 0 and r["splits"][1] == 10, r["splits"]
    # batch 3 stores the 320 first keys again: updates in upsert mode only
    assert r["updated"] == ([0, 0, 320] if scenario == "wrap_upsert" else [0, 0, 0]), r["updated"]
