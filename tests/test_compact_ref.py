"""The model of Compact (tests/compact_ref.py) on the CPU: on tables the
serial oracle builds from fixture streams, thinned by the Erase model, the rule
keeps every property DESIGN.md 4.9 lists -- the structure every probe relies on
(limits_ref.check_table, whose last assertion is Invariant I), every stored
pair exactly once, every key's Get and its copies in probe order, no segment
below the initial depth, a fixpoint that does not depend on the order the
pairs are taken in, and idempotence.  And the engine's C-ABI carries the new
entry point.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import compact_ref as CR
import erase_ref as E
import limits_ref as R
import scenarios as S
from conftest import REPO
from oracle import oracle as O

STREAMS = ["cap2_ins3k", "mixed_cap2_30k_ins80", "dup_wrap", "dup32", "dup_pairs", "cap8_ins20k"]
FRACTIONS = [0.5, 0.9]
LIMITS = [256, 512, 1024]
ERASE_SEED = 1234  # with it the cases below see no merge, >= 3 rounds, a drop refusal and the floor (test_suite_reaches_every_branch)
_TABLES, _CASES = {}, {}


def erased_table(name, frac):
    """(dump after the erase, initial depth, up to 3,000 staying keys): fixture
    stream `name` through the serial oracle, then a seeded fraction of its
    distinct keys erased by the Erase model.  Built once, never changed."""
    if (name, frac) not in _TABLES:
        init_cap, conv, ops, keys, vals = S.scenarios(O.hash64)[name]
        d0 = O.OracleCCEH.depth_for_hybrid(init_cap) if conv == "hybrid" else O.OracleCCEH.depth_for_src(init_cap)
        o = O.OracleCCEH(d0)
        o.mixed(ops, keys, vals)
        dump = o.dump()
        o.close()
        rng = np.random.default_rng(ERASE_SEED)
        distinct = np.unique(np.asarray(keys, np.uint64)[np.asarray(ops) == O.OP_INSERT])
        distinct = distinct[distinct < np.uint64(R.SENTINEL)]
        gone = rng.random(distinct.size) < frac
        t = E.ErasableTable(dump)
        t.erase_batch(distinct[gone])
        stay = distinct[~gone]
        _TABLES[(name, frac)] = (t.image(), d0, stay[rng.permutation(stay.size)[:3000]])
    return _TABLES[(name, frac)]


def compacted(name, frac, limit):
    if (name, frac, limit) not in _CASES:
        pre, d0, _ = erased_table(name, frac)
        _CASES[(name, frac, limit)] = CR.compact(pre, d0, limit)
    return _CASES[(name, frac, limit)]


def _pairs_sorted(d):
    k, v = np.asarray(d["keys"], np.uint64), np.asarray(d["values"], np.uint64)
    live = k != np.uint64(R.INVALID)
    p = np.stack([k[live], v[live]], axis=1)
    return p[np.lexsort((p[:, 1], p[:, 0]))]


@pytest.mark.parametrize("limit", LIMITS)
@pytest.mark.parametrize("frac", FRACTIONS)
@pytest.mark.parametrize("name", STREAMS)
def test_model_properties(name, frac, limit):
    pre, d0, stay = erased_table(name, frac)
    post, res = compacted(name, frac, limit)
    n0, n1 = len(pre["local_depth"]), len(post["local_depth"])
    print(f"{name} erased {frac} limit {limit}: {n0} -> {n1} segments, {res}")
    # the counts
    assert res["segments_before"] == n0 and res["segments_after"] == n1 == n0 - res["merges"]
    assert (res["merges"] == 0) == (res["rounds"] == 0) and res["rounds"] <= 30 - d0
    assert res["depth_before"] == pre["depth"] and res["depth_after"] == post["depth"] <= pre["depth"]
    # Invariant I and the rest of a valid table; no segment below the initial depth
    R.check_table(post, {"segments": n1}, n0)
    assert np.all(np.asarray(post["local_depth"]) >= d0)
    # every stored pair exactly once
    assert np.array_equal(_pairs_sorted(pre), _pairs_sorted(post))
    # Get, and the copies of every key in probe order (FindAnyway in probe order)
    a, b = E.ErasableTable(pre), E.ErasableTable(post)
    for k in stay.tolist():
        assert a.get(k) == b.get(k) and a.copies(k) == b.copies(k), k
    dk = np.asarray(pre["keys"], np.uint64)
    u, c = np.unique(dk[dk != np.uint64(R.INVALID)], return_counts=True)
    for k in u[c > 1][:200].tolist():  # the duplicates first of all
        assert a.copies(k) == b.copies(k) and len(a.copies(k)) > 1, k
    # idempotence
    again, res2 = CR.compact(post, d0, limit)
    assert res2["merges"] == 0 and res2["rounds"] == 0 and res2["refused"] == res["refused"]
    assert R.same_image(again, post)
    # no pair of the final table qualifies: each is over the limit or drops
    m = CR.CompactModel(post, d0)
    for i in m.pairs(limit):
        assert not m.merge(i)
    assert len(m.bad) == res["refused"]
    # the fixpoint does not depend on the order the pairs are taken in
    if n0 <= 64:
        for seed in (1, 2):
            other, ro = CR.compact_random_order(pre, d0, limit, seed)
            assert R.same_image(other, post), seed
            assert ro["merges"] == res["merges"] and ro["refused"] == res["refused"]


def test_suite_reaches_every_branch():
    """Conditions on the inputs, not on the rule: the parameters above contain
    a case that merges nothing, one of three or more rounds, a pair refused
    because its replay drops, and a table merged down to the floor of
    2^initial_depth segments."""
    seen = {"none": 0, "rounds3": 0, "refused": 0, "floor": 0}
    for name in STREAMS:
        for frac in FRACTIONS:
            for limit in LIMITS:
                post, res = compacted(name, frac, limit)
                d0 = erased_table(name, frac)[1]
                seen["none"] += res["merges"] == 0
                seen["rounds3"] += res["rounds"] >= 3
                seen["refused"] += res["refused"] >= 1
                seen["floor"] += res["merges"] > 0 and res["segments_after"] == 1 << d0
    print(seen)
    assert all(seen.values()), seen


def test_replay_order_and_drop():
    """The replay alone, on two crafted children: a child 1 whose cluster wraps
    past slot 1023 is walked from the cluster's true start, and a window that
    cannot take an entry refuses the pair."""
    keys = np.arange(1, 400000, dtype=np.uint64)
    line = (R.hash64(keys) & np.uint64(0xFF)).astype(np.int64)
    k255 = keys[line == 255][:6].tolist()   # windows 1020 .. 27
    k0 = keys[line == 0][:40].tolist()      # windows 0 .. 31
    empty = [R.INVALID] * R.SLOTS
    zero = [0] * R.SLOTS
    # child 1: line-255 keys at 1020..1023, 0, 1 (the wrap), then two line-0 keys at 2, 3
    c1 = list(empty)
    order = k255 + k0[:2]
    for j, k in enumerate(order):
        c1[(1020 + j) % R.SLOTS] = k
    v1 = [k ^ 7 if k != R.INVALID else 0 for k in c1]
    # child 0: two line-255 keys of its own at 1020, 1021
    c0 = list(empty)
    mine = keys[line == 255][6:8].tolist()
    c0[1020], c0[1021] = mine
    v0 = [k ^ 9 if k != R.INVALID else 0 for k in c0]
    pk, pv = CR.replay(c0, v0, c1, v1)
    want = mine + order  # child 0's stay, child 1's follow in probe order from the cluster's start
    assert [pk[(1020 + j) % R.SLOTS] for j in range(len(want))] == want
    assert pk.count(R.INVALID) == R.SLOTS - len(want)
    assert all(pv[j] == (pk[j] ^ (9 if pk[j] in mine else 7)) for j in range(R.SLOTS) if pk[j] != R.INVALID)
    # 20 + 20 entries of one window: the 33rd finds it full
    a, b = list(empty), list(empty)
    a[0:20], b[0:20] = k0[:20], k0[20:40]
    assert CR.replay(a, zero, b, zero) is None
    b[12:20] = [R.INVALID] * 8
    pk, _ = CR.replay(a, zero, b, zero)
    assert pk[:32] == k0[:20] + k0[20:32]


def test_compact_entry_point_is_declared_bound_and_built():
    src = open(os.path.join(REPO, "include", "pmdfc_cceh.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+pmdfc_cceh_compact\s*\(", src) and "pmdfc_compact_result_t" in src
    from pmdfc_amd.engine import EXPORTS, LIB_PATH, load_library
    import pmdfc_amd as P
    assert "pmdfc_cceh_compact" in EXPORTS
    out = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "pmdfc_cceh_compact" in {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert load_library().pmdfc_cceh_compact is not None and hasattr(P.CCEH, "Compact")
    from pmdfc_amd.kv import KV_EXPORTS, KV_LIB_PATH
    out = subprocess.run(["nm", "-D", "--defined-only", KV_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "pmdfc_kv_compact" in KV_EXPORTS and "pmdfc_kv_compact" in {l.split()[-1] for l in out.splitlines() if l.strip()}
