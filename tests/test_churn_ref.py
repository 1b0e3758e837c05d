"""The serial oracle's Erase (oracle/cceh_oracle.c oc_erase) and the churn
scripts (tests/churn_ref.py) on the CPU.

The contract of Erase is the rule of DESIGN.md 4.8 as tests/erase_ref.py
models it on a table that cannot split; where the two disagree the C code is
wrong.  The oracle's restatement exists because only the oracle splits: it is
held to the model on the fixture tables, on the crafted shapes and at every
erase step of every churn script -- exactly the states the GPU tests visit
(tests/test_gpu_churn_exact.py).  The rest asserts that each script reaches
what it is for; these are conditions on the oracle alone.
"""
import numpy as np
import pytest

import churn_ref as CR
import erase_ref as E
import limits_ref as R
import scenarios as S
from oracle import oracle as O

STREAMS = ["cap2_ins3k", "mixed_cap2_30k_ins80", "dup_wrap", "dup32", "dup_pairs"]
SHAPES = ["full_alt", "wide_wrap", "cyclic_heads", "backlog_c0"]


def oracle_table(name):
    """A fresh oracle after fixture stream `name` (of a crafted shape: the
    inserts before the trigger) and the keys the stream inserted."""
    sc = S.scenarios(O.hash64) if name in STREAMS else S.split_shapes(O.hash64)
    init_cap, conv, ops, keys, vals = sc[name]
    if name in SHAPES:
        n = S.split_shape_image_size(keys)
        ops, keys, vals = ops[:n], keys[:n], vals[:n]
    depth = O.OracleCCEH.depth_for_hybrid(init_cap) if conv == "hybrid" else O.OracleCCEH.depth_for_src(init_cap)
    o = O.OracleCCEH(depth)
    o.mixed(ops, keys, vals)
    return o, keys[np.asarray(ops) == O.OP_INSERT]


def _check(dump):
    n = len(dump["local_depth"])
    R.check_table(dump, {"segments": n}, n)


# ---- 1. the C erase against the Python contract

@pytest.mark.parametrize("name", STREAMS + SHAPES)
def test_oracle_erase_equals_model(name):
    o, ins = oracle_table(name)
    pre = o.dump()
    m = E.ErasableTable(pre)
    plan, _ = E.erase_plan(ins, 77)
    st = o.erase(plan)
    assert np.array_equal(st, m.erase_batch(plan)), name
    assert np.count_nonzero(st == O.ST_ERASED) > 30  # (cyclic_heads holds 97 keys)
    assert np.count_nonzero(st == O.ST_RESERVED_KEY) == 2
    post = o.dump()
    assert R.same_image(post, m.image()), name
    _check(post)
    assert o.depth == pre["depth"] and o.num_segments == len(pre["local_depth"])  # erase never touches the directory
    assert o.stats()["early_exit_mismatch"] == 0
    again = o.erase(plan)  # a second erase removes nothing
    assert np.all((again == O.ST_MISS) | (again == O.ST_RESERVED_KEY)) and R.same_image(o.dump(), post)
    o.close()


def test_oracle_erase_single_calls():
    """oc_erase one key at a time: a stored key, the same again, an absent key, the reserved keys."""
    o, ins = oracle_table("dup32")
    L = O.lib()
    u, c = np.unique(ins, return_counts=True)
    k32, k1 = int(u[np.argmax(c)]), int(u[c == 1][0])
    live = int(np.count_nonzero(o.dump()["keys"] != np.uint64(R.INVALID)))
    assert [L.oc_erase(o._t, k) for k in (k1, k1, 0x123456789ABCDEF, R.INVALID, R.SENTINEL, k32, k32)] == \
        [O.ST_ERASED, O.ST_MISS, O.ST_MISS, O.ST_RESERVED_KEY, O.ST_RESERVED_KEY, O.ST_ERASED, O.ST_MISS]
    d = o.dump()
    assert int(np.count_nonzero(d["keys"] != np.uint64(R.INVALID))) == live - 33  # all 32 copies went
    assert o.get(np.array([k1, k32], np.uint64))[1].tolist() == [O.ST_MISS, O.ST_MISS]
    _check(d)
    o.close()


@pytest.mark.parametrize("name", ["full_alt", "wide_wrap"])
def test_oracle_erases_a_table_to_empty(name):
    o, _ = oracle_table(name)
    pre = o.dump()
    keys = np.unique(np.asarray(pre["keys"], np.uint64))
    keys = keys[keys != np.uint64(R.INVALID)]
    keys = keys[np.random.default_rng(5).permutation(keys.size)]
    m = E.ErasableTable(pre)
    st = o.erase(keys)
    assert np.all(st == O.ST_ERASED) and np.array_equal(st, m.erase_batch(keys))
    d = o.dump()
    assert np.all(d["keys"] == np.uint64(R.INVALID)) and np.all(d["values"] == 0)
    assert R.same_image(d, m.image())
    o.close()


# ---- 2. every erase step of every script; 3. the table's structure there

@pytest.mark.parametrize("name", CR.NAMES)
def test_every_erase_step_equals_model(name):
    s = CR.script(name)
    r = CR.run_oracle(s)
    assert s.erase_steps()
    for i in s.erase_steps():
        m = E.ErasableTable(r.pre[i], upsert=s.upsert)
        assert np.array_equal(m.erase_batch(s.steps[i][1]), r.results[i]), (name, i)
        assert R.same_image(m.image(), r.post[i]), (name, i)
        _check(r.post[i])
        assert r.marks[i]["live"] == m.live()
    _check(r.final)
    last = len(s.steps)
    assert r.marks[last]["segments"] == len(r.final["local_depth"]) <= 512 and r.marks[last]["depth"] == r.final["depth"]


def test_insert_only_projection():
    s = CR.insert_only(CR.script("churn"))
    r = CR.run_oracle(s)
    assert all(np.all(st[1] == CR.OP_INSERT) for st in s.steps if st[0] == "mixed")
    for i in s.erase_steps():
        m = E.ErasableTable(r.pre[i])
        assert np.array_equal(m.erase_batch(s.steps[i][1]), r.results[i]) and R.same_image(m.image(), r.post[i]), i
    first, last = s.erase_steps()[0], len(s.steps)
    assert r.marks[last]["splits"] - r.marks[first]["splits"] >= 50
    _check(r.final)


# ---- 4. the scripts reach what they are for

def _reinserts(s, r, status):
    """Inserts of keys that an earlier step erased, answered `status`."""
    erased, n = np.zeros(0, np.uint64), 0
    for st, res in zip(s.steps, r.results):
        if st[0] == "erase":
            erased = np.union1d(erased, st[1][res == O.ST_ERASED])
        else:
            n += int(np.count_nonzero((st[1] == CR.OP_INSERT) & (res[1] == status) & np.isin(st[2], erased)))
    return n


def _growth(s, r):
    first, last = s.erase_steps()[0], len(s.steps)
    return (r.marks[last]["splits"] - r.marks[first]["splits"], r.marks[last]["doublings"] - r.marks[first]["doublings"])


def _statuses(s, r, kind):
    return np.concatenate([res if st[0] == "erase" else res[1] for st, res in zip(s.steps, r.results) if st[0] == kind])


@pytest.mark.parametrize("name,splits,doublings", [("churn", 50, 3), ("churn_upsert", 50, 3), ("churn_short", 10, 1)])
def test_churn_scripts_split_and_double_after_an_erase(name, splits, doublings):
    s = CR.script(name)
    r = CR.run_oracle(s)
    got = _growth(s, r)
    assert got[0] >= splits and got[1] >= doublings, got
    for i in s.erase_steps():
        st = r.results[i]
        assert np.count_nonzero(st == O.ST_ERASED) > 100 and np.count_nonzero(st == O.ST_MISS) > 100, (name, i)
        assert np.count_nonzero(st == O.ST_RESERVED_KEY) == 2
        assert np.all(np.isin(st, [O.ST_ERASED, O.ST_MISS, O.ST_RESERVED_KEY]))
    mixed = _statuses(s, r, "mixed")
    assert np.count_nonzero(mixed == O.ST_HIT) > 1000 and np.count_nonzero(mixed == O.ST_MISS) > 1000
    back = _reinserts(s, r, O.ST_INSERTED)
    updated = int(np.count_nonzero(mixed == O.ST_UPDATED))
    if name != "churn_short":
        # every segment is 7 levels deep two rounds before the end: an engine with max_batch 16,384 is at its
        # full bucket resolution (7 bits) from there on, which its medium, general and pipelined paths need
        assert int(np.min(r.post[s.erase_steps()[-3]]["local_depth"])) >= 7
        assert max(m["segments"] for m in r.marks.values()) <= 512
    if name == "churn":
        assert back >= 500 and updated == 0
        k, c = np.unique(r.final["keys"], return_counts=True)  # second copies are stored, and erased with the first
        assert np.count_nonzero(c[k != np.uint64(R.INVALID)] > 1) > 100 and CR.copies_erased(s, r) > 100
    elif name == "churn_upsert":
        assert updated > 1000 and back >= 100
        k, c = np.unique(r.final["keys"], return_counts=True)
        assert np.all(c[k != np.uint64(R.INVALID)] == 1) and CR.copies_erased(s, r) == 0
    print(f"{name}: {s.ops()} ops in {len(s.steps)} steps; after the first erase {got[0]} splits, {got[1]} doublings; "
          f"ERASED per erase step {[int(np.count_nonzero(r.results[i] == O.ST_ERASED)) for i in s.erase_steps()]}, "
          f"MISS {[int(np.count_nonzero(r.results[i] == O.ST_MISS)) for i in s.erase_steps()]}; "
          f"{back} re-inserts INSERTED, {updated} UPDATED; live at the end {r.marks[len(s.steps)]['live']}, "
          f"{r.marks[len(s.steps)]['segments']} segments, depth {r.marks[len(s.steps)]['depth']}")


def test_loss_after_erase_drops_after_the_erase():
    s = CR.script("loss_after_erase")
    r = CR.run_oracle(s)
    (e,) = s.erase_steps()
    before, after = r.marks[e]["split_loss"], r.marks[len(s.steps)]["split_loss"]
    assert after > before, (before, after)
    assert np.all(r.results[e] == O.ST_ERASED) and r.results[e].size >= 15
    # nothing is erased after step e, so a key stored then and absent at the end was dropped by a split
    stored = np.asarray(r.post[e]["keys"], np.uint64)
    stored = stored[stored != np.uint64(R.INVALID)]
    dropped = stored[~np.isin(stored, r.final["keys"])]
    assert dropped.size == after - before
    asked = np.concatenate([st[2][st[1] == CR.OP_GET] for st in s.steps[e + 1:]])
    assert np.any(np.isin(asked, dropped))
    assert _reinserts(s, r, O.ST_INSERTED) == r.results[e].size  # every erased key comes back at the end
    print(f"loss_after_erase: split_loss {before} before the erase step, {after} at the end; "
          f"{r.results[e].size} keys erased, {np.count_nonzero(np.isin(asked, dropped))} Gets of dropped keys")


def test_unsplittable_status_sequence():
    s = CR.script("unsplittable")
    r = CR.run_oracle(s)
    tail = r.results[-5:]
    assert tail[0][1].tolist() == [O.ST_UNSPLITTABLE]
    assert tail[1].tolist() == [O.ST_ERASED]
    assert tail[2][1].tolist() == [O.ST_INSERTED, O.ST_INSERTED, O.ST_HIT] and tail[2][0].tolist() == [0, 0, 201]
    assert np.all(tail[3][1] == O.ST_INSERTED) and tail[3][1].size == 30
    assert tail[4][1].tolist() == [O.ST_UNSPLITTABLE]
    (e,) = s.erase_steps()
    assert r.marks[e]["live"] == r.marks[len(s.steps)]["live"] - 32  # all 32 copies went, 32 came back
