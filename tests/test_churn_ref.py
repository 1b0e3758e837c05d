"""The serial oracle's Erase (oracle/cceh_oracle.c oc_erase) and the churn
scripts (tests/churn_ref.py) on the CPU.

The contract of Erase is the rule of DESIGN.md 4.8 as tests/erase_ref.py
models it on a table that cannot split; where the two disagree the C code is
wrong.  The oracle's restatement exists because only the oracle splits: it is
held to the model on the fixture tables, on the crafted shapes and at every
erase step of every churn script -- exactly the states the GPU tests visit
(tests/test_gpu_churn_exact.py).  The rest asserts that each script reaches
what it is for; these are conditions on the oracle alone.

The regrow scripts shrink their table through EraseMatching and Compact, which
the oracle follows through match_ref, compact_ref and oc_load (section 5
below): load(dump()) changes nothing, a load refuses what does not tile the
directory, and every such step leaves the table the GPU tests
(tests/test_gpu_regrow_exact.py) need it to leave.
"""
import numpy as np
import pytest

import churn_ref as CR
import compact_ref as C
import erase_ref as E
import limits_ref as R
import match_ref as M
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
        elif st[0] == "mixed":
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


# ---- 5. the oracle across EraseMatching and Compact: oc_load and the regrow scripts

REGROW = ["regrow", "regrow_short", "regrow_upsert", "lopsided"]
FULL_SIZE = ["regrow", "regrow_upsert", "lopsided"]
FULL_BITS = 7  # of tests/test_gpu_churn_exact.py: the bucket bits of a table at full resolution
SEG_LIMIT = 400  # room under the GPU tests' max_segments 512: no engine may answer CAPACITY


def _ld(d):
    return np.asarray(d["local_depth"], np.int64)


@pytest.mark.parametrize("upsert", [False, True])
def test_load_of_own_dump_changes_nothing(upsert):
    o, ins = oracle_table("mixed_cap2_30k_ins80")
    O.lib().oc_set_upsert(o._t, int(upsert))
    d, st, nseg = o.dump(), o.stats(), o.num_segments
    o.load(d)
    d2 = o.dump()
    assert R.same_image(d, d2) and np.array_equal(d["dir_canon"], d2["dir_canon"])
    assert o.stats() == st and (o.depth, o.num_segments) == (d["depth"], nseg)
    # upsert stays as it was: a stored key again is UPDATED under upsert, a second copy otherwise
    assert o.insert(ins[:1], np.array([7], np.uint64)).tolist() == [O.ST_UPDATED if upsert else O.ST_INSERTED]
    assert o.stats()["inserts"] == st["inserts"] + 1
    o.close()


@pytest.mark.parametrize("name", REGROW)
def test_reloading_run_equals_plain_run(name):
    """A run that loads its own dump after every step answers and stores what
    a run that never does answers and stores."""
    s = CR.script(name)
    a, b = CR.run_oracle(s), CR.run_oracle(s, reload=True)
    for i, st in enumerate(s.steps):
        if st[0] == "mixed":
            assert np.array_equal(a.results[i][0], b.results[i][0]) and np.array_equal(a.results[i][1], b.results[i][1]), i
            continue
        if st[0] == "erase":
            assert np.array_equal(a.results[i], b.results[i]), i
        else:
            assert a.results[i] == b.results[i], i
        assert R.same_image(a.pre[i], b.pre[i]) and R.same_image(a.post[i], b.post[i]), i
        assert a.marks[i] == b.marks[i], i
    assert R.same_image(a.final, b.final) and a.marks[len(s.steps)] == b.marks[len(s.steps)]


def test_load_refuses_what_does_not_tile_the_directory():
    o, _ = oracle_table("cap2_ins3k")
    before = o.dump()

    def image(depth, lds):
        n = len(lds)
        return {"depth": depth, "local_depth": np.array(lds, np.uint32),
                "keys": np.full(n * R.SLOTS, R.INVALID, np.uint64), "values": np.zeros(n * R.SLOTS, np.uint64)}

    for depth, lds in [(2, [0, 1]), (2, [3, 3, 2, 1]), (2, [1, 2]), (2, [1, 2, 2, 2]), (2, [2, 1, 2]), (2, [1, 1, 1]),
                       (0, [0]), (31, [1, 1]), (2, [])]:
        with pytest.raises(ValueError):
            o.load(image(depth, lds))
        assert R.same_image(o.dump(), before), (depth, lds)
    bad = image(2, [1, 2, 2])
    bad["keys"] = bad["keys"][:-1]
    with pytest.raises(ValueError):
        o.load(bad)
    o.load(image(3, [2, 3, 3, 1]))  # and one that tiles: an empty table of that shape, which fills and splits
    d = o.dump()
    assert d["local_depth"].tolist() == [2, 3, 3, 1] and d["prefix"].tolist() == [0, 2, 3, 1] and d["depth"] == 3
    assert d["dir_canon"].tolist() == [0, 0, 1, 2, 3, 3, 3, 3]
    keys = CR.uniform_keys(9, 0, 3000)
    assert np.all(o.insert(keys, keys) == O.ST_INSERTED) and np.all(o.get(keys)[1] == O.ST_HIT)
    _check(o.dump())
    assert o.num_segments > 4
    o.close()


def _two_steps_at_full_depth(s, r):
    """An engine asks for the smallest local depth when a batch starts, reads
    the answer when the next one starts and refines its buckets then
    (rebucket_now): fed a step per call it is at its full resolution from the
    second step after the one that made every segment 7 deep.  Before each
    compact step and before the end of a table that a Compact had shrunk, the
    oracle's table is that deep with three mixed steps still to come, so the
    last two ran at the full resolution whatever the cutting; before the first
    shrinking Compact with two to come, so the last one did."""
    merging = [c for c in s.steps_of("compact") if r.results[c]["merges"]]
    for at in s.steps_of("compact") + [len(s.steps)]:
        mixed = [j for j in range(at) if s.steps[j][0] == "mixed"]
        k = 4 if any(c < at for c in merging) else 3
        assert not any(mixed[-k] < c < at for c in merging), (s.name, at)
        assert r.min_ld[mixed[-k]] >= FULL_BITS, (s.name, at, r.min_ld)
        assert all(len(s.steps[j][1]) >= 9000 for j in mixed[1 - k:-1]), (s.name, at)


@pytest.mark.parametrize("name", REGROW)
def test_regrow_scripts_reach_what_they_are_for(name):
    s = CR.script(name)
    r = CR.run_oracle(s)
    last = len(s.steps)
    compacts, matches = s.steps_of("compact"), s.steps_of("match")
    assert compacts and s.depth == 1
    assert (len(matches) > 0) == (name in ("regrow", "regrow_short"))
    for i in sorted(r.marks):
        assert "split_loss" in r.marks[i] and r.marks[i]["segments"] <= SEG_LIMIT, (name, i)
    assert max(len(d["local_depth"]) for d in list(r.pre.values()) + [r.final]) <= SEG_LIMIT
    for i in compacts:
        res, pre, post = r.results[i], r.pre[i], r.post[i]
        want, again = C.compact(pre, s.depth, s.steps[i][1])
        assert again == res and R.same_image(post, want), (name, i)  # the oracle went on from the model's image
        _check(post)  # (Invariant I included)
        assert (res["segments_before"], res["depth_before"]) == (len(pre["local_depth"]), pre["depth"])
        assert (res["segments_after"], res["depth_after"]) == (len(post["local_depth"]), post["depth"])
        assert r.marks[i]["live"] == int(np.count_nonzero(pre["keys"] != np.uint64(R.INVALID)))  # every pair stays
        if name != "regrow_short":
            assert _ld(pre).min() >= FULL_BITS, (name, i, _ld(pre).min())
        if name == "lopsided":
            continue
        assert res["merges"] > 0 and post["depth"] < pre["depth"] and _ld(post).min() <= _ld(pre).min() - 2, (name, i, res)
    if name in FULL_SIZE:
        assert _ld(r.final).min() >= FULL_BITS
        _two_steps_at_full_depth(s, r)
    if name == "lopsided":
        nothing, shrink = compacts
        assert r.results[nothing]["merges"] == 0 and R.same_image(r.pre[nothing], r.post[nothing])
        pre, post, res = r.pre[shrink], r.post[shrink], r.results[shrink]
        assert res["merges"] > 0 and post["depth"] == pre["depth"]
        assert _ld(post).max() - _ld(post).min() >= 4, _ld(post)
        assert np.all(_ld(post)[np.asarray(post["prefix"]) >> (_ld(post) - 2).astype(np.uint64) == 0] >= FULL_BITS)
    if name == "regrow":
        assert max(r.results[i]["refused"] for i in compacts) > 0
        assert any(r.results[i]["depth_after"] > s.depth for i in compacts)  # a partial collapse as well
    if name == "regrow_upsert":
        assert len(np.unique(_ld(r.post[compacts[-1]]))) > 1  # the limit of 256 leaves two depths side by side
        k, c = np.unique(r.final["keys"], return_counts=True)
        assert np.all(c[k != np.uint64(R.INVALID)] == 1)
        assert np.count_nonzero(_statuses(s, r, "mixed") == O.ST_UPDATED) > 1000
    grown = r.marks[last]["splits"] - r.marks[compacts[-1]]["splits"]
    assert grown >= (10 if name == "regrow_short" else 100), grown  # the table split its way back after the last Compact
    mixed = _statuses(s, r, "mixed")
    assert np.all(np.isin(mixed, [O.ST_MISS, O.ST_HIT, O.ST_INSERTED, O.ST_UPDATED]))
    assert np.count_nonzero(mixed == O.ST_HIT) > 1000 and np.count_nonzero(mixed == O.ST_MISS) > 1000
    print(f"{name}: {s.ops()} ops in {len(s.steps)} steps; compact steps "
          f"{[(s.steps[i][1], r.results[i]['segments_before'], r.results[i]['segments_after'], r.results[i]['rounds'], r.results[i]['refused'], r.results[i]['depth_before'], r.results[i]['depth_after']) for i in compacts]} "
          f"(limit, segments before and after, rounds, refused, depth before and after); split_loss "
          f"{[r.marks[i]['split_loss'] for i in sorted(r.marks)]}; at the end {r.marks[last]['live']} live, "
          f"{r.marks[last]['segments']} segments, depth {r.marks[last]['depth']}, local depths "
          f"{_ld(r.final).min()}..{_ld(r.final).max()}")


def test_some_compact_step_is_refused_a_pair_and_one_merges_nothing():
    res = [CR.run_oracle(CR.script(n)).results[i] for n in REGROW for i in CR.script(n).steps_of("compact")]
    assert any(x["refused"] > 0 and x["merges"] > 0 for x in res)
    assert any(x["merges"] == 0 for x in res)


@pytest.mark.parametrize("name", ["regrow", "regrow_short"])
def test_match_steps_equal_model(name):
    s = CR.script(name)
    r = CR.run_oracle(s)
    for i in s.steps_of("match"):
        L, st, image = r.matched[i]
        live = int(np.count_nonzero(r.pre[i]["keys"] != np.uint64(R.INVALID)))
        assert L.size * 100 >= live and np.all(st == O.ST_ERASED), (name, i)
        assert R.same_image(r.post[i], image), (name, i)  # oc_erase of L is the model's erase of L
        res = r.results[i]
        assert res["removed"] == live - r.marks[i]["live"] >= L.size
        assert res["segments_scanned"] == len(r.pre[i]["local_depth"]) and res["segments_changed"] > 0
        assert not np.any(M.match_mask(r.post[i], s.steps[i][1], s.steps[i][2]))
        _check(r.post[i])
        # the generator's bookkeeping: the keys that went are gone to it as well, so that it asks for them
        # (MISS) and stores some again (INSERTED, never UPDATED or a second copy)
        asked = np.concatenate([x[2][x[1] == CR.OP_GET] for x in s.steps[i + 1:] if x[0] == "mixed"])
        assert np.count_nonzero(np.isin(asked, L)) > 50
        nxt = next(j for j in range(i + 1, len(s.steps)) if s.steps[j][0] == "mixed")
        g = (s.steps[nxt][1] == CR.OP_GET) & np.isin(s.steps[nxt][2], L)
        later = np.concatenate([x[2][x[1] == CR.OP_INSERT] for x in s.steps[i + 1:nxt + 1] if x[0] == "mixed"])
        quiet = g & ~np.isin(s.steps[nxt][2], later)
        assert np.all(r.results[nxt][1][quiet] == O.ST_MISS)


def test_insert_only_projection_keeps_the_new_steps():
    s = CR.script("regrow")
    p = CR.insert_only(s)
    assert [x[0] for x in p.steps] == [x[0] for x in s.steps]
    assert all(p.steps[i] is s.steps[i] for i in s.steps_of("match") + s.steps_of("compact"))
    r = CR.run_oracle(p)
    for i in p.steps_of("compact"):
        assert r.results[i]["merges"] > 0 and _ld(r.pre[i]).min() >= FULL_BITS
    assert _ld(r.final).min() >= FULL_BITS and max(m["segments"] for m in r.marks.values()) <= SEG_LIMIT
    _two_steps_at_full_depth(p, r)
    p = CR.insert_only(CR.script("lopsided"))
    q = CR.run_oracle(p)
    assert _ld(q.final).min() >= FULL_BITS and max(m["segments"] for m in q.marks.values()) <= SEG_LIMIT
    _two_steps_at_full_depth(p, q)
