"""The model of Erase (tests/erase_ref.py) on the CPU: on tables the serial
oracle builds from fixture streams the rule keeps the structure every probe
relies on (limits_ref.check_table, whose last assertion is Invariant I of
DESIGN.md 4.8), removes every copy of an erased key and nothing else, keeps the
order of the copies of other keys, and empties a table completely.  And the
engine's C-ABI carries the new entry point.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import erase_ref as E
import limits_ref as R
import scenarios as S
from conftest import REPO
from oracle import oracle as O

STREAMS = ["cap2_ins3k", "mixed_cap2_30k_ins80", "dup_wrap", "dup32", "dup_pairs"]
_DUMPS = {}


def oracle_dump(name):
    """The serial table after fixture stream `name` (built once, never changed)."""
    if name not in _DUMPS:
        sc = S.scenarios(O.hash64)
        sc.update(S.split_shapes(O.hash64))
        init_cap, conv, ops, keys, vals = sc[name]
        if name in S.split_shapes(O.hash64):  # the crafted image alone: the inserts before the trigger
            n = S.split_shape_image_size(keys)
            ops, keys, vals = ops[:n], keys[:n], vals[:n]
        depth = O.OracleCCEH.depth_for_hybrid(init_cap) if conv == "hybrid" else O.OracleCCEH.depth_for_src(init_cap)
        o = O.OracleCCEH(depth)
        o.mixed(ops, keys, vals)
        _DUMPS[name] = (o.dump(), keys[np.asarray(ops) == O.OP_INSERT])
        o.close()
    return _DUMPS[name]


def _check(t):
    img = t.image()
    n = len(img["local_depth"])
    R.check_table(img, {"segments": n}, n)
    return img


@pytest.mark.parametrize("name", STREAMS)
def test_model_erases_half_of_a_stream(name):
    dump, ins = oracle_dump(name)
    t = E.ErasableTable(dump)
    before = E.ErasableTable(dump)
    plan, stay = E.erase_plan(ins, 77)
    stored = {int(k) for k in np.unique(ins)} & {int(k) for k in dump["keys"]}  # (a split may have dropped some)
    want = np.array([R.ST_RESERVED_KEY if k >= R.SENTINEL else E.ST_ERASED if k in stored else R.ST_MISS
                     for k in plan.tolist()], np.uint8)
    st = t.erase_batch(plan)
    assert np.array_equal(st, want)
    assert np.count_nonzero(st == E.ST_ERASED) > 100 or name == "dup32"
    img = _check(t)
    for k in plan.tolist():  # erased keys miss, every copy is gone
        assert t.get(k)[1] in (R.ST_MISS, R.ST_RESERVED_KEY)
    assert not np.any(np.isin(img["keys"], plan[plan < np.uint64(R.SENTINEL)]))
    for k in stay.tolist():  # the others answer as before, their copies in the same order
        assert t.get(k) == before.get(k)
        assert t.copies(k) == before.copies(k)
    assert t.live() == before.live() - sum(len(before.copies(k)) for k in plan.tolist() if k in stored)
    # a second erase of everything in the plan removes nothing
    again = t.erase_batch(plan)
    assert np.all((again == R.ST_MISS) | (again == R.ST_RESERVED_KEY))
    assert R.same_image(t.image(), img)
    print(f"{name}: {np.count_nonzero(st == E.ST_ERASED)} erased, {t.moves} moves, longest chain {t.max_chain}")


@pytest.mark.parametrize("name", ["dup_wrap", "dup32", "dup_pairs"])
def test_model_erases_all_copies_of_duplicates(name):
    dump, ins = oracle_dump(name)
    t = E.ErasableTable(dump)
    u, c = np.unique(ins, return_counts=True)
    dups = [int(k) for k in u[c > 1] if len(t.copies(int(k))) > 1]
    assert dups
    for k in dups:
        assert t.erase(k) == E.ST_ERASED and t.copies(k) == [] and t.get(k) == (0, R.ST_MISS)
        assert t.erase(k) == R.ST_MISS
    img = _check(t)
    assert not np.any(np.isin(img["keys"], np.array(dups, np.uint64)))


@pytest.mark.parametrize("name", ["cap2_ins3k", "dup_wrap", "full_alt", "wide_wrap", "cyclic_heads"])
def test_model_erases_a_table_to_empty(name):
    """Every key erased in a random order -- full_alt is a segment with all
    1,024 slots taken, wide_wrap and cyclic_heads have clusters across slot
    1023 -- with the structure checked along the way: every slot {INVALID, 0}."""
    dump, ins = oracle_dump(name)
    t = E.ErasableTable(dump)
    keys = np.unique(np.asarray(dump["keys"], np.uint64))
    keys = keys[keys != np.uint64(R.INVALID)]
    keys = keys[np.random.default_rng(5).permutation(keys.size)]
    for i, k in enumerate(keys.tolist()):
        assert t.erase(k) == E.ST_ERASED
        if i % 97 == 0:
            _check(t)
    img = t.image()
    assert np.all(img["keys"] == np.uint64(R.INVALID)) and np.all(img["values"] == 0)
    print(f"{name}: {keys.size} keys, {t.moves} moves, longest chain {t.max_chain}")


def test_model_batch_order():
    """A stored key three times, an absent key twice, a key stored 32 times."""
    dump, ins = oracle_dump("dup32")
    t = E.ErasableTable(dump)
    u, c = np.unique(ins, return_counts=True)
    k32 = int(u[np.argmax(c)])
    assert len(t.copies(k32)) == 32
    k1 = int(u[c == 1][0])
    absent = 0x123456789ABCDEF
    assert t.get(absent)[1] == R.ST_MISS
    st = t.erase_batch(np.array([k1, k1, k1, absent, absent, k32], np.uint64))
    assert st.tolist() == [E.ST_ERASED, R.ST_MISS, R.ST_MISS, R.ST_MISS, R.ST_MISS, E.ST_ERASED]
    assert t.copies(k32) == []
    _check(t)


def test_erase_entry_point_is_declared_bound_and_built():
    src = open(os.path.join(REPO, "include", "pmdfc_cceh.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+pmdfc_cceh_erase\s*\(", src)
    assert re.search(r"#define\s+PMDFC_ST_ERASED\s+12\b", src)
    from pmdfc_amd.engine import EXPORTS, LIB_PATH, load_library
    import pmdfc_amd as P
    assert "pmdfc_cceh_erase" in EXPORTS and P.ST_ERASED == E.ST_ERASED == 12
    out = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "pmdfc_cceh_erase" in {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert load_library().pmdfc_cceh_erase is not None and hasattr(P.CCEH, "Erase")
    from pmdfc_amd.kv import KV_EXPORTS, KV_LIB_PATH
    out = subprocess.run(["nm", "-D", "--defined-only", KV_LIB_PATH], capture_output=True, text=True, check=True).stdout
    syms = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for s in ("pmdfc_kv_erase", "pmdfc_kv_erase_run"):
        assert s in KV_EXPORTS and s in syms
