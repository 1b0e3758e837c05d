"""The model of EraseMatching (tests/match_ref.py) on the CPU, on tables the
serial oracle builds: the five fixture streams, every crafted shape of
scenarios.split_shapes and the inode stream (48 files' pages in
CCEH_hybrid(2)).  After a call the structure every probe relies on holds
(limits_ref.check_table, Invariant I), no stored key matches, every other key
answers as before with its copies in the same order, `removed` is the count of
matching entries, a second call is a no-op, mask 0 empties the table -- and the
final image does not depend on the order in which the matching keys are erased
(three seeded permutations of L against L in order), which is what lets the
kernel take a segment's matches in the order that suits it.  And the engine's
C-ABI carries the entry point.

Every case asserts that it is not vacuous: between 10 % and 90 % of the live
entries match, except the cases named all and none.  The low-bit pairs
(mask, pattern) = (1, 0) and (3, 1) select about a half and a quarter of any
table's keys and run on every table; (7, 3) selects an eighth of uniform keys
but as little as 9 % of a crafted shape's, so it runs on the fixture streams
and the inode stream, and every crafted shape takes the first residue under
mask 7 that at least 10 % of its own entries have.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import erase_ref as E
import limits_ref as R
import match_ref as M
import scenarios as S
from conftest import REPO
from oracle import oracle as O

STREAMS = ["cap2_ins3k", "mixed_cap2_30k_ins80", "dup_wrap", "dup32", "dup_pairs"]
SHAPES = sorted(S.split_shapes(O.hash64))
PAIRS = [(1, 0), (3, 1), (7, 3)]
_DUMPS = {}


def oracle_dump(name):
    """The serial table of fixture stream or crafted shape `name`, or of the
    inode stream ("inodes"); built once, never changed."""
    if name in _DUMPS:
        return _DUMPS[name]
    if name == "inodes":
        _, _, keys = M.inode_stream()
        o = O.OracleCCEH(O.OracleCCEH.depth_for_hybrid(2))
        assert np.all(o.insert(keys, keys ^ np.uint64(0x1D0DE)) == O.ST_INSERTED)
    else:
        sc = S.scenarios(O.hash64)
        shapes = S.split_shapes(O.hash64)
        sc.update(shapes)
        init_cap, conv, ops, keys, vals = sc[name]
        if name in shapes:  # the crafted image alone: the inserts before the trigger
            n = S.split_shape_image_size(keys)
            ops, keys, vals = ops[:n], keys[:n], vals[:n]
        depth = O.OracleCCEH.depth_for_hybrid(init_cap) if conv == "hybrid" else O.OracleCCEH.depth_for_src(init_cap)
        o = O.OracleCCEH(depth)
        o.mixed(ops, keys, vals)
    _DUMPS[name] = o.dump()
    o.close()
    return _DUMPS[name]


def _check(t):
    img = t.image()
    n = len(img["local_depth"])
    R.check_table(img, {"segments": n}, n)
    return img


def _properties(dump, mask, patterns, share):
    """One call on the model; share: "some" (10 %..90 % must match), "all", "none"."""
    before = E.ErasableTable(dump)
    keys = np.asarray(dump["keys"], np.uint64)
    hit = M.match_mask(dump, mask, patterns)
    live = int(np.count_nonzero(keys != np.uint64(R.INVALID)))
    frac = np.count_nonzero(hit) / live
    if share == "some":
        assert 0.10 <= frac <= 0.90, frac
    elif share == "all":
        assert np.count_nonzero(hit) == live > 0
    else:
        assert not np.any(hit)
    L = M.matching_keys(dump, mask, patterns)
    assert np.unique(L).size == L.size == np.unique(keys[hit]).size
    t, res = M.erase_matching(dump, mask, patterns)
    img = _check(t)
    assert not np.any(M.match_mask(img, mask, patterns))  # no stored key matches
    assert res["removed"] == np.count_nonzero(hit) == live - t.live()
    assert res["segments_cleared"] <= res["segments_changed"] <= len(dump["local_depth"])
    assert res["segments_scanned"] == (len(dump["local_depth"]) if len(patterns) else 0)  # (no pattern: no scan)
    gone = set(L.tolist())
    for k in np.unique(keys[(keys != np.uint64(R.INVALID)) & ~hit]).tolist():
        assert k not in gone  # (a key matches with all its copies or with none)
        assert t.get(k) == before.get(k) and t.copies(k) == before.copies(k)
    for k in L.tolist():
        assert t.get(k) == (0, R.ST_MISS) and t.copies(k) == []
    t2, res2 = M.erase_matching(img, mask, patterns)  # a second call removes nothing
    assert res2["removed"] == res2["segments_changed"] == res2["segments_cleared"] == 0
    assert R.same_image(t2.image(), img)
    if share == "none":
        assert R.same_image(img, before.image())
    return img, L, frac


def _order_independent(dump, L, img):
    for seed in (1, 2, 3):
        t = E.ErasableTable(dump)
        st = t.erase_batch(L[np.random.default_rng(seed).permutation(L.size)])
        assert np.all(st == E.ST_ERASED)
        assert R.same_image(t.image(), img), seed


@pytest.mark.parametrize("mask,pattern", PAIRS)
@pytest.mark.parametrize("name", STREAMS + ["inodes"])
def test_model_on_streams(name, mask, pattern):
    dump = oracle_dump(name)
    img, L, frac = _properties(dump, mask, [pattern], "some")
    _order_independent(dump, L, img)
    print(f"{name} ({mask}, {pattern}): {L.size} keys, {100 * frac:.1f} % of the live entries")


@pytest.mark.parametrize("mask,pattern", PAIRS[:2])
@pytest.mark.parametrize("name", SHAPES)
def test_model_on_crafted_shapes(name, mask, pattern):
    dump = oracle_dump(name)
    img, L, frac = _properties(dump, mask, [pattern], "some")
    _order_independent(dump, L, img)
    print(f"{name} ({mask}, {pattern}): {L.size} keys, {100 * frac:.1f} % of the live entries")


@pytest.mark.parametrize("name", SHAPES)
def test_model_on_crafted_shapes_an_eighth(name):
    """An eighth of a crafted shape's keys: of the eight residues under mask 7
    the first that at least 10 % of this shape's live entries have (one does:
    their mean share is 12.5 %), chosen from the table alone."""
    dump = oracle_dump(name)
    keys = np.asarray(dump["keys"], np.uint64)
    live = keys[keys != np.uint64(R.INVALID)]
    share = np.bincount((live & np.uint64(7)).astype(np.int64), minlength=8) / live.size
    pattern = int(np.nonzero(share >= 0.10)[0][0])
    img, L, frac = _properties(dump, 7, [pattern], "some")
    assert frac <= 0.5
    _order_independent(dump, L, img)
    print(f"{name} (7, {pattern}): {L.size} keys, {100 * frac:.1f} % of the live entries")


def test_model_inode_patterns():
    """The inode stream under the inode mask: the two large files, half of the
    files, all of them (all), an absent inode (none), and 1,024 patterns with
    repeats of which 24 exist."""
    dump = oracle_dump("inodes")
    inos, pages, keys = M.inode_stream()
    assert len(dump["local_depth"]) == 16 and 7000 < keys.size < 9000
    assert np.count_nonzero(np.asarray(dump["keys"], np.uint64) != np.uint64(R.INVALID)) == keys.size
    big = M.inode_patterns(inos[[3, 4]])
    img, L, _ = _properties(dump, M.INODE_MASK, big, "some")
    assert L.size == 1350
    _order_independent(dump, L, img)
    half = M.inode_patterns(inos[::2])
    img, L, _ = _properties(dump, M.INODE_MASK, half, "some")
    assert L.size == int(pages[::2].sum())
    _order_independent(dump, L, img)
    absent = int(np.setdiff1d(np.arange(2, 100, dtype=np.uint64), inos)[0])
    many = np.concatenate([half, half[:10], np.arange(1 << 21, (1 << 21) + 990, dtype=np.uint64) << np.uint64(32)])
    assert many.size == M.MATCH_MAX
    t, res = M.erase_matching(dump, M.INODE_MASK, many)
    assert R.same_image(t.image(), img) and res["removed"] == L.size
    img, L, _ = _properties(dump, M.INODE_MASK, M.inode_patterns(inos), "all")
    assert np.all(img["keys"] == np.uint64(R.INVALID)) and np.all(img["values"] == 0)
    _properties(dump, M.INODE_MASK, [absent << 32], "none")
    _properties(dump, M.INODE_MASK, [], "none")
    # an empty slot never matches: the pattern that equals INVALID under the full mask
    _properties(dump, R.INVALID, [R.INVALID], "none")


@pytest.mark.parametrize("name", STREAMS + ["inodes", "full_alt", "wide_wrap", "cyclic_heads", "backlog_c0"])
def test_model_mask_zero_empties_the_table(name):
    dump = oracle_dump(name)
    img, L, _ = _properties(dump, 0, [0x1234], "all")
    assert np.all(img["keys"] == np.uint64(R.INVALID)) and np.all(img["values"] == 0)
    assert np.array_equal(img["local_depth"], dump["local_depth"]) and img["depth"] == dump["depth"]
    t, res = M.erase_matching(dump, 0, [0x1234])
    live = (np.asarray(dump["keys"], np.uint64) != np.uint64(R.INVALID)).reshape(-1, R.SLOTS).any(axis=1)
    assert res["segments_changed"] == res["segments_cleared"] == np.count_nonzero(live)


def test_erase_matching_entry_point_is_declared_bound_and_built():
    src = open(os.path.join(REPO, "include", "pmdfc_cceh.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+pmdfc_cceh_erase_matching\s*\(", src)
    assert re.search(r"#define\s+PMDFC_MATCH_MAX\s+1024\b", src)
    assert re.search(r"typedef\s+struct\s+pmdfc_erase_matching_result\s*\{[^}]*\buint64_t\s+removed\s*;[^}]*"
                     r"\buint32_t\s+segments_scanned\s*;[^}]*\buint32_t\s+segments_changed\s*;[^}]*"
                     r"\buint32_t\s+segments_cleared\s*;[^}]*\}\s*pmdfc_erase_matching_result_t\s*;", src)
    from pmdfc_amd.engine import EXPORTS, LIB_PATH, MATCH_MAX, load_library
    import pmdfc_amd as P
    assert "pmdfc_cceh_erase_matching" in EXPORTS and MATCH_MAX == M.MATCH_MAX == 1024
    out = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "pmdfc_cceh_erase_matching" in {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert load_library().pmdfc_cceh_erase_matching is not None and hasattr(P.CCEH, "EraseMatching")
    from pmdfc_amd.kv import KV, KV_EXPORTS, KV_LIB_PATH
    out = subprocess.run(["nm", "-D", "--defined-only", KV_LIB_PATH], capture_output=True, text=True, check=True).stdout
    syms = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert "pmdfc_kv_erase_matching" in KV_EXPORTS and "pmdfc_kv_erase_matching" in syms
    assert hasattr(KV, "erase_matching") and hasattr(KV, "invalidate_inodes")
