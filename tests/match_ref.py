"""Plain reference of EraseMatching (test infrastructure): DESIGN.md 4.10 on
the model of Erase (tests/erase_ref.py).

Pure numpy/Python: no engine, no oracle library.  A stored entry with key k
matches iff (k & mask) == (p & mask) for one of the patterns p; an empty slot
never matches.  L is the distinct stored keys that match, in canonical segment
order and slot order of the table before the call, a key stored several times
taken at its first copy, and the table afterwards is

    ErasableTable(dump_before).erase_batch(L)

which is the contract: there is no reference implementation (the reference's
invalidate_inode and invalidate_fs are empty).

tests/test_match_ref.py checks the model's properties on the CPU;
tests/test_gpu_erase_matching.py checks the engine against the model.
"""
import numpy as np

from erase_ref import ErasableTable
from limits_ref import INVALID, SLOTS

MATCH_MAX = 1024
INODE_MASK = 0xFFFFFFFF00000000


def match_mask(dump, mask, patterns) -> np.ndarray:
    """Per slot of the dump (canonical order): the slot holds a matching entry."""
    keys = np.asarray(dump["keys"], np.uint64)
    pats = np.asarray(patterns, np.uint64).reshape(-1)
    if pats.size == 0:
        return np.zeros(keys.size, bool)
    m = np.uint64(mask & INVALID)
    return (keys != np.uint64(INVALID)) & np.isin(keys & m, np.unique(pats & m))


def matching_keys(dump, mask, patterns) -> np.ndarray:
    """L: the distinct matching keys, each at its first copy, in canonical
    segment order and slot order."""
    keys = np.asarray(dump["keys"], np.uint64)[match_mask(dump, mask, patterns)]
    _, first = np.unique(keys, return_index=True)
    return keys[np.sort(first)]


def erase_matching(dump, mask, patterns, upsert=False):
    """-> (the ErasableTable afterwards, the result's four fields).  No pattern:
    nothing is scanned, as the engine returns before its launch."""
    hit = match_mask(dump, mask, patterns).reshape(-1, SLOTS)
    live = (np.asarray(dump["keys"], np.uint64) != np.uint64(INVALID)).reshape(-1, SLOTS)
    per_seg, live_seg = hit.sum(axis=1), live.sum(axis=1)
    t = ErasableTable(dump, upsert)
    t.erase_batch(matching_keys(dump, mask, patterns))
    res = {"removed": int(per_seg.sum()),
           "segments_scanned": int(per_seg.size) if np.asarray(patterns).size else 0,
           "segments_changed": int(np.count_nonzero(per_seg)),
           "segments_cleared": int(np.count_nonzero((per_seg > 0) & (per_seg == live_seg)))}
    return t, res


def inode_stream(seed=2024):
    """The cleancache stream of the tests: 48 inode numbers from [2, 2^20),
    page counts 1, 2, 3, 700, 650 and 43 draws from [20, 300), keys
    inode << 32 | page index, shuffled (about 7.9k keys).
    -> (inode numbers, page counts, keys)."""
    rng = np.random.default_rng(seed)
    inos = rng.choice(np.arange(2, 1 << 20, dtype=np.uint64), 48, replace=False)
    pages = np.concatenate([np.array([1, 2, 3, 700, 650]), rng.integers(20, 300, 43)]).astype(np.int64)
    keys = np.concatenate([(np.uint64(i) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
                           for i, n in zip(inos.tolist(), pages.tolist())])
    return inos, pages, keys[rng.permutation(keys.size)]


def inode_patterns(inos) -> np.ndarray:
    return np.asarray(inos, np.uint64) << np.uint64(32)
