"""scenarios.drop_log_stream on the CPU: the stream that takes a mixed batch
to its drop log's capacity (2^18 drops in one batch) and past it is what it
claims, on the serial oracle -- so that a failure of tests/test_gpu_drop_log.py
is the engine's and not the builder's.  These are conditions on the oracle
alone.
"""
import numpy as np
import pytest

import drop_log_ref as DR
import scenarios as S
from oracle import oracle as O

# (target, depth, spare, victims asked for per segment): the two full-size streams of test_gpu_drop_log.py and
# its small one.  Past the capacity every victim is asked for: which drops the log loses is up to the device.
CASES = {"at_capacity": (S.DROP_LOG_CAP, 14, 0, 4), "overflow": (S.DROP_LOG_CAP + 4, 14, 10, 32),
         "small": (300, 6, 0, 4)}
_MADE = {}


def made(name):
    if name not in _MADE:
        target, depth, spare, sample = CASES[name]
        s = S.drop_log_stream(target, depth=depth, seed=5, spare=spare, gets_per_segment=sample)
        _MADE[name] = (s, DR.reference(s))
    return _MADE[name]


@pytest.mark.parametrize("name", list(CASES))
def test_stream_drops_exactly_its_target(name):
    s, r = made(name)
    target, depth, spare, sample = CASES[name]
    ops, keys, vals = s["image"]
    bops, bkeys, bvals = s["batch"]
    ins = bops == S.OP_INSERT
    # the image: inserts only, all stored, no split, no loss
    assert np.all(ops == S.OP_INSERT) and np.all(r["image_st"] == O.ST_INSERTED)
    assert r["image_splits"] == 0 and r["image_loss"] == 0
    # no key is inserted twice, no value is the miss value
    allins = np.concatenate([keys, bkeys[ins]])
    assert np.unique(allins).size == allins.size
    assert np.all(vals != 0) and np.all(bvals[ins] != 0)
    # the batch drops exactly the target, one split per trigger
    assert np.all(r["batch_st"][ins] == O.ST_INSERTED)
    assert r["batch_loss"] == target == r["dropped"].size
    assert r["batch_dump"]["nseg"] == (1 << depth) + int(ins.sum()) and r["batch_dump"]["depth"] == depth + 1
    # every dropped key is a victim, of line 248 (a window that does not wrap) and of line 252 (one that does)
    assert np.all(np.isin(r["dropped"], s["classes"]["victims"]))
    lines = O.hash64(r["dropped"]) & np.uint64(0xFF)
    assert set(np.unique(lines).tolist()) == {248, 252}
    assert int((lines == 252).sum()) == 12 * min(1000, target // 40)
    # the first round: a Get of a stored key hits with its value, of a trigger or an absent key misses
    first = np.arange(bops.size) < int(np.argmax(ins))
    cls = s["batch_class"]
    stored = first & np.isin(cls, (S.DL_VICTIM, S.DL_HEAD, S.DL_BY_LOW, S.DL_BY_WRAP))
    assert stored.sum() > 0 and np.all(r["batch_st"][stored] == O.ST_HIT)
    assert np.array_equal(r["batch_out"][stored], S._vals(bkeys[stored], 0xD109))
    assert np.all(r["batch_st"][first & ~stored] == O.ST_MISS)
    # the second round: the triggers hit, the dropped keys miss, nothing else changed
    second = ~first & ~ins
    assert np.all(r["batch_st"][second & (cls == S.DL_TRIGGER)] == O.ST_HIT)
    assert np.array_equal(r["batch_st"][second] == O.ST_MISS, (r["batch_dropped"] | (cls == S.DL_ABSENT))[second])
    # the Gets reach dropped victims and survivors of both kinds of window, in both rounds
    bl = O.hash64(bkeys) & np.uint64(0xFF)
    for rnd in (first, second):
        for line in (248, 252):
            v = rnd & (cls == S.DL_VICTIM) & (bl == line)
            assert (v & r["batch_dropped"]).sum() > 0 and (v & ~r["batch_dropped"]).sum() > 0, (name, line)
    # Gets of stored keys whose window does not wrap: up to the capacity each scans the whole log once any
    # loss exists (past it none does), so the default sample keeps them to 2^17 a batch
    low = ~ins & np.isin(cls, (S.DL_VICTIM, S.DL_BY_LOW)) & (bl < 249)
    if sample == 4:
        assert int(low.sum()) <= 1 << 17
    else:  # every victim, in both rounds
        assert int((~ins & (cls == S.DL_VICTIM)).sum()) == 2 * s["classes"]["victims"].size


def test_spare_segments_split_later():
    """The batch of the kept-back segments: ten more N(7) splits, 280 more drops."""
    s, r = made("overflow")
    aops, akeys, _ = s["after"]
    ins = aops == S.OP_INSERT
    assert int(ins.sum()) == 10 and np.array_equal(akeys[ins], s["classes"]["spare_triggers"])
    assert np.all(r["after_st"][ins] == O.ST_INSERTED)
    assert r["after_loss"] - r["batch_loss"] == 280
    assert r["after_dump"]["nseg"] == r["batch_dump"]["nseg"] + 10
    first = np.arange(aops.size) < int(np.argmax(ins))
    sv = np.isin(akeys, s["classes"]["spare_victims"])
    assert np.all(r["after_st"][first & sv] == O.ST_HIT)
    assert int((r["after_st"][~first & ~ins & sv] == O.ST_MISS).sum()) == 280  # every victim is asked for
