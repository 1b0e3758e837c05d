"""A mixed batch at and past the capacity of its drop log (2^18 entries).

A mixed batch answers many Gets early against the pre-batch image and repairs
the ones whose key a split of the same batch dropped from the drop log
(k_mixed_verify / replay_unchecked_hit, cceh_kernels.hip).  The
contract (PMDFC_ST_SPLIT_LOST, include/pmdfc_cceh.h): up to 2^18 drops in one
batch every answer is the reference's; past that only a Get whose key a split
of the same batch dropped may come back SPLIT_LOST, with error_flags bit 16.

The streams are scenarios.drop_log_stream's (tests/test_drop_log_ref.py holds
them to what they claim on the CPU): ~9,900 copies of the split shapes
dense_drop and dense_drop_wrap in a depth-14 table, 262,144 or 262,148 drops in
one batch of ~820,000 ops, the serial oracle's answers computed once for all
cases (drop_log_ref.reference).  PMDFC_MIXED_JOIN is a process knob, so each
case is one child process that reads streams and answers from a file.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import drop_log_ref as DR
import scenarios as S
from pmdfc_amd.workload import uniform_keys

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pmdfc_amd as P  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_SPLIT_LOST = 1 << 16
SPARE = 10


@pytest.fixture(scope="module")
def case_file(tmp_path_factory):
    """The two full-size streams and the oracle's answers, in one file: `cap`
    drops exactly 2^18 entries, `over` 2^18 + 4 and keeps ten segments back;
    `overu`: the answers to `over` under last-writer-wins inserts."""
    z = {}
    for name, target, spare, sample in (("cap", S.DROP_LOG_CAP, 0, 4), ("over", S.DROP_LOG_CAP + 4, SPARE, 32)):
        s = S.drop_log_stream(target, depth=14, seed=5, spare=spare, gets_per_segment=sample)
        for part in ("image", "batch", "after"):
            for f, a in zip(("ops", "keys", "vals"), s[part]):
                z[f"{name}_{part}_{f}"] = a
        z[f"{name}_batch_class"] = s["batch_class"]
        for tag, upsert in ((name, False), (name + "u", True)):
            if upsert and name == "cap":
                continue
            r = DR.reference(s, upsert=upsert, after=spare > 0)
            assert r["image_loss"] == 0 and r["batch_loss"] == target
            for k, v in r.items():
                if k != "dropped":
                    z[f"{tag}_{k}"] = np.array(json.dumps(v)) if isinstance(v, dict) else np.asarray(v)
    path = str(tmp_path_factory.mktemp("drop_log") / "cases.npz")
    np.savez(path, **z)
    return path


CHILD = r'''
import json, sys, time, numpy as np
sys.path.insert(0, "tests")
import scenarios as S
import pmdfc_amd as P
z = np.load(sys.argv[1])
case, upsert = sys.argv[2], sys.argv[3] == "1"
ref = case + ("u" if upsert else "")

def table_record(t):
    d = t.dump()
    return dict(depth=int(d["depth"]), nseg=int(len(d["local_depth"])), keys_sha=S.sha(d["keys"]),
                values_sha=S.sha(d["values"]), local_depth_sha=S.sha(d["local_depth"].astype(np.uint64)))

def image(t, name):
    st = t.Insert(z[name + "_image_keys"], z[name + "_image_vals"])
    s = t.stats()
    return bool(np.all(st == P.ST_INSERTED)) and s["split_loss"] == 0 and s["splits"] == 0

def batch(t, name, ref, part):
    """One mixed batch against the oracle's answers, counted by kind of op."""
    ops = z[f"{name}_{part}_ops"]
    t0 = time.perf_counter()
    out, st = t.Mixed(ops, z[f"{name}_{part}_keys"], z[f"{name}_{part}_vals"])
    sec = time.perf_counter() - t0
    eout, est = z[f"{ref}_{part}_out"], z[f"{ref}_{part}_st"]
    ins = ops == S.OP_INSERT
    exact = (st == est) & (out == eout)
    lost = st == P.ST_SPLIT_LOST
    r = dict(ops=int(ops.size), seconds=round(sec, 3),
             inserts_wrong=int((ins & ~exact).sum()),
             gets_wrong=int((~ins & ~exact & ~lost).sum()),    # neither the oracle's answer nor SPLIT_LOST
             lost=int(lost.sum()), lost_with_value=int((lost & (out != 0)).sum()),
             lost_inserts=int((lost & ins).sum()))
    if part == "batch":
        dropped, cls = z[ref + "_batch_dropped"], z[name + "_batch_class"]
        r["lost_not_dropped"] = int((lost & ~dropped).sum())
        r["lost_by_class"] = {S.DL_CLASS_NAMES[c]: int((lost & ~dropped & (cls == c)).sum()) for c in range(1, 7)}
        r["wrong_by_class"] = {S.DL_CLASS_NAMES[c]: int((~exact & ~lost & (cls == c)).sum()) for c in range(7)}
        r["dropped_gets"] = int(dropped.sum())
    s = t.stats()
    r["error_flags"] = int(s["error_flags"])
    r["split_loss"] = int(s["split_loss"])
    r["want_split_loss"] = int(z[f"{ref}_{part}_loss"])
    r["table_equal"] = table_record(t) == json.loads(str(z[f"{ref}_{part}_dump"]))
    return r

res = {}
t = P.CCEH(depth=14, max_batch=1 << 21, max_segments=32768, upsert=upsert)
res["image"] = image(t, case)
res["batch"] = batch(t, case, ref, "batch")
if case == "over":
    res["after"] = batch(t, case, ref, "after")
    if not upsert:
        t.reset()
        res["reset_error_flags"] = int(t.stats()["error_flags"])
        res["replay_image"] = image(t, "cap")
        res["replay"] = batch(t, "cap", "cap", "batch")
t.close()
print(json.dumps(res))
'''

_RESULTS = {}


def child(case_file, case, mode=None, upsert=False):
    """One child per (case, mode, upsert), run once: its last output line."""
    key = (case, mode, upsert)
    if key not in _RESULTS:
        e = dict(os.environ)
        e.pop("PMDFC_MIXED_JOIN", None)
        if mode is not None:
            e["PMDFC_MIXED_JOIN"] = mode
        r = subprocess.run([sys.executable, "-c", CHILD, case_file, case, "1" if upsert else "0"], cwd=REPO, env=e,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        _RESULTS[key] = json.loads(r.stdout.strip().splitlines()[-1])
        print(key, json.dumps(_RESULTS[key]))
    return _RESULTS[key]


def _exact(b, split_loss):
    """A batch that equals the oracle's everywhere, with no SPLIT_LOST."""
    assert b["inserts_wrong"] == 0 and b["gets_wrong"] == 0, b
    assert b["lost"] == 0, b
    assert b["table_equal"], b
    assert b["split_loss"] == b["want_split_loss"] == split_loss, b


@pytest.mark.parametrize("mode", ["0", "1"])
def test_at_capacity(case_file, mode):
    """Exactly 2^18 drops in one batch: the log is full and nothing is lost.
    Every op's status and value and the final table equal the oracle's.
    (Measured on an MI355X: the batch of 822,166 ops 0.09 s in either mode,
    the case with its child process and the table's dump 3.3 s; building both
    streams and the oracle's answers, once for the file, 2.7 s.)"""
    r = child(case_file, "cap", mode)
    assert r["image"]
    _exact(r["batch"], S.DROP_LOG_CAP)
    assert r["batch"]["error_flags"] == 0


OVERFLOW = [("0", False), ("1", False), (None, True)]
OVERFLOW_IDS = ["join0", "join1", "upsert"]


@pytest.mark.parametrize("mode,upsert", OVERFLOW, ids=OVERFLOW_IDS)
def test_overflow(case_file, mode, upsert):
    """2^18 + 4 drops in one batch: the inserts, the final table and split_loss
    are the oracle's; a Get either has the oracle's answer or is
    (SPLIT_LOST, 0), and SPLIT_LOST falls only on Gets of keys the batch's
    splits dropped -- survivors of a splitting segment, its head keys,
    bystander keys, triggers and absent keys are exact; error_flags is bit 16
    exactly when some Get is SPLIT_LOST, and nothing else.
    Every victim is asked for in both rounds (which four drops the log loses
    is up to the device), so a lost drop that went unreported shows as a wrong
    answer: without the `nd > kDropLog` branch of replay_unchecked_hit exactly
    4 Gets are wrong.
    (Measured on an MI355X: the batch of 1,378,278 ops 0.12 s in either mode,
    0.06 s under upsert, 500,296 of its 524,296 Gets of dropped keys
    SPLIT_LOST, 8 under upsert; the case, whose child also runs
    test_after_overflow's batches, 5.1 s, 4.1 s under upsert.)"""
    r = child(case_file, "over", mode, upsert)
    assert r["image"]
    b = r["batch"]
    assert b["inserts_wrong"] == 0 and b["lost_inserts"] == 0, b
    assert b["table_equal"] and b["split_loss"] == b["want_split_loss"] == S.DROP_LOG_CAP + 4, b
    assert b["gets_wrong"] == 0, b
    assert b["lost_with_value"] == 0, b
    assert b["lost_not_dropped"] == 0, b
    assert b["lost"] <= b["dropped_gets"]
    assert b["error_flags"] == (ERR_SPLIT_LOST if b["lost"] else 0), b


@pytest.mark.parametrize("mode,upsert", OVERFLOW, ids=OVERFLOW_IDS)
def test_after_overflow(case_file, mode, upsert):
    """The next mixed batch on the same table (ten kept-back dense_drop
    segments split: 280 drops) is exact with no SPLIT_LOST -- the log started
    again at 0 -- while bit 16 stays as the overflowing batch left it.  After
    reset() error_flags is 0 and the at-capacity batch, replayed on the same
    handle, is exact."""
    r = child(case_file, "over", mode, upsert)
    _exact(r["after"], S.DROP_LOG_CAP + 4 + 28 * SPARE)
    assert r["after"]["error_flags"] == r["batch"]["error_flags"]
    if not upsert:
        assert r["reset_error_flags"] == 0
        assert r["replay_image"]
        _exact(r["replay"], S.DROP_LOG_CAP)
        assert r["replay"]["error_flags"] == 0


# The same builder small: 300 drops at depth 6, so that a failure of the
# builder cannot pass for a failure of the overflow path.
@pytest.fixture(scope="module")
def small():
    s = S.drop_log_stream(300, depth=6, seed=5)
    return s, DR.reference(s, after=False)


@pytest.mark.parametrize("cut", ["one_batch", "batches_of_997", "general"])
def test_small_stream_is_exact(small, cut):
    """300 drops in one batch (more than any split shape logs), whole, cut
    into batches of 997 ops from the image's first insert on, and padded with
    Gets of absent keys past the two-launch path's 8192 ops (the general
    pipeline, whose verify pass reads the drop log)."""
    s, r = small
    ops, keys, vals = (np.concatenate([a, b]) for a, b in zip(s["image"], s["batch"]))
    n_img = s["image"][0].size
    want_out = np.concatenate([np.zeros(n_img, np.uint64), r["batch_out"]])
    want_st = np.concatenate([r["image_st"], r["batch_st"]])
    if cut == "general":
        pad = uniform_keys(904, 0, 8193)
        ops = np.concatenate([ops, np.zeros(pad.size, np.uint8)])
        keys = np.concatenate([keys, pad])
        vals = np.concatenate([vals, np.zeros(pad.size, np.uint64)])
        want_out = np.concatenate([want_out, np.zeros(pad.size, np.uint64)])
        want_st = np.concatenate([want_st, np.full(pad.size, P.ST_MISS, np.uint8)])
    bounds = list(range(0, keys.size, 997)) + [keys.size] if cut == "batches_of_997" else [0, n_img, keys.size]
    # max_batch 8192: the table starts at its full bucket resolution (p1max = 6), batches up to 8192 ops take k_medium
    t = P.CCEH(depth=6, max_batch=1 << 14 if cut == "general" else 8192, max_segments=256)
    t.timing(events=True)
    out, st = t.MixedBatches(ops, keys, vals, bounds)
    assert (t.timing_read()["split"][1] >= 1) == (cut == "general")  # the general pipeline ran, or never
    bad = np.nonzero((st != want_st) | (out != want_out))[0]
    assert bad.size == 0, (bad[:8], st[bad[:8]], want_st[bad[:8]])
    s_ = t.stats()
    assert s_["split_loss"] == 300 and s_["error_flags"] == 0
    d = t.dump()
    assert dict(depth=int(d["depth"]), nseg=int(len(d["local_depth"])), keys_sha=S.sha(d["keys"]),
                values_sha=S.sha(d["values"]),
                local_depth_sha=S.sha(d["local_depth"].astype(np.uint64))) == r["batch_dump"]
    t.close()
