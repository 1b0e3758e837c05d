"""The serial oracle's answers to a scenarios.drop_log_stream, computed once
and shared by tests/test_drop_log_ref.py (the stream itself) and
tests/test_gpu_drop_log.py (the engine at and past its drop log's capacity).
"""
import numpy as np

import scenarios as S
from oracle import oracle as O

INVALID = np.uint64(2**64 - 1)


def _dump_record(o):
    d = o.dump()
    return dict(depth=int(d["depth"]), nseg=int(len(d["local_depth"])), keys_sha=S.sha(d["keys"]),
                values_sha=S.sha(d["values"]), local_depth_sha=S.sha(d["local_depth"].astype(np.uint64))), d["keys"]


def reference(s, upsert=False, after=True):
    """The oracle through the image, the batch and (after=True) the batch of
    the spare segments.  -> dict: image_st, image_loss; batch_out, batch_st,
    batch_loss (split_loss after the batch), batch_dump (depth, nseg and the
    hashes of keys / values / local depths); dropped (the stored inserts the
    batch's splits dropped, sorted), batch_dropped (per op of the batch: a Get
    of a dropped key); after_out, after_st, after_loss, after_dump."""
    o = O.OracleCCEH(s["depth"], upsert=upsert)
    ops, keys, vals = s["image"]
    r = dict(image_st=o.insert(keys, vals), image_loss=int(o.stats()["split_loss"]), image_splits=int(o.stats()["splits"]))
    bops, bkeys, bvals = s["batch"]
    r["batch_out"], r["batch_st"] = o.mixed(bops, bkeys, bvals)
    r["batch_loss"] = int(o.stats()["split_loss"])
    r["batch_dump"], table_keys = _dump_record(o)
    ins = bops == S.OP_INSERT
    stored = np.concatenate([keys, bkeys[ins][r["batch_st"][ins] == O.ST_INSERTED]])
    r["dropped"] = np.setdiff1d(stored, table_keys[table_keys != INVALID])
    r["batch_dropped"] = ~ins & np.isin(bkeys, r["dropped"])
    if after:
        r["after_out"], r["after_st"] = o.mixed(*s["after"])
        r["after_loss"] = int(o.stats()["split_loss"])
        r["after_dump"], _ = _dump_record(o)
    o.close()
    return r
