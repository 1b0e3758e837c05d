"""CPU checks behind tests/test_gpu_get_paths.py and the knob tests of
tests/test_gpu_options.py (no GPU here):
  - the probe-shape stream (scenarios.get_probe_shapes) stops Gets where it
    says it does, judged by the serial oracle alone -- conditions on the
    input, not measurements: a stream that fails them is what gets fixed;
  - every environment knob of csrc/knobs.h is set by some GPU test."""
import ast
import glob
import os
import re

import numpy as np

from conftest import REPO
import scenarios as S
from oracle import oracle as O


def probe_lines(o, q):
    """Per query: (lines the oracle's early-exit Get read, status)."""
    lines = np.empty(q.size, np.int64)
    st = np.empty(q.size, np.uint8)
    last = o.stats()["get_lines"]
    for i in range(q.size):
        st[i] = o.get(q[i:i + 1])[1][0]
        now = o.stats()["get_lines"]
        lines[i] = now - last
        last = now
    return lines, st


def test_probe_shape_stream_covers_every_stop():
    depth, ins, vals, q = S.get_probe_shapes(O.hash64)
    o = O.OracleCCEH(depth)
    assert np.all(o.insert(ins, vals) == O.ST_INSERTED)  # every insert stored
    assert np.unique(ins).size == ins.size
    assert o.stats()["splits"] == 0 and o.depth == depth and o.num_segments == 1 << depth
    lines, st = probe_lines(o, q)
    s = o.stats()
    assert s["early_exit_mismatch"] == 0
    assert s["get_lines"] == int(lines.sum())
    reserved = st == O.ST_RESERVED_KEY
    assert int(reserved.sum()) == 2 and np.all(lines[reserved] == 0)
    assert np.all(lines[~reserved] >= 1) and np.all(lines <= 8)
    home = (O.hash64(q) & np.uint64(0xFF)).astype(np.int64)
    hit, miss = st == O.ST_HIT, st == O.ST_MISS
    assert np.all(hit | miss | reserved)
    every = set(range(1, 9))
    for what, sel in (("hit", hit), ("miss", miss)):
        for parity in (0, 1):
            got = set(lines[sel & (home % 2 == parity)].tolist())
            assert got == every, (what, "odd" if parity else "even", sorted(got))
    wrap = home >= S.GET_SHAPE_WRAP_LINE
    assert set(lines[hit & wrap].tolist()) == every
    wm = set(lines[miss & wrap].tolist())
    assert {1, 8} <= wm and len(wm & {2, 3, 4, 5, 6, 7}) >= 3, sorted(wm)
    # a wrapping miss that stops past line 255, from an even and from an odd home line
    for parity in (0, 1):
        sel = miss & wrap & (home % 2 == parity)
        assert np.any(sel & (lines < 8) & (home + lines - 1 > 255)), parity
    # a key asked twice gets the same answer
    assert np.unique(q).size < q.size


def _env_sets(path):
    """PMDFC_* names a test source SETS: monkeypatch.setenv("NAME", ..), a
    subscript store x["NAME"] = .., or a key of a dict literal (the env dicts
    the child-process tests pass on).  Parsed, so comments and docstrings do
    not count; a name inside a child script's source string counts where that
    script sets it the same way."""
    names = set()

    def walk(tree):
        for n in ast.walk(tree):
            if isinstance(n, ast.Call) and getattr(n.func, "attr", "") == "setenv" and n.args:
                a = n.args[0]
                if isinstance(a, ast.Constant) and isinstance(a.value, str):
                    names.add(a.value)
            elif isinstance(n, (ast.Assign, ast.AugAssign)):
                for t in (n.targets if isinstance(n, ast.Assign) else [n.target]):
                    if isinstance(t, ast.Subscript) and isinstance(t.slice, ast.Constant):
                        names.add(t.slice.value)
            elif isinstance(n, ast.Dict):
                for k in n.keys:
                    if isinstance(k, ast.Constant) and isinstance(k.value, str):
                        names.add(k.value)
            elif isinstance(n, ast.Constant) and isinstance(n.value, str) and "PMDFC_" in n.value and "\n" in n.value:
                try:  # a child script kept in a string
                    walk(ast.parse(n.value))
                except SyntaxError:
                    pass

    with open(path) as f:
        walk(ast.parse(f.read()))
    return {x for x in names if isinstance(x, str) and x.startswith("PMDFC_")}


def test_every_knob_is_driven_off_default():
    """A knob of knobs.h that no GPU test sets is a branch of the shipped
    library that never ran: each name must be set (not just mentioned) in some
    tests/test_gpu_*.py."""
    with open(os.path.join(REPO, "pmdfc_amd", "csrc", "knobs.h")) as f:
        knobs = sorted(set(re.findall(r'"(PMDFC_[A-Z0-9_]+)"', f.read())))
    assert len(knobs) >= 23, knobs  # (the pattern still finds them)
    set_by = {}
    for path in sorted(glob.glob(os.path.join(REPO, "tests", "test_gpu_*.py"))):
        for name in _env_sets(path):
            set_by.setdefault(name, []).append(os.path.basename(path))
    missing = [k for k in knobs if k not in set_by]
    assert not missing, f"knobs no GPU test sets: {missing}"
