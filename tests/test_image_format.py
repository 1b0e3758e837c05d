"""The table image on the host (pmdfc_amd/image.py, pmdfc_amd/csrc/image.h): no GPU.

An image is the canonical dump and nothing else, so the serial oracle's dump
gives the bytes an engine holding the same table must snapshot
(tests/test_gpu_snapshot.py).  Here: the Python builder and parser round-trip
the oracle's dumps, and both validators -- image.py's and image.h's, the
latter through a stand-alone program built with the address and
undefined-behaviour sanitizers -- accept the untouched image and refuse each
corruption.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import scenarios as S
from oracle import oracle as O
from pmdfc_amd import image as I

from conftest import REPO

CASES = ["cap2_ins3k", "dup_wrap", "split_loss"]


@pytest.fixture(scope="module")
def tables():
    """name -> (initial_depth, the oracle's dump after the scenario's stream);
    `fresh`: CCEH_hybrid(16) untouched."""
    sc = S.scenarios(O.hash64)
    out = {}
    for name in CASES:
        init_cap, conv, ops, keys, vals = sc[name]
        d0 = O.OracleCCEH.depth_for_hybrid(init_cap)
        o = O.OracleCCEH(d0)
        o.mixed(ops, keys, vals)
        out[name] = (d0, o.dump())
    out["fresh"] = (4, O.OracleCCEH(4).dump())
    return out


def corruptions(img: bytes, initial_depth: int):
    """name -> a corrupt copy of a valid image.  Where the case is about the
    depths, the header's min / max / depth are kept true to the bytes, so the
    refusal is the range check's or the tiling's and not the summary's."""
    a = np.frombuffer(img, np.uint8)
    H = I.HEADER_BYTES
    nseg = I.parse_header(img)["nseg"]
    assert nseg % 4096 != 0  # (room for one more depth byte)

    def u32(v):
        return np.frombuffer(np.uint32(v).tobytes(), np.uint8)

    def u64(v):
        return np.frombuffer(np.uint64(v).tobytes(), np.uint8)

    def with_last_depth(v):
        b = a.copy()
        b[H + nseg - 1] = v
        ld = b[H:H + nseg]
        b[24:28], b[28:32], b[32:36] = u32(max(initial_depth, int(ld.max()))), u32(int(ld.min())), u32(int(ld.max()))
        return b.tobytes()

    magic = a.copy()
    magic[3] ^= 0x20
    version = a.copy()
    version[8] = 2
    # one segment too many: the last one twice (the running sum passes 1)
    over = np.concatenate([a, a[-I.SEGMENT_BYTES:]])
    over[H + nseg] = a[H + nseg - 1]
    over[40:48], over[56:64] = u64(nseg + 1), u64(I.total_bytes(nseg + 1))
    assert over.size == I.total_bytes(nseg + 1)
    return {
        "magic": magic.tobytes(),
        "version": version.tobytes(),
        "one_byte_short": img[:-1],
        "below_initial_depth": with_last_depth(initial_depth - 1),
        "depth_31": with_last_depth(31),
        "gap": with_last_depth(int(a[H + nseg - 1]) + 1),  # the last segment covers half its range
        "overlap": over.tobytes(),
    }


@pytest.mark.parametrize("name", CASES + ["fresh"])
def test_round_trip(name, tables):
    d0, od = tables[name]
    img = I.image_from_dump(od, d0)
    h = I.validate(img)
    nseg = len(od["local_depth"])
    assert h["nseg"] == nseg and h["initial_depth"] == d0 and h["depth"] == od["depth"]
    assert (h["shard_bits"], h["shard_id"], h["version"]) == (0, 0, 1)
    assert h["total_bytes"] == len(img) == 4096 + (nseg + 4095) // 4096 * 4096 + nseg * 16384
    assert h["live"] == int((od["keys"] != np.uint64(2**64 - 1)).sum())
    assert (h["min_ld"], h["max_ld"]) == (int(od["local_depth"].min()), int(od["local_depth"].max()))
    back = I.dump_from_image(img)
    assert back["depth"] == od["depth"]
    for f in ("dir_canon", "local_depth", "prefix", "keys", "values"):
        assert np.array_equal(back[f], od[f]), f
    assert I.image_from_dump(back, d0) == img
    # accepted as bytes, a numpy array and a memoryview alike
    assert I.parse_header(np.frombuffer(img, np.uint8)) == I.parse_header(memoryview(img)) == I.parse_header(img)


def test_empty_slots_are_written_as_zero(tables):
    d0, od = tables["cap2_ins3k"]
    dirty = dict(od)
    dirty["values"] = np.where(od["keys"] == np.uint64(2**64 - 1), np.uint64(0xDEAD), od["values"])
    assert I.image_from_dump(dirty, d0) == I.image_from_dump(od, d0)


def test_sharded_image_round_trip():
    """A shard's dump (prefixes carry the shard id above the local bits)."""
    ld = np.array([3, 4, 4], np.uint32)
    keys = np.full(3 * 1024, 2**64 - 1, np.uint64)
    d = {"local_depth": ld, "keys": keys, "values": np.zeros_like(keys)}
    img = I.image_from_dump(d, 2, shard_bits=2, shard_id=3)
    back = I.dump_from_image(img)
    assert back["depth"] == 4
    assert back["prefix"].tolist() == [0b110, 0b1110, 0b1111]
    assert back["dir_canon"].tolist() == [0, 0, 1, 2]


@pytest.mark.parametrize("name", CASES + ["fresh"])
def test_python_validator_refuses_each_corruption(name, tables):
    d0, od = tables[name]
    img = I.image_from_dump(od, d0)
    I.validate(img)
    bad = corruptions(img, d0)
    assert len(bad) == 7
    for case, b in bad.items():
        with pytest.raises(I.ImageError):
            I.validate(b)
            pytest.fail(f"{name}/{case} accepted")


SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _build_validator(tmp_path):
    """The stand-alone program with the sanitizers, their runtimes linked
    statically (a program whose sanitizer runtime is a shared library refuses
    to start in a process that preloads any other library) or else
    dynamically, or without them when neither builds and starts.
    -> (path, how it was built)."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    src = os.path.join(REPO, "tests", "cpp", "test_image_validate.cpp")
    tried = []
    for how, flags in (("static sanitizers", SANITIZE + ["-static-libasan", "-static-libubsan"]),
                       ("sanitizers", SANITIZE), ("UNSANITIZED", [])):
        exe = str(tmp_path / ("validate_" + how.split()[0].lower()))
        b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-o", exe, src] + flags,
                           capture_output=True, text=True)
        if b.returncode == 0:
            r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
            if not flags or "runtime does not come first" not in r.stderr:
                assert r.returncode == 0 and r.stdout.strip() == "OK", (how, r.stdout[-2000:], r.stderr[-2000:])
                return exe, how
            tried.append(how + ": its runtime must be loaded first")
        else:
            tried.append(how + ": does not build")
    raise AssertionError(tried)


def test_cpp_validator_under_sanitizers(tmp_path, tables):
    """image.h's validator, compiled alone (no HIP) into a program of its own:
    its built-in accept / refuse table, then the same image files the Python
    validator saw.  Nothing sanitized is loaded into this process."""
    exe, how = _build_validator(tmp_path)
    paths, want = [], []
    for name, (d0, od) in tables.items():
        img = I.image_from_dump(od, d0)
        for case, b in [("untouched", img)] + list(corruptions(img, d0).items()):
            p = tmp_path / f"{name}.{case}.img"
            p.write_bytes(b)
            paths.append(str(p))
            want.append(case == "untouched")
    r = subprocess.run([exe] + paths, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(paths)
    for p, ok, line in zip(paths, want, lines):
        code = int(line.split()[0])
        assert (code == 0) == ok and code >= 0, (os.path.basename(p), line)
    if how == "UNSANITIZED":
        pytest.skip("no usable sanitizer runtime on this machine: the validator passed every case UNSANITIZED")
