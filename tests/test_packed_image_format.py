"""The packed table image on the host (pmdfc_amd/image.py,
pmdfc_amd/csrc/packed_image.h): no GPU.

A packed image holds what the version-1 image holds -- the canonical dump --
with the empty slots left out: occupancy words and the dense live pairs.  Here:
the Python builder and parser round-trip the oracle's dumps, pack / unpack
convert to and from the version-1 bytes exactly, and both validators --
image.py's and packed_image.h's, the latter through a stand-alone program built
with the address and undefined-behaviour sanitizers -- accept the untouched
image and refuse each corruption.
"""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from pmdfc_amd import image as I

from conftest import REPO
from test_image_format import CASES, SANITIZE, corruptions, tables  # noqa: F401  (tables: the module's fixture)

INVALID = np.uint64(2**64 - 1)


def packed_corruptions(packed: bytes, initial_depth: int):
    """name -> a corrupt copy of a valid packed image: the packed format's own
    cases, then the version-1 depth corruptions (test_image_format.corruptions
    of the unpacked image, packed again without validation).  A padding that
    is empty in this image has no case."""
    a = np.frombuffer(packed, np.uint8)
    h = I.validate_packed(packed)
    nseg, live = h["nseg"], h["live"]
    H, o, p = I.HEADER_BYTES, I.packed_occ_offset(nseg), I.packed_pairs_offset(nseg)

    def edit(f):
        b = a.copy()
        f(b)
        return b.tobytes()

    def flip(b, at, bit=1):
        b[at] ^= bit

    def set_live(b, v):
        b[48:56] = np.frombuffer(struct.pack("<Q", v), np.uint8)

    out = {
        "magic": edit(lambda b: flip(b, 3, 0x20)),
        "v1_magic": edit(lambda b: b.__setitem__(slice(0, 8), np.frombuffer(I.MAGIC, np.uint8))),
        "version": edit(lambda b: b.__setitem__(8, 2)),
        "one_byte_short": packed[:-1],
        "occ_bit_flipped": edit(lambda b: flip(b, o + 77 % (nseg * 128), 0x04)),
        "live_plus_one": edit(lambda b: set_live(b, live + 1)),
        "header_padding": edit(lambda b: flip(b, 64)),
    }
    if live:
        out["live_minus_one"] = edit(lambda b: set_live(b, live - 1))
    if nseg % 4096:
        out["depth_padding"] = edit(lambda b: flip(b, H + nseg))
    if nseg % 32:
        out["occ_padding"] = edit(lambda b: flip(b, p - 1))
    if live % 256:
        out["pair_padding"] = edit(lambda b: flip(b, p + live * 16))
    for case, bad in corruptions(I.unpack(packed), initial_depth).items():
        if case in ("magic", "version", "one_byte_short"):
            continue
        v = np.frombuffer(bad, np.uint8)
        n = struct.unpack("<Q", v[40:48].tobytes())[0]
        pairs = v[H + I.depth_bytes(n):].view(np.uint64).reshape(-1, 2)
        out[case] = I.packed_from_dump({"local_depth": v[H:H + n], "keys": pairs[:, 0], "values": pairs[:, 1]},
                                       initial_depth)
    return out


@pytest.mark.parametrize("name", CASES + ["fresh"])
def test_round_trip(name, tables):
    d0, od = tables[name]
    packed = I.packed_from_dump(od, d0)
    h = I.validate_packed(packed)
    nseg = len(od["local_depth"])
    live = int((od["keys"] != INVALID).sum())
    assert (h["nseg"], h["live"], h["initial_depth"], h["depth"], h["version"]) == (nseg, live, d0, od["depth"], 1)
    assert len(packed) == I.packed_total_bytes(nseg, live) == h["total_bytes"]
    assert len(packed) == 4096 + (nseg + 4095) // 4096 * 4096 + (nseg * 128 + 4095) // 4096 * 4096 + \
        (live * 16 + 4095) // 4096 * 4096
    back = I.dump_from_packed(packed)
    assert back["depth"] == od["depth"]
    for f in ("dir_canon", "local_depth", "prefix", "keys", "values"):
        assert np.array_equal(back[f], od[f]), f
    v1 = I.image_from_dump(od, d0)
    assert I.unpack(packed) == v1
    assert I.pack(v1) == packed
    assert I.is_packed(packed) and not I.is_packed(v1)
    # the version-1 validator does not take it, nor the packed one a version-1 image
    with pytest.raises(I.ImageError):
        I.validate(packed)
    with pytest.raises(I.ImageError):
        I.validate_packed(v1)


def test_layout_by_hand():
    """Two segments of depth 1; slots 0 and 33 of the first, 1023 of the second."""
    keys = np.full(2048, INVALID, np.uint64)
    vals = np.zeros(2048, np.uint64)
    for s, k in ((0, 10), (33, 11), (1024 + 1023, 12)):
        keys[s], vals[s] = k, k + 100
    vals[5] = 0xDEAD  # the value of an empty slot is not in the image
    packed = np.frombuffer(I.packed_from_dump({"local_depth": [1, 1], "keys": keys, "values": vals}, 1), np.uint8)
    assert packed.size == 4096 * 4 and packed[:8].tobytes() == b"PMDFCPAK"
    words = packed[8192:8192 + 256].view("<u4")
    assert words[0] == 1 and words[1] == 2 and words[32 + 31] == 1 << 31 and int(words.astype(np.uint64).sum()) == 3 + (1 << 31)
    assert packed[12288:12288 + 48].view("<u8").tolist() == [10, 110, 11, 111, 12, 112]
    assert not packed[12288 + 48:].any()
    assert I.unpack(packed) == I.image_from_dump({"local_depth": [1, 1], "keys": keys, "values": vals}, 1)


def test_sharded_packed_round_trip():
    ld = np.array([3, 4, 4], np.uint32)
    keys = np.full(3 * 1024, INVALID, np.uint64)
    keys[1024 + 7] = 99
    d = {"local_depth": ld, "keys": keys, "values": np.where(keys == 99, np.uint64(5), np.uint64(0))}
    packed = I.packed_from_dump(d, 2, shard_bits=2, shard_id=3)
    h = I.validate_packed(packed)
    assert (h["shard_bits"], h["shard_id"], h["live"]) == (2, 3, 1)
    assert I.unpack(packed) == I.image_from_dump(d, 2, shard_bits=2, shard_id=3)
    assert I.dump_from_packed(packed)["prefix"].tolist() == [0b110, 0b1110, 0b1111]


@pytest.mark.parametrize("name", CASES + ["fresh"])
def test_python_validator_refuses_each_corruption(name, tables):
    d0, od = tables[name]
    packed = I.packed_from_dump(od, d0)
    I.validate_packed(packed)
    bad = packed_corruptions(packed, d0)
    # the cases every table has; the three paddings where the image has them
    assert {"magic", "v1_magic", "version", "one_byte_short", "occ_bit_flipped", "live_plus_one", "header_padding",
            "depth_padding", "below_initial_depth", "depth_31", "gap", "overlap"} <= set(bad)
    if name == "cap2_ins3k":
        assert {"occ_padding", "pair_padding", "live_minus_one"} <= set(bad)
    for case, b in bad.items():
        with pytest.raises(I.ImageError):
            I.validate_packed(b)
            pytest.fail(f"{name}/{case} accepted")
        with pytest.raises(I.ImageError):  # and the host-side conversion refuses it too
            I.unpack(b)


def _build_validator(tmp_path):
    """tests/cpp/test_packed_validate.cpp as a program of its own, built the
    way test_image_format builds its validator: sanitizer runtimes linked
    statically, else dynamically, else none.  -> (path, how it was built)."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    src = os.path.join(REPO, "tests", "cpp", "test_packed_validate.cpp")
    tried = []
    for how, flags in (("static sanitizers", SANITIZE + ["-static-libasan", "-static-libubsan"]),
                       ("sanitizers", SANITIZE), ("UNSANITIZED", [])):
        exe = str(tmp_path / ("packed_validate_" + how.split()[0].lower()))
        b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-o", exe, src] + flags,
                           capture_output=True, text=True)
        if b.returncode == 0:
            r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
            if not flags or "runtime does not come first" not in r.stderr:
                assert r.returncode == 0 and r.stdout.strip() == "OK", (how, r.stdout[-2000:], r.stderr[-2000:])
                return exe, how
            tried.append(how + ": its runtime must be loaded first")
        else:
            tried.append(how + ": does not build: " + b.stderr[-500:])
    raise AssertionError(tried)


def test_cpp_validator_under_sanitizers(tmp_path, tables):
    """packed_image.h's validator, compiled alone (no HIP) into a program of
    its own: its built-in accept / refuse table, then the same image files the
    Python validator saw.  Nothing sanitized is loaded into this process."""
    exe, how = _build_validator(tmp_path)
    paths, want = [], []
    for name, (d0, od) in tables.items():
        packed = I.packed_from_dump(od, d0)
        for case, b in [("untouched", packed)] + list(packed_corruptions(packed, d0).items()):
            p = tmp_path / f"{name}.{case}.pak"
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
