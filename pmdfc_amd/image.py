"""The table image of `CCEH.snapshot` / `CCEH.restore` on the host (no GPU call).

The format (pmdfc_amd/csrc/image.h) is one contiguous
little-endian buffer:

    [0, 4096)   header: magic "PMDFCIMG", u32 version (1), initial_depth,
                shard_bits, shard_id, depth, min local depth, max local depth,
                u32 0, u64 nseg, u64 live entries, u64 total bytes; rest zero
    [4096, S)   nseg local-depth bytes in canonical order, zero-padded to a
                multiple of 4096
    [S, total)  nseg x 1024 x {u64 key, u64 value} in canonical order, the
                value of an empty slot (key == INVALID) 0

It is the canonical dump (`CCEH.dump()`, and any dict of that shape) and
nothing else: prefixes and the logical directory follow from the local depths
in order, occupancy is key != INVALID.
"""
from __future__ import annotations

import struct

import numpy as np

MAGIC = b"PMDFCIMG"
VERSION = 1
HEADER_BYTES = 4096
ALIGN = 4096
SLOTS = 1024
SEGMENT_BYTES = SLOTS * 16
MAX_LOCAL_DEPTH = 30
INVALID = np.uint64(0xFFFFFFFFFFFFFFFF)
_HDR = struct.Struct("<8s8I3Q")  # 64 bytes
FIELDS = ("version", "initial_depth", "shard_bits", "shard_id", "depth", "min_ld", "max_ld")


class ImageError(ValueError):
    pass


def depth_bytes(nseg: int) -> int:
    return (nseg + ALIGN - 1) // ALIGN * ALIGN


def total_bytes(nseg: int) -> int:
    return HEADER_BYTES + depth_bytes(nseg) + nseg * SEGMENT_BYTES


def _bytes(buf) -> np.ndarray:
    if isinstance(buf, (bytes, bytearray, memoryview)):
        return np.frombuffer(buf, dtype=np.uint8)
    if hasattr(buf, "detach"):  # a torch tensor
        buf = buf.detach().cpu().numpy()
    return np.ascontiguousarray(buf).view(np.uint8).reshape(-1)


def parse_header(buf) -> dict:
    """The header's fields; ImageError for a wrong magic, version or byte count
    (the checks of image.h's parse_header)."""
    b = _bytes(buf)
    if b.size < HEADER_BYTES:
        raise ImageError("image shorter than its header")
    magic, *w = _HDR.unpack(b[:_HDR.size].tobytes())
    if magic != MAGIC:
        raise ImageError("image magic mismatch")
    h = dict(zip(FIELDS, w[:7]))
    h["nseg"], h["live"], h["total_bytes"] = w[8], w[9], w[10]
    if h["version"] != VERSION:
        raise ImageError("unknown image format version")
    if not (1 <= h["initial_depth"] <= MAX_LOCAL_DEPTH and h["shard_bits"] <= min(h["initial_depth"], 16)
            and h["shard_id"] < (1 << h["shard_bits"])):
        raise ImageError("image geometry out of range")
    if h["nseg"] == 0 or h["total_bytes"] != total_bytes(h["nseg"]) or b.size != h["total_bytes"]:
        raise ImageError("image byte count inconsistent with its segment count")
    if w[7] != 0 or b[_HDR.size:HEADER_BYTES].any():
        raise ImageError("image padding not zero")
    return h


def validate(buf) -> dict:
    """parse_header plus the local depths: each in [initial_depth, 30], tiling
    the shard's hash space exactly, and agreeing with the header's min, max and
    depth (image.h's validate_depths).  Returns the header."""
    b = _bytes(buf)
    h = parse_header(b)
    nseg = h["nseg"]
    ld = b[HEADER_BYTES:HEADER_BYTES + nseg].astype(np.int64)
    if (ld < h["initial_depth"]).any() or (ld > MAX_LOCAL_DEPTH).any():
        raise ImageError("image local depth out of range")
    span = np.int64(1) << (MAX_LOCAL_DEPTH - ld)
    start = np.cumsum(span) - span
    if (start & (span - 1)).any() or int(span.sum()) != 1 << (MAX_LOCAL_DEPTH - h["shard_bits"]):
        raise ImageError("image local depths do not tile the hash space")
    if b[HEADER_BYTES + nseg:HEADER_BYTES + depth_bytes(nseg)].any():
        raise ImageError("image padding not zero")
    if (int(ld.min()), int(ld.max())) != (h["min_ld"], h["max_ld"]) or \
            h["depth"] != max(h["initial_depth"], h["max_ld"]):
        raise ImageError("image header disagrees with its local depths")
    return h


def image_from_dump(dump: dict, initial_depth: int, shard_bits: int = 0, shard_id: int = 0) -> bytes:
    """The image bytes of a canonical dump (`CCEH.dump()` or a dict of the
    same shape: local_depth, keys, values in canonical order)."""
    ld = np.asarray(dump["local_depth"]).astype(np.uint8)
    nseg = int(ld.size)
    keys = np.ascontiguousarray(dump["keys"], dtype=np.uint64)
    vals = np.ascontiguousarray(dump["values"], dtype=np.uint64)
    if keys.size != nseg * SLOTS or vals.size != nseg * SLOTS:
        raise ImageError("dump arrays do not match its segment count")
    live = keys != INVALID
    out = np.zeros(total_bytes(nseg), np.uint8)
    max_ld = int(ld.max())
    out[:_HDR.size] = np.frombuffer(_HDR.pack(MAGIC, VERSION, initial_depth, shard_bits, shard_id,
                                              max(initial_depth, max_ld), int(ld.min()), max_ld, 0,
                                              nseg, int(live.sum()), out.size), np.uint8)
    out[HEADER_BYTES:HEADER_BYTES + nseg] = ld
    pairs = out[HEADER_BYTES + depth_bytes(nseg):].view(np.uint64).reshape(-1, 2)
    pairs[:, 0] = keys
    pairs[:, 1] = np.where(live, vals, np.uint64(0))
    return out.tobytes()


def dump_from_image(buf) -> dict:
    """The canonical dump an image holds, in the shape of `CCEH.dump()`:
    depth, dir_canon, local_depth, prefix, keys, values."""
    b = _bytes(buf)
    h = validate(b)
    nseg, sb = h["nseg"], h["shard_bits"]
    ld = b[HEADER_BYTES:HEADER_BYTES + nseg].astype(np.uint32)
    span = np.int64(1) << (MAX_LOCAL_DEPTH - ld.astype(np.int64))
    start = np.cumsum(span) - span
    prefix = (np.uint64(h["shard_id"]) << (ld - sb).astype(np.uint64)) | \
        (start >> (MAX_LOCAL_DEPTH - ld.astype(np.int64))).astype(np.uint64)
    # the logical directory: segment i owns 2^(depth - L_i) consecutive entries
    dir_canon = np.repeat(np.arange(nseg, dtype=np.uint32), (1 << (h["depth"] - ld.astype(np.int64))))
    pairs = b[HEADER_BYTES + depth_bytes(nseg):].view(np.uint64).reshape(-1, 2)
    return {"depth": h["depth"], "dir_canon": dir_canon, "local_depth": ld, "prefix": prefix,
            "keys": pairs[:, 0].copy(), "values": pairs[:, 1].copy()}


__all__ = ["ImageError", "parse_header", "validate", "image_from_dump", "dump_from_image", "total_bytes",
           "depth_bytes", "HEADER_BYTES", "MAGIC", "VERSION"]
