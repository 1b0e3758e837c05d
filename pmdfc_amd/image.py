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


# ---- the packed image (pmdfc_amd/csrc/packed_image.h): only the live entries
#
#     [0, 4096)   header: magic "PMDFCPAK", u32 version (1), then the fields
#                 of the version-1 header at the same offsets
#     [4096, S)   the local-depth bytes, as above
#     [S, O)      nseg x 32 u32 occupancy words in canonical order (bit s & 31
#                 of word s >> 5: slot s holds an entry), zero-padded to a
#                 multiple of 4096
#     [O, total)  live x {u64 key, u64 value} in canonical segment order, slot
#                 order within a segment, zero-padded to a multiple of 4096

PACKED_MAGIC = b"PMDFCPAK"
PACKED_VERSION = 1
OCC_WORDS = 32


def _align(n: int) -> int:
    return (n + ALIGN - 1) // ALIGN * ALIGN


def packed_occ_offset(nseg: int) -> int:
    return HEADER_BYTES + depth_bytes(nseg)


def packed_pairs_offset(nseg: int) -> int:
    return packed_occ_offset(nseg) + _align(nseg * OCC_WORDS * 4)


def packed_total_bytes(nseg: int, live: int) -> int:
    return packed_pairs_offset(nseg) + _align(live * 16)


def _as_v1_header(b: np.ndarray, nseg: int) -> np.ndarray:
    """header + depth region of a packed image as the version-1 validator reads
    them (its magic, version and byte count), for the shared depth checks"""
    v1 = np.zeros(total_bytes(nseg), np.uint8)
    n = HEADER_BYTES + depth_bytes(nseg)
    v1[:n] = b[:n]
    v1[:8] = np.frombuffer(MAGIC, np.uint8)
    v1[56:64] = np.frombuffer(struct.pack("<Q", v1.size), np.uint8)
    return v1


def validate_packed(buf) -> dict:
    """The checks of packed_image.h's validate: header (magic, version,
    geometry, byte counts against nseg and live), the local depths, the
    popcount of the occupancy words against live, every padding byte zero.
    Returns the header."""
    b = _bytes(buf)
    if b.size < HEADER_BYTES:
        raise ImageError("packed image shorter than its header")
    magic, *w = _HDR.unpack(b[:_HDR.size].tobytes())
    if magic != PACKED_MAGIC:
        raise ImageError("packed image magic mismatch")
    h = dict(zip(FIELDS, w[:7]))
    h["nseg"], h["live"], h["total_bytes"] = w[8], w[9], w[10]
    if h["version"] != PACKED_VERSION:
        raise ImageError("unknown packed image format version")
    if not (1 <= h["initial_depth"] <= MAX_LOCAL_DEPTH and h["shard_bits"] <= min(h["initial_depth"], 16)
            and h["shard_id"] < (1 << h["shard_bits"])):
        raise ImageError("packed image geometry out of range")
    nseg, live = h["nseg"], h["live"]
    if nseg == 0 or nseg > 1 << 30 or live > nseg * SLOTS or \
            h["total_bytes"] != packed_total_bytes(nseg, live) or b.size != h["total_bytes"]:
        raise ImageError("packed image byte count inconsistent with its segment and entry counts")
    if w[7] != 0 or b[_HDR.size:HEADER_BYTES].any():
        raise ImageError("packed image padding not zero")
    validate(_as_v1_header(b, nseg))  # the depths, by the version-1 rules
    o, p = packed_occ_offset(nseg), packed_pairs_offset(nseg)
    occ = b[o:o + nseg * OCC_WORDS * 4]
    if int(np.unpackbits(occ).sum()) != live:
        raise ImageError("packed image occupancy words do not count its live entries")
    if b[o + occ.size:p].any() or b[p + live * 16:].any():
        raise ImageError("packed image padding not zero")
    return h


def packed_from_dump(dump: dict, initial_depth: int, shard_bits: int = 0, shard_id: int = 0) -> bytes:
    """The packed image bytes of a canonical dump."""
    ld = np.asarray(dump["local_depth"]).astype(np.uint8)
    nseg = int(ld.size)
    keys = np.ascontiguousarray(dump["keys"], dtype=np.uint64)
    vals = np.ascontiguousarray(dump["values"], dtype=np.uint64)
    if keys.size != nseg * SLOTS or vals.size != nseg * SLOTS:
        raise ImageError("dump arrays do not match its segment count")
    live = keys != INVALID
    n = int(live.sum())
    out = np.zeros(packed_total_bytes(nseg, n), np.uint8)
    max_ld = int(ld.max())
    out[:_HDR.size] = np.frombuffer(_HDR.pack(PACKED_MAGIC, PACKED_VERSION, initial_depth, shard_bits, shard_id,
                                              max(initial_depth, max_ld), int(ld.min()), max_ld, 0,
                                              nseg, n, out.size), np.uint8)
    out[HEADER_BYTES:HEADER_BYTES + nseg] = ld
    o, p = packed_occ_offset(nseg), packed_pairs_offset(nseg)
    out[o:o + nseg * OCC_WORDS * 4] = np.packbits(live, bitorder="little")  # bit s & 31 of little-endian word s >> 5
    pairs = out[p:p + n * 16].view(np.uint64).reshape(-1, 2)
    pairs[:, 0] = keys[live]
    pairs[:, 1] = vals[live]
    return out.tobytes()


def _unpacked(b: np.ndarray, h: dict):
    """(keys, values) of every slot, the empty ones {INVALID, 0}"""
    nseg, n = h["nseg"], h["live"]
    o, p = packed_occ_offset(nseg), packed_pairs_offset(nseg)
    live = np.unpackbits(b[o:o + nseg * OCC_WORDS * 4], bitorder="little").astype(bool)
    pairs = b[p:p + n * 16].view(np.uint64).reshape(-1, 2)
    keys = np.full(nseg * SLOTS, INVALID, np.uint64)
    vals = np.zeros(nseg * SLOTS, np.uint64)
    keys[live] = pairs[:, 0]
    vals[live] = pairs[:, 1]
    return keys, vals


def unpack(packed) -> bytes:
    """The version-1 image holding the same table as a packed image."""
    b = _bytes(packed)
    h = validate_packed(b)
    nseg = h["nseg"]
    out = _as_v1_header(b, nseg)
    keys, vals = _unpacked(b, h)
    pairs = out[HEADER_BYTES + depth_bytes(nseg):].view(np.uint64).reshape(-1, 2)
    pairs[:, 0] = keys
    pairs[:, 1] = vals
    return out.tobytes()


def pack(image_v1) -> bytes:
    """The packed image holding the same table as a version-1 image."""
    b = _bytes(image_v1)
    h = validate(b)
    nseg = h["nseg"]
    pairs = b[HEADER_BYTES + depth_bytes(nseg):].view(np.uint64).reshape(-1, 2)
    return packed_from_dump({"local_depth": b[HEADER_BYTES:HEADER_BYTES + nseg], "keys": pairs[:, 0],
                             "values": pairs[:, 1]}, h["initial_depth"], h["shard_bits"], h["shard_id"])


def dump_from_packed(buf) -> dict:
    """The canonical dump a packed image holds, in the shape of `CCEH.dump()`."""
    return dump_from_image(unpack(buf))


def is_packed(buf) -> bool:
    b = _bytes(buf)
    return b.size >= 8 and b[:8].tobytes() == PACKED_MAGIC


__all__ = ["ImageError", "parse_header", "validate", "image_from_dump", "dump_from_image", "total_bytes",
           "depth_bytes", "HEADER_BYTES", "MAGIC", "VERSION", "validate_packed", "packed_from_dump", "dump_from_packed",
           "pack", "unpack", "packed_total_bytes", "packed_occ_offset", "packed_pairs_offset", "is_packed",
           "PACKED_MAGIC", "PACKED_VERSION"]
