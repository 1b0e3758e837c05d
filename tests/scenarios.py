"""Golden CCEH scenarios shared by tests/golden/gen_golden.py (which runs the
reference's own CCEH_hybrid.cpp on them) and the parity tests (which run the
oracle restatement and the HIP engine on them).

A scenario is a serial op stream (ops, keys, values) applied to
CCEH_hybrid(init_cap) in order; op 1 = Insert, op 0 = Get.  Values are never 0
(0 is NONE, the reference's miss value, server/util/pair.h:11).
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pmdfc_amd.workload import uniform_keys  # noqa: E402

OP_GET, OP_INSERT = 0, 1


def _vals(keys, salt=0x1234):
    v = keys ^ np.uint64(salt)
    v[v == 0] = np.uint64(1)
    return v


def insert_then_get(seed, n_ins, n_absent):
    ins = uniform_keys(seed, 0, n_ins)
    absent = uniform_keys(seed, n_ins, n_absent)
    keys = np.concatenate([ins, ins, absent])
    vals = np.concatenate([_vals(ins), np.zeros(n_ins + n_absent, np.uint64)])
    ops = np.concatenate([np.full(n_ins, OP_INSERT, np.uint8), np.zeros(n_ins + n_absent, np.uint8)])
    return ops, keys, vals


def mixed(seed, n_ops, p_insert=0.5):
    """Random interleaving: inserts of fresh keys; gets drawn from a pool that
    holds keys inserted earlier, keys inserted LATER in the stream and keys
    never inserted -- exercises Get-after-Insert ordering inside a batch."""
    rng = np.random.default_rng(seed)
    is_ins = rng.random(n_ops) < p_insert
    n_ins = int(is_ins.sum())
    fresh = uniform_keys(seed, 0, n_ins)
    never = uniform_keys(seed, n_ins, n_ops)
    pool = np.concatenate([fresh, never[: n_ins // 4 + 1]])
    keys = np.empty(n_ops, np.uint64)
    keys[is_ins] = fresh
    keys[~is_ins] = pool[rng.integers(0, pool.size, int((~is_ins).sum()))]
    vals = np.where(is_ins, _vals(keys), np.uint64(0)).astype(np.uint64)
    return is_ins.astype(np.uint8), keys, vals


def _find_key_with_low_byte(seed, want_low, hash64, count=1, start=0):
    out = []
    pos = start
    while len(out) < count:
        ks = uniform_keys(seed, pos, 1 << 14)
        h = hash64(ks)
        sel = ks[(h & np.uint64(0xFF)) == np.uint64(want_low)]
        out.extend(sel.tolist())
        pos += 1 << 14
    return np.array(out[:count], dtype=np.uint64)


def dup_wrap(seed, hash64, n_fill=6000):
    """duplicates of a key whose window wraps (y = 1020); the
    first copy in probe order changes after the segment splits."""
    k = _find_key_with_low_byte(seed + 7, 255, hash64)[0]
    fill = uniform_keys(seed, 0, n_fill)
    ops, keys, vals = [], [], []
    for i in range(5):
        ops.append(OP_INSERT); keys.append(k); vals.append(100 + i)
    ops.append(OP_GET); keys.append(k); vals.append(0)
    for j, f in enumerate(fill):
        ops.append(OP_INSERT); keys.append(f); vals.append(int(f ^ np.uint64(0x77)) or 1)
        if j % 500 == 0:
            ops.append(OP_GET); keys.append(k); vals.append(0)
    ops.append(OP_GET); keys.append(k); vals.append(0)
    return np.array(ops, np.uint8), np.array(keys, np.uint64), np.array(vals, np.uint64)


def dup32(seed, n_fill=3000):
    """32 copies of one key (the 33rd would hang the reference)."""
    k = uniform_keys(seed + 11, 0, 1)[0]
    fill = uniform_keys(seed, 0, n_fill)
    ops = [OP_INSERT] * 32 + [OP_GET] + [OP_INSERT] * n_fill + [OP_GET]
    keys = [k] * 32 + [k] + fill.tolist() + [k]
    vals = list(range(1, 33)) + [0] + [int(f ^ np.uint64(0x99)) or 1 for f in fill] + [0]
    return np.array(ops, np.uint8), np.array(keys, np.uint64), np.array(vals, np.uint64)


def dup_pairs(seed, n=20000):
    """Uniform stream where ~5% of inserts re-insert an earlier key (re-puts of
    the same longkey reach the server: client/julee.c:25)."""
    rng = np.random.default_rng(seed)
    base = uniform_keys(seed, 0, n)
    keys = base.copy()
    rep = rng.random(n) < 0.05
    rep[0] = False
    idx = np.arange(n)
    src = (rng.random(n) * idx).astype(np.int64)
    keys[rep] = base[src[rep]]
    ops = np.ones(n, np.uint8)
    vals = (np.arange(n, dtype=np.uint64) + np.uint64(1))
    q = np.concatenate([base, uniform_keys(seed, n, 1000)])
    return (np.concatenate([ops, np.zeros(q.size, np.uint8)]),
            np.concatenate([keys, q]),
            np.concatenate([vals, np.zeros(q.size, np.uint64)]))


def _find_keys(seed, hash64, want_low, want_top2, count):
    """`count` keys with h & 0xFF == want_low and h >> 62 == want_top2."""
    out, pos = [], 0
    while len(out) < count:
        ks = uniform_keys(seed, pos, 1 << 16)
        h = hash64(ks)
        sel = ks[((h & np.uint64(0xFF)) == np.uint64(want_low)) & ((h >> np.uint64(62)) == np.uint64(want_top2))]
        out.extend(sel.tolist())
        pos += 1 << 16
    return np.array(out[:count], dtype=np.uint64)


def _key_cells(hash64, prefix, pbits, seed=900, n=1 << 21):
    """Pick keys by home line, segment prefix and child bit: the keys of
    uniform_keys(seed, 0, n) whose top `pbits` hash bits equal `prefix` (they
    live in the segment of local depth L = pbits with that prefix), sorted
    into cells by home line h & 0xFF and by the bit that chooses the child
    when that segment splits, hash bit 63 - L.  The pool is filtered once;
    returns a factory of take(line, child, count) functions, each of which
    hands out a cell's keys in pool order, every key once."""
    ks = uniform_keys(seed, 0, n)
    h = hash64(ks)
    sel = (h >> np.uint64(64 - pbits)) == np.uint64(prefix)
    ks, h = ks[sel], h[sel]
    cell = ((h & np.uint64(0xFF)) | (((h >> np.uint64(63 - pbits)) & np.uint64(1)) << np.uint64(8))).astype(np.int64)
    order = np.argsort(cell, kind="stable")
    ks = ks[order]
    start = np.searchsorted(cell[order], np.arange(513))

    def taker():
        used = np.zeros(512, np.int64)

        def take(line, child, count=1):
            c = int(line) | (int(child) << 8)
            a = int(start[c] + used[c])
            if a + count > int(start[c + 1]):
                raise ValueError(f"key pool too small for line {line}, child {child}")
            used[c] += count
            return ks[a:a + count]
        return take
    return taker


# Crafted split images (split_shapes).  An insert of home line h takes the
# first free slot of [4h, 4h + 32) mod 1024, so a list of (home line, child
# bit, count) groups in insert order fixes the segment image exactly.  Each
# entry: the image groups, the trigger's (line, child), and what the shape
# guard of test_oracle_golden.py checks before the trigger -- the occupied
# slots and the clusters (maximal occupied runs, (first slot, length), the run
# through slot 1023 continued at slot 0).
def _per_line(lines, child, count=4):
    return [(h, child(h) if callable(child) else child, count) for h in lines]


def _cyclic_heads_image():
    """A cyclic parent on the cluster path.  Lines 255, 254, 253 (8 keys each,
    in that order) take 1020..1023 + 0..3, 1016..1019 + 4..7 and 1012..1015 +
    8..11, so the head is [0, 12) and the split replays its wrapped entries
    before the tail's, which then move past slot 1023; three more clusters
    start in slots 1..30 ([16, 19), [24, 26), [28, 36): the `a0 <= 30` loop,
    the last one reaching into word 1 with two entries of home line 8, whose
    position 32 lies below U = 36: the unit places them, the sweep skips
    them); the tail cluster starts at slot 980 with the trigger's full window
    (T = 980),
    so the wrap unit is 80 slots wide (< 128: the fast path).  Lines 100..104
    add a cluster with a backlog for the sweep proper.  Every group alternates
    its child bit key by key."""
    img = []
    for h, n in [(255, 8), (254, 8), (253, 8), (245, 32), (4, 3), (6, 2), (7, 6), (8, 2), (100, 12), (101, 4),
                 (102, 4), (103, 4), (104, 4)]:
        img += [(h, i & 1, 1) for i in range(n)]
    return img


def _wrap_drop_both_image():
    """A fast-path wrap unit that drops entries of BOTH children (split_loss
    drops from child 0 only).  Insert order and slots:
      4 keys of line 255, child 1 -> 1020..1023;
      28 keys of line 248, child 0 -> 992..1019 (its window is now full);
      8 keys of line 250, child 0 -> wrap to 0..7;
      20 keys of line 255, child 1 -> 8..27;  4 of line 0, child 1 -> 28..31;
      4 each of lines 1..5, child 1 -> 32..35, 36..39, ..., 48..51.
    The split replays the head [0, 52) first.  Child 0: line 250's 8 wrapped
    entries take 1000..1007, so line 248's 28 entries find 24 free slots in
    [992, 1024): 4 dropped.  Child 1: line 255's 20 head entries take
    1020..1023 and 0..15 and line 0's, 1's and 2's take 16..27 -- line 255's
    whole window -- so its 4 entries of the tail (parent 1020..1023) are
    dropped.  Lines 3..5 land at 28..39, positions 60..71 of the unit's
    128-bit map: line 4's window (map bits 48..79) is full below bit 64 and
    continues above it, the one place where ext32 must join the map's two
    words.  Lines 0..5 sit behind the wrapped entries in the head, so a sweep
    that did not mask the positions below U = 52 would place them at their
    home slots instead.  The unit is 84 slots wide."""
    return [(255, 1, 4), (248, 0, 28), (250, 0, 8), (255, 1, 20)] + [(h, 1, 4) for h in range(6)]


_BALLAST_LINES = range(100, 107)


def _dense_drop_image(k=7):
    """N(k), the densest drop of a non-wrapping window: a split that costs
    33 + 4k inserts and drops 4k entries.  Insert order and slots:
      32 keys of line 248, child 0 -> 992..1023 (the window is full);
      4 keys each of lines 256-k .. 255, child 0 -> their windows are full up
      to slot 1023: they wrap to 0..4k-1.
    The trigger is a key of line 248 with child bit 1 (it lands in the empty
    child: no second split).  The split replays the head [0, 4k) first; its
    entries take 4k slots of [996, 1024), so line 248's 32 entries find
    32 - 4k free slots in [992, 1024): the last 4k of them are dropped, and
    nothing else is.  The unit is 32 + 4k slots wide.
      Ballast: 4 keys each of lines 100..106, child 0 -> 400..427, a cluster
    of its own that the sweep moves as it lies.  It takes no part in the
    drops (drop_log_stream leaves it out); it makes the stream longer than
    256 ops from its first Get on, which the batch cuts of the tests rely on
    (SPLIT_SHAPE_ABSENT)."""
    return [(248, 0, 32)] + _per_line(range(256 - k, 256), 0) + _per_line(_BALLAST_LINES, 0)


def _dense_drop_wrap_image():
    """W, dropped entries of a WRAPPING window:
      32 keys of line 252, child 0 -> 1008..1023 and 0..15;
      4 keys each of lines 253, 254, 255, child 0 -> 16..19, 20..23, 24..27.
    The trigger is a key of line 252 with child bit 1.  The split replays the
    head [0, 28) first: line 252's 16 wrapped entries take 1008..1023, lines
    253..255 then take 0..11, so the tail's 16 entries of line 252 find 4 free
    slots (12..15) in their window: 12 are dropped.  44 slots wide.  Ballast
    as in _dense_drop_image."""
    return [(252, 0, 32)] + _per_line(range(253, 256), 0) + _per_line(_BALLAST_LINES, 0)


_WRAP_LINES = list(range(201, 256)) + list(range(0, 41))
_WRAP_DROP_LINES = list(range(217, 256)) + list(range(0, 30))
SPLIT_SHAPES = {
    # a completely full parent: all_full -> the generic replay
    "full_alt": dict(image=_per_line(range(256), lambda h: h & 1), trigger=(7, 1),
                     occupied=1024, clusters=[(0, 1024)]),
    "full_child0": dict(image=_per_line(range(256), 0), trigger=(7, 0), occupied=1024, clusters=[(0, 1024)]),
    "full_shifted": dict(image=[(255, 1, 8)] + _per_line(range(254), 0), trigger=(100, 0),
                         occupied=1024, clusters=[(0, 1024)]),
    # one 628-slot cluster outside any wrap unit, a backlog of 28 over ~19 words of the sweep
    "backlog_c0": dict(image=[(50, 0, 32)] + _per_line(range(51, 200), 0), trigger=(50, 0),
                       occupied=628, clusters=[(200, 628)]),
    "backlog_mixed": dict(image=[(50, 0, 32)] + _per_line(range(51, 200), lambda h: int(h % 3 == 0)),
                          trigger=(50, 0), occupied=628, clusters=[(200, 628)]),
    # a wrap unit wider than 128 slots: wide -> the generic replay
    "wide_wrap": dict(image=[(200, 0, 32)] + _per_line(_WRAP_LINES, 0), trigger=(200, 1),
                      occupied=416, clusters=[(800, 416)]),
    "wide_wrap_mix": dict(image=[(200, 1, 32)] + _per_line(_WRAP_LINES, lambda h: h & 1), trigger=(200, 1),
                          occupied=416, clusters=[(800, 416)]),
    "wide_wrap_drop": dict(image=[(216, 0, 32)] + _per_line(_WRAP_DROP_LINES, 0), trigger=(216, 0),
                           occupied=308, clusters=[(864, 308)]),
    # the cluster path through a narrow wrap unit (see the image builders)
    "cyclic_heads": dict(image=_cyclic_heads_image(), trigger=(245, 0), occupied=97,
                         clusters=[(16, 3), (24, 2), (28, 8), (400, 28), (980, 56)]),
    "wrap_drop_both": dict(image=_wrap_drop_both_image(), trigger=(248, 0), occupied=84, clusters=[(992, 84)]),
    # the densest drops, 28 and 12 per split: the images drop_log_stream replicates (see the image builders)
    "dense_drop": dict(image=_dense_drop_image(), trigger=(248, 1), occupied=88, clusters=[(400, 28), (992, 60)]),
    "dense_drop_wrap": dict(image=_dense_drop_wrap_image(), trigger=(252, 1), occupied=72,
                            clusters=[(400, 28), (1008, 44)]),
}
# name suffix -> (init_cap, hash prefix of the target segment, its local depth):
# CCEH_hybrid(2)'s segment 0 (child bit = hash bit 62), and segment 0b1011 of
# CCEH_hybrid(16) (child bit = hash bit 59; the split happens away from
# segment 0 and doubles a depth-4 directory)
SPLIT_SHAPE_TABLES = {"": (2, 0, 1), "_d4": (16, 0b1011, 4)}


SPLIT_SHAPE_ABSENT = 120  # absent keys at a stream's end (every stream is > 256 ops from its first Get on)
_SHAPE_POOLS = {}


def split_shape_parts(name, hash64):
    """Split shape `name` (a SPLIT_SHAPES name plus a SPLIT_SHAPE_TABLES
    suffix) in parts: (init_cap, prefix, L, image keys in insert order,
    trigger keys, absent keys)."""
    base, suffix = (name[:-3], "_d4") if name.endswith("_d4") else (name, "")
    init_cap, prefix, L = SPLIT_SHAPE_TABLES[suffix]
    if suffix not in _SHAPE_POOLS:  # one pool per table, filtered once
        _SHAPE_POOLS[suffix] = _key_cells(hash64, prefix, L)
    take = _SHAPE_POOLS[suffix]()
    sh = SPLIT_SHAPES[base]
    image = np.concatenate([take(h, c, n) for h, c, n in sh["image"]])
    trigger = take(*sh["trigger"])
    absent = uniform_keys(901, 0, SPLIT_SHAPE_ABSENT)
    return init_cap, prefix, L, image, trigger, absent


def split_shapes(hash64):
    """The crafted split images as streams, name -> (init_cap, convention, ops,
    keys, values): the image inserts, Gets of every image key, the trigger
    insert (its window is full: the segment splits), Gets of every image key
    again and of SPLIT_SHAPE_ABSENT absent keys.  No split happens before the trigger.
    SPLIT_SHAPES says what each image is and which branch of split_team
    (split_device.h) it pins; every shape comes for both SPLIT_SHAPE_TABLES."""
    s = {}
    for suffix in SPLIT_SHAPE_TABLES:
        for base in SPLIT_SHAPES:
            init_cap, _, _, image, trigger, absent = split_shape_parts(base + suffix, hash64)
            keys = np.concatenate([image, image, trigger, image, absent])
            ops = np.zeros(keys.size, np.uint8)
            ops[:image.size] = OP_INSERT
            ops[2 * image.size:2 * image.size + trigger.size] = OP_INSERT
            vals = np.where(ops == OP_INSERT, _vals(keys, 0x5A17), np.uint64(0)).astype(np.uint64)
            s[base + suffix] = (init_cap, "hybrid", ops, keys, vals)
    return s


def split_shape_image_size(keys):
    """n of a split_shapes stream: n inserts, n Gets, the trigger, n Gets, the absent Gets."""
    return (len(keys) - 1 - SPLIT_SHAPE_ABSENT) // 3


def split_shape_get_values(g, ops, keys, vals):
    """The reference's result of every Get of a split_shapes stream, in stream
    order, from its fixture entry g: get_hits_hex has one bit per Get (a hit
    returns the value the stream inserted with that key, no key is inserted
    twice), and the rebuilt array must hash to the reference's
    get_values_sha."""
    gets = np.asarray(ops) == OP_GET
    hit = np.unpackbits(np.frombuffer(bytes.fromhex(g["get_hits_hex"]), np.uint8))[:int(gets.sum())].astype(bool)
    ins = ~gets
    order = np.argsort(keys[ins], kind="stable")
    ik, iv = keys[ins][order], vals[ins][order]
    pos = np.minimum(np.searchsorted(ik, keys[gets]), ik.size - 1)
    assert np.all(ik[pos][hit] == keys[gets][hit])
    want = np.where(hit, iv[pos], np.uint64(0)).astype(np.uint64)
    full = np.zeros(len(ops), np.uint64)
    full[gets] = want
    assert sha(full) == g["get_values_sha"] and int(hit.sum()) == g["get_hits"]
    return want


def occupancy_clusters(occ):
    """Maximal runs of occupied slots of one segment (occ: 1024 booleans) as
    sorted (first slot, length); the run through slot 1023 continues at 0."""
    occ = np.asarray(occ, bool)
    if occ.all():
        return [(0, occ.size)]
    starts = np.nonzero(occ & ~np.roll(occ, 1))[0]
    out = []
    for a in starts.tolist():
        n = 0
        while occ[(a + n) % occ.size]:
            n += 1
        out.append((a, n))
    return out


def split_loss(seed, hash64, mixed=False, n_fill=3000):
    """Insert4split's silent drop (CCEH_hybrid.cpp:18-28), through
    the wrap unit (split_shapes below builds the other crafted split images).
    CCEH_hybrid(2): segment 0 holds hash prefix 0; every key
    here has h >> 62 == 0 (segment 0, and child 0 of its first split).
      A: 32 keys of home line 248 fill the window [992, 1024);
      B: 28 keys of home line 255 (window [1020, 1052) mod 1024) find
         1020..1023 taken and wrap to slots 0..27;
      C: keys of home line 248 find their window full -> split.
    The split replays the parent in slot order: B's wrapped entries (slots
    0..27) go first and take 1020..1023 and 0..23 of the child, so A's window
    [992, 1024) keeps 28 free slots for 32 entries -- 4 are dropped.  Then
    fill keys (more splits elsewhere) and Gets of everything.  mixed=True
    interleaves Gets of A and B before, between and after the splits (a
    mixed batch may answer a Get early against the pre-batch image; the
    engine places the drop before or after it through its drop log,
    DESIGN §2)."""
    a = _find_keys(seed, hash64, 248, 0, 36)
    b = _find_keys(seed + 1, hash64, 255, 0, 28)
    c, a = a[32:], a[:32]
    fill = uniform_keys(seed + 2, 0, n_fill)
    absent = uniform_keys(seed + 3, 0, 100)
    ops, keys = [], []

    def ins(ks):
        ops.extend([OP_INSERT] * len(ks))
        keys.extend(ks.tolist())

    def get(ks):
        ops.extend([OP_GET] * len(ks))
        keys.extend(ks.tolist())

    ins(a)
    ins(b)
    if mixed:
        get(a)
        get(b)
        for k in c:  # each trigger followed by Gets of A (some are dropped by now)
            ins(np.array([k], np.uint64))
            get(a[::3])
        ins(fill[: n_fill // 2])
        get(np.concatenate([a, b]))
        ins(fill[n_fill // 2:])
    else:
        ins(c)
        ins(fill)
    get(np.concatenate([a, b, c, fill, absent]))
    ops = np.array(ops, np.uint8)
    keys = np.array(keys, np.uint64)
    vals = np.where(ops == OP_INSERT, _vals(keys), np.uint64(0)).astype(np.uint64)
    return ops, keys, vals


def scenarios(hash64):
    """name -> (init_cap, convention, ops, keys, values)."""
    s = {}
    s["cap2_ins3k"] = (2, "hybrid") + insert_then_get(1, 3000, 1000)
    s["cap8_ins20k"] = (8, "hybrid") + insert_then_get(2, 20000, 5000)
    s["cap1024_ins100k"] = (1024, "hybrid") + insert_then_get(3, 100000, 20000)
    s["cap2_ins100k"] = (2, "hybrid") + insert_then_get(4, 100000, 10000)
    s["cap256_ins400k"] = (256, "hybrid") + insert_then_get(5, 400000, 50000)
    s["mixed_cap16_60k"] = (16, "hybrid") + mixed(6, 60000)
    s["mixed_cap2_30k_ins80"] = (2, "hybrid") + mixed(7, 30000, 0.8)
    s["dup_wrap"] = (2, "hybrid") + dup_wrap(8, hash64)
    s["dup32"] = (4, "hybrid") + dup32(9)
    s["dup_pairs"] = (32, "hybrid") + dup_pairs(10)
    # src/cceh.cpp twin: CCEH(initCap) -> depth floor(log2(initCap/1024))
    s["src_cap2m_ins50k"] = (2 << 20, "src") + insert_then_get(12, 50000, 5000)
    # Insert4split's drop (CCEH_hybrid.cpp:18-28) through the wrap unit
    s["split_loss"] = (2, "hybrid") + split_loss(13, hash64)
    s["split_loss_mixed"] = (2, "hybrid") + split_loss(13, hash64, mixed=True)
    return s


# Probe shapes of a pure Get (get_probe_shapes): where in its 8-line window a
# Get stops.  GET_SHAPE_DEPTH is the table's initial depth (8 segments, the
# segment of a key is h >> 61); nothing splits.
GET_SHAPE_DEPTH = 3
GET_SHAPE_STAIR_OFF = (0, 1, 5)  # segments 0..2: home line 8 i + off holds i + 1 keys, i = 0..31
GET_SHAPE_RANDOM = 420           # segment 3: random keys, overlapping windows
# segments 4..7: one partly filled wrapping window each, (home line, keys): a
# miss stops on line keys // 4 + 1 of the window: past line 255 for the first
# three, on line 255 for the last
GET_SHAPE_WRAP_PARTIAL = ((254, 10), (255, 18), (253, 26), (250, 22))
GET_SHAPE_WRAP_LINE = 249        # home lines from here on: the window wraps past line 255


def get_probe_shapes(hash64):
    """A table and a query set that stop Gets on every line of the window, as
    (initial_depth, insert_keys, values, query_keys), inserts and queries
    shuffled.  CCEH_hybrid at depth 3, no split: an insert takes the first free
    slot of its window, so the keys of one home line fill its lines in order.
      segments 0, 1, 2  staircases: home line 8 i + off (off = 0, 1, 5) holds
                        i + 1 keys, i = 0..31.  The windows of one staircase
                        never overlap: key j of a home line is a hit on line
                        j // 4 + 1, an absent key of that line misses on line
                        (i + 1) // 4 + 1, or after all 8 lines when i = 31.
                        off = 0: even home lines (the second line is loaded
                        with the first); off = 1, 5: odd ones, and the wrapping
                        home lines 249 and 253;
      segment 3         420 random keys: windows that overlap;
      segments 4..7     GET_SHAPE_WRAP_PARTIAL: wrapping windows filled up to
                        line 255 or a line past it, so a miss stops there.
    Queries: every inserted key, 3 absent keys per crafted home line (and of
    the empty wrapping home line 251 of segment 4), 1000 absent keys of
    segment 3, the two reserved keys, 40 keys a second time."""
    rng = np.random.default_rng(20261020)
    pool = np.unique(rng.integers(1, 1 << 62, 600000, dtype=np.uint64))
    h = hash64(pool)
    seg = (h >> np.uint64(64 - GET_SHAPE_DEPTH)).astype(np.int64)
    cell = seg * 256 + (h & np.uint64(0xFF)).astype(np.int64)
    order = np.argsort(cell, kind="stable")
    pool = pool[order]
    start = np.searchsorted(cell[order], np.arange(256 * (1 << GET_SHAPE_DEPTH) + 1))

    def take(s, line, n, skip=0):
        a = int(start[s * 256 + line]) + skip
        if a + n > int(start[s * 256 + line + 1]):
            raise ValueError(f"key pool too small for segment {s}, line {line}")
        return pool[a:a + n]

    ins, absent = [], []
    for s, off in enumerate(GET_SHAPE_STAIR_OFF):
        for i in range(32):
            ins.append(take(s, 8 * i + off, i + 1))
            absent.append(take(s, 8 * i + off, 3, skip=i + 1))
    s3 = pool[int(start[3 * 256]):int(start[4 * 256])]
    s3 = s3[rng.permutation(s3.size)]
    ins.append(s3[:GET_SHAPE_RANDOM])
    absent.append(s3[GET_SHAPE_RANDOM:GET_SHAPE_RANDOM + 1000])
    for j, (line, n) in enumerate(GET_SHAPE_WRAP_PARTIAL):
        ins.append(take(4 + j, line, n))
        absent.append(take(4 + j, line, 3, skip=n))
    absent.append(take(4, 251, 3))
    ins = np.concatenate(ins)
    ins = ins[rng.permutation(ins.size)]
    absent = np.concatenate(absent)
    q = np.concatenate([ins, absent, np.array([2**64 - 1, 2**64 - 2], np.uint64), ins[:30], absent[:10]])
    q = q[rng.permutation(q.size)]
    return GET_SHAPE_DEPTH, ins, _vals(ins, 0x6E7), q


# CCEH::FindAnyway fixtures (tests/golden/findany.json): scenarios whose
# final table the reference scans for these queries
FINDANY_CASES = ["dup_wrap", "dup32", "split_loss", "cap2_ins3k", "mixed_cap2_30k_ins80", "src_cap2m_ins50k"]


def findany_queries(keys):
    """The stream's distinct keys in first-occurrence order (at most 4000) and
    64 keys it never holds."""
    _, first = np.unique(keys, return_index=True)
    q = keys[np.sort(first)][:4000]
    return np.concatenate([q, uniform_keys(4242, 0, 64)]).astype(np.uint64)


def upsert_reinserts(seed, n=30000, p_re=0.15, p_get=0.3):
    """A mixed stream where ~15% of the inserts re-insert an earlier key with a
    new value (the client re-puts a longkey, client/julee.c:25) and Gets ask
    for inserted, re-inserted and absent keys: last-writer-wins must return
    the latest value."""
    rng = np.random.default_rng(seed)
    fresh = uniform_keys(seed, 0, n)
    absent = uniform_keys(seed, n, n // 10)
    ops = np.empty(n, np.uint8)
    keys = np.empty(n, np.uint64)
    nf = 0
    for i in range(n):
        r = rng.random()
        if r < p_get and nf:
            ops[i] = OP_GET
            keys[i] = fresh[rng.integers(0, nf)] if rng.random() < 0.9 else absent[rng.integers(0, absent.size)]
        elif r < p_get + p_re and nf:
            ops[i] = OP_INSERT
            keys[i] = fresh[rng.integers(0, nf)]
        else:
            ops[i] = OP_INSERT
            keys[i] = fresh[nf]
            nf += 1
    vals = np.where(ops == OP_INSERT, np.arange(1, n + 1, dtype=np.uint64), np.uint64(0)).astype(np.uint64)
    return ops, keys, vals


def dup_many(seed, copies=100, n_fill=3000):
    """100 copies of one key interleaved with fill inserts and Gets: in upsert
    mode a key never holds more than one slot (the reference as shipped hangs
    at the 33rd copy)."""
    k = uniform_keys(seed + 11, 0, 1)[0]
    fill = uniform_keys(seed, 0, n_fill)
    ops, keys, vals = [], [], []
    per = n_fill // copies
    for c in range(copies):
        ops += [OP_INSERT, OP_GET]
        keys += [int(k), int(k)]
        vals += [c + 1, 0]
        for f in fill[c * per:(c + 1) * per]:
            ops.append(OP_INSERT); keys.append(int(f)); vals.append(int(f ^ np.uint64(0x99)) or 1)
    ops.append(OP_GET); keys.append(int(k)); vals.append(0)
    return np.array(ops, np.uint8), np.array(keys, np.uint64), np.array(vals, np.uint64)


def upsert_scenarios(hash64):
    """Last-writer-wins scenarios, pinned by the reference's CCEH_hybrid.cpp
    with its overwrite clause (:153) enabled (oracle/_ref/ref_driver_upsert).
    name -> (init_cap, convention, ops, keys, values)."""
    s = {}
    s["up_dup_wrap"] = (2, "hybrid") + dup_wrap(8, hash64)
    s["up_dup_many"] = (4, "hybrid") + dup_many(9)
    s["up_dup_pairs"] = (32, "hybrid") + dup_pairs(10)
    s["up_reinserts_cap2"] = (2, "hybrid") + upsert_reinserts(14)
    s["up_reinserts_cap256"] = (256, "hybrid") + upsert_reinserts(15, n=120000, p_re=0.25)
    s["up_split_loss_mixed"] = (2, "hybrid") + split_loss(13, hash64, mixed=True)
    return s


def sha(a) -> str:
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def summarize(depth, local_depth, prefix, keys, values, get_values, ops):
    """Fixture record for a final table state + the Get results of a stream.
    keys/values are the canonical segment images (values 0 where key INVALID),
    get_values[i] is the Get result for op i (0 for inserts and misses)."""
    gv = np.where(np.asarray(ops) == OP_GET, get_values, 0).astype(np.uint64)
    return {
        "depth": int(depth),
        "nseg": int(len(local_depth)),
        "local_depth_sha": sha(np.asarray(local_depth, np.uint64)),
        "prefix_sha": sha(np.asarray(prefix, np.uint64)),
        "keys_sha": sha(np.asarray(keys, np.uint64)),
        "values_sha": sha(np.asarray(values, np.uint64)),
        "get_values_sha": sha(gv),
        "get_hits": int(np.count_nonzero(gv)),
        "occupied": int(np.count_nonzero(np.asarray(keys, np.uint64) != np.uint64(0xFFFFFFFFFFFFFFFF))),
    }


def cbfseq_cases():
    """Counting-BF insert-then-delete sequences (counting_bloom_filter.h:109-131):
    saturation at 255, deletes that conflict inside one batch, a key whose k
    hashes repeat an index (uint8 wrap on Delete), absent keys."""
    rng = np.random.default_rng(77)
    a = np.array([0x1234567], np.uint64)
    pool = uniform_keys(40, 0, 1500)
    dels = np.concatenate([a, a, pool[rng.integers(0, 1500, 400)], uniform_keys(41, 0, 100)])
    rng.shuffle(dels)
    t = (np.arange(10000, dtype=np.uint64) * np.uint64(14))
    big = uniform_keys(42, 0, 50000)
    return {
        "sat_conflict": (3, 1000, np.concatenate([np.repeat(a, 300), pool]), dels),
        "tiny_wrap": (4, 7, uniform_keys(43, 0, 3), uniform_keys(43, 0, 40)[rng.integers(0, 40, 30)]),
        "fastpath": (4, 1000000, big, np.concatenate([big[rng.permutation(50000)[:10000]],
                                                       uniform_keys(44, 0, 2000)])),
        "bftest_seq": (2, 100000, t[:9999], np.concatenate([t[:5000], t[9999:]])),
    }


def replay_trace(seed: int, n_lines: int, n_inodes: int = 2000, crlf: bool = False) -> bytes:
    """Synthetic trace in replay_KV's format (server/replay_KV.cpp:24-31):
    'seq ts OP inode inode_size offset size' with O/C/F/R/W ops, sizes that
    are 0, sub-page, page-multiple and ragged, some unaligned offsets, mixed
    spaces/tabs.  Reads mostly revisit written ranges.  No page is written
    more than 8 times (the reference hangs on a key's 33rd copy)."""
    rng = np.random.default_rng(seed)
    wcount = {}
    written = []
    out = []
    for i in range(n_lines):
        op = rng.choice([b"W", b"W", b"R", b"R", b"R", b"O", b"C", b"F"])
        if op == b"R" and written and rng.random() < 0.8:
            ino, off = written[int(rng.integers(0, len(written)))]
        else:
            ino = int(rng.integers(1, n_inodes + 1))
            off = 4096 * int(rng.integers(0, 256)) + (int(rng.integers(1, 4096)) if rng.random() < 0.05 else 0)
        size = int(rng.choice([0, 100, 4096, 5000, 8192, 12288, 20000, 65536]))
        if op == b"W":
            np_ = size // 4096 + (1 if size % 4096 else 0)
            pages = [((ino << 32) + off + 4096 * b) for b in range(np_)]
            if any(wcount.get(p, 0) >= 8 for p in pages):
                op = b"R"
            else:
                for p in pages:
                    wcount[p] = wcount.get(p, 0) + 1
                written.append((ino, off))
        sep = b"\t" if rng.random() < 0.1 else b" "
        fields = [str(i).encode(), b"%d.%06d" % (i // 1000, i % 1000), op, str(ino).encode(),
                  str(int(rng.integers(1, 1 << 30))).encode(), str(off).encode(), str(size).encode()]
        out.append(sep.join(fields) + (b"  " if rng.random() < 0.05 else b""))
    end = b"\r\n" if crlf else b"\n"
    return end.join(out) + end


def replay_trace_ops(text: bytes) -> int:
    """Ops in the whole trace (W/R pages), for num_data = everything."""
    tot = 0
    for ln in text.split(b"\n"):
        e = ln.split()
        if len(e) >= 7 and e[2][:1] in (b"W", b"R"):
            s = int(e[6])
            tot += s // 4096 + (1 if s % 4096 else 0)
    return tot


def extent_cases():
    """Extent streams for Insert_extent / Get_extent (both reference variants):
    non-overlapping extents (no duplicate heads), lens 1..300 plus a few long
    ones, heads with zero low 32 bits (inode << 32 shape, ffs((int)head) = 0)
    and head 0; queries inside and outside the extents.
    name -> (convention, init_cap, keys, clusters, lens, values, qkeys, qclusters)."""
    out = {}
    for name, conv, cap, n, seed in [("hyb_cap1024", "hybrid", 1024, 3000, 1),
                                     ("hyb_cap2", "hybrid", 2, 1500, 2),
                                     ("src_cap2m", "src", 1 << 21, 3000, 3),
                                     ("src_cap4096", "src", 4096, 1500, 4)]:
        rng = np.random.default_rng(seed)
        lens = rng.integers(1, 300, n).astype(np.uint64)
        lens[rng.integers(0, n, 5)] = rng.integers(1000, 5000, 5).astype(np.uint64)
        gaps = rng.integers(0, 64, n).astype(np.uint64)
        keys = np.cumsum(lens + gaps).astype(np.uint64) - lens
        keys[: n // 10] = (np.arange(1, n // 10 + 1, dtype=np.uint64) << np.uint64(32))  # low 32 bits zero
        keys[n // 10] = 0
        keys[n // 10 + 1:] += np.uint64(1 << 33)
        clusters = np.zeros(n, np.uint64)
        if conv == "src":
            clusters = (rng.integers(0, 3, n) * rng.integers(0, 8, n)).astype(np.uint64)
            clusters = np.minimum(clusters, lens - np.uint64(1))
            lens = lens - clusters  # src extents: the remaining pages from cluster
        vals = uniform_keys(seed + 100, 0, n) | np.uint64(1)
        qi = rng.integers(0, n, 4000)
        qoff = (rng.random(4000) * lens[qi].astype(np.float64)).astype(np.uint64)
        if conv == "src":
            qk, qc = keys[qi], clusters[qi] + qoff
        else:
            qk, qc = keys[qi] + qoff, np.zeros(4000, np.uint64)
        qk = np.concatenate([qk, uniform_keys(seed + 200, 0, 500)])
        qc = np.concatenate([qc, np.zeros(500, np.uint64)])
        out[name] = (conv, cap, keys, clusters, lens, vals, qk, qc)
    return out


def extent_expand(conv, keys, clusters, lens, vals, heads_fn):
    """Concatenated sub-extent heads/values of a batch of Insert_extent calls."""
    hk, hv = [], []
    for k, c, ln, v in zip(keys.tolist(), clusters.tolist(), lens.tolist(), vals.tolist()):
        h = heads_fn(k, ln, c, conv)
        hk.extend(h)
        hv.extend([v] * len(h))
    return np.array(hk, np.uint64), np.array(hv, np.uint64)


# hash64 (oracle.hash64, csrc/cceh_device.h) is a bijection on 64-bit values:
# multiplications by the odd constant 0xc6a4a7935bd1e995, x ^= x >> 47 steps
# (their own inverse: 2 * 47 > 64) and an xor with a constant.  Its inverse
# makes a key of any chosen hash, so a test can place keys by segment prefix,
# by child bit at every depth and by home line without a search.
_HASH_MUL = np.uint64(0xc6a4a7935bd1e995)
_HASH_MUL_INV = np.uint64(0x5f7a0ea7e59b19bd)  # _HASH_MUL * _HASH_MUL_INV == 1 mod 2^64
_HASH_SEED = np.uint64(0xc70697 ^ ((8 * 0xc6a4a7935bd1e995) & (2**64 - 1)))


def unhash64(h) -> np.ndarray:
    """The keys whose hash64 is h (a uint64 array): hash64 run backwards."""
    s47 = np.uint64(47)
    with np.errstate(over="ignore"):
        x = np.ascontiguousarray(h, dtype=np.uint64).copy()
        x ^= x >> s47
        x *= _HASH_MUL_INV
        x ^= x >> s47
        x *= _HASH_MUL_INV
        x ^= _HASH_SEED
        x *= _HASH_MUL_INV
        x ^= x >> s47
        x *= _HASH_MUL_INV
    return x


def keys_from_hash_fields(prefix, pbits, line, count, first=0, below=None):
    """`count` distinct keys by hash field: the top `pbits` hash bits are
    `prefix`, the home line h & 0xFF is `line`, and the bits in between number
    the keys first, first + 1, ... (distinct hashes, so distinct keys).
    below = (bit position b, width): the numbers go into the `width` bits
    that end at hash bit b (b = 63 is the top bit), so keys that share their
    top bits down to b + 1 differ right below them; default: the low end of
    the middle field, bits 8 and up."""
    n = np.arange(first, first + count, dtype=np.uint64)
    if below is None:
        shift, width = 8, 56 - pbits
    else:
        b, width = below
        shift = b - width + 1
        assert shift >= 8 and b < 64 - pbits
    assert first + count <= 1 << width
    h = (np.uint64(prefix) << np.uint64(64 - pbits)) if pbits else np.uint64(0)
    h = h | (n << np.uint64(shift)) | np.uint64(line)
    return unhash64(h)


def _field_keys(prefix, pbits, line, number):
    """keys_from_hash_fields for arrays that broadcast: the key whose hash has
    `prefix` in its top `pbits` bits, `number` from bit 8 up and home line `line`."""
    u = np.uint64
    h = (np.asarray(prefix, u) << u(64 - pbits)) | (np.asarray(number, u) << u(8)) | np.asarray(line, u)
    return unhash64(h)


# A mixed batch whose splits drop a chosen number of entries, up to and past
# the engine's drop log (2^18 entries: DESIGN §2, PMDFC_ST_SPLIT_LOST).  The
# segments are copies of the split shapes dense_drop (N(7), 28 drops in 61
# inserts, the victims in a non-wrapping window), dense_drop_wrap (W, 12 drops,
# the victims in a wrapping window) and one N(k) that lands on the target.
DROP_LOG_CAP = 1 << 18
DL_INSERT, DL_VICTIM, DL_HEAD, DL_BY_LOW, DL_BY_WRAP, DL_TRIGGER, DL_ABSENT = range(7)
DL_CLASS_NAMES = ["insert", "victim", "head", "bystander_low", "bystander_wrap", "trigger", "absent"]
_DL_BY_LINES = (100, 251)  # a bystander segment's stored keys: a window that does not wrap, one that does


def drop_log_stream(target_drops, depth=14, seed=1, gets_per_segment=4, spare=0):
    """A table image and one mixed batch on it whose splits drop exactly
    `target_drops` entries (a multiple of 4), on a depth-`depth` table.

    A random subset of the 2^depth initial segments splits, each once:
    min(1000, target // 40) W segments (12 drops each), then N(7) segments (28
    each) and, where a rest r remains, one N(r / 4).  Every key of a splitting
    segment has child bit 0 but its trigger, a key of the victims' line with
    child bit 1 (the empty child takes it: no second split).  `spare` further
    N(7) segments are stored and kept back for a later batch; every other
    segment is a bystander that holds 4 keys each of lines 100 and 251, of both
    children, and never splits.  No key is inserted twice, so the entries a
    batch dropped are the stored inserts that the final table does not hold.

    Returns a dict:
      depth, target
      image         (ops, keys, values): inserts only; no split, no loss
      batch         (ops, keys, values): a round of Gets, every trigger as an
                    Insert, the same Gets again in another order.  The Gets:
                    `gets_per_segment` victims of every splitting segment
                    (line 248 / 252, drawn at random: dropped ones and
                    survivors), all its head keys (lines 249..255), every
                    bystander key, the trigger keys (a miss before, a hit
                    after) and 3 (bystanders: 2) absent keys per segment
      batch_class   per op of the batch, DL_*
      after         (ops, keys, values): the same for the spare segments alone,
                    with every victim and the keys of 32 bystander segments
      classes       name -> keys: victims (all of them), heads, bystander_low,
                    bystander_wrap, triggers, absent, spare_victims, spare_triggers"""
    assert target_drops > 0 and target_drops % 4 == 0
    u = np.uint64
    rng = np.random.default_rng(seed)
    n_w = min(1000, target_drops // 40)
    n_7, r = divmod(target_drops - 12 * n_w, 28)
    nseg = 1 << depth
    n_split = n_w + n_7 + (1 if r else 0)
    assert n_split + spare + 32 <= nseg, "target too large for the table"
    order = rng.permutation(nseg).astype(u)
    pb = depth + 1
    base = u(int(rng.integers(0, 1 << 20)) << 6)  # the keys of a (segment, child, line) cell: base + 0, 1, ...
    val_salt = 0xD109

    def splitting(prefixes, vline, hlines):
        """Per segment (a row each): victims, heads, trigger, absent keys."""
        p0 = (prefixes << u(1))[:, None]
        vict = _field_keys(p0, pb, vline, base + np.arange(32, dtype=u)[None, :])
        hl = np.repeat(np.asarray(list(hlines), u), 4)[None, :]
        heads = _field_keys(p0, pb, hl, base + np.tile(np.arange(4, dtype=u), hl.size // 4)[None, :])
        trig = _field_keys(p0 | u(1), pb, vline, base)[:, 0]
        absent = np.concatenate([_field_keys(p0, pb, vline, base + u(40)), _field_keys(p0 | u(1), pb, vline, base + u(40)),
                                 _field_keys(p0, pb, 100, base + u(40))], axis=1)
        return vict, heads, trig, absent

    groups, a = [], 0
    for n, vline, hlines in ((n_w, 252, range(253, 256)), (n_7, 248, range(249, 256)),
                             (1 if r else 0, 248, range(256 - r // 4, 256)), (spare, 248, range(249, 256))):
        groups.append(splitting(order[a:a + n], vline, hlines))
        a += n
    by = order[a:]
    child = np.array([0, 1, 0, 1], u)[None, :]
    num = base + np.arange(4, dtype=u)[None, :]
    by_low = _field_keys((by << u(1))[:, None] | child, pb, _DL_BY_LINES[0], num)
    by_wrap = _field_keys((by << u(1))[:, None] | child, pb, _DL_BY_LINES[1], num)
    by_absent = np.concatenate([_field_keys((by << u(1))[:, None], pb, ln, base + u(40)) for ln in _DL_BY_LINES], axis=1)

    def stream(parts):
        """[(op, class, keys)] -> (ops, keys, values), per-op classes."""
        keys = np.concatenate([k.ravel() for _, _, k in parts])
        ops = np.concatenate([np.full(k.size, o, np.uint8) for o, _, k in parts])
        cls = np.concatenate([np.full(k.size, c, np.uint8) for _, c, k in parts])
        vals = np.where(ops == OP_INSERT, _vals(keys, val_salt), u(0)).astype(u)
        return (ops, keys, vals), cls

    # the image: each segment's victims, then its heads in line order
    image, _ = stream([(OP_INSERT, DL_INSERT, np.concatenate([g[0], g[1]], axis=1)) for g in groups]
                      + [(OP_INSERT, DL_INSERT, np.concatenate([by_low, by_wrap], axis=1))])

    def rounds(gs, sample, bys):
        """Gets, the triggers, the Gets again."""
        gets = []
        for vict, heads, trig, absent in gs:
            pick = np.argsort(rng.random(vict.shape), axis=1)[:, :sample]
            gets += [(DL_VICTIM, np.take_along_axis(vict, pick, axis=1)), (DL_HEAD, heads), (DL_TRIGGER, trig),
                     (DL_ABSENT, absent)]
        gets += [(DL_BY_LOW, bys[0]), (DL_BY_WRAP, bys[1]), (DL_ABSENT, bys[2])]
        gk = np.concatenate([k.ravel() for _, k in gets])
        gc = np.concatenate([np.full(k.size, c, np.uint8) for c, k in gets])
        p1, p2 = rng.permutation(gk.size), rng.permutation(gk.size)
        (ops, keys, vals), cls = stream([(OP_GET, 0, gk[p1]), (OP_INSERT, DL_INSERT, np.concatenate([g[2] for g in gs])),
                                         (OP_GET, 0, gk[p2])])
        cls[:gk.size] = gc[p1]
        cls[cls.size - gk.size:] = gc[p2]
        return (ops, keys, vals), cls

    batch, batch_class = rounds(groups[:3], gets_per_segment, (by_low, by_wrap, by_absent))
    after, _ = rounds(groups[3:], 32, (by_low[:32], by_wrap[:32], by_absent[:32]))
    cat = lambda i: np.concatenate([g[i].ravel() for g in groups[:3]])  # noqa: E731
    classes = dict(victims=cat(0), heads=cat(1), triggers=cat(2),
                   absent=np.concatenate([cat(3), by_absent.ravel()]), bystander_low=by_low.ravel(),
                   bystander_wrap=by_wrap.ravel(), spare_victims=groups[3][0].ravel(), spare_triggers=groups[3][2])
    return dict(depth=depth, target=target_drops, image=image, batch=batch, batch_class=batch_class, after=after,
                classes=classes)


# Streams that run a table out of room (tests/test_gpu_limits.py; the model of
# the exhausted table is tests/limits_ref.py).  Every stream is chosen so that
# no split of the serial table drops an entry (split_loss == 0 on an oracle
# with no segment limit: tests/test_limits_ref.py asserts it for each case),
# which lets a test account for every stored pair.
def limit_stream(seed, max_segments, load=3.0):
    """Uniform keys, `load` times the slots of max_segments segments."""
    keys = uniform_keys(seed, 0, int(load * max_segments * 1024))
    return keys, _vals(keys, 0x11A7)


def limit_upsert_stream(seed, max_segments, load=3.0, p_re=0.2):
    """limit_stream where ~20% of the inserts repeat an earlier key with a new
    value (under upsert: UPDATED where the key is stored, whatever the table's
    state; a repeat of a key that failed fails or succeeds on its own)."""
    keys, _ = limit_stream(seed, max_segments, load)
    n = keys.size
    rng = np.random.default_rng(seed)
    rep = rng.random(n) < p_re
    rep[0] = False
    src = (rng.random(n) * np.arange(n)).astype(np.int64)
    keys = keys.copy()
    base = keys.copy()
    keys[rep] = base[src[rep]]
    return keys, np.arange(1, n + 1, dtype=np.uint64)


def limit_mixed_batches(seed, keys, vals, n_ins, n_get):
    """The insert stream cut into mixed batches of n_ins inserts and n_get
    Gets, shuffled together: Gets of keys of earlier batches (stored, or
    failed and so absent), of keys this batch inserts (before or after their
    insert, which succeeds or fails) and of keys no batch inserts."""
    rng = np.random.default_rng(seed)
    never = uniform_keys(seed + 1000, 0, 4096)
    out = []
    for a in range(0, keys.size, n_ins):
        ik, iv = keys[a:a + n_ins], vals[a:a + n_ins]
        g = [rng.choice(ik, n_get // 3), rng.choice(never, n_get // 6)]
        g.append(rng.choice(keys[:a] if a else never, n_get - g[0].size - g[1].size))
        g = np.concatenate(g)
        k = np.concatenate([ik, g])
        v = np.concatenate([iv, np.zeros(g.size, np.uint64)])
        o = np.concatenate([np.full(ik.size, OP_INSERT, np.uint8), np.full(g.size, OP_GET, np.uint8)])
        p = rng.permutation(k.size)
        out.append((o[p], k[p], v[p]))
    return out


DEEP_CHAIN_DEPTH = 9     # the deep-chain tables start with 2^9 segments
DEEP_CHAIN_LINES = (7, 255, 130, 252, 64)  # home lines of the groups (255, 252: the window wraps)


def deep_chain_stream(D, seed, groups=3, n_uniform=12000, depth=DEEP_CHAIN_DEPTH):
    """A few segments with a long common hash prefix.  Group g is 33 keys of
    one home line whose hashes share their top D - 1 bits and differ right
    below them (the 6 bits from hash bit 64 - D down number the keys, so bit
    64 - D is 0 for the first 32 keys and 1 for the last).  32 of them fill
    the window; the 33rd splits its segment, and every split down to local
    depth D - 1 leaves all 32 in one child with the window still full: a chain
    of D - depth splits (depth: the table's initial depth) that ends at local
    depth D, with as many new segments, and a directory of depth D.  The
    groups lie in different initial segments.  Returns (keys, values, the groups' keys): a shuffle of
    n_uniform uniform keys and the groups, each group in its own order."""
    rng = np.random.default_rng(seed)
    tops = rng.choice(1 << depth, groups, replace=False)
    gk = []
    for g in range(groups):
        rest = int(rng.integers(0, 1 << (D - 1 - depth)))
        prefix = (int(tops[g]) << (D - 1 - depth)) | rest
        gk.append(keys_from_hash_fields(prefix, D - 1, DEEP_CHAIN_LINES[g % len(DEEP_CHAIN_LINES)], 33,
                                        below=(64 - D, 6)))
    uni = uniform_keys(seed, 0, n_uniform)
    # positions: the uniform keys keep their order, each group keeps its own
    tag = np.concatenate([np.full(uni.size, -1)] + [np.full(33, g) for g in range(groups)])
    tag = tag[rng.permutation(tag.size)]
    keys = np.empty(tag.size, np.uint64)
    keys[tag == -1] = uni
    for g in range(groups):
        keys[tag == g] = gk[g]
    return keys, _vals(keys, 0xD33B), gk


# The exhaustion cases of tests/test_gpu_limits.py: name -> the table (initial
# depth, max_segments = 2^depth + extra), the stream's seed, the batch size,
# the engine's max_batch (it sets the full bucket resolution p1max =
# floor(log2(max_batch)) - 7, which decides the path a batch takes) and what
# else the case sets.  Seeds: every (seed, depth, extra) below gives
# split_loss == 0 on an oracle with no segment limit (asserted by
# test_limits_ref.py::test_limit_streams_drop_nothing); a seed that did not
# was replaced by the next integer (none had to be).
LIMIT_CASES = {
    # one launch (k_mixed_small): batches up to 256 ops
    "small23": dict(depth=2, extra=1, seed=11, batch=23, max_batch=4096),
    "small64": dict(depth=2, extra=2, seed=12, batch=64, max_batch=4096),
    "small256": dict(depth=2, extra=7, seed=13, batch=256, max_batch=4096),
    # two launches (k_part + k_medium) at full bucket resolution: p1max = 2 and 6
    "medium1000": dict(depth=2, extra=7, seed=13, batch=1000, max_batch=1000),
    "medium8192": dict(depth=6, extra=1, seed=14, batch=8192, max_batch=8192),
    # the general path, lean first pass: all 64 buckets request splits in the
    # round that exhausts the arena; and on a table below its bucket resolution
    "general65536": dict(depth=6, extra=7, seed=15, batch=65536, max_batch=65536),
    "general2000_ramp": dict(depth=2, extra=2, seed=12, batch=2000, max_batch=16384),
    "fast_apply0": dict(depth=6, extra=2, seed=16, batch=65536, max_batch=65536, env={"PMDFC_FAST_APPLY": "0"}),
    "cp0": dict(depth=6, extra=7, seed=15, batch=16384, max_batch=16384, env={"PMDFC_CP": "0"}),
    "team0": dict(depth=6, extra=1, seed=14, batch=65536, max_batch=65536, env={"PMDFC_SPLIT_TEAM_MAX": "0"}),
    # mixed batches (batch inserts + gets Gets), small, medium and general with each forced mode
    "mixed_small": dict(depth=2, extra=1, seed=11, batch=150, gets=100, max_batch=4096),
    "mixed_medium": dict(depth=2, extra=7, seed=13, batch=600, gets=400, max_batch=1000),
    "mixed_join0": dict(depth=6, extra=7, seed=15, batch=12000, gets=8000, max_batch=65536,
                        env={"PMDFC_MIXED_JOIN": "0"}),
    "mixed_join1": dict(depth=6, extra=7, seed=15, batch=12000, gets=8000, max_batch=65536,
                        env={"PMDFC_MIXED_JOIN": "1"}),
    "upsert_small": dict(depth=2, extra=2, seed=17, batch=256, max_batch=4096, upsert=True),
    "upsert_general": dict(depth=6, extra=2, seed=18, batch=65536, max_batch=65536, upsert=True),
    "upsert_mixed": dict(depth=6, extra=2, seed=18, batch=12000, gets=8000, max_batch=65536, upsert=True),
}
# pipelined Insert_batches and the served front-end: (depth, extra, seed) of LIMIT_CASES rows
LIMIT_PIPELINED = dict(depth=6, extra=7, seed=15, batch=12000, max_batch=16383)
LIMIT_SERVED = dict(depth=2, extra=2, seed=12, batch=1500, max_batch=8192)

# deep chains inside the pool: (D, seed), each seed with split_loss == 0 as above
DEEP_CHAIN_CASES = [(12, 21), (18, 22), (22, 23)]
# past the pool: tables whose pool is a few thousand entries beyond the fixed
# slots, through the small, the medium and the general path (batch: ops per
# batch; tail: uniform keys before each later retry of the chains' triggers)
_DEEP_POOL_D5 = dict(D=22, seed=24, groups=3, depth=5, n_uniform=4000, max_batch=4096, max_segments=128, tail=500)
DEEP_POOL_CASES = {
    "small": dict(_DEEP_POOL_D5, batch=200),
    "medium": dict(_DEEP_POOL_D5, batch=512),
    "general": dict(D=22, seed=25, groups=3, depth=7, n_uniform=12000, max_batch=16384, max_segments=256, tail=8200,
                    batch=12200),
}
