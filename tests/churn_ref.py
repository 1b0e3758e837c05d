"""Churn scripts and their serial answer (test infrastructure).

Erase exists for churn: keys leave, fresh keys come, segments
keep splitting and the directory keeps doubling.  A script is a seeded list of
steps, ("mixed", ops, keys, values) of at most STEP_MAX ops or ("erase", keys),
one round's whole erase (Erase takes it in pieces), applied in order to one table; run_oracle gives what the serial oracle
(oracle/cceh_oracle.c, which now carries Erase) answers to every step, its
dump around every erase step and at the end, and its counters there.

  churn             10 rounds from CCEH_hybrid(2), each a few mixed steps (60 %
                    inserts: fresh keys, ~10 % re-inserts of keys erased in
                    earlier rounds, ~5 % second copies of live keys; 40 % Gets
                    of live, erased and never-stored keys) and one erase step
                    (a seeded half of the live keys, 200 never-stored keys, 50
                    keys a second time, the two reserved keys, shuffled).  The
                    rounds grow by half each, so the table splits and doubles
                    after every erase; the live set ends near 70k keys, and
                    from the eighth erase on every segment is 7 levels deep.
  churn_short       the same generator at ~26k ops, for the small cuttings.
  churn_upsert      churn with 25 % re-inserts of live keys, for upsert tables.
  loss_after_erase  scenarios.split_loss(13, mixed=True) with an erase step
                    before its triggers and the erased keys at its end.
  unsplittable      dup32, the 33rd copy, erase, two copies, 32 again, the 33rd.

Two more step kinds let a script shrink its table:
("match", mask, patterns), EraseMatching, whose serial answer is Erase of
match_ref.matching_keys of the oracle's dump, and ("compact", fill_limit),
Compact, whose answer is compact_ref.compact of the oracle's dump at the
script's initial depth; the oracle, which cannot merge, starts again from that
image (oc_load) when something merged.  The regrow scripts (the generator
_regrow: _churn's mixed and erase steps under a plan) use them:

  regrow            72k fresh keys (every segment 7 or 8 deep), match (mask 7,
                    two patterns: a quarter of the keys), erase 90 %, compact
                    512 (depth 8 -> 4), 40k keys, erase 50 %, 46k keys (7 deep
                    again, with two whole steps to spare), erase 95 %, compact
                    1024 (to depth 3, four pairs refused for a drop), 76k
                    keys: 7 deep a third time.  About 560k ops.
  regrow_short      the same plan at 6k, 2k, 5k and 7k keys (~48k ops, depth
                    4 -> 1 -> 4 -> 1 -> 4), for the small cuttings, the served
                    front-end and the shards.
  regrow_upsert     an upsert table, 25 % re-inserts of live keys: 72k keys,
                    erase 90 %, compact 512, 76k keys, erase 90 %, compact 256
                    (partial: local depths 5 and 6 stay), 76k keys.
  lopsided          75k keys, a compact 256 that merges nothing, one erase of
                    97 % of the keys outside the first quarter of the hash
                    space, compact 512 (local depths 3 to 8 under an unchanged
                    depth 8), 30k and 60k keys.

tests/test_churn_ref.py checks on the CPU that the scripts reach what they
are for and that every erase step of the oracle is erase_ref's;
tests/test_gpu_churn_exact.py and tests/test_gpu_regrow_exact.py replay them
on the engine.
"""
import numpy as np

import compact_ref
import match_ref
import scenarios as S
from limits_ref import INVALID, SENTINEL, hash64
from oracle import oracle as O
from pmdfc_amd.workload import uniform_keys

OP_GET, OP_INSERT = 0, 1
STEP_MAX = 16384


class Script:
    """name, the table's initial depth and insert mode, and the steps."""

    def __init__(self, name, depth, upsert, steps):
        self.name, self.depth, self.upsert, self.steps = name, depth, upsert, steps
        for s in steps:  # (an erase step is one round's whole erase; Erase takes it in pieces of max_batch)
            if s[0] == "match":  # (mask, patterns: at most MATCH_MAX of them)
                assert len(s) == 3 and 1 <= len(s[2]) <= 1024, (name, s[0])
                continue
            if s[0] == "compact":  # (fill_limit)
                assert len(s) == 2 and 1 <= s[1] <= 1024, (name, s)
                continue
            assert s[0] == "erase" or (s[0] == "mixed" and len(s[1]) <= STEP_MAX), (name, s[0], len(s[1]))

    def steps_of(self, kind):
        return [i for i, s in enumerate(self.steps) if s[0] == kind]

    def erase_steps(self):
        return self.steps_of("erase")

    def ops(self):
        return sum(len(s[1]) for s in self.steps if s[0] in ("mixed", "erase"))


def _mixed_steps(ops, keys, vals):
    return [("mixed", ops[a:a + STEP_MAX], keys[a:a + STEP_MAX], vals[a:a + STEP_MAX])
            for a in range(0, len(ops), STEP_MAX)]


def _churn(name, seed, rounds, f0, growth, p_again=0.05, p_back=0.10, upsert=False):
    """The churn generator.  Round r inserts about f0 * growth^r fresh keys.
    The generator follows the keys it believes live (inserted and not erased
    since) and gone (erased and not inserted again); a split may drop a live
    key, which only turns some Get or erase of it into a miss.  Values number
    the inserts of the whole script from 1 on, so every copy of a key differs."""
    rng = np.random.default_rng(seed)
    never = uniform_keys(seed + 1, 0, 1 << 16)
    live = np.zeros(0, np.uint64)
    gone = np.zeros(0, np.uint64)
    pos, serial, steps = 0, 0, []
    for r in range(rounds):
        nf = int(f0 * growth ** r)
        n_ins = int(nf / (1.0 - p_again - p_back))
        fresh = uniform_keys(seed, pos, nf)
        pos += nf
        take = rng.permutation(gone.size)[:int(p_back * n_ins)]
        back = gone[take]
        gone = np.delete(gone, take)
        pool = np.concatenate([live, fresh, back])  # live by the end of the round's mixed steps
        again = pool[rng.integers(0, pool.size, int(p_again * n_ins))]
        ins = np.concatenate([fresh, back, again])
        n_get = ins.size * 2 // 3  # 60 % inserts, 40 % Gets
        past = gone if gone.size else never
        gets = np.concatenate([pool[rng.integers(0, pool.size, n_get // 2)],
                               past[rng.integers(0, past.size, n_get // 4)],
                               never[rng.integers(0, never.size, n_get - n_get // 2 - n_get // 4)]])
        keys = np.concatenate([ins, gets])
        ops = np.concatenate([np.full(ins.size, OP_INSERT, np.uint8), np.full(gets.size, OP_GET, np.uint8)])
        p = rng.permutation(keys.size)
        ops, keys = ops[p], keys[p]
        vals = np.zeros(keys.size, np.uint64)
        vals[ops == OP_INSERT] = np.arange(serial + 1, serial + 1 + ins.size, dtype=np.uint64)
        serial += ins.size
        steps += _mixed_steps(ops, keys, vals)
        live = np.unique(pool)
        go = rng.random(live.size) < 0.5
        out = live[go]
        plan = np.concatenate([out, never[rng.integers(0, never.size, 200)], out[rng.permutation(out.size)[:50]],
                               np.array([INVALID, SENTINEL], np.uint64)])
        steps.append(("erase", plan[rng.permutation(plan.size)]))
        live = live[~go]
        gone = np.concatenate([gone, out])
    stored = np.concatenate([s[2][s[1] == OP_INSERT] for s in steps if s[0] == "mixed"])
    assert not np.any(np.isin(never, stored)) and np.all(stored < np.uint64(SENTINEL))
    return Script(name, 1, upsert, steps)


def _regrow(name, seed, plan, p_again=0.05, p_back=0.03, upsert=False):
    """The shrink-and-regrow generator.  `plan` lists what happens in order:
      ("ins", n)               n fresh keys, about p_back re-inserts of gone keys and p_again second copies of
                               live keys, and Gets equal to two thirds of the inserts (live, gone, never-stored
                               keys as in _churn), shuffled, in mixed steps;
      ("erase", f)             one erase step: a seeded fraction f of the live keys, with _churn's 200 never-stored
                               keys, 50 repeats and the two reserved keys;
      ("erase", f, pred)       the same over the live keys k with pred(hash64(k)) only;
      ("match", mask, pats)    the step itself; the live keys under the pattern become gone;
      ("compact", fill_limit)  the step itself.
    live and gone are kept as in _churn, values number the inserts from 1 on."""
    rng = np.random.default_rng(seed)
    never = uniform_keys(seed + 1, 0, 1 << 16)
    live = np.zeros(0, np.uint64)
    gone = np.zeros(0, np.uint64)
    pos, serial, steps = 0, 0, []
    for act in plan:
        if act[0] == "ins":
            nf = act[1]
            n_ins = int(nf / (1.0 - p_again - p_back))
            fresh = uniform_keys(seed, pos, nf)
            pos += nf
            take = rng.permutation(gone.size)[:int(p_back * n_ins)]
            back = gone[take]
            gone = np.delete(gone, take)
            pool = np.concatenate([live, fresh, back])
            again = pool[rng.integers(0, pool.size, int(p_again * n_ins))]
            ins = np.concatenate([fresh, back, again])
            n_get = ins.size * 2 // 3
            past = gone if gone.size else never
            gets = np.concatenate([pool[rng.integers(0, pool.size, n_get // 2)],
                                   past[rng.integers(0, past.size, n_get // 4)],
                                   never[rng.integers(0, never.size, n_get - n_get // 2 - n_get // 4)]])
            keys = np.concatenate([ins, gets])
            ops = np.concatenate([np.full(ins.size, OP_INSERT, np.uint8), np.full(gets.size, OP_GET, np.uint8)])
            p = rng.permutation(keys.size)
            ops, keys = ops[p], keys[p]
            vals = np.zeros(keys.size, np.uint64)
            vals[ops == OP_INSERT] = np.arange(serial + 1, serial + 1 + ins.size, dtype=np.uint64)
            serial += ins.size
            steps += _mixed_steps(ops, keys, vals)
            live = np.unique(pool)
        elif act[0] == "erase":
            go = rng.random(live.size) < act[1]
            if len(act) > 2:
                go &= act[2](hash64(live))
            out = live[go]
            plan_k = np.concatenate([out, never[rng.integers(0, never.size, 200)], out[rng.permutation(out.size)[:50]],
                                     np.array([INVALID, SENTINEL], np.uint64)])
            steps.append(("erase", plan_k[rng.permutation(plan_k.size)]))
            live = live[~go]
            gone = np.concatenate([gone, out])
        elif act[0] == "match":
            mask, pats = np.uint64(act[1]), np.asarray(act[2], np.uint64)
            steps.append(("match", int(mask), pats))
            go = np.isin(live & mask, pats & mask)
            gone = np.concatenate([gone, live[go]])
            live = live[~go]
        else:
            assert act[0] == "compact"
            steps.append(("compact", act[1]))
    stored = np.concatenate([s[2][s[1] == OP_INSERT] for s in steps if s[0] == "mixed"])
    assert not np.any(np.isin(never, stored)) and np.all(stored < np.uint64(SENTINEL))
    return Script(name, 1, upsert, steps)


def _regrow_plan(a, b, c, d):
    """regrow's plan at a, b, c and d fresh keys."""
    return [("ins", a), ("match", 7, [3, 5]), ("erase", 0.90), ("compact", 512),
            ("ins", b), ("erase", 0.50), ("ins", c), ("erase", 0.95), ("compact", 1024), ("ins", d)]


def _top2_nonzero(h):
    return (h >> np.uint64(62)) != np.uint64(0)


# loss_after_erase: the erase step removes each stored key with probability
# 1/3.  What is stored then is A (32 keys of home line 248 in slots 992..1023)
# and B (28 keys of home line 255, wrapped to slots 0..27).  The split that the
# first trigger asks for drops an entry only if the window [992, 1024) is full
# again after the erase and still holds at least 29 keys of A: the shift moves
# B's entries into the slots 1020.. that A's erased keys leave, so at most 3
# keys of A may go (and at least one should, or the erase leaves the window as
# it was).  1 seed in ~500 draws such a third; 671 is the first from 0 up that
# does and erases at least a quarter of the 60 keys.  test_churn_ref.py asserts
# what the seed is for: split_loss grows after the erase step.
LOSS_ERASE_SEED = 671


def _loss_after_erase():
    ops, keys, vals = S.split_loss(13, hash64, mixed=True)
    cut = 32 + 28 + 60  # the inserts of A and B and their first Gets: before the first trigger
    stored = keys[:cut][ops[:cut] == OP_INSERT]
    go = np.random.default_rng(LOSS_ERASE_SEED).random(stored.size) < 1 / 3
    assert 1 <= np.count_nonzero(go & ((hash64(stored) & np.uint64(0xFF)) == np.uint64(248))) <= 3
    gone = stored[go]
    back_v = np.arange(1, gone.size + 1, dtype=np.uint64) + np.uint64(1 << 40)
    r_ops = np.concatenate([ops[cut:], np.full(gone.size, OP_INSERT, np.uint8), np.full(gone.size, OP_GET, np.uint8)])
    r_keys = np.concatenate([keys[cut:], gone, gone])
    r_vals = np.concatenate([vals[cut:], back_v, np.zeros(gone.size, np.uint64)])
    steps = _mixed_steps(ops[:cut], keys[:cut], vals[:cut]) + [("erase", gone)] + _mixed_steps(r_ops, r_keys, r_vals)
    return Script("loss_after_erase", 1, False, steps)


def _unsplittable():
    init_cap, _, ops, keys, vals = S.scenarios(hash64)["dup32"]
    u, c = np.unique(keys[ops == OP_INSERT], return_counts=True)
    k = u[np.argmax(c)]
    assert c.max() == 32

    def ins(n, first):
        return ("mixed", np.full(n, OP_INSERT, np.uint8), np.full(n, k, np.uint64),
                np.arange(first, first + n, dtype=np.uint64))

    steps = _mixed_steps(ops, keys, vals) + [
        ins(1, 100),                                                    # the 33rd copy: UNSPLITTABLE
        ("erase", np.array([k], np.uint64)),                            # ERASED, all 32 copies
        ("mixed", np.array([1, 1, 0], np.uint8), np.full(3, k, np.uint64), np.array([201, 202, 0], np.uint64)),
        ins(30, 301),                                                   # 32 copies again
        ins(1, 400),                                                    # UNSPLITTABLE again
    ]
    return Script("unsplittable", O.OracleCCEH.depth_for_hybrid(init_cap), False, steps)


_BUILDERS = {
    "churn": lambda: _churn("churn", 101, 10, 2100, 1.5),
    "churn_short": lambda: _churn("churn_short", 102, 5, 300, 2.0),
    "churn_upsert": lambda: _churn("churn_upsert", 103, 10, 2100, 1.5, p_again=0.25, upsert=True),
    "loss_after_erase": _loss_after_erase,
    "unsplittable": _unsplittable,
    "regrow": lambda: _regrow("regrow", REGROW_SEED, _regrow_plan(72000, 40000, 46000, 76000)),
    "regrow_short": lambda: _regrow("regrow_short", 202, _regrow_plan(6000, 2000, 5000, 7000)),
    "regrow_upsert": lambda: _regrow("regrow_upsert", 203, [
        ("ins", 72000), ("erase", 0.90), ("compact", 512), ("ins", 76000), ("erase", 0.90), ("compact", 256),
        ("ins", 76000)], p_again=0.25, upsert=True),
    "lopsided": lambda: _regrow("lopsided", 204, [
        ("ins", 75000), ("compact", 256), ("erase", 0.97, _top2_nonzero), ("compact", 512), ("ins", 30000), ("ins", 60000)]),
}
# A compact step is refused a pair when one within the limit would drop an entry in its replay.  At limit 1024 on a
# table thinned to 5 % that happens at these sizes under every seed tried (201..212: 1 to 4 pairs); 201 leaves four
# at regrow's second compact step, and tests/test_churn_ref.py asserts refused > 0 there.
REGROW_SEED = 201
NAMES = list(_BUILDERS)
_SCRIPTS, _RUNS = {}, {}


def script(name) -> Script:
    """Script `name`, built once and never changed."""
    if name not in _SCRIPTS:
        _SCRIPTS[name] = _BUILDERS[name]()
    return _SCRIPTS[name]


def insert_only(s: Script) -> Script:
    """The script without its Gets (for the insert-only calls)."""
    name = s.name + "/inserts"
    if name not in _SCRIPTS:
        steps = []
        for st in s.steps:
            if st[0] == "mixed":
                m = st[1] == OP_INSERT
                steps.append(("mixed", st[1][m], st[2][m], st[3][m]))
            else:
                steps.append(st)
        _SCRIPTS[name] = Script(name, s.depth, s.upsert, steps)
    return _SCRIPTS[name]


class Run:
    """The oracle's answer to a script.
    results[i]  a mixed step's (values, statuses), an erase step's statuses, a
                match step's four result fields (match_ref.erase_matching), a
                compact step's counts (compact_ref.compact);
    pre[i], post[i]  the dump before and after erase, match or compact step i;
                final: at the end;
    marks[i]    depth, segments, live and the oracle's counters after erase,
                match or compact step i; marks[len(steps)]: at the end;
    matched[i]  a match step's (the keys L it erased in order, their statuses,
                the model table's image afterwards);
    min_ld[i]   the smallest local depth after step i, of whatever kind."""

    def __init__(self):
        self.results, self.pre, self.post, self.marks, self.final, self.stats = [], {}, {}, {}, None, None
        self.matched, self.min_ld = {}, []


def _mark(o, dump):
    m = dict(o.stats())
    m.update(depth=o.depth, segments=o.num_segments,
             live=int(np.count_nonzero(np.asarray(dump["keys"], np.uint64) != np.uint64(INVALID))))
    return m


def run_oracle(s: Script, depth=None, upsert=None, reload=False) -> Run:
    """Computed once per (script, depth, upsert) and cached: leave it unchanged.
    A match step is the contract of match_ref.py: Erase of the matching keys of
    the dump, in its order.  A compact step is the model's: compact_ref.compact
    of the dump at the run's initial depth, which the oracle loads (oc_load)
    when something merged and ignores otherwise.  reload: the oracle also loads
    its own dump after every step, which must change nothing."""
    depth = s.depth if depth is None else depth
    upsert = s.upsert if upsert is None else upsert
    key = (s.name, depth, upsert, reload)
    if key in _RUNS:
        return _RUNS[key]
    o = O.OracleCCEH(depth, upsert=upsert)
    r = Run()
    for i, st in enumerate(s.steps):
        if st[0] == "mixed":
            r.results.append(o.mixed(st[1], st[2], st[3]))
        else:
            r.pre[i] = o.dump()
            if st[0] == "erase":
                r.results.append(o.erase(st[1]))
            elif st[0] == "match":
                L = match_ref.matching_keys(r.pre[i], st[1], st[2])
                m, res = match_ref.erase_matching(r.pre[i], st[1], st[2], upsert)
                r.results.append(res)
                r.matched[i] = (L, o.erase(L), m.image())
            else:
                want, res = compact_ref.compact(r.pre[i], depth, st[1])
                r.results.append(res)
                if res["merges"] > 0:
                    o.load(want)
            r.post[i] = o.dump()
            r.marks[i] = _mark(o, r.post[i])
        r.min_ld.append(int(np.min(o.dump()["local_depth"])))
        if reload:
            o.load(o.dump())
    r.final = o.dump()
    r.marks[len(s.steps)] = _mark(o, r.final)
    r.stats = o.stats()
    assert r.stats["early_exit_mismatch"] == 0  # (Invariant I: the early exit of every Get found what the full scan finds)
    o.close()
    _RUNS[key] = r
    return r


def copies_erased(s: Script, r: Run) -> int:
    """Sum over the keys answered ERASED of (copies stored at that moment - 1):
    the counts an attached counting filter keeps too many."""
    extra = 0
    for i in s.erase_steps():
        k, c = np.unique(np.asarray(r.pre[i]["keys"], np.uint64), return_counts=True)
        hit = s.steps[i][1][r.results[i] == O.ST_ERASED]  # (each key ERASED once per step: its repeats miss)
        extra += int(np.sum(c[np.searchsorted(k, hit)] - 1))
    return extra
