"""Inputs that put the device-side op expansion (expand_file and k_chunk_write,
sydelta_filewalk.hip) at its record, lane and unit edges -- built on the CPU, no GPU needed.

A *script* is a list of pieces laid out one after the other in the source:
    ("C", g, k)   k consecutive basis blocks from block g
    ("D", length) that many random literal bytes
    ("X", g)      block g with one byte substituted (a literal of the block's size)
`build` turns a script into (src, basis, expected_ops, records) for a seeded random basis;
tests/test_walk_expand_cases.py proves the expected ops equal the C oracle's, so that "this
file has 108 records" is a checked statement, and tests/test_gpu_walk_expand.py runs them.

The module also restates, in plain Python, what the units of a walk stage and how the host
and the kernels chain them (`walk_unit`, `expand_model`, `chunk_model`): the CPU test uses
it to place the designed record (the dropped or cut leading literal, the Data record that is
extended, the Copy that starts a unit) at the unit it is claimed for.  It models the plan,
not the kernels' arithmetic: that runs only on a GPU.
"""
from __future__ import annotations

import functools
import random
from typing import NamedTuple


# --------------------------------------------------------------------------
# helpers the issue names
# --------------------------------------------------------------------------
def lds_cap(max_nblk: int) -> int:
    """Records expand_file can gather: the walk's dynamic LDS (walk_lds, sydelta_filewalk.hip:49:
    a Bloom filter and a slot table of fw words each, 1792 bytes of roll and pass tables, the
    file's weak values) less 272 bytes of unit starts, over 20 bytes per record (a 16-byte
    WalkRec and its 4-byte op prefix; sydelta_filewalk.hip:680)."""
    nb = max(1, max_nblk)
    fw = 64
    while fw < 2 * nb:
        fw *= 2
    return (1792 + 8 * fw + 4 * ((nb + 3) & ~3) - 272) // 20


def records_of(ops, bs: int) -> int:
    """Run-length records of an op list by the kernel's rule (copy(), sydelta_filewalk.hip:411):
    a Data op is a record; a Copy joins the open run only when its block follows the run's last."""
    n, prev = 0, None  # prev: the block of the previous op when it was a Copy
    for k, a, _ in ops:
        if k == "D":
            n += 1
            prev = None
        else:
            g = a // bs
            if prev is None or g != prev + 1:
                n += 1
            prev = g
    return n


def build(script, nb: int, bs: int, ls: int | None = None, seed: int = 0, append_at: int | None = None):
    """(src, basis, expected_ops, records) of a script over a random basis of nb blocks, the
    last one of ls bytes (None: full).  A short last block may only end the script: it is
    matched only as the source's last ls bytes (the tail rule, generator.rs:156-184).
    append_at = E: one more block equal to src[E:E+bs] is appended to the basis (it must not be
    visited by the greedy walk: the expected ops do not use it)."""
    rng = random.Random(seed)
    blocks = [rng.randbytes(bs) for _ in range(nb)]
    if ls is not None and nb:
        assert 0 < ls <= bs
        blocks[-1] = blocks[-1][:ls]
    src = bytearray()
    ops = []

    def lit(data: bytes):
        if ops and ops[-1][0] == "D":
            ops[-1] = ("D", ops[-1][1], ops[-1][2] + len(data))
        else:
            ops.append(("D", len(src), len(data)))
        src.extend(data)

    for i, p in enumerate(script):
        if p[0] == "C":
            _, g, k = p
            assert 0 <= g and g + k <= nb and k > 0, p
            for j in range(g, g + k):
                if len(blocks[j]) < bs:
                    assert i == len(script) - 1 and j == g + k - 1, "a short last block only ends the source"
                ops.append(("C", j * bs, len(blocks[j])))
                src.extend(blocks[j])
        elif p[0] == "D":
            if p[1]:
                lit(rng.randbytes(p[1]))
        else:
            b = bytearray(blocks[p[1]])
            b[rng.randrange(len(b))] ^= rng.randrange(1, 256)
            lit(bytes(b))
    basis = b"".join(blocks)
    src = bytes(src)
    if append_at is not None:
        assert (ls is None or ls == bs) and append_at + bs <= len(src)
        basis += src[append_at:append_at + bs]
    return src, basis, ops, records_of(ops, bs)


def expand_ops(recs, bs: int, nbf: int, ls: int):
    """The ops of run-length records ([kind, a, off]; expand_records, sydelta_api.cpp)."""
    ops = []
    for kind, a, off in recs:
        if not kind:
            ops.append(("D", off, a))
        else:
            ops.extend(("C", g * bs, ls if g + 1 == nbf else bs) for g in range(a, a + kind))
    return ops


# --------------------------------------------------------------------------
# the plan restated: units, their staged records, the chaining rules
# --------------------------------------------------------------------------
def _basis_info(basis: bytes, bs: int):
    nbf = -(-len(basis) // bs)
    return nbf, (len(basis) - (nbf - 1) * bs if nbf else 0)


@functools.lru_cache(maxsize=8)
def _table(basis: bytes, bs: int):
    tab = {}
    for g in range(len(basis) // bs):  # full-size blocks: the lowest index of equal ones wins
        tab.setdefault(basis[g * bs:(g + 1) * bs], g)
    return tab


def walk_unit(src: bytes, basis: bytes, bs: int, entry: int, end: int, final: bool):
    """(records, exit) of one unit of k_walk_files: the greedy walk of [entry, end), its Copy
    runs by copy()'s rule, the literal run up to `end` (a final unit: the tail rule, then up
    to the source's end)."""
    tab = _table(basis, bs)
    nbf, ls = _basis_info(basis, bs)
    L = len(src)
    recs, run = [], [0, 0]

    def close():
        if run[0]:
            recs.append([run[0], run[1], 0])
        run[0] = 0

    def data(lo, hi):
        if hi > lo:
            close()
            recs.append([0, hi - lo, lo])

    def copy(g):
        if run[0] and g == run[1] + run[0]:
            run[0] += 1
        else:
            close()
            run[0], run[1] = 1, g

    x = lit = entry
    while x < end:
        g = tab.get(src[x:x + bs])
        if g is None:
            x += 1
            continue
        data(lit, x)
        copy(g)
        x += bs
        lit = x
    if final:
        if nbf and ls < bs and L >= ls and src[L - ls:] == basis[len(basis) - ls:] and L - ls >= lit:
            data(lit, L - ls)
            copy(nbf - 1)
            lit = L
        data(lit, L)
        ex = L
    else:
        data(lit, end)
        ex = max(x, end)
    close()
    return recs, ex


def file_units(src_len: int, nbf: int, bs: int, G: int, min_seg: int = 8):
    """[(entry, end, final)] of one file of a batch (match_walk_files, sydelta_api.cpp:2873-2882;
    min_seg 8: SYDELTA_FILE_SEGS is set)."""
    p1 = src_len - bs + 1 if (nbf and src_len >= bs) else 0
    nb = -(-p1 // bs)
    segb = max(min_seg, -(-nb // G)) if G > 1 else max(nb, 1)
    units, e0 = [], 0
    while True:
        e1 = min(p1, e0 + segb * bs)
        units.append((e0, e1, e1 >= p1))
        e0 = e1
        if e0 >= p1:
            return units


def _chain(first, entry, pe):
    """How a unit entered at `entry` takes the true entry pe (the previous exit): "" (they
    agree), "drop" / "cut" (its leading literal run ends at / passes pe), or "bad"."""
    if entry == pe:
        return ""
    if pe > entry and first is not None and first[0] == 0 and first[2] == entry and first[2] + first[1] >= pe:
        return "drop" if first[2] + first[1] == pe else "cut"
    return "bad"


def expand_model(src: bytes, basis: bytes, bs: int, G: int, cap: int):
    """expand_file's plan for one file: units, their record counts, why it would report bad
    ("units", "cap", "chain" or None), each unit's chaining event, the merged records."""
    nbf, ls = _basis_info(basis, bs)
    units = file_units(len(src), nbf, bs, G)
    out = {"units": units, "nu": len(units), "bad": None, "events": [], "counts": [], "m": 0, "ops": None}
    if len(units) > 64:
        out["bad"] = "units"
        return out
    walks = [walk_unit(src, basis, bs, e0, e1, fin) for e0, e1, fin in units]
    out["counts"] = [len(r) for r, _ in walks]
    if sum(out["counts"]) > cap:
        out["bad"] = "cap"
        return out
    merged = []
    for k, ((e0, _, _), (recs, _)) in enumerate(zip(units, walks)):
        recs = [list(r) for r in recs]
        ev = _chain(recs[0] if recs else None, e0, walks[k - 1][1]) if k else ""
        out["events"].append(ev)
        if ev == "bad":
            out["bad"] = "chain"
            return out
        if ev == "drop":
            recs = recs[1:]
        elif ev == "cut":
            pe = walks[k - 1][1]
            recs[0] = [0, recs[0][2] + recs[0][1] - pe, pe]
        for r in recs:
            if not r[0] and merged and not merged[-1][0] and merged[-1][2] + merged[-1][1] == r[2]:
                merged[-1][1] += r[1]
            else:
                merged.append(r)
    out["m"] = len(merged)
    out["ops"] = expand_ops(merged, bs, nbf, ls)
    return out


def chunk_units(src_len: int, nbf: int, bs: int, seg: int):
    """([(entry, end, final)], ub) of one final chunk from position 0 (chunk_units and
    chunk_pipe_launch, sydelta_api.cpp): segments of `seg` blocks; two parts (70 % / 30 %)
    from 512 segments.  (The last part is cut again only when its own segment size is below
    `seg`; the cases that reach two parts use seg 8, the least.)"""
    p1 = src_len - bs + 1 if (nbf and src_len >= bs) else 0
    units, s0 = [], 0
    while s0 < p1:
        e = min(p1, s0 + seg * bs)
        units.append((s0, e, e >= p1))
        s0 = e
    nu = len(units)
    ub = [0, min(nu - 1, max(1, nu * 7 // 10)), nu] if nu >= 512 else [0, nu]
    return units, ub


def chunk_model(src: bytes, basis: bytes, bs: int, seg: int):
    """chunk_pipe_finish's plan when every part is written on the device: per unit its staged
    record count, skip, cut flag, ext, whether its first record joins the previous op, and
    whether that join is a patch (the owner lies in an earlier part); `stop`: the first unit
    that has to be walked again (None: none)."""
    nbf, ls = _basis_info(basis, bs)
    units, ub = chunk_units(len(src), nbf, bs, seg)
    walks = [walk_unit(src, basis, bs, e0, e1, fin) for e0, e1, fin in units]
    plan, stop, owner, last = [], None, None, None  # last: the last record planned so far
    part_of = [next(j for j in range(len(ub) - 1) if ub[j] <= u < ub[j + 1]) for u in range(len(units))]
    all_recs = []
    for u, ((e0, _, _), (recs, _)) in enumerate(zip(units, walks)):
        recs = [list(r) for r in recs]
        ev = _chain(recs[0] if recs else None, e0, walks[u - 1][1]) if u else ""
        if ev == "bad":
            stop = u
            break
        p = {"cnt": len(recs), "skip": 0, "cut": 0, "ext": 0, "join": False, "patch": False, "event": ev, "nops": 0}
        if ev == "drop":
            recs = recs[1:]
            p["skip"] = 1
        elif ev == "cut":
            pe = walks[u - 1][1]
            recs[0] = [0, recs[0][2] + recs[0][1] - pe, pe]
            p["cut"] = 1
        if recs and not recs[0][0] and last is not None and not last[0] and last[2] + last[1] == recs[0][2]:
            p["join"] = True
            p["skip"] += 1
            p["cut"] = 0
            if owner is not None and part_of[owner] == part_of[u]:
                plan[owner]["ext"] += recs[0][1]
            else:
                p["patch"] = True
            last[1] += recs[0][1]
            recs = recs[1:]
        p["nops"] = sum(r[0] or 1 for r in recs)
        if recs:
            owner = u
            all_recs.extend(recs)
            last = all_recs[-1]
        plan.append(p)
    return {"units": units, "ub": ub, "plan": plan, "stop": stop,
            "ops": expand_ops(all_recs, bs, nbf, ls) if stop is None else None}


# --------------------------------------------------------------------------
# script pieces
# --------------------------------------------------------------------------
def singles(count: int, nb: int, literals: bool = False, first: int = 0):
    """`count` one-op records: Copies of non-consecutive blocks (3 apart, mod nb), every other
    one a 1-byte literal when `literals`."""
    out = []
    for i in range(count):
        if literals and i % 2 == (count % 2):  # (an odd count starts with a Copy, an even one with a literal)
            out.append(("D", 1))
        else:
            out.append(("C", (first + 3 * i) % nb, 1))
    return out


def mixed(m: int, nb: int, start: str):
    """m records, Data and Copy runs in turn (runs of 1-3 blocks), starting with `start`."""
    out = []
    for i in range(m):
        if (i % 2 == 0) == (start == "D"):
            out.append(("D", 1 + i % 5))
        else:
            out.append(("C", (7 * i) % (nb - 3), 1 + i % 3))
    return out


def segment(b0: int, nblocks: int, R: int, start: str):
    """Blocks [b0, b0 + nblocks) of an unshifted (or uniformly shifted) source as R records,
    Data and Copy in turn from `start`; every record one block but the first Copy run, which
    takes the rest (R 1 from "D": one literal run)."""
    assert 1 <= R <= nblocks
    kinds = [("D", "C")[(i + (start == "C")) % 2] for i in range(R)]
    if "C" not in kinds:
        assert R == 1
        return [("D", nblocks)]  # (in blocks: scaled by the caller)
    rest, out, g = nblocks - R, [], b0
    for kd in kinds:
        if kd == "C":
            k = 1 + rest
            rest = 0
            out.append(("C", g, k))
            g += k
        else:
            out.append(("X", g))
            g += 1
    assert g == b0 + nblocks
    return out


def _scaled(pieces, bs):
    return [("D", p[1] * bs) if p[0] == "D" else p for p in pieces]


# --------------------------------------------------------------------------
# cases
# --------------------------------------------------------------------------
class Case(NamedTuple):
    name: str
    src: bytes
    basis: bytes
    bs: int
    ops: list      # the builder's expected ops
    records: int   # records_of(ops)
    claims: dict   # what the case is named for (asserted on the CPU)


def case(name, script, nb, bs=256, ls=None, seed=0, append_at=None, **claims) -> Case:
    src, basis, ops, rec = build(script, nb, bs, ls, seed, append_at)
    return Case(name, src, basis, bs, ops, rec, claims)


class Batch(NamedTuple):
    name: str
    bs: int
    files: tuple
    segs: str      # SYDELTA_FILE_SEGS
    expect: str    # "dev": every file expanded on the device; "host": the batch fell back

    @property
    def max_nblk(self):
        return max(-(-len(c.basis) // self.bs) for c in self.files)

    @property
    def cap(self):
        return lds_cap(self.max_nblk)


def _fillers(nb: int, bs: int, seed: int, count: int = 6):
    """A few plain files of at most nb blocks (one of exactly nb: the batch's largest basis)."""
    out = [case(f"filler{seed}_full", [("C", 0, nb)], nb, bs, seed=seed)]
    for i in range(1, count):
        k = max(4, min(nb, 4 + 3 * i))
        out.append(case(f"filler{seed}_{i}", [("C", 0, 2), ("D", 1 + i), ("C", 2, k - 2)], k, bs,
                        ls=(bs // 2 + i if i % 2 else None), seed=seed + i))
    return out


@functools.lru_cache(maxsize=None)
def capacity_batches(max_nblk: int):
    """(good, over): files of cap - 1 and cap records (with and without 1-byte literals between
    the Copies) in a batch whose largest basis has max_nblk blocks; the same batch with one
    file of cap + 1 records."""
    cap = lds_cap(max_nblk)
    counts = [cap] if max_nblk >= 1024 else [cap - 1, cap]
    files = _fillers(max_nblk, 256, 100 + max_nblk, 4)
    for r in counts:
        for lits in (False, True):
            files.append(case(f"rec{r}{'lit' if lits else ''}", singles(r, max_nblk, lits), max_nblk,
                              seed=r + lits, records=r))
    over = case(f"rec{cap + 1}", singles(cap + 1, max_nblk, True), max_nblk, seed=7, records=cap + 1)
    good = Batch(f"cap{max_nblk}", 256, tuple(files), "1", "dev")
    return good, Batch(f"cap{max_nblk}over", 256, tuple(files + [over]), "1", "host")


MERGED = (0, 1, 2, 63, 64, 65, 127, 128, 129)


@functools.lru_cache(maxsize=None)
def merged_batch():
    files = _fillers(64, 256, 200, 3)
    for m in MERGED:
        for start in ("D", "C"):
            if m == 0 and start == "C":
                continue
            files.append(case(f"m{m}{start}", mixed(m, 64, start), 64, seed=300 + m, records=m))
    files.append(case("empty_basis", [("D", 700)], 0, seed=1, records=1))
    files.append(case("short_source", [("D", 100)], 20, seed=2, records=1))
    files.append(case("short_equal", [("C", 0, 1)], 1, ls=100, seed=3, records=1))  # the tail rule alone
    return Batch("merged", 256, tuple(files), "1", "dev")


OPCOUNTS = (63, 64, 65, 128, 4097)
RUNS = (1, 64, 65, 200, 1000)
RUN_STARTS = (0, 63, 64)


@functools.lru_cache(maxsize=None)
def opcount_batch():
    files = []
    for t in OPCOUNTS:
        if t == 4097:
            script = [("C", 0, 1000), ("D", 3)] + [("C", 0, 1000)] * 3 + [("C", 0, 96)]
            nb = 1024
        else:
            script = [("C", 0, t // 3), ("D", 3), ("C", 100, t - 1 - t // 3)]
            nb = 256
        files.append(case(f"ops{t}", script, nb, seed=400 + t, nops=t))
    for k in RUNS:
        for p in RUN_STARTS:
            pre = [("D", 1) if i % 3 == 2 else ("C", (7, 3)[i % 2], 1) for i in range(p)]
            script = pre + [("C", 20, k), ("D", 2), ("C", 5, 1)]
            files.append(case(f"run{k}at{p}", script, 1024 if k > 200 else 256, seed=500 + k + p, run=(p, k)))
    files.append(case("run1024", [("C", 0, 1024)], 1024, seed=600, run=(0, 1024)))
    pre = [("D", 1) if i % 3 == 2 else ("C", (7, 3)[i % 2], 1) for i in range(70)]
    files.append(case("run1000after70", pre + [("C", 0, 1000)], 1024, seed=601, run=(70, 1000)))
    return Batch("opcounts", 256, tuple(files), "1", "dev")


@functools.lru_cache(maxsize=None)
def lastblock_batch(bs: int):
    ls = bs // 3 + 1
    files = _fillers(12, bs, 700 + bs, 3)
    files.append(case("full_last_mid", [("C", 0, 3), ("C", 11, 1), ("D", 5), ("C", 4, 2)], 12, bs, seed=1))
    files.append(case("full_last_in_run", [("C", 8, 4), ("C", 0, 2)], 12, bs, seed=2))
    files.append(case("tail_absorbed", [("C", 0, 2), ("D", 3), ("C", 5, 7)], 12, bs, ls=ls, seed=3, last=("C", 11 * bs, ls)))
    files.append(case("tail_after_literal", [("C", 0, 2), ("D", 3), ("C", 5, 6), ("D", 9), ("C", 11, 1)], 12, bs, ls=ls,
                      seed=4, last=("C", 11 * bs, ls)))
    return Batch(f"lastblock{bs}", bs, tuple(files), "1", "dev")


def _shifted(s: int, nslots: int, edits: bool, bs: int = 256, seg: int = 8):
    """Block 0, s inserted bytes, then blocks 1 .. nslots - 1 (every unit after the first starts
    s bytes before a block, inside the previous unit's last Copy); edits: the first block past
    each unit boundary is a literal instead."""
    script = [("C", 0, 1), ("D", s)]
    g = 1
    while g < nslots:
        e = min(nslots, (g // seg + 1) * seg)
        if edits and g % seg == 0:
            script.append(("X", g))
            g += 1
        script.append(("C", g, e - g))
        g = e
    return script


@functools.lru_cache(maxsize=None)
def joins_batch():
    """Three units of 8 blocks per file (SYDELTA_FILE_SEGS=3)."""
    files = _fillers(8, 256, 800, 3)
    files.append(case("lit_crosses", [("C", 0, 6), ("D", 1024), ("C", 10, 14)], 24, seed=1, events=["", "", ""], nops=21))
    files.append(case("lit_swallows_unit", [("C", 0, 6), ("D", 3072), ("C", 18, 6)], 24, seed=2, events=["", "", ""],
                      nops=13))
    files.append(case("lit_is_unit", [("C", 0, 8), ("D", 2048), ("C", 16, 8)], 24, seed=3, events=["", "", ""], nops=17))
    return Batch("joins", 256, tuple(files), "3", "dev")


@functools.lru_cache(maxsize=None)
def shifted_batch():
    """Five units of 8 blocks per file (SYDELTA_FILE_SEGS=5)."""
    files = _fillers(8, 256, 900, 3)
    for s in (1, 255):
        files.append(case(f"shift{s}_drop", _shifted(s, 40, False), 40, seed=10 + s, events=[""] + ["drop"] * 4))
        files.append(case(f"shift{s}_cut", _shifted(s, 40, True), 40, seed=20 + s, events=[""] + ["cut"] * 4))
    return Batch("shifted", 256, tuple(files), "5", "dev")


def _good_small(count: int, seed: int):
    """Good files of at most 40 blocks: shifted, literal joins, mixed records."""
    out = []
    for i in range(count):
        k = i % 4
        if k == 0:
            out.append(case(f"g{seed}_{i}", _shifted(1 + (17 * i) % 255, 40, i % 8 == 0), 40, seed=seed + i))
        elif k == 1:
            out.append(case(f"g{seed}_{i}", [("C", 0, 6), ("D", 600 + 50 * i), ("C", 10, 14)], 24, seed=seed + i))
        elif k == 2:
            out.append(case(f"g{seed}_{i}", mixed(10 + i % 40, 40, "DC"[i % 2]), 40, seed=seed + i))
        else:
            out.append(case(f"g{seed}_{i}", [("C", 0, 3), ("D", 2 + i), ("C", 5, 7)], 12, ls=90 + i, seed=seed + i))
    return out


NOCHAIN_E = 2048  # the first unit boundary of an 8-block segmentation at bs 256


@functools.lru_cache(maxsize=None)
def nochain_batch():
    """64 good files and one whose second unit starts with a Copy (of the appended block, equal
    to the source at the boundary the first unit's last Copy crosses): it needs a re-walk."""
    files = _good_small(64, 1000)
    files.insert(40, case("nochain", _shifted(7, 40, False), 40, seed=5, append_at=NOCHAIN_E,
                          events=["", "bad"]))
    return Batch("nochain", 256, tuple(files), "5", "host")


@functools.lru_cache(maxsize=None)
def unitcount_batches():
    out = []
    for nblk, G, expect in ((512, 64, "dev"), (520, 65, "host")):
        script = [("C", 0, 7), ("D", 512), ("C", 9, 91), ("X", 100), ("C", 101, nblk - 101)]
        files = _fillers(8, 256, 1100, 2) + [case(f"units{G}", script, nblk, seed=G, nu=G)]
        out.append(Batch(f"units{G}", 256, tuple(files), str(G), expect))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def pairs_batch():
    """130 good files from the groups above (sydelta_delta_pairs_device, SYDELTA_FILE_SEGS=5)."""
    files = [c for c in merged_batch().files] + list(lastblock_batch(256).files) + \
        [c for c in joins_batch().files] + [c for c in shifted_batch().files]
    files += _good_small(130 - len(files), 2000)
    assert len(files) == 130
    return Batch("pairs", 256, tuple(files), "5", "dev")


def file_batches():
    """Every batch of the match_batch cases, in the order they are run."""
    out = []
    for nb in (32, 64, 1024):
        out.extend(capacity_batches(nb))
    out += [merged_batch(), opcount_batch()] + [lastblock_batch(bs) for bs in (256, 320, 8192)]
    out += [joins_batch(), shifted_batch(), nochain_batch()] + list(unitcount_batches())
    return out


# --------------------------------------------------------------------------
# k_chunk_write: one file, a chunk's segments
# --------------------------------------------------------------------------
class ChunkCase(NamedTuple):
    name: str
    src: bytes
    basis: bytes
    bs: int
    ops: list
    seg: int       # blocks per segment ("" in the environment when 128)
    dx: str        # SYDELTA_DEVICE_EXPAND
    claims: dict   # per unit: what chunk_model must say


def _chunk(name, script, nb, seg, dx="1", bs=256, ls=None, seed=0, append_at=None, **claims) -> ChunkCase:
    src, basis, ops, _ = build(script, nb, bs, ls, seed, append_at)
    return ChunkCase(name, src, basis, bs, ops, seg, dx, claims)


SEG_RECORDS = {128: (1, 63, 64, 65, 127, 128), 1024: (1, 63, 64, 65, 127, 128, 129, 200)}


@functools.lru_cache(maxsize=None)
def chunk_records_case(seg: int):
    """Case 10: one segment per record count (odd counts start and end with a Copy run, even
    ones start with a literal: no segment's first record joins the previous one), then ten
    blocks and the short last block."""
    script, counts = [], SEG_RECORDS[seg]
    for i, r in enumerate(counts):
        script += segment(i * seg, seg, r, "C" if r % 2 else "D")
    nb = len(counts) * seg + 11
    script.append(("C", len(counts) * seg, 11))
    return _chunk(f"records_seg{seg}", script, nb, seg, ls=77, seed=seg, counts=counts)


@functools.lru_cache(maxsize=None)
def chunk_ext_case():
    """Case 11 at 256-block segments: units of 64, 65 and 131 records whose last record is a
    literal that runs into the next segment (ext), the last of them across a wholly literal
    segment (its ext taken twice; that unit writes no op)."""
    S = 256
    script = segment(0, S, 64, "C") + segment(S, S, 2, "D")
    script += segment(2 * S, S, 65, "D") + segment(3 * S, S, 2, "D")
    script += segment(4 * S, S, 131, "D") + _scaled(segment(5 * S, S, 1, "D"), 256) + segment(6 * S, S, 2, "D")
    script.append(("C", 7 * S, 11))
    return _chunk("ext", script, 7 * S + 11, S, ls=77, seed=11,
                  owners={0: 64, 2: 65, 4: 131}, silent=5)


CHUNK_SHIFT = 5


@functools.lru_cache(maxsize=None)
def chunk_skip_case():
    """Case 12 at the default 128-block segments, the source shifted by 5 bytes after block 0:
    unit 1's leading literal ends at the previous exit (dropped: skip 1, 102 records), unit 2's
    passes it (cut, 100 records), unit 3 is one literal run, cut at its start and extended by
    unit 4's leading literal (which is joined: skip 1)."""
    S = 128
    script = [("C", 0, 1), ("D", CHUNK_SHIFT), ("C", 1, S - 1)]
    script += segment(S, S, 101, "C") + segment(2 * S, S, 100, "D")
    script += _scaled(segment(3 * S, S, 1, "D"), 256) + segment(4 * S, S, 4, "D")
    script.append(("C", 5 * S, 11))
    return _chunk("skip", script, 5 * S + 11, S, ls=77, seed=12)


PATCH_BLOCKS = 4200


@functools.lru_cache(maxsize=None)
def chunk_patch_case():
    """Case 13: 8-block segments, two parts; a two-block literal straddles the part boundary,
    so the device-written part's first record joins the host-assembled part's last op."""
    bs, nb, ls = 256, PATCH_BLOCKS, 77
    units, ub = chunk_units((nb - 1) * bs + ls, nb, bs, 8)
    assert len(ub) == 3
    cut = units[ub[1]][0] // bs  # the first block of the last part
    rng = random.Random(13)
    lits = sorted(set(rng.sample(range(10, nb - 10), 40)) - {cut - 2, cut - 1, cut, cut + 1})
    marks = sorted(lits + [cut - 1])
    script, g = [], 0
    for b in marks:
        if b > g:
            script.append(("C", g, b - g))
        if b == cut - 1:
            script.append(("D", 2 * bs))
            g = b + 2
        else:
            script.append(("X", b))
            g = b + 1
    script.append(("C", g, nb - g))
    return _chunk("patch", script, nb, 8, dx="", ls=ls, seed=13, boundary=ub[1])


@functools.lru_cache(maxsize=None)
def chunk_rewalk_case(dx: str):
    """Case 14: 8-block segments, two parts, the source shifted by 7 bytes; the basis gets one
    more block equal to the source at a segment boundary of the last part, so that unit starts
    with a Copy and is walked again after the device wrote the units before it."""
    bs, nslots = 256, PATCH_BLOCKS
    L = nslots * bs + 7
    units, ub = chunk_units(L, nslots + 1, bs, 8)
    assert len(ub) == 3
    u = ub[1] + 50
    return _chunk(f"rewalk_dx{dx or 'unset'}", _shifted(7, nslots, False), nslots, 8, dx=dx, seed=14,
                  append_at=units[u][0], stop=u)


@functools.lru_cache(maxsize=None)
def chunk_tail_cases(bs: int):
    """Case 15: the short last block in the final unit, absorbed by a run and after a literal."""
    ls = bs // 2 + 3
    a = _chunk(f"tail_absorbed_bs{bs}", [("C", 0, 100), ("X", 100), ("C", 101, 199)], 300, 128, bs=bs, ls=ls, seed=bs)
    b = _chunk(f"tail_after_literal_bs{bs}", [("C", 0, 100), ("X", 100), ("C", 101, 198), ("D", 9), ("C", 299, 1)],
               300, 128, bs=bs, ls=ls, seed=bs + 1)
    return a, b


def chunk_cases():
    out = [chunk_records_case(128), chunk_records_case(1024), chunk_ext_case(), chunk_skip_case(), chunk_patch_case(),
           chunk_rewalk_case(""), chunk_rewalk_case("1")]
    for bs in (256, 4096):
        out.extend(chunk_tail_cases(bs))
    return out
