"""The collision scenarios of tests/adler_twins.py hold what they are built for: twins share
Adler-32 and differ in XXH3; on every scenario the two oracles agree, the delta rebuilds the
source, and the op list is the one written out by hand in the builder (the Copy offsets of
the later candidates, Data over the twins no basis block matches, no Copy for the tail's
twin).  CPU only: the GPU paths are held to the same scenarios in test_gpu_collisions.py."""
import random
import zlib

import pytest

import adler_twins as T
from oracle import oracle as O

BLOCK_SIZES = [256, 320, 1024, 4096, 8192, 65536]


@pytest.mark.parametrize("bs", BLOCK_SIZES)
def test_twins_share_adler_differ_in_xxh3(bs):
    rng = random.Random(bs)
    for n in (bs, bs // 2 + 3, 85):
        blk = rng.randbytes(n)
        fam = T.family(blk, rng, 25)
        assert len(set(fam)) == 25 and all(len(x) == n for x in fam)
        assert {zlib.adler32(x) for x in fam} == {zlib.adler32(blk)}
        assert {O.py_adler32(x) for x in fam[:3]} == {zlib.adler32(blk)}
        assert len({O.py_xxh3(x) for x in fam}) == 25
    one = T.twin(blk, rng, 1)  # a single step already is a twin
    assert one != blk and zlib.adler32(one) == zlib.adler32(blk) and O.py_xxh3(one) != O.py_xxh3(blk)
    assert sum(a != b for a, b in zip(one, blk)) == 4


def _c_ops(oracle_c, sc):
    if sc.sig is not None:
        w, s, z = sc.sig
    else:
        w, s, z = oracle_c.compute_checksums(sc.basis, sc.bs)
    return O.ops_from_arrays(*oracle_c.generate_delta(sc.src, w, s, z, sc.bs))


def _py_ops(sc):
    if sc.sig is not None:
        w, s, z = sc.sig
        sigs = [O.BlockChecksum(i, i * sc.bs, int(z[i]), int(w[i]), int(s[i])) for i in range(len(w))]
    else:
        sigs = O.py_compute_checksums(sc.basis, sc.bs)
    return O.py_generate_delta(sc.src, sigs, sc.bs)


@pytest.mark.parametrize("bs", BLOCK_SIZES)
def test_scenarios_oracles_agree_and_show_their_fact(oracle_c, bs):
    scs = T.scenarios(bs)
    names = [sc.name for sc in scs]
    assert len(set(names)) == len(names)
    for want in ("later-candidate", "family", "dup+collision", "synthetic-R6", "overlap(1)", "overlap(63)",
                 "overlap(64)", "overlap(65)", f"overlap({bs - 1})"):
        assert want in names, want
    assert sum(n.startswith("tail-twin") for n in names) == 2 and sum(n.startswith("tail-true") for n in names) == 2
    if bs == 8192:
        assert {"overlap(4095)", "overlap(4096)", "overlap(4097)"} <= set(names)
    if bs == 4096:
        assert {f"overlap({d})" for d in (7, 8, 9, 4095, 4096, 4097)} <= set(names)
    for sc in scs:
        ops = _c_ops(oracle_c, sc)
        assert ops == sc.expect, (bs, sc.name)
        if bs <= 1024:
            assert _py_ops(sc) == ops, (bs, sc.name)
        if sc.sig is None:
            assert O.py_apply_delta(sc.basis, sc.src, ops) == sc.src, (bs, sc.name)
            assert sc.nblocks() <= 64


@pytest.mark.parametrize("bs", [256, 4096])
def test_scenarios_structural_facts(oracle_c, bs):
    """The facts by themselves, from the oracle's ops and the inputs (not from `expect`)."""
    by = {sc.name: sc for sc in T.scenarios(bs)}
    adler = zlib.adler32

    def blocks(sc):
        return [sc.basis[o:o + bs] for o in range(0, len(sc.basis), bs)]

    # later-candidate: the Copies name blocks 3 and 2; F3 (weak of the family, no block's strong) is Data
    sc = by["later-candidate"]
    ops, b = _c_ops(oracle_c, sc), blocks(sc)
    assert [o for o in ops if o[0] == "C"][:2] == [("C", 3 * bs, bs), ("C", 2 * bs, bs)]
    assert b[3] == b[4] and len({adler(x) for x in (b[0], b[2], b[3])}) == 1 and len({b[0], b[2], b[3]}) == 3
    f3 = sc.src[2 + bs:2 + 2 * bs]
    assert adler(f3) == adler(b[0]) and f3 not in b and ("D", 2 + bs, bs) in ops
    # overlap: the window at 0 has block 0's weak value, not its content; the hit starts d later
    for d in T.overlap_distances(bs):
        sc = by[f"overlap({d})"]
        ops, b = _c_ops(oracle_c, sc), blocks(sc)
        assert adler(sc.src[:bs]) == adler(b[0]) and sc.src[:bs] != b[0] and sc.src[d:d + bs] == b[1]
        assert ops == [("D", 0, d), ("C", bs, bs), ("C", 0, bs)]
    # ... and behind a literal run of bs + 37 bytes: the false window lies off the block grid
    for d in (1, 65, bs - 1):
        sc = by[f"overlap({bs + 37}+{d})"]
        ops, b, o = _c_ops(oracle_c, sc), blocks(sc), bs + 37
        assert adler(sc.src[o:o + bs]) == adler(b[0]) and sc.src[o:o + bs] != b[0] and sc.src[o + d:o + d + bs] == b[1]
        assert ops == [("D", 0, o + d), ("C", bs, bs), ("C", 0, bs)]
    # family: 24 candidates of one weak value, hits on the last, a middle and the first; F24 is Data
    sc = by["family"]
    ops, b = _c_ops(oracle_c, sc), blocks(sc)
    assert len(b) == 24 and len(set(b)) == 24 and len({adler(x) for x in b}) == 1
    f24 = sc.src[2 + bs:2 + 2 * bs]
    assert adler(f24) == adler(b[0]) and f24 not in b and ("D", 2 + bs, bs) in ops
    assert [o[1] // bs for o in ops if o[0] == "C"] == [23, 5, 0]
    # dup+collision: the lowest index among the blocks with the equal strong hash
    sc = by["dup+collision"]
    b = blocks(sc)
    assert b[0] == b[2] and b[1] == b[3] and len({adler(x) for x in b}) == 1
    assert [o[1] // bs for o in _c_ops(oracle_c, sc)] == [1, 4, 0]
    # tail: the twin's suffix has the last block's weak value and size, and gets no Copy
    for name, sc in by.items():
        if name.startswith("tail-t"):
            t = sc.last_size()
            ops = _c_ops(oracle_c, sc)
            assert adler(sc.src[-t:]) == adler(sc.basis[-t:])
            if name.startswith("tail-twin"):
                assert sc.src[-t:] != sc.basis[-t:] and [o for o in ops if o[0] == "C"] == [("C", 0, bs)]
            else:
                assert ops[-1] == ("C", 2 * bs, t)
    assert {sc.last_size() > 240 for n, sc in by.items() if n.startswith("tail-twin")} == {True, False}
    # synthetic-R6: a full window matched against the short last entry, no size check
    sc = by["synthetic-R6"]
    assert int(sc.sig[2][-1]) == 100 and int(sc.sig[0][-1]) == adler(sc.src[:bs])
    assert _c_ops(oracle_c, sc) == [("C", bs, 100), ("C", bs, 100), ("C", 0, bs)]
