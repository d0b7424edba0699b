"""The saturated corpus of tests/saturated_cases.py is what it claims (CPU, the C oracle alone).

tests/test_gpu_saturated.py compares the device with the oracle on this corpus; the comparison
says something only where the bytes reach the bounds of the deferred-modulo code and the hits
fall where an accumulated error would lose them.  So, per family and pair:

(1) the largest 64-byte stripe sum (16 320) and in-stripe weighted sum (514 080) are reached;
    the mixed family {0xFD, 0xFE, 0xFF} comes within 1 % of both, the striped family swings by
    a whole stripe (less its marker byte) in both directions between neighbours;
(2) the oracle's op list holds Copies of whole blocks, at source positions off the block grid,
    on the first, a middle and the last position of the rolling run of the kernel the pair is
    for (kScanRun, a lane's 64 positions, kWRun: read back from the kernel sources here);
(3) every byte of the source that came from the basis is a Copy byte, whole block by whole
    block and the partial last block by the tail rule: only the junk is literal (the density
    floor: a condition on the pairs, met by the oracle alone);
(4) the oracle's ops rebuild the source.

It also checks the oracle itself where the device is compared with it above 128 KiB: its
Adler-32 against the closed form of a constant block at the block sizes on either side of the
two 32-bit overflows of the row layout, and its rolling update against a fresh hash there.
"""
import os
import re
import time

import numpy as np
import pytest

import saturated_cases as S
from oracle import oracle as O

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sy_amd", "csrc")
MOD = 65521


def _ops(oracle_c, basis, src, bs):
    w, s, z = oracle_c.compute_checksums(basis, bs)
    return O.ops_from_arrays(*oracle_c.generate_delta(src, w, s, z, bs))


def _check_pair(oracle_c, basis, src, bs, run, rel, per_target=1):
    ops = _ops(oracle_c, basis, src, bs)
    got = S.copies_by_run_position(ops, bs, run, rel)
    assert all(v >= per_target for v in got.values()), (bs, run, rel, got)
    nfull = len(basis) // bs
    copies = [o for o in ops if o[0] == "C"]
    assert sum(1 for o in copies if o[2] == bs) >= nfull, (bs, len(copies), nfull)
    assert sum(o[2] for o in copies) == len(basis) and sum(o[2] for o in ops) == len(src)
    if len(basis) % bs:
        assert ops[-1][0] == "C" and ops[-1][2] == len(basis) % bs  # the tail rule
    assert O.py_apply_delta(basis, src, ops) == src
    return got


def test_run_lengths_match_the_kernels():
    kern = open(os.path.join(CSRC, "sydelta_kernels.hip")).read()
    walk = open(os.path.join(CSRC, "sydelta_filewalk.hip")).read()

    def const(text, name):
        return int(re.search(r"constexpr \w+ %s = (\d+);" % name, text).group(1))

    assert const(kern, "kScanRun") == S.RUN_SCAN
    assert const(kern, "kR2") == S.RUN_LANE           # k_scan_lds: positions per thread
    assert const(kern, "kWTR") // 64 == S.RUN_LANE    # k_scan_r, k_scan_g: a wave tile's positions per lane
    assert const(walk, "kWRun") == S.RUN_WALK


@pytest.mark.parametrize("family", S.FAMILY_NAMES)
def test_family_reaches_the_bounds(family):
    data = S.family_bytes(family, 1 << 20)
    assert data == S.family_bytes.__wrapped__(family, 1 << 20)  # seeded: the same bytes every time
    assert not set(data) & set(S.JUNK)
    ssum, wsum = S.stripe_sums(data)
    print(family, int(ssum.max()), int(wsum.max()), float(np.frombuffer(data, np.uint8).mean()))
    if family == "fdff":
        assert 0.99 * S.STRIPE_SUM_MAX <= ssum.max() <= S.STRIPE_SUM_MAX
        assert 0.99 * S.STRIPE_WSUM_MAX <= wsum.max() <= S.STRIPE_WSUM_MAX
        assert ssum.min() >= 0.99 * S.STRIPE_SUM_MAX  # every stripe, not only the best
    else:
        assert ssum.max() == S.STRIPE_SUM_MAX and wsum.max() == S.STRIPE_WSUM_MAX
    if family == "stripes":
        d = np.diff(ssum)
        assert d.max() >= S.STRIPE_SUM_MAX - 0xF0 and d.min() <= -(S.STRIPE_SUM_MAX - 0xF0)
    if family == "ramp":
        # a stripe that is 0xFF from offset k on has weighted sum 255 * (2016 - k (k - 1) / 2):
        # the weight of the mean byte sits above the stripe's middle
        part = ssum < S.STRIPE_SUM_MAX
        assert part.any() and (wsum[part] * 2 > ssum[part] * 63).all()
    if family != "ff":
        blocks = {data[i:i + 256] for i in range(0, len(data) - 255, 256)}
        assert len(blocks) > 0.9 * (len(data) // 256), "blocks are distinct"


@pytest.mark.parametrize("case", S.SCAN_CASES, ids=lambda c: c[0])
def test_scan_pairs_place_the_copies(case, oracle_c):
    _, _, bs, run, _ = case
    assert set(S.scan_families(bs)) >= set(S.FAMILY_NAMES) - {"ff"}
    for family in S.scan_families(bs):
        basis, src = S.pair(family, bs, run)
        assert len(basis) <= 4 << 20 and len(src) <= 4 << 20
        # a block size that is a multiple of the run keeps a whole run of blocks on its target
        _check_pair(oracle_c, basis, src, bs, run, False, per_target=2 if bs % run == 0 else 1)


@pytest.mark.parametrize("bs", S.WALK_BLOCK_SIZES)
def test_walk_pairs_place_the_copies(bs, oracle_c):
    pairs = S.walk_pairs(bs)
    assert len(pairs) == 40 and {len(b) % bs != 0 for b, _ in pairs} == {True}
    for basis, src in pairs:
        _check_pair(oracle_c, basis, src, bs, S.RUN_WALK, True)


def test_chunk_pair_places_the_copies(oracle_c):
    basis, src = S.chunk_pair()
    assert len(basis) // (S.CHUNK_BS * S.CHUNK_SEG) >= 512 and len(src) <= 16 << 20
    got = _check_pair(oracle_c, basis, src, S.CHUNK_BS, S.RUN_WALK, True, per_target=30)
    assert sum(got.values()) == 90


def _adler_constant(byte, n):
    """Adler-32 of n bytes of one value, in closed form: A = 1 + n x, B = n + x n (n + 1) / 2."""
    return (((n + byte * n * (n + 1) // 2) % MOD) << 16) | ((1 + n * byte) % MOD)


@pytest.mark.parametrize("bs", [131072, 2245696, 2245760, 16843008, 16843072])
def test_oracle_exact_above_128k(bs, oracle_c):
    """The oracle reduces after every byte, so no block size overflows it; 17 MB take well
    under a second."""
    t0 = time.perf_counter()
    block = np.full(bs, 0xFF, np.uint8)
    assert oracle_c.adler32(block) == _adler_constant(0xFF, bs)
    block[:] = 0xFD
    assert oracle_c.adler32(block) == _adler_constant(0xFD, bs)
    w, s, z = oracle_c.compute_checksums(np.full(2 * bs + bs // 3, 0xFF, np.uint8), bs)
    assert w.tolist() == [_adler_constant(0xFF, bs)] * 2 + [_adler_constant(0xFF, bs // 3)]
    assert z.tolist() == [bs, bs, bs // 3] and s[0] == s[1] == oracle_c.xxh3(np.full(bs, 0xFF, np.uint8))
    print(bs, f"{time.perf_counter() - t0:.2f} s")


def test_oracle_match_exact_at_2245760(oracle_c):
    """generator.rs rolls in u32 with n * old: exact while 255 n < 2^32 (n <= 16 843 009).  At
    n = 2 245 760 a shifted source is all Copy after its prefix, so every roll agreed with the
    fresh hashes of the signature."""
    bs = 2245760
    basis = S.family_bytes("fdff", 3 * bs, 3)
    w, s, z = oracle_c.compute_checksums(basis, bs)
    for src in (basis, b"12345" + basis):
        ops = O.ops_from_arrays(*oracle_c.generate_delta(src, w, s, z, bs))
        pre = len(src) - len(basis)
        assert ops == ([("D", 0, pre)] if pre else []) + [("C", k * bs, bs) for k in range(3)]


def test_row_layout_cap():
    """A lane of the row layout adds at most 4 x 30 600 to its 32-bit weighted sum per 1 KiB
    piece (0xFF bytes): 35 089 pieces are the most that stay below 2^32."""
    cap = S.row_hash_max_n()
    assert cap == 35089 * 1024 and cap % 64 == 0
    per_piece = 4 * 255 * sum(range(16))
    assert per_piece * (cap // 1024) < 2 ** 32 <= per_piece * (cap // 1024 + 1)
    # the row totals that the 32-bit form of the sums lost: the first block sizes past 2^32
    assert 255 * 120 * (2245696 // 16) < 2 ** 32 <= 255 * 120 * (2245760 // 16)
    assert 255 * 16843008 < 2 ** 32 <= 1 + 255 * 16843072
