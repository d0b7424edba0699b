"""Whole-file XXH3-64 on the device (k_xxh_pieces + k_xxh_chain) against the oracle's
hash_file (integrity/xxhash3.rs:17-33): every XXH3 length class, block/stripe edges,
unaligned file starts, batches whose chains are ragged within a wave, one 1 GiB
file (a 1 Mi-step scramble chain), and the kernels' own edges: the chain's rounds of 64 steps,
waves that mix chain lengths, the table search at one to four rounds, load16u's alignment
classes and a file that ends with the tensor."""
import random

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 3, 4, 8, 9, 16, 17, 100, 128, 129, 200, 240, 241, 255, 256, 1023, 1024, 1025, 1087, 1088, 1089,
         1100, 2047, 2048, 2049, 4096, 33 * 1024 + 5, 64 * 1024, 65 * 1024 + 63, (1 << 20) + 1, (3 << 20) + 777]


def _dev(b: bytes, shift: int = 0):
    import torch

    t = torch.zeros(len(b) + shift + 64, dtype=torch.uint8, device="cuda")
    if b:
        t[shift:shift + len(b)] = torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    return t[shift:shift + len(b)]


@pytest.mark.parametrize("shift", [0, 1, 5, 16])
@pytest.mark.parametrize("n", SIZES)
def test_single_file(n, shift, gpu):
    data = random.Random(n * 7 + shift).randbytes(n)
    assert gpu.xxh3(_dev(data, shift)) == O.py_hash_file(data)


def ragged_lens(seed, rng=None):
    """The lengths of test_batch_ragged(seed) (tests/test_xxh_scratch_host.py checks the scratch
    bound on the same batches)."""
    rng = rng or random.Random(seed)
    return [rng.choice([0, 5, 17, 200, 241, 1500, 70000, 130 * 1024 + 3, 300000, 1 << 20]) + rng.randrange(0, 64)
            for _ in range(37)]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_batch_ragged(seed, gpu):
    import torch

    rng = random.Random(seed)
    lens = ragged_lens(seed, rng)
    offs, pos = [], 0
    for ln in lens:
        pos += rng.randrange(0, 19)  # arbitrary (unaligned) file starts
        offs.append(pos)
        pos += ln
    blob = rng.randbytes(pos + 64)
    buf = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
    got = gpu.xxh3_batch(buf, offs, lens)
    exp = [O.py_hash_file(blob[o:o + ln]) for o, ln in zip(offs, lens)]
    assert [int(x) for x in got] == exp


def test_batch_rejects_out_of_range(gpu):
    import torch

    buf = torch.zeros(1000, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        gpu.xxh3_batch(buf, [990], [20])

    from sy_amd._lib import lib

    offs = np.array([990], dtype=np.uint64)
    lens = np.array([20], dtype=np.uint64)
    out = np.zeros(1, dtype=np.uint64)
    rc = lib.sydelta_xxh3_batch_device(0, buf.data_ptr(), 1000, offs.ctypes.data, lens.ctypes.data, 1, None,
                                       out.ctypes.data)
    assert rc != 0 and b"outside" in lib.sydelta_last_error()


def test_one_gib(gpu):
    import torch

    n = (1 << 30) + 12345
    buf = torch.empty(n, dtype=torch.uint8, device="cuda")
    gpu.synth_fill(buf, seed=21)
    host = buf.cpu().numpy().tobytes()
    assert gpu.xxh3(buf) == O.py_xxh3(host)


# ---------------------------------------------------------------------------
# K9 at its edges.  k_xxh_chain keeps two register batches of 32 steps: a round of 64 in the
# "every chain of the wave runs" loop (up to the wave's shortest chain, nmin) and in the
# ragged loop (up to its longest, nmax).  A file of (s + 1) * 1024 + r bytes, 1 <= r <= 1024,
# has s + 1 full blocks and a chain of s steps; r = 1024 is the full last KiB that XXH3 still
# hashes as the partial block (15 tail stripes and the last stripe).
# ---------------------------------------------------------------------------
KIB = 1024
STEP_EDGES = [0, 1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 191, 192, 193]
TAILS = [1, 64, 65, 1023, 1024]
_EDGE_BLOB = random.Random(0x9A).randbytes(196 * KIB)


@pytest.mark.parametrize("shift", [0, 3])
@pytest.mark.parametrize("s", STEP_EDGES)
def test_chain_step_edges(s, shift, gpu):
    for r in TAILS:
        n = (s + 1) * KIB + r
        data = _EDGE_BLOB[7 * r % 256:][:n]
        assert len(data) == n
        assert gpu.xxh3(_dev(data, shift)) == O.py_hash_file(data), (s, r)


def _check_batch(gpu, lens, seed, tail=64):
    """Files of the given lengths with gaps of 0-18 bytes in one tensor of random bytes that ends
    `tail` bytes after the last file; every device hash against the oracle's."""
    import torch

    rng = random.Random(seed)
    offs, pos = [], 0
    for ln in lens:
        pos += rng.randrange(0, 19)
        offs.append(pos)
        pos += ln
    blob = rng.randbytes(pos + tail)
    buf = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
    got = gpu.xxh3_batch(buf, offs, lens)
    exp = [O.py_hash_file(blob[o:o + ln]) for o, ln in zip(offs, lens)]
    bad = [(f, lens[f]) for f in range(len(lens)) if int(got[f]) != exp[f]]
    assert not bad, bad[:10]


def _steps_len(steps, r):
    return 200 if steps is None else (steps + 1) * KIB + r


_WAVE = [193, 129, 128, 127, 65, 64, 63, None]  # chain steps; None: a 200-byte file, no block


def _mixed_waves():
    one = [_steps_len(s, TAILS[i % 5]) for i, s in enumerate(_WAVE)]
    yield "short-last", one                  # the short files have the highest fpfx
    yield "short-first", one[::-1]
    sixteen = [_steps_len(s, TAILS[(i + 2) % 5]) for i, s in enumerate(_WAVE + [192, 130, 126, 97, 66, 62, 1, 0])]
    yield "two-waves", sixteen
    twenty = sixteen + [_steps_len(s, r) for s, r in [(191, 1024), (64, 1), (None, 0), (0, 1024)]]
    yield "inactive-groups", twenty          # 8 + 8 + 4: the last wave has four idle groups
    yield "long-short", [1 << 20, 5]
    yield "short-long", [5, 1 << 20]
    for name, lens in [("one-wave", one), ("two-waves", sixteen), ("inactive-groups", twenty)]:
        lens = list(lens)
        random.Random(len(lens)).shuffle(lens)  # `order` is not the identity
        yield name + "-shuffled", lens


@pytest.mark.parametrize("case", list(_mixed_waves()), ids=lambda c: c[0])
def test_waves_that_mix_chain_lengths(case, gpu):
    name, lens = case
    assert max(lens) <= 1 << 20
    _check_batch(gpu, lens, seed=len(lens) * 31 + len(name))


def _table_lens(nfull, seed, hi):
    """nfull files with at least one full block, mostly one block (1025..hi bytes) with a
    two- or three-block file every 16th, and a file of <= 240 bytes (in `order`, absent from
    phase A's table) after every fourth."""
    rng = np.random.default_rng(seed)
    full = rng.integers(1025, hi + 1, nfull)
    full[0], full[1 % nfull] = 1025, 2048
    multi = np.arange(5, nfull, 16)
    full[multi] = rng.integers(2049, 4097, len(multi))
    nsmall = nfull // 4 + 1
    lens = np.empty(nfull + nsmall, dtype=np.int64)
    small_at = np.zeros(nfull + nsmall, dtype=bool)
    small_at[rng.choice(nfull + nsmall, nsmall, replace=False)] = True
    lens[~small_at] = full
    lens[small_at] = rng.choice([0, 1, 16, 129, 200, 240], nsmall)
    return lens


@pytest.mark.parametrize("nfull,hi", [(63, 2048), (64, 2048), (65, 2048), (4095, 2048), (4096, 2048), (4097, 2048),
                                      (262200, 1100)])
def test_table_search_depth(nfull, hi, gpu):
    """k_xxh_pieces finds a wave's file by a 64-way search over the files with a full block:
    one round up to 64 of them, two up to 4096, three up to 262144, then four."""
    import torch

    lens = _table_lens(nfull, nfull, hi)
    assert int(((lens > 240) & ((lens - 1) >> 10 > 0)).sum()) == nfull
    rng = np.random.default_rng(nfull + 1)
    gaps = rng.integers(0, 19, len(lens))
    offs = np.cumsum(gaps) + np.concatenate([[0], np.cumsum(lens)[:-1]])
    total = int(offs[-1] + lens[-1])
    buf = torch.empty(total, dtype=torch.uint8, device="cuda")
    gpu.synth_fill(buf, seed=nfull)
    got = gpu.xxh3_batch(buf, offs, lens)
    host = memoryview(buf.cpu().numpy())
    exp = np.fromiter((O.py_hash_file(host[o:o + n]) for o, n in zip(offs.tolist(), lens.tolist())),
                      dtype=np.uint64, count=len(lens))
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, (bad[:10].tolist(), lens[bad[:10]].tolist())


@pytest.mark.parametrize("shift", [2, 3, 4, 8, 12, 15])
def test_three_blocks_at_every_alignment_class(shift, gpu):
    """load16u: 16-aligned, 4-aligned but not 16-aligned (no fifth dword), and the byte shifts."""
    for n in (3 * KIB + 1, 3 * KIB + 700, 4 * KIB):
        data = _EDGE_BLOB[shift:shift + n]
        assert gpu.xxh3(_dev(data, shift)) == O.py_hash_file(data), n


@pytest.mark.parametrize("lead", [0, 1, 4, 13])
def test_last_file_ends_on_the_last_byte(lead, gpu):
    """No byte behind the last file: its last stripe and its two blocks end with the tensor."""
    _check_batch(gpu, [lead, 1500, 100, 3 * KIB + 5, 2049], seed=40 + lead, tail=0)
