"""BLAKE3-256 on the device (k_b3_chunks + k_b3_tree) against the from-specification
reference of tests/blake3_ref.py: block and chunk edges, tail blocks, one wave of chunks and
the launches above it, unaligned file starts, ragged batches, batches whose files share
waves (every chunk count from 1 to 66; level-1 nodes packed one launch up), pieces of a sharded file
joined on the host, a caller's stream, and the streamed path API."""
import random

import numpy as np
import pytest

import blake3_ref as R

pytestmark = pytest.mark.gpu

KIB = 1024
SMALL = [0, 1, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2047, 2048, 2049, 3072, 3073, 4097, 5121, 7169, 8193,
         31744, 102400]
WAVE = [65535, 65536, 65537, 66560, 66561]  # around 64 chunks
LEVELS = [c * KIB + x for c in (127, 128, 129, 4095, 4096, 4097) for x in (0, 1)] + [(4 << 20) + 1025]
SIZES = SMALL + WAVE + LEVELS

_BLOB = random.Random(0xB3).randbytes(max(SIZES))
_expected = {}


def _data(n: int) -> bytes:
    return _BLOB[len(_BLOB) - n:] if n else b""


def _expect(n: int) -> bytes:
    if n not in _expected:
        _expected[n] = R.blake3(_data(n))
    return _expected[n]


def _dev(b: bytes, shift: int = 0):
    import torch

    t = torch.zeros(len(b) + shift + 64, dtype=torch.uint8, device="cuda")
    if b:
        t[shift:shift + len(b)] = torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    return t[shift:shift + len(b)]


@pytest.mark.parametrize("shift", [0, 1, 5, 16])
@pytest.mark.parametrize("n", SIZES)
def test_single_file(n, shift, gpu):
    assert gpu.blake3(_dev(_data(n), shift)) == _expect(n)


@pytest.mark.parametrize("n", sorted(R.VECTORS))
def test_published_vectors(n, gpu):
    assert gpu.blake3(_dev(R.pattern(n))).hex() == R.VECTORS[n]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_batch_ragged(seed, gpu):
    import torch

    rng = random.Random(seed)
    lens = [rng.choice([0, 5, 64, 1024, 1025, 1500, 70000, 130 * 1024 + 3, 300000, 1 << 20]) + rng.randrange(0, 64)
            for _ in range(37)]
    offs, pos = [], 0
    for ln in lens:
        pos += rng.randrange(0, 19)  # arbitrary (unaligned) file starts
        offs.append(pos)
        pos += ln
    blob = rng.randbytes(pos + 64)
    buf = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
    got = gpu.blake3_batch(buf, offs, lens)
    assert got.shape == (37, 32) and got.dtype == np.uint8
    for f, (o, ln) in enumerate(zip(offs, lens)):
        assert got[f].tobytes() == R.blake3(blob[o:o + ln]), (f, o, ln)


def test_batch_of_single_chunk_files(gpu):
    import torch

    rng = random.Random(7)
    lens = [rng.choice([0, 1, 63, 64, 65, 1000, 1023, 1024]) if f % 3 else rng.randrange(0, 1025) for f in range(200)]
    offs, pos = [], 0
    for ln in lens:
        pos += rng.randrange(0, 19)
        offs.append(pos)
        pos += ln
    blob = rng.randbytes(pos)
    buf = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
    got = gpu.blake3_batch(buf, offs, lens)
    for f, (o, ln) in enumerate(zip(offs, lens)):
        assert got[f].tobytes() == R.blake3(blob[o:o + ln]), (f, o, ln)


def _check_shared_waves(gpu, chunk_counts, seed):
    """A batch of files of the given chunk counts, file n of (n - 1) KiB + 1 B (n odd) or n KiB
    (n even) and always the same bytes, at unaligned starts with gaps of 0-18 bytes."""
    import torch

    rng = random.Random(seed)
    lens = [(n - 1) * KIB + (1 if n & 1 else KIB) for n in chunk_counts]
    offs, pos = [], 0
    for ln in lens:
        pos += rng.randrange(0, 19)
        offs.append(pos)
        pos += ln
    buf = torch.zeros(pos + 64, dtype=torch.uint8, device="cuda")
    for o, ln in zip(offs, lens):
        buf[o:o + ln] = torch.frombuffer(bytearray(_data(ln)), dtype=torch.uint8).cuda()
    got = gpu.blake3_batch(buf, offs, lens)
    bad = [(f, n) for f, n in enumerate(chunk_counts) if got[f].tobytes() != _expect(lens[f])]
    assert not bad, bad[:10]


@pytest.mark.parametrize("order", ["shuffled", "ascending", "descending"])
def test_batch_of_every_chunk_count_in_shared_waves(order, gpu):
    """Files of 3 to 64 chunks sit at power-of-two slots (seg_align) of waves they share with
    their neighbours, and wave_levels finds a node's sibling at lane ^ 2^l: every chunk count
    from 1 to 66, with different alignments side by side."""
    counts = list(range(1, 67))
    if order == "shuffled":
        random.Random(66).shuffle(counts)
    elif order == "descending":
        counts.reverse()
    _check_shared_waves(gpu, counts, seed=len(order))


def test_batch_packs_level_one_nodes(gpu):
    """The same packing one launch up: files of 65 to 4096 chunks leave 2 to 64 nodes that share
    a k_b3_tree wave (here 2, 2, 3, 4 and 33), between files that finished in the first launch;
    the file of 4097 chunks (65 nodes) alone needs a third launch."""
    _check_shared_waves(gpu, [65, 1, 128, 3, 129, 64, 193, 1, 2112, 3, 4097, 64, 3], seed=5)


def test_batch_rejects_out_of_range(gpu):
    import torch

    buf = torch.zeros(1000, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        gpu.blake3_batch(buf, [990], [20])

    from sy_amd._lib import lib

    offs = np.array([990], dtype=np.uint64)
    lens = np.array([20], dtype=np.uint64)
    out = np.zeros(32, dtype=np.uint8)
    rc = lib.sydelta_blake3_batch_device(0, buf.data_ptr(), 1000, offs.ctypes.data, lens.ctypes.data, 1, None,
                                         out.ctypes.data)
    assert rc != 0 and b"outside" in lib.sydelta_last_error()


@pytest.fixture(scope="module")
def sharded(gpu):
    """16 MiB + 777 B of synthetic bytes on the device, their reference hash and the device's."""
    import torch

    n = (16 << 20) + 777
    buf = torch.empty(n, dtype=torch.uint8, device="cuda")
    gpu.synth_fill(buf, seed=33)
    return buf, R.blake3(buf.cpu().numpy()), gpu.blake3(buf)


@pytest.mark.parametrize("piece", [1 << 20, 64 << 10])
def test_subtrees_joined(piece, sharded, gpu):
    from sy_amd import shard

    buf, ref, whole = sharded
    ps = R.pieces(buf.numel(), piece // KIB)
    cvs = [gpu.blake3_subtree(buf[o:o + ln], fc) for o, ln, fc, _ in ps]
    joined = shard.blake3_join(cvs, [c for *_, c in ps])
    assert joined == whole == ref


def test_subtree_uses_the_chunk_counter(sharded, gpu):
    from sy_amd import shard

    buf, ref, _ = sharded
    ps = R.pieces(buf.numel(), 1024)
    cvs = [gpu.blake3_subtree(buf[o:o + ln], fc) for o, ln, fc, _ in ps]
    o, ln, fc, _ = ps[3]
    assert gpu.blake3_subtree(buf[o:o + ln], fc) == cvs[3] == R.subtree_cv(buf[o:o + ln].cpu().numpy(), fc)
    moved = gpu.blake3_subtree(buf[o:o + ln], fc + 1)  # not a multiple of the piece's chunks
    assert moved != cvs[3] and moved == R.subtree_cv(buf[o:o + ln].cpu().numpy(), fc + 1)
    assert shard.blake3_join(cvs[:3] + [moved] + cvs[4:], [c for *_, c in ps]) != ref


def test_callers_stream(gpu):
    import torch

    n = 300 * KIB + 17
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        buf = _dev(_data(n), 3)
        got = gpu.blake3(buf, stream=s)
    assert got == R.blake3(_data(n))


def test_hash_data_and_hash_file(tmp_path, gpu):
    from sy_amd.delta import Blake3Hasher

    n = (3 << 20) + 5
    p = tmp_path / "f"
    p.write_bytes(_data(n))
    exp = R.blake3(_data(n))
    assert Blake3Hasher.hash_file(p) == exp
    assert Blake3Hasher.hash_data(_data(n)) == exp
    assert Blake3Hasher.hash_data(b"abc").hex() == R.ABC


@pytest.mark.late
def test_hash_file_in_pieces(tmp_path, gpu):
    """128 MiB + 1 KiB + 1 B: two full 64 MiB pieces and a tail of two chunks."""
    import torch

    from sy_amd.delta import Blake3Hasher

    n = (128 << 20) + KIB + 1
    buf = torch.empty(n, dtype=torch.uint8, device="cuda")
    gpu.synth_fill(buf, seed=44)
    host = buf.cpu().numpy()
    p = tmp_path / "big"
    host.tofile(p)
    exp = R.blake3(host)
    assert gpu.blake3(buf) == exp
    assert Blake3Hasher.hash_file(p) == exp


def test_kernels_show_in_the_profile(gpu):
    gpu.set_profiling(True)
    try:
        gpu.profile(reset=True)
        gpu.blake3(_dev(_data(102400)))
        prof = gpu.profile(reset=True)
    finally:
        gpu.set_profiling(False)
    assert prof["k_b3_chunks"]["count"] == 1
    assert prof["k_b3_tree"]["count"] == 1  # 100 chunks: two nodes above the waves
