"""Local transport on the device: k_block_cmp against the
oracle's block-compare loop (local.rs:541-619) and the device change-ratio estimate
(k_hash_blocks, ratio.rs:78-192) against the oracle, on ratio.rs's own test files and
on seeded inputs with misaligned buffers, block sizes not a multiple of 16, short
(<= 240-byte) blocks, unequal lengths, one large case checked by properties, and constructed
cases with one changed byte at every loop position of k_block_cmp and of a sampled block."""
import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

MiB = 1 << 20
BS = 64 * 1024


def _dev(b, shift=0):
    import torch

    t = torch.zeros(len(b) + shift + 1, dtype=torch.uint8, device="cuda")
    if len(b):
        t[shift:shift + len(b)] = torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    return t[shift:shift + len(b)]


def _cases():
    rng = np.random.default_rng(11)
    base = rng.integers(0, 256, 3 * MiB + 12345, dtype=np.uint8).tobytes()
    yield "same", base, base, BS
    edited = bytearray(base)
    for p in rng.integers(0, len(base), 40):
        edited[p] ^= 0x5A
    yield "edits", bytes(edited), base, BS
    yield "src-longer", base, base[:2 * MiB + 17], BS
    yield "dst-longer", base[:MiB + 3], base, BS
    yield "odd-bs", bytes(edited), base, 1000 + 7
    yield "short-blocks", bytes(edited[:200000]), base[:200000], 240
    yield "tiny-blocks", bytes(edited[:50000]), base[:50000], 13
    yield "empty-src", b"", base[:1000], BS
    yield "empty-dst", base[:1000], b"", BS


CASES = list(_cases())


@pytest.mark.parametrize("shift", [0, 1, 4])
@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_block_compare_matches_oracle(case, shift, gpu):
    name, src, dst, bs = case
    flags, changed, lit, written = O.py_block_compare(src, dst, bs)
    got, st = gpu.block_compare(_dev(src, shift), _dev(dst), bs)
    assert got.cpu().tolist() == flags
    assert st == {"blocks": len(flags), "changed_blocks": changed, "literal_bytes": lit, "bytes_written": written}


@pytest.mark.parametrize("sample_count,threshold", [(None, None), (5, None), (1, 0.5), (0, None), (64, 0.1)])
@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_change_ratio_matches_oracle(case, sample_count, threshold, gpu):
    name, src, dst, bs = case
    r, sampled, changed, use, thr = O.py_estimate_change_ratio(src, dst, bs, sample_count, threshold)
    got = gpu.estimate_change_ratio(_dev(src, 1), _dev(dst), bs, sample_count, threshold)
    assert got == {"change_ratio": r, "blocks_sampled": sampled, "blocks_changed": changed, "use_delta": use,
                   "threshold": thr}


@pytest.mark.parametrize("name", ["same", "all_changed", "partial", "threshold", "size"])
def test_change_ratio_reference_files(name, gpu):
    # The files of ratio.rs:200-307.
    src = bytearray(b"\x2a" * MiB)
    dst = bytes(b"\x2a" * MiB)
    if name == "all_changed":
        dst = b"\x63" * MiB
    elif name == "partial":
        src[:256 * 1024] = b"\x63" * (256 * 1024)
    elif name == "threshold":
        src[:800 * 1024] = b"\x63" * (800 * 1024)
    elif name == "size":
        src = bytearray(b"\x2a" * (2 * MiB))
    got = gpu.estimate_change_ratio(_dev(bytes(src)), _dev(dst), BS)
    exp = O.py_estimate_change_ratio(bytes(src), dst, BS)
    assert (got["change_ratio"], got["blocks_sampled"], got["blocks_changed"], got["use_delta"]) == exp[:4]
    if name == "threshold":
        assert not got["use_delta"]
        assert gpu.estimate_change_ratio(_dev(bytes(src)), _dev(dst), BS, threshold=0.90)["use_delta"]


def test_block_compare_large_properties(gpu):
    # 1 GiB: flags equal a torch reduction over the reshaped block view, and exactly
    # the edited blocks are flagged.
    import torch

    n, bs = 1 << 30, BS
    src = torch.empty(n, dtype=torch.uint8, device="cuda")
    gpu.synth_fill(src, seed=5)
    dst = src.clone()
    g = torch.Generator().manual_seed(3)
    pos = torch.randint(0, n, (500,), generator=g)
    dst[pos.cuda()] ^= 1
    got, st = gpu.block_compare(src, dst, bs)
    exp = torch.zeros(n // bs, dtype=torch.uint8)
    exp[torch.unique(pos // bs)] = 1
    assert torch.equal(got.cpu(), exp)
    assert st["changed_blocks"] == int(exp.sum()) and st["literal_bytes"] == int(exp.sum()) * bs
    assert st["bytes_written"] == n


@pytest.mark.parametrize("sample_count,threshold", [(None, None), (5, None), (1, 0.5), (0, None), (1000, 0.1)])
@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_change_ratio_paths_match_oracle(case, sample_count, threshold, tmp_path):
    """The path-level estimate_change_ratio (files read on the host, sampled blocks
    hashed on the device) against the oracle on the same bytes."""
    from sy_amd import delta

    name, src, dst, bs = case
    ps, pd = tmp_path / "source.bin", tmp_path / "dest.bin"
    ps.write_bytes(src)
    pd.write_bytes(dst)
    r, sampled, changed, use, thr = O.py_estimate_change_ratio(src, dst, bs, sample_count, threshold)
    got = delta.estimate_change_ratio(ps, pd, bs, sample_count, threshold)
    assert (got.change_ratio, got.blocks_sampled, got.blocks_changed, got.use_delta, got.threshold) == \
        (r, sampled, changed, use, thr)


@pytest.mark.parametrize("name", ["same", "all_changed", "partial", "threshold", "size", "small_sample"])
def test_change_ratio_paths_reference_tests(name, tmp_path):
    """ratio.rs:199-325, the reference's own tests, through the path API."""
    from sy_amd import delta

    src = bytearray(b"\x2a" * MiB)
    dst = bytes(b"\x2a" * MiB)
    if name == "all_changed":
        dst = b"\x63" * MiB
    elif name == "partial":
        src[:256 * 1024] = b"\x63" * (256 * 1024)
    elif name == "threshold":
        src[:800 * 1024] = b"\x63" * (800 * 1024)
    elif name == "size":
        src = bytearray(b"\x2a" * (2 * MiB))
    ps, pd = tmp_path / "source.bin", tmp_path / "dest.bin"
    ps.write_bytes(bytes(src))
    pd.write_bytes(dst)
    r = delta.estimate_change_ratio(ps, pd, BS, 5 if name == "small_sample" else None)
    if name in ("same", "small_sample"):
        assert r.blocks_changed == 0 and r.change_ratio == 0.0 and r.use_delta
        assert r.blocks_sampled == (5 if name == "small_sample" else 16)
    elif name == "all_changed":
        assert r.blocks_changed == r.blocks_sampled and r.change_ratio == 1.0 and not r.use_delta
    elif name == "partial":
        assert 0 < r.blocks_changed < r.blocks_sampled and 0.0 < r.change_ratio < 1.0 and r.use_delta
    elif name == "threshold":
        assert not r.use_delta
        assert delta.estimate_change_ratio(ps, pd, BS, threshold=0.90).use_delta
    else:
        assert not r.use_delta


@pytest.mark.late
def test_change_ratio_paths_large_sample(tmp_path, gpu):
    """More samples than one 64 MiB batch: 300 MiB files, 64 KiB blocks, every block
    sampled, edits in 37 of them."""
    from sy_amd import delta

    n = 300 * MiB
    base = O.synth_bytes(n, 21)
    ed = base.copy()
    rng = np.random.default_rng(4)
    blocks = rng.choice(n // BS, 37, replace=False)
    ed[blocks * BS + 17] ^= 0x11
    ps, pd = tmp_path / "source.bin", tmp_path / "dest.bin"
    ed.tofile(ps)
    base.tofile(pd)
    r = delta.estimate_change_ratio(ps, pd, BS, sample_count=n // BS)
    exp = O.py_estimate_change_ratio(ed.tobytes(), base.tobytes(), BS, n // BS)
    assert (r.change_ratio, r.blocks_sampled, r.blocks_changed, r.use_delta) == exp[:4]
    assert r.blocks_changed == 37


# ---------------------------------------------------------------------------
# k_block_cmp returns one bit per block: every byte position must be able to set it.
# The constructed cases change one byte (bit 0 or bit 7 of it) in every even block and none in
# the odd ones, so the flags alternate 1, 0; each case checks the oracle's flags against that
# pattern as well as the device's.
# ---------------------------------------------------------------------------
VBS = 16 * 1283  # 20528: per lane one round of the 4x-unrolled loop (vectors 0-1023), then the
#                  remainder loop twice (vectors 1024-1279, 1280-1282)
# in-block offsets: the first and last byte of a vector and of the block; lane 255 and lane 0 of
# the unrolled slots u = 0-3; the remainder loop's first and last vector and its second round;
# the four dwords of a vector of the unrolled loop (600) and of the remainder loop (1100)
VPOS = [0, 15, 16, 16 * 255 + 7, 16 * 256, 16 * 512 + 3, 16 * 768, 16 * 1023 + 15, 16 * 1024, 16 * 1279 + 8,
        16 * 1280, VBS - 1] + [16 * v + d for v in (600, 1100) for d in (0, 4, 8, 12)]
_CMP_BASE = np.random.default_rng(23).integers(0, 256, 2 * len(VPOS) * VBS + VBS, dtype=np.uint8)


def _flip(buf, at, bit):
    out = buf.copy()
    out[at] ^= 1 << bit
    return out


def _check_flags(gpu, src, dst, bs, want, sshift=0, dshift=0, oracle=True):
    src, dst = bytes(src), bytes(dst)
    nb = -(-len(src) // bs)
    want = np.asarray(want, dtype=np.uint8)
    assert want.shape == (nb,)
    if oracle:  # the oracle's loop must say the same as the construction
        flags, changed, lit, written = O.py_block_compare(src, dst, bs)
        assert flags == want.tolist()
    sizes = np.minimum(bs, len(src) - np.arange(nb, dtype=np.int64) * bs)
    got, st = gpu.block_compare(_dev(src, sshift), _dev(dst, dshift), bs)
    got = got.cpu().numpy()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (bad[:10].tolist(), got[bad[:10]].tolist())
    assert st == {"blocks": nb, "changed_blocks": int(want.sum()), "literal_bytes": int(sizes[want != 0].sum()),
                  "bytes_written": len(src)}


def _even_blocks_changed(base, bs, pos, bit):
    """dst = base with byte pos[j] of block 2j changed; the flags alternate 1, 0."""
    at = np.array([2 * j * bs + p for j, p in enumerate(pos)])
    assert at.max() < len(base)
    return _flip(base, at, bit), [1, 0] * len(pos)


@pytest.mark.parametrize("bit", [0, 7])
@pytest.mark.parametrize("sshift,dshift", [(0, 0), (16, 32)])
def test_block_compare_vector_path_positions(sshift, dshift, bit, gpu):
    src = _CMP_BASE[:2 * len(VPOS) * VBS]
    dst, want = _even_blocks_changed(src, VBS, VPOS, bit)
    _check_flags(gpu, src, dst, VBS, want, sshift, dshift)


@pytest.mark.parametrize("bit", [0, 7])
@pytest.mark.parametrize("where", ["first-tail-byte", "last-byte", "neither"])
def test_block_compare_byte_tail(where, bit, gpu):
    """A last block of 16 * 5 + 9 bytes in both files: five vectors and a tail of nine bytes."""
    n = 4 * VBS + 16 * 5 + 9
    src = _CMP_BASE[:n]
    dst, want = _even_blocks_changed(src, VBS, [16 * 1279 + 8, VBS - 1], bit)
    if where != "neither":
        dst[4 * VBS + 80 if where == "first-tail-byte" else n - 1] ^= 1 << bit
    _check_flags(gpu, src, dst, VBS, want + [0 if where == "neither" else 1])


@pytest.mark.parametrize("case", ["dst-1", "dst+1", "dst+1-full", "dst-2-blocks-3"])
def test_block_compare_unequal_lengths(case, gpu):
    """Equal bytes, unequal lengths: a block differs when its two reads differ in length."""
    base = _CMP_BASE[:5 * VBS + 100]
    if case == "dst-1":
        _check_flags(gpu, base, base[:-1], VBS, [0, 0, 0, 0, 0, 1])
        _check_flags(gpu, base[:5 * VBS], base[:5 * VBS - 1], VBS, [0, 0, 0, 0, 1])
    elif case == "dst+1":
        _check_flags(gpu, base[:-1], base, VBS, [0, 0, 0, 0, 0, 1])
    elif case == "dst+1-full":  # the source ends with a block: the longer destination changes nothing
        _check_flags(gpu, base[:5 * VBS], base[:5 * VBS + 1], VBS, [0, 0, 0, 0, 0])
    else:  # 3 * VBS + 97 bytes: block 3 is short in dst, blocks 4 and 5 are missing
        _check_flags(gpu, base, base[:len(base) - 2 * VBS - 3], VBS, [0, 0, 0, 1, 1, 1])


@pytest.mark.parametrize("bit", [0, 7])
@pytest.mark.parametrize("bs,sshift,dshift", [(1007, 0, 0), (1007, 1, 0), (1007, 0, 1), (1007, 1, 1),
                                              (4096, 1, 0), (4096, 0, 1), (4096, 1, 1)])
def test_block_compare_byte_path_positions(bs, sshift, dshift, bit, gpu):
    """Blocks off a 16-byte boundary take the byte loop: 256 lanes, so offsets 255 | 256 and
    511 are a lane's first and second round.  (bs = 1007 unshifted: blocks 0 and 16 are aligned
    and take the vector path with a 15-byte tail.)"""
    pos = [0, 255, 256, 511, bs - 1]
    if bs == 1007:
        pos += [bs - 1] * 4  # block 16: the last byte of the 15-byte tail of an aligned block
    src = _CMP_BASE[:2 * len(pos) * bs]
    dst, want = _even_blocks_changed(src, bs, pos, bit)
    _check_flags(gpu, src, dst, bs, want, sshift, dshift)


@pytest.mark.parametrize("bit", [0, 7])
def test_block_compare_grid_stride(bit, gpu):
    """More blocks than the grid's 2^20 workgroups: blocks 2^20 and up are a workgroup's second."""
    bs, n = 2, 2 * ((1 << 20) + 6) + 1
    src = np.resize(_CMP_BASE, n)
    blocks = np.array([0, (1 << 20) - 1, 1 << 20, (1 << 20) + 5, (1 << 20) + 6])
    dst = _flip(src, blocks * bs + np.array([0, 1, 1, 0, 0]), bit)
    want = np.zeros((1 << 20) + 7, dtype=np.uint8)
    want[blocks] = 1
    _check_flags(gpu, src, dst, bs, want, oracle=False)  # the expected flags are the construction


@pytest.mark.parametrize("nblocks", [20, 40])
@pytest.mark.parametrize("bs", [240, 241, 1000, 65536])
def test_change_ratio_sees_one_byte_of_a_sampled_block(bs, nblocks, gpu):
    """Default sampling (20 samples).  Of 20 blocks every one is sampled (step 20 // 19 = 1), so
    a byte anywhere counts; of 40 blocks the even ones are (step 2), so the odd ones and the last
    block are the unsampled blocks a byte must not count in.  bs 240 | 241: k_hash_blocks' short
    and long form."""
    src = np.resize(_CMP_BASE, nblocks * bs)
    dsrc = _dev(bytes(src), 1)

    def changed(dst):
        exp = O.py_estimate_change_ratio(bytes(src), bytes(dst), bs)
        got = gpu.estimate_change_ratio(dsrc, _dev(bytes(dst)), bs)
        assert got == {"change_ratio": exp[0], "blocks_sampled": exp[1], "blocks_changed": exp[2],
                       "use_delta": exp[3], "threshold": exp[4]}
        assert got["blocks_sampled"] == 20
        return got["blocks_changed"]

    assert changed(src) == 0
    step = nblocks // 19
    sampled = [0, 9 * step, 19 * step]
    for k in sampled:
        for p in (0, bs // 2, bs - 1):
            assert changed(_flip(src, k * bs + p, 0)) == 1, (k, p)
    assert changed(_flip(src, np.array([k * bs + bs - 1 for k in sampled]), 7)) == 3
    if nblocks == 40:
        for k in (1, 21, 39):
            for p in (0, bs // 2, bs - 1):
                assert changed(_flip(src, k * bs + p, 0)) == 0, (k, p)
