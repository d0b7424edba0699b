"""GPU parity on the saturated corpus (tests/saturated_cases.py): bytes at the top of the range
the deferred-modulo bounds of the Adler code are written for, hits on the first, a middle and
the last position of each kernel's rolling run.  Op lists bit-exact against
oracle_c.generate_delta, signatures against oracle_c.compute_checksums; every case names the
kernel it is for and reads from gpu.profile that it ran.

Inside the production domain (block sizes up to 128 KiB): the five signature kernels, the four
scans with every position rolled (SYDELTA_PROBE=0), the aligned probe, k_verify_w on its row
and its wave path, the tail rule, K10 over a batch of small files and over a chunk
(k_preroll, k_chunk_write).

Above it: the signature, single and batched, at the block sizes on either side of the two
32-bit overflows that the row layout's row sums had (0xFF bytes: the weighted sum passes 2^32
between 2 245 696 and 2 245 760, the byte sum between 16 843 008 and 16 843 072; the weak hash
came out wrong there, silently), at the row layout's cap and behind it, and at 8 MiB of random
bytes; the match at 2 245 760 through k_scan_g and the probe, and the refusal of the route
whose launch cannot hold such a window (k_scan).
"""
import functools
import random

import numpy as np
import pytest

import saturated_cases as S
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SCAN_ENV = ("SYDELTA_SCAN_SMALL", "SYDELTA_SCAN_WIDE", "SYDELTA_PROBE", "SYDELTA_WDEF_CAP")


def _to_dev(data, shift: int = 0):
    """data on the device at `shift` bytes past an allocation's start, 16 readable bytes behind it."""
    import torch

    raw = torch.zeros(len(data) + shift + 16, dtype=torch.uint8, device="cuda")
    if len(data):
        raw[shift:shift + len(data)] = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    return raw[shift:shift + len(data)]


def _profiled(gpu, fn):
    import torch

    gpu.set_profiling(True)
    gpu.profile(reset=True)
    try:
        out = fn()
        torch.cuda.synchronize()
        return out, gpu.profile(reset=True)
    finally:
        gpu.set_profiling(False)


def _sig_lists(w, s):
    return w.cpu().numpy().view(np.uint32).tolist(), s.cpu().numpy().view(np.uint64).tolist()


@functools.lru_cache(None)
def _oracle_sig(data: bytes, bs: int):
    w, s, _ = O.C().compute_checksums(data, bs, threads=8)
    return w.tolist(), s.tolist()


@functools.lru_cache(None)
def _oracle_ops(basis: bytes, src: bytes, bs: int):
    C = O.C()
    w, s, z = C.compute_checksums(basis, bs, threads=8)
    return O.ops_from_arrays(*C.generate_delta(src, w, s, z, bs))


def _device_ops(gpu, basis: bytes, src: bytes, bs: int):
    import torch

    b = _to_dev(basis)
    w, s = gpu.signature(b, bs)
    nb = w.numel()
    idx = gpu.Index(w, s, bs, (len(basis) - (nb - 1) * bs) if nb else 0)
    try:
        d = gpu.match(idx, _to_dev(src), length=len(src))
        torch.cuda.synchronize()
        return d
    finally:
        idx.close()


def _set_env(monkeypatch, env):
    for k in SCAN_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# ---------------------------------------------------------------------------
# signature kernels, block sizes up to 128 KiB
# ---------------------------------------------------------------------------
SIG_BS = [17, 240, 1007, 4096, 8192, 131071, 131072]


def _sig_data(family, bs, seed=0):
    """At least nine blocks and 64 KiB (several workgroups of every kernel), a partial last block."""
    return S.family_bytes(family, max(9 * bs, 64 << 10) // bs * bs + bs // 3 + 5, seed)


@pytest.mark.parametrize("shift", [0, 3])
@pytest.mark.parametrize("bs", SIG_BS)
def test_signature_single(bs, shift, gpu):
    """k_sig_fast (whole 64-byte stripes, an aligned buffer), k_sig_wave (any other block above
    240 bytes, and the partial last block), k_sig_scalar (up to 240 bytes)."""
    want = "k_sig_fast" if bs % 64 == 0 and bs >= 256 and not shift else "k_sig_wave" if bs > 240 else "k_sig_scalar"
    for family in S.FAMILY_NAMES:
        data = _sig_data(family, bs)
        (w, s), prof = _profiled(gpu, lambda: gpu.signature(_to_dev(data, shift), bs))
        assert want in prof, (family, prof)
        assert _sig_lists(w, s) == _oracle_sig(data, bs), (family, bs, shift)


@pytest.mark.parametrize("shift", [0, 3])
@pytest.mark.parametrize("bs", SIG_BS)
def test_signature_batch(bs, shift, gpu):
    """k_sig_fast_batch + k_sig_list (whole stripes, 16-byte aligned files), else k_sig_batch: two
    files of each family, one of them a single whole block, and an empty one."""
    import torch

    rows = bs % 64 == 0 and bs >= 256 and not shift
    files = [b""]
    for family in S.FAMILY_NAMES:
        files += [_sig_data(family, bs, 1)[:4 * bs + bs // 3 + 5], S.family_bytes(family, bs, 2)]
    offs, pos = [], shift
    for f in files:
        offs.append(pos)
        pos += (len(f) + 15) // 16 * 16
    packed = bytearray(pos + 16)
    for o, f in zip(offs, files):
        packed[o:o + len(f)] = f
    buf = torch.from_numpy(np.frombuffer(bytes(packed), np.uint8).copy()).cuda()
    (w, s), prof = _profiled(gpu, lambda: gpu.signature_batch(buf, offs, [len(f) for f in files], bs))
    if rows:
        assert "k_sig_fast_batch" in prof and "k_sig_list" in prof and "k_sig_batch" not in prof, prof
    else:
        assert "k_sig_batch" in prof and "k_sig_fast_batch" not in prof, prof
    ew, es = [], []
    for f in files:
        fw, fs = _oracle_sig(f, bs)
        ew += fw
        es += fs
    assert _sig_lists(w, s) == (ew, es)


# ---------------------------------------------------------------------------
# the scans, every position rolled
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.SCAN_CASES, ids=lambda c: c[0])
def test_scan_kernels(case, gpu, monkeypatch):
    """One scan kernel per case (k_scan_lds, k_scan_r and k_scan_g in small mode, wide k_scan_g,
    k_scan); k_scan_g's weak hits go through k_verify_w, four windows per wave on whole stripes
    and one per wave at 1007; the partial last block through the tail rule (k_tail)."""
    _, want, bs, run, env = case
    _set_env(monkeypatch, dict(env, SYDELTA_PROBE="0"))
    for family in S.scan_families(bs):
        basis, src = S.pair(family, bs, run)
        d, prof = _profiled(gpu, lambda: _device_ops(gpu, basis, src, bs))
        assert want in prof, (family, prof)
        assert (want != "k_scan_g") or "k_verify_w" in prof, (family, prof)
        got = d.tuples()
        assert got == _oracle_ops(basis, src, bs), (family, bs)
        assert got[-1][0] == "C" and got[-1][2] == len(basis) % bs  # the tail rule's Copy


@pytest.mark.parametrize("bs", [4096, 131072, 1007, 131071])
def test_probe_identical_source(bs, gpu, monkeypatch):
    """The aligned probe on a source equal to its basis (a match source starts 16-byte aligned):
    k_probe_rows on whole stripes, k_probe elsewhere; every block is a Copy."""
    _set_env(monkeypatch, {"SYDELTA_PROBE": "1"})
    for family in S.FAMILY_NAMES:
        basis = _sig_data(family, bs, 3)
        d, prof = _profiled(gpu, lambda: _device_ops(gpu, basis, basis, bs))
        assert "k_probe" in prof, prof
        assert d.tuples() == _oracle_ops(basis, basis, bs), (family, bs)
        assert d.stats["copy_ops"] == -(-len(basis) // bs)


# ---------------------------------------------------------------------------
# K10
# ---------------------------------------------------------------------------
def _pack(parts):
    import torch

    offs, pos = [], 0
    for p in parts:
        offs.append(pos)
        pos += (len(p) + 15) & ~15
    host = bytearray(pos + 16)
    for o, p in zip(offs, parts):
        host[o:o + len(p)] = p
    buf = torch.from_numpy(np.frombuffer(bytes(host), np.uint8).copy()).cuda()
    return buf, np.array(offs, np.uint64), np.array([len(p) for p in parts], np.uint64)


@pytest.mark.parametrize("bs", S.WALK_BLOCK_SIZES)
def test_walk_files(bs, gpu, monkeypatch):
    """k_walk_files over 40 small files (sydelta_delta_pairs_device): the hits behind each literal
    run fall on the first, a middle and the last start of walk_roll's 64."""
    for k in ("SYDELTA_FILE_WALK", "SYDELTA_DEVICE_EXPAND", "SYDELTA_PROBE"):
        monkeypatch.delenv(k, raising=False)
    pairs = S.walk_pairs(bs)
    bbuf, boff, blen = _pack([b for b, _ in pairs])
    sbuf, soff, slen = _pack([s for _, s in pairs])
    (out, tot), prof = _profiled(gpu, lambda: gpu.delta_pairs(bbuf, boff, blen, sbuf, soff, slen, bs))
    assert "k_walk_files" in prof and "k_idx_insert" not in prof, prof
    for i, ((basis, src), d) in enumerate(zip(pairs, out)):
        assert d.tuples() == _oracle_ops(basis, src, bs), (bs, i)
    assert tot["copy_ops"] == sum(d.stats["copy_ops"] for d in out)


def test_chunk_path(gpu, monkeypatch):
    """The chunk path in two parts with the first part pre-rolled and the ops written on the
    device (k_preroll, k_walk_files, k_chunk_write; the settings of
    test_gpu_file_walk.test_chunk_pipeline_two_parts): 90 misses to roll from on saturated bytes."""
    basis, src = S.chunk_pair()
    bs = S.CHUNK_BS
    for k in ("SYDELTA_CHUNK_WALK", "SYDELTA_PROBE", "SYDELTA_CHUNK_PIPE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in (("SYDELTA_PREROLL", "1"), ("SYDELTA_SLIM_WALK", "1"), ("SYDELTA_CHUNK_SEG", str(S.CHUNK_SEG)),
                 ("SYDELTA_CHUNK_SEG_LAST", "8"), ("SYDELTA_DEVICE_EXPAND", "1")):
        monkeypatch.setenv(k, v)

    def run():
        b = _to_dev(basis)
        w, s = gpu.signature(b, bs)
        idx = gpu.Index(w, s, bs, len(basis) - (w.numel() - 1) * bs)
        try:
            c = gpu.Chunk(idx, _to_dev(src), 0, len(src), 0, len(src))
            try:
                d, _ = c.walk(0)
            finally:
                c.close()
            return gpu.join_deltas([d], len(src), bs)
        finally:
            idx.close()

    d, prof = _profiled(gpu, run)
    assert "k_preroll" in prof and "k_chunk_write" in prof and prof["k_walk_files"]["count"] >= 2, prof
    assert d.tuples() == _oracle_ops(basis, src, bs)


# ---------------------------------------------------------------------------
# block sizes above 128 KiB
# ---------------------------------------------------------------------------
BIG_BS = [2245696, 2245760, 16843008, 16843072]


def _big_bytes(family, n, seed):
    """(not kept: tens of MB each)"""
    return S.family_bytes.__wrapped__(family, n, seed)


def _big_file(family, bs, seed):
    """Two whole blocks and a partial one."""
    return _big_bytes(family, 2 * bs + 1007, seed)


_big_sig = _oracle_sig.__wrapped__


@pytest.mark.parametrize("bs", BIG_BS)
def test_signature_big_blocks_single(bs, gpu):
    """On 0xFF bytes the row's weighted sum fits 32 bits at 2 245 696 and not at 2 245 760, its
    byte sum at 16 843 008 and not at 16 843 072 (2^32 = 225 mod 65521: the weak hash's high,
    then low half came out wrong).  Before the row sums were made 64-bit the cases from
    2 245 760 on failed: 0xdfac3b9d for 0xdecb3b9d there, 0x2e073ec1 for 0x27e03fa2 at 16 843 072."""
    for family in ("ff", "fdff"):
        data = _big_file(family, bs, 5)
        (w, s), prof = _profiled(gpu, lambda: gpu.signature(_to_dev(data), bs))
        assert "k_sig_fast" in prof, prof
        got, exp = _sig_lists(w, s), _big_sig(data, bs)
        print(bs, family, [hex(x) for x in got[0]], [hex(x) for x in exp[0]])
        assert got == exp, (family, bs)


@pytest.mark.parametrize("bs", BIG_BS)
def test_signature_big_blocks_batch(bs, gpu):
    files = [_big_file("ff", bs, 6), _big_file("fdff", bs, 6)]
    buf, offs, lens = _pack(files)
    (w, s), prof = _profiled(gpu, lambda: gpu.signature_batch(buf, offs, lens, bs))
    assert "k_sig_fast_batch" in prof and "k_sig_list" in prof, prof
    ew, es = _big_sig(files[0], bs)
    fw, fs = _big_sig(files[1], bs)
    got = _sig_lists(w, s)
    print(bs, [hex(x) for x in got[0]], [hex(x) for x in ew + fw])
    assert got == (ew + fw, es + fs)


def test_signature_8mib_random(gpu):
    bs = 8 << 20
    data = random.Random(8).randbytes(2 * bs + 1007)
    (w, s), prof = _profiled(gpu, lambda: gpu.signature(_to_dev(data), bs))
    assert "k_sig_fast" in prof, prof
    exp = _big_sig(data, bs)
    assert _sig_lists(w, s) == exp
    buf, offs, lens = _pack([data])
    (w, s), prof = _profiled(gpu, lambda: gpu.signature_batch(buf, offs, lens, bs))
    assert "k_sig_fast_batch" in prof, prof
    assert _sig_lists(w, s) == exp


@pytest.mark.parametrize("past", [0, 64])
def test_signature_row_layout_cap(past, gpu):
    """One block at the largest window of the row layout (a lane's 32-bit sums provable at byte
    255: kRowHashMaxN) and one 64 bytes larger, which the 64-bit wave kernels take."""
    bs = S.row_hash_max_n() + past
    data = _big_bytes("ff", bs, 7)
    exp = _big_sig(data, bs)
    (w, s), prof = _profiled(gpu, lambda: gpu.signature(_to_dev(data), bs))
    assert ("k_sig_wave" if past else "k_sig_fast") in prof and ("k_sig_fast" if past else "k_sig_wave") not in prof, prof
    assert _sig_lists(w, s) == exp
    buf, offs, lens = _pack([data])
    (w, s), prof = _profiled(gpu, lambda: gpu.signature_batch(buf, offs, lens, bs))
    assert ("k_sig_batch" if past else "k_sig_fast_batch") in prof, prof
    assert ("k_sig_fast_batch" if past else "k_sig_batch") not in prof, prof
    assert _sig_lists(w, s) == exp


BIG_MATCH = 2245760


@pytest.mark.parametrize("family", ["fdff", "ff-sparse0"])
def test_match_at_2245760(family, gpu, monkeypatch):
    """A 3-block basis at n = 2 245 760, the sources `basis` and b"12345" + basis.  k_scan_g's LDS
    (the level-1 filter and a 256-entry table) and grid (ceil(tiles / per), per a multiple of
    the run of 2048 tiles) do not grow with the window, k_verify_w takes it in rows, the probe
    one window per row: scanned (SYDELTA_PROBE=0) and probed (1).  (Distinct blocks: on constant
    data every one of the 4.5 M positions would hash 2.2 MB.)"""
    bs = BIG_MATCH
    basis = _big_bytes(family, 3 * bs, 9)
    for src in (basis, b"12345" + basis):
        exp = _oracle_ops.__wrapped__(basis, src, bs)
        assert [o for o in exp if o[0] == "C"] == [("C", k * bs, bs) for k in range(3)]
        _set_env(monkeypatch, {"SYDELTA_PROBE": "0"})
        d, prof = _profiled(gpu, lambda: _device_ops(gpu, basis, src, bs))
        assert "k_scan_g" in prof and "k_verify_w" in prof and "k_scan" not in prof, prof
        assert d.tuples() == exp
        _set_env(monkeypatch, {"SYDELTA_PROBE": "1"})
        d, prof = _profiled(gpu, lambda: _device_ops(gpu, basis, src, bs))
        assert "k_probe" in prof, prof
        assert d.tuples() == exp


def test_match_refuses_per_thread_scan_above_its_lds(gpu, monkeypatch):
    """Without the level-1 filter (SYDELTA_SCAN_WIDE=0) windows above 8 KiB go to k_scan, which
    keeps 16 bytes of LDS per 64 bytes of a tile plus one window: 433 024 is the last window whose
    launch fits 160 KiB (578 KiB at 2 245 760).  The match refuses on the host, before any launch."""
    from sy_amd._lib import SYDELTA_E_INVAL, SyDeltaError

    _set_env(monkeypatch, {"SYDELTA_SCAN_WIDE": "0"})
    bs = BIG_MATCH
    basis = _big_bytes("fdff", 3 * bs, 9)
    with pytest.raises(SyDeltaError) as e:
        _profiled(gpu, lambda: _device_ops(gpu, basis, basis, bs))
    assert e.value.code == SYDELTA_E_INVAL
    assert "block_size 2245760" in str(e.value) and "up to 433024" in str(e.value), str(e.value)
    # the largest window it takes still runs
    bs = 433024
    basis = _big_bytes("fdff", 3 * bs + 1007, 10)
    src = b"12345" + basis
    d, prof = _profiled(gpu, lambda: _device_ops(gpu, basis, src, bs))
    assert "k_scan" in prof and "k_scan_g" not in prof, prof
    assert d.tuples() == _oracle_ops.__wrapped__(basis, src, bs)
