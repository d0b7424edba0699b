"""wire.zstd_compress_batch_device (sydelta_zstd_compress_batch_device; k_zstdb_block,
k_zstdb_frame): the zstd frames of a whole batch of texts in one call.  File f's frame must equal
the sequential host form's (tests/csrc/zstd_ref.cpp through test_zstd.ref_compress) and the
single call's byte for byte, and the system libzstd must decode it to the text."""
import ctypes
import functools
import os
import random
import re
import threading

import numpy as np
import pytest

import test_zstd as Z

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0xA5
K = 128 << 10
E_INVAL = -3


@functools.lru_cache(None)
def _mixed():
    """(texts, their reference frames), made once.  The order puts a two-block text first, a
    three-block text behind it and a three-block text last, so that with rounds of 1 the first
    and the last file, and with rounds of 3 a middle and the last file, straddle rounds."""
    rng = random.Random(21)
    base = Z.delta_json(rng, 800, 0.5)
    copies = Z.delta_json(rng, 9000, 0.01)
    assert len(base) > K + 1 and len(copies) > 3 * K
    texts = [base[:K + 1], copies[:3 * K], b"", b"{", bytes(rng.randrange(256) for _ in range(5000)), base[:1023],
             base[:1024], base[:K - 1], base[:K], Z.delta_json(rng, 300, 0.9), b"", b"", b"7" * 300000]
    return texts, [Z.ref_compress(t) for t in texts]


def _blocks(n):
    return max(1, -(-n // K))


def _straddlers(texts, rnd):
    """The files whose blocks fall into two rounds of `rnd` blocks."""
    out, b = [], 0
    for f, t in enumerate(texts):
        nb = _blocks(len(t))
        if b // rnd != (b + nb - 1) // rnd:
            out.append(f)
        b += nb
    return out


def _pack(texts, lead=64, tail=64):
    """The texts at multiples of 16 in an arena of exactly their packed size, canary bytes in
    front, behind and in the pads: (whole tensor, arena view, offsets, lengths)."""
    import torch

    offs, pos = [], 0
    for t in texts:
        pos = -(-pos // 16) * 16
        offs.append(pos)
        pos += len(t)
    host = np.full(lead + pos + tail, CANARY, dtype=np.uint8)
    for o, t in zip(offs, texts):
        host[lead + o:lead + o + len(t)] = np.frombuffer(t, dtype=np.uint8)
    whole = torch.from_numpy(host).cuda()
    assert whole.data_ptr() % 16 == 0 and lead % 16 == 0
    return (whole, whole[lead:lead + pos], np.array(offs, dtype=np.uint64),
            np.array([len(t) for t in texts], dtype=np.uint64))


def _device(data: bytes):
    import torch

    t = torch.zeros(len(data) + 16, dtype=torch.uint8, device="cuda")
    if data:
        t[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    return t[:len(data)]


def _check_frames(host, foffs, flens, refs):
    at = 0
    for f, r in enumerate(refs):
        assert int(foffs[f]) == at and int(flens[f]) == len(r), f
        assert host[at:at + len(r)].tobytes() == r, f
        at += len(r)
    return at


def _run_mixed(lead):
    """The mixed batch into an arena of exactly the need at `lead` bytes past a 16-byte boundary;
    checks frames, tables and every canary."""
    import torch

    from sy_amd import wire

    texts, refs = _mixed()
    whole, arena, toffs, tlens = _pack(texts)
    before = whole.cpu().numpy().copy()
    need = sum(len(r) for r in refs)
    obase = torch.full((64 + need + 64,), CANARY, dtype=torch.uint8, device="cuda")
    out, foffs, flens = wire.zstd_compress_batch_device(arena, toffs, tlens, out=obase[16 + lead:16 + lead + need])
    torch.cuda.synchronize()
    assert out.numel() == need == int(foffs[-1] + flens[-1])  # out_need: the frames' total
    host = obase.cpu().numpy()
    assert _check_frames(host[16 + lead:], foffs, flens, refs) == need
    assert (host[:16 + lead] == CANARY).all() and (host[16 + lead + need:] == CANARY).all()
    assert np.array_equal(whole.cpu().numpy(), before)  # the input arena, its pads and its guards
    return host[16 + lead:16 + lead + need].tobytes()


@pytest.mark.parametrize("lead", [0, 3])
def test_mixed_batch_frames_tables_and_guards(gpu, lead):
    from sy_amd import wire

    texts, refs = _mixed()
    assert sum(len(t) for t in texts) <= 2 << 20
    packed = _run_mixed(lead)
    at = 0
    for f, (t, r) in enumerate(zip(texts, refs)):
        frame = packed[at:at + len(r)]
        at += len(r)
        assert Z.zstd_decode(frame, len(t)) == t, f
        if lead == 0:
            assert bytes(wire.zstd_compress_device(_device(t)).cpu().numpy()) == frame, f
    assert len(refs[2]) == 17  # the empty text's frame


def test_arena_from_the_bound(gpu):
    """out=None: one call into an arena of sydelta_zstd_batch_bound bytes, trimmed."""
    from sy_amd import wire

    texts, refs = _mixed()
    _, arena, toffs, tlens = _pack(texts)
    out, foffs, flens = wire.zstd_compress_batch_device(arena, toffs, tlens)
    assert out.numel() == _check_frames(out.cpu().numpy(), foffs, flens, refs)


@pytest.mark.parametrize("rnd", ["1", "3"])
def test_rounds_straddled_by_files(gpu, rnd):
    texts, _ = _mixed()
    s = _straddlers(texts, int(rnd))
    last = len(texts) - 1
    assert last in s and any(0 < f < last for f in s), s
    if rnd == "1":
        assert 0 in s
    old = os.environ.get("SYDELTA_ZSTD_BATCH")
    os.environ["SYDELTA_ZSTD_BATCH"] = rnd
    try:
        _run_mixed(0)  # the same frames as with one round
    finally:
        if old is None:
            os.environ.pop("SYDELTA_ZSTD_BATCH", None)
        else:
            os.environ["SYDELTA_ZSTD_BATCH"] = old


@functools.lru_cache(None)
def _small():
    rng = random.Random(600)
    texts = [Z.delta_json(rng, 3 + f % 38, 0.2) for f in range(600)]
    assert sum(len(t) for t in texts) <= 2 << 20 and max(len(t) for t in texts) <= K
    return texts, [Z.ref_compress(t) for t in texts]


def _documented_launches():
    """DESIGN.md states the launches of a round; the test takes its expectation from there, not
    from the run."""
    txt = " ".join(open(os.path.join(ROOT, "DESIGN.md")).read().split())
    m = re.search(r"(\d+) profiled launches per round and (\d+) more per call", txt)
    assert m, "DESIGN.md no longer states the batched zstd compressor's launches"
    return int(m.group(1)), int(m.group(2))


def test_600_files_in_one_round_of_launches(gpu):
    """The launches depend on the rounds, never on the files: 600 small texts are one round, the
    call makes no more profiled launches than DESIGN.md documents for one, and 60 texts make as
    many."""
    from sy_amd import wire

    texts, refs = _small()
    per_round, per_call = _documented_launches()
    counts = {}
    for n in (600, 60):
        _, arena, toffs, tlens = _pack(texts[:n])
        gpu.set_profiling(True)
        gpu.profile(reset=True)
        try:
            out, foffs, flens = wire.zstd_compress_batch_device(arena, toffs, tlens)
            prof = gpu.profile(reset=True)
        finally:
            gpu.set_profiling(False)
        assert out.numel() == _check_frames(out.cpu().numpy(), foffs, flens, refs[:n])
        assert any(k.startswith("k_zstdb_block") for k in prof) and any(k.startswith("k_zstdb_frame") for k in prof), prof
        counts[n] = sum(v["count"] for k, v in prof.items() if k != "__busy__")
    assert counts[600] <= per_round * 1 + per_call, counts
    assert counts[600] == counts[60], counts


def test_end_to_end_pairs_to_texts_to_frames(gpu):
    """delta_pairs_handle on 64 pairs of 64 KiB (block size 256) -> the batch's texts -> their
    frames (device.delta_batch_to_wire): every frame decodes, on the device and by libzstd, to
    the host writer's text of that delta."""
    import torch

    from sy_amd import wire

    rng = np.random.default_rng(64)
    bs, n = 256, 64 << 10
    bases, srcs = [], []
    for f in range(64):
        basis = rng.integers(0, 256, n, dtype=np.uint8)
        ed = basis.copy()
        for q in rng.integers(0, n - 600, 1 + f % 5):
            ed[q:q + 1 + 37 * (f % 16)] ^= np.uint8(1 + f)
        bases.append(basis)
        srcs.append(ed if f % 8 else basis.copy())

    def pack(arrs):
        host = np.concatenate(arrs + [np.zeros(16, dtype=np.uint8)])
        return (torch.from_numpy(host).cuda(), np.arange(len(arrs), dtype=np.uint64) * np.uint64(n),
                np.full(len(arrs), n, dtype=np.uint64))

    bbuf, boff, blen = pack(bases)
    sbuf, soff, slen = pack(srcs)
    batch = gpu.delta_pairs_handle(bbuf, boff, blen, sbuf, soff, slen, bs)
    try:
        frames, foffs, flens = gpu.delta_batch_to_wire(batch, sbuf, soff, slen)
        deltas = batch.deltas()
    finally:
        batch.close()
    torch.cuda.synchronize()
    host = frames.cpu().numpy()
    assert int(foffs[0]) == 0 and frames.numel() == int(foffs[-1] + flens[-1])
    for f in range(64):
        d = deltas[f]
        text = wire.delta_to_json(d.kind, d.a, d.b, d.source_size, d.block_size, srcs[f])
        o, l = int(foffs[f]), int(flens[f])
        assert o == (int(foffs[f - 1] + flens[f - 1]) if f else 0)
        assert Z.zstd_decode(host[o:o + l].tobytes(), len(text)) == text, f
        assert bytes(wire.zstd_decompress_device(frames[o:o + l].clone()).cpu().numpy()) == text, f


def _raw(lib, d_in, in_len, toffs, tlens, n, d_out, out_len, tables=True):
    foffs, flens = np.full(max(n, 1), 7, dtype=np.uint64), np.full(max(n, 1), 7, dtype=np.uint64)
    need = ctypes.c_uint64(7)
    rc = lib.sydelta_zstd_compress_batch_device(0, d_in, in_len, toffs.ctypes.data if tables else None,
                                                tlens.ctypes.data, n, d_out, out_len, foffs.ctypes.data,
                                                flens.ctypes.data, ctypes.byref(need), None)
    return rc, foffs, flens, need.value, (lib.sydelta_last_error() or b"").decode()


def test_refusals_the_short_arena_and_the_size_query(gpu):
    import torch

    from sy_amd._lib import lib

    texts, refs = _small()
    texts, refs = texts[:12], refs[:12]
    whole, arena, toffs, tlens = _pack(texts)
    need = sum(len(r) for r in refs)
    obase = torch.full((16 + need + 64,), CANARY, dtype=torch.uint8, device="cuda")
    d_in, in_len, d_out = arena.data_ptr(), arena.numel(), obase.data_ptr() + 16

    def refused(want, d=d_in, to=toffs, tl=tlens, tables=True):
        rc, _, _, nd, msg = _raw(lib, d, in_len, to, tl, 12, d_out, need, tables)
        torch.cuda.synchronize()
        assert rc == E_INVAL and nd == 0 and want in msg, (rc, msg)
        assert bool((obase == CANARY).all())

    to = toffs.copy()
    to[5] += np.uint64(8)
    refused("file 5: text offset", to=to)
    refused("16-byte aligned", d=d_in + 8)
    tl = tlens.copy()
    tl[11] += np.uint64(1)  # one byte past the arena
    refused("file 11: text [", tl=tl)
    to = toffs.copy()
    to[3] = np.uint64((1 << 64) - 16)
    refused("file 3: text [", to=to)
    refused("NULL table", tables=False)

    # the size query, and nfiles == 0
    rc, fo0, fl0, nd, _ = _raw(lib, d_in, in_len, toffs, tlens, 12, None, 0)
    assert rc == 0 and nd == need and bool((obase == CANARY).all())
    rc, _, _, nd0, _ = _raw(lib, d_in, in_len, toffs, tlens, 0, None, 0)
    assert rc == 0 and nd0 == 0
    # one byte short: refused with the sizes reported and nothing behind the arena written
    rc, fo1, fl1, nd, msg = _raw(lib, d_in, in_len, toffs, tlens, 12, d_out, need - 1)
    torch.cuda.synchronize()
    assert rc == E_INVAL and nd == need and f"arena holds {need - 1}, the batch needs {need}" in msg, (rc, msg)
    host = obase.cpu().numpy()
    assert (host[:16] == CANARY).all() and (host[16 + need - 1:] == CANARY).all()
    # and the arena that holds them
    rc, fo2, fl2, nd, _ = _raw(lib, d_in, in_len, toffs, tlens, 12, d_out, need)
    torch.cuda.synchronize()
    assert rc == 0 and nd == need
    for fo, fl in ((fo0, fl0), (fo1, fl1)):
        assert np.array_equal(fo, fo2) and np.array_equal(fl, fl2)
    host = obase.cpu().numpy()
    assert _check_frames(host[16:], fo2, fl2, refs) == need and (host[16 + need:] == CANARY).all()


def test_two_threads_on_their_own_streams(gpu):
    import torch

    from sy_amd import wire

    texts, refs = _mixed()
    halves = [(texts[:6], refs[:6]), (texts[6:], refs[6:])]
    packs = [_pack(t) for t, _ in halves]
    streams = [torch.cuda.Stream() for _ in halves]
    torch.cuda.synchronize()
    results, errors = [None, None], []

    def work(i):
        try:
            _, arena, toffs, tlens = packs[i]
            for _ in range(2):
                results[i] = wire.zstd_compress_batch_device(arena, toffs, tlens, stream=streams[i])
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    torch.cuda.synchronize()
    for (out, foffs, flens), (_, r) in zip(results, halves):
        assert out.numel() == _check_frames(out.cpu().numpy(), foffs, flens, r)
