"""wire.zstd_decompress_batch_device (sydelta_zstd_decompress_batch_device; the k_unzb_*
kernels): the zstd frames of a whole batch decoded in one call, the texts packed at multiples
of 16.  File f's text must equal its input and what the single call writes for that frame
alone; the tables must follow the packing rule; nothing outside the texts may change.

* The corpus batch (libzstd's frames of tests/zstd_frames.py, the hand-assembled frames, our
  own encoder's): frames and output at tensor offsets (1, 7) and (7, 1), the size query and an
  arena one byte short.
* Equality with the single call, file by file.
* The round trip behind the sender's batched calls, and the receiver chain up to apply_batch.
* The malformed list in the middle of a batch, with and without the status table, and the
  three cases in which a file must not see its predecessor's tables, history or text.
* 3 000 and 65 small frames (lane-per-file kernels across workgroups, the last one partly
  filled), the launch count for 3 and 300 files, four host threads on their own streams."""
import ctypes
import functools
import random
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import test_zstd as Z
import zstd_frames as F

pytestmark = pytest.mark.gpu

CANARY = 0xA5
E_INVAL = -3
# unz::Err (sydelta_unzstd.hpp), the low word of a status key
CODE = {"wrong-magic": 1, "len-3": 2, "len-5": 2, "checksum-flag": 5, "dictionary-id-1": 4, "reserved-fhd-bit": 3,
        "block-type-3": 8, "block-beyond-len": 2, "no-last-block": 2 << 32 | 2, "first-block-treeless": 14,
        "first-block-repeat-mode": 14, "ll0-offset-before-start": 19, "trailing-byte": 7}


@functools.lru_cache(None)
def _corpus():
    """[(name, frame, text)]: 80 files of 0 bytes to 3.1 MB, 22 MB of text."""
    out = [(n, f, d) for n, (f, d) in F.corpus().items()]
    out += [(f"own-{n}", Z.ref_compress(d), d) for n, d in F.own_texts()]
    out += [(n, f, d) for n, (f, d) in F.hand_frames().items()]
    return out


def _arena(frames, lead=0):
    """The frames back to back `lead` bytes into a tensor: (arena view, foffs, flens)."""
    import torch

    blob = b"".join(frames)
    t = torch.zeros(lead + max(1, len(blob)), dtype=torch.uint8, device="cuda")
    if blob:
        t[lead:lead + len(blob)] = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
    flens = np.array([len(f) for f in frames], dtype=np.uint64)
    foffs = np.concatenate([[0], np.cumsum(flens)[:-1]]).astype(np.uint64)
    return t[lead:lead + len(blob)], foffs, flens


def _packing(lens):
    """The packing rule: (text_off, out_need)."""
    offs, pos = [], 0
    for n in lens:
        offs.append(pos)
        pos += -(-n // 16) * 16
    return np.array(offs, dtype=np.uint64), (offs[-1] + lens[-1] if lens else 0)


def _raw(lib, arena, foffs, flens, d_out, out_len, status=False):
    n = len(foffs)
    toffs, tlens, st = (np.full(max(n, 1), 7, dtype=np.uint64) for _ in range(3))
    need = ctypes.c_uint64(7)
    rc = lib.sydelta_zstd_decompress_batch_device(0, arena.data_ptr(), arena.numel(), foffs.ctypes.data, flens.ctypes.data,
                                                  n, d_out, out_len, toffs.ctypes.data, tlens.ctypes.data,
                                                  st.ctypes.data if status else None, ctypes.byref(need), None)
    return rc, toffs[:n], tlens[:n], st[:n], need.value, (lib.sydelta_last_error() or b"").decode()


def _check_texts(host, base, toffs, tlens, texts):
    """Every text at its place, and every other byte of `host` still the canary."""
    want_off, need = _packing([len(t) for t in texts])
    assert np.array_equal(toffs, want_off) and [int(x) for x in tlens] == [len(t) for t in texts]
    mask = np.ones(len(host), dtype=bool)
    for f, t in enumerate(texts):
        o = base + int(want_off[f])
        assert host[o:o + len(t)].tobytes() == t, f
        mask[o:o + len(t)] = False
    assert (host[mask] == CANARY).all()
    return need


@pytest.mark.parametrize("fo,oo", [(1, 7), (7, 1)])
def test_corpus_batch_texts_tables_and_guards(gpu, fo, oo):
    import torch

    from sy_amd import wire
    from sy_amd._lib import lib

    items = _corpus()
    texts = [d for _, _, d in items]
    arena, foffs, flens = _arena([f for _, f, _ in items], fo)
    want_off, need = _packing([len(t) for t in texts])
    buf = torch.full((oo + need + 9,), CANARY, dtype=torch.uint8, device="cuda")
    out, toffs, tlens = wire.zstd_decompress_batch_device(arena, foffs, flens, out=buf[oo:oo + need])
    torch.cuda.synchronize()
    assert out.numel() == need and out.data_ptr() == buf.data_ptr() + oo
    assert _check_texts(buf.cpu().numpy(), oo, toffs, tlens, texts) == need
    # the size query and an arena one byte short: nothing written, SYDELTA_OK, the same sizes
    buf.fill_(CANARY)
    for d_out, cap in ((None, 0), (buf.data_ptr() + oo, need - 1)):
        rc, to, tl, _, nd, msg = _raw(lib, arena, foffs, flens, d_out, cap)
        torch.cuda.synchronize()
        assert rc == 0 and nd == need, (rc, msg)
        assert np.array_equal(to, want_off) and np.array_equal(tl, tlens)
        assert bool((buf == CANARY).all())
    # out=None: sized by a query of its own
    out2, to2, tl2 = wire.zstd_decompress_batch_device(arena, foffs, flens)
    assert out2.numel() == need and np.array_equal(to2, toffs) and np.array_equal(tl2, tlens)
    host = out2.cpu().numpy()
    for f, t in enumerate(texts):
        assert host[int(toffs[f]):int(toffs[f]) + len(t)].tobytes() == t, f


def test_every_file_equals_the_single_call(gpu):
    from sy_amd import wire

    items = _corpus()
    arena, foffs, flens = _arena([f for _, f, _ in items], 3)
    out, toffs, tlens = gpu.wire_batch_to_text(arena, foffs, flens)
    host = out.cpu().numpy()
    for f, (name, _, _) in enumerate(items):
        o, l = int(foffs[f]), int(flens[f])
        alone = wire.zstd_decompress_device(arena[o:o + l])
        assert int(tlens[f]) == alone.numel(), name
        assert host[int(toffs[f]):int(toffs[f] + tlens[f])].tobytes() == alone.cpu().numpy().tobytes(), name


@pytest.fixture(scope="module")
def sender(gpu):
    """70 pairs of 8-40 KiB (block size 256) through the sender's batched calls."""
    import torch

    from sy_amd import wire

    rng = np.random.default_rng(70)
    bs = 256
    bases, srcs = [], []
    for f in range(70):
        n = int(rng.integers(8 << 10, 40 << 10))
        basis = rng.integers(0, 256, n, dtype=np.uint8)
        p = int(rng.integers(0, n + 1))
        ed = np.concatenate([basis[:p], rng.integers(0, 256, 1 + 61 * (f % 7), dtype=np.uint8), basis[p:]])
        for q in rng.integers(0, len(ed), 6):
            ed[q] ^= np.uint8(rng.integers(1, 256))
        bases.append(basis)
        srcs.append(ed if f % 8 else basis.copy())

    def pack(arrs):
        offs, _ = _packing([len(a) for a in arrs])
        host = np.zeros(int(offs[-1]) + len(arrs[-1]) + 32, dtype=np.uint8)
        for o, a in zip(offs, arrs):
            host[int(o):int(o) + len(a)] = a
        return torch.from_numpy(host).cuda(), offs, np.array([len(a) for a in arrs], dtype=np.uint64)

    bbuf, boff, blen = pack(bases)
    sbuf, soff, slen = pack(srcs)
    batch = gpu.delta_pairs_handle(bbuf, boff, blen, sbuf, soff, slen, bs)
    try:
        text, toffs, tlens = wire.delta_batch_to_json_device(batch, sbuf, soff, slen)
    finally:
        batch.close()
    frames, foffs, flens = wire.zstd_compress_batch_device(text, toffs, tlens)
    torch.cuda.synchronize()
    return dict(bs=bs, srcs=srcs, pack=pack, bbuf=bbuf, boff=boff, blen=blen, text=text, toffs=toffs, tlens=tlens,
                frames=frames, foffs=foffs, flens=flens)


def test_round_trip_behind_the_senders_calls(gpu, sender):
    """decompress_batch(compress_batch(arena)) returns the arena's own tables and texts."""
    import torch

    s = sender
    got, toffs, tlens = gpu.wire_batch_to_text(s["frames"], s["foffs"], s["flens"])
    assert np.array_equal(toffs, s["toffs"]) and np.array_equal(tlens, s["tlens"])
    assert got.numel() == s["text"].numel() == int(toffs[-1] + tlens[-1])
    for f in range(len(toffs)):  # the pads of the two arenas are not compared
        a, b = int(toffs[f]), int(toffs[f] + tlens[f])
        assert torch.equal(got[a:b], s["text"][a:b]), f


def test_receiver_chain_to_apply_batch(gpu, sender):
    """The batch's texts parsed file by file, then applied in one call: the sources."""
    import torch

    from sy_amd import wire

    s = sender
    text, toffs, tlens = gpu.wire_batch_to_text(s["frames"], s["foffs"], s["flens"])
    parsed, lits = [], []
    for f in range(len(toffs)):
        ops, lit_t, ss, blk = wire.delta_from_json_device(text[int(toffs[f]):int(toffs[f] + tlens[f])].clone())
        assert (ss, blk) == (len(s["srcs"][f]), s["bs"])
        parsed.append(gpu.DeviceDelta(np.array([o[0] for o in ops], dtype=np.uint32),
                                      np.array([o[1] for o in ops], dtype=np.uint64),
                                      np.array([o[2] for o in ops], dtype=np.uint64), ss, blk, {}))
        lits.append(lit_t.cpu().numpy())
    lbuf, loff, llen = s["pack"](lits)
    got, ooffs, _ = gpu.apply_batch(s["bbuf"], s["boff"], s["blen"], parsed, lbuf, loff, llen)
    torch.cuda.synchronize()
    host = got.cpu().numpy()
    for f, src in enumerate(s["srcs"]):
        assert host[int(ooffs[f]):int(ooffs[f]) + len(src)].tobytes() == src.tobytes(), f


def _with_tables():
    """A corpus frame whose blocks define a Huffman table, and one that defines FSE tables."""
    huf = fse = None
    for name, (frame, data) in F.corpus().items():
        blocks = [b for b in F.describe(frame)["blocks"] if b["type"] == 2]
        if huf is None and blocks and blocks[-1]["lit"] == 2:
            huf = (frame, data)
        if fse is None and blocks and 2 in blocks[-1].get("modes", ()):
            fse = (frame, data)
    assert huf and fse
    return huf, fse


def test_malformed_frames_in_the_middle_of_a_batch(gpu):
    import torch

    from sy_amd import wire
    from sy_amd._lib import SyDeltaError

    small = F.corpus()["json-small-s1"]
    two = F.hand_frames()["hand-two-blocks"]
    one = F.corpus()["one-s3"]
    huf, fse = _with_tables()
    bad = F.malformed()
    assert set(CODE) == set(bad) == set(F.MALFORMED_REASON)
    cases = [(name, [small, (frame, b""), two, one]) for name, frame in bad.items()]
    # a file finds no table, no history and no text of the file before it
    cases += [("first-block-treeless", [huf, (bad["first-block-treeless"], b""), small]),
              ("first-block-repeat-mode", [fse, (bad["first-block-repeat-mode"], b""), small]),
              ("ll0-offset-before-start", [two, (bad["ll0-offset-before-start"], b""), small])]
    good_arena, gfo, gfl = _arena([small[0], two[0], one[0]], 1)
    good_texts = [small[1], two[1], one[1]]
    for name, files in cases:
        arena, foffs, flens = _arena([f for f, _ in files], 5)
        texts = [d for _, d in files]
        _, need = _packing([len(t) for t in texts])
        buf = torch.full((3 + need + 9,), CANARY, dtype=torch.uint8, device="cuda")
        # without the status table: the call's error names the file, nothing is written
        with pytest.raises(SyDeltaError) as e:
            wire.zstd_decompress_batch_device(arena, foffs, flens, out=buf[3:])
        torch.cuda.synchronize()
        assert e.value.code == E_INVAL, name
        assert "file 1: zstd frame:" in str(e.value) and F.MALFORMED_REASON[name] in str(e.value), (name, str(e.value))
        with pytest.raises(SyDeltaError) as e1:  # the single call's reason, word for word
            wire.zstd_decompress_device(arena[int(foffs[1]):int(foffs[1] + flens[1])])
        assert e.value.strerror == "file 1: " + e1.value.strerror, (name, e.value.strerror, e1.value.strerror)
        assert bool((buf == CANARY).all()), name
        # with it: the file's own status, no room taken, the neighbours exact
        out, toffs, tlens, status = wire.zstd_decompress_batch_device(arena, foffs, flens, out=buf[3:], refused_ok=True)
        torch.cuda.synchronize()
        assert [int(x) for x in status] == [0, CODE[name]] + [0] * (len(files) - 2), (name, status)
        assert int(tlens[1]) == 0 and out.numel() == need
        assert _check_texts(buf.cpu().numpy(), 3, toffs, tlens, texts) == need, name
        # and a valid batch right afterwards decodes
        gbuf = torch.full((_packing([len(t) for t in good_texts])[1] + 5,), CANARY, dtype=torch.uint8, device="cuda")
        out, toffs, tlens = wire.zstd_decompress_batch_device(good_arena, gfo, gfl, out=gbuf)
        _check_texts(gbuf.cpu().numpy(), 0, toffs, tlens, good_texts)


@functools.lru_cache(None)
def _many():
    """3 000 frames of json-small-sized texts: libzstd streamed and one-shot, and our encoder's."""
    rng = random.Random(3000)
    texts = [Z.delta_json(rng, 1 + f % 5, 0.5) for f in range(3000)]
    ways = (lambda d: F.stream_compress(d, 3), lambda d: F.oneshot_compress(d, 3), Z.ref_compress)
    return texts, [ways[f % 3](t) for f, t in enumerate(texts)]


@pytest.mark.parametrize("n", [3000, 65])
def test_many_small_files(gpu, n):
    texts, frames = _many()
    arena, foffs, flens = _arena(frames[:n], 1)
    out, toffs, tlens = gpu.wire_batch_to_text(arena, foffs, flens)
    want_off, need = _packing([len(t) for t in texts[:n]])
    assert out.numel() == need and np.array_equal(toffs, want_off)
    host = out.cpu().numpy()
    for f, t in enumerate(texts[:n]):
        assert int(tlens[f]) == len(t) and host[int(toffs[f]):int(toffs[f]) + len(t)].tobytes() == t, f


def test_launches_do_not_depend_on_the_files(gpu):
    import torch

    texts, frames = _many()
    counts = {}
    for n in (3, 300):
        arena, foffs, flens = _arena(frames[:n])
        _, need = _packing([len(t) for t in texts[:n]])
        out = torch.empty(need, dtype=torch.uint8, device="cuda")
        gpu.set_profiling(True)
        gpu.profile(reset=True)
        try:
            got, toffs, tlens = gpu.wire_batch_to_text(arena, foffs, flens, out=out)
            prof = gpu.profile(reset=True)
        finally:
            gpu.set_profiling(False)
        assert got.numel() == need
        host = got.cpu().numpy()
        for f, t in enumerate(texts[:n]):
            assert host[int(toffs[f]):int(toffs[f]) + len(t)].tobytes() == t, f
        assert all(k.startswith("k_unzb_") for k in prof if k != "__busy__"), prof
        counts[n] = {k: v["count"] for k, v in prof.items() if k != "__busy__"}
    assert counts[3] == counts[300], counts
    # every stage once (the profiler counts the 32 rounds of the pointer doubling as one scope)
    stages = ("count", "scan", "tables", "decode", "stitch", "resolve", "sizes", "arena", "place", "jump", "gather")
    assert counts[3] == {f"k_unzb_{s}": 1 for s in stages}, counts


def test_four_threads_on_their_own_streams(gpu):
    import torch

    items = _corpus()
    batches = [items[k::4] for k in range(4)]
    arenas = [_arena([f for _, f, _ in b], k) for k, b in enumerate(batches)]
    torch.cuda.synchronize()

    def one(k):
        st = torch.cuda.Stream()
        arena, foffs, flens = arenas[k]
        ok = 0
        for _ in range(3):
            with torch.cuda.stream(st):
                out, toffs, tlens = gpu.wire_batch_to_text(arena, foffs, flens, stream=st)
            host = out.cpu().numpy()
            ok += all(host[int(toffs[f]):int(toffs[f] + tlens[f])].tobytes() == d for f, (_, _, d) in enumerate(batches[k]))
        return ok

    with ThreadPoolExecutor(4) as ex:
        assert list(ex.map(one, range(4))) == [3] * 4
