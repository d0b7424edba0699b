"""wire.checksums_batch_to_json_device / wire.checksums_batch_from_json_device
(sydelta_checksums_batch_to_json_device, k_sigb_*; sydelta_checksums_batch_from_json_device,
k_sigpb_*) and the closed steps device.signature_batch_text / device.batch_index_from_text.

The reference of every text is json.dumps with serde's separators and checksum.rs's field order
(test_gpu_sigjson._dumps) of the C oracle's signature; the reference of every parse is the
oracle's signature, the single device call on the text alone and the host parser.  The CPU suite
runs the same bodies under ASan/UBSan (tests/test_sig_batch_host.py)."""
import ctypes
import functools
import re

import numpy as np
import pytest

from test_gpu_sigjson import _dumps
from test_sig_batch_host import _expected_messages, _refused_texts

pytestmark = pytest.mark.gpu

# neighbouring empty files, the tile edges of the writer (256 entries), one file of three tiles
# and one entry, and sizes between
COUNTS = [1, 0, 2, 0, 0, 255, 256, 257, 513, 0, 3, 7, 64, 65, 100, 128, 129, 200, 31, 3 * 256 + 1]
PAD = b'{1,{"index":2,'


@functools.lru_cache(maxsize=None)
def _files(bs):
    """Per file: (bytes, weak, strong, size) with the C oracle's signature; last blocks of 1
    byte, of bs bytes and between."""
    from oracle import oracle as O

    oc = O.C()
    out = []
    for f, n in enumerate(COUNTS):
        last = (1, bs, max(1, bs // 3))[f % 3]
        host = O.synth_bytes((n - 1) * bs + last if n else 0, 0x51B0000 + 131 * f + bs)
        out.append((host,) + tuple(oc.compute_checksums(host, bs)))
    return out


def _extremes(bs):
    """Hand-made values: weak 0 / 9 / 10 / 2^32 - 1, strong 0 / 2^64 - 1."""
    out = []
    for f, n in enumerate(COUNTS):
        i = np.arange(n)
        w = np.array([0, 9, 10, 0xFFFFFFFF], dtype=np.uint32)[i % 4]
        s = np.array([0, (1 << 64) - 1], dtype=np.uint64)[(i // 4) % 2]
        z = np.full(n, bs, dtype=np.uint64)
        if n:
            z[-1] = (1, bs)[f % 2]
        out.append((None, w, s, z))
    return out


def _tables(files):
    nb = np.array([len(w) for _, w, _, _ in files], dtype=np.uint64)
    last = np.array([int(z[-1]) if len(z) else 0 for _, _, _, z in files], dtype=np.uint64)
    return nb, last


def _soa(files):
    import torch

    w = np.concatenate([w for _, w, _, _ in files]).astype(np.uint32)
    s = np.concatenate([s for _, _, s, _ in files]).astype(np.uint64)
    return torch.from_numpy(w.view(np.int32)).cuda(), torch.from_numpy(s.view(np.int64)).cuda()


def _check_packing(toffs, tlens):
    at = 0
    for f in range(len(toffs)):
        assert int(toffs[f]) == at, f
        at += (int(tlens[f]) + 15) // 16 * 16


@pytest.mark.parametrize("source", ["oracle", "extremes"])
@pytest.mark.parametrize("bs", [4096, 1007])
def test_writer_equals_json_dumps(bs, source, gpu):
    import torch

    from sy_amd._lib import check, lib

    if source == "oracle":
        files = _files(bs)
        lens = np.array([len(h) for h, *_ in files], dtype=np.uint64)
        offs = np.concatenate([[0], np.cumsum((lens + np.uint64(15)) // np.uint64(16) * np.uint64(16))[:-1]]).astype(np.uint64)
        buf = np.zeros(int(offs[-1] + lens[-1]) + 16, dtype=np.uint8)
        for (h, *_), o in zip(files, offs):
            buf[int(o):int(o) + len(h)] = h
        w, s = gpu.signature_batch(torch.from_numpy(buf).cuda(), offs, lens, bs)
        ew, es = _soa(files)
        assert torch.equal(w, ew) and torch.equal(s, es)
    else:
        files = _extremes(bs)
        w, s = _soa(files)
    nb, last = _tables(files)
    refs = [_dumps(fw, fs, fz, bs) for _, fw, fs, fz in files]

    text, toffs, tlens = gpu_wire().checksums_batch_to_json_device(w, s, nb, last, bs)
    host = text.cpu().numpy()
    _check_packing(toffs, tlens)
    for f, ref in enumerate(refs):
        assert int(tlens[f]) == len(ref), f
        assert host[int(toffs[f]):int(toffs[f]) + len(ref)].tobytes() == ref, (f, COUNTS[f])
    need = int(toffs[-1] + tlens[-1])
    assert text.numel() == need
    assert need <= lib.sydelta_checksums_batch_to_json_bound(nb.ctypes.data, last.ctypes.data, len(nb), bs)

    # every destination phase inside a 0xEE guard: texts exact, pads and guards untouched
    inside = np.zeros(need, dtype=bool)
    for f in range(len(refs)):
        inside[int(toffs[f]):int(toffs[f] + tlens[f])] = True
    for shift in (0, 1, 3, 15):
        arena = torch.full((need + 96,), 0xEE, dtype=torch.uint8, device="cuda")
        to, tl = np.zeros_like(toffs), np.zeros_like(tlens)
        got = ctypes.c_uint64()
        check(lib.sydelta_checksums_batch_to_json_device(0, w.data_ptr(), s.data_ptr(), nb.ctypes.data, last.ctypes.data,
                                                         len(nb), bs, arena.data_ptr() + 32 + shift, need, to.ctypes.data,
                                                         tl.ctypes.data, ctypes.byref(got), None))
        a = arena.cpu().numpy()
        assert got.value == need and np.array_equal(to, toffs) and np.array_equal(tl, tlens)
        body = a[32 + shift:32 + shift + need]
        assert np.array_equal(body[inside], host[inside]), shift
        assert (body[~inside] == 0xEE).all() and (a[:32 + shift] == 0xEE).all() and (a[32 + shift + need:] == 0xEE).all(), shift

    # the size query: a NULL arena, and an arena one byte short, write nothing
    for ptr, cap in ((None, 0), (1, need - 1)):
        arena = torch.full((need + 96,), 0xEE, dtype=torch.uint8, device="cuda")
        to, tl = np.zeros_like(toffs), np.zeros_like(tlens)
        got = ctypes.c_uint64()
        check(lib.sydelta_checksums_batch_to_json_device(0, w.data_ptr(), s.data_ptr(), nb.ctypes.data, last.ctypes.data,
                                                         len(nb), bs, arena.data_ptr() + 32 if ptr else None, cap,
                                                         to.ctypes.data, tl.ctypes.data, ctypes.byref(got), None))
        assert got.value == need and np.array_equal(to, toffs) and np.array_equal(tl, tlens)
        assert bool((arena == 0xEE).all())


def gpu_wire():
    from sy_amd import wire

    return wire


def _pack(texts, how):
    """The arena with the texts at multiples of 16 ('pack16') or at odd offsets ('odd'), its pad
    bytes spelling '{', digits and commas."""
    import torch

    offs, at = [], 3 if how == "odd" else 0
    for t in texts:
        offs.append(at)
        at += len(t) + 1 + (len(t) & 3) if how == "odd" else (len(t) + 15) // 16 * 16
    arena = np.frombuffer((PAD * ((at + 5) // len(PAD) + 1))[:at + 5], dtype=np.uint8).copy()
    for t, o in zip(texts, offs):
        arena[o:o + len(t)] = np.frombuffer(t, dtype=np.uint8)
    return torch.from_numpy(arena).cuda(), np.array(offs, dtype=np.uint64), np.array([len(t) for t in texts], dtype=np.uint64)


def _check_parse(res, files, order):
    weak, strong, nblocks, last = res[:4]
    hw, hs = weak.cpu().numpy().view(np.uint32), strong.cpu().numpy().view(np.uint64)
    at = 0
    for k, f in enumerate(order):
        _, fw, fs, fz = files[f]
        assert int(nblocks[k]) == len(fw), (k, f)
        assert int(last[k]) == (int(fz[-1]) if len(fz) else 0), (k, f)
        assert np.array_equal(hw[at:at + len(fw)], fw) and np.array_equal(hs[at:at + len(fs)], fs), (k, f)
        at += len(fw)
    assert at == weak.numel() == strong.numel()


@pytest.mark.parametrize("form", ["staged", "plain"])
@pytest.mark.parametrize("layout", ["pack16", "odd", "reversed", "repeated"])
@pytest.mark.parametrize("bs", [4096, 1007])
def test_parser_equals_the_oracle(bs, layout, form, gpu, monkeypatch):
    """form: the waves read their tile through LDS (the default), or from global memory
    (SYDELTA_SIGB_STAGE=0, read per call: the form tools/sig_batch_bench.py measures against)."""
    import torch

    from sy_amd._lib import check, lib

    monkeypatch.setenv("SYDELTA_SIGB_STAGE", "1" if form == "staged" else "0")
    wire = gpu_wire()
    files = _files(bs)
    order = list(range(len(files)))
    if layout == "reversed":
        order.reverse()
    texts = [_dumps(*files[f][1:], bs) for f in order]
    arena, toffs, tlens = _pack(texts, "odd" if layout in ("odd", "reversed") else "pack16")
    if layout == "repeated":  # one text listed twice: the same place, two files
        order.append(order[8])
        toffs, tlens = np.append(toffs, toffs[8]), np.append(tlens, tlens[8])
    res = wire.checksums_batch_from_json_device(arena, toffs, tlens, bs)
    _check_parse(res, files, order)

    if layout == "pack16":  # every file also as the single call and the host parser give it
        hw, hs = res[0].cpu().numpy().view(np.uint32), res[1].cpu().numpy().view(np.uint64)
        at = 0
        for k, t in enumerate(texts):
            recs, n = wire.checksums_from_json_device(arena[int(toffs[k]):int(toffs[k] + tlens[k])])
            one = recs.cpu().numpy().view(wire._SIG_DTYPE)
            assert n == int(res[2][k])
            assert np.array_equal(one["weak"], hw[at:at + n]) and np.array_equal(one["strong"], hs[at:at + n]), k
            assert np.array_equal(one, wire.checksums_from_json(t)), k
            at += n
        # the size query: an SoA one entry short is not written, guards intact; one that fits is
        need = res[0].numel()
        for cap in (need - 1, need):
            gw = torch.full((need + 32,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            gs = torch.full((need + 32,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
            so, nb, ls = (np.zeros(len(toffs), dtype=np.uint64) for _ in range(3))
            got = ctypes.c_uint64()
            check(lib.sydelta_checksums_batch_from_json_device(
                0, arena.data_ptr(), arena.numel(), toffs.ctypes.data, tlens.ctypes.data, len(toffs), bs,
                gw.data_ptr() + 64, gs.data_ptr() + 128, cap, so.ctypes.data, nb.ctypes.data, ls.ctypes.data, None,
                ctypes.byref(got), None))
            assert got.value == need and np.array_equal(nb, res[2]) and np.array_equal(ls, res[3])
            assert np.array_equal(so, np.concatenate([[0], np.cumsum(nb)[:-1]]).astype(np.uint64))
            wrote = cap >= need
            assert bool((gw[:16] == 0x5A5A5A5A).all()) and bool((gw[16 + need:] == 0x5A5A5A5A).all())
            assert bool((gs[:16] == 0x5A5A5A5A5A5A5A5A).all()) and bool((gs[16 + need:] == 0x5A5A5A5A5A5A5A5A).all())
            if wrote:
                assert torch.equal(gw[16:16 + need], res[0]) and torch.equal(gs[16:16 + need], res[1])
            else:
                assert bool((gw == 0x5A5A5A5A).all()) and bool((gs == 0x5A5A5A5A5A5A5A5A).all())


@pytest.mark.parametrize("name", sorted(_refused_texts()))
def test_a_refused_text_between_two_good_files(name, gpu):
    """Raising mode names the lowest refused file and the byte; status mode gives the exact
    status word, and both neighbours stay exact."""
    from sy_amd._lib import SyDeltaError

    wire = gpu_wire()
    bs = 4096
    files = _files(bs)
    a, b = 7, 2  # 257 blocks and 2
    texts = [_dumps(*files[a][1:], bs), _refused_texts(bs)[name], _dumps(*files[b][1:], bs)]
    msg = _expected_messages(bs)[name]
    m = re.search(r"at byte (\d+)", msg)
    want = 1 + int(m.group(1)) + ((1 << 63) if "is not block" in msg else 0)
    for how in ("pack16", "odd"):
        arena, toffs, tlens = _pack(texts, how)
        with pytest.raises(SyDeltaError) as e:
            wire.checksums_batch_from_json_device(arena, toffs, tlens, bs)
        assert str(e.value).endswith(msg), (str(e.value), msg)
        weak, strong, nblocks, last, status = wire.checksums_batch_from_json_device(arena, toffs, tlens, bs, refused_ok=True)
        assert [int(x) for x in status] == [0, want, 0], [hex(int(x)) for x in status]
        hw, hs = weak.cpu().numpy().view(np.uint32), strong.cpu().numpy().view(np.uint64)
        na, nm, nbb = (int(x) for x in nblocks)
        assert na == len(files[a][1]) and nbb == len(files[b][1]) and nm == texts[1].count(b"{")
        assert np.array_equal(hw[:na], files[a][1]) and np.array_equal(hs[:na], files[a][2])
        assert np.array_equal(hw[na + nm:], files[b][1]) and np.array_equal(hs[na + nm:], files[b][2])
        assert int(last[0]) == int(files[a][3][-1]) and int(last[2]) == int(files[b][3][-1])


def _pairs(nfiles, bs, nblk):
    """nfiles bases of nblk blocks and their edited sources, packed at multiples of the file size."""
    from oracle import oracle as O

    n = nblk * bs
    basis = np.concatenate([O.synth_bytes(n, 0x51BC0000 + f) for f in range(nfiles)])
    src = basis.copy()
    rng = np.random.default_rng(17)
    for f in range(nfiles):
        for p in rng.integers(0, n, size=1 + f % 3):
            src[f * n + int(p)] ^= 0x5A
    offs = np.arange(nfiles, dtype=np.uint64) * np.uint64(n)
    lens = np.full(nfiles, n, dtype=np.uint64)
    return basis, src, offs, lens


@pytest.mark.parametrize("nfiles", [66, 3])
def test_round_trip_and_closed_loop(nfiles, gpu, oracle_c):
    """signature_batch -> the writer -> the parser returns the signature's own SoA and tables;
    batch_index_from_text + match_batch gives, file for file, delta_pairs' ops and the C oracle's;
    with one refused text every other file's delta is unchanged."""
    import torch

    from oracle import oracle as O

    wire = gpu_wire()
    bs, nblk = 256, 32
    hb, hsrc, offs, lens = _pairs(nfiles, bs, nblk)
    basis, src = torch.from_numpy(hb).cuda(), torch.from_numpy(hsrc).cuda()
    w, s = gpu.signature_batch(basis, offs, lens, bs)
    text, toffs, tlens = gpu.signature_batch_text(basis, offs, lens, bs)
    _check_packing(toffs, tlens)
    pw, ps, nb, last = wire.checksums_batch_from_json_device(text, toffs, tlens, bs)
    assert torch.equal(pw, w) and torch.equal(ps, s)
    assert (nb == nblk).all() and (last == bs).all()

    ref, _ = gpu.delta_pairs(basis, offs, lens, src, offs, lens, bs)
    gpu.set_profiling(True)
    try:
        gpu.profile(reset=True)
        ix = gpu.batch_index_from_text(text, toffs, tlens, bs)
        got, _ = gpu.match_batch(ix, src, offs, lens)
        prof = gpu.profile(reset=True)
    finally:
        gpu.set_profiling(False)
    ix.close()
    print("kernels:", sorted(k for k in prof if not k.startswith("__")))
    assert {"k_sigpb_count", "k_sigpb_sizes", "k_sigpb_parse"} <= set(prof)
    n = nblk * bs
    for f in range(nfiles):
        assert got[f].tuples() == ref[f].tuples(), f
        fw, fs, fz = oracle_c.compute_checksums(hb[f * n:(f + 1) * n], bs)
        assert got[f].tuples() == O.ops_from_arrays(*oracle_c.generate_delta(hsrc[f * n:(f + 1) * n], fw, fs, fz, bs)), f

    # one refused text: it keeps its place, every other file's delta is unchanged
    bad = text.clone()
    r = nfiles // 2
    bad[int(toffs[r]) + 9] = ord(" ")  # {"index": 0
    ix, status = gpu.batch_index_from_text(bad, toffs, tlens, bs, refused_ok=True)
    assert [f for f in range(nfiles) if status[f]] == [r] and int(status[r]) == 1 + 1
    got, _ = gpu.match_batch(ix, src, offs, lens)
    ix.close()
    for f in range(nfiles):
        if f != r:
            assert got[f].tuples() == ref[f].tuples(), f


def test_the_launch_lists_do_not_depend_on_the_file_count(gpu):
    """sydelta_profile_json names the kernels a call launched: the same list, with the same
    counts, for 3 files and for 300, for each of the two calls."""
    import torch

    wire = gpu_wire()
    bs = 4096
    lists = {}
    for nfiles in (3, 300):
        w = torch.arange(2 * nfiles, dtype=torch.int32, device="cuda")
        s = torch.arange(2 * nfiles, dtype=torch.int64, device="cuda") * 0x1234567
        nb, last = np.full(nfiles, 2, dtype=np.uint64), np.full(nfiles, 17, dtype=np.uint64)
        gpu.set_profiling(True)
        try:
            gpu.profile(reset=True)
            text, toffs, tlens = wire.checksums_batch_to_json_device(w, s, nb, last, bs)
            pw = gpu.profile(reset=True)
            res = wire.checksums_batch_from_json_device(text, toffs, tlens, bs)
            pp = gpu.profile(reset=True)
        finally:
            gpu.set_profiling(False)
        assert torch.equal(res[0], w) and torch.equal(res[1], s)
        lists[nfiles] = [sorted((k, v["count"]) for k, v in p.items() if not k.startswith("__")) for p in (pw, pp)]
    assert lists[3] == lists[300], lists
    assert lists[3][0] == [("k_sigb_files", 1), ("k_sigb_len", 1), ("k_sigb_write", 1)], lists[3]
    assert lists[3][1] == [("k_sigpb_count", 1), ("k_sigpb_parse", 1), ("k_sigpb_sizes", 1)], lists[3]
