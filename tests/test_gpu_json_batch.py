"""wire.delta_batch_to_json_device (sydelta_delta_batch_to_json_device; k_jsonb_len,
k_jsonb_write): the Delta texts of a whole batch written on the device in one call.  The
expected text of every file is the host writer's (sydelta_delta_to_json), which is also held
to tests/delta_json_ref.py here."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import delta_json_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0xA5
U64_MAX = (1 << 64) - 1
EDGES = [0, 9, 10, 99, 100, 999, 1000, 10**9 - 1, 10**9, (1 << 32) - 1, 1 << 32, 10**10, 10**19 - 1, 10**19,
         U64_MAX - 1, U64_MAX]
_OP_DTYPE = np.dtype([("kind", "<u4"), ("reserved", "<u4"), ("a", "<u8"), ("b", "<u8")])


def _copies(n, rng):
    return [("C", int(rng.integers(0, 1 << 40)), int(rng.integers(0, 1 << 20))) for _ in range(n)]


@functools.lru_cache(None)
def _edge_files():
    """(ops as (kind, a, b), source_size, block_size, literal bytes) of the hand-made files."""
    rng = np.random.default_rng(7)
    files = []

    def rnd(n):
        return rng.integers(0, 256, n, dtype=np.uint8)

    for n in (0, 1, 255, 256, 257, 513):                       # Copy runs around the tile size
        files.append((_copies(n, rng), 1 << 20, 4096, rnd(0)))
    sizes = (0, 1, 15, 16, 17, 4095, 4096, 4097, 8192, 12288)  # 12288: the smallest with a middle chunk
    for n in sizes:                                            # one Data op each, read at offset 3
        files.append(([("D", 3, n)], n, 4096, rnd(n + 5)))
    lit = rnd(13000)
    alt = []
    for i, n in enumerate(sizes):                              # Copy and Data alternating
        alt += [("C", EDGES[i], EDGES[-1 - i]), ("D", int(rng.integers(0, 13000 - n)), n)]
    files.append((alt, 10**19, 9, lit))
    files.append((alt[::-1], 0, 0, lit))                       # a Data op first, a Copy last
    # every pair of digit classes in the Copy fields and in source_size / block_size
    files.append(([("C", a, b) for a in EDGES for b in EDGES], U64_MAX, U64_MAX, rnd(0)))
    for a, b in ((0, 0), (9, 10), (99, 100), (U64_MAX, 0), (12345678, 1)):  # the last: a text of 48 characters
        files.append(([], a, b, rnd(0)))
    # literals of one digit class, and digit-class changes on thread (16-byte) and wave boundaries
    # of a chunk, for the sizing's lanes (64 bytes) and the writer's threads (16 bytes, 1 KiB a wave)
    files.append(([("D", 0, 12288)], 1, 1, np.zeros(12288, dtype=np.uint8)))
    files.append(([("D", 1, 12287)], 1, 1, np.full(12288, 255, dtype=np.uint8)))
    for lo, hi in ((9, 10), (99, 100)):
        for period in (16, 64, 1024, 4096):
            i = np.arange(12288)
            pat = np.where((i // period) % 2 == 0, lo, hi).astype(np.uint8)
            files.append(([("D", 0, 12288), ("D", 5, 4096), ("D", 16, 1024)], 2, 3, pat))
            files.append(([("D", period - 1, 2), ("D", period, 1), ("C", 1, 2), ("D", period - 1, 4097)], 2, 3, pat))
    return files


_CACHE = {}


def _expected(files):
    """The host writer's text of every file, held to the independent reference; computed once."""
    key = id(files)
    if key not in _CACHE:
        from sy_amd import wire

        texts = []
        for ops, ss, bs, lit in files:
            kind = np.array([0 if o[0] == "C" else 1 for o in ops], dtype=np.uint32)
            a = np.array([o[1] for o in ops], dtype=np.uint64)
            b = np.array([o[2] for o in ops], dtype=np.uint64)
            t = wire.delta_to_json(kind, a, b, ss, bs, lit)
            ref = R.compact([o if o[0] == "C" else ("D", lit[o[1]:o[1] + o[2]].tobytes()) for o in ops], ss, bs)
            assert t == ref
            texts.append(t)
        _CACHE[key] = texts
    return _CACHE[key]


def _deltas(gpu, files):
    out = []
    for ops, ss, bs, _ in files:
        kind = np.array([0 if o[0] == "C" else 1 for o in ops], dtype=np.uint32)
        a = np.array([o[1] for o in ops], dtype=np.uint64)
        b = np.array([o[2] for o in ops], dtype=np.uint64)
        out.append(gpu.DeviceDelta(kind, a, b, ss, bs, {}))
    return out


def _pack_literals(files, lead):
    """The files' literal bytes back to back (odd lengths, so any alignment) after `lead` bytes."""
    import torch

    offs, pos = [], lead
    for _, _, _, lit in files:
        offs.append(pos)
        pos += len(lit)
    host = np.full(pos + 7, 0x33, dtype=np.uint8)
    for o, (_, _, _, lit) in zip(offs, files):
        host[o:o + len(lit)] = lit
    return (torch.from_numpy(host).cuda(), np.array(offs, dtype=np.uint64),
            np.array([len(f[3]) for f in files], dtype=np.uint64))


def _handles(lib, files):
    hs = []
    for ops, ss, bs, _ in files:
        arr = np.zeros(len(ops), dtype=_OP_DTYPE)
        for i, o in enumerate(ops):
            arr[i] = (0 if o[0] == "C" else 1, 0, o[1], o[2])
        h = lib.sydelta_delta_from_ops(arr.ctypes.data if len(ops) else None, len(ops), ss, bs)
        assert h
        hs.append(h)
    return hs


def _call(lib, ptrs, n, lbuf, loff, llen, out_ptr, out_len):
    toffs, tlens = np.full(n, 7, dtype=np.uint64), np.full(n, 7, dtype=np.uint64)
    need = ctypes.c_uint64(7)
    rc = lib.sydelta_delta_batch_to_json_device(0, ptrs, n, lbuf.data_ptr(), lbuf.numel(), loff.ctypes.data,
                                                llen.ctypes.data, out_ptr, out_len, toffs.ctypes.data,
                                                tlens.ctypes.data, ctypes.byref(need), None)
    return rc, toffs, tlens, need.value


def _check_arena(host, base, toffs, tlens, texts):
    """Every text in place, every other byte of the arena (guards and pads) still the canary."""
    want = np.full(len(host), CANARY, dtype=np.uint8)
    at = 0
    for f, t in enumerate(texts):
        assert int(toffs[f]) == at and int(tlens[f]) == len(t), f
        o = base + at
        assert host[o:o + len(t)].tobytes() == t, f
        want[o:o + len(t)] = np.frombuffer(t, dtype=np.uint8)
        at += -(-len(t) // 16) * 16
    assert np.array_equal(host, want)


@pytest.mark.parametrize("out_lead,lit_lead", [(0, 1), (1, 3), (3, 7), (8, 5), (15, 9)])
def test_tile_edges_packing_and_guards(gpu, out_lead, lit_lead):
    """Copy runs around the tile size, Data ops around the chunk size, alternating ops, digit
    classes, literal patterns: every text is the host writer's, packed at multiples of 16 from
    an arena that starts at any offset, and no other byte of the arena changes."""
    import torch

    from sy_amd import wire

    texts = _expected(_edge_files())
    assert any(len(t) % 16 == 0 for t in texts) and any(len(t) % 16 for t in texts)
    lbuf, loff, llen = _pack_literals(_edge_files(), lit_lead)
    need = sum(-(-len(t) // 16) * 16 for t in texts[:-1]) + len(texts[-1])
    base = torch.full((64 + need + 64,), CANARY, dtype=torch.uint8, device="cuda")
    assert base.data_ptr() % 16 == 0
    arena = base[16 + out_lead:16 + out_lead + need]  # exactly the packed size
    out, toffs, tlens = wire.delta_batch_to_json_device(_deltas(gpu, _edge_files()), lbuf, loff, llen, out=arena)
    torch.cuda.synchronize()
    assert out.numel() == need and out.data_ptr() == arena.data_ptr()
    _check_arena(base.cpu().numpy(), 16 + out_lead, toffs, tlens, texts)


def test_arena_from_the_bound(gpu):
    """out=None: one call into an arena of sydelta_delta_batch_to_json_bound bytes, trimmed."""
    import torch

    from sy_amd import wire

    texts = _expected(_edge_files())
    lbuf, loff, llen = _pack_literals(_edge_files(), 1)
    out, toffs, tlens = wire.delta_batch_to_json_device(_deltas(gpu, _edge_files()), lbuf, loff, llen)
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert out.data_ptr() % 16 == 0 and (toffs % np.uint64(16) == 0).all()
    assert len(host) == int(toffs[-1] + tlens[-1])
    for f, t in enumerate(texts):
        assert host[int(toffs[f]):int(toffs[f] + tlens[f])].tobytes() == t, f


def test_sizing_without_an_arena_writes_nothing(gpu):
    """d_out NULL, and an arena one byte short: the same offsets, lengths and need as the
    writing call, and no byte written."""
    import torch

    from sy_amd._lib import lib

    files = _edge_files()[:24]
    texts = _expected(_edge_files())[:24]
    lbuf, loff, llen = _pack_literals(files, 3)
    need = sum(-(-len(t) // 16) * 16 for t in texts[:-1]) + len(texts[-1])
    hs = _handles(lib, files)
    try:
        ptrs = (ctypes.c_void_p * len(hs))(*hs)
        base = torch.full((need + 32,), CANARY, dtype=torch.uint8, device="cuda")
        rc, to0, tl0, n0 = _call(lib, ptrs, len(hs), lbuf, loff, llen, None, 0)
        rc1, to1, tl1, n1 = _call(lib, ptrs, len(hs), lbuf, loff, llen, base.data_ptr() + 16, need - 1)
        torch.cuda.synchronize()
        assert rc == 0 and rc1 == 0 and n0 == n1 == need
        assert bool((base == CANARY).all())
        rc2, to2, tl2, n2 = _call(lib, ptrs, len(hs), lbuf, loff, llen, base.data_ptr() + 16, need)
        torch.cuda.synchronize()
    finally:
        for h in hs:
            lib.sydelta_delta_free(h)
    assert rc2 == 0 and n2 == need
    for to, tl in ((to0, tl0), (to1, tl1)):
        assert np.array_equal(to, to2) and np.array_equal(tl, tl2)
    _check_arena(base.cpu().numpy(), 16, to2, tl2, texts)


def test_the_same_delta_twice(gpu):
    import torch

    from sy_amd._lib import lib

    files = [_edge_files()[16], _edge_files()[3]]  # alternating ops; 256 Copies
    texts = [_expected(_edge_files())[16], _expected(_edge_files())[3]]
    lbuf, loff, llen = _pack_literals(files, 1)
    hs = _handles(lib, files)
    try:
        order = [0, 1, 0, 0, 1]
        ptrs = (ctypes.c_void_p * len(order))(*[hs[i] for i in order])
        lo, ll = loff[order].copy(), llen[order].copy()
        bound = lib.sydelta_delta_batch_to_json_bound(ptrs, len(order))
        base = torch.full((bound + 32,), CANARY, dtype=torch.uint8, device="cuda")
        rc, toffs, tlens, need = _call(lib, ptrs, len(order), lbuf, lo, ll, base.data_ptr() + 16, bound)
        torch.cuda.synchronize()
    finally:
        for h in hs:
            lib.sydelta_delta_free(h)
    assert rc == 0 and need <= bound
    _check_arena(base.cpu().numpy(), 16, toffs, tlens, [texts[i] for i in order])


@functools.lru_cache(None)
def _small_files(n=600):
    """n small files: a few Copies around one or two short literals."""
    rng = np.random.default_rng(600)
    files = []
    for f in range(n):
        lit = rng.integers(0, 256, 60 + f % 50, dtype=np.uint8)
        ops = [("C", 4096 * i, 4096) for i in range(f % 7)] + [("D", f % 9, 20 + f % 21)] + \
              [("C", 4096 * (9 + i), 4096 - (f % 3)) for i in range(f % 4)]
        if f % 5 == 0:
            ops.append(("D", 0, len(lit)))
        files.append((ops, 4096 * 16 + f, 4096, lit))
    return files


def _documented_launches():
    """DESIGN.md states the slice size and the launches per call; the test takes its
    expectation from there, not from the run."""
    txt = " ".join(open(os.path.join(ROOT, "DESIGN.md")).read().split())
    m = re.search(r"a slice holds at most (\d+) tiles and (\d+) pairs", txt)
    k = re.search(r"(\d+) profiled launch(?:es)? per slice and (\d+) more per call", txt)
    assert m and k, "DESIGN.md no longer states the batched JSON writer's slice size and launches"
    return int(m.group(1)), int(m.group(2)), int(k.group(1)), int(k.group(2))


def test_600_files_in_one_slice_of_launches(gpu):
    """The launches depend on the table slices, never on the files: 600 small files are one
    slice, and the call makes no more profiled launches than DESIGN.md documents for one."""
    import torch

    from sy_amd import wire

    texts = _expected(_small_files())
    lbuf, loff, llen = _pack_literals(_small_files(), 1)
    deltas = _deltas(gpu, _small_files())
    slice_tiles, slice_pairs, per_slice, per_call = _documented_launches()
    tiles = sum(max(1, len(ops)) for ops, _, _, _ in _small_files())  # an upper bound: a tile per op
    pairs = sum(len(ops) + 1 for ops, _, _, _ in _small_files())
    assert tiles <= slice_tiles and pairs <= slice_pairs - 257
    gpu.set_profiling(True)
    gpu.profile(reset=True)
    try:
        out, toffs, tlens = wire.delta_batch_to_json_device(deltas, lbuf, loff, llen)
        prof = gpu.profile(reset=True)
    finally:
        gpu.set_profiling(False)
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    for f, t in enumerate(texts):
        assert host[int(toffs[f]):int(toffs[f] + tlens[f])].tobytes() == t, f
    assert any(k.startswith("k_jsonb_len") for k in prof) and any(k.startswith("k_jsonb_write") for k in prof), prof
    count = sum(v["count"] for k, v in prof.items() if k != "__busy__")
    assert count <= per_slice * 1 + per_call, prof


@functools.lru_cache(None)
def _many_ops_files():
    """72 files of 2000 ops: 144 000 ops, above the 2^17 from which the host plan and the slice
    filling run on the host pool; about 143 000 pairs are three slices."""
    rng = np.random.default_rng(17)
    files = []
    for f in range(72):
        lit = rng.integers(0, 256, 500 + f, dtype=np.uint8)
        ops = []
        for i in range(2000):
            if i % 97 == f % 97:
                ops.append(("D", int(rng.integers(0, 400)), int(rng.integers(0, 100))))
            else:
                ops.append(("C", int(rng.integers(0, 1 << 34)), 4096))
        files.append((ops, 1 << 23, 4096, lit))
    return files


def test_large_batch_planned_on_the_host_pool(gpu):
    import torch

    from sy_amd import wire

    texts = _expected(_many_ops_files())
    assert sum(len(f[0]) for f in _many_ops_files()) >= 1 << 17
    lbuf, loff, llen = _pack_literals(_many_ops_files(), 5)
    out, toffs, tlens = wire.delta_batch_to_json_device(_deltas(gpu, _many_ops_files()), lbuf, loff, llen)
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    at = 0
    for f, t in enumerate(texts):
        assert int(toffs[f]) == at and int(tlens[f]) == len(t), f
        assert host[at:at + len(t)].tobytes() == t, f
        at += -(-len(t) // 16) * 16


def test_end_to_end_pairs_to_texts_to_sources(gpu):
    """delta_pairs_handle on 64 small pairs (block size 256) -> the batch's texts -> each text
    parsed on the device -> apply_batch: the sources come back exactly."""
    import torch

    from sy_amd import wire

    rng = np.random.default_rng(64)
    bs = 256
    bases, srcs = [], []
    for f in range(64):
        n = int(rng.integers(0, 24 * bs))
        basis = rng.integers(0, 256, n, dtype=np.uint8)
        p = int(rng.integers(0, n + 1))
        ed = np.concatenate([basis[:p], rng.integers(0, 256, 1 + f % 3, dtype=np.uint8), basis[p:]])
        for q in rng.integers(0, len(ed), 4):
            ed[q] ^= np.uint8(rng.integers(1, 256))
        bases.append(basis)
        srcs.append(ed if f % 8 else basis.copy())

    def pack(arrs):
        offs, pos = [], 0
        for a in arrs:
            offs.append(pos)
            pos += -(-len(a) // 16) * 16
        host = np.zeros(pos + 16, dtype=np.uint8)
        for o, a in zip(offs, arrs):
            host[o:o + len(a)] = a
        return (torch.from_numpy(host).cuda(), np.array(offs, dtype=np.uint64),
                np.array([len(a) for a in arrs], dtype=np.uint64))

    bbuf, boff, blen = pack(bases)
    sbuf, soff, slen = pack(srcs)
    batch = gpu.delta_pairs_handle(bbuf, boff, blen, sbuf, soff, slen, bs)
    try:
        out, toffs, tlens = wire.delta_batch_to_json_device(batch, sbuf, soff, slen)
        deltas = batch.deltas()
    finally:
        batch.close()
    host_src = sbuf.cpu().numpy()
    parsed, lits = [], []
    for f in range(64):
        text = out[int(toffs[f]):int(toffs[f] + tlens[f])]
        d = deltas[f]
        lit = host_src[int(soff[f]):int(soff[f] + slen[f])]
        assert bytes(text.cpu().numpy()) == wire.delta_to_json(d.kind, d.a, d.b, d.source_size, d.block_size, lit), f
        ops, lit_t, ss, blk = wire.delta_from_json_device(text.clone())
        assert (ss, blk) == (len(srcs[f]), bs)
        parsed.append(gpu.DeviceDelta(np.array([o[0] for o in ops], dtype=np.uint32),
                                      np.array([o[1] for o in ops], dtype=np.uint64),
                                      np.array([o[2] for o in ops], dtype=np.uint64), ss, blk, {}))
        lits.append(lit_t.cpu().numpy())
    lbuf, loff, llen = pack(lits)
    got, ooffs, _ = gpu.apply_batch(bbuf, boff, blen, parsed, lbuf, loff, llen)
    torch.cuda.synchronize()
    host = got.cpu().numpy()
    for f, s in enumerate(srcs):
        assert host[int(ooffs[f]):int(ooffs[f]) + len(s)].tobytes() == s.tobytes(), f


def test_refusals_name_the_file_and_op_and_write_nothing(gpu):
    """Refused on the host before any launch: a Data op past its file's literal range, a
    literal range that leaves the arena, a NULL delta."""
    import torch

    from sy_amd._lib import lib

    files = [list(f) for f in _small_files()[:12]]
    lbuf, loff, llen = _pack_literals(files, 1)
    base = torch.full((1 << 16,), CANARY, dtype=torch.uint8, device="cuda")

    def refused(hs, lo, ll, want):
        ptrs = (ctypes.c_void_p * len(hs))(*hs)
        rc, _, _, need = _call(lib, ptrs, len(hs), lbuf, lo, ll, base.data_ptr() + 16, base.numel() - 32)
        torch.cuda.synchronize()
        msg = lib.sydelta_last_error().decode()
        assert rc == -3 and need == 0, (rc, msg)
        assert msg.startswith(want), msg
        assert bool((base == CANARY).all())

    bad = [list(f) for f in files]
    ops = list(bad[7][0])
    ops[2] = ("D", int(llen[7]) - 3, 4)  # one byte past file 7's literal range, still inside the arena
    bad[7][0] = ops
    hs = _handles(lib, bad)
    try:
        refused(hs, loff, llen, "file 7: op 2: Data")
    finally:
        for h in hs:
            lib.sydelta_delta_free(h)
    hs = _handles(lib, files)
    try:
        ll = llen.copy()
        ll[11] = np.uint64(lbuf.numel() - int(loff[11]) + 1)
        refused(hs, loff, ll, "file 11: literal range")
        lo = loff.copy()
        lo[4] = np.uint64(U64_MAX - 1)
        refused(hs, lo, llen, "file 4: literal range")
        refused(hs[:5] + [None] + hs[6:], loff, llen, "file 5: NULL delta")
        # and the good batch is written
        ptrs = (ctypes.c_void_p * len(hs))(*hs)
        rc, toffs, tlens, need = _call(lib, ptrs, len(hs), lbuf, loff, llen, base.data_ptr() + 16, base.numel() - 32)
        torch.cuda.synchronize()
    finally:
        for h in hs:
            lib.sydelta_delta_free(h)
    assert rc == 0
    _check_arena(base.cpu().numpy(), 16, toffs, tlens, _expected(_small_files())[:12])
