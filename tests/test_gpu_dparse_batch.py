"""wire.delta_batch_from_json_device (sydelta_delta_batch_from_json_device; the k_dpb_* kernels
over the wave bodies of K7d, sy_amd/csrc/sydelta_kernels.hip) and device.apply_wire_batch on the
GPU.  Every file of a batch is compared with the single call on its text alone
(sydelta_delta_from_json_device) and with the independent reference (delta_json_ref.py).

Geometry: a tile is up to 64 chunks (4096 text bytes) of one file, a wave; four tiles to a
workgroup; the lane-per-file kernels take 64 files per workgroup.  Texts: delta_json_cases.py."""
import ctypes
import functools

import numpy as np
import pytest

import delta_json_cases as cases
from delta_json_ref import compact, first_bad_re, parse_ref

pytestmark = [pytest.mark.gpu]

E_INVAL = -3
PAD = 32
POISON = np.frombuffer(b"1,22,133,4,5,66,", np.uint8)  # what lies between the texts: digits and commas


def _dev(host: np.ndarray):
    import torch

    return torch.from_numpy(np.ascontiguousarray(host)).cuda()


@functools.lru_cache(maxsize=None)
def _single(text: bytes):
    """The single call on `text` alone: ("ok", ops, literal bytes, source_size, block_size), or
    ("bad", the byte it names); held to the reference.  One parse per distinct text."""
    import torch

    from sy_amd import wire
    from sy_amd._lib import SyDeltaError

    ref, bad = parse_ref(text), first_bad_re(text)
    assert (ref is None) == (bad is not None)
    buf = torch.full((16 + len(text) + 16,), 0x31, dtype=torch.uint8, device="cuda")
    view = buf[16:16 + len(text)]
    if text:
        view.copy_(torch.frombuffer(bytearray(text), dtype=torch.uint8))
    try:
        ops, lit, n, bs = wire.delta_from_json_device(view)
    except SyDeltaError as e:
        msg = e.args[1]
        assert e.code == E_INVAL and "not serde's compact form at byte " in msg, msg
        at = int(msg.rsplit(" ", 1)[1])
        assert at == bad, (at, bad)
        return ("bad", at)
    lit = bytes(lit.cpu().numpy())
    assert ([("C", a, b) if k == 0 else ("D", lit[a:a + b]) for k, a, b in ops], n, bs) == ref
    return ("ok", ops, lit, n, bs)


def _pack(texts, odd: bool):
    """The texts in one arena: at multiples of 16, or (odd) at offsets 1, 3, 5, 7 past one; the
    bytes between them spell digits and commas.  -> (device arena, toffs, tlens)."""
    toffs, pos = [], 0
    for k, t in enumerate(texts):
        pos = (pos + 15) & ~15
        if odd:
            pos += (1, 3, 5, 7)[k % 4]
        toffs.append(pos)
        pos += len(t)
    host = np.resize(POISON, pos + 16).copy()
    for o, t in zip(toffs, texts):
        host[o:o + len(t)] = np.frombuffer(t, np.uint8)
    return _dev(host), np.array(toffs, dtype=np.uint64), np.array([len(t) for t in texts], dtype=np.uint64)


class Got:
    pass


def _raw(arena, toffs, tlens, d_lit, lit_cap, status: bool, want_out: bool = True):
    """One call: rc, message, tables, need, and the deltas copied out."""
    from sy_amd import device as dev
    from sy_amd._lib import lib

    n = len(toffs)
    g = Got()
    g.loffs, g.llens = np.full(n, 7, dtype=np.uint64), np.full(n, 7, dtype=np.uint64)
    g.status = np.full(n, 7, dtype=np.uint64) if status else None
    need, h = ctypes.c_uint64(7), ctypes.c_void_p()
    g.rc = lib.sydelta_delta_batch_from_json_device(
        0, arena.data_ptr(), arena.numel(), toffs.ctypes.data, tlens.ctypes.data, n, d_lit, lit_cap, g.loffs.ctypes.data,
        g.llens.ctypes.data, g.status.ctypes.data if status else None, ctypes.byref(need),
        ctypes.byref(h) if want_out else None, None)
    g.msg = (lib.sydelta_last_error() or b"").decode() if g.rc else ""
    g.need = need.value
    g.deltas = None
    if h:
        b = dev.DeltaBatch(h)
        assert b.count == n
        g.deltas = [(list(zip(d.kind.tolist(), d.a.tolist(), d.b.tolist())), d.source_size, d.block_size, d.stats)
                    for d in b.deltas()]
        g.stats = b.stats
        b.close()
    return g


def _packing(g):
    at = 0
    for f in range(len(g.loffs)):
        assert int(g.loffs[f]) == at, (f, g.loffs[f], at)
        at += (int(g.llens[f]) + 15) & ~15
    assert g.need == (int(g.loffs[-1] + g.llens[-1]) if len(g.loffs) else 0)


def _run(texts, odd=False, phase=0, status=False):
    """The batch parsed into a literal arena of exactly lit_need bytes at `phase` inside a 0xEE
    guard; every parsed file compared with the single call, guards and pads intact."""
    import torch

    arena, toffs, tlens = _pack(texts, odd)
    q = _raw(arena, toffs, tlens, None, 0, status, want_out=False)  # the size query
    assert q.rc == 0 or not status, q.msg
    guard = torch.full((PAD + phase + q.need + PAD,), 0xEE, dtype=torch.uint8, device="cuda")
    lo = PAD + phase
    g = _raw(arena, toffs, tlens, guard.data_ptr() + lo, q.need, status)
    torch.cuda.synchronize()
    assert g.need == q.need and np.array_equal(g.loffs, q.loffs) and np.array_equal(g.llens, q.llens)
    _packing(g)
    host = guard.cpu().numpy()
    own = np.zeros(host.size, dtype=bool)
    for f in range(len(texts)):
        own[lo + int(g.loffs[f]):lo + int(g.loffs[f] + g.llens[f])] = True
    assert (host[~own] == 0xEE).all(), "a guard or pad byte of the literal arena was written"
    if g.rc != 0:
        assert g.deltas is None
        return g
    tot = {"copy_ops": 0, "data_ops": 0, "literal_bytes": 0}
    for f, t in enumerate(texts):
        one = _single(t)
        ops, n, bs, stats = g.deltas[f]
        if one[0] == "bad":
            assert status and int(g.status[f]) == 1 + one[1], (f, g.status[f], one)
            assert ops == []
            continue
        assert not status or int(g.status[f]) == 0, (f, g.status[f])
        assert (ops, n, bs) == (one[1], one[3], one[4]), f
        o, l = lo + int(g.loffs[f]), int(g.llens[f])
        assert host[o:o + l].tobytes() == one[2], f
        want = {"copy_ops": sum(k == 0 for k, _, _ in ops), "data_ops": sum(k == 1 for k, _, _ in ops),
                "literal_bytes": len(one[2])}
        assert {k: stats[k] for k in want} == want, f
        for k in tot:
            tot[k] += want[k]
    assert {k: g.stats[k] for k in tot} == tot
    return g


def _small_texts():
    return [compact(ops, n, bs) for ops, n, bs in cases.small_accepted()]


def _geometry_texts():
    texts = [t for name, _, t in cases.end_cases() if name.startswith("end-1-")]
    assert len(texts) == 12
    want = {f"token-{cases.WAVE}{off:+d}" for off in (-70, -1, 0, 1)}
    edge = [t for name, _, t in cases.boundary_cases() if name in want]
    assert len(edge) == 4
    return texts + edge + [t for _, _, t in cases.density_cases()] + _small_texts()


@pytest.mark.parametrize("odd,phase", [(False, 0), (True, 0), (False, 1), (True, 3)])
def test_geometry_edges_in_one_batch(odd, phase, gpu):
    """Region ends around a wave's end, the longest token across it, the literal-density
    extremes and the small texts, as files of one batch: at multiples of 16 (the dword staging
    where the file's start allows it) and at odd offsets (the byte staging), the literal arena
    at phases 0, 1 and 3."""
    _run(_geometry_texts(), odd=odd, phase=phase)


@pytest.mark.parametrize("nfiles", [1, 64, 65, 200])
def test_file_counts_around_the_lane_per_file_workgroup(nfiles, gpu):
    small = _small_texts()
    _run([small[f % len(small)] for f in range(nfiles)], odd=bool(nfiles & 1), phase=nfiles % 4)


def test_size_query_and_an_arena_one_byte_short(gpu):
    """lit=None and an arena one byte short: SYDELTA_OK, the same sizes, *out filled, no byte
    written."""
    import torch

    from sy_amd import wire

    texts = _geometry_texts()
    arena, toffs, tlens = _pack(texts, False)
    full = _run(texts)
    q = _raw(arena, toffs, tlens, None, 0, False)
    guard = torch.full((PAD + full.need + PAD,), 0xEE, dtype=torch.uint8, device="cuda")
    short = _raw(arena, toffs, tlens, guard.data_ptr() + PAD, full.need - 1, False)
    torch.cuda.synchronize()
    assert bool((guard == 0xEE).all())
    for g in (q, short):
        assert g.rc == 0 and g.need == full.need
        assert np.array_equal(g.loffs, full.loffs) and np.array_equal(g.llens, full.llens)
        assert [d[:3] for d in g.deltas] == [d[:3] for d in full.deltas]
    # the wrapper: one size query, one writing call
    batch, lit, loffs, llens = wire.delta_batch_from_json_device(arena, toffs, tlens)
    batch.close()
    assert lit.numel() == full.need and np.array_equal(loffs, full.loffs) and np.array_equal(llens, full.llens)


def _refused_in_the_middle(bad_text, first, last):
    one = _single(bad_text)
    assert one[0] == "bad"
    g = _run([first, bad_text, last], odd=True, phase=1, status=True)
    assert g.rc == 0 and int(g.status[1]) == 1 + one[1] and int(g.status[0]) == 0 and int(g.status[2]) == 0
    e = _run([first, bad_text, last], odd=True, phase=1, status=False)
    assert e.rc == E_INVAL and e.msg == f"file 1: Delta JSON: not serde's compact form at byte {one[1]}", e.msg
    return g


def test_small_refused_texts_between_two_good_files(gpu):
    small = _small_texts()
    for t in cases.small_refused():
        _refused_in_the_middle(t, small[3], small[4])


def test_refusals_inside_fast_chunks_with_nonzero_bases(gpu):
    """One changed text per kind at the first chunk of wave 1 and at the last chunk the fast
    path owns of a ~70 KiB text, as file 1 of 3 behind a file with chunks and literals of its
    own: the byte named is the single call's, measured inside the file, and the neighbours are
    exact."""
    _, base, r0, r1 = cases.refuse_base()
    dens = dict((n, t) for n, _, t in cases.density_cases())
    chunks = cases.target_chunks(base, r0, r1)
    seen = 0
    for where in ("wave1-start", "last-fast"):
        per_kind = {}
        for _, kind, t in cases.deterministic_changes(base, chunks[where]):
            if kind not in per_kind and parse_ref(t) is None:
                per_kind[kind] = t
        assert sorted(per_kind) == sorted(cases.KINDS), (where, sorted(per_kind))
        for kind, t in per_kind.items():
            g = _refused_in_the_middle(t, dens["mixed"], dens["sparse"])
            assert int(g.llens[0]) > 0 and int(g.loffs[1]) > 0
            seen += 1
    assert seen == 10


def test_round_trip_pairs_to_wire_to_files(gpu):
    """delta_pairs_handle -> delta_batch_to_wire -> apply_wire_batch: the outputs are the
    sources; and the DeltaBatch the parse returns writes the original texts again."""
    import torch

    from sy_amd import wire

    rng = np.random.default_rng(175)
    bs, n = 512, 64 << 10
    bases = [rng.integers(0, 256, n, dtype=np.uint8) for _ in range(6)]
    srcs = []
    for f, basis in enumerate(bases):
        ed = basis.copy()
        for q in rng.integers(0, n - 700, 2 + f):
            ed[q:q + 1 + 97 * f] ^= np.uint8(1 + f)
        srcs.append(ed)
    srcs[1] = bases[1].copy()                           # an identical pair
    srcs[3] = rng.integers(0, 256, n, dtype=np.uint8)   # an all-new source
    srcs[4] = np.zeros(0, dtype=np.uint8)               # an empty source

    def pack(arrs):
        lens = np.array([len(a) for a in arrs], dtype=np.uint64)
        offs = np.concatenate([[0], np.cumsum((lens + np.uint64(15)) & ~np.uint64(15))[:-1]]).astype(np.uint64)
        host = np.zeros(int(offs[-1] + lens[-1]) + 16, dtype=np.uint8)
        for o, a in zip(offs, arrs):
            host[int(o):int(o) + len(a)] = a
        return _dev(host), offs, lens

    bbuf, boff, blen = pack(bases)
    sbuf, soff, slen = pack(srcs)
    batch = gpu.delta_pairs_handle(bbuf, boff, blen, sbuf, soff, slen, bs)
    try:
        text0, toffs0, tlens0 = wire.delta_batch_to_json_device(batch, sbuf, soff, slen)
        frames, foffs, flens = gpu.delta_batch_to_wire(batch, sbuf, soff, slen)
    finally:
        batch.close()
    out, ooffs, stats = gpu.apply_wire_batch(bbuf, boff, blen, frames, foffs, flens)
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    for f, s in enumerate(srcs):
        o = int(ooffs[f])
        assert int(stats["bytes_written"][f]) == len(s), f
        assert np.array_equal(host[o:o + len(s)], s), f
    # the parse's own batch feeds the JSON writer back into the original texts
    text, toffs, tlens = gpu.wire_batch_to_text(frames, foffs, flens)
    parsed, lit, loffs, llens = wire.delta_batch_from_json_device(text, toffs, tlens)
    try:
        text1, toffs1, tlens1 = wire.delta_batch_to_json_device(parsed, lit, loffs, llens)
    finally:
        parsed.close()
    assert np.array_equal(tlens1, tlens0) and np.array_equal(toffs1, toffs0)
    h0, h1 = text0.cpu().numpy(), text1.cpu().numpy()
    for f in range(len(srcs)):
        o, l = int(toffs0[f]), int(tlens0[f])
        assert np.array_equal(h0[o:o + l], h1[o:o + l]), f


def test_a_refused_text_in_apply_wire_batch_names_its_file(gpu):
    import torch

    from sy_amd import wire
    from sy_amd._lib import SyDeltaError

    small = _small_texts()
    texts = [small[2], cases.small_refused()[9], small[2]]  # [1,256]
    arena, toffs, tlens = _pack(texts, False)
    frames, foffs, flens = wire.zstd_compress_batch_device(arena, toffs, tlens)
    basis = torch.zeros(3 * 4096, dtype=torch.uint8, device="cuda")
    with pytest.raises(SyDeltaError, match="file 1: Delta JSON: not serde's compact form at byte"):
        gpu.apply_wire_batch(basis, [0, 4096, 8192], [4096] * 3, frames, foffs, flens)


def test_the_launch_list_does_not_depend_on_the_file_count(gpu):
    """sydelta_profile_json names the kernels a call launched: the same list, with the same
    counts, for 3 files and for 200."""
    from sy_amd import wire

    small = _small_texts()
    lists = {}
    for nfiles in (3, 200):
        arena, toffs, tlens = _pack([small[1 + f % (len(small) - 1)] for f in range(nfiles)], False)
        gpu.set_profiling(True)
        try:
            gpu.profile(reset=True)
            batch, *_ = wire.delta_batch_from_json_device(arena, toffs, tlens)
            batch.close()
            prof = gpu.profile(reset=True)
        finally:
            gpu.set_profiling(False)
        lists[nfiles] = sorted((k, v["count"]) for k, v in prof.items() if not k.startswith("__"))
    assert lists[3] == lists[200], lists
    names = [k for k, _ in lists[3]]
    assert names == ["k_dpb_count", "k_dpb_parse", "k_dpb_place", "k_dpb_sizes", "k_dpb_tail"], names
    assert all(c == 2 for _, c in lists[3]), lists[3]  # the size query and the writing call
