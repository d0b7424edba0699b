"""GPU parity on real weak-hash collisions, and the device expansion's hand-back to the host.

Every match path rests on generator.rs:121-155: a window whose Adler-32 is a basis block's is
a hit only if its XXH3 is equal too, and among several blocks of that weak value the first in
index order with the equal strong hash wins.  The other GPU tests' inputs (random, periodic,
two-letter data) never hold two different blocks of one weak value, so the candidate scans
(K10's self_lookup and walk_lookup, the scans' candidate lists), the walk's resumption one
byte after a weak hit that fails verification, and the tail rule against a suffix with the
last block's weak value only, ran without one.  The scenarios of tests/adler_twins.py (checked
against both oracles in tests/test_adler_twins.py) put one on each route; every op list is
compared op for op with the C oracle's.

The second part reaches each reason for which k_walk_files' expansion (expand_file) hands a
batch back to the host, and pins sydelta_expand_counters exactly."""
import ctypes
import functools
import random

import pytest

import adler_twins as T
from oracle import oracle as O
from test_gpu_file_walk import _batch, _cases, _chunk_walk, _expanded, _oracle_ops, _pack, _to_dev

pytestmark = pytest.mark.gpu


def _expect(sc):
    """The C oracle's op list of a scenario (its own signature arrays for synthetic-R6)."""
    C = O.C()
    if sc.sig is not None:
        w, s, z = sc.sig
    else:
        w, s, z = C.compute_checksums(sc.basis, sc.bs)
    ops = O.ops_from_arrays(*C.generate_delta(sc.src, w, s, z, sc.bs))
    assert ops == sc.expect, sc.name  # (the fact the scenario exists for)
    return ops


@functools.lru_cache(maxsize=None)
def _scenarios(bs):
    """The scenarios at bs and their expected op lists, computed once."""
    scs = T.scenarios(bs)
    return scs, [_expect(sc) for sc in scs]


@functools.lru_cache(maxsize=None)
def _batch_inputs(bs):
    """One batch of 80 files: every scenario, padded with _cases files; the signature overrides
    (synthetic-R6) and the oracle's op lists."""
    scs, exp = _scenarios(bs)
    pad = _cases(random.Random(5000 + bs), bs, 80 - len(scs))
    pairs = pad[:40] + [(sc.src, sc.basis) for sc in scs] + pad[40:]
    sigs = {40 + i: (sc.sig[0], sc.sig[1]) for i, sc in enumerate(scs) if sc.sig is not None}
    C = O.C()
    want = [_oracle_ops(C, s, b, bs) for s, b in pad[:40]] + exp + [_oracle_ops(C, s, b, bs) for s, b in pad[40:]]
    # with the bases' own signatures (the one-call form hashes them itself)
    own = [_oracle_ops(C, *pairs[f], bs) if f in sigs else want[f] for f in range(len(pairs))]
    assert len(pairs) == 80 and all(-(-len(b) // bs) <= 64 for _, b in pairs)
    return pairs, sigs, want, own


# ---------------------------------------------------------------------------
# a batch of small files: K10 self-indexed (self_lookup, the LDS table's atomicMin)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dx", ["0", "1"])
@pytest.mark.parametrize("bs", [256, 320, 1024, 4096, 8192])
def test_batch_self_indexed_walk(gpu, monkeypatch, bs, dx):
    pairs, sigs, want, own = _batch_inputs(bs)
    monkeypatch.delenv("SYDELTA_FILE_SEGS", raising=False)
    out, tot, prof = _batch(gpu, pairs, bs, "1", monkeypatch, dx, sigs)
    assert "k_walk_files" in prof, prof
    for f, d in enumerate(out):
        assert d.tuples() == want[f], (bs, dx, f)
        assert d.source_size == len(pairs[f][0]) and d.block_size == bs
    assert tot["copy_ops"] == sum(d.stats["copy_ops"] for d in out) == sum(k == "C" for w in want for k, _, _ in w)
    assert tot["literal_bytes"] == sum(d.stats["literal_bytes"] for d in out)
    assert tot["literal_bytes"] == sum(b for w in want for k, _, b in w if k == "D")
    # the classifier path (aligned probe, scans, host walk) on the same batch
    out0, tot0, prof0 = _batch(gpu, pairs, bs, "0", monkeypatch, dx, sigs)
    assert "k_walk_files" not in prof0, prof0
    assert [d.tuples() for d in out0] == want
    assert tot0["copy_ops"] == tot["copy_ops"] and tot0["literal_bytes"] == tot["literal_bytes"]
    # the one-call form (it hashes the bases itself)
    monkeypatch.setenv("SYDELTA_DEVICE_EXPAND", dx)
    bbuf, boff, blen = _pack([b for _, b in pairs])
    sbuf, soff, slen = _pack([s for s, _ in pairs])
    gpu.set_profiling(True)
    gpu.profile(reset=True)
    outp, totp = gpu.delta_pairs(bbuf, boff, blen, sbuf, soff, slen, bs)
    profp = gpu.profile(reset=True)
    gpu.set_profiling(False)
    assert "k_walk_files" in profp, profp
    assert [d.tuples() for d in outp] == own
    assert totp["copy_ops"] == sum(k == "C" for w in own for k, _, _ in w)


# ---------------------------------------------------------------------------
# one file: gpu.match through the classifier's routes
# ---------------------------------------------------------------------------
def _match(gpu, sc):
    if sc.sig is not None:  # the arrays as sent, from the host
        idx = gpu.Index(sc.sig[0], sc.sig[1], sc.bs, int(sc.sig[2][-1]))
    else:
        b = _to_dev(sc.basis)
        w, s = gpu.signature(b[:len(sc.basis)], sc.bs)
        idx = gpu.Index(w, s, sc.bs, sc.last_size())
    d = gpu.match(idx, _to_dev(sc.src), length=len(sc.src))
    idx.close()
    return d


def _match_all(gpu, bs):
    """Every scenario at bs through gpu.match; the kernels that ran."""
    scs, exp = _scenarios(bs)
    gpu.set_profiling(True)
    gpu.profile(reset=True)
    try:
        got = [_match(gpu, sc).tuples() for sc in scs]
        prof = gpu.profile(reset=True)
    finally:
        gpu.set_profiling(False)
    for sc, g, e in zip(scs, got, exp):
        assert g == e, (bs, sc.name)
    return prof


_KNOBS = ("SYDELTA_PROBE", "SYDELTA_SCAN_SMALL", "SYDELTA_FILE_WALK", "SYDELTA_CHUNK_WALK", "SYDELTA_DEVICE_WALK",
          "SYDELTA_DEVICE_WALK_MIN", "SYDELTA_PHASE_PROBE", "SYDELTA_DEVICE_EXPAND", "SYDELTA_FILE_SEGS")


def _defaults(monkeypatch):
    for k in _KNOBS:
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("bs", [512, 4096, 8192, 65536])
def test_match_default_route(gpu, monkeypatch, bs):
    _defaults(monkeypatch)
    _match_all(gpu, bs)


@pytest.mark.parametrize("small", ["0", "1"])
@pytest.mark.parametrize("bs", [1024, 4096])
def test_match_scan_routes(gpu, monkeypatch, bs, small):
    """Every position scanned (SYDELTA_PROBE=0): k_scan_lds, or the register-fed scans' small
    mode (k_scan_r at bs 4096, else k_scan_g with k_verify_w), as test_scan_small_index_modes."""
    _defaults(monkeypatch)
    monkeypatch.setenv("SYDELTA_PROBE", "0")
    monkeypatch.setenv("SYDELTA_SCAN_SMALL", small)
    prof = _match_all(gpu, bs)
    want = "k_scan_lds" if small == "0" else ("k_scan_r" if bs == 4096 else "k_scan_g")
    assert want in prof, prof
    if want == "k_scan_g":
        assert "k_verify_w" in prof, prof


@pytest.mark.parametrize("bs", [512, 4096, 8192])
def test_match_aligned_probe(gpu, monkeypatch, bs):
    """SYDELTA_PROBE=1: the aligned probe first, scans only where it misses."""
    _defaults(monkeypatch)
    monkeypatch.setenv("SYDELTA_PROBE", "1")
    _match_all(gpu, bs)


@pytest.mark.parametrize("probe", ["0", "1"])
@pytest.mark.parametrize("bs", [512, 4096])
def test_match_device_resolved_walk(gpu, monkeypatch, bs, probe):
    """K5b (the settings of test_gpu_device_walk.py's device_walk fixture): the walk resolved
    on the device from the hit lists, or handed back to the host walk; the counters show it."""
    from sy_amd._lib import lib

    _defaults(monkeypatch)
    for k, v in (("SYDELTA_DEVICE_WALK", "1"), ("SYDELTA_DEVICE_WALK_MIN", "1"), ("SYDELTA_CHUNK_WALK", "0"),
                 ("SYDELTA_FILE_WALK", "0"), ("SYDELTA_PHASE_PROBE", "0"), ("SYDELTA_PROBE", probe)):
        monkeypatch.setenv(k, v)

    def counters():
        a, b = ctypes.c_uint64(), ctypes.c_uint64()
        lib.sydelta_walk_counters(ctypes.byref(a), ctypes.byref(b))
        return a.value, b.value

    w0, f0 = counters()
    _match_all(gpu, bs)
    w1, f1 = counters()
    assert w1 > w0 or (probe == "1" and f1 > f0), "the device walk did not run"


# ---------------------------------------------------------------------------
# a chunk of one file: K10 on the global index (walk_lookup's candidate loop)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cw", ["", "0"])
@pytest.mark.parametrize("nchunks", [1, 3])
@pytest.mark.parametrize("bs", [256, 4096])
def test_chunk_walk_global_index(gpu, monkeypatch, bs, nchunks, cw):
    """gpu.Chunk in 1 and 3 chunks (as many as the source has blocks of window starts, cut at
    block multiples: the Copy after a failed weak hit crosses into the next chunk), walked by
    K10 on the index's global tables, or (SYDELTA_CHUNK_WALK=0) classified and walked on the host."""
    _defaults(monkeypatch)
    if cw:
        monkeypatch.setenv("SYDELTA_CHUNK_WALK", cw)
    scs, exp = _scenarios(bs)
    gpu.set_profiling(True)
    gpu.profile(reset=True)
    try:
        got = []
        for sc in scs:
            npos = len(sc.src) - bs + 1
            nb = -(-npos // bs)
            k = min(nchunks, nb)
            cuts = [nb * j // k for j in range(1, k)]
            bounds = [0] + [c * bs for c in cuts] + [npos]
            assert bounds == sorted(set(bounds))
            sig = sc.sig[:2] if sc.sig is not None else None
            got.append(_chunk_walk(gpu, sc.src, sc.basis, bs, bounds, sig).tuples())
        prof = gpu.profile(reset=True)
    finally:
        gpu.set_profiling(False)
    assert ("k_walk_files" in prof) == (cw == ""), prof
    for sc, g, e in zip(scs, got, exp):
        assert g == e, (bs, nchunks, cw, sc.name)


# ---------------------------------------------------------------------------
# the device expansion's hand-back (expand_file, sydelta_filewalk.hip)
# ---------------------------------------------------------------------------
XBS = 256


def _expand_cap(max_nblk):
    """Records expand_file holds for one file: cap = (lds_bytes - 272) / (sizeof(WalkRec) + 4),
    sizeof(WalkRec) = 16, lds_bytes = walk_lds(self_nb).total with self_nb the most blocks of any
    basis of the batch: 4 fw (filter) + 1024 + 4 * 64 + 8 * 64 + 4 fw (table) + 4 * roundup4(nb),
    fw = 2^k >= 2 nb, k >= 6 (walk_lds, self_bits)."""
    k = 6
    while (1 << k) < 2 * max_nblk:
        k += 1
    fw = 1 << k
    total = 4 * fw + 1024 + 4 * 64 + 8 * 64 + 4 * fw + 4 * ((max_nblk + 3) & ~3)
    return (total - 272) // 20


def _records(ops, bs):
    """Run-length records of an op list (WalkRec): a Data op, or a run of Copies of consecutive blocks."""
    n, prev = 0, None
    for k, a, _ in ops:
        if k == "D" or prev is None or a != prev + bs:
            n += 1
        prev = a if k == "C" else None
    return n


@functools.lru_cache(maxsize=None)
def _small_files():
    """80 small files at bs 256, one unit each whatever the segment count chosen (sources of
    at most 30 blocks: a segment has at least 32): the scenarios and _cases files."""
    scs, exp = _scenarios(XBS)
    C = O.C()
    pad = [p for p in _cases(random.Random(6000), XBS, 200) if len(p[0]) <= 30 * XBS and len(p[1]) <= 30 * XBS]
    pad = pad[:80 - len(scs)]
    pairs = [(sc.src, sc.basis) for sc in scs] + pad
    sigs = {i: (sc.sig[0], sc.sig[1]) for i, sc in enumerate(scs) if sc.sig is not None}
    want = exp + [_oracle_ops(C, s, b, XBS) for s, b in pad]
    assert len(pairs) == 80
    return pairs, sigs, want


def _run_expand(gpu, monkeypatch, pairs, sigs, want, segs):
    """The batch through K10 with the device expansion on; every file's ops and the totals
    checked; returns the rise of sydelta_expand_counters."""
    _defaults(monkeypatch)
    if segs:
        monkeypatch.setenv("SYDELTA_FILE_SEGS", segs)
    x0 = _expanded()
    out, tot, prof = _batch(gpu, pairs, XBS, "1", monkeypatch, "1", sigs)
    x1 = _expanded()
    assert "k_walk_files" in prof, prof
    for f, d in enumerate(out):
        assert d.tuples() == want[f], f
    for key in ("copy_ops", "data_ops", "literal_bytes", "weak_hits", "verified_hits"):
        assert tot[key] == sum(d.stats[key] for d in out), key
    assert tot["copy_ops"] == sum(k == "C" for w in want for k, _, _ in w)
    assert tot["literal_bytes"] == sum(b for w in want for k, _, b in w if k == "D")
    return x1[0] - x0[0], x1[1] - x0[1]


def test_expand_clean_batch(gpu, monkeypatch):
    pairs, sigs, want = _small_files()
    assert _run_expand(gpu, monkeypatch, pairs, sigs, want, "") == (80, 0)


def _record_file(rng, npairs):
    """A source of npairs x (1 junk byte + a basis block, never the previous one's successor):
    2 npairs records (a Data op and a one-block Copy run each)."""
    blocks = [rng.randbytes(XBS) for _ in range(64)]
    src = b"".join(bytes([rng.randrange(256)]) + blocks[(7 * i) % 64] for i in range(npairs))
    return src, b"".join(blocks)


@pytest.mark.parametrize("segs", ["1", ""])
@pytest.mark.parametrize("over", [0, 10])
def test_expand_too_many_records(gpu, monkeypatch, over, segs):
    """One file of the batch with cap + 10 records (cap: _expand_cap of the batch's largest
    basis, this file's 64 blocks: 140): the LDS cannot hold them, the host takes the batch.
    With cap records exactly the device still expands every file.  segs 1: one unit per file."""
    pairs, sigs, want = _small_files()
    cap = _expand_cap(64)
    assert cap == 140 and max(-(-len(b) // XBS) for _, b in pairs) <= 64
    src, basis = _record_file(random.Random(61), (cap + over) // 2)
    ops = _oracle_ops(O.C(), src, basis, XBS)
    assert _records(ops, XBS) == cap + over
    pairs, want = list(pairs), list(want)
    pairs[50], want[50] = (src, basis), ops
    assert _run_expand(gpu, monkeypatch, pairs, sigs, want, segs) == ((0, 1) if over else (80, 0))


def test_expand_too_many_units(gpu, monkeypatch):
    """SYDELTA_FILE_SEGS=100: a source of 820 blocks is cut into segments of
    max(8, ceil(820 / 100)) = 9 blocks (match_walk_files), 92 units: more than the 64 that
    expand_file chains."""
    pairs, sigs, want = _small_files()
    rng = random.Random(62)
    basis = rng.randbytes(900 * XBS + 17)
    s = bytearray(basis[:820 * XBS + 100])
    s[300 * XBS + 5:300 * XBS + 5] = b"+"
    for _ in range(5):
        s[rng.randrange(len(s))] ^= 0x41
    src = bytes(s)
    nb = -(-(len(src) - XBS + 1) // XBS)
    assert nb >= 800 and -(-nb // max(8, -(-nb // 100))) > 64 and -(-len(basis) // XBS) <= 1024
    pairs, want = list(pairs), list(want)
    pairs[50], want[50] = (src, basis), _oracle_ops(O.C(), src, basis, XBS)
    assert _run_expand(gpu, monkeypatch, pairs, sigs, want, "100") == (0, 1)


def _simple_files():
    """80 files whose segments chain whatever the cut: random bases with substitutions and one
    insertion (a segment entered at a block multiple finds its first hit where the previous
    segment's last Copy ended, or later), and the scenarios."""
    scs, exp = _scenarios(XBS)
    rng = random.Random(63)
    pairs, want, C = [(sc.src, sc.basis) for sc in scs], list(exp), O.C()
    sigs = {i: (sc.sig[0], sc.sig[1]) for i, sc in enumerate(scs) if sc.sig is not None}
    while len(pairs) < 80:
        basis = rng.randbytes(rng.randint(9, 40) * XBS + rng.randint(1, XBS - 1))
        s = bytearray(basis)
        for _ in range(3):
            s[rng.randrange(len(s))] ^= 0x17
        p = rng.randrange(len(s))
        s[p:p] = rng.randbytes(rng.randint(1, 5))
        pairs.append((bytes(s), basis))
        want.append(_oracle_ops(C, bytes(s), basis, XBS))
    return pairs, sigs, want


def test_expand_units_do_not_chain(gpu, monkeypatch):
    """SYDELTA_FILE_SEGS=5, segments of 8 blocks.  Data of period 3 holds a basis block at every
    window start; after one leading junk byte the walk copies from 1, 257, ..., so the first
    segment's exit is 8 * 256 + 1, while the second segment, entered at 8 * 256, opens with a
    Copy there: neither entered at the exit nor a literal run reaching it (expand_file's bad = 1).
    No seed is involved: the pair is fixed by construction.  The same batch without that file
    expands on the device."""
    pairs, sigs, want = _simple_files()
    assert _run_expand(gpu, monkeypatch, pairs, sigs, want, "5") == (80, 0)
    basis = (b"abc" * (14 * XBS))[:40 * XBS]
    src = b"Z" + basis[:36 * XBS]
    ops = _oracle_ops(O.C(), src, basis, XBS)
    assert ops[0] == ("D", 0, 1) and all(k == "C" for k, _, _ in ops[1:-1])
    pairs, want = list(pairs), list(want)
    pairs[50], want[50] = (src, basis), ops
    assert _run_expand(gpu, monkeypatch, pairs, sigs, want, "5") == (0, 1)
