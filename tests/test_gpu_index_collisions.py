"""The collision build of a single-file index over device arrays.

Block i is entry i of order / cstrong; only the weak values that several blocks share get a
run, ascending by block, in the region behind the first n entries (k_idx_insert_one,
k_idx_fix_runs, k_idx_fix_place), and a collision list that does not fit the region with its
owners (or a run of more than 256 blocks) sends the index back to the sort build (index_wait
reads the flag).  Random data holds
no such weak values, so the signature of 20 000 random blocks (the C oracle's) is edited before
the index is made: blocks are given another block's weak value, and sometimes its strong value.
Every op list is compared with oracle.generate_delta on the same edited arrays; the sources hold
the planted blocks at block multiples and one byte off them.

The region of a 20 000-block index has C = max(4096, 2^ceil(log2(n / 64))) = 4096 entries."""
import functools
import threading

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

N = 20000
CAP = 4096
_KNOBS = ("SYDELTA_PROBE", "SYDELTA_SCAN_SMALL", "SYDELTA_CHUNK_WALK", "SYDELTA_DEVICE_WALK", "SYDELTA_L1",
          "SYDELTA_PHASE_PROBE")


@functools.lru_cache(maxsize=None)
def _basis(bs):
    """20 000 random blocks and their signature; computed once per block size, never changed."""
    rng = np.random.default_rng(1000 + bs)
    data = rng.integers(0, 256, N * bs, dtype=np.uint8)
    w, s, z = O.C().compute_checksums(data, bs, threads=8)
    # the rare natural twin would move the capacity cases' counts: none at these seeds
    assert len(np.unique(w)) == N, "the random basis holds a weak-value twin; pick another seed"
    for a in (data, w, s, z):
        a.setflags(write=False)
    return data, w, s, z


def _dev(a):
    import torch

    t = torch.zeros(a.size + 16, dtype=torch.uint8, device="cuda")
    t[:a.size] = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t


def _source(data, bs, blocks, rng):
    """The given basis blocks twice each -- in a stretch that keeps them at block multiples, then
    each behind one junk byte more (one byte off, two bytes off, ...) -- between random bytes."""
    parts = [rng.integers(0, 256, 3 * bs, dtype=np.uint8)]
    for t in blocks:
        parts.append(data[t * bs:(t + 1) * bs])
    parts.append(rng.integers(0, 256, bs + 7, dtype=np.uint8))
    for t in blocks:
        parts.append(rng.integers(0, 256, 1, dtype=np.uint8))
        parts.append(data[t * bs:(t + 1) * bs])
    parts.append(rng.integers(0, 256, 2 * bs + 11, dtype=np.uint8))
    return np.concatenate(parts)


def _match(gpu, w, s, bs, src, streams=1):
    """gpu.match against an index made from device copies of (w, s); the kernels that ran.
    streams > 1: as many host threads, each matching the same index on a stream of its own."""
    import torch

    dw = torch.from_numpy(w.view(np.int32).copy()).cuda()
    ds = torch.from_numpy(s.view(np.int64).copy()).cuda()
    sd = _dev(src)
    torch.cuda.synchronize()
    gpu.set_profiling(True)
    gpu.profile(reset=True)
    try:
        idx = gpu.Index(dw, ds, bs, bs)
        if streams == 1:
            got = [gpu.match(idx, sd, length=src.size).tuples()]
        else:
            got = [None] * streams
            gate = threading.Barrier(streams)

            def run(k):
                st = torch.cuda.Stream()
                gate.wait()
                got[k] = gpu.match(idx, sd, stream=st, length=src.size).tuples()

            th = [threading.Thread(target=run, args=(k,)) for k in range(streams)]
            for t in th:
                t.start()
            for t in th:
                t.join()
        idx.close()
        prof = gpu.profile(reset=True)
    finally:
        gpu.set_profiling(False)
    return got, prof


def _expect(w, s, z, bs, src):
    return O.ops_from_arrays(*O.C().generate_delta(src, w, s, z, bs))


def _entries(w):
    """Entries the collision region needs: every block of a weak value that several blocks share."""
    _, c = np.unique(w, return_counts=True)
    return int(c[c >= 2].sum())


def _plant(w, s, members, target, same_strong=()):
    """Give every block of `members` the weak value of `target` (and those of same_strong its
    strong value too)."""
    for j in members:
        if j != target:
            w[j] = w[target]
    for j in same_strong:
        s[j] = s[target]


def _runs(rng, used, length, lo=0, hi=N):
    """`length` distinct unused blocks of [lo, hi), ascending."""
    out = []
    while len(out) < length:
        j = int(rng.integers(lo, hi))
        if j not in used:
            used.add(j)
            out.append(j)
    return sorted(out)


def _planted(bs, seed):
    """The signature with every kind of run planted in several slots at once, and the blocks the
    source is made of.  seed moves every run's blocks: which of them wins the table's slot (and
    so whether the owner is the lowest) is up to the hardware, so the placements vary instead."""
    data, w0, s0, z = _basis(bs)
    w, s = w0.copy(), s0.copy()
    rng = np.random.default_rng(seed)
    used, targets = set(), []
    # run lengths 2, 3, 24, 64, 65, distinct strong values; the block the source holds is the
    # first, a middle one and the last of the run (65: the sweep's second step of 64 candidates)
    for length in (2, 3, 24, 64, 65):
        for pick in (0, length // 2, length - 1):
            m = _runs(rng, used, length)
            _plant(w, s, m, m[pick])
            targets.append(m[pick])
    # equal strong values: the lower index must win, whichever block the source's bytes are
    for length, (lo, hi) in ((2, (1, 0)), (3, (2, 0)), (24, (23, 5)), (65, (64, 63))):
        m = _runs(rng, used, length)
        _plant(w, s, m, m[lo], same_strong=[m[hi]])
        targets.append(m[lo])
    # runs whose blocks sit in one workgroup of the insert, in neighbouring ones, and far apart
    for lo, hi in ((512, 768), (1024, 1536), (0, N)):
        m = _runs(rng, used, 5, lo, hi)
        _plant(w, s, m, m[3])
        targets.append(m[3])
    # ... and untouched blocks beside them
    targets += _runs(rng, used, 6)
    order = [targets[i] for i in rng.permutation(len(targets))]
    return w, s, z, _source(data, bs, order, rng), targets


def _defaults(monkeypatch):
    for k in _KNOBS:
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("route", ["default", "scan", "probe"])
@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("bs", [256, 4096])
def test_planted_runs(gpu, monkeypatch, bs, seed, route):
    """Run lengths, the pick within a run, equal strong values and placements, in one signature;
    through the default route, with every position scanned (the fat table's multi entries) and
    with the aligned probe first (k_probe_lookup)."""
    _defaults(monkeypatch)
    if route != "default":
        monkeypatch.setenv("SYDELTA_PROBE", "0" if route == "scan" else "1")
    w, s, z, src, targets = _planted(bs, seed)
    exp = _expect(w, s, z, bs, src)
    # every planted block is found twice, and an equal strong value sends the Copy to the lower block
    assert sum(k == "C" for k, _, _ in exp) == 2 * len(targets)
    (got,), prof = _match(gpu, w, s, bs, src)
    assert got == exp
    assert "k_idx_fix" in prof and "k_idx_order" not in prof, prof


@pytest.mark.parametrize("bs", [256, 4096])
def test_two_threads_one_index(gpu, monkeypatch, bs):
    """Two host threads match one index at once, each on its own stream: both wait for the build
    (and only one of them settles it)."""
    _defaults(monkeypatch)
    w, s, z, src, _ = _planted(bs, 3)
    exp = _expect(w, s, z, bs, src)
    for _ in range(3):
        got, _ = _match(gpu, w, s, bs, src, streams=2)
        assert got[0] == exp and got[1] == exp


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("bs", [256, 4096])
def test_no_collisions_tiny(gpu, monkeypatch, bs, n):
    _defaults(monkeypatch)
    data, w0, s0, z0 = _basis(bs)
    w, s, z = w0[:n].copy(), s0[:n].copy(), z0[:n].copy()
    src = _source(data, bs, list(range(n)), np.random.default_rng(7))
    exp = _expect(w, s, z, bs, src)
    assert sum(k == "C" for k, _, _ in exp) == 2 * n
    (got,), prof = _match(gpu, w, s, bs, src)
    assert got == exp
    assert "k_idx_order" not in prof, prof


@pytest.mark.parametrize("entries", [CAP - 1, CAP, CAP + 1])
@pytest.mark.parametrize("bs", [256, 4096])
def test_capacity_edges(gpu, monkeypatch, bs, entries):
    """Collision list and owners of exactly C - 1, C and C + 1 entries (pairs, and one run of
    three where the count is odd): the last does not fit and the sort build runs instead."""
    _defaults(monkeypatch)
    data, w0, s0, z = _basis(bs)
    w, s = w0.copy(), s0.copy()
    rng = np.random.default_rng(40 + entries)
    perm = [int(x) for x in rng.permutation(N)[:entries]]
    runs, at = [], 0
    if entries % 2:
        runs.append(sorted(perm[:3]))
        at = 3
    runs += [sorted(perm[i:i + 2]) for i in range(at, entries, 2)]
    for m in runs:
        _plant(w, s, m, m[-1])
    assert _entries(w) == entries
    targets = [m[-1] for m in runs[:40]] + [m[0] for m in runs[40:50]]  # (the latter: no longer found)
    src = _source(data, bs, targets, rng)
    exp = _expect(w, s, z, bs, src)
    assert sum(k == "C" for k, _, _ in exp) == 2 * 40
    (got,), prof = _match(gpu, w, s, bs, src)
    assert got == exp
    assert ("k_idx_order" in prof) == (entries > CAP), prof


@pytest.mark.parametrize("length", [256, 257])
@pytest.mark.parametrize("bs", [256, 4096])
def test_longest_chained_run(gpu, monkeypatch, bs, length):
    """A run of 256 blocks is the longest the fix-up chains; one more and the sort build runs.
    The source holds the run's last block (every candidate swept) and its first."""
    _defaults(monkeypatch)
    data, w0, s0, z = _basis(bs)
    w, s = w0.copy(), s0.copy()
    rng = np.random.default_rng(500 + length)
    m = _runs(rng, set(), length)
    _plant(w, s, m, m[-1])
    assert _entries(w) == length
    src = _source(data, bs, [m[-1], m[0], m[-1]], rng)
    exp = _expect(w, s, z, bs, src)
    assert sum(k == "C" for k, _, _ in exp) == 4
    (got,), prof = _match(gpu, w, s, bs, src)
    assert got == exp
    assert ("k_idx_order" in prof) == (length > 256), prof


@pytest.mark.parametrize("bs", [256, 4096])
def test_identical_blocks_overflow(gpu, monkeypatch, bs):
    """20 000 identical blocks: the list overflows at once, the sort build runs, and every Copy
    comes from block 0."""
    _defaults(monkeypatch)
    data, _, _, _ = _basis(bs)
    block = data[:bs]
    basis = np.tile(block, N)
    w, s, z = O.C().compute_checksums(basis, bs, threads=8)
    assert len(np.unique(w)) == 1 and len(np.unique(s)) == 1
    rng = np.random.default_rng(9)
    src = np.concatenate([np.tile(block, 5), rng.integers(0, 256, 3, dtype=np.uint8), np.tile(block, 3),
                          rng.integers(0, 256, bs + 1, dtype=np.uint8), block])
    exp = _expect(w, s, z, bs, src)
    copies = [op for op in exp if op[0] == "C"]
    assert len(copies) == 9 and all(a == 0 for _, a, _ in copies)
    (got,), prof = _match(gpu, w, s, bs, src)
    assert got == exp
    assert "k_idx_order" in prof, prof
