"""k_scan_r's launch-wide run queue: the waves of every workgroup claim runs
-- pairs of 16384-position tiles -- from one counter in global memory instead of each workgroup
dividing a fixed range.  Pinned here: position counts around a tile and a run (the last, odd tile
is a run of one), runs cut at segment boundaries, and a launch with a few more runs than waves.

One basis of 16 392 blocks at bs 4096 (the level-1 path), signed by the C oracle, under both
level-1 layouts (SYDELTA_L1)."""
import functools

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

BS = 4096
NB = 16384 + 8
TILE = 16384
_KNOBS = ("SYDELTA_PROBE", "SYDELTA_SCAN_SMALL", "SYDELTA_CHUNK_WALK", "SYDELTA_DEVICE_WALK", "SYDELTA_L1",
          "SYDELTA_PHASE_PROBE", "SYDELTA_EARLY_RIBBON")


@pytest.fixture(params=["bloom", "ribbon"])
def level1(request, monkeypatch):
    for k in _KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SYDELTA_L1", request.param)
    return request.param


@functools.lru_cache(maxsize=None)
def _basis():
    import torch

    import sy_amd.device as dev

    t = torch.empty(NB * BS + 16, dtype=torch.uint8, device="cuda")
    dev.synth_fill(t[:NB * BS], 0x5E1D0821)
    torch.cuda.synchronize()
    basis = t[:NB * BS].cpu().numpy()
    w, s, z = O.C().compute_checksums(basis, BS, threads=8)
    for a in (basis, w, s, z):
        a.setflags(write=False)
    return t[:NB * BS], basis, w, s, z


def _match(gpu, src_t, length):
    """The op list, the stats and the kernels that ran, against a fresh index of the basis."""
    import torch

    _, _, w, s, _ = _basis()
    dw = torch.from_numpy(w.view(np.int32).copy()).cuda()
    ds = torch.from_numpy(s.view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    gpu.set_profiling(True)
    gpu.profile(reset=True)
    try:
        idx = gpu.Index(dw, ds, BS, BS)
        d = gpu.match(idx, src_t, length=length)
        idx.close()
        prof = gpu.profile(reset=True)
    finally:
        gpu.set_profiling(False)
    return d, prof


def _dev(a):
    import torch

    t = torch.zeros(a.size + 16, dtype=torch.uint8, device="cuda")
    t[:a.size] = torch.from_numpy(a.copy()).cuda()
    return t


@pytest.mark.parametrize("npos", [1, 2, TILE, TILE + 1, 2 * TILE, 2 * TILE + 1, 3 * TILE, 3 * TILE + 4095])
def test_position_counts(gpu, monkeypatch, level1, npos):
    """Exactly npos positions; a basis block whose window is the last position, and one at position
    0 where the two do not overlap."""
    monkeypatch.setenv("SYDELTA_PROBE", "0")
    _, basis, w, s, z = _basis()
    rng = np.random.default_rng(npos)
    src = rng.integers(0, 256, npos + BS - 1, dtype=np.uint8)
    src[npos - 1:npos - 1 + BS] = basis[77 * BS:78 * BS]
    if npos - 1 >= BS:
        src[:BS] = basis[5000 * BS:5001 * BS]
    exp = O.ops_from_arrays(*O.C().generate_delta(src, w, s, z, BS))
    assert sum(k == "C" for k, _, _ in exp) == (2 if npos - 1 >= BS else 1)
    d, prof = _match(gpu, _dev(src), src.size)
    assert d.tuples() == exp
    assert d.stats["positions"] == npos
    assert "k_scan_r" in prof, prof


def test_segments(gpu, monkeypatch, level1):
    """SYDELTA_PROBE=1: the aligned probe first, then many short segments scanned on demand (a
    mixed source: a literal stretch, sparse substitutions, a shift, planted copies, an untouched
    stretch); a run never spans two segments."""
    monkeypatch.setenv("SYDELTA_PROBE", "1")
    _, basis, w, s, z = _basis()
    rng = np.random.default_rng(0x5E1D0822)
    q = 170 * BS
    a = basis[:q].copy()
    m = rng.random(q) < 0.05
    a[m] ^= rng.integers(1, 256, int(m.sum()), dtype=np.uint8)
    b = basis[q:3 * q].copy()
    for k in rng.choice(b.size // BS, b.size // BS // 10, replace=False):
        b[k * BS + rng.integers(0, BS)] ^= 0x5A
    c = basis[3 * q:4 * q]
    parts = [a, b, np.concatenate([c[:1000], rng.integers(0, 256, 17, dtype=np.uint8), c[1000:]])]
    for _ in range(60):
        parts.append(rng.integers(0, 256, int(rng.integers(1, 3 * BS)), dtype=np.uint8))
        k = int(rng.integers(0, NB))
        parts.append(basis[k * BS:(k + 1) * BS])
        if rng.random() < 0.3:
            parts.append(basis[k * BS:(k + 1) * BS])
    parts.append(basis[4 * q:5 * q])
    src = np.concatenate(parts)
    assert 3 << 20 < src.size < 5 << 20
    exp = O.ops_from_arrays(*O.C().generate_delta(src, w, s, z, BS))
    d, prof = _match(gpu, _dev(src), src.size)
    assert d.tuples() == exp
    assert d.stats["copy_ops"] > 500
    assert "k_scan_r" in prof, prof


def test_more_runs_than_waves(gpu, monkeypatch, level1):
    """(CUs x 12 + 5) runs and one tile more: an odd tile count, just over one run per wave of a
    launch of one workgroup of twelve waves per CU.  A literal source filled on the device with 64
    basis blocks planted off the grid: the analytic op list, and the oracle on 16 neighbourhoods."""
    import torch

    monkeypatch.setenv("SYDELTA_PROBE", "0")
    basis_t, _, w, s, z = _basis()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tiles = 2 * (cus * 12 + 5) + 1
    npos = tiles * TILE - 100  # (the last tile partial)
    n = npos + BS - 1
    src_t = torch.empty(n + 16, dtype=torch.uint8, device="cuda")
    gpu.synth_fill(src_t[:n], 0x5E1D0823)
    rng = np.random.default_rng(0x5E1D0824)
    # (slots from 1: the oracle's neighbourhoods start two blocks before a planted block)
    slots = np.sort(1 + rng.choice((n - 8 * BS) // (4 * BS), 64, replace=False))
    pos = [int(sl * 4 * BS + BS + rng.integers(1, BS)) for sl in slots]
    blks = [int(k) for k in rng.integers(0, NB, 64)]
    for p, k in zip(pos, blks):
        src_t[p:p + BS] = basis_t[k * BS:(k + 1) * BS]
    torch.cuda.synchronize()
    d, prof = _match(gpu, src_t, n)
    expect, lit = [], 0
    for p, k in zip(pos, blks):
        expect += [("D", lit, p - lit), ("C", k * BS, BS)]
        lit = p + BS
    expect.append(("D", lit, n - lit))
    assert d.tuples() == expect
    assert d.stats["positions"] == npos and d.stats["verified_hits"] == 64
    assert "k_scan_r" in prof, prof
    C = O.C()
    for p, k in list(zip(pos, blks))[:16]:
        lo, hi = p - 2 * BS, p + 3 * BS
        win = src_t[lo:hi].cpu().numpy()
        got = O.ops_from_arrays(*C.generate_delta(win, w, s, z, BS))
        assert got == [("D", 0, 2 * BS), ("C", k * BS, BS), ("D", 3 * BS, 2 * BS)], (p, k)
