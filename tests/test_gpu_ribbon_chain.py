"""The chain in front of a level-1 scan: the ribbon's counts cleared by one
kernel and its words by nothing, k_ribbon_list loading a thread's keys together, the scan extras
queued on the stream that built the index, and the copy-heavy sample's lookups queued behind a
device-side wait for the collision build (they read no table if that build overflowed).

Two bases of 16 392 blocks at bs 4096 (the smallest that take the level-1 path: a few blocks above
kLdsFilterKeys), filled on the device and signed by the C oracle; SYDELTA_L1=ribbon forces the
ribbon at this size.  Every op list is compared with the C oracle's on the whole source, under
each of the three points the ribbon is started at (SYDELTA_EARLY_RIBBON)."""
import functools

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

BS = 4096
NB = 16384 + 8  # > kLdsFilterKeys blocks: k_scan_r with a level-1 filter
_KNOBS = ("SYDELTA_PROBE", "SYDELTA_SCAN_SMALL", "SYDELTA_CHUNK_WALK", "SYDELTA_DEVICE_WALK", "SYDELTA_L1",
          "SYDELTA_PHASE_PROBE", "SYDELTA_EARLY_RIBBON")


@pytest.fixture(params=["0", "1", "2"])
def early(request, monkeypatch):
    for k in _KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SYDELTA_L1", "ribbon")
    monkeypatch.setenv("SYDELTA_EARLY_RIBBON", request.param)
    return request.param


def _dev(a):
    import torch

    t = torch.zeros(a.size + 16, dtype=torch.uint8, device="cuda")
    t[:a.size] = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t


def _planted(basis, blocks, rng):
    """Random bytes with the given basis blocks behind gaps of 1..3 blocks (any byte count)."""
    parts = []
    for t in blocks:
        parts.append(rng.integers(0, 256, int(rng.integers(BS, 3 * BS + 1)), dtype=np.uint8))
        parts.append(basis[t * BS:(t + 1) * BS])
    parts.append(rng.integers(0, 256, BS + 5, dtype=np.uint8))
    return np.concatenate(parts)


@functools.lru_cache(maxsize=None)
def _world():
    """Both bases (device tensor, signature), their sources and the oracle's op lists; made once."""
    import torch

    import sy_amd.device as dev

    C = O.C()
    out = {}
    for name, seed, nplant in (("A", 0x5E1D0801, 512), ("B", 0x5E1D0802, 64)):
        t = torch.empty(NB * BS + 16, dtype=torch.uint8, device="cuda")
        dev.synth_fill(t[:NB * BS], seed)
        torch.cuda.synchronize()
        basis = t[:NB * BS].cpu().numpy()
        w, s, z = C.compute_checksums(basis, BS, threads=8)
        rng = np.random.default_rng(seed)
        blocks = [int(b) for b in rng.choice(NB, nplant, replace=False)]
        src = {"planted": _planted(basis, blocks, rng)}
        if name == "A":
            # literal-heavy for the sample: one basis block in every 8, never on the 1-in-16 grid
            lit = rng.integers(0, 256, 8 << 20, dtype=np.uint8)
            for k in range(3, lit.size // BS, 8):
                lit[k * BS:(k + 1) * BS] = basis[(5 * k + 1) * BS:(5 * k + 2) * BS]
            heavy = basis[:8 << 20].copy()
            for p in rng.integers(0, heavy.size, 40):
                heavy[p] ^= 0x5A
            src["literal"], src["heavy"] = lit, heavy
        exp = {k: O.ops_from_arrays(*C.generate_delta(v, w, s, z, BS)) for k, v in src.items()}
        assert sum(k == "C" for k, _, _ in exp["planted"]) == nplant
        for a in (basis, w, s, z, *src.values()):
            a.setflags(write=False)
        out[name] = {"t": t[:NB * BS], "w": w, "s": s, "z": z, "src": src, "exp": exp,
                     "dsrc": {k: _dev(v) for k, v in src.items()}}
    torch.cuda.synchronize()
    return out


def _index(gpu, B):
    import torch

    dw = torch.from_numpy(B["w"].view(np.int32).copy()).cuda()
    ds = torch.from_numpy(B["s"].view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    return gpu.Index(dw, ds, BS, BS)


def _match(gpu, idx, B, kind, stream=None):
    """One match, and the kernels that ran since the profile was last read."""
    d = gpu.match(idx, B["dsrc"][kind], stream=stream, length=B["src"][kind].size)
    return d.tuples(), gpu.profile(reset=True)


@pytest.fixture
def profiled(gpu):
    gpu.set_profiling(True)
    gpu.profile(reset=True)
    yield gpu
    gpu.set_profiling(False)


def _recycled(gpu, W):
    """Index A, a match, close; index B of the same size takes A's pool; three times over: a
    stale count or key list of the pool's previous ribbon would lose or invent a Copy."""
    for _ in range(3):
        for name in ("A", "B"):
            gpu.profile(reset=True)
            idx = _index(gpu, W[name])
            got, prof = _match(gpu, idx, W[name], "planted")
            idx.close()
            assert got == W[name]["exp"]["planted"], name
            assert "k_ribbon_build" in prof and "k_scan_r" in prof, prof


def test_recycled_pool_every_key(profiled, monkeypatch, early):
    """SYDELTA_PROBE=0: every position goes through the scan, so a key the ribbon's lists lost
    (A's source holds 512 distinct basis blocks off the grid) loses its Copy."""
    monkeypatch.setenv("SYDELTA_PROBE", "0")
    W = _world()
    gpu = profiled
    idx = _index(gpu, W["A"])
    got, prof = _match(gpu, idx, W["A"], "planted")
    idx.close()
    assert got == W["A"]["exp"]["planted"]
    assert "k_ribbon_build" in prof and "k_scan_r" in prof, prof
    _recycled(gpu, W)


def test_sampled_route(profiled, early):
    """SYDELTA_PROBE unset: the sample's lookups wait for the build on the device.  A literal
    source goes to the classifier, a copy-heavy one on the same index to K10, and the literal
    one again finds ribbon and extras built."""
    W = _world()
    gpu = profiled
    A = W["A"]
    gpu.profile(reset=True)
    idx = _index(gpu, A)
    got, prof = _match(gpu, idx, A, "literal")
    assert got == A["exp"]["literal"]
    assert "k_ribbon_build" in prof and "k_scan_r" in prof and "k_walk_files" not in prof, prof
    assert "k_probe_sample" in prof and "k_idx_extras" in prof, prof
    got, prof = _match(gpu, idx, A, "heavy")
    assert got == A["exp"]["heavy"]
    assert "k_walk_files" in prof and "k_scan_r" not in prof, prof
    got, prof = _match(gpu, idx, A, "literal")
    idx.close()
    assert got == A["exp"]["literal"]
    assert "k_scan_r" in prof and "k_ribbon_build" not in prof and "k_idx_extras" not in prof, prof


def test_created_never_matched(profiled, monkeypatch, early):
    """An index whose ribbon was started at creation (SYDELTA_EARLY_RIBBON=2) is closed without
    a match; its pool goes on to the next indexes."""
    monkeypatch.setenv("SYDELTA_PROBE", "0")
    W = _world()
    gpu = profiled
    _index(gpu, W["A"]).close()
    _recycled(gpu, W)


def test_second_stream(profiled, monkeypatch, early):
    """The same index matched from the library's stream, then from a stream of the caller's:
    the second scan is ordered after ribbon and extras by their events."""
    import torch

    monkeypatch.setenv("SYDELTA_PROBE", "0")
    W = _world()
    gpu = profiled
    A = W["A"]
    idx = _index(gpu, A)
    got, prof = _match(gpu, idx, A, "planted")
    assert got == A["exp"]["planted"]
    assert "k_ribbon_build" in prof and "k_scan_r" in prof, prof
    st = torch.cuda.Stream()
    got, prof = _match(gpu, idx, A, "planted", stream=st)
    st.synchronize()
    idx.close()
    assert got == A["exp"]["planted"]
    assert "k_scan_r" in prof and "k_ribbon_build" not in prof, prof


def test_collision_overflow_sampled(profiled, early):
    """A collision list one entry over its region (the construction of
    tests/test_gpu_index_collisions.py: 20 000 random blocks, pairs of blocks given one weak value,
    4097 entries against a region of 4096) with the sample on: the sample's lookups and pre-roll,
    queued behind the build before its flag was read, read no table; the sort build runs and they
    run again."""
    import torch

    gpu = profiled
    bs, n, cap = 256, 20000, 4096
    rng = np.random.default_rng(1256)
    data = rng.integers(0, 256, n * bs, dtype=np.uint8)
    C = O.C()
    w, s, z = C.compute_checksums(data, bs, threads=8)
    assert len(np.unique(w)) == n
    perm = [int(x) for x in rng.permutation(n)[:cap + 1]]
    runs = [sorted(perm[:3])] + [sorted(perm[i:i + 2]) for i in range(3, cap + 1, 2)]
    for m in runs:
        for j in m[:-1]:
            w[j] = w[m[-1]]
    _, c = np.unique(w, return_counts=True)
    assert int(c[c >= 2].sum()) == cap + 1
    parts = []
    for t in [m[-1] for m in runs[:40]]:
        parts.append(rng.integers(0, 256, int(rng.integers(3 * bs, 9 * bs)), dtype=np.uint8))
        parts.append(data[t * bs:(t + 1) * bs])
    parts.append(rng.integers(0, 256, 2 * bs + 11, dtype=np.uint8))
    src = np.concatenate(parts)
    exp = O.ops_from_arrays(*C.generate_delta(src, w, s, z, bs))
    assert sum(k == "C" for k, _, _ in exp) == 40
    dw = torch.from_numpy(w.view(np.int32).copy()).cuda()
    ds = torch.from_numpy(s.view(np.int64).copy()).cuda()
    sd = _dev(src)
    assert sd.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    gpu.profile(reset=True)
    idx = gpu.Index(dw, ds, bs, bs)
    d = gpu.match(idx, sd, length=src.size)
    idx.close()
    prof = gpu.profile(reset=True)
    assert d.tuples() == exp
    assert "k_idx_order" in prof and "k_probe_sample" in prof, prof


def test_bloom_after_ribbon(profiled, oracle_c, monkeypatch):
    """An index of 852 008 blocks (the ribbon by default from kRibMinKeys = 852 000) scanned first over
    2^31 + 8192 positions -- the ribbon, so the extras are queued without the Bloom -- and then
    over a 4 MiB source, below kRibMinScan: that scan reads the Bloom and has to fill it first.
    The sizes are the smallest at which this path exists (an index that chooses between the two
    filters per scan has at least kRibMinKeys blocks, and the first scan takes the ribbon only
    from kRibMinScan = 2^31 positions): ~5.5 GB of device memory, filled and signed on the device;
    the case takes ~0.25 s."""
    import torch

    for k in _KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SYDELTA_PROBE", "0")
    gpu = profiled
    nb = 852000 + 8
    basis_t = torch.empty(nb * BS + 16, dtype=torch.uint8, device="cuda")
    gpu.synth_fill(basis_t[:nb * BS], 0x5E1D0811)
    n1 = (1 << 31) + 8192 + BS - 1
    src1 = torch.empty(n1 + 16, dtype=torch.uint8, device="cuda")
    gpu.synth_mutate(src1[:n1], basis_t[:n1], 0x5E1D0812, 50000)
    rng = np.random.default_rng(0x5E1D0813)
    blks = [int(b) for b in rng.choice(nb, 8, replace=False)]
    small = rng.integers(0, 256, 4 << 20, dtype=np.uint8)
    pos = [int(k * 100 * BS + rng.integers(1, BS)) for k in range(1, 9)]
    for p, b in zip(pos, blks):
        small[p:p + BS] = basis_t[b * BS:(b + 1) * BS].cpu().numpy()
    small_t = _dev(small)
    w, s = gpu.signature(basis_t[:nb * BS], BS)
    torch.cuda.synchronize()
    gpu.profile(reset=True)
    idx = gpu.Index(w, s, BS, BS)
    d1 = gpu.match(idx, src1, length=n1)
    prof1 = gpu.profile(reset=True)
    d2 = gpu.match(idx, small_t, length=small.size)
    prof2 = gpu.profile(reset=True)
    idx.close()
    assert "k_ribbon_build" in prof1 and "k_scan_r" in prof1 and "k_idx_extras" in prof1, prof1
    assert d1.stats["positions"] == n1 - BS + 1
    assert "k_scan_r" in prof2 and "k_idx_extras" in prof2 and "k_ribbon_build" not in prof2, prof2
    hw = w.cpu().numpy().view(np.uint32)
    hs = s.cpu().numpy().view(np.uint64)
    hz = np.full(nb, BS, np.uint64)
    exp = O.ops_from_arrays(*oracle_c.generate_delta(small, hw, hs, hz, BS))
    assert sum(k == "C" for k, _, _ in exp) == 8
    assert d2.tuples() == exp
