"""The match call's preamble queues the copy-heavy sample's hashing before it waits for the
index (sydelta_match_device): what the sample decides must not move.  One copy-heavy and one
literal-heavy pair of 8 MiB at bs 4096, 16-byte-aligned sources: the first is still walked by
K10 as one chunk (k_walk_files), the second still scanned by the classifier, both samples still
run (k_probe_sample, k_probe), and both give the oracle's op list."""
import functools

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

BS = 4096
SIZE = 8 << 20


@functools.lru_cache(maxsize=None)
def _pairs():
    rng = np.random.default_rng(77)
    basis = rng.integers(0, 256, SIZE, dtype=np.uint8)
    heavy = basis.copy()  # copy-heavy: a few substituted bytes
    for p in rng.integers(0, SIZE, 40):
        heavy[p] ^= 0x5A
    literal = rng.integers(0, 256, SIZE, dtype=np.uint8)  # literal-heavy: three blocks of the basis, one off the grid
    literal[100 * BS:101 * BS] = basis[7 * BS:8 * BS]
    literal[900 * BS:901 * BS] = basis[8 * BS:9 * BS]
    literal[1500 * BS + 13:1501 * BS + 13] = basis[2000 * BS:2001 * BS]
    C = O.C()
    w, s, z = C.compute_checksums(basis, BS, threads=8)
    exp = {k: O.ops_from_arrays(*C.generate_delta(v, w, s, z, BS)) for k, v in (("heavy", heavy), ("literal", literal))}
    for a in (basis, heavy, literal):
        a.setflags(write=False)
    return basis, {"heavy": heavy, "literal": literal}, exp


@pytest.mark.parametrize("kind", ["heavy", "literal"])
def test_route_and_ops(gpu, monkeypatch, kind):
    import torch

    for k in ("SYDELTA_PROBE", "SYDELTA_CHUNK_WALK", "SYDELTA_SCAN_SMALL", "SYDELTA_DEVICE_WALK", "SYDELTA_L1",
              "SYDELTA_PHASE_PROBE"):
        monkeypatch.delenv(k, raising=False)
    basis, srcs, exp = _pairs()
    b = torch.from_numpy(basis.copy()).cuda()
    sd = torch.from_numpy(srcs[kind].copy()).cuda()
    assert sd.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    gpu.set_profiling(True)
    gpu.profile(reset=True)
    try:
        w, s = gpu.signature(b, BS)
        idx = gpu.Index(w, s, BS, BS)
        d = gpu.match(idx, sd)
        idx.close()
        prof = gpu.profile(reset=True)
    finally:
        gpu.set_profiling(False)
    assert d.tuples() == exp[kind]
    ncopy = sum(k == "C" for k, _, _ in exp[kind])
    assert ncopy == (3 if kind == "literal" else ncopy) and (kind == "literal" or ncopy > 2000)
    assert "k_probe_sample" in prof and "k_probe" in prof, prof  # both samples ran
    assert ("k_walk_files" in prof) == (kind == "heavy"), prof
    assert any(k.startswith("k_scan") for k in prof) == (kind == "literal"), prof
