"""The batched Delta JSON writer (sydelta_delta_batch_to_json_device) without a GPU.

tests/csrc/json_batch_check.cpp, a stand-alone program built with g++ -fsanitize=address,
undefined, includes sy_amd/csrc/sydelta_jsonbatch.hpp and runs what the entry point and its
kernels run: the host plan (validation, tiles, slices) and the per-lane sizing and per-thread
writing bodies, on host memory with the literal arena, the output arena and every table
allocated at their exact sizes.  2000 seeded random batches (1..40 files, 0..600 ops per file,
Data sizes 0..20 000, Copy fields at the digit-class edges, random literal and output
alignments, every 200th batch with a file that spans table slices) are compared with a plain
writer in the program; every refusal of the contract must name its file and op.  The program
exits non-zero on the first mismatch.

The entry point itself: an empty batch is OK without a device, NULL tables are invalid, a
non-empty batch on a machine without a GPU is SYDELTA_E_NODEV (no CPU fallback).  The bound
(pure host code) covers the packed size of the host writer's texts."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sy_amd", "csrc")
OUT = os.path.join(ROOT, "build", "asan")
FLAGS = ["-std=c++17", "-O2", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
         "-I" + os.path.join(ROOT, "include"), "-I" + CSRC]

REFUSALS = ["file 13: op 77: Data [4988, +10) outside the literal range",
            "file 13: op 77: Data [4998, +0) outside the literal range",
            "file 13: op 77: Data [18446744073709551614, +5) outside the literal range",
            "file 13: op 77: Data [5, +18446744073709551614) outside the literal range",
            "file 13: op 77: unknown kind",
            "file 19: literal range", "file 6: literal range", "file 9: NULL delta",
            "file 5: op 3: Data"]

_OP_DTYPE = np.dtype([("kind", "<u4"), ("reserved", "<u4"), ("a", "<u8"), ("b", "<u8")])
U64_MAX = (1 << 64) - 1


@pytest.mark.timeout(900)
@pytest.mark.skipif(shutil.which("g++") is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime.h"),
                    reason="needs g++ and the HIP headers")
def test_plan_and_tile_bodies_under_asan_ubsan():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "json_batch_check")
    r = subprocess.run(["g++"] + FLAGS + [os.path.join(ROOT, "tests", "csrc", "json_batch_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, "2000", "7"], capture_output=True, text=True, env=env, timeout=800)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-6000:])
    assert "json_batch_check ok: 2000 batches" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    rejects = [ln[len("reject "):] for ln in r.stdout.splitlines() if ln.startswith("reject ")]
    for want in REFUSALS:  # each refused for its own reason, naming its file and op
        assert any(ln.startswith(want) for ln in rejects), (want, rejects)


def test_empty_batch_needs_no_device():
    from sy_amd._lib import lib

    need = ctypes.c_uint64(77)
    assert lib.sydelta_delta_batch_to_json_device(0, None, 0, None, 0, None, None, None, 0, None, None,
                                                  ctypes.byref(need), None) == 0
    assert need.value == 0
    assert lib.sydelta_delta_batch_to_json_bound(None, 0) == 0


def test_null_tables_are_invalid():
    from sy_amd._lib import lib

    need = ctypes.c_uint64(77)
    assert lib.sydelta_delta_batch_to_json_device(0, None, 3, None, 0, None, None, None, 0, None, None,
                                                  ctypes.byref(need), None) == -3
    assert b"NULL table" in lib.sydelta_last_error()
    assert need.value == 0
    assert lib.sydelta_delta_batch_to_json_bound(None, 3) == U64_MAX


def test_no_gpu_fails_loudly():
    """A non-empty batch without a GPU: SYDELTA_E_NODEV, never a CPU fallback (with a GPU the
    same batch of one delta without ops is sized: 41 characters, nothing written)."""
    import torch

    from sy_amd._lib import lib

    h = lib.sydelta_delta_from_ops(None, 0, 0, 4096)
    assert h
    try:
        z = np.zeros(1, dtype=np.uint64)
        to, tl = np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint64)
        ptrs = (ctypes.c_void_p * 1)(h)
        need = ctypes.c_uint64()
        rc = lib.sydelta_delta_batch_to_json_device(0, ptrs, 1, None, 0, z.ctypes.data, z.ctypes.data, None, 0,
                                                    to.ctypes.data, tl.ctypes.data, ctypes.byref(need), None)
    finally:
        lib.sydelta_delta_free(h)
    if torch.cuda.is_available():
        assert rc == 0 and need.value == len(b'{"ops":[],"source_size":0,"block_size":4096}') == int(tl[0])
    else:
        assert rc == -1


def test_bound_covers_the_host_writers_packed_size():
    """sydelta_delta_batch_to_json_bound against the lengths sydelta_delta_to_json reports for
    random deltas (literal bytes of every digit class), packed at multiples of 16."""
    from sy_amd._lib import lib

    rng = np.random.default_rng(20)
    edges = [0, 9, 10, 99, 100, 10**9 - 1, 10**9, (1 << 32) - 1, 1 << 32, 10**19 - 1, 10**19, U64_MAX]
    for trial in range(40):
        nfiles = int(rng.integers(1, 12))
        hs, packed = [], 0
        try:
            for f in range(nfiles):
                nops = int(rng.integers(0, 60))
                lit = rng.integers(0, 256 if trial % 3 else 10, int(rng.integers(0, 3000)), dtype=np.uint8)
                if trial % 5 == 0:
                    lit[:] = 255
                ops = np.zeros(nops, dtype=_OP_DTYPE)
                for i in range(nops):
                    if rng.integers(0, 2):
                        ops[i] = (0, 0, edges[int(rng.integers(0, len(edges)))], edges[int(rng.integers(0, len(edges)))])
                    else:
                        b = int(rng.integers(0, len(lit) + 1))
                        ops[i] = (1, 0, int(rng.integers(0, len(lit) - b + 1)), b)
                ss, bs = edges[int(rng.integers(0, len(edges)))], edges[int(rng.integers(0, len(edges)))]
                h = lib.sydelta_delta_from_ops(ops.ctypes.data if nops else None, nops, ss, bs)
                assert h
                hs.append(h)
                n = ctypes.c_uint64()
                lp = lit.ctypes.data if lit.size else ctypes.c_void_p(1)
                assert lib.sydelta_delta_to_json(h, lp, lit.size, None, 0, ctypes.byref(n)) == 0
                packed = ((packed + 15) & ~15) + n.value
            ptrs = (ctypes.c_void_p * nfiles)(*hs)
            bound = lib.sydelta_delta_batch_to_json_bound(ptrs, nfiles)
            assert packed <= bound < U64_MAX
            assert bound <= 8 * packed + 64 * nfiles  # a bound, not a guess: at most 4 characters per literal byte
            ptrs[nfiles // 2] = None
            assert lib.sydelta_delta_batch_to_json_bound(ptrs, nfiles) == U64_MAX
        finally:
            for h in hs:
                lib.sydelta_delta_free(h)
