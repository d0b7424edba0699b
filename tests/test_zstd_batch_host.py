"""The batched zstd compressor (sydelta_zstd_compress_batch_device) without a GPU.

tests/csrc/zstd_batch_check.cpp, a stand-alone program built with g++ -fsanitize=address,
undefined together with the reference encoder tests/csrc/zstd_ref.cpp, includes
sy_amd/csrc/sydelta_zstdbatch.hpp and runs what the entry point and its kernels run: the host
plan (validation, the per-file block table), the bisection that finds a block's file, the
sequential form of the block coder, the per-round placement (placed lengths, scan, carried
base) and the per-thread placement body, on host memory with every arena and table allocated at
its exact size.  The packed arena must equal the frames built file by file, for rounds of 1, 3
and all blocks: empty texts first, last and adjacent, lengths 1, 1023, 1024, 128 KiB - 1,
128 KiB, 128 KiB + 1 and 3 x 128 KiB, files whose blocks straddle rounds, then seeded random
batches.  A too-small arena keeps the sizes and leaves the guard region behind it intact; every
refusal of the contract names its file.  The program exits non-zero on the first mismatch.

The entry point itself: an empty batch is OK without a device, NULL tables and every bad table
entry are refused before a device is touched, a valid batch on a machine without a GPU is
SYDELTA_E_NODEV (no CPU fallback).  The bound is the sum of the single frames' bounds."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import test_zstd as Z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sy_amd", "csrc")
OUT = os.path.join(ROOT, "build", "asan")
FLAGS = ["-std=c++17", "-O2", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
         "-I" + os.path.join(ROOT, "include"), "-I" + CSRC]

REFUSALS = ["the input arena must be 16-byte aligned",
            "file 2: text offset 40 is not a multiple of 16",
            "file 2: text [96, +5) leaves its arena of 100 bytes",
            "file 1: text [112, +0) leaves its arena of 100 bytes",
            "file 1: text [18446744073709551600, +32) leaves its arena",
            "file 3: text [48, +18446744073709551615) leaves its arena",
            "file 1: NULL input arena"]

U64_MAX = (1 << 64) - 1
E_INVAL, E_NODEV = -3, -1


@pytest.mark.timeout(600)
@pytest.mark.skipif(shutil.which("g++") is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime.h"),
                    reason="needs g++ and the HIP headers")
def test_plan_rounds_and_placement_under_asan_ubsan():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "zstd_batch_check")
    srcs = [os.path.join(ROOT, "tests", "csrc", f) for f in ("zstd_batch_check.cpp", "zstd_ref.cpp")]
    r = subprocess.run(["g++"] + FLAGS + srcs + ["-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, "8", "7"], capture_output=True, text=True, env=env, timeout=500)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-6000:])
    assert "zstd_batch_check ok: 10 batches" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    rejects = [ln[len("reject "):] for ln in r.stdout.splitlines() if ln.startswith("reject ")]
    for want in REFUSALS:  # each refused for its own reason, naming its file
        assert any(ln.startswith(want) for ln in rejects), (want, rejects)


def _call(lib, d_in, in_len, toff, tlen, n, d_out=None, out_len=0, need=None, tables=True):
    toff = np.asarray(toff, dtype=np.uint64)
    tlen = np.asarray(tlen, dtype=np.uint64)
    foff, flen = np.zeros(max(n, 1), dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint64)
    rc = lib.sydelta_zstd_compress_batch_device(
        0, d_in, in_len, toff.ctypes.data if tables else None, tlen.ctypes.data if tables else None, n, d_out, out_len,
        foff.ctypes.data, flen.ctypes.data, ctypes.byref(need) if need is not None else None, None)
    return rc, (lib.sydelta_last_error() or b"").decode()


def test_empty_batch_needs_no_device():
    from sy_amd._lib import lib

    need = ctypes.c_uint64(77)
    assert lib.sydelta_zstd_compress_batch_device(0, None, 0, None, None, 0, None, 0, None, None, ctypes.byref(need),
                                                  None) == 0
    assert need.value == 0
    assert lib.sydelta_zstd_batch_bound(None, 0) == 0


def test_refusals_come_before_any_device():
    """Every refusal of the contract, on a machine with or without a GPU: SYDELTA_E_INVAL with
    the file named, never SYDELTA_E_NODEV."""
    from sy_amd._lib import lib

    need = ctypes.c_uint64(77)
    rc, msg = _call(lib, None, 0, [0] * 3, [0] * 3, 3, need=need, tables=False)
    assert rc == E_INVAL and "NULL table" in msg and need.value == 0
    rc, msg = _call(lib, None, 0, [0], [0], 1, need=None)
    assert rc == E_INVAL and "NULL out_need" in msg
    A = 0x7000_0000_1000  # never dereferenced: the tables are refused first
    for d_in, in_len, toff, tlen, want in [
            (A + 8, 100, [0], [10], "16-byte aligned"),
            (A, 100, [0, 16, 40], [10, 10, 10], "file 2: text offset 40 is not a multiple of 16"),
            (A, 100, [0, 16, 96], [10, 10, 5], "file 2: text [96, +5) leaves its arena of 100 bytes"),
            (A, 100, [0, U64_MAX - 15], [10, 32], "file 1: text ["),
            (A, 100, [0, 16], [10, U64_MAX], "file 1: text ["),
            (None, 100, [0, 16], [0, 1], "file 1: NULL input arena")]:
        need = ctypes.c_uint64(77)
        rc, msg = _call(lib, d_in, in_len, toff, tlen, len(toff), need=need)
        assert rc == E_INVAL and want in msg, (rc, msg, want)
        assert need.value == 0
    rc, msg = _call(lib, A, 100, [0], [10], 1, d_out=None, out_len=64, need=ctypes.c_uint64())
    assert rc == E_INVAL and "NULL output arena" in msg


def test_no_gpu_fails_loudly():
    """A valid batch without a GPU: SYDELTA_E_NODEV, never a CPU fallback (with a GPU the same
    batch of two empty texts is sized: two frames of 17 bytes, nothing written)."""
    import torch

    from sy_amd._lib import lib

    need = ctypes.c_uint64()
    rc, _ = _call(lib, None, 0, [0, 0], [0, 0], 2, need=need)
    if torch.cuda.is_available():
        assert rc == 0 and need.value == 34
    else:
        assert rc == E_NODEV


def test_bound_is_the_sum_of_the_frame_bounds():
    from sy_amd._lib import lib

    rng = np.random.default_rng(3)
    K = 128 << 10
    lens = [0, 1, 1023, 1024, K - 1, K, K + 1, 3 * K, 3 * K + 1, 1 << 40] + [int(x) for x in rng.integers(0, 1 << 22, 50)]
    for n in (1, 2, 7, len(lens)):
        arr = np.array(lens[:n], dtype=np.uint64)
        want = sum(Z.frame_bound(x) for x in lens[:n])
        assert lib.sydelta_zstd_batch_bound(arr.ctypes.data, n) == want
        assert want == sum(int(lib.sydelta_zstd_bound(x)) for x in lens[:n])
    assert lib.sydelta_zstd_batch_bound(None, 4) == U64_MAX
    for bad in ([U64_MAX - 100, 5], [U64_MAX // 2, U64_MAX // 2, 1 << 20], [U64_MAX]):
        arr = np.array(bad, dtype=np.uint64)
        assert lib.sydelta_zstd_batch_bound(arr.ctypes.data, len(bad)) == U64_MAX
