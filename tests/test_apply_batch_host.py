"""The batched device apply (sydelta_apply_delta_batch_device) without a GPU.

tests/csrc/apply_batch_check.cpp, a stand-alone program built with g++ -fsanitize=address,
undefined, includes sy_amd/csrc/sydelta_applybatch.hpp and runs what the entry point and its
kernel run: the host plan (validation, merging, slices, the tile table) and the per-span copy
body, thread by thread, on host memory with every arena and every slice table allocated at
its exact size.  2000 seeded random batches (1..40 files, op sizes 0..200 KiB, random
alignments, contiguous and non-contiguous neighbours, every 400th batch with a file of more
runs than a slice holds) are compared with a byte loop over the ops; every refusal of the
contract must name its file and op.  The program exits non-zero on the first mismatch.

The entry point itself: an empty batch is OK without a device, a non-empty one on a machine
without a GPU is SYDELTA_E_NODEV (no CPU fallback)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sy_amd", "csrc")
OUT = os.path.join(ROOT, "build", "asan")
FLAGS = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
         "-I" + os.path.join(ROOT, "include"), "-I" + CSRC]

REFUSALS = ["file 13: op 77: Copy{offset 4991, size 10} past the end of the basis",
            "file 13: op 77: Copy{offset 18446744073709551615, size 2} past the end of the basis",
            "file 13: op 77: Data [4988, +10) outside the literal range",
            "file 13: op 77: Data [18446744073709551614, +5) outside the literal range",
            "file 13: op 77: unknown kind",
            "file 13: op 99: output needs more than its capacity",
            "file 19: basis range", "file 4: basis range", "file 19: literal range", "file 6: literal range",
            "file 19: output range", "file 0: output range", "file 9: NULL delta",
            "file 5: op 3: Data"]


@pytest.mark.timeout(900)
@pytest.mark.skipif(shutil.which("g++") is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime.h"),
                    reason="needs g++ and the HIP headers")
def test_plan_and_span_copy_under_asan_ubsan():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "apply_batch_check")
    r = subprocess.run(["g++"] + FLAGS + [os.path.join(ROOT, "tests", "csrc", "apply_batch_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, "2000", "7"], capture_output=True, text=True, env=env, timeout=800)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-6000:])
    assert "apply_batch_check ok: 2000 batches" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    rejects = [ln[len("reject "):] for ln in r.stdout.splitlines() if ln.startswith("reject ")]
    for want in REFUSALS:  # each refused for its own reason, naming its file and op
        assert any(ln.startswith(want) for ln in rejects), (want, rejects)


def _empty_delta(lib):
    h = lib.sydelta_delta_from_ops(None, 0, 0, 4096)
    assert h
    return h


def test_empty_batch_needs_no_device():
    from sy_amd._lib import DeltaStatsC, lib

    tot = DeltaStatsC(1, 2, 3)
    assert lib.sydelta_apply_delta_batch_device(0, None, 0, None, None, None, None, 0, None, None, None, 0, None, None,
                                                0, None, None, ctypes.byref(tot)) == 0
    assert (tot.operations_count, tot.literal_bytes, tot.bytes_written) == (0, 0, 0)
    assert lib.sydelta_delta_batch_ptrs(None, None, 0) == 0


def test_null_tables_are_invalid():
    from sy_amd._lib import lib

    assert lib.sydelta_apply_delta_batch_device(0, None, 0, None, None, None, None, 0, None, None, None, 0, None, None,
                                                3, None, None, None) == -3
    assert b"NULL table" in lib.sydelta_last_error()


def test_no_gpu_fails_loudly():
    """A non-empty batch without a GPU: SYDELTA_E_NODEV, never a CPU fallback (with a GPU the
    same batch of one empty delta is applied: OK, nothing written)."""
    import torch

    from sy_amd._lib import DeltaStatsC, lib

    h = _empty_delta(lib)
    try:
        z = np.zeros(1, dtype=np.uint64)
        ptrs = (ctypes.c_void_p * 1)(h)
        st = DeltaStatsC()
        rc = lib.sydelta_apply_delta_batch_device(0, None, 0, z.ctypes.data, z.ctypes.data, ptrs, None, 0, z.ctypes.data,
                                                  z.ctypes.data, None, 0, z.ctypes.data, z.ctypes.data, 1, None,
                                                  ctypes.byref(st), None)
    finally:
        lib.sydelta_delta_free(h)
    assert rc == (0 if torch.cuda.is_available() else -1)
