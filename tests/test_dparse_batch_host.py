"""The batched Delta JSON parse (sydelta_delta_batch_from_json_device) without a GPU.

tests/csrc/dparse_batch_check.cpp, a stand-alone program built with g++ -fsanitize=address,
undefined, includes sy_amd/csrc/sydelta_dparsebatch.hpp and tests/csrc/dparse_wave.hpp and runs
what the entry point and its kernels run -- the plan, the tail body, count / place / parse per
file on the shared chunk table with the batch's ranks, the literal arena -- on host memory with
every array at its exact size, the files' stages in shuffled order, over texts from
delta_json_cases.py (written here):

* every small_accepted() text and the four density_cases() in one batch, in file order,
  reversed and shuffled, one text listed twice, the text arena at byte offsets 0, 1 and 7 (the
  texts at multiples of 16 and at odd offsets), the pad bytes spelling digits and commas, the
  literal arena at phases 0, 1 and 3 inside a 0xA5 guard: every file's ops and literal bytes
  equal those of its text parsed alone by the single call's steps, the packing rule holds, pads
  and guards are intact;
* every small_refused() text between two good files: its own status, the byte
  delta_json_ref.first_bad names, and both neighbours exact;
* a file ending in a Data op directly before one starting with a Data op; empty-ops texts
  first, last and adjacent.

A build with -DDPARSEB_PLANT_BUG (a Data op's a left relative to the batch's literals) must
fail the same run.

The entry point itself: an empty batch is OK without a device, every host refusal comes before
a device is touched and names its file, a valid batch on a machine without a GPU is
SYDELTA_E_NODEV (no CPU fallback)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import delta_json_cases as C
from delta_json_ref import compact, first_bad

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "build", "asan")

needs_toolchain = pytest.mark.skipif(shutil.which("g++") is None or
                                     not os.path.exists("/opt/rocm/include/hip/hip_runtime.h"),
                                     reason="needs g++ and the HIP headers")

U64_MAX = (1 << 64) - 1
E_INVAL, E_NODEV = -3, -1


def _build(name: str, extra=()) -> str:
    from test_host_sanitizers import FLAGS  # the host sanitizer builds' flags

    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, name)
    r = subprocess.run(["g++"] + FLAGS + list(extra) + ["-I" + os.path.join(ROOT, "tests", "csrc"),
                                                        os.path.join(ROOT, "tests", "csrc", "dparse_batch_check.cpp"),
                                                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def _run(exe: str, corpus_dir: str):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    return subprocess.run([exe, corpus_dir, "7"], capture_output=True, text=True, env=env, timeout=900)


def _refused():
    return {f"rej-{i}": t for i, t in enumerate(C.small_refused())}


@pytest.fixture(scope="module")
def corpus_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("dparse_batch")
    lines = []

    def put(name, kind, text):
        (d / f"{name}.json").write_bytes(text)
        lines.append(f"{name} {kind}")

    for i, (ops, n, bs) in enumerate(C.small_accepted()):
        put(f"acc-{i}", "ok", compact(ops, n, bs))
    for name, _, text in C.density_cases():
        put(name, "ok", text)
    put("tail-data", "ok", compact([("C", 0, 512), ("D", bytes(range(40, 140)))], 612, 512))
    put("head-data", "ok", compact([("D", bytes(range(200, 256)) * 2), ("C", 512, 512)], 624, 512))
    for name, text in _refused().items():
        put(name, "reject", text)
    (d / "manifest.txt").write_text("\n".join(lines) + "\n")
    return str(d)


@needs_toolchain
@pytest.mark.timeout(900)
def test_batch_stages_under_asan_ubsan(corpus_dir):
    r = _run(_build("dparse_batch_check"), corpus_dir)
    print(r.stdout[-3000:])
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-6000:])
    assert "dparse_batch_check ok" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    rejects = dict(re.findall(r"^reject (\S+): file 1: Delta JSON: not serde's compact form at byte (\d+)$", r.stdout, re.M))
    texts = _refused()
    assert sorted(rejects) == sorted(texts)
    for name, at in rejects.items():  # each refused at the byte the grammar names
        assert int(at) == first_bad(texts[name]), (name, at, texts[name])


@needs_toolchain
@pytest.mark.timeout(900)
def test_planted_bug_is_caught(corpus_dir):
    r = _run(_build("dparse_batch_check_bug", ["-DDPARSEB_PLANT_BUG"]), corpus_dir)
    assert r.returncode != 0
    assert "AddressSanitizer" in r.stderr or "FAIL " in r.stdout


def _call(lib, d_text, text_len, toff, tlen, n, d_lit=None, lit_len=0, need=None, tables=True, status=False, out=None):
    toff = np.asarray(toff, dtype=np.uint64)
    tlen = np.asarray(tlen, dtype=np.uint64)
    loff, llen, st = (np.zeros(max(n, 1), dtype=np.uint64) for _ in range(3))
    rc = lib.sydelta_delta_batch_from_json_device(
        0, d_text, text_len, toff.ctypes.data if tables else None, tlen.ctypes.data if tables else None, n, d_lit, lit_len,
        loff.ctypes.data, llen.ctypes.data, st.ctypes.data if status else None,
        ctypes.byref(need) if need is not None else None, ctypes.byref(out) if out is not None else None, None)
    return rc, (lib.sydelta_last_error() or b"").decode()


def test_empty_batch_needs_no_device():
    from sy_amd._lib import lib

    need = ctypes.c_uint64(77)
    out = ctypes.c_void_p()
    assert lib.sydelta_delta_batch_from_json_device(0, None, 0, None, None, 0, None, 0, None, None, None,
                                                    ctypes.byref(need), ctypes.byref(out), None) == 0
    assert need.value == 0 and out.value
    assert lib.sydelta_delta_batch_count(out) == 0
    lib.sydelta_delta_batch_free(out)
    need = ctypes.c_uint64(77)
    assert lib.sydelta_delta_batch_from_json_device(0, None, 0, None, None, 0, None, 0, None, None, None,
                                                    ctypes.byref(need), None, None) == 0
    assert need.value == 0


def test_refusals_come_before_any_device():
    """Every host refusal of the contract, on a machine with or without a GPU: SYDELTA_E_INVAL
    with the file named, never SYDELTA_E_NODEV."""
    from sy_amd._lib import lib

    need = ctypes.c_uint64(77)
    rc, msg = _call(lib, None, 0, [0] * 3, [0] * 3, 3, need=need, tables=False)
    assert rc == E_INVAL and "NULL table" in msg and need.value == 0
    rc, msg = _call(lib, None, 0, [0], [0], 1, need=None)
    assert rc == E_INVAL and "NULL lit_need" in msg
    A = 0x7000_0000_1001  # never dereferenced: the tables are refused first
    for d_text, text_len, toff, tlen, want in [
            (A, 100, [0, 16, 96], [10, 10, 5], "file 2: text [96, +5) leaves its arena of 100 bytes"),
            (A, 100, [0, 101], [10, 0], "file 1: text [101, +0) leaves its arena of 100 bytes"),
            (A, 100, [0, U64_MAX - 15], [10, 32], "file 1: text [18446744073709551600, +32) leaves its arena"),
            (A, 100, [0, 16], [10, U64_MAX], "file 1: text [16, +18446744073709551615) leaves its arena"),
            (None, 100, [0, 16], [0, 1], "file 1: NULL text arena")]:
        for status in (False, True):
            need = ctypes.c_uint64(77)
            out = ctypes.c_void_p(5)
            rc, msg = _call(lib, d_text, text_len, toff, tlen, len(toff), need=need, status=status, out=out)
            assert rc == E_INVAL and want in msg, (rc, msg, want)
            assert need.value == 0 and not out.value
    rc, msg = _call(lib, A, 100, [0], [10], 1, d_lit=None, lit_len=64, need=ctypes.c_uint64())
    assert rc == E_INVAL and "NULL literal arena of 64 bytes" in msg


def test_no_gpu_fails_loudly():
    """A valid batch without a GPU: SYDELTA_E_NODEV, never a CPU fallback.  (With a GPU the same
    batch of two texts of 3 bytes, each its file's refusal at byte 0 and no call error, is
    refused naming file 0.)"""
    import torch

    from sy_amd._lib import lib

    need = ctypes.c_uint64()
    if torch.cuda.is_available():
        buf = torch.zeros(16, dtype=torch.uint8, device="cuda")
        rc, msg = _call(lib, buf.data_ptr(), 16, [0, 3], [3, 3], 2, need=need)
        assert rc == E_INVAL and msg == "file 0: Delta JSON: not serde's compact form at byte 0"
    else:
        rc, _ = _call(lib, 0x7000_0000_1001, 16, [0, 3], [3, 3], 2, need=need)
        assert rc == E_NODEV
