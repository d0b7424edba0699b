"""The batched zstd decoder (sydelta_zstd_decompress_batch_device) without a GPU.

tests/csrc/unzstd_batch_check.cpp, a stand-alone program built with g++ -fsanitize=address,
undefined and linked to the system libzstd as unzstd_check.cpp is, includes
sy_amd/csrc/sydelta_unzstdbatch.hpp and runs what the entry point and its kernels run, thread
by thread in shuffled orders, on host memory with every array at its exact size, over batches
cut from the corpus directory of test_unzstd_host.py (the same files, written here):

* the whole corpus (libzstd s1, s3, s19 and o3, our encoder's frames, the hand frames) in one
  batch, in file order, reversed and shuffled, the frame arena at byte offsets 0, 1 and 7, the
  text arena in a guard buffer (0xA5, the pad bytes poisoned): every text equals the decode of
  its frame alone, the packing rule holds, pads and guards are intact, and an arena one byte
  short gets the same sizes and no byte;
* every entry of F.malformed() in the middle of three good frames: its own status and reason,
  text_len 0, its neighbours exact; with the status table absent the call's error names it and
  nothing is written (the whole arena is poisoned);
* first-block-treeless and first-block-repeat-mode directly behind a frame that defines such
  tables, ll0-offset-before-start directly behind a non-empty text: refused, each;
* empty texts first, last and adjacent; 1, 64, 65 and 200 files;
* the 4 GiB arena limit from two frames of 16 384 RLE blocks of 128 KiB, as a size query: each
  alone is 2 GiB, together they are refused before any scratch is sized;
* seeded mutants between two good frames: never a sanitizer report, and a file's result in the
  batch (status, or bytes) is its result alone.

A build with -DUNZSTDB_PLANT_BUG (the offset check made arena-relative) must fail the same run.

The entry point itself: an empty batch is OK without a device, every host refusal comes before
a device is touched and names its file, a valid batch on a machine without a GPU is
SYDELTA_E_NODEV (no CPU fallback)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import zstd_frames as F
from test_unzstd_host import FORMS_OK, FORMS_REJECT
from test_zstd import _libzstd, ref_compress

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "build", "asan")
MUTANTS = 3  # per frame: the run stays in the order of unzstd_check's

needs_toolchain = pytest.mark.skipif(shutil.which("g++") is None or _libzstd() is None or
                                     not os.path.exists("/opt/rocm/include/hip/hip_runtime.h"),
                                     reason="needs g++, the HIP headers and the system libzstd")

U64_MAX = (1 << 64) - 1
E_INVAL, E_NODEV = -3, -1


def _build(name: str, extra=()) -> str:
    from test_host_sanitizers import FLAGS  # the host sanitizer builds' flags

    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, name)
    r = subprocess.run(["g++"] + FLAGS + list(extra) + [os.path.join(ROOT, "tests", "csrc", "unzstd_batch_check.cpp"),
                                                        F.libzstd_path(), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def _run(exe: str, corpus_dir: str, mutants: int):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    return subprocess.run([exe, corpus_dir, str(mutants), "7"], capture_output=True, text=True, env=env, timeout=1500)


@pytest.fixture(scope="module")
def corpus_dir(tmp_path_factory):
    """The files test_unzstd_host.py's fixture writes."""
    d = tmp_path_factory.mktemp("unzstd_batch")
    lines = []

    def put(name, kind, frame, data=None):
        (d / f"{name}.frame").write_bytes(frame)
        if data is not None:
            (d / f"{name}.out").write_bytes(data)
        lines.append(f"{name} {kind}")

    for name, (frame, data) in F.corpus().items():
        put(name, "ok", frame, data)
    for name, data in F.own_texts():
        put(f"own-{name}", "ok", ref_compress(data), data)
    for name, (frame, data) in F.hand_frames().items():
        put(name, "ok", frame, data)
    for name, frame in F.malformed().items():
        put(name, "reject", frame)
    # the assembled families test_unzstd_host.py mutates, and the ones it has refused: each
    # refused one, a twin one byte short of its offset among them, between good frames
    for name in FORMS_OK:
        frame, ops = F.form(name)
        put(name, "ok", frame, F.expect(ops).tobytes())
    for name in FORMS_REJECT:
        put(name, "reject", F.form_refused(name))
    (d / "manifest.txt").write_text("\n".join(lines) + "\n")
    return str(d)


@needs_toolchain
@pytest.mark.timeout(1800)
def test_batch_stages_under_asan_ubsan(corpus_dir):
    r = _run(_build("unzstd_batch_check"), corpus_dir, MUTANTS)
    print(r.stdout[-3000:])
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-6000:])
    assert "unzstd_batch_check ok" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    rejects = {ln.split()[1].rstrip(":"): ln for ln in r.stdout.splitlines() if ln.startswith("reject ")}
    forms = {name: rejects.pop(name) for name in FORMS_REJECT}
    assert sorted(rejects) == sorted(F.malformed()) == sorted(F.MALFORMED_REASON)
    for name, line in rejects.items():  # each refused for its own reason, its file named
        assert "file 1: zstd frame: block " in line and F.MALFORMED_REASON[name] in line, line
    for name, line in forms.items():
        assert "file 1: zstd frame: " + F.FORMS_REFUSED[name] in line, line
    limit = [ln for ln in r.stdout.splitlines() if ln.startswith("limit: ")]
    assert len(limit) == 1 and "the batch regenerates" in limit[0] and "split it below 4 GiB" in limit[0]
    refused = [ln[len("refuse "):] for ln in r.stdout.splitlines() if ln.startswith("refuse ")]
    for want in ("file 2: frame [96, +5) leaves its arena of 100 bytes", "file 1: frame [18446744073709551600, +32) leaves",
                 "file 1: frame [16, +18446744073709551615) leaves", "file 1: NULL input arena", "NULL output arena of 64 bytes"):
        assert any(ln.startswith(want) for ln in refused), (want, refused)


@needs_toolchain
@pytest.mark.timeout(900)
def test_planted_bug_is_caught(corpus_dir):
    r = _run(_build("unzstd_batch_check_bug", ["-DUNZSTDB_PLANT_BUG"]), corpus_dir, 0)
    assert r.returncode != 0
    assert "AddressSanitizer" in r.stderr or "FAIL " in r.stdout


def _call(lib, d_in, in_len, foff, flen, n, d_out=None, out_len=0, need=None, tables=True, status=False):
    foff = np.asarray(foff, dtype=np.uint64)
    flen = np.asarray(flen, dtype=np.uint64)
    toff, tlen, st = (np.zeros(max(n, 1), dtype=np.uint64) for _ in range(3))
    rc = lib.sydelta_zstd_decompress_batch_device(
        0, d_in, in_len, foff.ctypes.data if tables else None, flen.ctypes.data if tables else None, n, d_out, out_len,
        toff.ctypes.data, tlen.ctypes.data, st.ctypes.data if status else None,
        ctypes.byref(need) if need is not None else None, None)
    return rc, (lib.sydelta_last_error() or b"").decode()


def test_empty_batch_needs_no_device():
    from sy_amd._lib import lib

    need = ctypes.c_uint64(77)
    assert lib.sydelta_zstd_decompress_batch_device(0, None, 0, None, None, 0, None, 0, None, None, None,
                                                    ctypes.byref(need), None) == 0
    assert need.value == 0


def test_refusals_come_before_any_device():
    """Every host refusal of the contract, on a machine with or without a GPU: SYDELTA_E_INVAL
    with the file named, never SYDELTA_E_NODEV."""
    from sy_amd._lib import lib

    need = ctypes.c_uint64(77)
    rc, msg = _call(lib, None, 0, [0] * 3, [0] * 3, 3, need=need, tables=False)
    assert rc == E_INVAL and "NULL table" in msg and need.value == 0
    rc, msg = _call(lib, None, 0, [0], [0], 1, need=None)
    assert rc == E_INVAL and "NULL out_need" in msg
    A = 0x7000_0000_1001  # never dereferenced: the tables are refused first
    for d_in, in_len, foff, flen, want in [
            (A, 100, [0, 16, 96], [10, 10, 5], "file 2: frame [96, +5) leaves its arena of 100 bytes"),
            (A, 100, [0, 101], [10, 0], "file 1: frame [101, +0) leaves its arena of 100 bytes"),
            (A, 100, [0, U64_MAX - 15], [10, 32], "file 1: frame [18446744073709551600, +32) leaves its arena"),
            (A, 100, [0, 16], [10, U64_MAX], "file 1: frame [16, +18446744073709551615) leaves its arena"),
            (None, 100, [0, 16], [0, 1], "file 1: NULL input arena")]:
        for status in (False, True):
            need = ctypes.c_uint64(77)
            rc, msg = _call(lib, d_in, in_len, foff, flen, len(foff), need=need, status=status)
            assert rc == E_INVAL and want in msg, (rc, msg, want)
            assert need.value == 0
    rc, msg = _call(lib, A, 100, [0], [10], 1, d_out=None, out_len=64, need=ctypes.c_uint64())
    assert rc == E_INVAL and "NULL output arena of 64 bytes" in msg


def test_no_gpu_fails_loudly():
    """A valid batch without a GPU: SYDELTA_E_NODEV, never a CPU fallback.  (With a GPU the same
    batch of two frames of 3 bytes, each its file's "truncated frame" and no call error, is
    refused naming file 0.)"""
    import torch

    from sy_amd._lib import lib

    need = ctypes.c_uint64()
    if torch.cuda.is_available():
        buf = torch.zeros(16, dtype=torch.uint8, device="cuda")
        rc, msg = _call(lib, buf.data_ptr(), 16, [0, 3], [3, 3], 2, need=need)
        assert rc == E_INVAL and msg == "file 0: zstd frame: block 0: truncated frame"
    else:
        rc, _ = _call(lib, 0x7000_0000_1001, 16, [0, 3], [3, 3], 2, need=need)
        assert rc == E_NODEV
