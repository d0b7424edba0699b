"""The batched signature JSON writer and parser (sydelta_checksums_batch_to_json_device,
sydelta_checksums_batch_from_json_device) without a GPU.

tests/csrc/sig_batch_check.cpp, a stand-alone program built with g++ -fsanitize=address,
undefined, includes sy_amd/csrc/sydelta_sigbatch.hpp and runs what the entry points and their
kernels run -- the plans, the tile's file, the writer's per-tile bodies, the parser's count /
sizes / parse on the shared chunk table with the batch's ranks, the staged span's accessor -- on
host memory with every array at its exact size and the stages' tiles and files in shuffled
order, at block sizes 4096 and 1007:

* writer: files of 0, 1, 2, 255, 256, 257 and 513 blocks with neighbouring empty files, the
  hand-made extremes (weak 0 / 9 / 10 / 2^32 - 1, strong 0 / 2^64 - 1), last_size 1 and bs, the
  arena at byte phases 0, 1 and 7 inside a 0xA5 guard: every text equals the single writer's
  bodies run on the file alone, the packing rule holds, pads and guards are intact;
* parser: the same texts in file order, reversed and shuffled, packed at multiples of 16 and at
  odd offsets, one text listed twice, the arena at phases 0, 1 and 7, the pad bytes spelling
  '{', digits and commas, a '{' on the last byte of a chunk and of a 4 KiB tile, "[]" between
  two files inside one tile span, the SoA at its exact size: every file equals its text parsed
  alone by the single parser's bodies, and the staged accessor never leaves its span on a
  well-formed text;
* refusals, each between two good files that stay exact, with the status word and the byte.

A build with -DSIGB_PLANT_BUG (a file's entries written relative to the batch instead of
sig_off[f]) must fail the same run.

The entry points themselves: an empty batch is OK without a device, every host refusal comes
before a device is touched and names its file, the bound function, and a valid batch on a
machine without a GPU is SYDELTA_E_NODEV (no CPU fallback)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "build", "asan")

needs_toolchain = pytest.mark.skipif(shutil.which("g++") is None or
                                     not os.path.exists("/opt/rocm/include/hip/hip_runtime.h"),
                                     reason="needs g++ and the HIP headers")

U64_MAX = (1 << 64) - 1
E_INVAL, E_NODEV = -3, -1
A = 0x7000_0000_1000  # never dereferenced: the tables are refused first


def _build(name: str, extra=()) -> str:
    from test_host_sanitizers import FLAGS  # the host sanitizer builds' flags

    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, name)
    r = subprocess.run(["g++"] + FLAGS + list(extra) + [os.path.join(ROOT, "tests", "csrc", "sig_batch_check.cpp"),
                                                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def _run(exe: str):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    return subprocess.run([exe, "7"], capture_output=True, text=True, env=env, timeout=600)


# The refusals of the check program at bs 4096: five entries built as the program builds them
# (weak 1000 + 37 i, strong 0x9E3779B97F4A7C15 (i + 1) mod 2^64, last size bs - 1), the byte
# worked out here from the text.
def _entries(bs, n=5):
    return [dict(index=i, offset=i * bs, size=bs - 1 if i + 1 == n else bs, weak=1000 + 37 * i,
                 strong=(0x9E3779B97F4A7C15 * (i + 1)) & U64_MAX) for i in range(n)]


def _text(entries):
    parts, braces, at = [], [], 1
    for e in entries:
        s = ('{"index":%s,"offset":%s,"size":%s,"weak":%s,"strong":%s}'
             % (e["index"], e["offset"], e["size"], e["weak"], e["strong"]))
        braces.append(at)
        parts.append(s)
        at += len(s) + 1
    return "[" + ",".join(parts) + "]", braces


def _refused_texts(bs=4096):
    """name -> the refused text, as the check program builds them (tests/test_gpu_sig_batch.py
    runs the same list on the device)."""
    def edit(i, **kw):
        e = _entries(bs)
        e[i].update(kw)
        return _text(e)[0].encode()

    good = _text(_entries(bs))[0].encode()
    both = _entries(bs)
    both[1]["size"] = bs + 7
    both[3]["weak"] = "00"
    return {
        "space-after-comma": good.replace(b",", b", ", 1),
        "missing-bracket": good[:-1],
        "Weak": good.replace(b'"weak"', b'"Weak"', 1),
        "leading-zero": edit(1, weak="0%d" % (1000 + 37)),
        "weak-2^32": edit(2, weak=1 << 32),
        "above-u64": edit(2, strong=1 << 64),
        "one-byte": b"[",
        "no-bytes": b"",
        "index-off-by-one": edit(2, index=3),
        "offset": edit(3, offset=3 * bs + 1),
        "size-not-bs": edit(1, size=bs + 1),
        "last-size-0": edit(4, size=0),
        "last-size-bs+1": edit(4, size=bs + 1),
        "both-kinds": _text(both)[0].encode(),
    }


def _expected_messages(bs=4096):
    """name -> the message of file 1.  A spelling refusal names the '{' of the entry the bad byte
    belongs to (the entry's thread refuses it), or byte 1's entry for a bad separator behind it."""
    good, br = _text(_entries(bs))
    sp = "file 1: checksum JSON: not serde's compact form at byte %d"
    lay = "file 1: checksum JSON: entry at byte %d is not block %d of a signature with block size %d"
    e = {}
    e["space-after-comma"] = sp % br[0]   # the first ',' is inside entry 0
    e["missing-bracket"] = sp % br[4]     # the last entry finds no ']'
    e["Weak"] = sp % br[0]
    e["leading-zero"] = sp % br[1]
    e["weak-2^32"] = sp % br[2]
    e["above-u64"] = sp % br[2]
    e["one-byte"] = sp % 0
    e["no-bytes"] = sp % 0
    e["index-off-by-one"] = lay % (br[2], 2, bs)
    e["offset"] = lay % (br[3], 3, bs)    # the offset grows by one digit at most: same '{'
    e["size-not-bs"] = lay % (br[1], 1, bs)
    e["last-size-0"] = lay % (br[4], 4, bs)
    e["last-size-bs+1"] = lay % (br[4], 4, bs)
    e["both-kinds"] = sp % br[3]
    return e


@needs_toolchain
@pytest.mark.timeout(600)
def test_batch_bodies_under_asan_ubsan():
    r = _run(_build("sig_batch_check"))
    print(r.stdout[-3000:])
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-6000:])
    assert "sig_batch_check ok" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    got = dict(re.findall(r"^reject (\S+): (.*)$", r.stdout, re.M))
    assert got == _expected_messages()


@needs_toolchain
@pytest.mark.timeout(600)
def test_planted_bug_is_caught():
    r = _run(_build("sig_batch_check_bug", ["-DSIGB_PLANT_BUG"]))
    assert r.returncode != 0
    assert "AddressSanitizer" in r.stderr or "FAIL " in r.stdout


def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def _write(lib, weak, strong, nblocks, last, n, bs, out=None, out_len=0, need=None, tables=True):
    nb, ls = _u64(nblocks), _u64(last)
    toff, tlen = (np.full(max(n, 1), 77, dtype=np.uint64) for _ in range(2))
    rc = lib.sydelta_checksums_batch_to_json_device(
        0, weak, strong, nb.ctypes.data if tables else None, ls.ctypes.data if tables else None, n, bs, out, out_len,
        toff.ctypes.data, tlen.ctypes.data, ctypes.byref(need) if need is not None else None, None)
    return rc, (lib.sydelta_last_error() or b"").decode()


def _parse(lib, text, text_len, toff, tlen, n, bs, need=None, tables=True, status=False):
    to, tl = _u64(toff), _u64(tlen)
    so, nb, ls, st = (np.zeros(max(n, 1), dtype=np.uint64) for _ in range(4))
    rc = lib.sydelta_checksums_batch_from_json_device(
        0, text, text_len, to.ctypes.data if tables else None, tl.ctypes.data if tables else None, n, bs, None, None, 0,
        so.ctypes.data, nb.ctypes.data, ls.ctypes.data, st.ctypes.data if status else None,
        ctypes.byref(need) if need is not None else None, None)
    return rc, (lib.sydelta_last_error() or b"").decode()


def test_empty_batch_needs_no_device():
    from sy_amd._lib import lib

    need = ctypes.c_uint64(77)
    assert lib.sydelta_checksums_batch_to_json_device(0, None, None, None, None, 0, 4096, None, 0, None, None,
                                                      ctypes.byref(need), None) == 0
    assert need.value == 0
    need = ctypes.c_uint64(77)
    assert lib.sydelta_checksums_batch_from_json_device(0, None, 0, None, None, 0, 4096, None, None, 0, None, None, None,
                                                        None, ctypes.byref(need), None) == 0
    assert need.value == 0
    assert lib.sydelta_checksums_batch_to_json_bound(None, None, 0, 4096) == 0


def test_writer_refusals_come_before_any_device():
    """Every host refusal of the writer's contract, on a machine with or without a GPU:
    SYDELTA_E_INVAL with the file named, never SYDELTA_E_NODEV."""
    from sy_amd._lib import lib

    need = ctypes.c_uint64(77)
    rc, msg = _write(lib, A, A, [1] * 3, [1] * 3, 3, 4096, need=need, tables=False)
    assert rc == E_INVAL and "NULL table" in msg and need.value == 0
    rc, msg = _write(lib, A, A, [1], [1], 1, 4096, need=None)
    assert rc == E_INVAL and "NULL out_need" in msg
    for weak, strong, nblocks, last, bs, want in [
            (None, A, [0, 2], [0, 5], 4096, "NULL signature arrays"),
            (A, None, [0, 2], [0, 5], 4096, "NULL signature arrays"),
            (A, A, [1], [1], 0, "block_size 0 out of range"),
            (A, A, [1], [1], (1 << 32) + 1, "block_size 4294967297 out of range"),
            (A, A, [2, 3], [7, 0], 4096, "file 1: last_size 0 outside (0, 4096]"),
            (A, A, [2, 0, 3], [7, 0, 4097], 4096, "file 2: last_size 4097 outside (0, 4096]"),
            (A, A, [1, (1 << 32) + 1], [1, 1 << 32], 1 << 32, "file 1: offsets of 4294967297 blocks overflow"),
            # a sum of nblocks that overflows: its first file already holds too many tiles
            (A, A, [1 << 63, 1 << 63], [1, 1], 1, "file 0: the batch holds more than 2^31 tiles"),
            (A, A, [1, 1 << 40], [1, 1], 1, "file 1: the batch holds more than 2^31 tiles")]:
        need = ctypes.c_uint64(77)
        rc, msg = _write(lib, weak, strong, nblocks, last, len(nblocks), bs, need=need)
        assert rc == E_INVAL and want in msg, (rc, msg, want)
        assert need.value == 0
    # a batch without entries needs no SoA ... (it reaches the device: NODEV or OK)
    rc, msg = _write(lib, None, None, [0, 0], [0, 0], 2, 4096, need=ctypes.c_uint64())
    assert rc in (0, E_NODEV), (rc, msg)


def test_parser_refusals_come_before_any_device():
    from sy_amd._lib import lib

    need = ctypes.c_uint64(77)
    rc, msg = _parse(lib, None, 0, [0] * 3, [0] * 3, 3, 4096, need=need, tables=False)
    assert rc == E_INVAL and "NULL table" in msg and need.value == 0
    rc, msg = _parse(lib, None, 0, [0], [0], 1, 4096, need=None)
    assert rc == E_INVAL and "NULL sig_need" in msg
    for text, text_len, toff, tlen, bs, want in [
            (A, 100, [0, 16, 96], [10, 10, 5], 4096, "file 2: text [96, +5) leaves its arena of 100 bytes"),
            (A, 100, [0, 101], [10, 0], 4096, "file 1: text [101, +0) leaves its arena of 100 bytes"),
            (A, 100, [0, U64_MAX - 15], [10, 32], 4096, "file 1: text [18446744073709551600, +32) leaves its arena"),
            (A, 100, [0, 16], [10, U64_MAX], 4096, "file 1: text [16, +18446744073709551615) leaves its arena"),
            (None, 100, [0, 16], [0, 1], 4096, "file 1: NULL text arena"),
            (A, 100, [0], [10], 0, "block_size 0 out of range"),
            (A, 100, [0], [10], (1 << 32) + 1, "block_size 4294967297 out of range"),
            (A, 1 << 40, [0, 0], [1 << 36, 1 << 36], 4096, "more than 2^31 chunks of text at file 1")]:
        for status in (False, True):
            need = ctypes.c_uint64(77)
            rc, msg = _parse(lib, text, text_len, toff, tlen, len(toff), bs, need=need, status=status)
            assert rc == E_INVAL and want in msg, (rc, msg, want)
            assert need.value == 0


def _digits_sum(n, m):
    return sum(len(str(i * m)) for i in range(n))


def test_bound_function():
    """sydelta_checksums_batch_to_json_bound: per file the longest text its implied fields allow
    (weak 10 digits, strong 20), rounded up to 16; UINT64_MAX on a NULL table or overflow."""
    from sy_amd._lib import lib

    def bound(nblocks, last, bs):
        nb, ls = _u64(nblocks), _u64(last)
        return lib.sydelta_checksums_batch_to_json_bound(nb.ctypes.data, ls.ctypes.data, len(nb), bs)

    def longest(n, last, bs):
        if n == 0:
            return 2
        fixed = n * 47 + 1 + _digits_sum(n, 1) + _digits_sum(n, bs) + (n - 1) * len(str(bs)) + len(str(last))
        return fixed + 30 * n

    for bs in (4096, 1007, 1, 1 << 32):
        files = [(0, 0), (1, 1), (1, bs), (255, bs), (257, 1), (0, 0), (1001, max(1, bs // 2))]
        want = sum((longest(n, last, bs) + 15) // 16 * 16 for n, last in files)
        assert bound([n for n, _ in files], [l for _, l in files], bs) == want, bs
    assert lib.sydelta_checksums_batch_to_json_bound(None, None, 3, 4096) == U64_MAX
    assert bound([1], [1], 0) == U64_MAX
    assert bound([1], [1], (1 << 32) + 1) == U64_MAX
    assert bound([1 << 60], [1], 4096) == U64_MAX
    assert bound([1 << 54] * 1024, [1] * 1024, 1) == U64_MAX


def test_no_gpu_fails_loudly():
    """A valid batch without a GPU: SYDELTA_E_NODEV, never a CPU fallback.  (With a GPU the
    writer's size query of two files without blocks is OK, 16 + 2 bytes, and the parser's batch
    of two texts of 1 byte, each its file's refusal at byte 0 and no call error, is refused
    naming file 0.)"""
    import torch

    from sy_amd._lib import lib

    need = ctypes.c_uint64()
    if torch.cuda.is_available():
        rc, msg = _write(lib, None, None, [0, 0], [0, 0], 2, 4096, need=need)
        assert rc == 0 and need.value == 18, (rc, msg)
        buf = torch.zeros(16, dtype=torch.uint8, device="cuda")
        rc, msg = _parse(lib, buf.data_ptr(), 16, [0, 3], [1, 1], 2, 4096, need=need)
        assert rc == E_INVAL and msg == "file 0: checksum JSON: not serde's compact form at byte 0"
    else:
        rc, _ = _write(lib, A, A, [2, 1], [5, 4096], 2, 4096, need=need)
        assert rc == E_NODEV
        rc, _ = _parse(lib, A, 64, [0, 16], [2, 2], 2, 4096, need=need)
        assert rc == E_NODEV
