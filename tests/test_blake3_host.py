"""CPU tests of the BLAKE3 boundary: the five entry points exist, the host-side join of
chaining values (sydelta_blake3_join, shard.blake3_join) agrees with the from-specification
reference and refuses pieces outside its contract, empty inputs need no device, a missing
GPU or file is a loud error, and the portable compress / tree / join of sydelta_blake3.hpp
runs clean under AddressSanitizer + UndefinedBehaviorSanitizer as a program of its own."""
import json
import os
import re
import shutil
import subprocess

import pytest

import blake3_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["sydelta_blake3_device", "sydelta_blake3_batch_device", "sydelta_blake3_subtree_device",
           "sydelta_blake3_join", "sydelta_blake3_file"]
DECOMPOSITIONS = [(npieces, last, cut) for npieces in range(2, 10) for last, cut in [(1, 0), (3, 0), (4, 1000)]]


def test_header_and_library_export_the_symbols():
    from sy_amd import _lib

    txt = open(os.path.join(ROOT, "include", "sydelta.h")).read()
    assert "#define SYDELTA_BLAKE3_LEN 32" in txt
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\bT (sydelta_[a-z0-9_]+)", out.stdout))
    table = {n for n, _, _ in _lib.SIGNATURES}
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, txt), s
        assert s in exported and s in table, s
    assert _lib.lib.sydelta_abi_version() == 1


@pytest.mark.parametrize("npieces,last,cut", DECOMPOSITIONS)
def test_join_of_reference_subtrees(npieces, last, cut):
    from sy_amd import shard

    total = (npieces - 1) * 4096 + last * 1024 - cut
    data = R.pattern(total)
    ps = R.pieces(total, 4)
    cvs = [R.subtree_cv(data[o:o + ln], fc) for o, ln, fc, _ in ps]
    assert shard.blake3_join(cvs, [c for *_, c in ps]) == R.blake3(data)


def test_join_refuses_pieces_outside_the_contract():
    from sy_amd import shard
    from sy_amd._lib import SyDeltaError

    cv = [bytes([i]) * 32 for i in range(4)]
    for chunks in ([3, 3, 1],      # not a power of two
                   [4, 2, 4],      # unequal pieces
                   [4, 4, 5],      # the last one larger than the others
                   [4, 0],         # an empty last piece
                   [4],            # a single piece is blake3()'s
                   []):
        with pytest.raises(SyDeltaError) as e:
            shard.blake3_join(cv[:len(chunks)], chunks)
        assert e.value.code == -3
    assert len(shard.blake3_join(cv[:3], [4, 4, 1])) == 32


def test_empty_inputs_need_no_device(tmp_path):
    from sy_amd.delta import Blake3Hasher

    p = tmp_path / "empty"
    p.write_bytes(b"")
    assert Blake3Hasher.hash_data(b"").hex() == R.VECTORS[0]
    assert Blake3Hasher.hash_file(p).hex() == R.VECTORS[0]


def test_missing_file_is_an_io_error(tmp_path):
    from sy_amd._lib import SyDeltaError
    from sy_amd.delta import Blake3Hasher

    with pytest.raises(SyDeltaError) as e:
        Blake3Hasher.hash_file(tmp_path / "nonexistent")
    assert e.value.code == -5  # SYDELTA_E_IO, like io::Error from File::open


def test_no_gpu_fails_loudly(tmp_path):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from sy_amd._lib import SyDeltaError
    from sy_amd.delta import Blake3Hasher

    with pytest.raises(SyDeltaError) as e:
        Blake3Hasher.hash_data(b"abc")
    assert e.value.code == -1  # SYDELTA_E_NODEV: no silent CPU fallback
    p = tmp_path / "abc"
    p.write_bytes(b"abc")
    with pytest.raises(SyDeltaError) as e:
        Blake3Hasher.hash_file(p)
    assert e.value.code == -1


def test_portable_header_under_asan_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "blake3_subtrees.json")))
    lines = ["hash %d %s" % (n, R.VECTORS[n]) for n in (0, 1, 64, 65, 1023, 1024, 1025, 2049, 5121, 31744)]
    lines += ["cv %d %d %s" % (c["len"], c["first_chunk"], c["cv"]) for c in golden["subtrees"]]
    lines += ["join %d %d %s" % (c["len"], c["piece_chunks"], c["hash"]) for c in golden["joins"]]
    cases = tmp_path / "cases.txt"
    cases.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "blake3_host_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "sy_amd", "csrc"),
                        os.path.join(ROOT, "tests", "csrc", "blake3_host_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, str(cases)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "blake3_host_check ok: %d cases" % len(lines) in r.stdout
    assert "runtime error" not in r.stderr
