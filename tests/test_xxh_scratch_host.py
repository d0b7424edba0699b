"""k_xxh_chain's unchecked batch prefetch stays inside its scratch, proved without a GPU.

A lane of k_xxh_chain loads its row of the C scratch in batches of kChainBatch up to the longest
chain of its wave, from its own file's first record: a short file sorted into a wave with a
long one reads up to nmax records past its row, and from row 7 past the eight rows.  The
scratch therefore has a tail (xxh_scratch_records, sydelta_internal.hpp).

tests/csrc/xxh_scratch_check.cpp, a stand-alone program built with g++
-fsanitize=address,undefined, rebuilds the host tables of sydelta_xxh3_batch_device for a batch
of lengths, walks the kernel's loop bounds for every wave (they must agree with the constexpr
xxh_chain_last_load the sizing is derived from) and requires every lane group's last load of
row 7 inside the allocation, which it then really allocates and reads.  Batches: the three of
test_gpu_integrity.test_batch_ragged, [1 MiB, 5], [5, 1 MiB], [1 GiB + 12345, 1, 241, 2049],
every non-increasing batch of 1 to 9 files with block counts from {0, 1, 2, 63, 64, 65, 66, 129}
and its reverse, and 2000 seeded random batches.  Built with the scratch sized as eight rows
alone, as it was before the tail, the same program must fail, by the excesses computed by
hand below."""
import os
import re
import shutil
import subprocess

import pytest

from test_gpu_integrity import ragged_lens

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sy_amd", "csrc")
OUT = os.path.join(ROOT, "build", "asan")
FLAGS = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
         "-I" + os.path.join(ROOT, "include"), "-I" + CSRC]
MiB, GiB = 1 << 20, 1 << 30
NAMED = {
    "ragged1": ragged_lens(1), "ragged2": ragged_lens(2), "ragged3": ragged_lens(3),
    "long-short": [MiB, 5], "short-long": [5, MiB], "gib": [GiB + 12345, 1, 241, 2049],
    "one-mib": [MiB], "one-gib": [GiB],
}
# Excess of the worst load over the last record of the eight rows, by hand:
# [1 MiB, 5]: 1023 blocks, nmax = 1022 steps, the ragged loop's last round starts at k = 960 and
# loads Cn[960 + 95]; the 5-byte file starts at fpfx = npieces = 1023, so row 7's load is record
# 7 * cstride + 1023 + 1 + 1055 against a last record of 7 * cstride + 1023 + 95: 961 beyond.
# [5, 1 MiB]: both files start at record 0: 1 + 1055 - (1023 + 95) = -62, inside.
# A 1 GiB file alone: 1048575 blocks, the last round starts at k = 1048512:
# 1 + 1048512 + 95 - (1048575 + 95) = -62 as well (both block counts are 63 mod 64).
EXCESS = {"long-short": 961, "short-long": -62, "one-mib": -62, "one-gib": -62}
# test_batch_ragged's batches, from an independent model of the loop bounds: seed 1 puts a
# 293-block file of 300047 B into the wave of a 1 MiB file (nmax 1023).
EXCESS.update({"ragged1": 376, "ragged2": -1, "ragged3": 58})

needs_toolchain = pytest.mark.skipif(
    shutil.which("g++") is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime.h"),
    reason="needs g++ and the HIP headers")


def _run(tmp_path, name, extra):
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, name)
    src = os.path.join(ROOT, "tests", "csrc", "xxh_scratch_check.cpp")
    r = subprocess.run(["g++"] + FLAGS + extra + [src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    cases = tmp_path / "cases.txt"
    cases.write_text("".join("%s %s\n" % (k, " ".join(map(str, v))) for k, v in NAMED.items()))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, str(cases)], capture_output=True, text=True, env=env, timeout=250)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-6000:]
    return r, {k: int(v) for k, v in re.findall(r"^(\S+) excess=(-?\d+)$", r.stdout, re.M)}


@pytest.mark.timeout(300)
@needs_toolchain
def test_every_prefetch_is_inside_the_scratch(tmp_path):
    r, excess = _run(tmp_path, "xxh_scratch_check", [])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-6000:])
    # 8 named + 2 x (multisets of 1..9 out of 8 counts = C(17, 8) - 1) + 2000 random
    assert "xxh_scratch_check ok: 8 named, %d batches" % (8 + 2 * 24309 + 2000) in r.stdout
    assert set(excess) == set(NAMED) and all(excess[k] == v for k, v in EXCESS.items()), excess
    assert excess["ragged1"] > 0 and excess["gib"] > 0  # the suite's own batch read past the rows


@pytest.mark.timeout(300)
@needs_toolchain
def test_the_check_fails_on_eight_rows_alone(tmp_path):
    """The sizing before the tail (8 * xxh_chain_records): the check must see the over-read."""
    r, excess = _run(tmp_path, "xxh_scratch_check_rows_only", ["-DXXH_SCRATCH_ROWS_ONLY"])
    assert r.returncode == 1 and "xxh_scratch_check FAILED" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
    for name in ("ragged1", "long-short", "gib"):
        assert re.search(r"^FAIL %s: .* loads record" % name, r.stdout, re.M), name
    assert not re.search(r"^FAIL (short-long|one-mib|one-gib):", r.stdout, re.M)
    assert all(excess[k] == v for k, v in EXCESS.items()), excess
