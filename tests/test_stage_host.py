"""The pinned staging ring (sy_amd/csrc/sydelta_stage.hpp) without a GPU.

tests/csrc/stage_check.cpp, a stand-alone program built with g++ -fsanitize=address,undefined,
includes the header alone and defines the HIP calls it makes (hipHostMalloc, hipHostFree,
hipEventCreateWithFlags, hipStreamCreateWithFlags, hipEventRecord, hipEventSynchronize,
hipStreamWaitEvent, hipMemcpyAsync) as recorders: a copy lands only when an event behind it is
synchronised or its stream is drained, and its source is checksummed when queued and again when
it lands.  The program drives the ring the way sydelta_apply_delta_device and the four batch
calls do (one stream, a copy stream, half-ring groups, array uploads whose length is no multiple
of a slot, the growing piece table), for 2, 4 and 8 slots and 1, slots, slots + 1 and
3 * slots + 1 uses, on two devices.  It exits non-zero if a slot is handed out or rewritten with
bytes in flight, an upload is not followed by exactly one record of its slot's event on its
stream, one of the first `slots` uses waits, two devices share an event, or the pinned buffer
is allocated more than once or not freed (the leak check is on).  A driver that skips the wait
must be caught first."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sy_amd", "csrc")
OUT = os.path.join(ROOT, "build", "asan")
FLAGS = ["-std=c++17", "-O2", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
         "-I" + os.path.join(ROOT, "include"), "-I" + CSRC]


@pytest.mark.timeout(300)
@pytest.mark.skipif(shutil.which("g++") is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"),
                    reason="needs g++ and the HIP headers")
def test_slot_protocol_under_asan_ubsan():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "stage_check")
    src = os.path.join(ROOT, "tests", "csrc", "stage_check.cpp")
    r = subprocess.run(["g++"] + FLAGS + [src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=200)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-6000:])
    assert "stage_check ok: 144 calls" in r.stdout  # 3 ring sizes x 4 shapes x 4 counts x 3 passes
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_the_header_stands_alone():
    """sydelta_stage.hpp includes the HIP runtime API and the standard library, nothing of the
    project: a host program can include it alone."""
    with open(os.path.join(CSRC, "sydelta_stage.hpp")) as f:
        incs = [ln.split()[1] for ln in f if ln.startswith("#include")]
    assert "<hip/hip_runtime_api.h>" in incs
    assert all(i.startswith("<") for i in incs) and [i for i in incs if "hip" in i] == ["<hip/hip_runtime_api.h>"]
