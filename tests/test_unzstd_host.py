"""The zstd decoder's stage bodies (sy_amd/csrc/sydelta_unzstd.hpp) on the CPU under
ASan + UBSan: tests/csrc/unzstd_check.cpp, a stand-alone program, runs them the way the
kernels do (thread by thread, shuffled, every array at its exact size, frame and output at
exact sizes and all alignments) over

* the libzstd corpus of tests/zstd_frames.py (every input streamed at levels 1, 3, 19 and
  compressed one-shot at level 3), whose coverage is asserted here so that another libzstd
  cannot silently stop producing a form;
* frames of our own encoder (its sequential host form, test_zstd.ref_compress): the only
  direct-representation weights and 14-byte headers;
* hand-assembled frames (RLE literals, RLE_Mode sequences, all three sequence-count forms),
  each checked against libzstd first;
* the families assembled from RFC 8878 for the forms no sender writes (tests/zstd_frames.py:
  offset codes 17 to 21 and 24, the length extremes, 12-bit Huffman trees, deep chains, empty
  and many blocks), every frame of every family checked against libzstd first, and a libzstd
  frame with a match 5 MiB back; the larger ones decoded only, not mutated;
* the fixed malformed list, the twins one byte short of their offset and the block of 128 KiB + 1:
  an error each that names its block, nothing written;
* 200 seeded mutants of every one of these frames: never a sanitizer report; whenever libzstd
  accepts a mutant, the same bytes, or a refusal whose condition the program finds in the
  frame's bytes with a reader of its own (the issue's own refusals and RFC 8878's limits that
  libzstd 1.4.8 does not enforce); any other refusal fails.

The coverage assertions and the libzstd check of the hand-assembled frames run inside the
test that runs the program.

A build with -DUNZSTD_PLANT_BUG (the offset check dropped) must fail the same run."""
import os
import shutil
import subprocess

import pytest

import zstd_frames as F
from test_zstd import _libzstd, ref_compress, zstd_decode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "build", "asan")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None or _libzstd() is None or
                                not os.path.exists("/opt/rocm/include/hip/hip_runtime.h"),
                                reason="needs g++, the HIP headers and the system libzstd")


# The assembled families of tests/zstd_frames.py: mutated 200 times, decoded at exact sizes only
# (the large ones; wide-seq's 32 MiB take the program ten seconds), and refused.
FORMS_OK = ("of17", "ml-max", "ll-max") + F.HUF_FORMS + ("deep1-1", "deep1-2", "deep3", "empties", "empties-seq")
FORMS_VALID = ("of18", "of19", "of20", "of21", "wide-seq", "deep1-3", "deep1-64", "deep-block", "many-blocks")
FORMS_REJECT = tuple(f"of{k}-short" for k in range(17, 22)) + ("ml-over",)


def _build(name: str, extra=()) -> str:
    from test_host_sanitizers import FLAGS  # the host sanitizer builds' flags

    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, name)
    r = subprocess.run(["g++"] + FLAGS + list(extra) + [os.path.join(ROOT, "tests", "csrc", "unzstd_check.cpp"),
                                                        F.libzstd_path(), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def _run(exe: str, corpus_dir: str, mutants: int):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    return subprocess.run([exe, corpus_dir, str(mutants), "7"], capture_output=True, text=True, env=env, timeout=1500)


@pytest.fixture(scope="module")
def corpus_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("unzstd")
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
    for name in FORMS_OK + FORMS_VALID:
        frame, ops = F.form(name)
        put(name, "ok" if name in FORMS_OK else "valid", frame, F.expect(ops).tobytes())
    put("far-s19", "valid", *F.far_frame())
    for name in FORMS_REJECT:
        put(name, "reject", F.form_refused(name))
    (d / "manifest.txt").write_text("\n".join(lines) + "\n")
    return str(d)


def _assert_corpus_covers_what_it_claims():
    """The forms the issue's table names, found in the frames this libzstd writes."""
    c = F.corpus()
    for name, (frame, data) in c.items():
        assert zstd_decode(frame, len(data)) == data, name
    d = {name: F.describe(frame) for name, (frame, _) in c.items()}
    # streamed frames: no content size, no checksum (libzstd writes a zero content size for no input)
    assert all(v["fhd"] == 0 for k, v in d.items() if not k.endswith("-o3") and not k.startswith("empty-"))
    comp = [b for v in d.values() for b in v["blocks"] if b["type"] == 2]
    for name in ("json-copies", "json-mixed", "json-literals"):
        assert len(d[f"{name}-s3"]["blocks"]) == 4, name
    assert {b["lit"] for b in comp} >= {0, 2, 3}  # Raw, Compressed and Treeless literals
    assert {b["streams"] for b in comp if b["lit"] >= 2} == {1, 4}
    assert "fse" in {b.get("weights") for b in comp}
    modes = {m for b in comp if "modes" in b for m in b["modes"]}
    assert modes >= {0, 2, 3}  # Predefined, FSE_Compressed, Repeat
    assert any(b.get("modes") == (3, 3, 2) for b in d["json-literals-s19"]["blocks"])
    assert any(b["nseq"] == 0 for b in d["printable-x3-s3"]["blocks"])
    o3 = d["json-copies-o3"]
    assert o3["fhd"] >> 5 & 1 and o3["fhd"] >> 6 == 2 and o3["header"] == 9  # Single_Segment, 4-byte content size
    small = d["json-small-s1"]["blocks"]
    assert len(small) == 1 and small[0]["type"] == 2 and small[0]["modes"] == (0, 0, 0)
    assert [b["type"] for b in d["one-s3"]["blocks"]] == [0] and d["empty-s3"]["blocks"][0]["size"] == 0
    assert 1 in {b["type"] for b in d["sevens-s3"]["blocks"]}
    assert [b["type"] for b in d["random-5000-s3"]["blocks"]] == [0]
    assert [b["type"] for b in d["random-300000-s3"]["blocks"]] == [0, 0, 0]
    tail = d["json-128k+1-s3"]["blocks"]
    assert [b["type"] for b in tail] == [2, 0] and tail[1]["size"] == 1
    own = {name: F.describe(ref_compress(data)) for name, data in F.own_texts() if name in ("copies", "small")}
    assert own["copies"]["header"] == 14 and own["copies"]["fhd"] >> 6 == 3
    assert "direct" in {b.get("weights") for v in own.values() for b in v["blocks"]}


def _assert_hand_assembled_frames_are_what_libzstd_reads():
    for name, (frame, data) in F.hand_frames().items():
        assert zstd_decode(frame, len(data)) == data, name
    assert F.describe(F.rle_seq_frame([32768]))["blocks"][0]["nseq"] == 32768
    bad = F.malformed()
    assert F.libzstd_accepts(bad["ll0-offset-before-start"], 1 << 20) is None
    assert F.libzstd_accepts(bad["first-block-treeless"], 1 << 20) is None
    assert F.libzstd_accepts(bad["first-block-repeat-mode"], 1 << 20) is None


def _assert_table_descriptions_reach_what_they_claim():
    """The FSE table descriptions read from the spec (F.read_ncount): what the corpus reaches, and
    what the far frame adds to it."""
    logs, less, top = [0, 0, 0], [False] * 3, [0, 0, 0]
    for name, (frame, _) in F.corpus().items():
        for tabs in F.fse_tables(frame):
            for j, (log, probs) in tabs.items():
                logs[j], less[j], top[j] = max(logs[j], log), less[j] or -1 in probs, max(top[j], len(probs) - 1)
    assert logs == [9, 8, 9] and all(less), (logs, less)  # LL / OF / ML at their largest accuracy logs
    assert top[0] < 32 and top[1] < 22, top  # which is why the far frame is there
    frame, data = F.far_frame()
    assert zstd_decode(frame, len(data)) == data
    tabs = F.fse_tables(frame)
    assert any(len(t[1][1]) - 1 >= 22 for t in tabs if 1 in t)  # an FSE-compressed offset table with code 22
    assert any(len(t[0][1]) - 1 >= 32 for t in tabs if 0 in t)  # and a literal-length table with code 32


def _assert_assembled_families_are_what_libzstd_reads():
    """Every frame of every family, the GPU test's large ones included."""
    import numpy as np

    for name in F.FORMS:
        frame, ops = F.form(name)
        want = F.expect(ops)
        got = zstd_decode(frame, len(want) + 1)
        assert len(got) == len(want) and np.array_equal(np.frombuffer(got, dtype=np.uint8), want), name
    assert len(F.expect(F.form("of27")[1])) == (1 << 28) + 44
    for name in ("ml-max", "ll-max"):
        assert len(F.expect(F.form(name)[1])) == 128 << 10
    assert max(b["lit_regen"] for b in F.describe(F.form("huf12-4x131072")[0])["blocks"]) == 131072
    for name in F.FORMS_REFUSED:
        got = F.libzstd_accepts(F.form_refused(name), 1 << 29)
        # libzstd 1.4.8 accepts the block of 128 KiB + 1: stricter here by design
        assert (got is not None and len(got) == (128 << 10) + 1) if name == "ml-over" else got is None, name


@pytest.mark.timeout(1800)
def test_stage_bodies_under_asan_ubsan(corpus_dir):
    _assert_corpus_covers_what_it_claims()
    _assert_hand_assembled_frames_are_what_libzstd_reads()
    _assert_table_descriptions_reach_what_they_claim()
    _assert_assembled_families_are_what_libzstd_reads()
    r = _run(_build("unzstd_check"), corpus_dir, 200)
    print(r.stdout[-3000:])
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-6000:])
    assert "unzstd_check ok" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    rejects = {ln.split()[1].rstrip(":"): ln for ln in r.stdout.splitlines() if ln.startswith("reject ")}
    forms = {name: rejects.pop(name) for name in FORMS_REJECT}
    assert sorted(rejects) == sorted(F.malformed()) == sorted(F.MALFORMED_REASON)
    for name, line in rejects.items():  # each refused for its own reason
        assert F.MALFORMED_REASON[name] in line, line
    for name, line in forms.items():  # and at its own block
        assert F.FORMS_REFUSED[name] in line, line


@pytest.mark.timeout(900)
def test_planted_bug_is_caught(corpus_dir):
    r = _run(_build("unzstd_check_bug", ["-DUNZSTD_PLANT_BUG"]), corpus_dir, 0)
    assert r.returncode != 0
    assert "AddressSanitizer" in r.stderr or "FAIL ll0-offset-before-start" in r.stdout
    # the twins one byte short of their offset are accepted by that build as well
    assert "AddressSanitizer" in r.stderr or any(f"FAIL of{k}-short: accepted" in r.stdout for k in range(17, 22))
