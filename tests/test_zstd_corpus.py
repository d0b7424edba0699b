"""The shaped corpus of tests/zstd_corpus.py is what it claims (CPU).

tests/test_gpu_zstd_parse.py compares the device block coder with the sequential host form
on that corpus; the comparison says something only where the texts reach the forms that the
device codes in its own way.  So (1) libzstd decodes every host frame back to its text (the
host form is a sound reference there), and (2) the corpus's summed shape, read by
zstd_ref_shape (tests/csrc/zstd_ref.cpp) from the blocks whose literals + sequences content
won, meets the floors in FLOORS.  The floors are conditions on the corpus, not measurements:
when a generator change drops one, the generator changes.

The committed corpus, 241 texts of 4341291 bytes in all, measures (the test checks these lines
against what it reads, so they stay true):

    blocks_won                   213   (floor 150)
    seqs                       58237
    max_seqs_in_block           1936
    ov1_ll0                      931   (floor 200)
    ov2_ll0                      720   (floor 200)
    ov3_ll0                      439   (floor 200)
    ov1_lln                    20171   (floor 150)
    ov2_lln                      772   (floor 150)
    ov3_lln                      448   (floor 150)
    max_rep_run                   26
    max_rep_run_block_seqs      1508
    max_rep_run_over64            26   (floor 9)
    ll0_at_rep0                   99   (floor 8)
    max_match                 126072   (floor 100000)
    match_over512                457   (floor 200)
    end_on_512                   125   (floor 50)
    last_ends_at_n               178   (floor 100)
    lit_raw                      118   (floor 40)
    lit_one                       54   (floor 15)
    lit_four                      41   (floor 15)
    rle_blocks                    43   (floor 20)
    rle_over1                     13   (floor 5)
    rle_over64                     5   (floor 2)
    one_seq_blocks                30   (floor 10)
    dist_over4096               9408   (floor 500)
    dup_history_turns             86   (floor 20)
"""
import ctypes
import functools
import os
import shutil

import pytest

import test_zstd as Z
import zstd_corpus

pytestmark = pytest.mark.skipif(shutil.which("g++") is None or Z._libzstd() is None or
                                not os.path.exists("/opt/rocm/include/hip/hip_runtime.h"),
                                reason="needs g++, the HIP headers and the system libzstd")

# the order of enum Shape in tests/csrc/zstd_ref.cpp; max_* keep the largest value, the others add up
SHAPE_NAMES = ("blocks_won", "seqs", "max_seqs_in_block",
               "ov1_ll0", "ov2_ll0", "ov3_ll0", "ov1_lln", "ov2_lln", "ov3_lln",
               "max_rep_run", "max_rep_run_block_seqs", "max_rep_run_over64",
               "ll0_at_rep0", "max_match", "match_over512", "end_on_512", "last_ends_at_n",
               "lit_raw", "lit_one", "lit_four",
               "rle_blocks", "rle_over1", "rle_over64", "one_seq_blocks", "dist_over4096", "dup_history_turns")

FLOORS = {"blocks_won": 150, "one_seq_blocks": 10, "rle_blocks": 20, "rle_over1": 5, "rle_over64": 2,
          "lit_raw": 40, "lit_one": 15, "lit_four": 15,
          "ov1_ll0": 200, "ov2_ll0": 200, "ov3_ll0": 200, "ov1_lln": 150, "ov2_lln": 150, "ov3_lln": 150,
          "max_rep_run_over64": 9, "ll0_at_rep0": 8, "match_over512": 200, "max_match": 100000,
          "end_on_512": 50, "last_ends_at_n": 100, "dist_over4096": 500}
# One more, not in the list the corpus was first built to: sequences whose Offset_Value changes when
# the history is taken as the three latest distinct distances (zstd_ref_shape says how it arises).
# Only the sequential fallback of the device's history scan codes them right, and with that fallback
# switched off for them the device's frames differed on just the texts that hold them.  Every text
# of the dup-history family must hold one (test_dup_history_family), and the corpus 20 in all:
# several per text on the larger texts, so that they fall into different batches of 64 sequences.
FLOORS["dup_history_turns"] = 20


@functools.lru_cache(None)
def _lib():
    lib = ctypes.CDLL(Z.build_ref())
    lib.zstd_ref_shape.restype = ctypes.c_size_t
    lib.zstd_ref_shape.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
    return lib


def shape_of(texts):
    """The summed shape of some texts, by name."""
    c = (ctypes.c_uint64 * len(SHAPE_NAMES))()
    for t in texts:
        src = ctypes.create_string_buffer(t, len(t))
        assert _lib().zstd_ref_shape(src, len(t), c, len(SHAPE_NAMES)) == len(SHAPE_NAMES)
    return dict(zip(SHAPE_NAMES, (int(v) for v in c)))


@functools.lru_cache(None)
def shape():
    return shape_of(t for _, _, t in zstd_corpus.corpus())


def test_corpus_frames_decode():
    texts = zstd_corpus.corpus()
    assert texts == zstd_corpus.corpus.__wrapped__()  # seeded: the same texts every time
    assert len(texts) >= 150 and max(len(t) for _, _, t in texts) <= 2 * zstd_corpus.BLOCK
    for fam, i, t in texts:
        assert Z.zstd_decode(Z.ref_compress(t), len(t)) == t, (fam, i)


def test_corpus_shape_meets_floors():
    got = shape()
    print({k: got[k] for k in SHAPE_NAMES})
    low = {k: (got[k], f) for k, f in FLOORS.items() if got[k] < f}
    assert not low, low
    texts = zstd_corpus.corpus()
    assert f"{len(texts)} texts of {sum(len(t) for _, _, t in texts)} bytes" in __doc__
    stale = [k for k in SHAPE_NAMES if f"    {k:<24}{got[k]:>8}" not in __doc__]
    assert not stale, ("the docstring's measured shape is stale", {k: got[k] for k in stale})


def test_dup_history_family():
    """Each of these small texts holds the form by itself: they are what the single call sees of it."""
    texts = [(i, t) for fam, i, t in zstd_corpus.corpus() if fam == "dup-history"]
    assert texts
    for i, t in texts:
        assert shape_of([t])["dup_history_turns"] >= 1, i
