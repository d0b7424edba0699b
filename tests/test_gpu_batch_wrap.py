"""The batch calls past the end of their pinned staging rings (sy_amd/csrc/sydelta_stage.hpp):
each uploads its host tables through a few pinned slots, and a batch with more pieces than
slots reuses a slot while the call runs.  One case per call, each just past the wrap, each
against the reference its own test file uses.  The ring sizes are read from the headers and
every case first asserts that it wraps: a later change of a ring must fail the premise here,
not pass it without reusing a slot."""
import functools
import os
import re

import numpy as np
import pytest

import test_gpu_apply_batch as A
import test_gpu_json_batch as J
import test_zstd as Z
from oracle import oracle as O

pytestmark = pytest.mark.gpu

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sy_amd", "csrc")


def _const(header, name):
    """`constexpr uint32_t <name> = <decimal or a << b>` of a header in sy_amd/csrc."""
    text = open(os.path.join(CSRC, header)).read()
    m = re.search(r"constexpr uint32_t %s = (\d+)u?(?: << (\d+))?;" % name, text)
    assert m, (header, name)
    return int(m.group(1)) << int(m.group(2) or 0)


def _launches(gpu, call, kernel):
    """call() under the profiler: its result and the launches of `kernel`."""
    gpu.set_profiling(True)
    gpu.profile(reset=True)
    try:
        res = call()
        prof = gpu.profile(reset=True)
    finally:
        gpu.set_profiling(False)
    return res, sum(v["count"] for k, v in prof.items() if k.startswith(kernel))


def test_apply_batch_five_slices_in_a_ring_of_four(gpu):
    """600 files of 120 ops, Copy and Data alternating so that no two merge: 72 000 runs.  A
    slice holds at most kSliceRuns runs and is one k_applyb launch, so the table goes up in
    five slices and the fifth reuses the first's slot."""
    import torch

    ring, per = _const("sydelta_applybatch.hpp", "kRing"), _const("sydelta_applybatch.hpp", "kSliceRuns")
    nfiles, nops = 600, 120
    assert ring * per < nfiles * nops <= (ring + 1) * per  # more than a ring of slices, by one
    rng = np.random.default_rng(54)
    basis = rng.integers(0, 256, 4096, dtype=np.uint8)
    lit = rng.integers(0, 256, 4096, dtype=np.uint8)
    bbuf, boff, blen = A._pack([basis])
    lbuf, loff, llen = A._pack([lit])
    kind = np.arange(nops, dtype=np.uint32) % 2
    deltas, want, literal = [], [], []
    for f in range(nfiles):  # every file reads the one basis and the one literal buffer
        a = rng.integers(0, 4000, nops).astype(np.uint64)
        b = rng.integers(1, 90, nops).astype(np.uint64)
        deltas.append(gpu.DeviceDelta(kind, a, b, 0, 4096, {}))
        ops = [("D" if k else "C", int(x), int(y)) for k, x, y in zip(kind, a, b)]
        want.append(O.py_apply_delta(basis.tobytes(), lit.tobytes(), ops))
        literal.append(int(b[kind == 1].sum()))
    rep = np.zeros(nfiles, dtype=np.uint64)
    (out, ooffs, stats), launches = _launches(
        gpu, lambda: gpu.apply_batch(bbuf, rep + boff[0], rep + blen[0], deltas, lbuf, rep + loff[0], rep + llen[0]),
        "k_applyb")
    torch.cuda.synchronize()
    assert launches == ring + 1
    A._check_outputs(out, ooffs, want)
    assert A._stats_rows(stats) == [(nops, n, len(w)) for n, w in zip(literal, want)]


def test_json_batch_nine_slices_the_third_group_reuses_the_first(gpu):
    """_many_ops_files repeated to the smallest file count that gives nine slices: whole files
    go into a slice while their pairs (a pair per Copy op and one for the tail) leave room for
    a full Copy tile, so the count follows from kSlicePairs; a slice is one k_jsonb_len launch.
    The ring's two halves are groups of kRing / 2 slices: the ninth slice opens the third group,
    in the first group's slots."""
    import torch

    from sy_amd import wire

    ring, pairs, tile = (_const("sydelta_jsonbatch.hpp", n) for n in ("kRing", "kSlicePairs", "kCopyTile"))
    base = J._many_ops_files()
    texts = J._expected(base)
    per_file = [sum(1 for o in ops if o[0] == "C") + 1 for ops, _, _, _ in base]

    def slices(n):
        count, used = 1, 0
        for f in range(n):
            if used and per_file[f % len(base)] + tile > pairs - used:
                count, used = count + 1, 0
            used += per_file[f % len(base)]
        return count

    nfiles = next(n for n in range(1, 4096) if slices(n) == ring + 1)
    assert slices(nfiles) == ring + 1 == 9 and slices(nfiles - 1) == ring
    files = [base[f % len(base)] for f in range(nfiles)]
    lbuf, loff, llen = J._pack_literals(files, 5)
    one = J._deltas(gpu, base)
    (out, toffs, tlens), launches = _launches(
        gpu, lambda: wire.delta_batch_to_json_device([one[f % len(base)] for f in range(nfiles)], lbuf, loff, llen),
        "k_jsonb_len")
    torch.cuda.synchronize()
    assert launches == ring + 1
    host = out.cpu().numpy()
    at = 0
    for f in range(nfiles):
        t = texts[f % len(base)]
        assert int(toffs[f]) == at and int(tlens[f]) == len(t), f
        assert host[at:at + len(t)].tobytes() == t, f
        at += -(-len(t) // 16) * 16


@functools.lru_cache(None)
def _empty_frames():
    """2 * kStageFiles + 1 empty texts compressed in one call: (arena on the host, foffs, flens)."""
    import torch

    from sy_amd import wire

    slots, per = _const("sydelta_zstdbatch.hpp", "kStageSlots"), _const("sydelta_zstdbatch.hpp", "kStageFiles")
    assert (slots, per) == (2, 32768)
    n = slots * per + 1  # the third piece of the file table goes through the first slot again
    z = np.zeros(n, dtype=np.uint64)
    out, foffs, flens = wire.zstd_compress_batch_device(torch.empty(0, dtype=torch.uint8, device="cuda"), z, z)
    torch.cuda.synchronize()
    return out.cpu().numpy(), foffs, flens


def test_zstd_batch_three_pieces_of_the_file_table_in_two_slots(gpu):
    arena, foffs, flens = _empty_frames()
    n = len(foffs)
    assert n == 2 * 32768 + 1
    empty = Z.ref_compress(b"")
    assert len(empty) == 17
    assert np.array_equal(foffs, 17 * np.arange(n, dtype=np.uint64)) and (flens == 17).all()
    assert len(arena) == 17 * n  # out_need
    assert arena.tobytes() == empty * n


def test_unzstd_batch_three_pieces_of_the_file_table_in_two_slots(gpu):
    """The frames of the compress case fed back, 2 * 40 960 + 1 of them (the table of frames
    wraps; the bases, 16 384 to a slot, take six more uses behind it)."""
    import torch

    from sy_amd import wire

    slots, slot_bytes = _const("sydelta_unzstdbatch.hpp", "kStageSlots"), _const("sydelta_unzstdbatch.hpp", "kStageBytes")
    assert slots == 2 and slot_bytes // 16 == 40960  # sizeof(unzb::File) == 16
    arena, foffs, _ = _empty_frames()
    n = slots * (slot_bytes // 16) + 1
    pick = foffs[np.arange(n) % len(foffs)]
    text, toffs, tlens, status = wire.zstd_decompress_batch_device(torch.from_numpy(arena).cuda(), pick,
                                                                   np.full(n, 17, dtype=np.uint64), refused_ok=True)
    torch.cuda.synchronize()
    assert text.numel() == 0  # out_need
    assert not tlens.any() and not status.any() and not toffs.any()
