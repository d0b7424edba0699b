"""The device zstd decoder (sydelta_unzstd.hip, sydelta_unzstdbatch.hip) on the frame forms no
sender here writes: the families tests/zstd_frames.py assembles from RFC 8878 (its docstring
lists them), whose expectation is a replay of (literals, offset, match length) that shares
nothing with the decoder, and which libzstd decodes to the same bytes.

* Every family through wire.zstd_decompress_device, a test each: offset codes 17 to 27 (of27:
  256 MiB of output, the one size at which k_unz_place and k_unz_gather go round their grid-stride
  loop twice), LL code 35 and ML code 52 filling a block to exactly 128 KiB, 24 + 12 + 12 extra
  bits a sequence, Huffman trees of 12 and 11 bits (the 4096-entry LDS copy), chains as long as
  the output up to 128 MiB (jump shares above 256 bytes from 8 MiB on), empty blocks, 3000 blocks.
  Frames of at most 1 MiB also by size query, at exact capacity with guard bytes, one byte short
  and at tensor offsets (1, 7) and (7, 1).
* F.far_frame(): libzstd at level 19 with a match 5 MiB back, whose FSE-compressed tables hold the
  offset and literal-length codes the families carry in RLE_Mode.
* The refused twins (an offset one byte before the output's start, for every offset code; a block
  of 128 KiB + 1): SYDELTA_E_INVAL naming block and reason, nothing written, a valid decode right
  afterwards.  The sanitizer build of tests/test_unzstd_host.py has passed the same frames.
* One batch of all families up to of25 with corpus frames between them, and one with refused
  frames between good ones, through the batched call.
* The profile of the largest decodes: the run went through the place, doubling and gather kernels.

Offset codes 28 to 31 are not reached: they need 512 MiB to 2 GiB of output."""
import random

import numpy as np
import pytest

import test_zstd as Z
import zstd_frames as F
from sy_amd import wire
from test_gpu_unzstd import _bytes, _check_all_forms, _dev
from test_gpu_unzstd_batch import CANARY, _arena, _check_texts, _packing

pytestmark = pytest.mark.gpu

SMALL = 1 << 20
K_OFFSET, K_BLOCK_BIG = 19, 9  # unz::Err (sydelta_unzstd.hpp), the low word of a status key
# the batch: every family but the three largest (its text stays below 200 MiB)
BATCH = tuple(n for n in F.FORMS if n not in ("of26", "of27", "deep1-1024"))
BETWEEN = ("json-small-s1", "one-s3", "empty-s3", "json-mixed-s19", "random-5000-s3")


def _same(got, want: np.ndarray, name: str):
    """A device tensor against the expectation, compared on the device."""
    import torch

    w = torch.from_numpy(want).to(got.device)
    assert got.numel() == w.numel(), (name, got.numel(), w.numel())
    if not torch.equal(got, w):
        at = int((got != w).nonzero()[0])
        pytest.fail(f"{name}: first difference at byte {at} of {w.numel()}: {int(got[at])} for {int(w[at])}")


def _decode_checked(name: str):
    frame, ops = F.form(name)
    want = F.expect(ops)
    ref = Z.zstd_decode(frame, len(want) + 1)  # libzstd is the referee of the assembler
    assert len(ref) == len(want) and np.array_equal(np.frombuffer(ref, dtype=np.uint8), want), name
    del ref
    d_frame = _dev(frame)
    _same(wire.zstd_decompress_device(d_frame), want, name)
    return frame, want, d_frame


@pytest.mark.parametrize("name", [n for n in F.FORMS if n not in ("of27", "deep1-1024")])
def test_family_decodes_on_device(name, gpu):
    frame, want, _ = _decode_checked(name)
    if len(want) <= SMALL:
        _check_all_forms(frame, want.tobytes(), name)


def test_far_libzstd_frame_decodes_on_device(gpu):
    """libzstd at level 19 with a match 5 MiB back: FSE-compressed tables that hold offset code 22
    and literal-length code 34 (asserted by tests/test_unzstd_host.py on the CPU)."""
    frame, data = F.far_frame()
    tabs = F.fse_tables(frame)
    assert any(len(t[1][1]) - 1 >= 22 for t in tabs if 1 in t) and any(len(t[0][1]) - 1 >= 32 for t in tabs if 0 in t)
    _same(wire.zstd_decompress_device(_dev(frame)), np.frombuffer(data, dtype=np.uint8).copy(), "far-s19")


@pytest.mark.parametrize("name", ["of27", "deep1-1024"])
def test_largest_decodes_go_through_the_doubling_kernels(name, gpu):
    """of27: 2^28 + 44 bytes, above the 2^20 workgroups of 256 bytes that k_unz_place and k_unz_gather
    launch at most.  deep1-1024: 128 MiB that hang from byte 0 by one chain.  A second decode into a
    tensor of the known size, profiled: one scope each of place, the doubling (the profiler counts
    its kUnzRounds launches as one scope) and gather, and no kernel of another path."""
    import torch

    _, want, d_frame = _decode_checked(name)
    out = torch.full((len(want) + 9,), CANARY, dtype=torch.uint8, device="cuda")
    gpu.set_profiling(True)
    gpu.profile(reset=True)
    try:
        got = wire.zstd_decompress_device(d_frame, out=out[:len(want)])
        prof = gpu.profile(reset=True)
    finally:
        gpu.set_profiling(False)
    _same(got, want, name)
    assert bool((out[len(want):] == CANARY).all())
    counts = {k: v["count"] for k, v in prof.items() if k != "__busy__"}
    assert all(k.startswith("k_unz_") for k in counts), counts
    for stage in ("tables", "decode", "stitch", "resolve", "place", "jump", "gather"):
        assert counts.get(f"k_unz_{stage}") == 1, counts


@pytest.mark.parametrize("name", list(F.FORMS_REFUSED))
def test_refused_frames_write_nothing(name, gpu):
    import torch

    from sy_amd._lib import SYDELTA_E_INVAL, SyDeltaError

    frame = F.form_refused(name)
    assert (F.libzstd_accepts(frame, 1 << 29) is None) == (name != "ml-over")
    d_frame = _dev(frame)
    size = (128 << 10) + 1 if name == "ml-over" else (1 << int(name[2:4]) + 1) + 23  # what it would regenerate
    buf = torch.full((size + 9,), CANARY, dtype=torch.uint8, device="cuda")
    for out in (None, buf[:size], buf[1:8]):  # the size query too, and an output far too small
        with pytest.raises(SyDeltaError) as e:
            wire.zstd_decompress_device(d_frame, out=out)
        assert e.value.code == SYDELTA_E_INVAL, name
        assert "zstd frame" in str(e.value) and F.FORMS_REFUSED[name] in str(e.value), (name, str(e.value))
        torch.cuda.synchronize()
        assert bool((buf == CANARY).all()), name
    good, data = F.hand_frames()["hand-two-blocks"]
    assert _bytes(wire.zstd_decompress_device(_dev(good))) == data, name


def test_all_families_in_one_batch(gpu):
    """Shuffled with a fixed seed, corpus frames between them: every text at the packing rule's
    offset, equal to the expectation and to the single call's, every other byte untouched."""
    import torch

    items = [(n,) + F.form(n) for n in BATCH]
    items = [(n, f, F.expect(ops)) for n, f, ops in items]
    items += [(n, F.corpus()[n][0], np.frombuffer(F.corpus()[n][1], dtype=np.uint8)) for n in BETWEEN]
    items.append(("far-s19", F.far_frame()[0], np.frombuffer(F.far_frame()[1], dtype=np.uint8)))
    random.Random(17).shuffle(items)
    lens = [len(w) for _, _, w in items]
    want_off, need = _packing(lens)
    assert need < 1 << 28  # far below the 4 GiB limit
    arena, foffs, flens = _arena([f for _, f, _ in items], 3)
    host = np.full(5 + need + 9, CANARY, dtype=np.uint8)
    for o, (_, _, w) in zip(want_off, items):
        host[5 + int(o):5 + int(o) + len(w)] = w
    buf = torch.full((5 + need + 9,), CANARY, dtype=torch.uint8, device="cuda")
    out, toffs, tlens = gpu.wire_batch_to_text(arena, foffs, flens, out=buf[5:5 + need])
    assert out.numel() == need and np.array_equal(toffs, want_off) and [int(x) for x in tlens] == lens
    _same(buf, host, "the batch's arena")
    for f, (name, _, w) in enumerate(items):
        o, l = int(foffs[f]), int(flens[f])
        alone = wire.zstd_decompress_device(arena[o:o + l])
        assert torch.equal(alone, out[int(toffs[f]):int(toffs[f]) + len(w)]), name


def test_refused_frames_between_good_ones_in_a_batch(gpu):
    import torch

    from sy_amd._lib import SYDELTA_E_INVAL, SyDeltaError

    def good(name):
        frame, ops = F.form(name)
        return frame, F.expect(ops).tobytes()

    files = [F.corpus()["json-small-s1"], (F.form_refused("of20-short"), b""), good("deep3"),
             (F.form_refused("ml-over"), b""), good("empties-seq"), good("of17")]
    texts = [d for _, d in files]
    arena, foffs, flens = _arena([f for f, _ in files], 5)
    _, need = _packing([len(t) for t in texts])
    buf = torch.full((3 + need + 9,), CANARY, dtype=torch.uint8, device="cuda")
    with pytest.raises(SyDeltaError) as e:  # without the status table: the first refused file, nothing written
        wire.zstd_decompress_batch_device(arena, foffs, flens, out=buf[3:])
    torch.cuda.synchronize()
    assert e.value.code == SYDELTA_E_INVAL
    assert "file 1: zstd frame: " + F.FORMS_REFUSED["of20-short"] in str(e.value), str(e.value)
    assert bool((buf == CANARY).all())
    out, toffs, tlens, status = wire.zstd_decompress_batch_device(arena, foffs, flens, out=buf[3:], refused_ok=True)
    torch.cuda.synchronize()
    assert [int(x) for x in status] == [0, 16 << 32 | K_OFFSET, 0, K_BLOCK_BIG, 0, 0], status
    assert out.numel() == need
    assert _check_texts(buf.cpu().numpy(), 3, toffs, tlens, texts) == need
