"""The device zstd block coder against the sequential host form on the shaped corpus.

z_block (sy_amd/csrc/sydelta_kernels.hip) codes what zstd::block_content_seq codes, but
everything behind the candidate search is its own wave-parallel code that no CPU test runs:
the take bitmap by ballots, 256 speculative segment walks chained by thread 0, literals and
sequence starts gathered by popcount ranks, the repeat-offset history resolved 64 sequences
at a time by a wave scan (with a sequential fallback), the literals section, and the
sequence bitstream with three FSE state chains on lanes 0 to 2 (none for a table in RLE
mode).  tests/zstd_corpus.py reaches those forms and tests/test_zstd_corpus.py holds it to
that; here every frame of the device must equal the host form's (tests/csrc/zstd_ref.cpp),
which libzstd decodes to the text: through the batched call, through the single call, and
through the batched call again with the texts in reverse order, since the coder's per-block
scratch in HBM is only partly zeroed and a frame must not depend on what an earlier block
left there."""
import functools

import numpy as np
import pytest

import test_zstd as Z
import zstd_corpus

pytestmark = pytest.mark.gpu


@functools.lru_cache(None)
def _refs():
    """The host form's frame of every corpus text, coded once."""
    return tuple(Z.ref_compress(t) for _, _, t in zstd_corpus.corpus())


def _blocks(frame: bytes):
    """(type, size, content offset) of the frame's blocks, walked by their 3-byte headers."""
    out, o = [], 14
    while o + 3 <= len(frame):
        h = int.from_bytes(frame[o:o + 3], "little")
        kind, size = (h >> 1) & 3, h >> 3
        out.append((kind, size, o + 3))
        o += 3 + (1 if kind == 1 else size)
        if h & 1:
            break
    return out


def _describe(fam, idx, text, got: bytes, ref: bytes) -> str:
    """Where a device frame leaves the host form's: the first differing block on each side,
    and whether libzstd still decodes the device frame to the text."""
    bg, br = _blocks(got), _blocks(ref)
    where = "no block differs (frame header or length)"
    for b in range(max(len(bg), len(br))):
        g = bg[b] if b < len(bg) else None
        r = br[b] if b < len(br) else None
        same = g and r and g[:2] == r[:2] and \
            got[g[2]:g[2] + (1 if g[0] == 1 else g[1])] == ref[r[2]:r[2] + (1 if r[0] == 1 else r[1])]
        if not same:
            where = f"block {b}: device (type, size) {g and g[:2]}, host {r and r[:2]}"
            break
    try:
        valid = "decodes to the text" if Z.zstd_decode(got, len(text)) == text else "decodes to another text"
    except ValueError as e:
        valid = f"libzstd refuses it ({e})"
    return f"{fam}[{idx}] of {len(text)} bytes: {len(got)} bytes for {len(ref)}; {where}; the device frame {valid}"


def _check(entries, frames):
    """entries: (family, index, text, host frame); frames: the device's, in the same order."""
    bad = [_describe(fam, i, t, g, r) for (fam, i, t, r), g in zip(entries, frames) if g != r]
    assert not bad, f"{len(bad)} of {len(entries)} frames differ from the host form:\n" + "\n".join(bad[:10])


def _batched(entries):
    import torch

    from sy_amd import wire

    offs, pos = [], 0
    for _, _, t, _ in entries:
        pos = -(-pos // 16) * 16
        offs.append(pos)
        pos += len(t)
    host = np.zeros(pos + 16, dtype=np.uint8)
    for o, (_, _, t, _) in zip(offs, entries):
        host[o:o + len(t)] = np.frombuffer(t, dtype=np.uint8)
    arena = torch.from_numpy(host).cuda()[:pos]
    out, foffs, flens = wire.zstd_compress_batch_device(arena, np.array(offs, dtype=np.uint64),
                                                        np.array([len(e[2]) for e in entries], dtype=np.uint64))
    got = out.cpu().numpy()
    return [got[int(o):int(o) + int(l)].tobytes() for o, l in zip(foffs, flens)]


def _entries():
    return [(fam, i, t, r) for (fam, i, t), r in zip(zstd_corpus.corpus(), _refs())]


def test_batched_call_equals_host_form(gpu):
    entries = _entries()
    _check(entries, _batched(entries))


def test_single_call_equals_host_form(gpu):
    """k_zstd_block's own addressing: every family's longest text (two blocks in three of
    them), every text of <= 1 KiB and the dup-history family, small texts made for this call."""
    import torch

    from sy_amd import wire

    every = _entries()
    longest = {name: max((e for e in every if e[0] == name), key=lambda e: len(e[2])) for name, _ in zstd_corpus.FAMILIES}
    entries = [e for e in every if len(e[2]) <= 1024 or longest[e[0]] is e or e[0] == "dup-history"]
    assert max(len(e[2]) for e in entries) > zstd_corpus.BLOCK
    frames = []
    for _, _, t, _ in entries:
        d = torch.zeros(len(t) + 16, dtype=torch.uint8, device="cuda")
        d[:len(t)] = torch.frombuffer(bytearray(t), dtype=torch.uint8).cuda()
        frames.append(bytes(wire.zstd_compress_device(d[:len(t)]).cpu().numpy()))
    _check(entries, frames)


def test_second_run_in_reverse_order_equals_host_form(gpu):
    """The same process codes the corpus again, last text first: every block now meets the
    scratch (bests, sequences, literals, stream words, FSE tables) of some other text's."""
    entries = _entries()
    _check(entries, _batched(entries))
    back = entries[::-1]
    _check(back, _batched(back))
