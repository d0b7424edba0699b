"""The block coder's '{' distance counts (z_gap_count) over the first 259 bytes of a block.

Those positions count byte by byte, and the lanes of one wave step through the distances
together: two '{' at the same distance from an earlier one (Copy ops repeat every 44 bytes or
so) add to the same LDS word in the same step.  With a plain ++ such a pair counted once; a
3563-byte text whose distances 52 and 80 then stood 15 : 16 instead of 17 : 16 chose another
candidate distance and coded 1465 bytes where the sequential host form codes 1464.  Small
copy-heavy texts, where the first 259 bytes carry a large part of the counts, through the
single and the batched call against tests/csrc/zstd_ref.cpp."""
import functools
import random

import numpy as np
import pytest

import test_zstd as Z

pytestmark = pytest.mark.gpu


@functools.lru_cache(None)
def _texts():
    rng = random.Random(600)
    small = [Z.delta_json(rng, 3 + f % 38, 0.2) for f in range(600)]
    rng = random.Random(44)
    texts = [small[365]] + [Z.delta_json(rng, k, lit) for k in (6, 12, 25, 40, 90) for lit in (0.0, 0.1, 0.3)]
    assert len(texts[0]) == 3563 and sum(len(t) for t in texts) <= 256 << 10
    return texts, [Z.ref_compress(t) for t in texts]


def test_single_call_counts_colliding_gaps(gpu):
    import torch

    from sy_amd import wire

    texts, refs = _texts()
    for f, (t, r) in enumerate(zip(texts, refs)):
        d = torch.zeros(len(t) + 16, dtype=torch.uint8, device="cuda")
        d[:len(t)] = torch.frombuffer(bytearray(t), dtype=torch.uint8).cuda()
        frame = bytes(wire.zstd_compress_device(d[:len(t)]).cpu().numpy())
        assert len(frame) == len(r) and frame == r, (f, len(t), len(frame), len(r))
        assert Z.zstd_decode(frame, len(t)) == t, f


def test_batched_call_counts_colliding_gaps(gpu):
    import torch

    from sy_amd import wire

    texts, refs = _texts()
    offs, pos = [], 0
    for t in texts:
        pos = -(-pos // 16) * 16
        offs.append(pos)
        pos += len(t)
    host = np.zeros(pos + 16, dtype=np.uint8)
    for o, t in zip(offs, texts):
        host[o:o + len(t)] = np.frombuffer(t, dtype=np.uint8)
    arena = torch.from_numpy(host).cuda()[:pos]
    out, foffs, flens = wire.zstd_compress_batch_device(arena, np.array(offs, dtype=np.uint64),
                                                        np.array([len(t) for t in texts], dtype=np.uint64))
    got = out.cpu().numpy()
    for f, r in enumerate(refs):
        o, l = int(foffs[f]), int(flens[f])
        assert l == len(r) and got[o:o + l].tobytes() == r, (f, l, len(r))
