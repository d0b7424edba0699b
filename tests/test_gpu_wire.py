"""Device Delta JSON writer (K7) against the host writer and against an independent
writer -- Python's json.dumps with serde's compact separators and the field order of
generator.rs:10-25 (ssh.rs:1003 serde_json::to_string(&delta)): bit-identical text for
copy-heavy, literal-heavy (multi-chunk Data runs) and mixed deltas, including empty
Data ops, and for a text past 2^32 bytes."""
import json
import random

import numpy as np
import pytest

from sy_amd import wire

pytestmark = pytest.mark.gpu


def _cases():
    rng = random.Random(9)
    src = rng.randbytes(3 << 20)
    yield "one-literal", [1], [0], [len(src)], src
    yield "empty", [], [], [], src
    yield "empty-data", [1, 0, 1], [0, 4096, 5], [0, 4096, 0], src
    kind, a, b = [], [], []
    pos = 0
    while pos < len(src) - 20000:
        if rng.random() < 0.5:
            kind.append(0); a.append(rng.randrange(1 << 40)); b.append(rng.choice([4096, 8192, 17]))
        else:
            n = rng.choice([1, 2, 99, 4095, 4096, 4097, 16383, 16384, 16385, 40000])
            kind.append(1); a.append(pos); b.append(n)
            pos += n
    yield "mixed", kind, a, b, src
    yield "copies", [0] * 5000, [i * 8192 for i in range(5000)], [8192] * 5000, src


def _dumps(kind, a, b, source_size, bs, src) -> bytes:
    """serde_json::to_string(&Delta) restated with json.dumps (generator.rs:10-25:
    DeltaOp::Copy{offset,size} / DeltaOp::Data(Vec<u8>), then source_size, block_size)."""
    ops = [{"Copy": {"offset": x, "size": y}} if k == 0 else {"Data": list(src[x:x + y])}
           for k, x, y in zip(kind, a, b)]
    return json.dumps({"ops": ops, "source_size": source_size, "block_size": bs}, separators=(",", ":")).encode()


@pytest.mark.parametrize("case", list(_cases()), ids=lambda c: c[0])
def test_device_json_equals_host(case, gpu):
    import torch

    name, kind, a, b, src = case
    host = wire.delta_to_json(kind, a, b, len(src), 4096, src)
    d = torch.frombuffer(bytearray(src), dtype=torch.uint8).cuda()
    dev = wire.delta_to_json_device(kind, a, b, len(src), 4096, d)
    torch.cuda.synchronize()
    got = bytes(dev.cpu().numpy())
    assert len(got) == len(host)
    assert got == host
    assert got == _dumps(kind, a, b, len(src), 4096, src)


def test_device_json_past_4gib_against_dumps(gpu):
    """A 1.25 GiB literal run of a 256-byte period (a permutation of 0..255), then a
    Copy and a short Data run: > 4 GiB of text.  json.dumps writes one period's text and
    the ops around the run; the device text is compared with them on the device, the
    run as a [periods x period-text] view."""
    import torch

    P, L = 256, 5 << 28
    perm = np.random.default_rng(17).permutation(P).astype(np.uint8)
    lit = torch.from_numpy(perm).cuda().repeat(L // P + 1)[:L + 16].contiguous()
    kind, a, b = [1, 0, 1], [0, 12345, 100], [L, 4096, 5]
    text = wire.delta_to_json_device(kind, a, b, L + 4096, 4096, lit[:L])
    torch.cuda.synchronize()
    period = json.dumps(perm.tolist(), separators=(",", ":"))[1:-1].encode() + b","  # "v0,v1,...,v255,"
    T = len(period)
    head = b'{"ops":[{"Data":['
    rest = json.dumps({"ops": [{"Data": []}, {"Copy": {"offset": 12345, "size": 4096}},
                               {"Data": perm[100:105].tolist()}], "source_size": L + 4096, "block_size": 4096},
                      separators=(",", ":")).encode()
    rest = rest[rest.index(b"]},"):]  # from the first (empty) Data op's "]"
    nrep = L // P
    assert text.numel() == len(head) + nrep * T - 1 + len(rest)
    assert text.numel() > (1 << 32)
    assert bytes(text[:len(head)].cpu().numpy()) == head
    body = text[len(head):len(head) + nrep * T].view(nrep, T)
    row = torch.frombuffer(bytearray(period), dtype=torch.uint8).cuda()
    assert bool((body[:-1] == row).all())
    assert bool((body[-1, :T - 1] == row[:T - 1]).all())
    assert bytes(text[len(head) + nrep * T - 1:].cpu().numpy()) == rest


def test_device_json_text_past_4gib(gpu):
    """A 1.25 GiB literal run: ~3.75 GiB of Data text plus a second run pushes the text
    offsets past 2^32 (a 32-bit scan would wrap)."""
    import torch

    L = 5 << 28  # 1.25 GiB
    lit = torch.full((L + 16,), 200, dtype=torch.uint8, device="cuda")  # "200," per byte
    lit[L - 1] = 7
    kind, a, b = [1, 0, 1], [0, 12345, L - 5], [L, 4096, 5]
    text = wire.delta_to_json_device(kind, a, b, L + 4096, 4096, lit[:L])
    torch.cuda.synchronize()
    body0 = 9 + 4 * (L - 1) + 1 + 2              # {"Data":[200,...,200,7]}
    copy = 1 + len('{"Copy":{"offset":12345,"size":4096}}')
    tail_data = 1 + len('{"Data":[200,200,200,200,7]}')
    tail = len('],"source_size":%d,"block_size":4096}' % (L + 4096))
    assert text.numel() == 8 + body0 + copy + tail_data + tail
    assert text.numel() > (1 << 32)
    head = bytes(text[:24].cpu().numpy())
    assert head == b'{"ops":[{"Data":[200,200'
    end = bytes(text[-(copy + tail_data + tail + 7):].cpu().numpy())
    assert end == (b'200,7]},{"Copy":{"offset":12345,"size":4096}},{"Data":[200,200,200,200,7]}'
                   + b'],"source_size":%d,"block_size":4096}' % (L + 4096))


# ---------------------------------------------------------------------------
# k_json_write's staging: the scan over 256 threads, the 4 * 4096 + 32 byte LDS text, the
# 16-byte stores phased on the destination address; k_json_len's and k_json_write's
# unaligned literal loads.  Each text against delta_json_ref.compact (json.dumps) and the
# host writer, then back through the device parser (K7d) to the ops and literals.
# ---------------------------------------------------------------------------
from delta_json_ref import compact  # noqa: E402


def _ops_of(kind, a, b, lit: bytes):
    return [("C", x, y) if k == 0 else ("D", lit[x:x + y]) for k, x, y in zip(kind, a, b)]


def _check_text(kind, a, b, ss, bs, lit: bytes, d_lit=None):
    """Device text == compact == host text; the device parser reads it back.  Returns the text."""
    import torch

    ops = _ops_of(kind, a, b, lit)
    ref = compact(ops, ss, bs)
    assert wire.delta_to_json(kind, a, b, ss, bs, lit) == ref
    if d_lit is None:
        d_lit = torch.frombuffer(bytearray(lit) or bytearray(1), dtype=torch.uint8).cuda()[:len(lit)]
    dev = wire.delta_to_json_device(kind, a, b, ss, bs, d_lit)
    torch.cuda.synchronize()
    got = dev.cpu().numpy().tobytes()
    assert len(got) == len(ref)
    assert got == ref
    dops, dl, dss, dbs = wire.delta_from_json_device(dev)
    back = dl.cpu().numpy().tobytes()
    assert ([("C", x, y) if k == 0 else ("D", back[x:x + y]) for k, x, y in dops], dss, dbs) == (ops, ss, bs)
    return ref


def _mixed_small():
    rng = random.Random(12)
    lit = rng.randbytes(30000)
    kind, a, b, pos = [], [], [], 0
    for n in (0, 1, 5000, 4096, 0, 4097, 17, 8192, 3):
        kind += [0, 1]
        a += [rng.randrange(1 << rng.choice((4, 30, 63))), pos]
        b += [4096, n]
        pos += n
    return kind, a, b, lit


def test_device_json_destination_alignment(gpu):
    """d_out at offsets 1, 3, 8, 15 from a 16-byte boundary with out_cap == len exactly:
    the text, and every byte around it unchanged; with out_cap == len - 1 nothing is
    written and *out_len is still len."""
    import ctypes

    import torch

    from sy_amd._lib import check, lib

    kind, a, b, lit = _mixed_small()
    ref = _check_text(kind, a, b, len(lit), 4096, lit)
    d_lit = torch.frombuffer(bytearray(lit), dtype=torch.uint8).cuda()
    h = wire._delta_handle(kind, a, b, len(lit), 4096)
    try:
        got = ctypes.c_uint64()
        for shift in (1, 3, 8, 15):
            for cap in (len(ref), len(ref) - 1):
                out = torch.full((len(ref) + 64,), 0xEE, dtype=torch.uint8, device="cuda")
                assert out.data_ptr() % 16 == 0
                check(lib.sydelta_delta_to_json_device(h, d_lit.data_ptr(), d_lit.numel(), out.data_ptr() + 16 + shift,
                                                       cap, ctypes.byref(got), None))
                torch.cuda.synchronize()
                o = out.cpu().numpy()
                assert got.value == len(ref), (shift, cap)
                if cap == len(ref):
                    assert o[16 + shift:16 + shift + len(ref)].tobytes() == ref, shift
                    assert (o[:16 + shift] == 0xEE).all() and (o[16 + shift + len(ref):] == 0xEE).all(), shift
                else:
                    assert (o == 0xEE).all(), shift
    finally:
        lib.sydelta_delta_free(h)


@pytest.mark.parametrize("value,n", [(255, 4096), (0, 4096), (255, 4097), (0, 4097), (255, 8192), (0, 8192),
                                     (255, 12288), (0, 12288)])
def test_device_json_full_chunk_on_every_destination_phase(value, n, gpu):
    """A Data op of n equal bytes as a non-first op, in pieces of 4096 bytes: one piece that
    carries Sep, First and Last (4096; all-255: 16410 of the 16416 staged bytes at phase
    15; all-0: the shortest text), a Last piece of 1 byte (4097), a full First and a full
    Last piece (8192), a middle piece with neither (12288).  The digits of the Copy before
    the op put its first piece on each destination phase 0..15."""
    lit = bytes([value]) * n + b"\x07"
    phases = set()
    for digits in range(1, 17):
        kind, a, b = [0, 1, 1], [10 ** (digits - 1), 0, n], [1, n, 1]
        ref = _check_text(kind, a, b, n + 1, 4096, lit)
        phases.add(ref.index(b',{"Data"') % 16)
    assert phases == set(range(16))


@pytest.mark.parametrize("shift", [0, 1])
def test_device_json_digit_class_changes_at_thread_and_wave_boundaries(shift, gpu):
    """1-, 2- and 3-digit values changing exactly every 16 bytes (a thread's share, and so
    at every 1024-byte wave boundary too), and the same pattern one byte later."""
    pat = []
    for k in range(3 * 4096 // 16):
        pat += [(9, 10, 99, 100, 255, 0, 200, 7)[k % 8]] * 16
    lit = bytes([5] * shift + pat)
    _check_text([1, 0, 1], [0, 1, 4096 + shift], [4096 + shift, 1, len(lit) - 4096 - shift], len(lit), 4096, lit)


@pytest.mark.parametrize("view", [1, 2, 3])
def test_device_json_literal_base_off_alignment(view, gpu):
    """The literal tensor viewed at offsets 1, 2, 3 with Data ops whose source offsets are
    multiples of 16: the base, not the op, sends k_json_len and k_json_write down their
    unaligned loads."""
    import torch

    rng = random.Random(50 + view)
    lit = rng.randbytes(3 * 4096 + 160)
    whole = torch.frombuffer(bytearray(b"\xEE" * view + lit + b"\xEE" * 16), dtype=torch.uint8).cuda()
    assert whole.data_ptr() % 16 == 0
    d_lit = whole[view:view + len(lit)]
    kind, a, b = [1, 0, 1, 1, 1], [0, 99, 4096 + 64, 2 * 4096 + 64, 3 * 4096 + 96], [4096 + 64, 4096, 4096, 4096 + 32, 64]
    assert all(x % 16 == 0 for k, x in zip(kind, a) if k == 1)
    _check_text(kind, a, b, len(lit), 4096, lit, d_lit)
