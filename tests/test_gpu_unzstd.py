"""zstd frames decoded on the device (K7u, sydelta_zstd_decompress_device): step 2 of
sy-remote's apply-delta (sy-remote.rs:153-179), so that the receiver's text never leaves HBM.

* The libzstd corpus of tests/zstd_frames.py (streaming at levels 1, 3, 19 and one-shot, the
  frames a real sy sender writes), the hand-assembled frames and frames of our own encoder,
  each equal to its input: by size query, at exact capacity and one byte short (nothing
  written, SYDELTA_OK, the size reported), with frame and output at tensor offsets 1 and 7.
* decompress(compress(text)) == text with both directions on the device.
* The receiver chain device.apply_wire for a libzstd frame, a frame of our own encoder and
  an uncompressed payload.
* The fixed malformed list (the one the sanitizer build of tests/test_unzstd_host.py has
  passed on the CPU): SYDELTA_E_INVAL each, and a valid decode right afterwards.
* Four host threads decoding different frames on their own streams."""
import ctypes
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import test_zstd as Z
import zstd_frames as F
from sy_amd import wire

pytestmark = pytest.mark.gpu

INPUTS = ("json-copies", "json-mixed", "json-literals", "json-small", "one", "empty", "sevens", "random-5000",
          "random-300000", "printable-x3", "two-symbols", "runs", "json-128k+1")


def _dev(data: bytes, offset: int = 0):
    import torch

    t = torch.zeros(offset + max(1, len(data)), dtype=torch.uint8, device="cuda")
    if data:
        t[offset:offset + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    return t[offset:offset + len(data)]


def _bytes(t) -> bytes:
    return t.cpu().numpy().tobytes()


def _check_all_forms(frame: bytes, data: bytes, name: str):
    import torch

    from sy_amd._lib import check, lib

    assert _bytes(wire.zstd_decompress_device(_dev(frame))) == data, name  # size query, then decode
    for fo, oo in ((1, 7), (7, 1)):
        d_frame = _dev(frame, fo)
        n = ctypes.c_uint64()
        # exact capacity, output at offset oo of a tensor whose other bytes must stay
        buf = torch.full((oo + len(data) + 9,), 0xA5, dtype=torch.uint8, device="cuda")
        got = wire.zstd_decompress_device(d_frame, out=buf[oo:oo + len(data)])
        assert got.numel() == len(data)
        h = _bytes(buf)
        assert h[oo:oo + len(data)] == data, name
        assert h[:oo] == b"\xa5" * oo and h[oo + len(data):] == b"\xa5" * 9, name
        if data:  # one byte short: nothing written, OK, the size reported
            buf.fill_(0xA5)
            check(lib.sydelta_zstd_decompress_device(0, d_frame.data_ptr(), d_frame.numel(), buf[oo:].data_ptr(),
                                                     len(data) - 1, ctypes.byref(n), None))
            torch.cuda.synchronize()
            assert n.value == len(data) and _bytes(buf) == b"\xa5" * buf.numel(), name


@pytest.mark.parametrize("name", INPUTS)
def test_libzstd_frames_decode_on_device(name, gpu):
    assert set(INPUTS) == set(F.corpus_inputs())
    for way, _ in F.WAYS:
        frame, data = F.corpus()[f"{name}-{way}"]
        _check_all_forms(frame, data, f"{name}-{way}")


def test_hand_assembled_frames_decode_on_device(gpu):
    for name, (frame, data) in F.hand_frames().items():
        assert Z.zstd_decode(frame, len(data)) == data, name
        _check_all_forms(frame, data, name)


@pytest.mark.parametrize("case", F.own_texts(), ids=lambda c: c[0])
def test_round_trip_on_device(case, gpu):
    """Our own encoder's frames: the host form's (direct weights, 14-byte header), and
    decompress(compress(text)) == text with both directions on the device."""
    name, data = case
    assert _bytes(wire.zstd_decompress_device(_dev(Z.ref_compress(data)))) == data
    frame = wire.zstd_compress_device(_dev(data))
    assert _bytes(wire.zstd_decompress_device(frame)) == data


def test_receiver_chain_on_device(gpu):
    """match -> Delta JSON (device) -> the sender's frame -> device.apply_wire == source."""
    import torch

    bs, n = 4096, 2 << 20
    basis = torch.empty(n, dtype=torch.uint8, device="cuda")
    gpu.synth_fill(basis, 0x5E1D0A11)
    h = basis.cpu().numpy().copy()
    rng = np.random.default_rng(5)
    for p in rng.integers(0, n, 40):
        h[p] ^= 0x5A
    ins = int(rng.integers(0, n))
    h = np.concatenate([h[:ins], rng.integers(0, 256, 777).astype(np.uint8), h[ins:]])
    src = torch.from_numpy(h).cuda()
    w, s = gpu.signature(basis, bs)
    ix = gpu.Index(w, s, bs, bs)
    delta = gpu.match(ix, src)
    ix.close()
    assert delta.stats["copy_ops"] > 0 and delta.stats["literal_bytes"] > 0
    text = wire.delta_to_json_device(delta.kind, delta.a, delta.b, src.numel(), bs, src)
    payloads = {"libzstd streaming level 3": _dev(F.stream_compress(_bytes(text), 3)),
                "our encoder": wire.zstd_compress_device(text), "uncompressed": text}
    assert _bytes(payloads["libzstd streaming level 3"][:4]) == F.MAGIC and _bytes(payloads["our encoder"][:4]) == F.MAGIC
    for name, payload in payloads.items():
        out, st = gpu.apply_wire(basis, payload)
        assert st["bytes_written"] == src.numel(), name
        assert torch.equal(out, src), name


def test_malformed_frames_are_refused(gpu):
    from sy_amd._lib import SYDELTA_E_INVAL, SyDeltaError

    frame, data = F.hand_frames()["hand-two-blocks"]
    good = _dev(frame)
    assert set(F.MALFORMED_REASON) == set(F.malformed())
    for name, bad in F.malformed().items():
        with pytest.raises(SyDeltaError) as e:
            wire.zstd_decompress_device(_dev(bad))
        assert e.value.code == SYDELTA_E_INVAL, name
        assert "zstd frame" in str(e.value) and F.MALFORMED_REASON[name] in str(e.value), (name, str(e.value))
        assert _bytes(wire.zstd_decompress_device(good)) == data, name


def test_four_threads_on_their_own_streams(gpu):
    import torch

    names = ("json-mixed-s3", "json-copies-s19", "printable-x3-s3", "sevens-s1")
    frames = [(_dev(F.corpus()[n][0]), F.corpus()[n][1]) for n in names]
    torch.cuda.synchronize()

    def one(k):
        st = torch.cuda.Stream()
        d_frame, data = frames[k]
        ok = 0
        for _ in range(20):
            with torch.cuda.stream(st):
                got = wire.zstd_decompress_device(d_frame, stream=st)
            ok += _bytes(got) == data
        return ok

    with ThreadPoolExecutor(4) as ex:
        assert list(ex.map(one, range(4))) == [20] * 4
