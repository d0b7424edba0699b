"""Frames for the zstd decoder's tests (tests/test_unzstd_host.py, tests/test_gpu_unzstd.py):
the system libzstd driven the way compress/mod.rs:70-75 drives it (streaming, no pledged
size), hand-assembled frames for the forms libzstd never emits, the fixed malformed list,
and a small frame reader that says which forms a frame holds, so that a test can assert
what its corpus covers."""
import ctypes
import functools
import random

from test_zstd import _cases, _libzstd, delta_json, zstd_decode

MAGIC = b"\x28\xb5\x2f\xfd"
E_CONTINUE, E_END = 0, 2
C_LEVEL = 100  # ZSTD_c_compressionLevel


class _Buf(ctypes.Structure):  # ZSTD_inBuffer / ZSTD_outBuffer
    _fields_ = [("p", ctypes.c_void_p), ("size", ctypes.c_size_t), ("pos", ctypes.c_size_t)]


@functools.lru_cache(None)
def _z():
    z = _libzstd()
    if z is None:
        return None
    z.ZSTD_createCCtx.restype = ctypes.c_void_p
    z.ZSTD_freeCCtx.argtypes = [ctypes.c_void_p]
    z.ZSTD_CCtx_setParameter.restype = ctypes.c_size_t
    z.ZSTD_CCtx_setParameter.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    z.ZSTD_compressStream2.restype = ctypes.c_size_t
    z.ZSTD_compressStream2.argtypes = [ctypes.c_void_p, ctypes.POINTER(_Buf), ctypes.POINTER(_Buf), ctypes.c_int]
    z.ZSTD_compressBound.restype = ctypes.c_size_t
    z.ZSTD_compressBound.argtypes = [ctypes.c_size_t]
    z.ZSTD_compress.restype = ctypes.c_size_t
    z.ZSTD_compress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    return z


def libzstd_path() -> str:
    """File of the loaded libzstd (the sanitizer program links it)."""
    for line in open("/proc/self/maps"):
        # the system library alone: test_zstd's host form is build/zstd_ref/libzstd_ref.so, and which
        # of the two the kernel maps lower depends on what else the process has loaded
        if "/libzstd.so" in line:
            return line.split()[-1]
    raise RuntimeError("libzstd is not loaded")


def stream_compress(data: bytes, level: int = 3, step: int = 32 << 10) -> bytes:
    """ZSTD_compressStream2 fed in `step`-byte pieces, then ZSTD_e_end: no content size."""
    z = _z()
    cctx = z.ZSTD_createCCtx()
    try:
        assert not z.ZSTD_isError(z.ZSTD_CCtx_setParameter(cctx, C_LEVEL, level))
        cap = z.ZSTD_compressBound(len(data)) + 64
        dst = ctypes.create_string_buffer(cap)
        src = ctypes.create_string_buffer(data, max(1, len(data)))
        out = _Buf(ctypes.cast(dst, ctypes.c_void_p), cap, 0)
        pos = 0
        while pos < len(data):
            n = min(step, len(data) - pos)
            inp = _Buf(ctypes.cast(src, ctypes.c_void_p).value + pos, n, 0)
            while inp.pos < inp.size:
                r = z.ZSTD_compressStream2(cctx, ctypes.byref(out), ctypes.byref(inp), E_CONTINUE)
                assert not z.ZSTD_isError(r)
            pos += n
        inp = _Buf(ctypes.cast(src, ctypes.c_void_p), 0, 0)
        while True:
            r = z.ZSTD_compressStream2(cctx, ctypes.byref(out), ctypes.byref(inp), E_END)
            assert not z.ZSTD_isError(r)
            if r == 0:
                break
        return dst.raw[:out.pos]
    finally:
        z.ZSTD_freeCCtx(cctx)


def oneshot_compress(data: bytes, level: int = 3) -> bytes:
    z = _z()
    cap = z.ZSTD_compressBound(len(data)) + 64
    dst = ctypes.create_string_buffer(cap)
    src = ctypes.create_string_buffer(data, max(1, len(data)))
    r = z.ZSTD_compress(dst, cap, src, len(data), level)
    assert not z.ZSTD_isError(r)
    return dst.raw[:r]


def libzstd_accepts(frame: bytes, cap: int):
    """The bytes libzstd regenerates, or None when it refuses the frame."""
    try:
        return zstd_decode(frame, cap)
    except ValueError:
        return None


# ---- hand-assembled frames -----------------------------------------------------------
HEADER = MAGIC + b"\x00\x38"  # FHD 0: no content size, no checksum; a 128 KiB window


def block(btype: int, content: bytes, last: bool, size: int | None = None) -> bytes:
    h = (len(content) if size is None else size) << 3 | btype << 1 | int(last)
    return h.to_bytes(3, "little") + content


def rle_seq_content(n: int, byte: int = 0x41, ll_sym: int = 1) -> bytes:
    """RLE literals (n of `byte`), n sequences in RLE_Mode: LL = ll_sym, OF code 0, ML code 0
    (a 3-byte match at repeat offset 1): with ll_sym 1 the byte 4 n times."""
    lit = (1 | 3 << 2 | n << 4).to_bytes(3, "little") + bytes([byte])
    if n < 128:
        cnt = bytes([n])
    elif n < 0x7F00:
        cnt = bytes([(n >> 8) + 128, n & 255])
    else:
        cnt = b"\xff" + (n - 0x7F00).to_bytes(2, "little")
    return lit + cnt + b"\x54" + bytes([ll_sym, 0, 0]) + b"\x01"


def rle_seq_frame(ns, byte: int = 0x41, ll_sym: int = 1) -> bytes:
    ns = list(ns)
    return HEADER + b"".join(block(2, rle_seq_content(n, byte + i, ll_sym), i == len(ns) - 1)
                             for i, n in enumerate(ns))


HAND_COUNTS = (1, 127, 128, 32511, 32512, 32768)


def hand_frames():
    """name -> (frame, expected bytes); each one is checked against libzstd by its test."""
    out = {f"hand-n{n}": (rle_seq_frame([n]), b"A" * (4 * n)) for n in HAND_COUNTS}
    out["hand-two-blocks"] = (rle_seq_frame([1000, 5]), b"A" * 4000 + b"B" * 20)
    return out


# ---- the corpus ------------------------------------------------------------------------
@functools.lru_cache(None)
def corpus_inputs():
    rng = random.Random(3)  # with this seed every JSON text has 4 blocks and level 19 writes modes (3, 3, 2)
    cases = dict(_cases())
    js = delta_json(rng, 8000, 0.01)
    mixed, literals = delta_json(rng, 2500, 0.3), delta_json(rng, 800, 0.9)
    rng = random.Random(11)
    printable = bytes(rng.randrange(32, 127) for _ in range(300000))
    return {
        "json-copies": js,
        "json-mixed": mixed,
        "json-literals": literals,
        "json-small": delta_json(rng, 3, 0.5),
        "one": b"{",
        "empty": b"",
        "sevens": b"7" * 300000,
        "random-5000": bytes(rng.randrange(256) for _ in range(5000)),
        "random-300000": random.Random(12).randbytes(300000),
        "printable-x3": printable * 3,
        "two-symbols": bytes(rng.choice(b"01") for _ in range(70000)),
        "runs": cases["runs"],
        "json-128k+1": js[:(128 << 10) + 1],
    }


WAYS = (("s1", lambda d: stream_compress(d, 1)), ("s3", lambda d: stream_compress(d, 3)),
        ("s19", lambda d: stream_compress(d, 19)), ("o3", lambda d: oneshot_compress(d, 3)))


@functools.lru_cache(None)
def corpus():
    """name -> (frame, expected bytes): every input compressed four ways by libzstd."""
    out = {}
    for name, data in corpus_inputs().items():
        for way, fn in WAYS:
            out[f"{name}-{way}"] = (fn(data), data)
    return out


def own_texts():
    """The texts whose frames our own encoder writes (test_zstd._cases)."""
    return list(_cases())


# ---- the fixed malformed list ----------------------------------------------------------
def malformed():
    good = rle_seq_frame([5])
    raw = HEADER + block(0, b"hello", True)
    return {
        "wrong-magic": b"\x27" + raw[1:],
        "len-3": raw[:3],
        "len-5": raw[:5],
        "checksum-flag": MAGIC + b"\x04\x38" + raw[6:] + b"\x00\x00\x00\x00",
        "dictionary-id-1": MAGIC + b"\x01\x38\x01" + raw[6:],
        "reserved-fhd-bit": MAGIC + b"\x08\x38" + raw[6:],
        "block-type-3": HEADER + block(3, b"hello", True),
        "block-beyond-len": HEADER + block(0, b"hello", True, size=6),
        "no-last-block": HEADER + block(0, b"hello", False) + block(0, b"again", False),
        "first-block-treeless": HEADER + block(2, bytes([3 | 0 << 2 | (4 & 15) << 4, 4 >> 4 | 1 << 6, 0]) + b"\x01\x00",
                                               True),
        "first-block-repeat-mode": HEADER + block(2, b"\x08A" + b"\x01\xfc" + b"\x01", True),
        "ll0-offset-before-start": rle_seq_frame([5], ll_sym=0),
        "trailing-byte": good + b"\x00",
    }


# what sydelta_last_error must name for each entry of the malformed list
MALFORMED_REASON = {
    "wrong-magic": "bad magic",
    "len-3": "truncated",
    "len-5": "truncated",
    "checksum-flag": "Content_Checksum",
    "dictionary-id-1": "Dictionary_ID",
    "reserved-fhd-bit": "reserved Frame_Header_Descriptor bit",
    "block-type-3": "block 0: reserved block type 3",
    "block-beyond-len": "block 0: truncated",
    "no-last-block": "block 2: truncated",
    "first-block-treeless": "block 0: Treeless literals or Repeat_Mode with no earlier table",
    "first-block-repeat-mode": "block 0: Treeless literals or Repeat_Mode with no earlier table",
    "ll0-offset-before-start": "block 0: offset reaches before the start of the output",
    "trailing-byte": "bytes behind the last block",
}


# ---- what a frame holds ----------------------------------------------------------------
def describe(frame: bytes) -> dict:
    """FHD, header size and per block: type, and for Compressed blocks the literals type,
    stream count, whether the Huffman weights are FSE-compressed or direct, the sequence
    count and the three modes.  Reads headers only."""
    assert frame[:4] == MAGIC
    fhd = frame[4]
    single, fid, did = fhd >> 5 & 1, fhd >> 6, fhd & 3
    pos = 5 + (0 if single else 1) + (4 if did == 3 else did) + (single if fid == 0 else 1 << fid)
    info = {"fhd": fhd, "header": pos, "blocks": []}
    while True:
        h = int.from_bytes(frame[pos:pos + 3], "little")
        pos += 3
        last, btype, size = h & 1, h >> 1 & 3, h >> 3
        b = {"type": btype, "size": size}
        if btype == 2:
            p = frame[pos:pos + size]
            lt, sf = p[0] & 3, p[0] >> 2 & 3
            if lt < 2:
                lh = (1, 2, 1, 3)[sf]
                regen = int.from_bytes(p[:lh], "little") >> (3 if lh == 1 else 4)
                csize, streams = (regen if lt == 0 else 1), 0
            else:
                lh = (3, 3, 4, 5)[sf]
                v = int.from_bytes(p[:lh], "little") >> 4
                bits = (10, 10, 14, 18)[sf]
                regen, csize, streams = v & ((1 << bits) - 1), v >> bits, 1 if sf == 0 else 4
                if lt == 2:
                    b["weights"] = "fse" if p[lh] < 128 else "direct"
            q = lh + csize
            n = p[q]
            q += 1
            if n == 255:
                n, q = int.from_bytes(p[q:q + 2], "little") + 0x7F00, q + 2
            elif n >= 128:
                n, q = (n - 128 << 8) + p[q], q + 1
            b.update(lit=lt, streams=streams, nseq=n, lit_regen=regen)
            if n:
                b["modes"] = (p[q] >> 6, p[q] >> 4 & 3, p[q] >> 2 & 3)
        info["blocks"].append(b)
        pos += 1 if btype == 1 else size
        if last:
            break
    assert pos == len(frame)
    return info
