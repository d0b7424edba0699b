"""Frames for the zstd decoder's tests (tests/test_unzstd_host.py, tests/test_gpu_unzstd.py):
the system libzstd driven the way compress/mod.rs:70-75 drives it (streaming, no pledged
size), hand-assembled frames for the forms libzstd never emits, the fixed malformed list,
and a small frame reader that says which forms a frame holds, so that a test can assert
what its corpus covers.

The families assembled from RFC 8878 (FORMS, FORMS_REFUSED; form(), form_refused(), expect()),
for the forms no sender here writes, each checked against libzstd by the CPU suite:

* of17 ... of27: offset code k in RLE_Mode behind an RLE prefix of 2^(k+1) bytes, three
  sequences with the offsets 2^k - 3, 2^(k+1) - 4 and a mixed pattern; of27 regenerates 2^28 + 44
  bytes.  of{k}-short: one byte of prefix too few for the second offset (refused).  Offset codes
  28-31 are not reached: they need 512 MiB to 2 GiB of output and a libzstd decode of the same.
* ml-max, ll-max: ML code 52 and LL code 35 filling a block to exactly 128 KiB; ml-over: one byte
  more (refused here, accepted by libzstd 1.4.8); wide-seq: sequences of 24 + 12 + 12 extra bits
  (LL 31, OF 24, ML 48) behind 32 MiB.
* huf12-*, huf11-*: direct-representation trees of depth 12 and 11 (libzstd writes at most 11
  bits), 1 stream of 700 literals, 4 streams of 9001 and of 6, and 4 streams of 131072 literals
  with 18-bit sizes.
* deep1-B (B = 1, 2, 3, 64, 1024): B blocks of 128 KiB that all hang from byte 0 by offset 1;
  deep3: three interleaved chains; deep-block: 63 blocks each copying the block before it.
* empties, empties-seq: Raw and RLE blocks of size 0 before, between and behind others, and a
  match reaching back over them; many-blocks: 3000 tiny blocks of all three types.
* far_frame(): libzstd at level 19 finding a match 5 MiB back, whose FSE-compressed tables hold
  the codes the hand-made frames carry in RLE_Mode only (read_ncount, fse_tables)."""
import ctypes
import functools
import random

import numpy as np

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


# ---- frames assembled from RFC 8878 for the forms no sender writes ---------------------
# (value of the code with all extra bits zero, number of extra bits): RFC 8878 section 3.1.1.3.2.1.1
LL_CODE = [(v, 0) for v in range(16)] + [(16, 1), (18, 1), (20, 1), (22, 1), (24, 2), (28, 2), (32, 3), (40, 3), (48, 4),
                                         (64, 6), (128, 7), (256, 8), (512, 9), (1024, 10), (2048, 11), (4096, 12),
                                         (8192, 13), (16384, 14), (32768, 15), (65536, 16)]
ML_CODE = [(v + 3, 0) for v in range(32)] + [(35, 1), (37, 1), (39, 1), (41, 1), (43, 2), (47, 2), (51, 3), (59, 3),
                                             (67, 4), (83, 4), (99, 5), (131, 7), (259, 8), (515, 9), (1027, 10),
                                             (2051, 11), (4099, 12), (8195, 13), (16387, 14), (32771, 15), (65539, 16)]
BLOCK_MAX = 128 << 10


def hdr(window_log: int) -> bytes:
    """Magic, FHD 0, Window_Descriptor with exponent window_log - 10 and mantissa 0."""
    assert 10 <= window_log <= 41
    return MAGIC + bytes([0, (window_log - 10) << 3])


# What a frame regenerates is written down beside it as a list of operations, which expect()
# replays: ("raw", bytes), ("rle", byte, n) and ("match", offset, length).
def rle_prefix(nbytes: int, first: int = 0):
    """(blocks, ops): RLE blocks of 128 KiB (4 bytes each in the frame) and one shorter block for a
    remainder, none of them last; the byte changes from block to block."""
    parts, ops, i = [], [], first
    while nbytes:
        n, byte = min(nbytes, BLOCK_MAX), 0x30 + i % 10
        parts.append(block(1, bytes([byte]), False, size=n))
        ops.append(("rle", byte, n))
        nbytes -= n
        i += 1
    return b"".join(parts), ops


def _seq_count(n: int) -> bytes:
    assert 0 < n < 0x7F00 + 65536
    if n < 128:
        return bytes([n])
    if n < 0x7F00:
        return bytes([(n >> 8) + 128, n & 255])
    return b"\xff" + (n - 0x7F00).to_bytes(2, "little")


def seq_block(nlit: int, byte: int, lc: int, oc: int, mc: int, seqs, last: bool, raw_empty: bool = False) -> bytes:
    """A Compressed block: nlit RLE literals of `byte` in the shortest header form that holds nlit
    (raw_empty: Raw literals of 0 bytes instead), all three tables in RLE_Mode with the symbols
    lc, oc, mc, and seqs = [(ll_extra, of_extra, ml_extra)].  In RLE_Mode no state bits are
    read, so the bitstream holds, in reading order, the end mark and per sequence the extra
    bits of the offset, the match length and the literal length, each most significant bit
    first: one integer stored little-endian, the zero padding above the mark."""
    if raw_empty:
        assert nlit == 0
        lit = b"\x00"
    elif nlit < 32:
        lit = bytes([1 | nlit << 3, byte])
    elif nlit < 4096:
        lit = (1 | 1 << 2 | nlit << 4).to_bytes(2, "little") + bytes([byte])
    else:
        assert nlit < 1 << 20
        lit = (1 | 3 << 2 | nlit << 4).to_bytes(3, "little") + bytes([byte])
    v = 1
    for le, oe, me in seqs:
        for nbits, x in ((oc, oe), (ML_CODE[mc][1], me), (LL_CODE[lc][1], le)):
            assert 0 <= x < 1 << nbits
            v = v << nbits | x
    stream = v.to_bytes((v.bit_length() + 7) // 8, "little")
    return block(2, lit + _seq_count(len(seqs)) + b"\x54" + bytes([lc, oc, mc]) + stream, last)


def seq_ops(nlit: int, byte: int, lc: int, oc: int, mc: int, seqs):
    """What seq_block's block regenerates (every Offset_Value above 3: no repeat codes)."""
    ops, used = [], 0
    for le, oe, me in seqs:
        ll, ml, value = LL_CODE[lc][0] + le, ML_CODE[mc][0] + me, (1 << oc) + oe
        assert value > 3
        if ll:
            ops.append(("rle", byte, ll))
        ops.append(("match", value - 3, ml))
        used += ll
    assert used <= nlit
    if nlit > used:
        ops.append(("rle", byte, nlit - used))
    return ops


def huf_codes(weights):
    """symbol -> (code, bits) of a complete weight list (the implied last weight included): RFC 8878
    section 4.2.1.3: symbols sorted by (weight, symbol) from code 0, the code incremented within a
    length and shifted right by the difference when the length drops."""
    total = sum(1 << w - 1 for w in weights if w)
    depth = total.bit_length() - 1
    assert total == 1 << depth
    codes, code, prev = {}, 0, None
    for w, s in sorted((w, s) for s, w in enumerate(weights) if w):
        bits = depth + 1 - w
        if prev is not None:
            code >>= prev - bits
        codes[s] = (code, bits)
        code, prev = code + 1, bits
    assert code == 1 << prev  # the code space is used up
    return codes, depth


def huf_block(weights, lits: bytes, streams: int, last: bool = True) -> bytes:
    """A Compressed block of Huffman literals and no sequences: a direct-representation tree
    (header byte 127 + the number of listed weights, the weights in 4 bits each, the first in
    the high nibble, the last weight implied), 1 or 4 streams (each the end mark and the codes
    in order as one little-endian integer, behind a 6-byte jump table for 4), the smallest
    size format that holds the sizes."""
    codes, _ = huf_codes(weights)
    listed = list(weights[:-1])
    assert 127 + len(listed) <= 255 and max(listed) < 16
    # the last weight must be what the listed ones imply
    rest = (1 << sum(1 << w - 1 for w in listed if w).bit_length()) - sum(1 << w - 1 for w in listed if w)
    assert rest == 1 << weights[-1] - 1
    nib = listed + [0] * (len(listed) & 1)
    tree = bytes([127 + len(listed)]) + bytes(nib[i] << 4 | nib[i + 1] for i in range(0, len(nib), 2))

    def stream(part):
        v = 1
        for s in part:
            code, bits = codes[s]
            v = v << bits | code
        return v.to_bytes((v.bit_length() + 7) // 8, "little")

    n = len(lits)
    if streams == 1:
        payload = tree + stream(lits)
        forms = (0,)
    else:
        assert streams == 4 and n >= 6
        seg = (n + 3) // 4
        parts = [stream(lits[j * seg:(j + 1) * seg]) for j in range(3)] + [stream(lits[3 * seg:])]
        assert all(len(p) < 65536 for p in parts[:3])
        payload = tree + b"".join(len(p).to_bytes(2, "little") for p in parts[:3]) + b"".join(parts)
        forms = (1, 2, 3)
    for sf in forms:
        bits = (10, 10, 14, 18)[sf]
        if n < 1 << bits and len(payload) < 1 << bits:
            break
    else:
        raise AssertionError("the literals do not fit a size format")
    head = (2 | sf << 2 | n << 4 | len(payload) << (4 + bits)).to_bytes((3, 3, 4, 5)[sf], "little")
    content = head + payload + b"\x00"
    assert len(content) < BLOCK_MAX
    return block(2, content, last)


def expect(ops) -> np.ndarray:
    """The bytes a list of operations regenerates (uint8).  Shares nothing with the decoder."""
    total = sum(len(op[1]) if op[0] == "raw" else op[2] for op in ops)
    out = np.empty(total, dtype=np.uint8)
    pos = 0
    for op in ops:
        if op[0] == "raw":
            out[pos:pos + len(op[1])] = np.frombuffer(op[1], dtype=np.uint8)
            pos += len(op[1])
        elif op[0] == "rle":
            out[pos:pos + op[2]] = op[1]
            pos += op[2]
        else:
            _, off, ml = op
            assert 0 < off <= pos, (off, pos)
            done = 0  # an overlapping match repeats the `off` bytes before it: whole periods, doubling
            while done < ml:
                n = min(off + done, ml - done)
                out[pos + done:pos + done + n] = out[pos - off:pos - off + n]
                done += n
            pos += ml
    assert pos == total
    return out


OF_CODES = tuple(range(17, 28))  # 28-31 need 512 MiB to 2 GiB of output
DEEP1 = (1, 2, 3, 64, 1024)
W12 = [1, 1] + list(range(2, 13))  # depth 12: symbols 0 and 1 have 12-bit codes, symbol 12 one bit
W11 = [1, 1] + list(range(2, 12))  # depth 11
ML_MAX = (1, 0x41, 1, 2, 52, [(0, 0, 65532)])   # 1 literal, then offset 1 for 131071 bytes
BARE = (0, 0, 0, 2, 52, [(0, 0, 65533)])        # nothing but a match of 131072 bytes at offset 1


def _of_frame(k: int, prefix: int):
    seqs = [(0, 0, 0), (0, (1 << k) - 1, 0), (0, 0x5555555 & ((1 << k) - 1), 0)]
    args = (20, 0x61, 4, k, 5, seqs)
    blocks, ops = rle_prefix(prefix)
    return hdr(k + 2) + blocks + seq_block(*args, True), ops + seq_ops(*args)


def _bare(oc: int, oe: int, last: bool):
    args = (0, 0, 0, oc, 52, [(0, oe, 65533)])
    return seq_block(*args, last, raw_empty=True), seq_ops(*args)


def _chain(head: bytes, ops, n: int, oc: int, oe: int, window_log: int = 17):
    """`head` (blocks, not last) and n bare matches of 128 KiB behind it."""
    parts = [_bare(oc, oe, i == n - 1) for i in range(n)]
    return hdr(window_log) + head + b"".join(p for p, _ in parts), ops + [o for _, oo in parts for o in oo]


def _huf_lits(weights, n: int, seed: int) -> bytes:
    """Every symbol once, from both ends inwards (the longest and the shortest codes also where only
    six literals fit), then symbols drawn as their code lengths want them."""
    rng = random.Random(seed)
    ns = len(weights)
    first = [s // 2 if s % 2 == 0 else ns - 1 - s // 2 for s in range(ns)][:n]
    return bytes(first + rng.choices(range(len(weights)), weights=[1 << w for w in weights], k=n - len(first)))


def _huf_frame(weights, n: int, streams: int, seed: int):
    lits = _huf_lits(weights, n, seed)
    return HEADER + huf_block(weights, lits, streams), [("raw", lits)]


def _empties(last: bool):
    parts = [(0, b"", None), (1, b"z", 0), (0, b"ab", None), (0, b"", None), (1, b"y", 0), (1, b"c", 3), (0, b"", None),
             (0, b"de", None), (1, b"x", 0)]
    blocks = b"".join(block(t, c, last and i == len(parts) - 1, size=s) for i, (t, c, s) in enumerate(parts))
    return blocks, [("raw", b"ab"), ("rle", 0x63, 3), ("raw", b"de")]


def _many_blocks(n: int = 3000):
    rng = random.Random(3000)
    parts, ops = [], []
    for i in range(n):
        last, j = i == n - 1, i // 3
        if i % 3 == 0:
            raw = rng.randbytes(1 + j % 5)
            parts.append(block(0, raw, last))
            ops.append(("raw", raw))
        elif i % 3 == 1:
            byte = 0x30 + j % 10
            parts.append(block(1, bytes([byte]), last, size=j % 4))
            if j % 4:
                ops.append(("rle", byte, j % 4))
        else:  # one literal and a match of 3 to 10 bytes that may reach over the blocks before it
            args = (1, 0x41 + j % 26, 1, 2 + j % 2, j % 8, [(0, j % 3, 0)])
            parts.append(seq_block(*args, last))
            ops += seq_ops(*args)
    return HEADER + b"".join(parts), ops


def _wide_seq(oc: int):
    """Two sequences of oc + 12 + 12 extra bits behind a prefix of 2^(oc + 1) bytes."""
    full = (1 << oc) - 1
    seqs = [(4095, full, 4095), (0xA5A, 0x5A5A5A & full, 0x5A5)]
    args = (8191 + 4096 + 0xA5A + 7, 0x62, 31, oc, 48, seqs)
    blocks, ops = rle_prefix(1 << oc + 1)
    return hdr(oc + 2) + blocks + seq_block(*args, True), ops + seq_ops(*args)


def _forms():
    f = {}
    for k in OF_CODES:
        f[f"of{k}"] = functools.partial(_of_frame, k, 1 << k + 1)
    f["ml-max"] = lambda: (HEADER + seq_block(*ML_MAX, True), seq_ops(*ML_MAX))
    ll_max = (131069, 0x63, 35, 2, 0, [(65533, 0, 0)])
    f["ll-max"] = lambda: (HEADER + seq_block(*ll_max, True), seq_ops(*ll_max))
    f["wide-seq"] = functools.partial(_wide_seq, 24)
    for depth, w in ((12, W12), (11, W11)):
        f[f"huf{depth}-1x700"] = functools.partial(_huf_frame, w, 700, 1, depth)
        f[f"huf{depth}-4x9001"] = functools.partial(_huf_frame, w, 9001, 4, depth + 100)
        f[f"huf{depth}-4x6"] = functools.partial(_huf_frame, w, 6, 4, depth + 200)
    f["huf12-4x131072"] = functools.partial(_huf_frame, W12, 131072, 4, 312)
    for b in DEEP1:
        f[f"deep1-{b}"] = functools.partial(_chain, seq_block(*ML_MAX, b == 1), seq_ops(*ML_MAX), b - 1, 2, 0)
    f["deep3"] = lambda: _chain(block(0, b"xyz", False), [("raw", b"xyz")], 2, 2, 2)
    noise = random.Random(5).randbytes(BLOCK_MAX)
    f["deep-block"] = lambda: _chain(block(0, noise, False), [("raw", noise)], 63, 17, 3, 18)
    f["empties"] = lambda: (HEADER + _empties(True)[0], _empties(True)[1])
    over = (2, 0x66, 2, 3, 7, [(0, 4, 0)])  # 2 literals, then 10 bytes from offset 9: the frame's first byte
    f["empties-seq"] = lambda: (HEADER + _empties(False)[0] + seq_block(*over, False) + block(0, b"", True),
                                _empties(False)[1] + seq_ops(*over))
    f["many-blocks"] = _many_blocks
    return f


FORMS = _forms()
# refused: name -> the reason sydelta_last_error must name, with the block's index
FORMS_REFUSED = {f"of{k}-short": f"block {1 << k - 16}: offset reaches before the start of the output" for k in OF_CODES}
FORMS_REFUSED["ml-over"] = "block 0: block regenerates more than 128 KiB"
HUF_FORMS = tuple(n for n in FORMS if n.startswith("huf"))


def form(name: str):
    """(frame, ops) of a valid family member; expect(ops) is what it regenerates.  Built anew at
    every call: the large ones are not kept."""
    return FORMS[name]()


def form_refused(name: str) -> bytes:
    """A frame of FORMS_REFUSED.  of{k}-short: of{k} with a prefix of 2^(k+1) - 21 bytes, so that
    the second sequence's offset 2^(k+1) - 4 reaches one byte before the output's start."""
    if name == "ml-over":
        return HEADER + seq_block(1, 0x41, 1, 2, 52, [(0, 0, 65533)], True)
    k = int(name[2:4])
    assert name == f"of{k}-short"
    return _of_frame(k, (1 << k + 1) - 21)[0]


@functools.lru_cache(None)
def far_input() -> bytes:
    """300 KB of random bytes, about 5 MiB of Delta JSON and the same 300 KB again: streamed at
    level 19 (an 8 MiB window) the second copy is found 5 MiB back."""
    # random bytes in which no three bytes come twice: level 19 takes 3-byte matches, which cut
    # plain random bytes into literal runs of a few thousand at most
    rng, seen, noise = random.Random(21), set(), bytearray(b"\x00\x00")
    while len(noise) < 300000:
        b = rng.randrange(256)
        if (noise[-2], noise[-1], b) not in seen:
            seen.add((noise[-2], noise[-1], b))
            noise.append(b)
    noise = bytes(noise)
    rng = random.Random(22)
    filler = b"".join(delta_json(rng, 4000, 0.3) for _ in range(7))
    assert 4 << 20 < len(filler) < 7 << 20, len(filler)
    return noise + filler + noise


@functools.lru_cache(None)
def far_frame():
    """(frame, data): far_input() streamed by libzstd at level 19."""
    data = far_input()
    return stream_compress(data, 19), data


# ---- the FSE table descriptions of a frame, read as RFC 8878 section 4.1.1 says ----------
def read_ncount(p: bytes):
    """(accuracy log, probabilities, bytes used) of an FSE table description; a probability of -1
    is "less than one"."""
    bits, pos = int.from_bytes(p, "little"), 0

    def peek(n):
        return bits >> pos & ((1 << n) - 1)

    log = peek(4) + 5
    pos = 4
    remaining, probs = 1 << log, []
    while remaining > 0:
        # a value in [0, remaining + 1]: the first `low` values take one bit less
        nb = (remaining + 1).bit_length()
        low = (1 << nb) - 1 - (remaining + 1)
        v = peek(nb - 1)
        if v < low:
            pos += nb - 1
        else:
            v = peek(nb)
            pos += nb
            if v >= 1 << nb - 1:
                v -= low
        prob = v - 1
        probs.append(prob)
        remaining -= abs(prob)
        if prob == 0:  # repeat flags: two bits of further zeros, again after a 3
            while True:
                r = peek(2)
                pos += 2
                probs += [0] * r
                if r < 3:
                    break
    assert remaining == 0 and pos <= 8 * len(p)
    return log, probs, (pos + 7) // 8


def fse_tables(frame: bytes):
    """Per Compressed block with sequences: {0 (LL) | 1 (OF) | 2 (ML): (accuracy log,
    probabilities)} for the tables the block defines in FSE_Compressed_Mode."""
    info, out = describe(frame), []
    pos = info["header"]
    for b in info["blocks"]:
        pos += 3
        if b["type"] == 2 and b["nseq"]:
            p = frame[pos:pos + b["size"]]
            lh = (1, 2, 1, 3)[p[0] >> 2 & 3] if b["lit"] < 2 else (3, 3, 4, 5)[p[0] >> 2 & 3]
            if b["lit"] == 0:
                csize = b["lit_regen"]
            elif b["lit"] == 1:
                csize = 1
            else:
                bits = (10, 10, 14, 18)[p[0] >> 2 & 3]
                csize = int.from_bytes(p[:lh], "little") >> (4 + bits)
            q = lh + csize
            q += 1 if p[q] < 128 else 2 if p[q] < 255 else 3
            q += 1  # the modes byte
            tabs = {}
            for j, mode in enumerate(b["modes"]):
                if mode == 1:
                    q += 1
                elif mode == 2:
                    log, probs, used = read_ncount(p[q:])
                    tabs[j] = (log, probs)
                    q += used
            out.append(tabs)
        pos += 1 if b["type"] == 1 else b["size"]
    return out
