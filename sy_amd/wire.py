"""Wire formats of the delta path: serde_json's compact text of
Vec<BlockChecksum> (sy-remote.rs:146-147, ssh.rs:967-973) and of Delta
(ssh.rs:1003, sy-remote.rs:175), written and parsed by libsydelta (sydelta_wire.cpp;
the Delta writer also on the device)."""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._lib import check, lib

_OP_DTYPE = np.dtype([("kind", "<u4"), ("reserved", "<u4"), ("a", "<u8"), ("b", "<u8")])
_SIG_DTYPE = np.dtype([("index", "<u8"), ("offset", "<u8"), ("size", "<u8"), ("weak", "<u4"),
                       ("reserved", "<u4"), ("strong", "<u8")])


def sig_array(index, offset, size, weak, strong) -> np.ndarray:
    a = np.zeros(len(index), dtype=_SIG_DTYPE)
    a["index"], a["offset"], a["size"], a["weak"], a["strong"] = index, offset, size, weak, strong
    return a


def checksums_to_json(sigs: np.ndarray) -> bytes:
    """sigs: structured array (sig_array)."""
    sigs = np.ascontiguousarray(sigs, dtype=_SIG_DTYPE)
    n = lib.sydelta_checksums_to_json(sigs.ctypes.data if len(sigs) else None, len(sigs), None, 0)
    buf = ctypes.create_string_buffer(n)
    lib.sydelta_checksums_to_json(sigs.ctypes.data if len(sigs) else None, len(sigs), buf, n)
    return buf.raw[:n]


def checksums_from_json(text: bytes) -> np.ndarray:
    out = ctypes.POINTER(_lib.BlockChecksumC)()
    n = ctypes.c_uint64()
    check(lib.sydelta_checksums_from_json(text, len(text), ctypes.byref(out), ctypes.byref(n)))
    try:
        if not n.value:
            return np.zeros(0, dtype=_SIG_DTYPE)
        raw = ctypes.string_at(out, n.value * _SIG_DTYPE.itemsize)
        return np.frombuffer(raw, dtype=_SIG_DTYPE).copy()
    finally:
        if n.value:
            lib.sydelta_checksums_free(out)


def _delta_handle(kind, a, b, source_size: int, block_size: int):
    n = len(kind)
    ops = np.zeros(n, dtype=_OP_DTYPE)
    if n:
        ops["kind"], ops["a"], ops["b"] = kind, a, b
    h = lib.sydelta_delta_from_ops(ops.ctypes.data if n else None, n, source_size, block_size)
    if not h:
        raise ValueError("bad op array")
    return h


def delta_to_json(kind, a, b, source_size: int, block_size: int, lit: bytes | np.ndarray) -> bytes:
    """Delta text from an op table whose Data ops index `lit` (host bytes)."""
    lit = np.ascontiguousarray(np.frombuffer(bytes(lit), dtype=np.uint8) if isinstance(lit, (bytes, bytearray))
                               else lit, dtype=np.uint8)
    h = _delta_handle(kind, a, b, source_size, block_size)
    try:
        n = ctypes.c_uint64()
        lp = lit.ctypes.data if lit.size else ctypes.c_void_p(1)  # non-NULL: use lit even when empty
        check(lib.sydelta_delta_to_json(h, lp, lit.size, None, 0, ctypes.byref(n)))
        buf = ctypes.create_string_buffer(n.value)
        check(lib.sydelta_delta_to_json(h, lp, lit.size, buf, n.value, ctypes.byref(n)))
        return buf.raw[:n.value]
    finally:
        lib.sydelta_delta_free(h)


def delta_to_json_device(kind, a, b, source_size: int, block_size: int, d_lit, stream=None):
    """The same text written on the device from literal bytes in HBM (torch uint8
    tensor); returns the text as a uint8 device tensor."""
    import torch

    from .device import _ptr, _stream

    h = _delta_handle(kind, a, b, source_size, block_size)
    try:
        n = ctypes.c_uint64()
        check(lib.sydelta_delta_to_json_device(h, _ptr(d_lit), d_lit.numel(), None, 0, ctypes.byref(n),
                                               _stream(stream)))
        out = torch.empty(n.value + 16, dtype=torch.uint8, device=d_lit.device)
        check(lib.sydelta_delta_to_json_device(h, _ptr(d_lit), d_lit.numel(), _ptr(out), out.numel(),
                                               ctypes.byref(n), _stream(stream)))
        return out[:n.value]
    finally:
        lib.sydelta_delta_free(h)


def delta_batch_to_json_device(deltas, lit, loffs, llens, out=None, stream=None):
    """The Delta texts of a whole batch written on the device in one call
    (sydelta_delta_batch_to_json_device): file f's text is delta_to_json's of deltas[f], its
    Data ops reading lit[loffs[f] + op.a, +op.b) (for a batched match's deltas: the sources'
    offsets and lengths).  `deltas` is a DeltaBatch or a list of DeviceDelta.  The texts are
    packed into `out` in file order, each starting on a multiple of 16; with out=None an arena
    of sydelta_delta_batch_to_json_bound bytes is allocated, so one call does.
    Returns (out trimmed to the packed size, toffs, tlens) with file f's text at
    out[toffs[f] : toffs[f] + tlens[f]].  Raises SyDeltaError (SYDELTA_E_INVAL) when a given
    `out` does not hold the texts: nothing was written."""
    import torch

    from .device import _OP_DTYPE as _DEV_OP_DTYPE
    from .device import DeltaBatch, _ptr, _stream

    arrs = [np.ascontiguousarray(x, dtype=np.uint64) for x in (loffs, llens)]
    own = []
    if isinstance(deltas, DeltaBatch):
        n = deltas.count
        ptrs = (ctypes.c_void_p * max(n, 1))()
        if int(lib.sydelta_delta_batch_ptrs(deltas.h, ptrs, n)) != n:
            raise ValueError("delta batch changed size")
    else:
        n = len(deltas)
        ptrs = (ctypes.c_void_p * max(n, 1))()
        for f, d in enumerate(deltas):
            if d.handle is not None:  # the library's own delta: no copy of the ops
                ptrs[f] = d.handle.h if isinstance(d.handle.h, int) else d.handle.h.value
                continue
            k = len(d.kind)
            ops = np.zeros(k, dtype=_DEV_OP_DTYPE)
            if k:
                ops["kind"], ops["a"], ops["b"] = d.kind, d.a, d.b
            h = lib.sydelta_delta_from_ops(ops.ctypes.data if k else None, k, d.source_size, d.block_size)
            if not h:
                for o in own:
                    lib.sydelta_delta_free(o)
                raise ValueError(f"file {f}: bad op array")
            own.append(h)
            ptrs[f] = h
    try:
        if any(len(a) != n for a in arrs):
            raise ValueError("offset / length tables and deltas differ in length")
        if out is None:
            bound = int(lib.sydelta_delta_batch_to_json_bound(ptrs, n))
            if bound == 0xFFFFFFFFFFFFFFFF:
                raise ValueError("no bound for the batch's text (a NULL delta or a size that overflows)")
            out = torch.empty(max(bound, 1), dtype=torch.uint8, device=lit.device)
        toffs = np.zeros(n, dtype=np.uint64)
        tlens = np.zeros(n, dtype=np.uint64)
        need = ctypes.c_uint64()
        check(lib.sydelta_delta_batch_to_json_device(
            lit.device.index or 0, ptrs, n, _ptr(lit) if lit.numel() else None, lit.numel(), arrs[0].ctypes.data,
            arrs[1].ctypes.data, _ptr(out), out.numel(), toffs.ctypes.data, tlens.ctypes.data, ctypes.byref(need),
            _stream(stream)))
        if need.value > out.numel():
            raise _lib.SyDeltaError(_lib.SYDELTA_E_INVAL, f"the batch's text needs {need.value} bytes, out holds {out.numel()}")
    finally:
        for o in own:
            lib.sydelta_delta_free(o)
    return out[:need.value], toffs, tlens


def checksums_to_json_device(d_weak, d_strong, block_size: int, last_size: int, stream=None):
    """serde_json::to_string(&Vec<BlockChecksum>) of a signature in HBM (the weak/strong
    tensors of device.signature), written on the device (sy-remote.rs:146-147); returns
    the text as a uint8 device tensor."""
    import torch

    from .device import _ptr, _stream

    nb = d_weak.numel()
    if d_strong.numel() != nb:
        raise ValueError("weak and strong arrays differ in length")
    n = ctypes.c_uint64()
    wp, sp = (_ptr(d_weak), _ptr(d_strong)) if nb else (None, None)
    check(lib.sydelta_checksums_to_json_device(wp, sp, nb, block_size, last_size, None, 0, ctypes.byref(n),
                                               _stream(stream)))
    out = torch.empty(n.value + 16, dtype=torch.uint8, device=d_weak.device)
    check(lib.sydelta_checksums_to_json_device(wp, sp, nb, block_size, last_size, _ptr(out), out.numel(),
                                               ctypes.byref(n), _stream(stream)))
    return out[:n.value]


def checksums_from_json_device(d_text, stream=None):
    """serde_json::from_str::<Vec<BlockChecksum>> of a compact text in HBM (uint8 device
    tensor) parsed on the device; returns the entries as a uint8 device tensor of
    n * 40 bytes (sydelta_block_checksum records) and n.  Raises SyDeltaError for text in
    any other spelling (parse that with checksums_from_json)."""
    import torch

    from .device import _ptr, _stream

    n = ctypes.c_uint64()
    check(lib.sydelta_checksums_from_json_device(_ptr(d_text), d_text.numel(), None, 0, ctypes.byref(n),
                                                 _stream(stream)))
    out = torch.empty(max(1, n.value) * _SIG_DTYPE.itemsize, dtype=torch.uint8, device=d_text.device)
    check(lib.sydelta_checksums_from_json_device(_ptr(d_text), d_text.numel(), _ptr(out), n.value, ctypes.byref(n),
                                                 _stream(stream)))
    return out[:n.value * _SIG_DTYPE.itemsize], n.value


def checksums_batch_to_json_device(weak, strong, nblocks, last_sizes, block_size: int, out=None, stream=None):
    """The signature texts of a whole batch written on the device in one call
    (sydelta_checksums_batch_to_json_device): weak / strong are the concatenated SoA in file
    order (device.signature_batch), file f's text is checksums_to_json_device's of its
    nblocks[f] entries with last_sizes[f] ("[]" for a file without blocks).  The texts are
    packed into `out` in file order, each starting on a multiple of 16; with out=None an arena
    of sydelta_checksums_batch_to_json_bound bytes is allocated, so one call does.
    Returns (out trimmed to the packed size, toffs, tlens).  Raises SyDeltaError
    (SYDELTA_E_INVAL) when a given `out` does not hold the texts: nothing was written."""
    import torch

    from .device import _ptr, _stream

    arrs = [np.ascontiguousarray(x, dtype=np.uint64) for x in (nblocks, last_sizes)]
    n = len(arrs[0])
    if len(arrs[1]) != n:
        raise ValueError("nblocks and last_sizes differ in length")
    if strong.numel() != weak.numel():
        raise ValueError("weak and strong arrays differ in length")
    if n and weak.numel() < sum(int(x) for x in arrs[0]):
        raise ValueError("the SoA holds fewer entries than nblocks sums to")
    if out is None:
        bound = int(lib.sydelta_checksums_batch_to_json_bound(arrs[0].ctypes.data, arrs[1].ctypes.data, n, block_size))
        if bound == 0xFFFFFFFFFFFFFFFF:
            raise ValueError("no bound for the batch's text (a block size out of range or a size that overflows)")
        out = torch.empty(max(bound, 1), dtype=torch.uint8, device=weak.device)
    toffs = np.zeros(n, dtype=np.uint64)
    tlens = np.zeros(n, dtype=np.uint64)
    need = ctypes.c_uint64()
    have = weak.numel() > 0
    check(lib.sydelta_checksums_batch_to_json_device(
        weak.device.index or 0, _ptr(weak) if have else None, _ptr(strong) if have else None, arrs[0].ctypes.data,
        arrs[1].ctypes.data, n, block_size, _ptr(out), out.numel(), toffs.ctypes.data, tlens.ctypes.data,
        ctypes.byref(need), _stream(stream)))
    if need.value > out.numel():
        raise _lib.SyDeltaError(_lib.SYDELTA_E_INVAL, f"the batch's text needs {need.value} bytes, out holds {out.numel()}")
    return out[:need.value], toffs, tlens


def checksums_batch_from_json_device(text, toffs, tlens, block_size: int, refused_ok=False, stream=None):
    """The signature texts of a whole batch parsed on the device in one call
    (sydelta_checksums_batch_from_json_device): file f's text is text[toffs[f] : toffs[f] +
    tlens[f]] (a uint8 device tensor and tables of any alignment and order), parsed by
    checksums_from_json_device's grammar and held to the layout of a signature with
    `block_size`.  Returns (weak, strong, nblocks, last_sizes): the concatenated SoA in file
    order (int32 / int64 device tensors holding the u32 / u64 bit patterns, as
    device.signature_batch returns them) and its tables, which is what device.BatchIndex takes.
    The SoA is sized from the text (one entry per 50 bytes at the most), so one call does.

    A refused text raises SyDeltaError (SYDELTA_E_INVAL, "file F: checksum JSON: ...").  With
    refused_ok=True the call succeeds instead and returns (weak, strong, nblocks, last_sizes,
    status): status[f] is 0 for a parsed file, 1 + P for a spelling refusal at byte P and
    (1 << 63) | (1 + P) for an entry at byte P that is not in the layout; such a file keeps its
    place in the SoA (its slots unspecified) and its text is for checksums_from_json."""
    import torch

    from .device import _ptr, _stream

    arrs = [np.ascontiguousarray(x, dtype=np.uint64) for x in (toffs, tlens)]
    n = len(arrs[0])
    if len(arrs[1]) != n:
        raise ValueError("offset and length tables differ in length")
    # the shortest entry, [{"index":0,"offset":0,"size":1,"weak":0,"strong":0}, is 52 bytes; only
    # a refused text can count more '{' than that, and then the call is repeated with room
    cap = int((arrs[1] // np.uint64(50) + np.uint64(1)).sum()) if n else 0
    soffs = np.zeros(n, dtype=np.uint64)
    nblocks = np.zeros(n, dtype=np.uint64)
    lasts = np.zeros(n, dtype=np.uint64)
    status = np.zeros(n, dtype=np.uint64) if refused_ok else None
    need = ctypes.c_uint64()
    for _ in range(2):
        weak = torch.empty(max(1, cap), dtype=torch.int32, device=text.device)
        strong = torch.empty(max(1, cap), dtype=torch.int64, device=text.device)
        check(lib.sydelta_checksums_batch_from_json_device(
            text.device.index or 0, _ptr(text) if text.numel() else None, text.numel(), arrs[0].ctypes.data,
            arrs[1].ctypes.data, n, block_size, _ptr(weak), _ptr(strong), weak.numel(), soffs.ctypes.data,
            nblocks.ctypes.data, lasts.ctypes.data, status.ctypes.data if refused_ok else None, ctypes.byref(need),
            _stream(stream)))
        if need.value <= weak.numel():
            break
        cap = need.value
    res = (weak[:need.value], strong[:need.value], nblocks, lasts)
    return res + (status,) if refused_ok else res


def delta_from_json_device(d_text, stream=None):
    """serde_json::from_str::<Delta> of a compact Delta JSON text in HBM (uint8 device
    tensor) parsed on the device: returns (ops as [(kind, a, b)] with Data ops indexing the
    literal tensor, the literal bytes as a uint8 device tensor, source_size, block_size).
    Raises SyDeltaError for text in any other spelling (parse that with delta_from_json)."""
    import torch

    from .device import _ptr, _stream

    n = ctypes.c_uint64()
    check(lib.sydelta_delta_from_json_device(_ptr(d_text), d_text.numel(), None, 0, ctypes.byref(n), None,
                                             _stream(stream)))
    lit = torch.empty(max(1, n.value), dtype=torch.uint8, device=d_text.device)
    h = ctypes.c_void_p()
    check(lib.sydelta_delta_from_json_device(_ptr(d_text), d_text.numel(), _ptr(lit), lit.numel(), ctypes.byref(n),
                                             ctypes.byref(h), _stream(stream)))
    try:
        cnt = lib.sydelta_delta_num_ops(h)
        ops_p = lib.sydelta_delta_ops(h)
        ops = [(int(ops_p[i].kind), int(ops_p[i].a), int(ops_p[i].b)) for i in range(cnt)]
        return ops, lit[:n.value], int(lib.sydelta_delta_source_size(h)), int(lib.sydelta_delta_block_size(h))
    finally:
        lib.sydelta_delta_free(h)


def delta_batch_from_json_device(text, toffs, tlens, lit=None, refused_ok=False, stream=None):
    """The Delta texts of a whole batch parsed on the device in one call
    (sydelta_delta_batch_from_json_device): file f's text is text[toffs[f] : toffs[f] +
    tlens[f]] (a uint8 device tensor and tables of any alignment and order: what
    zstd_decompress_batch_device returns), its delta what delta_from_json_device gives for that
    text alone.  The literal bytes are packed into `lit` in file order, each file's at a
    multiple of 16; with lit=None the sizes are asked for first and an arena of that size is
    allocated, so the parse runs twice: a caller that knows a bound passes `lit` for a single
    call.  Returns (DeltaBatch, lit, loffs, llens): file f's Data ops index lit[loffs[f] :
    loffs[f] + llens[f]], which is what device.apply_batch takes.

    A text in any other spelling raises SyDeltaError (SYDELTA_E_INVAL, "file F: Delta JSON: not
    serde's compact form at byte P").  With refused_ok=True the call succeeds instead and
    returns (DeltaBatch, lit, loffs, llens, status): status[f] is 0 for a parsed file, else
    1 + P; such a file's delta has no ops, and its text is for delta_from_json."""
    import torch

    from .device import DeltaBatch, _ptr, _stream

    arrs = [np.ascontiguousarray(x, dtype=np.uint64) for x in (toffs, tlens)]
    n = len(arrs[0])
    if len(arrs[1]) != n:
        raise ValueError("offset and length tables differ in length")
    loffs = np.zeros(n, dtype=np.uint64)
    llens = np.zeros(n, dtype=np.uint64)
    status = np.zeros(n, dtype=np.uint64) if refused_ok else None
    need = ctypes.c_uint64()
    tp = _ptr(text) if text.numel() else None

    def call(o, h):
        check(lib.sydelta_delta_batch_from_json_device(
            text.device.index or 0, tp, text.numel(), arrs[0].ctypes.data, arrs[1].ctypes.data, n,
            _ptr(o) if o is not None and o.numel() else None, o.numel() if o is not None else 0, loffs.ctypes.data,
            llens.ctypes.data, status.ctypes.data if refused_ok else None, ctypes.byref(need),
            ctypes.byref(h) if h is not None else None, _stream(stream)))

    if lit is None:
        call(None, None)
        lit = torch.empty(max(1, need.value), dtype=torch.uint8, device=text.device)
    h = ctypes.c_void_p()
    call(lit, h)
    batch = DeltaBatch(h)
    if need.value > lit.numel():
        batch.close()
        raise _lib.SyDeltaError(_lib.SYDELTA_E_INVAL, f"the batch's literals need {need.value} bytes, lit holds {lit.numel()}")
    res = (batch, lit[:need.value], loffs, llens)
    return res + (status,) if refused_ok else res


def zstd_compress_device(d_text, stream=None, device: int | None = None):
    """zstd frame (Huffman literals, FSE-coded sequences) of the bytes of a uint8 device tensor, as a uint8
    device tensor: the compression ssh.rs:1009-1017 applies to the Delta JSON.  The
    tensor must start 16-byte aligned (torch allocations and views at offset 0 do)."""
    import torch

    from .device import _ptr, _stream

    if device is None:
        device = d_text.device.index or 0
    n = d_text.numel()
    out = torch.empty(int(lib.sydelta_zstd_bound(n)) + 16, dtype=torch.uint8, device=d_text.device)
    got = ctypes.c_uint64()
    check(lib.sydelta_zstd_compress_device(device, _ptr(d_text) if n else None, n, _ptr(out), out.numel(),
                                           ctypes.byref(got), _stream(stream)))
    return out[:got.value]


def zstd_compress_batch_device(text, toffs, tlens, out=None, stream=None):
    """The zstd frames of a whole batch of texts in one call (sydelta_zstd_compress_batch_device):
    file f's frame is zstd_compress_device's of text[toffs[f] : toffs[f] + tlens[f]].  `text`
    is a uint8 device tensor that starts 16-byte aligned and every toffs[f] is a multiple of 16:
    what delta_batch_to_json_device returns.  The frames are packed into `out` back to back in
    file order; with out=None an arena of sydelta_zstd_batch_bound bytes is allocated, so one
    call does.  Returns (out trimmed to the packed size, foffs, flens) with file f's frame at
    out[foffs[f] : foffs[f] + flens[f]].  Raises SyDeltaError (SYDELTA_E_INVAL) when a given
    `out` does not hold the frames."""
    import torch

    from .device import _ptr, _stream

    arrs = [np.ascontiguousarray(x, dtype=np.uint64) for x in (toffs, tlens)]
    n = len(arrs[0])
    if len(arrs[1]) != n:
        raise ValueError("offset and length tables differ in length")
    if out is None:
        bound = int(lib.sydelta_zstd_batch_bound(arrs[1].ctypes.data, n))
        if bound == 0xFFFFFFFFFFFFFFFF:
            raise ValueError("no bound for the batch's frames (the lengths overflow)")
        out = torch.empty(max(bound, 1), dtype=torch.uint8, device=text.device)
    foffs = np.zeros(n, dtype=np.uint64)
    flens = np.zeros(n, dtype=np.uint64)
    need = ctypes.c_uint64()
    check(lib.sydelta_zstd_compress_batch_device(
        text.device.index or 0, _ptr(text) if text.numel() else None, text.numel(), arrs[0].ctypes.data,
        arrs[1].ctypes.data, n, _ptr(out), out.numel(), foffs.ctypes.data, flens.ctypes.data, ctypes.byref(need),
        _stream(stream)))
    return out[:need.value], foffs, flens


def zstd_decompress_device(d_frame, stream=None, device: int | None = None, out=None):
    """The bytes of one zstd frame held in a uint8 device tensor, decoded on the device
    (sy-remote.rs:160-166: compress::decompress), as a uint8 device tensor: frames of any
    zstd writer (libzstd at any level, streaming or one-shot, and zstd_compress_device's).
    One size query, then the decode into a tensor of that size: the stages up to the size
    (scan, tables, entropy decode, stitch) run twice, so a caller that knows a bound passes
    `out` (a uint8 device tensor) for a single call, the result a view of it; the measured
    rates are of that form.  Raises SyDeltaError (SYDELTA_E_INVAL)
    for what the device decoder refuses (a checksummed frame, a dictionary, a second frame,
    corrupt content, an `out` too small): decode that on the host."""
    import torch

    from .device import _ptr, _stream

    if device is None:
        device = d_frame.device.index or 0
    n = ctypes.c_uint64()
    fp = _ptr(d_frame) if d_frame.numel() else None
    if out is None:
        check(lib.sydelta_zstd_decompress_device(device, fp, d_frame.numel(), None, 0, ctypes.byref(n),
                                                 _stream(stream)))
        out = torch.empty(max(1, n.value), dtype=torch.uint8, device=d_frame.device)
    cap = out.numel()
    check(lib.sydelta_zstd_decompress_device(device, fp, d_frame.numel(), _ptr(out), cap, ctypes.byref(n),
                                             _stream(stream)))
    if n.value > cap:
        raise _lib.SyDeltaError(_lib.SYDELTA_E_INVAL, f"zstd frame regenerates {n.value} bytes, out holds {cap}")
    return out[:n.value]


def zstd_decompress_batch_device(frames, foffs, flens, out=None, refused_ok=False, stream=None):
    """The texts of a whole batch of zstd frames in one call
    (sydelta_zstd_decompress_batch_device): file f's frame is frames[foffs[f] : foffs[f] +
    flens[f]] (a uint8 device tensor and tables of any alignment and order: what
    zstd_compress_batch_device returns, or any sender's payloads), its text what
    zstd_decompress_device returns for that frame alone.  The texts are packed into `out` in
    file order, each at a multiple of 16 (delta_batch_to_json_device's layout).  With out=None
    the sizes are asked for first and an arena of that size is allocated: the stages up to the
    stitch (counts, scan, tables, entropy decode, stitch, offsets) run twice, so a caller that
    knows a bound passes `out` for a single call.  Returns (text, toffs, tlens) with file f's
    text at text[toffs[f] : toffs[f] + tlens[f]]; nothing else of `out` is changed.

    A frame the device decoder refuses (see zstd_decompress_device) raises SyDeltaError
    (SYDELTA_E_INVAL, "file F: zstd frame: block B: <reason>") and nothing is written.  With
    refused_ok=True the call succeeds instead and returns (text, toffs, tlens, status):
    status[f] is 0 for a decoded file, else (block << 32) | code; such a file has tlens[f] = 0
    and takes no room, and its payload is for the host decoder.  A batch of 4 GiB or more of
    text is refused: split it."""
    import torch

    from .device import _ptr, _stream

    arrs = [np.ascontiguousarray(x, dtype=np.uint64) for x in (foffs, flens)]
    n = len(arrs[0])
    if len(arrs[1]) != n:
        raise ValueError("offset and length tables differ in length")
    toffs = np.zeros(n, dtype=np.uint64)
    tlens = np.zeros(n, dtype=np.uint64)
    status = np.zeros(n, dtype=np.uint64) if refused_ok else None
    need = ctypes.c_uint64()
    fp = _ptr(frames) if frames.numel() else None

    def call(o):
        check(lib.sydelta_zstd_decompress_batch_device(
            frames.device.index or 0, fp, frames.numel(), arrs[0].ctypes.data, arrs[1].ctypes.data, n,
            _ptr(o) if o is not None and o.numel() else None, o.numel() if o is not None else 0, toffs.ctypes.data,
            tlens.ctypes.data, status.ctypes.data if refused_ok else None, ctypes.byref(need), _stream(stream)))

    if out is None:
        call(None)
        out = torch.empty(max(1, need.value), dtype=torch.uint8, device=frames.device)
    call(out)
    if need.value > out.numel():
        raise _lib.SyDeltaError(_lib.SYDELTA_E_INVAL, f"the batch's text needs {need.value} bytes, out holds {out.numel()}")
    res = (out[:need.value], toffs, tlens)
    return res + (status,) if refused_ok else res


def delta_from_json(text: bytes):
    """-> (ops as [("C", offset, size) | ("D", literal bytes)], source_size, block_size)."""
    h = ctypes.c_void_p()
    check(lib.sydelta_delta_from_json(text, len(text), ctypes.byref(h)))
    try:
        nops = int(lib.sydelta_delta_num_ops(h))
        ops = []
        for i in range(nops):
            o = lib.sydelta_delta_ops(h)[i]
            if o.kind == _lib.OP_COPY:
                ops.append(("C", int(o.a), int(o.b)))
            else:
                p = lib.sydelta_delta_literal(h, i)
                ops.append(("D", ctypes.string_at(p, int(o.b)) if o.b else b""))
        return ops, int(lib.sydelta_delta_source_size(h)), int(lib.sydelta_delta_block_size(h))
    finally:
        lib.sydelta_delta_free(h)
