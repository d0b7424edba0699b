"""The device-only parts of the Delta JSON parse (K7d: k_dparse_count / _place / k_dparse,
sy_amd/csrc/sydelta_kernels.hip) against an independent reference (delta_json_ref.py:
json.loads + a re-serialisation check for what is accepted, the grammar restated for the
position a refusal names): the LDS staging of a wave's text (dword and byte copy, the
136-byte halo), the SWAR fast path that replaces the chunk bodies inside a literal run,
and the literal slab with its phased dword stores.

Geometry: one thread per 64 text bytes, chunk c = [8 + 64c, 8 + 64(c + 1)); a wave covers
4096 bytes, a workgroup 16384 (texts: delta_json_cases.py).

Every text runs in the three call shapes -- the length query (d_lit NULL, out NULL),
validate-only with out, and the full parse into a literal buffer of exactly lit_len bytes
with 0xEE guards around it -- which must agree: accepted exactly when parse_ref accepts,
with its ops and literals (and the host parser's); refused with SYDELTA_E_INVAL at
first_bad.  No text is skipped: a change that leaves a text compact is an accept case.

Marked firstrun with its sibling test_gpu_dparse.py."""
import ctypes

import numpy as np
import pytest

import delta_json_cases as cases
from delta_json_ref import first_bad_re, parse_ref
from sy_amd import wire

pytestmark = [pytest.mark.gpu, pytest.mark.late, pytest.mark.firstrun]

TEXT_OFFSETS = (0, 1, 2, 3, 5, 4, 8, 12)  # 1, 2, 3, 5: the byte copy of the staging; 0, 4, 8, 12: the dword copy
LIT_OFFSETS = (0, 1, 2, 3)                # every phase of the literal store
PAD = 16


class Text:
    """A text in device memory at a chosen offset from a 16-byte boundary, digits around it."""

    def __init__(self, text: bytes, off: int):
        import torch

        self.n, self.off = len(text), off
        self.buf = torch.full((PAD + off + len(text) + PAD,), 0x31, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.view = self.buf[PAD + off:PAD + off + len(text)]
        self.view.copy_(torch.frombuffer(bytearray(text), dtype=torch.uint8))
        self.ptr = self.buf.data_ptr() + PAD + off

    def patch(self, idx: np.ndarray, vals: np.ndarray):
        import torch

        self.view[torch.from_numpy(idx).cuda()] = torch.from_numpy(vals).cuda()


def _call(t: Text, lit_ptr, cap, want_out: bool):
    """One call: (rc, position named or None, lit_len, ops or None, source_size, block_size)."""
    from sy_amd._lib import lib

    n, h = ctypes.c_uint64(), ctypes.c_void_p()
    rc = lib.sydelta_delta_from_json_device(t.ptr, t.n, lit_ptr, cap, ctypes.byref(n), ctypes.byref(h) if want_out else None,
                                            None)
    if rc != 0:
        assert not h
        msg = lib.sydelta_last_error().decode()
        assert "not serde's compact form at byte " in msg, msg
        return rc, int(msg.rsplit(" ", 1)[1]), n.value, None, None, None
    if not want_out:
        return 0, None, n.value, None, None, None
    try:
        cnt = lib.sydelta_delta_num_ops(h)
        p = lib.sydelta_delta_ops(h)
        ops = [(int(p[i].kind), int(p[i].a), int(p[i].b)) for i in range(cnt)]
        return 0, None, n.value, ops, int(lib.sydelta_delta_source_size(h)), int(lib.sydelta_delta_block_size(h))
    finally:
        lib.sydelta_delta_free(h)


def check_text(t: Text, text: bytes, lit_off: int, host_parse: bool = True):
    """The three call shapes on `text` (already in t) against the reference; True: accepted."""
    import torch

    from sy_amd._lib import SYDELTA_E_INVAL

    ref, bad = parse_ref(text), first_bad_re(text)
    assert (ref is None) == (bad is not None)
    q = _call(t, None, 0, False)
    v = _call(t, None, 0, True)
    nlit = q[2]
    guard = torch.full((PAD + lit_off + nlit + PAD,), 0xEE, dtype=torch.uint8, device="cuda")
    lo = PAD + lit_off
    f = _call(t, guard.data_ptr() + lo, nlit, True)  # lit_cap == lit_len exactly
    g = guard.cpu().numpy()
    assert (g[:lo] == 0xEE).all() and (g[lo + nlit:] == 0xEE).all(), "bytes around the literal buffer written"
    if ref is None:
        for name, r in (("query", q), ("validate", v), ("full", f)):
            assert (r[0], r[1]) == (SYDELTA_E_INVAL, bad), (name, r[:3], bad)
        return False
    for name, r in (("query", q), ("validate", v), ("full", f)):
        assert r[0] == 0 and r[2] == nlit, (name, r[:3], "the reference accepts")
    assert v[3:] == f[3:]
    lit = g[lo:lo + nlit].tobytes()
    got = [("C", a, b) if k == 0 else ("D", lit[a:a + b]) for k, a, b in f[3]]
    assert (got, f[4], f[5]) == ref
    assert nlit == sum(len(o[1]) for o in ref[0] if o[0] == "D")
    if host_parse:
        assert wire.delta_from_json(text) == ref
    return True


def test_region_ends_near_wave_and_workgroup_boundaries(gpu):
    """E - 8 = 4096k + d around the fast path's `lo + 72 > e` cut and the partial last wave
    (k = 1, 5) and workgroup (k = 4)."""
    for name, ops, text in cases.end_cases():
        assert check_text(Text(text, 0), text, 0), name


@pytest.mark.parametrize("edge", [cases.WAVE, cases.GROUP])
def test_longest_token_across_a_boundary(edge, gpu):
    """The 68-byte Copy op (70 with its follower) starting -70..+1 bytes from a wave's / a
    workgroup's end: read through the 136-byte halo of the wave that owns its '{'."""
    n = 0
    for name, ops, text in cases.boundary_cases():
        if name.startswith(f"token-{edge}"):
            assert check_text(Text(text, 0), text, 0), name
            n += 1
    assert n == 72


def test_literal_density_extremes(gpu):
    """All 0..9 (a wave's literal range is exactly the slab: the `<=` of `staged`), all
    >= 100, a mix of the digit-count edges, and a copy-heavy text whose waves own 0-3
    literals (the byte-by-byte store) or no op start (k_dparse_place's early return)."""
    for name, ops, text in cases.density_cases():
        assert check_text(Text(text, 0), text, 0), name


@pytest.mark.parametrize("name", ["mixed", "copy-heavy"])
def test_text_and_literal_alignment(name, gpu):
    """The text at offsets 1, 2, 3, 5 (byte copy) and 4, 8, 12 (dword copy), the literal
    buffer at phases 0..3 with lit_cap == lit_len and guard bytes around it."""
    text = dict((n, t) for n, _, t in cases.density_cases())[name]
    for toff in TEXT_OFFSETS[1:]:
        t = Text(text, toff)
        for loff in LIT_OFFSETS:
            assert check_text(t, text, loff, host_parse=False), (toff, loff)


def _changed(base: bytes, texts, k0: int = 0):
    """Each changed text patched into the base on the device, at a text offset and a literal
    phase that rotate with the text's number, checked, and the base restored."""
    base_np = np.frombuffer(base, np.uint8)
    held = {off: Text(base, off) for off in TEXT_OFFSETS}
    accepted = refused = 0
    for k, text in enumerate(texts, k0):
        t = held[TEXT_OFFSETS[k % len(TEXT_OFFSETS)]]
        cur = np.frombuffer(text, np.uint8)
        idx = np.nonzero(cur != base_np)[0]
        t.patch(idx, cur[idx])
        if check_text(t, text, LIT_OFFSETS[(k // len(TEXT_OFFSETS)) % 4]):
            accepted += 1
        else:
            refused += 1
        t.patch(idx, base_np[idx])
    return accepted, refused


_BASE = cases.refuse_base()


@pytest.mark.parametrize("where", list(cases.target_chunks(_BASE[1], _BASE[2], _BASE[3])))
def test_one_byte_changed_inside_a_fast_chunk(where, gpu):
    """A value made 256..999, a leading zero, ',' -> a digit, a digit -> ',', and a byte of
    no literal run, at in-chunk indices 0, 1, 2, 3, 31, 60..63 and in the 8 look-ahead
    bytes, of a chunk the fast path owns (a ~70 KiB text: Copy, 22000 literals, Copy)."""
    _, base, r0, r1 = _BASE
    chunk = cases.target_chunks(base, r0, r1)[where]
    texts = [t for _, _, t in cases.deterministic_changes(base, chunk)]
    assert 250 < len(texts) < 500  # x 3 call shapes: under 1500 parses
    accepted, refused = _changed(base, texts)
    assert refused > 200 and accepted + refused == len(texts)


def test_random_bytes_changed_anywhere(gpu):
    """1-3 bytes changed anywhere in [8, E), 300 texts."""
    _, base, _, _ = _BASE
    accepted, refused = _changed(base, cases.random_changes(base, 300, 99))
    assert accepted + refused == 300 and refused > 200
