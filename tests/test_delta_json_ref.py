"""The reference the K7d / K7 GPU tests are held to (tests/delta_json_ref.py), checked on
the CPU before any GPU is involved:

* parse_ref against the host parser (wire.delta_from_json, a full serde_json parser): what
  parse_ref accepts, the host parser reads as the same delta; what the host parser
  refuses, parse_ref refuses; and the spellings the device parser must refuse (compact
  form only) are refused by parse_ref although the host parser reads some of them.
* first_bad names a position exactly when parse_ref refuses, on a few thousand seeded
  mutations of small texts and on the long texts of the GPU tests; first_bad_re (the
  same rule as a regular expression, for the long texts) names the same position.
* The deterministic list of changed texts of the GPU tests (delta_json_cases.py) really
  holds refusals of every kind it claims, in every chunk it aims at, and the texts with
  exact geometry have it.
"""
import random

import pytest

import delta_json_cases as cases
from delta_json_ref import compact, first_bad, first_bad_re, parse_ref
from sy_amd import wire
from sy_amd._lib import SyDeltaError


def _host(text):
    try:
        return wire.delta_from_json(text)
    except SyDeltaError:
        return None


def test_parse_ref_agrees_with_host_parser_on_accepted_texts():
    for ops, ss, bs in cases.small_accepted():
        text = compact(ops, ss, bs)
        assert parse_ref(text) == (ops, ss, bs) == _host(text)
        assert first_bad(text) is None and first_bad_re(text) is None


def test_parse_ref_refuses_what_the_device_must_refuse():
    n_host_reads = 0
    for text in cases.small_refused():
        assert parse_ref(text) is None, text
        assert first_bad(text) is not None, text
        assert first_bad_re(text) == first_bad(text), text
        n_host_reads += _host(text) is not None
    assert n_host_reads >= 3  # whitespace, another key order, an unknown key: serde reads them


@pytest.mark.parametrize("bad", [
    '{"ops":[],"ops":[],"source_size":0,"block_size":4}',
    '{"ops":[],"source_size":0,"source_size":1,"block_size":4}',
    '{"ops":[{"Copy":{"offset":0,"size":1,"size":2}}],"source_size":1,"block_size":4}',
    '{"ops":[{"Data":[256]}],"source_size":1,"block_size":4}',
    '{"ops":[{"Data":[01]}],"source_size":1,"block_size":4}',
    '{"ops":[{"Copy":{"offset":00,"size":1}}],"source_size":1,"block_size":4}',
    '{"ops":[],"source_size":01,"block_size":4}',
    '{"ops":[{"Data":[true]}],"source_size":1,"block_size":4}',
    '{"ops":[{"Data":[1.0]}],"source_size":1,"block_size":4}',
    '{"ops":[{"Data":[1e0]}],"source_size":1,"block_size":4}',
    '{"ops":[{"Copy":{"offset":18446744073709551616,"size":1}}],"source_size":1,"block_size":4}',
    '{"ops":[],"source_size":18446744073709551616,"block_size":4}',
    '{"ops":[{"Data":[-0]}],"source_size":1,"block_size":4}',
])
def test_parse_ref_refuses_malformed(bad):
    assert parse_ref(bad.encode()) is None
    assert first_bad(bad.encode()) is not None
    assert _host(bad.encode()) is None


def test_first_bad_exactly_when_parse_ref_refuses_on_mutations():
    """Seeded mutations (1-3 bytes replaced, inserted or deleted) of small texts with every
    kind of op, of the shortest text and of a text with the longest token."""
    rng = random.Random(77)
    bases = [compact(*c) for c in cases.small_accepted()]
    bases += [compact([("C", 4096, 4096), ("D", b"\x01\xff"), ("D", b"")], 8192, 4096),
              compact([("D", bytes([0, 9, 10, 99, 100, 199, 200, 255])), cases.LONGEST_COPY, ("D", b"\x07")], 2**64 - 1, 2**64 - 1)]
    bases = [b for b in bases if len(b) < 400]
    alphabet = b'0123456789,,{}[]:"aDC -.e' + bytes([0, 0x80, 0xFF])
    n = accepted = 0
    for base in bases:
        for _ in range(600):
            b = bytearray(base)
            for _ in range(rng.randint(1, 3)):
                how, at = rng.randrange(3), rng.randrange(len(b))
                if how == 0:
                    b[at] = rng.choice(alphabet)
                elif how == 1:
                    b.insert(at, rng.choice(alphabet))
                elif len(b) > 1:
                    del b[at]
            t = bytes(b)
            ref, bad = parse_ref(t), first_bad(t)
            assert (bad is None) == (ref is not None), (t, bad, ref)
            assert first_bad_re(t) == bad, t
            if ref is not None:
                assert _host(t) == ref, t
                accepted += 1
            n += 1
    assert n >= 3000 and 20 <= accepted <= n // 2


def test_texts_with_exact_geometry():
    """The accepted texts of the GPU tests: in form, and the runs have the lengths asked for."""
    rng = random.Random(1)
    for L in list(range(1, 40)) + [4096, 4097, 16384 - 11]:
        vals = cases.run_with_text_len(L, rng)
        assert len(",".join(map(str, vals))) == L
    n = 0
    for gen in (cases.end_cases, cases.boundary_cases, cases.density_cases):
        for name, ops, text in gen():
            assert parse_ref(text) == (ops, parse_ref(text)[1], 4096), name
            assert first_bad_re(text) is None, name
            assert len(text) < 100 << 10
            n += 1
    assert n == 36 + 144 + 4
    # dense: every chunk inside the run starts 32 literals, a wave's range is the whole slab
    dense = compact(cases.dense_ops(), 3, 4096)
    assert dense[8 + 4096:8 + 8192].count(b",") == 2048


def test_changed_texts_hold_refusals_of_every_kind():
    """The deterministic list: per chunk aimed at, at least one text of every kind is
    refused (by parse_ref), some are accepted (they stay in the list as accept cases), and
    first_bad / first_bad_re agree with parse_ref on each."""
    ops, base, r0, r1 = cases.refuse_base()
    assert parse_ref(base) == (ops, 5, 4096) and len(ops[1][1]) >= 20000 and 65 << 10 < len(base) < 100 << 10
    assert len(base) > 4 * cases.GROUP
    total = accepted = 0
    for name, chunk in cases.target_chunks(base, r0, r1).items():
        refused = dict.fromkeys(cases.KINDS, 0)
        lo = 8 + 64 * chunk
        assert r0 < lo and lo + 72 <= r1, name  # the chunk and its look-ahead: digits and commas only
        for k, (i, kind, t) in enumerate(cases.deterministic_changes(base, chunk)):
            assert len(t) == len(base) and t != base
            ref, bad = parse_ref(t), first_bad_re(t)
            assert (bad is None) == (ref is not None), (name, i, kind)
            if k % 16 == 0:
                assert first_bad(t) == bad, (name, i, kind)
            if ref is None:
                refused[kind] += 1
                # the literal before a changed first digit ... the literal after a comma at index 71
                assert lo - 4 <= bad <= lo + 72, (name, i, kind, bad)
            else:
                accepted += 1
            total += 1
        assert all(refused[k] > 0 for k in cases.KINDS), (name, refused)
    assert accepted > 0 and total > 2000
    # the random changes: mostly refusals, each in agreement
    n_ref = 0
    for k, t in enumerate(cases.random_changes(base, 300, 99)):
        ref, bad = parse_ref(t), first_bad_re(t)
        assert (bad is None) == (ref is not None)
        if k % 30 == 0:
            assert first_bad(t) == bad
        n_ref += ref is None
    assert n_ref > 200
