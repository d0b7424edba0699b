"""TEST INFRASTRUCTURE: an independent reference for the compact Delta JSON (K7, K7d).
Pure Python; imports nothing from sy_amd.

* compact(ops, source_size, block_size): serde_json::to_string(&Delta) restated with
  json.dumps (generator.rs:10-25: DeltaOp::Copy{offset,size} / DeltaOp::Data(Vec<u8>),
  then source_size, block_size; serde's separators).
* parse_ref(text): the contract of sydelta_delta_from_json_device (include/sydelta.h): a
  text is accepted exactly when it is the compact text of a Delta, and then parses to it.
  json.loads reads it, the structure and the number types are checked, and the parse has
  to re-serialise to the very same bytes.
* first_bad(text): the position the device parser names for a refused text.  The
  grammar of the head comment of sy_amd/csrc/sydelta_dparse.hpp restated position by
  position, with the head and tail checks of sydelta_delta_from_json_device before it:

    text   = '{"ops":[' region '],"source_size":' u64 ',"block_size":' u64 '}'
    region = [8, E), E the last '],"source_size":' within the last 96 bytes of the text
    op start       '{' at 8, or '{' right after '},'
    literal start  a digit right after '[' or ','
    Copy op   '{"Copy":{"offset":' u64 ',"size":' u64 '}}' follow
    Data op   '{"Data":[' then ']}' follow, or a digit (a literal start)
    literal   u8, then ',' and a digit, or ']}' follow
    follow    the region's end, or ',{'
    u64 / u8  digits, no leading zero unless the number is 0, in range
    no token reads past E

  The device names the smallest op start or literal start whose token fails, 8 when a
  non-empty region does not open with an op."""
import json
import re

U64 = (1 << 64) - 1
HEAD = b'{"ops":['
TAIL_KEY = b'],"source_size":'
BS_KEY = b',"block_size":'
TAIL_WINDOW = 96


def compact(ops, source_size, block_size) -> bytes:
    """ops: [("C", offset, size) | ("D", bytes)]."""
    return json.dumps({"ops": [{"Copy": {"offset": o[1], "size": o[2]}} if o[0] == "C" else {"Data": list(o[1])}
                               for o in ops], "source_size": source_size, "block_size": block_size},
                      separators=(",", ":")).encode()


def _u64(x) -> bool:
    return type(x) is int and 0 <= x <= U64


def parse_ref(text: bytes):
    """(ops, source_size, block_size), or None for a text that is not a Delta's compact text."""
    try:
        d = json.loads(bytes(text).decode("ascii"))
    except (ValueError, RecursionError):  # UnicodeDecodeError and JSONDecodeError are ValueErrors
        return None
    if type(d) is not dict or set(d) != {"ops", "source_size", "block_size"}:
        return None
    if type(d["ops"]) is not list or not _u64(d["source_size"]) or not _u64(d["block_size"]):
        return None
    ops = []
    for o in d["ops"]:
        if type(o) is not dict or len(o) != 1:
            return None
        (k, v), = o.items()
        if k == "Copy":
            if type(v) is not dict or set(v) != {"offset", "size"} or not _u64(v["offset"]) or not _u64(v["size"]):
                return None
            ops.append(("C", v["offset"], v["size"]))
        elif k == "Data":
            if type(v) is not list or not all(type(x) is int and 0 <= x <= 255 for x in v):
                return None
            ops.append(("D", bytes(v)))
        else:
            return None
    got = ops, d["source_size"], d["block_size"]
    return got if compact(*got) == bytes(text) else None


def _dec(t: bytes, p: int, end: int, maxv: int) -> int:
    """Digits of the number at t[p, end) (0: none, a leading zero, or a value past maxv)."""
    k = 0
    while p + k < end and 0x30 <= t[p + k] <= 0x39:
        k += 1
    if k == 0 or k > 20 or (k > 1 and t[p] == 0x30) or int(t[p:p + k]) > maxv:  # 2^64 has 20 digits
        return 0
    return k


def _is_digit(c: int) -> bool:
    return 0x30 <= c <= 0x39


def region_end(text: bytes):
    """(E, None) for a text whose head and tail are in form, else (None, the position the
    host side of sydelta_delta_from_json_device names)."""
    t = bytes(text)
    n = len(t)
    if n < len(HEAD) + len(TAIL_KEY) + 17:  # the shortest text: {"ops":[],"source_size":0,"block_size":0}
        return None, 0
    if t[:8] != HEAD:
        return None, 0
    tl = min(n - 8, TAIL_WINDOW)
    base = n - tl
    at = t.rfind(TAIL_KEY, base)
    if at < 0:
        return None, base
    q = at + len(TAIL_KEY)
    k = _dec(t, q, n, U64)
    if not k:
        return None, q
    q += k
    if t[q:q + len(BS_KEY)] != BS_KEY:
        return None, q
    q += len(BS_KEY)
    k = _dec(t, q, n, U64)
    if not k:
        return None, q
    q += k
    if not (q + 1 == n and t[q] == 0x7D):
        return None, q
    return at, None


def _follow(t: bytes, q: int, e: int) -> bool:
    return q == e or (q + 1 < e and t[q] == 0x2C and t[q + 1] == 0x7B)


def _lit(t: bytes, q: int, e: int, s: bytes):
    """q past s when t[q:] spells s inside the region, else None."""
    return q + len(s) if q + len(s) <= e and t[q:q + len(s)] == s else None


def _op_ok(t: bytes, p: int, e: int) -> bool:
    q = _lit(t, p, e, b'{"Copy":{"offset":')
    if q is not None:
        k = _dec(t, q, e, U64)
        if not k:
            return False
        q = _lit(t, q + k, e, b',"size":')
        if q is None:
            return False
        k = _dec(t, q, e, U64)
        if not k:
            return False
        q = _lit(t, q + k, e, b"}}")
        return q is not None and _follow(t, q, e)
    q = _lit(t, p, e, b'{"Data":[')
    if q is None:
        return False
    if q < e and t[q] == 0x5D:  # empty Data
        q = _lit(t, q + 1, e, b"}")
        return q is not None and _follow(t, q, e)
    return q < e and _is_digit(t[q])  # the first literal: checked as a literal start


def _literal_ok(t: bytes, p: int, e: int) -> bool:
    k = _dec(t, p, e, 255)
    if not k:
        return False
    q = p + k
    if q < e and t[q] == 0x2C:
        return q + 1 < e and _is_digit(t[q + 1])
    q = _lit(t, q, e, b"]}")
    return q is not None and _follow(t, q, e)


_BAD_LITERAL = re.compile(rb"(?<=[\[,])(?=[0-9])(?!(?:0|[1-9][0-9]?|1[0-9][0-9]|2[0-4][0-9]|25[0-5])"
                          rb"(?:,[0-9]|\]\}(?:,\{|\Z)))")
_OP_START = re.compile(rb"(?<=\},)\{")


def first_bad_re(text: bytes):
    """first_bad for long texts (tens of KiB, thousands of them in the GPU tests): the
    literal rule as one regular expression searched over the region (endpos = E, so no
    token reads past it), the op rule with _op_ok at each op start.  test_delta_json_ref
    holds it to first_bad."""
    t = bytes(text)
    e, bad = region_end(t)
    if e is None:
        return bad
    if e == 8:
        return None
    if t[8] != 0x7B:
        return 8
    m = _BAD_LITERAL.search(t, 8, e)
    best = m.start() if m else None
    if not _op_ok(t, 8, e):
        return 8
    for m in _OP_START.finditer(t, 8, e):
        if best is not None and m.start() > best:
            break
        if not _op_ok(t, m.start(), e):
            return m.start()
    return best


def first_bad(text: bytes):
    """The byte the device parser names, or None for a text in the compact form."""
    t = bytes(text)
    e, bad = region_end(t)
    if e is None:
        return bad
    if e == 8:
        return None
    if t[8] != 0x7B:
        return 8
    for p in range(8, e):
        c = t[p]
        if c == 0x7B:
            if (p == 8 or (t[p - 1] == 0x2C and t[p - 2] == 0x7D)) and not _op_ok(t, p, e):
                return p
        elif _is_digit(c) and t[p - 1] in (0x5B, 0x2C) and not _literal_ok(t, p, e):
            return p
    return None
