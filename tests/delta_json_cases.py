"""TEST INFRASTRUCTURE: Delta JSON texts aimed at what only the K7d kernels run (the LDS
staging, the SWAR fast path, the literal slab; sy_amd/csrc/sydelta_kernels.hip), shared
by the GPU tests (test_gpu_dparse_edges.py), the CPU check of the lists themselves
(test_delta_json_ref.py) and the emulated device (csrc/emulated_checks.py).  Pure Python.

Geometry: one thread per 64 text bytes, chunk c = [8 + 64c, 8 + 64(c + 1)); a wave covers
4096 bytes, a workgroup 16384.  The fast path takes chunk c when c > 0 and the chunk ends
at least 8 bytes before the region's end E (8 + 64c + 72 <= E)."""
import random

from delta_json_ref import compact

CHUNK, WAVE, GROUP = 64, 4096, 16384
DATA_HEAD = len(b'{"ops":[{"Data":[')  # 17: where the run of a text's first Data op starts
LONGEST_COPY = ("C", 2**64 - 1, 2**64 - 1)  # 68 bytes of text, 70 with the ',{' after it
EDGE_VALUES = (0, 9, 10, 99, 100, 199, 200, 255)


def run_with_text_len(L: int, rng: random.Random) -> bytes:
    """Byte values whose comma-joined text is exactly L >= 1 characters long."""
    assert L >= 1
    parts, rest = [], L + 1  # a value of k digits takes k + 1 characters with its comma
    while rest > 8:
        parts.append(rng.choice((2, 3, 4)))
        rest -= parts[-1]
    parts += {2: [2], 3: [3], 4: [4], 5: [2, 3], 6: [3, 3], 7: [3, 4], 8: [4, 4]}[rest]
    vals = bytes(rng.randrange(10) if k == 2 else rng.randrange(10, 100) if k == 3 else rng.randrange(100, 256)
                 for k in parts)
    assert len(",".join(map(str, vals))) == L
    return vals


def end_cases():
    """One Data op whose region end E has E - 8 = 4096k + d: around the fast path's
    8 + 64c + 72 > E cut and around the partial last wave and workgroup."""
    rng = random.Random(41)
    for k in (1, 4, 5):
        for d in (-73, -72, -71, -1, 0, 1, 63, 64, 65, 71, 72, 73):
            ops = [("D", run_with_text_len(WAVE * k + d + 8 - DATA_HEAD - 2, rng))]
            text = compact(ops, 1, 4096)
            assert text.rindex(b'],"source_size"') - 8 == WAVE * k + d
            yield f"end-{k}-{d}", ops, text


def boundary_cases():
    """The longest token starting at every offset -70..+1 from the first wave's and the
    first workgroup's end, a run of exact length before it and >= 200 literals after."""
    rng = random.Random(42)
    for edge in (8 + WAVE, 8 + GROUP):
        for off in range(-70, 2):
            start = edge + off
            ops = [("D", run_with_text_len(start - DATA_HEAD - 3, rng)), LONGEST_COPY, ("D", rng.randbytes(200 + off % 7))]
            text = compact(ops, 2, 4096)
            assert text.index(b'{"Copy"') == start
            yield f"token-{edge - 8}{off:+d}", ops, text


def dense_ops():   # 32 literal starts per chunk: a wave's literal range is exactly the slab
    rng = random.Random(43)
    return [("D", bytes(rng.randrange(10) for _ in range(7000)))]  # 14 KiB: 3.4 waves


def sparse_ops():  # every value >= 100: 16 literal starts per chunk
    rng = random.Random(44)
    return [("D", bytes(rng.randrange(100, 256) for _ in range(3500)))]


def mixed_ops():
    rng = random.Random(45)
    return [("C", 7, 4096), ("D", bytes(rng.choice(EDGE_VALUES) for _ in range(5000))), ("D", b""), ("C", 0, 1)]


def copy_heavy_ops():
    """Copies with Data ops of 0-3 bytes sprinkled in (waves that own 1-3 literals), and
    a run of > 2 waves in the middle (waves with no op start)."""
    rng = random.Random(46)

    def sprinkle(n):
        for _ in range(n):
            if rng.random() < 0.7:
                yield ("C", rng.randrange(1 << rng.choice((8, 20, 40, 63))), rng.choice((4096, 17, 0)))
            else:
                yield ("D", rng.randbytes(rng.randrange(4)))

    return list(sprinkle(400)) + [("D", rng.randbytes(3500))] + list(sprinkle(400))


def density_cases():
    for name, ops in (("dense", dense_ops()), ("sparse", sparse_ops()), ("mixed", mixed_ops()),
                      ("copy-heavy", copy_heavy_ops())):
        yield name, ops, compact(ops, 3, 4096)


# ---- small texts: the accepted and refused spellings the emulated checks and
# test_gpu_dparse.py use
def small_accepted():
    rng = random.Random(21)
    yield [], 0, 4096
    yield [("D", b"")], 0, 1
    yield [("C", 0, 4096)], 4096, 4096
    yield [("D", bytes(range(256)) * 3)], 768, 4096
    yield [("D", b""), ("C", 2**64 - 1, 2**64 - 1), ("D", b"\x00")], 7, 9
    for _ in range(6):
        ops = []
        for _ in range(rng.randint(1, 60)):
            if rng.random() < 0.6:
                ops.append(("C", rng.randrange(1 << 40), rng.choice([4096, 17, 0])))
            else:
                ops.append(("D", rng.randbytes(rng.choice([0, 1, 2, 63, 64, 65, 300]))))
        yield ops, rng.randrange(1 << 50), rng.choice([512, 4096, 131072])


def small_refused():
    good = compact([("C", 4096, 4096), ("D", b"\x01\xff"), ("D", b"")], 8192, 4096)
    return [b"", b"{}", b'{"ops":[]}', good[:-1], good + b" ", b" " + good, good.replace(b",", b", ", 1),
            good.replace(b'"Copy"', b'"copy"'), good.replace(b'"offset":4096,"size":4096', b'"size":4096,"offset":4096'),
            good.replace(b"[1,255]", b"[1,256]"), good.replace(b"[1,255]", b"[01,255]"), good.replace(b"[1,255]", b"[1,,255]"),
            good.replace(b"[1,255]", b"[1,255,]"), good.replace(b"[1,255]", b"[-1,255]"), good.replace(b"},{", b"}{", 1),
            good.replace(b'"source_size":8192', b'"source_size":08192'),
            good.replace(b'"block_size":4096}', b'"block_size":4096,"x":1}'),
            good.replace(b'{"Data":[]}', b'{"Data":[],"x":0}'), good.replace(b'{"ops":[', b'{"ops" :['),
            good.replace(b"]}]", b"]}}]"),
            good.replace(b'{"Copy":{"offset":4096,"size":4096}}', b'{"Copy":{"offset":4096,"size":4096},"x":1}'),
            # junk before the first op: the chain must start at byte 8
            b'{"ops":[xyz},{"Data":[5]}],"source_size":1,"block_size":1}',
            b'{"ops":[1},{"Copy":{"offset":0,"size":1}}],"source_size":1,"block_size":1}',
            good.replace(b'{"ops":[{', b'{"ops":[ {', 1),
            # the tail: numbers out of range, a second key, a missing brace
            good.replace(b'"source_size":8192', b'"source_size":18446744073709551616'),
            good.replace(b'"block_size":4096', b'"block_size":'), good.replace(b'"block_size":4096}', b'"block_size":4096]'),
            good.replace(b',"block_size"', b',"Block_size"')]


# ---- refused texts
PERIOD = (7, 10, 100, 255, 42, 199, 0, 9, 99, 200)  # "7,10,100,255,42,199,0,9,99,200,": 31 characters
FOREIGN = tuple(b'{}[]:"-.ea ') + (0x00, 0x80, 0xFF)
IN_CHUNK = (0, 1, 2, 3, 31, 60, 61, 62, 63) + tuple(range(64, 72))  # and the 8 look-ahead bytes
KINDS = ("over-255", "leading-zero", "comma-to-digit", "digit-to-comma", "foreign")


def refuse_base():
    """Copy, one Data op of 22000 literals (the 31-character period, so every value
    meets every in-chunk index), Copy: ~70 KiB, more than 4 workgroups."""
    ops = [("C", 123456, 4096), ("D", bytes(PERIOD[i % len(PERIOD)] for i in range(22000))), ("C", 2**40, 17)]
    text = compact(ops, 5, 4096)
    r0 = text.index(b"[", 9) + 1
    return ops, text, r0, text.index(b"]", r0)


def target_chunks(text: bytes, r0: int, r1: int):
    """The first and the last chunk that lie, with their 8 bytes of look-ahead, inside the
    run [r0, r1) (the first and last the fast path owns), chunks at the start, middle and
    end of a wave, and the first and last chunk of a workgroup."""
    first, last = (r0 + 1 - 8 + CHUNK - 1) // CHUNK, (r1 - 72 - 8) // CHUNK
    assert first == 1 and last > 1024 and 8 + CHUNK * last + 72 <= r1
    return {"first-fast": first, "wave1-start": 64, "wave1-mid": 95, "wave1-end": 127, "group1-start": 256,
            "wave7-mid": 479, "group1-end": 511, "last-fast": last}


def _literal_at(t: bytes, p: int):
    """(start, digits) of the literal that covers p, or follows the comma at p."""
    if t[p] == 0x2C:
        p += 1
    while 0x30 <= t[p - 1] <= 0x39:
        p -= 1
    k = 0
    while 0x30 <= t[p + k] <= 0x39:
        k += 1
    return p, k


def changes_at(text: bytes, p: int):
    """(kind, changed text) for every kind of change at byte p of a literal run."""
    def put(q, new):
        return text[:q] + new + text[q + len(new):]

    s, k = _literal_at(text, p)
    if k == 3:
        yield "over-255", put(s, b"9")                      # 9xx
        if text[s:s + 3] == b"255":
            yield "over-255", put(s + 2, b"6")              # 256
        if text[s:s + 3] == b"199":
            yield "over-255", put(s, b"2")                  # 299
    if k >= 2:
        yield "leading-zero", put(s, b"0")                  # 10 -> 00, 100 -> 000, 42 -> 02
    if text[s:s + 3] == b"100":
        yield "leading-zero", put(s, b"010")
    if text[p] == 0x2C:
        yield "comma-to-digit", put(p, b"5")                # a literal of >= 4 digits (or one > 255)
    else:
        yield "digit-to-comma", put(p, b",")                # an empty element, or two shorter values
    for b in FOREIGN:
        yield "foreign", put(p, bytes([b]))


def deterministic_changes(text: bytes, chunk: int):
    """Every kind of change at the IN_CHUNK indices of one chunk: (index, kind, text)."""
    lo = 8 + CHUNK * chunk
    for i in IN_CHUNK:
        for kind, t in changes_at(text, lo + i):
            yield i, kind, t


def random_changes(text: bytes, n: int, seed: int):
    """n texts with 1-3 bytes changed anywhere in [8, E)."""
    rng = random.Random(seed)
    e = text.rindex(b'],"source_size"')
    alphabet = b'0123456789,,,,{}[]:"aDC -' + bytes([0, 0x80, 0xFF])
    for _ in range(n):
        b = bytearray(text)
        for _ in range(rng.randint(1, 3)):
            b[rng.randrange(8, e)] = rng.choice(alphabet)
        yield bytes(b)
