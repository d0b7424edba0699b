"""Texts shaped for the zstd block coder's literals + sequences path (generators only, seeded).

The device coder (z_block in sy_amd/csrc/sydelta_kernels.hip) rewrites everything behind
the candidate search in wave-parallel form; these texts reach the forms it treats apart:
blocks of one sequence and tables in RLE mode, sequence counts on either side of 64 and
256, repeat offsets in every form (also after a literal length of 0), runs of repeat
takers, a repeat history that holds a value twice, matches that jump whole 512-position segments or nearly a whole block, Raw / one
stream / four stream literals beside sequences, and block-size edges.  What the corpus
holds is measured and held to floors by tests/test_zstd_corpus.py; the device is compared
with the host form on it by tests/test_gpu_zstd_parse.py."""
import functools
import json
import random

BLOCK = 128 << 10


def _unit(rng, n, lo=97, hi=123):
    return bytes(rng.randrange(lo, hi) for _ in range(n))


def _unit_rep(rng):
    """unit * r: one sequence per block, all three tables in RLE mode."""
    for n in (7, 12, 40, 100, 255):
        for r in (3, 5, 9, 17, 30):
            yield _unit(rng, n) * r


def _fixed_phase(rng):
    """A period whose last `width` bytes change every repetition: reps - 1 sequences of one
    match length (an ML table in RLE mode beside FSE ones), 4, 69 and 299 of them.  The first
    changed byte walks through 75 values, so within the hash candidates' reach (2048 + period
    < 75 * period) no earlier repetition matches further than the previous one."""
    values = list(range(48, 123))
    for period in (29, 33, 64):
        for reps in (5, 70, 300):
            for width in (1, 3):
                body = _unit(rng, period - width)
                rng.shuffle(values)
                yield b"".join(body + bytes([values[r % 75]]) + _unit(rng, width - 1) for r in range(reps))


def _mutated(rng, period, size, every, lo=97, hi=123):
    """A period whose unit changes one byte at a random phase every `every` repetitions
    (0: never), cut at `size` bytes."""
    u = bytearray(_unit(rng, period, lo, hi))
    parts, have, r = [], 0, 0
    while have < size:
        parts.append(bytes(u))
        have += period
        r += 1
        if every and r % every == 0:
            at = rng.randrange(period)
            u[at] = (u[at] - lo + rng.randrange(1, hi - lo)) % (hi - lo) + lo
    return b"".join(parts)[:size]


def _random_phase(rng, lo=97, hi=123):
    for period in (20, 37, 64, 111, 200):
        for every in (1, 2, 5):
            yield _mutated(rng, period, rng.randrange(800, 5000), every, lo, hi)
            yield _mutated(rng, period, rng.randrange(10000, 40000), every, lo, hi)
    for period, every, size in ((600, 0, 30000), (600, 1, 60000), (1500, 0, 50000), (1500, 3, 120000),
                                (5000, 0, 200000), (5000, 2, 60000)):
        yield _mutated(rng, period, size, every, lo, hi)


def _wide_bytes(rng):
    """The same over bytes 40..239: a literal >= 0x80 keeps the literals Raw."""
    yield from _random_phase(rng, 40, 240)


def _interleaved(rng):
    """Texts drawn from 2, 3 and 5 units: the distances alternate, so the older entries of
    the repeat history are used, also after a literal length of 0."""
    for nu in (2, 3, 5):
        for ulen in (9, 24, 70):
            for sep in (b"", b"{", b"},{"):
                units = [_unit(rng, ulen + k) for k in range(nu)]
                size = rng.randrange(4000, 30000)
                parts, have = [], 0
                while have < size:
                    parts.append(rng.choice(units) + sep)
                    have += len(parts[-1])
                yield b"".join(parts)


def _c5(rng):
    """The C5 shape of test_zstd._cases(): consecutive block Copies, a literal op now and then."""
    for nops in (100, 400, 1500):
        for bs in (4096, 8192, 65536):
            for every in (13, 97):
                ops = [{"Copy": {"offset": k * bs, "size": bs}} if k % every else {"Data": [k % 256] * 30}
                       for k in range(nops)]
                yield json.dumps({"ops": ops, "source_size": nops * bs, "block_size": bs}, separators=(",", ":")).encode()


def _structured(rng):
    """test_zstd.test_ref_structured_texts' generator at 300 to 30 000 bytes."""
    for _ in range(40):
        units = [bytes(rng.randrange(97, 97 + rng.randint(2, 20)) for _ in range(rng.randint(1, 60)))
                 for _ in range(rng.randint(1, 6))]
        target = rng.randint(300, 30000)
        parts, size = [], 0
        while size < target:
            u = rng.choice(units)
            k = rng.random()
            if k < 0.3:
                piece = b"{" + u
            elif k < 0.5:
                piece = u[:rng.randint(0, len(u))]
            elif k < 0.6:
                piece = bytes([rng.randrange(256)]) * rng.randint(1, 9)
            else:
                piece = b"{" + u + b"}"
            parts.append(piece)
            size += len(piece)
        yield b"".join(parts)


def _dup_history(rng):
    """Period 600 changing a byte every 1 to 3 repetitions, past three hash rounds: a match whose
    best is a hash candidate some periods back is coded at the repeat distance, the next one
    follows it with no literal at that same distance (the history then holds it twice) and a
    later one reaches past the pair.  The smallest texts with that form, so that the single
    call meets it too."""
    for every in (1, 2, 3):
        for size in (9000, 14000, 20000):
            yield _mutated(rng, 600, size, every)


def _cuts(rng):
    """One mutated-period text cut around the block size."""
    base = _mutated(rng, 150, 2 * BLOCK, 2)
    for n in (BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK - 1):
        yield base[:n]


def _tiny(rng):
    for n in (6, 7, 8, 11, 12, 13, 16, 17, 23, 24, 31, 32, 33, 40):
        u = _unit(rng, rng.randrange(1, 5), 97, 100)
        yield (u * n)[:n]
        yield _unit(rng, n, 97, 99)


FAMILIES = (("unit-rep", _unit_rep), ("fixed-phase", _fixed_phase), ("random-phase", _random_phase),
            ("wide-bytes", _wide_bytes), ("interleaved", _interleaved), ("c5", _c5), ("structured", _structured),
            ("cuts", _cuts), ("tiny", _tiny), ("dup-history", _dup_history))


@functools.lru_cache(None)
def corpus():
    """((family, index in the family, text), ...), the same on every call."""
    out = []
    for f, (name, gen) in enumerate(FAMILIES):
        out.extend((name, i, t) for i, t in enumerate(gen(random.Random(9000 + f))))
    return tuple(out)
