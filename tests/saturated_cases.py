"""Bytes at the top of the Adler sums' range, and (basis, source) pairs built on them
(generators only, seeded).

Every kernel that carries Adler-32 state defers the modulo: byte sums and position-weighted
sums stay in 32-bit registers under bounds worked out for a byte value of 255 (row_hash, the
four scans, walk_roll, k_preroll).  Random bytes (mean 127.5) reach half of those bounds.  The
families here reach them:

    ff          every byte 0xFF
    fdff        bytes drawn from {0xFD, 0xFE, 0xFF}: distinct blocks, sums within 1 % of the bound
    ff-sparse0  0xFF with a 0x00 about every 61 bytes
    stripes     64-byte stripes of 0x00 and 0xFF in turn (the largest in - out swing of either
                sign in one roll round); one marker byte in each 0x00 stripe keeps blocks distinct
    ramp        stripes that are 0x00 up to a seeded in-stripe offset and 0xFF from there on (the
                weight sits at the high offsets), or 0xFF throughout

A pair's source is its basis cut into three runs of whole blocks, each behind a few bytes that
occur in no family (JUNK).  The junk lengths put the Copies of the three runs on the first, a
middle and the last position of a thread's rolling run, at source positions off the block grid:
an error that builds up behind the run's anchor then costs a Copy and changes the op list.  A
scan thread rolls positions [k * run, (k + 1) * run) of the source, so there the position
modulo `run` counts (rel False); the walk (walk_roll, k_preroll) rolls from the position behind
the miss, so there the length of the literal run in front of the Copy counts (rel True).

What the corpus holds is measured and held to floors by tests/test_saturated_corpus.py with
the C oracle alone; the device is compared with the oracle on it by tests/test_gpu_saturated.py.
"""
import functools

import numpy as np

STRIPE = 64
STRIPE_SUM_MAX = 255 * STRIPE                          # 16 320
STRIPE_WSUM_MAX = 255 * (STRIPE * (STRIPE - 1) // 2)   # 514 080: sum of j * byte, j < 64
JUNK = (0xFA, 0xFB, 0xFC)                              # in no family: markers stay below 0xF0


def _ff(rng, n):
    return np.full(n, 0xFF, np.uint8)


def _fdff(rng, n):
    return rng.integers(0xFD, 0x100, n, dtype=np.uint8)


def _ff_sparse0(rng, n):
    a = np.full(n, 0xFF, np.uint8)
    a[rng.random(n) < 1 / 61] = 0
    return a


def _stripes(rng, n):
    ns = -(-n // STRIPE)
    a = np.zeros(ns * STRIPE, np.uint8)
    s = a.reshape(ns, STRIPE)
    s[1::2] = 0xFF
    zero = np.arange(0, ns, 2)
    s[zero, rng.integers(0, STRIPE, zero.size)] = rng.integers(1, 0xF0, zero.size, dtype=np.uint8)
    return a[:n]


def _ramp(rng, n):
    ns = -(-n // STRIPE)
    first_ff = rng.integers(0, 49, ns)  # 0: the whole stripe is 0xFF
    a = np.where(np.arange(STRIPE)[None, :] >= first_ff[:, None], 0xFF, 0).astype(np.uint8)
    return a.reshape(-1)[:n]


FAMILIES = (("ff", _ff), ("fdff", _fdff), ("ff-sparse0", _ff_sparse0), ("stripes", _stripes), ("ramp", _ramp))
FAMILY_NAMES = tuple(name for name, _ in FAMILIES)


@functools.lru_cache(None)
def family_bytes(family: str, n: int, seed: int = 0) -> bytes:
    """n bytes of a family, the same on every call."""
    f = FAMILY_NAMES.index(family)
    return FAMILIES[f][1](np.random.default_rng(7700 + 97 * seed + f), n).tobytes()


def stripe_sums(data: bytes):
    """(byte sum, sum of j * byte) of each whole 64-byte stripe of data, as int64 arrays."""
    a = np.frombuffer(data, np.uint8)[:len(data) // STRIPE * STRIPE].reshape(-1, STRIPE).astype(np.int64)
    return a.sum(axis=1), (a * np.arange(STRIPE)).sum(axis=1)


def run_targets(run: int):
    """The first, a middle and the last position of a rolling run."""
    return (0, run // 2, run - 1)


def shifted_source(basis: bytes, bs: int, run: int, rel: bool, seed: int = 0, nruns: int = 3) -> bytes:
    """The basis as nruns runs of whole blocks (the last with the partial block), each behind
    junk whose length puts the run's first Copy on run_targets(run)[i % 3] and off the block grid."""
    rng = np.random.default_rng(8800 + seed)
    nfull = len(basis) // bs
    assert nfull >= nruns >= 3
    cuts = [i * nfull // nruns * bs for i in range(nruns)] + [len(basis)]
    out = bytearray()
    for i, (lo, hi) in enumerate(zip(cuts, cuts[1:])):
        r = run_targets(run)[i % 3]
        # rel: the roll starts behind the miss at len(out), so the Copy at len(out) + L is its
        # start number L - 1; else the Copy's own position counts
        L = ((r + 1) if rel else (r - len(out))) % run
        while L < 3 or (len(out) + L) % bs == 0:
            L += run
        out += rng.choice(JUNK, L).astype(np.uint8).tobytes()
        out += basis[lo:hi]
    return bytes(out)


def basis_len(bs: int) -> int:
    """Nine blocks or a scan tile's worth of them, and a partial last block."""
    return max(9 * bs, (1 << 20) if bs >= 1024 else (1 << 19)) // bs * bs + bs // 3 + 5


@functools.lru_cache(None)
def pair(family: str, bs: int, run: int, rel: bool = False):
    """(basis, source) of a family at a block size."""
    basis = family_bytes(family, basis_len(bs), bs)
    return basis, shifted_source(basis, bs, run, rel, bs)


def copies_by_run_position(ops, bs: int, run: int, rel: bool):
    """How many Copies of whole blocks at source positions off the block grid fall on each of
    run_targets(run): by position modulo run, or (rel) by the literal run in front of them."""
    got = dict.fromkeys(run_targets(run), 0)
    pos, prev = 0, None
    for op in ops:
        kind, size = op[0], op[2]
        if kind == "C" and size == bs and pos % bs != 0:
            at = None
            if not rel:
                at = pos % run
            elif prev is not None and prev[0] == "D":
                at = (prev[2] - 1) % run
            if at in got:
                got[at] += 1
        pos += size
        prev = op
    return got


# The rolling run of each scan kernel (sy_amd/csrc/sydelta_kernels.hip: kScanRun for k_scan, a
# lane's 64 positions in the LDS-staged and register-fed scans) and of the walk
# (sy_amd/csrc/sydelta_filewalk.hip: kWRun); tests/test_saturated_corpus.py reads them back
# from the sources.
RUN_SCAN = 256
RUN_LANE = 64
RUN_WALK = 64

# (id, kernel that must run, block size, run, environment): every position rolled (SYDELTA_PROBE=0)
SCAN_CASES = (
    ("lds-1024", "k_scan_lds", 1024, RUN_LANE, {"SYDELTA_SCAN_SMALL": "0"}),
    ("lds-8192", "k_scan_lds", 8192, RUN_LANE, {"SYDELTA_SCAN_SMALL": "0"}),
    ("r-small-4096", "k_scan_r", 4096, RUN_LANE, {"SYDELTA_SCAN_SMALL": "1"}),
    ("g-small-256", "k_scan_g", 256, RUN_LANE, {"SYDELTA_SCAN_SMALL": "1"}),
    ("g-small-8192", "k_scan_g", 8192, RUN_LANE, {"SYDELTA_SCAN_SMALL": "1"}),
    ("g-small-1007", "k_scan_g", 1007, RUN_LANE, {"SYDELTA_SCAN_SMALL": "1"}),  # k_verify_w: one window per wave
    ("g-wide-8256", "k_scan_g", 8256, RUN_LANE, {}),
    ("g-wide-131072", "k_scan_g", 131072, RUN_LANE, {}),
    ("scan-9999", "k_scan", 9999, RUN_SCAN, {"SYDELTA_SCAN_WIDE": "0"}),
    ("scan-131072", "k_scan", 131072, RUN_SCAN, {"SYDELTA_SCAN_WIDE": "0"}),
)
WALK_BLOCK_SIZES = (256, 4096, 8192)


def scan_families(bs: int):
    """The families a scan case runs at a block size.  Every window of constant data is a
    verified hit, so with every position rolled the hashing grows with positions x block size
    (137 GB at 128 KiB for 1 MiB of source): the constant family stays at windows up to 8 KiB,
    where it reaches every scan kernel; ff-sparse0 carries 0xFF runs to the larger windows."""
    return FAMILY_NAMES if bs <= 8192 else tuple(f for f in FAMILY_NAMES if f != "ff")


def row_hash_max_n() -> int:
    """kRowHashMaxN of sy_amd/csrc/sydelta_internal.hpp: the largest window of the row layout."""
    import os
    import re

    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sy_amd", "csrc",
                        "sydelta_internal.hpp")
    m = re.search(r"constexpr uint32_t kRowHashMaxN = (\d+)u \* (\d+)u;", open(path).read())
    return int(m.group(1)) * int(m.group(2))


@functools.lru_cache(None)
def walk_pairs(bs: int, nfiles: int = 40):
    """((basis, source), ...): small files of every family in turn, 6 to 18 blocks and a partial
    one, the Copies placed for the walk's roll."""
    out = []
    for i in range(nfiles):
        n = (6 + (i * 7) % 13) * bs + (i * 37 + 11) % bs
        basis = family_bytes(FAMILY_NAMES[i % len(FAMILY_NAMES)], n, 1000 + i)
        out.append((basis, shifted_source(basis, bs, RUN_WALK, True, 1000 + i)))
    return tuple(out)


CHUNK_BS = 256
CHUNK_SEG = 64  # blocks per segment (SYDELTA_CHUNK_SEG): 600 segments, so the chunk is walked in two parts


@functools.lru_cache(None)
def chunk_pair():
    """(basis, source) for the chunk path (k_preroll, k_chunk_write): 120 segments of each family
    and 90 literal runs, each a miss that the pre-roll rolls from."""
    per = 120 * CHUNK_SEG * CHUNK_BS
    basis = b"".join(family_bytes(f, per, 2000) for f in FAMILY_NAMES) + family_bytes("fdff", 77, 2001)
    return basis, shifted_source(basis, CHUNK_BS, RUN_WALK, True, 2000, nruns=90)
