"""TEST INFRASTRUCTURE: blocks that share an Adler-32 and differ in XXH3, and the small
(source, basis) pairs built from them that put a real weak-hash collision on every match
path's walked route (generator.rs:121-155: a window whose weak value is a basis block's is a
hit only if its strong hash is equal too; among several blocks of that weak value the first
in index order with the equal strong hash wins).

Random, periodic and low-alphabet inputs never contain two *different* blocks of one weak
value at block sizes >= 256 with tens of blocks per file, and duplicated blocks share both
hashes; twins are built instead.  A plain helper module (like blake3_ref.py), used by
tests/test_adler_twins.py (the builders checked against both oracles),
tests/test_gpu_collisions.py and tests/csrc/emulated_checks.py.
"""
from __future__ import annotations

import random
import zlib
from dataclasses import dataclass, field

import numpy as np


def twin(block: bytes, rng: random.Random, k: int = 3) -> bytes:
    """A block different from `block` with the same Adler-32.

    One step picks i, j with |i - j| >= 2 (so i, i+1, j, j+1 are four positions) whose bytes
    have headroom and applies +1, -1 at (i, i+1) and -1, +1 at (j, j+1).  The byte sum moves
    by +1 -1 -1 +1 = 0, and the position-weighted sum sum (n - p) b_p by
    (n - i) - (n - i - 1) - (n - j) + (n - j - 1) = 0: both halves of Adler-32 are unchanged
    as integers, before the reduction mod 65521.  k steps; repeated (each time k more) in the
    unlikely case that they cancelled."""
    n = len(block)
    if n < 4:
        raise ValueError("a twin needs four positions")
    b = bytearray(block)
    while True:
        done = 0
        for _ in range(10000):
            if done == k:
                break
            i, j = rng.randrange(n - 1), rng.randrange(n - 1)
            if abs(i - j) < 2 or b[i] == 255 or b[i + 1] == 0 or b[j] == 0 or b[j + 1] == 255:
                continue
            b[i] += 1
            b[i + 1] -= 1
            b[j] -= 1
            b[j + 1] += 1
            done += 1
        if done < k:
            raise ValueError("no headroom for a twin (constant 0x00 / 0xFF data?)")
        if bytes(b) != block:
            return bytes(b)


def family(block: bytes, rng: random.Random, count: int, k: int = 3) -> list:
    """`count` distinct blocks of one Adler-32, the first `block` itself."""
    fam, seen = [block], {block}
    while len(fam) < count:
        t = twin(fam[rng.randrange(len(fam))], rng, k)
        if t not in seen:
            seen.add(t)
            fam.append(t)
    assert len({zlib.adler32(x) for x in fam}) == 1
    return fam


@dataclass
class Scenario:
    """One (source, basis) pair and the op list it exists for (`expect`: what the oracle
    must give, written out by hand; tests/test_adler_twins.py holds the oracles to it, so a
    builder cannot silently degrade into an input without the collision)."""

    name: str
    bs: int
    src: bytes
    basis: bytes
    expect: list
    # synthetic-R6 only: the signature arrays (weak, strong, size) instead of the basis's own
    sig: tuple | None = field(default=None)

    def nblocks(self) -> int:
        return -(-len(self.basis) // self.bs)

    def last_size(self) -> int:
        k = self.nblocks()
        return len(self.basis) - (k - 1) * self.bs if k else 0


def _rng(name: str, bs: int, seed: int) -> random.Random:
    return random.Random(f"{name}/{bs}/{seed}")


def later_candidate(bs: int, seed: int = 0) -> Scenario:
    """Basis F0 X F1 F2 F2 + a short tail; source "zz" F2 F3 F1 "q" F0 X.  F2 is the third
    candidate of its weak value (after F0, F1, whose strong hashes differ) and stands twice:
    block 3, the lower, wins.  F1 is the second candidate: block 2.  F3 has the family's weak
    value and no basis block's strong hash: Data, and the walk resumes one byte on."""
    rng = _rng("later", bs, seed)
    f = family(rng.randbytes(bs), rng, 4)
    x = rng.randbytes(bs)
    tail = rng.randbytes(bs // 3 + 1)
    basis = f[0] + x + f[1] + f[2] + f[2] + tail
    src = b"zz" + f[2] + f[3] + f[1] + b"q" + f[0] + x
    exp = [("D", 0, 2), ("C", 3 * bs, bs), ("D", 2 + bs, bs), ("C", 2 * bs, bs), ("D", 2 + 3 * bs, 1), ("C", 0, bs),
           ("C", bs, bs)]
    return Scenario("later-candidate", bs, src, basis, exp)


def overlap(bs: int, d: int, seed: int = 0, lead: int = 0) -> Scenario:
    """W0 = (P + Y)[:bs] with |P| = d.  Basis twin(W0) Y + a short tail; source P Y twin(W0).
    The window at 0 has a basis block's weak value only; the true hit starts d later, inside
    the span a walk that wrongly resumed at x + n would skip (d < n), or beyond it.
    lead: as many unmatched bytes first, so that the walk meets the false window off its
    block grid, among the window starts it rolls after a miss, and the true hit behind it."""
    rng = _rng("overlap", bs, (seed * 1000003 + d) * 1000003 + lead)
    p, y = rng.randbytes(d), rng.randbytes(bs)
    t = twin((p + y)[:bs], rng)
    basis = t + y + rng.randbytes(bs // 4 + 3)
    src = rng.randbytes(lead) + p + y + t
    name = f"overlap({lead}+{d})" if lead else f"overlap({d})"
    return Scenario(name, bs, src, basis, [("D", 0, lead + d), ("C", bs, bs), ("C", 0, bs)])


def family24(bs: int, seed: int = 0) -> Scenario:
    """Basis F0...F23, source "ab" F23 F24 F5 F0: a 24-long candidate list with the hit on its
    last member, on a middle one and on the first, and a 25th twin that is in no basis block."""
    rng = _rng("family", bs, seed)
    f = family(rng.randbytes(bs), rng, 25)
    basis = b"".join(f[:24])
    src = b"ab" + f[23] + f[24] + f[5] + f[0]
    exp = [("D", 0, 2), ("C", 23 * bs, bs), ("D", 2 + bs, bs), ("C", 5 * bs, bs), ("C", 0, bs)]
    return Scenario("family", bs, src, basis, exp)


def dup_collision(bs: int, seed: int = 0) -> Scenario:
    """Basis F0 F1 F0 F1 F2, source F1 F2 F0: among the blocks of one weak value the lowest
    index with the equal strong hash wins (1, not 3; 0, not 2), past candidates that differ."""
    rng = _rng("dup", bs, seed)
    f = family(rng.randbytes(bs), rng, 3)
    basis = f[0] + f[1] + f[0] + f[1] + f[2]
    src = f[1] + f[2] + f[0]
    return Scenario("dup+collision", bs, src, basis, [("C", bs, bs), ("C", 4 * bs, bs), ("C", 0, bs)])


def tail_twin(bs: int, seed: int = 0, t: int | None = None) -> tuple:
    """The basis X Y T ends in a short block T (t bytes).  One source ends in twin(T) -- the
    last block's weak value and size, not its strong hash: no tail Copy -- and one in T: the
    tail Copy (generator.rs:156-184)."""
    rng = _rng("tail", bs, seed)
    t = bs // 2 + 3 if t is None else t
    x, y, tl = rng.randbytes(bs), rng.randbytes(bs), rng.randbytes(t)
    basis = x + y + tl
    miss = Scenario(f"tail-twin({t})", bs, b"k" + x + twin(tl, rng), basis,
                    [("D", 0, 1), ("C", 0, bs), ("D", 1 + bs, t)])
    hit = Scenario(f"tail-true({t})", bs, b"k" + x + tl, basis, [("D", 0, 1), ("C", 0, bs), ("C", 2 * bs, t)])
    return miss, hit


def synthetic_r6(bs: int, seed: int = 0) -> Scenario:
    """Signature arrays no basis produces (the receiver's are taken as sent): entry 0 a full
    block Q; the last entry, of size 100, carries the (weak, strong) of a full window W.  A
    full window is matched without a size check (generator.rs:127-133), so the source W W Q
    gives Copy(bs, 100) twice, then Copy(0, bs).  `basis` is a stand-in of the same shape (Q +
    100 bytes) for the paths that hash a basis themselves, to be overridden by `sig`."""
    from oracle import oracle as O

    rng = _rng("r6", bs, seed)
    q, w = rng.randbytes(bs), rng.randbytes(bs)
    weak = np.array([zlib.adler32(q), zlib.adler32(w)], np.uint32)
    strong = np.array([O.C().xxh3(q), O.C().xxh3(w)], np.uint64)
    size = np.array([bs, 100], np.uint64)
    exp = [("C", bs, 100), ("C", bs, 100), ("C", 0, bs)]
    return Scenario("synthetic-R6", bs, w + w + q, q + rng.randbytes(100), exp, (weak, strong, size))


# k_scan_r (n = 4096 only, sydelta_kernels.hip): a wave tile is kWTR = 4096 positions, 64 per
# lane, rolled in batches of kB3 = 8; k_walk_files / k_preroll (walk_roll): kWRun = 64 starts
# per lane, kWSub = 4096 per roll pass.
def overlap_distances(bs: int) -> list:
    d = [1, 63, 64, 65, bs - 1]  # a lane's 64-start run
    if bs == 8192:
        d += [4095, 4096, 4097]  # the 4096-start roll pass (kWSub)
    if bs == 4096:
        d += [7, 8, 9, 4096, 4097]  # k_scan_r: a batch (kB3 = 8) and the wave tile (kWTR = 4096; 4095 = bs - 1)
    return sorted(set(d))


def scenarios(bs: int, seed: int = 0, r6: bool = True) -> list:
    """Every scenario at block size bs (synthetic-R6 last, when asked for)."""
    out = [later_candidate(bs, seed)]
    out += [overlap(bs, d, seed) for d in overlap_distances(bs)]
    out += [overlap(bs, d, seed, lead=bs + 37) for d in (1, 65, bs - 1)]
    out += [family24(bs, seed), dup_collision(bs, seed)]
    out += list(tail_twin(bs, seed))
    # a second tail length, on the other side of tail_matches' 240-byte split
    out += list(tail_twin(bs, seed + 1, 200 if bs // 2 + 3 > 240 else bs - 6))
    if r6:
        out.append(synthetic_r6(bs, seed))
    return out
