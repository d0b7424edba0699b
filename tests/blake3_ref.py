"""BLAKE3-256 written from the specification (test infrastructure, no test in here).

Two forms of the hash, which must agree:

* ``blake3_recursive``: plain Python, the tree by the specification's rule (the left
  subtree holds the largest power of two of chunks strictly below the chunk count);
* ``blake3``: numpy, vectorised across chunks, the tree level by level (neighbours
  pair up, an odd last node moves up unchanged).

``subtree_cv(data, first_chunk)`` is the non-root chaining value of a piece whose first
chunk is chunk ``first_chunk`` of a larger input, and ``join`` merges such values.
"""
import numpy as np

IV = (0x6A09E667, 0xBB67AE85, 0x3C6EF372, 0xA54FF53A, 0x510E527F, 0x9B05688C, 0x1F83D9AB, 0x5BE0CD19)
PERM = (2, 6, 3, 10, 7, 0, 4, 13, 1, 11, 12, 5, 9, 14, 15, 8)
CHUNK_START, CHUNK_END, PARENT, ROOT = 1, 2, 4, 8
M32 = 0xFFFFFFFF


# ---------------------------------------------------------------------------
# plain form
# ---------------------------------------------------------------------------
def _rotr(x, r):
    return ((x >> r) | (x << (32 - r))) & M32


def _g(s, a, b, c, d, mx, my):
    s[a] = (s[a] + s[b] + mx) & M32
    s[d] = _rotr(s[d] ^ s[a], 16)
    s[c] = (s[c] + s[d]) & M32
    s[b] = _rotr(s[b] ^ s[c], 12)
    s[a] = (s[a] + s[b] + my) & M32
    s[d] = _rotr(s[d] ^ s[a], 8)
    s[c] = (s[c] + s[d]) & M32
    s[b] = _rotr(s[b] ^ s[c], 7)


def compress(cv, m, counter, block_len, flags):
    """The first 8 output words (the next chaining value, or with ROOT the hash)."""
    s = list(cv) + list(IV[:4]) + [counter & M32, (counter >> 32) & M32, block_len, flags]
    m = list(m)
    for r in range(7):
        _g(s, 0, 4, 8, 12, m[0], m[1])
        _g(s, 1, 5, 9, 13, m[2], m[3])
        _g(s, 2, 6, 10, 14, m[4], m[5])
        _g(s, 3, 7, 11, 15, m[6], m[7])
        _g(s, 0, 5, 10, 15, m[8], m[9])
        _g(s, 1, 6, 11, 12, m[10], m[11])
        _g(s, 2, 7, 8, 13, m[12], m[13])
        _g(s, 3, 4, 9, 14, m[14], m[15])
        m = [m[PERM[i]] for i in range(16)]
    return [s[i] ^ s[i + 8] for i in range(8)]


def _words(b):
    return [int.from_bytes(b[i:i + 4], "little") for i in range(0, len(b), 4)]


def _bytes(w):
    return b"".join(int(x).to_bytes(4, "little") for x in w)


def _chunk_cv(chunk, counter, root):
    cv = list(IV)
    nb = max(1, -(-len(chunk) // 64))
    for b in range(nb):
        blk = chunk[64 * b:64 * b + 64]
        fl = (CHUNK_START if b == 0 else 0) | ((CHUNK_END | (ROOT if root else 0)) if b == nb - 1 else 0)
        cv = compress(cv, _words(blk.ljust(64, b"\0")), counter, len(blk), fl)
    return cv


def _parent(left, right, root):
    return compress(IV, list(left) + list(right), 0, 64, PARENT | (ROOT if root else 0))


def _subtree(data, first_chunk, root, memo=None):
    n = max(1, -(-len(data) // 1024))
    if n == 1:
        if memo is None:
            return _chunk_cv(data, first_chunk, root)
        key = (data, first_chunk, root)
        if key not in memo:
            memo[key] = _chunk_cv(data, first_chunk, root)
        return memo[key]
    left = 1 << ((n - 1).bit_length() - 1)  # the largest power of two strictly below n
    return _parent(_subtree(data[:left * 1024], first_chunk, False, memo),
                   _subtree(data[left * 1024:], first_chunk + left, False, memo), root)


def blake3_recursive(data: bytes, memo=None) -> bytes:
    """memo: a dict that keeps chunk chaining values by (chunk bytes, counter, root flag)
    between calls, for callers that hash many inputs with chunks in common."""
    return _bytes(_subtree(bytes(data), 0, True, memo))


def subtree_cv_recursive(data: bytes, first_chunk: int, memo=None) -> bytes:
    return _bytes(_subtree(bytes(data), first_chunk, False, memo))


# ---------------------------------------------------------------------------
# numpy form: every array holds one word of many independent compressions
# ---------------------------------------------------------------------------
def _np_rotr(x, r):
    return (x >> np.uint32(r)) | (x << np.uint32(32 - r))


def _np_g(s, a, b, c, d, mx, my):
    s[a] = s[a] + s[b] + mx
    s[d] = _np_rotr(s[d] ^ s[a], 16)
    s[c] = s[c] + s[d]
    s[b] = _np_rotr(s[b] ^ s[c], 12)
    s[a] = s[a] + s[b] + my
    s[d] = _np_rotr(s[d] ^ s[a], 8)
    s[c] = s[c] + s[d]
    s[b] = _np_rotr(s[b] ^ s[c], 7)


def _np_compress(cv, m, counter, block_len, flags):
    """cv: (8, n) uint32; m: (16, n); counter: (n,) uint64; block_len, flags: (n,) uint32 -> (8, n)."""
    n = cv.shape[1]
    s = [cv[i].copy() for i in range(8)] + [np.full(n, IV[i], dtype=np.uint32) for i in range(4)]
    s += [(counter & np.uint64(M32)).astype(np.uint32), (counter >> np.uint64(32)).astype(np.uint32),
          block_len.astype(np.uint32), flags.astype(np.uint32)]
    idx = list(range(16))
    for r in range(7):
        _np_g(s, 0, 4, 8, 12, m[idx[0]], m[idx[1]])
        _np_g(s, 1, 5, 9, 13, m[idx[2]], m[idx[3]])
        _np_g(s, 2, 6, 10, 14, m[idx[4]], m[idx[5]])
        _np_g(s, 3, 7, 11, 15, m[idx[6]], m[idx[7]])
        _np_g(s, 0, 5, 10, 15, m[idx[8]], m[idx[9]])
        _np_g(s, 1, 6, 11, 12, m[idx[10]], m[idx[11]])
        _np_g(s, 2, 7, 8, 13, m[idx[12]], m[idx[13]])
        _np_g(s, 3, 4, 9, 14, m[idx[14]], m[idx[15]])
        idx = [idx[PERM[i]] for i in range(16)]
    return np.stack([s[i] ^ s[i + 8] for i in range(8)])


def _np_tree(data, first_chunk, root):
    if not isinstance(data, np.ndarray):
        data = np.frombuffer(bytes(data), dtype=np.uint8)
    ln = data.size
    n = max(1, -(-ln // 1024))
    padded = np.zeros(n * 1024, dtype=np.uint8)
    padded[:ln] = data
    words = padded.view("<u4").reshape(n, 16, 16)  # chunk, block, word
    clen = np.full(n, 1024, dtype=np.int64)
    clen[-1] = ln - (n - 1) * 1024
    nblk = np.maximum(1, -(-clen // 64))
    counter = np.arange(n, dtype=np.uint64) + np.uint64(first_chunk)
    cv = np.repeat(np.array(IV, dtype=np.uint32)[:, None], n, axis=1)
    with np.errstate(over="ignore"):
        for b in range(16):
            live = b < nblk
            if not live.any():
                break
            bl = np.clip(clen - 64 * b, 0, 64).astype(np.uint32)
            fl = np.where(b == 0, CHUNK_START, 0) | np.where(b == nblk - 1, CHUNK_END | (ROOT if root and n == 1 else 0), 0)
            new = _np_compress(cv, np.ascontiguousarray(words[:, b, :].T), counter, bl, fl.astype(np.uint32))
            cv = np.where(live[None, :], new, cv)
        while cv.shape[1] > 1:  # level by level
            k = cv.shape[1]
            half = k // 2
            m = np.concatenate([cv[:, 0:2 * half:2], cv[:, 1:2 * half:2]], axis=0)
            flags = np.full(half, PARENT | (ROOT if root and k == 2 else 0), dtype=np.uint32)
            up = _np_compress(np.repeat(np.array(IV, dtype=np.uint32)[:, None], half, axis=1), m,
                              np.zeros(half, dtype=np.uint64), np.full(half, 64, dtype=np.uint32), flags)
            cv = np.concatenate([up, cv[:, 2 * half:]], axis=1)
    return cv[:, 0].astype("<u4").tobytes()


def blake3(data) -> bytes:
    """BLAKE3-256 of bytes or a uint8 array (level-wise, vectorised across chunks)."""
    return _np_tree(data, 0, True)


def subtree_cv(data, first_chunk: int) -> bytes:
    return _np_tree(data, first_chunk, False)


def pieces(total_len: int, piece_chunks: int):
    """(offset, length, first_chunk, chunks) of the pieces of piece_chunks chunks of an input."""
    step = piece_chunks * 1024
    return [(o, min(step, total_len - o), o // 1024, -(-min(step, total_len - o) // 1024))
            for o in range(0, total_len, step)]


def join(cvs) -> bytes:
    """Root hash from the chaining values of equal power-of-two pieces (the last one may be
    shorter), in order: the levels above the pieces, pairing neighbours."""
    level = [_words(c) for c in cvs]
    assert len(level) >= 2
    while len(level) > 1:
        k = len(level)
        nxt = [_parent(level[i], level[i + 1], k == 2) for i in range(0, k - 1, 2)]
        if k & 1:
            nxt.append(level[-1])
        level = nxt
    return _bytes(level[0])


def pattern(n: int) -> bytes:
    """The input of the published test vectors."""
    return bytes(i % 251 for i in range(n))


# BLAKE3-256 of pattern(n), from the published test vectors
VECTORS = {
    0: "af1349b9f5f9a1a6a0404dea36dcc9499bcb25c9adc112b7cc9a93cae41f3262",
    1: "2d3adedff11b61f14c886e35afa036736dcd87a74d27b5c1510225d0f592e213",
    64: "4eed7141ea4a5cd4b788606bd23f46e212af9cacebacdc7d1f4c6dc7f2511b98",
    65: "de1e5fa0be70df6d2be8fffd0e99ceaa8eb6e8c93a63f2d8d1c30ecb6b263dee",
    1023: "10108970eeda3eb932baac1428c7a2163b0e924c9a9e25b35bba72b28f70bd11",
    1024: "42214739f095a406f3fc83deb889744ac00df831c10daa55189b5d121c855af7",
    1025: "d00278ae47eb27b34faecf67b4fe263f82d5412916c1ffd97c8cb7fb814b8444",
    2048: "e776b6028c7cd22a4d0ba182a8bf62205d2ef576467e838ed6f2529b85fba24a",
    2049: "5f4d72f40d7a5f82b15ca2b2e44b1de3c2ef86c426c95c1af0b6879522563030",
    3072: "b98cb0ff3623be03326b373de6b9095218513e64f1ee2edd2525c7ad1e5cffd2",
    3073: "7124b49501012f81cc7f11ca069ec9226cecb8a2c850cfe644e327d22d3e1cd3",
    4097: "9b4052b38f1c5fc8b1f9ff7ac7b27cd242487b3d890d15c96a1c25b8aa0fb995",
    5121: "628bd2cb2004694adaab7bbd778a25df25c47b9d4155a55f8fbd79f2fe154cff",
    7169: "a003fc7a51754a9b3c7fae0367ab3d782dccf28855a03d435f8cfe74605e7817",
    8193: "bab6c09cb8ce8cf459261398d2e7aef35700bf488116ceb94a36d0f5f1b7bc3b",
    16384: "f875d6646de28985646f34ee13be9a576fd515f76b5b0a26bb324735041ddde4",
    31744: "62b6960e1a44bcc1eb1a611a8d6235b6b4b78f32e7abc4fb4c6cdcce94895c47",
    102400: "bc3e3d41a1146b069abffad3c0d44860cf664390afce4d9661f7902e7943e085",
}
ABC = "6437b3ac38465133ffb63b75273a8db548c558465d79db03fd359c6cd5bd9d85"
