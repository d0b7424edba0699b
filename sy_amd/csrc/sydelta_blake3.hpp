// sydelta_blake3.hpp — BLAKE3-256 (unkeyed hash mode), written from the BLAKE3 specification:
// the compression function shared by the device kernels (sydelta_blake3.hip) and the host
// (sydelta_blake3.cpp: joining chaining values, the constant hash of an empty input), and
// the launcher of the kernels.  The portable part compiles with any C++17 compiler.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SYDELTA_B3_FN __host__ __device__ __forceinline__
#else
#define SYDELTA_B3_FN inline
#endif

namespace sydelta {
namespace b3 {

constexpr uint32_t kChunkStart = 1, kChunkEnd = 2, kParent = 4, kRoot = 8;
constexpr uint32_t kBlockLen = 64, kChunkLen = 1024;
constexpr uint32_t kIV0 = 0x6A09E667u, kIV1 = 0xBB67AE85u, kIV2 = 0x3C6EF372u, kIV3 = 0xA54FF53Au;
constexpr uint32_t kIV4 = 0x510E527Fu, kIV5 = 0x9B05688Cu, kIV6 = 0x1F83D9ABu, kIV7 = 0x5BE0CD19u;

// Message word read at position i of round r: the spec permutes the message block between
// rounds; applied r times to the identity that is a fixed table, so with the rounds
// unrolled the permutation names registers and moves nothing.
constexpr int sched(int r, int i) {
    constexpr int perm[16] = {2, 6, 3, 10, 7, 0, 4, 13, 1, 11, 12, 5, 9, 14, 15, 8};
    int v = i;
    for (int k = 0; k < r; ++k) v = perm[v];
    return v;
}

template <int R, int I>
struct SchedAt {
    static constexpr int v = sched(R, I);
};

SYDELTA_B3_FN uint32_t rotr(uint32_t x, int r) { return (x >> r) | (x << (32 - r)); }

// the quarter round: 2 three-operand adds, 2 adds, 4 xors, 4 rotates
SYDELTA_B3_FN void g(uint32_t& a, uint32_t& b, uint32_t& c, uint32_t& d, uint32_t mx, uint32_t my) {
    a = a + b + mx;
    d = rotr(d ^ a, 16);
    c = c + d;
    b = rotr(b ^ c, 12);
    a = a + b + my;
    d = rotr(d ^ a, 8);
    c = c + d;
    b = rotr(b ^ c, 7);
}

template <int R>
SYDELTA_B3_FN void round_fn(uint32_t (&s)[16], const uint32_t (&m)[16]) {
#define SYDELTA_B3_M(i) m[SchedAt<R, i>::v]
    g(s[0], s[4], s[8], s[12], SYDELTA_B3_M(0), SYDELTA_B3_M(1));
    g(s[1], s[5], s[9], s[13], SYDELTA_B3_M(2), SYDELTA_B3_M(3));
    g(s[2], s[6], s[10], s[14], SYDELTA_B3_M(4), SYDELTA_B3_M(5));
    g(s[3], s[7], s[11], s[15], SYDELTA_B3_M(6), SYDELTA_B3_M(7));
    g(s[0], s[5], s[10], s[15], SYDELTA_B3_M(8), SYDELTA_B3_M(9));
    g(s[1], s[6], s[11], s[12], SYDELTA_B3_M(10), SYDELTA_B3_M(11));
    g(s[2], s[7], s[8], s[13], SYDELTA_B3_M(12), SYDELTA_B3_M(13));
    g(s[3], s[4], s[9], s[14], SYDELTA_B3_M(14), SYDELTA_B3_M(15));
#undef SYDELTA_B3_M
}

// cv <- the first 8 words of compress(cv, m, counter, block_len, flags): the next chaining
// value, or with kRoot the 32-byte hash (as little-endian words).
SYDELTA_B3_FN void compress(uint32_t (&cv)[8], const uint32_t (&m)[16], uint64_t counter, uint32_t block_len,
                            uint32_t flags) {
    uint32_t s[16] = {cv[0], cv[1], cv[2], cv[3], cv[4], cv[5], cv[6], cv[7],
                      kIV0,  kIV1,  kIV2,  kIV3,  (uint32_t)counter, (uint32_t)(counter >> 32), block_len, flags};
    round_fn<0>(s, m);
    round_fn<1>(s, m);
    round_fn<2>(s, m);
    round_fn<3>(s, m);
    round_fn<4>(s, m);
    round_fn<5>(s, m);
    round_fn<6>(s, m);
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 8; ++i) cv[i] = s[i] ^ s[i + 8];
}

SYDELTA_B3_FN void iv(uint32_t (&cv)[8]) {
    cv[0] = kIV0, cv[1] = kIV1, cv[2] = kIV2, cv[3] = kIV3;
    cv[4] = kIV4, cv[5] = kIV5, cv[6] = kIV6, cv[7] = kIV7;
}

// left <- the parent node of (left, right): key = IV, counter 0, block_len 64
SYDELTA_B3_FN void parent(uint32_t (&left)[8], const uint32_t (&right)[8], bool root) {
    const uint32_t m[16] = {left[0],  left[1],  left[2],  left[3],  left[4],  left[5],  left[6],  left[7],
                            right[0], right[1], right[2], right[3], right[4], right[5], right[6], right[7]};
    iv(left);
    compress(left, m, 0, kBlockLen, kParent | (root ? kRoot : 0u));
}

// Chunks of an input of len bytes (an empty input is one empty chunk).
constexpr uint64_t chunks_of(uint64_t len) { return len ? (len + kChunkLen - 1) / kChunkLen : 1; }

// The tree over n leaves, level by level: nodes 2i and 2i+1 of a level join into node i of
// the next, an odd last node moves up unchanged.  That is the spec's tree (the left subtree
// holds the largest power of two of leaves below n): by induction a level's node i covers
// leaves [i 2^l, min((i+1) 2^l, n)), so below the top the left child of every parent is a
// full power of two and the right child is what remains.
// cvs (n * 8 words) is reduced in place to cvs[0..8); root marks the last parent.
inline void reduce_levels(uint32_t* cvs, uint64_t n, bool root) {
    while (n > 1) {
        const uint64_t half = n / 2;
        for (uint64_t i = 0; i < half; ++i) {
            uint32_t l[8], r[8];
            for (int k = 0; k < 8; ++k) l[k] = cvs[16 * i + k], r[k] = cvs[16 * i + 8 + k];
            parent(l, r, root && n == 2);
            for (int k = 0; k < 8; ++k) cvs[8 * i + k] = l[k];
        }
        if (n & 1)
            for (int k = 0; k < 8; ++k) cvs[8 * half + k] = cvs[8 * (n - 1) + k];
        n = half + (n & 1);
    }
}

// Portable whole-input form (host: tiny inputs and checks; not a hot path).  root = false
// gives the chaining value of the subtree whose first chunk is chunk first_chunk of a
// larger input.  out: 8 little-endian words.
inline void hash_host(const uint8_t* p, uint64_t len, uint64_t first_chunk, bool root, uint32_t out[8]) {
    const uint64_t n = chunks_of(len);
    uint32_t* cvs = new uint32_t[8 * n];
    for (uint64_t c = 0; c < n; ++c) {
        const uint64_t clen = len - c * kChunkLen < kChunkLen ? len - c * kChunkLen : kChunkLen;
        const uint32_t nb = clen ? (uint32_t)((clen + 63) / 64) : 1;
        uint32_t cv[8];
        iv(cv);
        for (uint32_t b = 0; b < nb; ++b) {
            const uint64_t left = clen - 64ull * b;
            const uint32_t bl = left < 64 ? (uint32_t)left : 64;
            uint8_t blk[64] = {0};
            for (uint32_t k = 0; k < bl; ++k) blk[k] = p[c * kChunkLen + 64 * b + k];
            uint32_t m[16];
            for (int k = 0; k < 16; ++k)
                m[k] = (uint32_t)blk[4 * k] | (uint32_t)blk[4 * k + 1] << 8 | (uint32_t)blk[4 * k + 2] << 16 |
                       (uint32_t)blk[4 * k + 3] << 24;
            const uint32_t fl = (b == 0 ? kChunkStart : 0u) | (b + 1 == nb ? kChunkEnd | (root && n == 1 ? kRoot : 0u) : 0u);
            compress(cv, m, first_chunk + c, bl, fl);
        }
        for (int k = 0; k < 8; ++k) cvs[8 * c + k] = cv[k];
    }
    reduce_levels(cvs, n, root);
    for (int k = 0; k < 8; ++k) out[k] = cvs[k];
    delete[] cvs;
}

inline void words_to_bytes(const uint32_t w[8], uint8_t out[32]) {
    for (int k = 0; k < 8; ++k)
        for (int b = 0; b < 4; ++b) out[4 * k + b] = (uint8_t)(w[k] >> (8 * b));
}
inline void bytes_to_words(const uint8_t in[32], uint32_t w[8]) {
    for (int k = 0; k < 8; ++k)
        w[k] = (uint32_t)in[4 * k] | (uint32_t)in[4 * k + 1] << 8 | (uint32_t)in[4 * k + 2] << 16 |
               (uint32_t)in[4 * k + 3] << 24;
}

// Pieces of one input: every piece but the last holds the same power of two of chunks
// (so each starts at a multiple of it), the last between 1 and that many.
inline bool pieces_ok(const uint64_t* piece_chunks, uint64_t npieces) {
    if (npieces < 2 || !piece_chunks) return false;
    const uint64_t p = piece_chunks[0];
    if (!p || (p & (p - 1))) return false;
    for (uint64_t i = 1; i + 1 < npieces; ++i)
        if (piece_chunks[i] != p) return false;
    return piece_chunks[npieces - 1] >= 1 && piece_chunks[npieces - 1] <= p;
}

// The root hash from the pieces' chaining values, in order (pieces_ok holds): each piece is
// a node of one level of the tree, so the levels above it are reduce_levels over the pieces.
inline void join(const uint8_t* cvs, uint64_t npieces, uint8_t out[32]) {
    uint32_t* w = new uint32_t[8 * npieces];
    for (uint64_t i = 0; i < npieces; ++i) bytes_to_words(cvs + 32 * i, w + 8 * i);
    reduce_levels(w, npieces, true);
    words_to_bytes(w, out);
    delete[] w;
}

}  // namespace b3
}  // namespace sydelta

#if defined(__HIPCC__)
#include "sydelta_internal.hpp"

namespace sydelta {
// One node table per launch (device memory), sorted by start.  A lane of the launch owns
// slot t: the entry with the largest start <= t, node i = t - start of it (idle when
// i >= n).  start is a multiple of min(64, 2^ceil(log2 n)), so the nodes a wave pairs up
// in its six levels sit in one wave at lanes that differ in one bit.
struct B3Seg {
    uint64_t start;  // first slot
    uint64_t n;      // nodes (chunk launch: chunks of the file)
    uint64_t out;    // n <= 64: index of the 32-byte result; else the first slot in the next launch's array
    uint64_t off;    // chunk launch: the file's first byte in the buffer
    uint64_t len;    // chunk launch: the file's length
};
// BLAKE3 of nsegs files of d_buf.  segs[0] (nsegs entries, total0 slots) describes the chunk
// launch (k_b3_chunks: one lane per 1 KiB chunk, then six tree levels in the wave); level j
// of the nlevels following tables (lv_segs[j], lv_nsegs[j] entries, lv_total[j] slots) a
// launch of k_b3_tree over the chaining values the launch before it left in d_cv[(j & 1)].
// Chunk counters start at first_chunk; root = false leaves the top node an ordinary
// chaining value (a piece of a larger input).  Results: d_out + 32 * out.  Nothing here
// waits for the stream.
hipError_t launch_blake3(const uint8_t* d_buf, const B3Seg* segs, uint64_t nsegs, uint64_t total0,
                         const B3Seg* const* lv_segs, const uint64_t* lv_nsegs, const uint64_t* lv_total, int nlevels,
                         uint32_t* const d_cv[2], uint64_t first_chunk, bool root, uint8_t* d_out, hipStream_t s,
                         Profiler* prof);
}  // namespace sydelta
#endif
