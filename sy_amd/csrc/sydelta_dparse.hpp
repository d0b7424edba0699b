// sydelta_dparse.hpp — K7d: the receiver's parse of the Delta JSON on the device,
// `serde_json::from_str::<Delta>` (sy-remote.rs:175) for text in the compact form the
// sender writes (serde_json::to_string, ssh.rs:1003; sydelta_delta_to_json_device):
//
//   {"ops":[{"Copy":{"offset":O,"size":S}},{"Data":[b0,b1,...]},...],"source_size":N,"block_size":B}
//
// The head (`{"ops":[`) and the tail (`],"source_size":N,"block_size":B}`) are checked on
// the host; the device parses the ops region R = [8, E) between them.  In the compact
// form, inside R:
//   * an op starts at each '{' at 8 or right after "},";
//   * a literal byte starts at each digit right after '[' or ',' (the Copy fields' digits
//     follow ':'), so literal k of the delta is the k-th such digit;
// so one thread per 64-byte chunk counts both, two exclusive scans rank them, the op
// starts are placed by rank, and then each thread parses the ops and literal bytes that
// start in its chunk: a Copy op whole, a Data op's head (its literal range is the count
// of literal starts between its '{' and the next op's), each literal byte with the
// character after it (',' + digit, or "]}" + the next op / the end).  The ops and the
// literals between them then chain from 8 to E, so every byte of R is checked by some
// thread.  Any other spelling is refused with its first byte; the host parser
// (sydelta_delta_from_json) takes those.
//
// Every function below is the body of one thread (sydelta_kernels.hip); the host
// emulation of the device layer (tests/csrc/fake_device.cpp) and the sanitizer build
// (tests/csrc/kernel_bodies_fuzz.cpp) run the same bodies on the CPU.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sydelta.h"
#include "sydelta_sigjson.hpp"  // get_dec, get_lit

namespace sydelta {
namespace dparse {

constexpr uint32_t kChunk = 64;   // text bytes per thread
constexpr uint64_t kHead = 8;     // {"ops":[
constexpr uint64_t kNoBad = UINT64_MAX;

struct DArgs {
    const uint8_t* t;  // the whole text
    uint64_t e;        // end of the ops region (its ']')
    uint64_t nc;       // chunks of [kHead, e)
    // The literal rank of the text's first literal.  0 for a text parsed alone; in a batch
    // (sydelta_dparsebatch.hpp) the ranks run through all files, and a Data op's a = its
    // rank - lbase indexes the file's own literal range.
    uint64_t lbase = 0;
};

__host__ __device__ __forceinline__ bool is_digit(uint8_t c) { return c >= '0' && c <= '9'; }
// T: the text as a byte pointer, or any type with operator[](uint64_t) -> uint8_t (the
// kernels read their wave's tile from LDS, LdsText in sydelta_kernels.hip)
template <class T>
__host__ __device__ __forceinline__ bool op_start(const T& t, uint64_t p) {
    return t[p] == '{' && (p == kHead || (t[p - 1] == ',' && t[p - 2] == '}'));
}
template <class T>
__host__ __device__ __forceinline__ bool lit_start(const T& t, uint64_t p) {
    return is_digit(t[p]) && (t[p - 1] == '[' || t[p - 1] == ',');
}
__host__ __device__ __forceinline__ uint64_t chunk_lo(const DArgs& a, uint64_t c) { return kHead + c * kChunk; }
__host__ __device__ __forceinline__ uint64_t chunk_hi(const DArgs& a, uint64_t c) {
    const uint64_t h = kHead + (c + 1) * kChunk;
    return h < a.e ? h : a.e;
}

// Op starts and literal starts in chunk c.
template <class T>
__host__ __device__ inline void chunk_count(const DArgs& a, const T& t, uint64_t c, uint64_t& nops, uint64_t& nlit) {
    nops = nlit = 0;
    for (uint64_t p = chunk_lo(a, c); p < chunk_hi(a, c); ++p) {
        nops += op_start(t, p);
        nlit += lit_start(t, p);
    }
}
__host__ __device__ inline void chunk_count(const DArgs& a, uint64_t c, uint64_t& nops, uint64_t& nlit) {
    chunk_count(a, a.t, c, nops, nlit);
}

// Position of every op start of chunk c, by rank.
template <class T>
__host__ __device__ inline void chunk_place(const DArgs& a, const T& t, uint64_t c, uint64_t rank, uint64_t* pos) {
    for (uint64_t p = chunk_lo(a, c); p < chunk_hi(a, c); ++p)
        if (op_start(t, p)) pos[rank++] = p;
}
__host__ __device__ inline void chunk_place(const DArgs& a, uint64_t c, uint64_t rank, uint64_t* pos) {
    chunk_place(a, a.t, c, rank, pos);
}

// Literal starts before position x (kHead <= x <= e): the chunk's rank plus a recount.
template <class T>
__host__ __device__ inline uint64_t lits_before(const DArgs& a, const T& t, const uint64_t* lrank, uint64_t x) {
    if (x >= a.e) return lrank[a.nc];  // lrank holds nc + 1 entries: the total last
    const uint64_t c = (x - kHead) / kChunk;
    uint64_t r = lrank[c];
    for (uint64_t p = chunk_lo(a, c); p < x; ++p) r += lit_start(t, p);
    return r;
}

// What may follow an op ending at q: ',' and the next op's '{', or the region's end.
template <class T>
__host__ __device__ __forceinline__ bool op_follow(const DArgs& a, const T& t, uint64_t q) {
    return q == a.e || (q + 1 < a.e && t[q] == ',' && t[q + 1] == '{');
}

// Chunk c's ops and literal bytes.  orank/lrank: exclusive scans (lrank with the total
// at nc), pos: op starts by rank (nops: the rank behind the text's last op).  Writes
// ops[rank] (kind, a = literal offset (rank - a.lbase) or basis offset, b = size) and
// lit[rank] (lit NULL: checked only; L: a byte
// pointer, or a type with operator bool and operator[](uint64_t) -> uint8_t&, the kernel's
// LDS staging).  Returns the first bad position in the chunk or kNoBad.
template <class T, class L = uint8_t*>
__host__ __device__ inline uint64_t chunk_parse(const DArgs& a, const T& t, uint64_t c, const uint64_t* orank,
                                               const uint64_t* lrank, const uint64_t* pos, uint64_t nops,
                                               sydelta_op* ops, L lit) {
    const uint64_t len = a.e;  // no token of R reads past its ']'
    uint64_t ork = orank[c], lrk = lrank[c];
    // The chain starts at the first op: a non-empty region must open with one, or the
    // bytes before the first "},{" would be checked by no thread.
    if (c == 0 && a.e > kHead && !op_start(t, kHead)) return kHead;
    for (uint64_t p = chunk_lo(a, c); p < chunk_hi(a, c); ++p) {
        if (op_start(t, p)) {
            uint64_t q = p, o = 0, sz = 0;
            uint32_t k;
            sydelta_op op{};
            if (sigjson::get_lit(t, len, q, "{\"Copy\":{\"offset\":")) {
                if (!(k = sigjson::get_dec(t, len, q, UINT64_MAX, o))) return p;
                q += k;
                if (!sigjson::get_lit(t, len, q, ",\"size\":") || !(k = sigjson::get_dec(t, len, q, UINT64_MAX, sz)))
                    return p;
                q += k;
                if (!sigjson::get_lit(t, len, q, "}}") || !op_follow(a, t, q)) return p;
                op.kind = SYDELTA_OP_COPY;
                op.a = o;
                op.b = sz;
            } else {
                q = p;
                if (!sigjson::get_lit(t, len, q, "{\"Data\":[")) return p;
                if (q < len && t[q] == ']') {  // empty Data
                    ++q;
                    if (!sigjson::get_lit(t, len, q, "}") || !op_follow(a, t, q)) return p;
                } else if (!(q < len && is_digit(t[q]))) {
                    return p;  // the first literal (checked by its own thread) must start here
                }
                // the recounts reach other chunks' text (the next op may be anywhere): a.t
                const uint64_t l0 = lits_before(a, a.t, lrank, q);
                const uint64_t next = ork + 1 < nops ? pos[ork + 1] : a.e;
                op.kind = SYDELTA_OP_DATA;
                op.a = l0 - a.lbase;
                op.b = lits_before(a, a.t, lrank, next) - l0;
            }
            ops[ork++] = op;
        } else if (lit_start(t, p)) {
            uint64_t v = 0;
            const uint32_t k = sigjson::get_dec(t, len, p, 255, v);
            if (!k) return p;
            uint64_t q = p + k;
            if (q < len && t[q] == ',') {
                if (!(q + 1 < len && is_digit(t[q + 1]))) return p;
            } else {
                if (!sigjson::get_lit(t, len, q, "]}") || !op_follow(a, t, q)) return p;
            }
            if (lit) lit[lrk] = (uint8_t)v;
            ++lrk;
        }
    }
    return kNoBad;
}
__host__ __device__ inline uint64_t chunk_parse(const DArgs& a, uint64_t c, const uint64_t* orank,
                                               const uint64_t* lrank, const uint64_t* pos, uint64_t nops,
                                               sydelta_op* ops, uint8_t* lit) {
    return chunk_parse<const uint8_t*, uint8_t*>(a, a.t, c, orank, lrank, pos, nops, ops, lit);
}

// ---------------------------------------------------------------------------
// The wave form of the three kernels (k_dparse_count / _place / k_dparse): a wave takes
// 64 consecutive chunks, stages their text in LDS rows, classifies the chunks of a
// literal run with SWAR masks instead of the bodies above, and stores its literal bytes
// from an LDS slab with whole dwords.  The arithmetic of that form is below, so that the
// CPU suite runs it too (tests/csrc/dparse_wave.hpp: the emulated device and the
// sanitizer build); the LDS accesses themselves stay in sydelta_kernels.hip.
// ---------------------------------------------------------------------------
constexpr uint32_t kDpRow = 68;                          // LDS bytes per staged 64-byte row
constexpr uint32_t kDpBefore = 8;                        // bytes staged before the wave's first chunk
constexpr uint32_t kDpSpan = 64 * 64 + kDpBefore + 136;  // staged bytes per wave
constexpr uint32_t kDpRows = (kDpSpan + 63) / 64;
constexpr uint32_t kDpLitMax = 64 * (kChunk / 2);        // a 64-byte chunk starts at most 32 literals

// Byte d of the staged span in the row array (64-byte rows padded to kDpRow).
template <class I>
__host__ __device__ __forceinline__ I stage_off(I d) { return (d >> 6) * kDpRow + (d & 63); }
// The span of the wave whose first chunk is c0: text [p0, p0 + n).
__host__ __device__ __forceinline__ uint64_t stage_p0(const DArgs& a, uint64_t c0) {
    return chunk_lo(a, c0) - kDpBefore;  // >= 0: chunk 0 starts at kHead = 8
}
__host__ __device__ __forceinline__ uint32_t stage_len(const DArgs& a, uint64_t p0) {
    const uint64_t hi = p0 + kDpSpan < a.e ? p0 + kDpSpan : a.e;
    return (uint32_t)(hi - p0);
}

// The fast path: a chunk of 64 digits and commas (inside a Data op's literal run: almost
// all of a literal-heavy delta's text) is classified from 18 dwords, its 64 bytes and 8
// bytes of look-ahead.  fast_chunk: chunk c may take it (not the first chunk, not within
// 72 bytes of the region's end or of the staged span's); d0 = its offset in the span
// (8 + 64 * lane: dword-aligned, each dword inside one row).
__host__ __device__ __forceinline__ bool fast_chunk(const DArgs& a, uint64_t c, uint64_t p0, uint64_t n, uint32_t& d0) {
    const uint64_t lo = chunk_lo(a, c);
    if (c == 0 || lo + 72 > a.e) return false;  // the first chunk, the tail: the bodies
    d0 = (uint32_t)(lo - p0);
    return !(d0 + 72 > n);
}
__host__ __device__ __forceinline__ uint32_t fast_bits4(uint32_t m) {  // bit 7 of each byte -> bits 0..3
    return ((m >> 7) & 1u) | ((m >> 14) & 2u) | ((m >> 21) & 4u) | ((m >> 28) & 8u);
}
__host__ __device__ __forceinline__ uint32_t fast_digits4(uint32_t x) {
    const uint32_t t = x ^ 0x30303030u;
    return fast_bits4(~(((t & 0x7F7F7F7Fu) + 0x76767676u) | t) & 0x80808080u);
}
__host__ __device__ __forceinline__ uint32_t fast_eq4(uint32_t x, uint32_t pat) {
    const uint32_t y = x ^ pat;
    return fast_bits4(~(((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y) & 0x80808080u);
}
// x[18]: the chunk's dwords and two of look-ahead; pb: the byte before the chunk.  True:
// the chunk is digits and commas only and every literal starting in it (bit i of lits: at
// byte i) is 1-3 digits followed by ',' and a digit, so chunk_count / chunk_parse would
// find exactly these literals and nothing else (their values: fast_values); any other
// chunk (ops, the end of a run, a bad byte) takes the bodies.
__host__ __device__ __forceinline__ bool fast_classify(const uint32_t* x, uint32_t pb, uint64_t& lits) {
    uint64_t D = 0, C = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        D |= (uint64_t)fast_digits4(x[k]) << (4 * k);
        C |= (uint64_t)fast_eq4(x[k], 0x2C2C2C2Cu) << (4 * k);
    }
    if ((D | C) != ~0ull) return false;
    const uint32_t DL = fast_digits4(x[16]) | (fast_digits4(x[17]) << 4);  // look-ahead bytes 64..71
    const uint32_t CL = fast_eq4(x[16], 0x2C2C2C2Cu) | (fast_eq4(x[17], 0x2C2C2C2Cu) << 4);
    const uint64_t L = D & ((C << 1) | (uint64_t)(pb == ',' || pb == '['));
    // digits / commas at i+1, i+2, i+3 (with the look-ahead)
    const uint64_t D1 = (D >> 1) | ((uint64_t)DL << 63), D2 = (D >> 2) | ((uint64_t)DL << 62),
                   D3 = (D >> 3) | ((uint64_t)DL << 61), D4 = (D >> 4) | ((uint64_t)DL << 60);
    const uint64_t C1 = (C >> 1) | ((uint64_t)CL << 63), C2 = (C >> 2) | ((uint64_t)CL << 62),
                   C3 = (C >> 3) | ((uint64_t)CL << 61);
    // 1 digit: ',' then a digit; 2: digit, ',', digit; 3: digit, digit, ',', digit; 4+: bad
    const uint64_t len1 = ~D1, len2 = D1 & ~D2, len3 = D1 & D2 & ~D3;
    const uint64_t follow = (len1 & C1 & D2) | (len2 & C2 & D3) | (len3 & C3 & D4);
    if (L & ~follow) return false;
    lits = L;
    return true;
}
// Byte i of the fast chunk (constant i after unrolling).
__host__ __device__ __forceinline__ uint32_t fast_byte(const uint32_t* x, int i) {
    return (x[i >> 2] >> (8 * (i & 3))) & 0xFFu;
}
// The values of a classified chunk's literals: put(rank, value) for each, the ranks from
// r0 (the chunk's) by popcount.  False: a leading zero or a value > 255, which sends the
// chunk to the body (what was put before is written again, or the text is refused).
template <class Put>
__host__ __device__ __forceinline__ bool fast_values(const uint32_t* x, uint64_t lits, uint64_t r0, Put put) {
    bool good = true;
#pragma unroll
    for (int i = 0; i < 64; ++i) {
        if (!((lits >> i) & 1)) continue;
        const uint32_t b0 = fast_byte(x, i) - '0', b1 = fast_byte(x, i + 1) - '0', b2 = fast_byte(x, i + 2) - '0';
        const bool two = b1 < 10, three = two && b2 < 10;
        const uint32_t v = three ? b0 * 100 + b1 * 10 + b2 : two ? b0 * 10 + b1 : b0;
        good &= v <= 255 && !(two && b0 == 0);
        put(r0 + (uint64_t)__builtin_popcountll(lits & ((1ull << i) - 1)), v);
    }
    return good;
}
// The wave's literal range [l0, l1) of an output whose address has phase ph (address &
// 3): bytes [l0, a0) up to a dword boundary of the absolute address, whole dwords [a0, a1),
// bytes [a1, l1).  a0 >= a1: no whole dword, the range goes byte by byte.
__host__ __device__ __forceinline__ void lit_split(uint64_t l0, uint64_t l1, uint32_t phase, uint64_t& a0, uint64_t& a1) {
    const int64_t ph = (int64_t)phase;
    a0 = (uint64_t)((((int64_t)l0 + ph + 3) & ~3ll) - ph);
    const int64_t a1s = (((int64_t)l1 + ph) & ~3ll) - ph;
    a1 = a1s < (int64_t)a0 ? a0 : (uint64_t)a1s;
}

}  // namespace dparse
}  // namespace sydelta
