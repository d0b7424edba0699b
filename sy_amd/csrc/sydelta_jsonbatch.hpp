// sydelta_jsonbatch.hpp — sydelta_delta_batch_to_json_device (K7b): serde_json::to_string(&Delta)
// (ssh.rs:1003) for a whole batch of deltas in a few launches, the texts packed into one
// arena at 16-byte aligned offsets.
//
// Host: every file's ops are validated and cut into tiles.  A tile is a run of up to
// kCopyTile consecutive Copy ops of one file, or one chunk of at most kChunk literal bytes of
// a Data op; a file's head {"ops":[ rides on its first tile, its tail
// ],"source_size":N,"block_size":B} on its last one, and a file without ops is one tile that
// carries both.  The Copy ops' fields and the tails' two numbers go into a table of pairs.
// Tiles and pairs reach the device in slices (kSliceTiles tiles, kSlicePairs pairs).
// Device: a wave sizes each tile (k_jsonb_len: the digits of a Copy run's fields, or of a
// chunk's literal bytes, on top of the characters the host knows), a scan places the tiles,
// per-file lengths and their 16-rounded scan place the texts, and a workgroup per tile
// composes the tile's text in LDS at the 16-byte phase of its destination and stores it
// with aligned 16-byte stores; the partial granules at a tile's two ends are written byte by
// byte, so neighbouring tiles and texts never race and the pad bytes stay untouched.
//
// The plan (host) and the per-thread bodies (host and device, over a memory policy) are
// shared with tests/csrc/json_batch_check.cpp, which runs them on host memory.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>

#include "../../include/sydelta.h"

#define JSONB_HD __host__ __device__ inline
#if defined(__clang__)
#define JSONB_UNROLL _Pragma("unroll")
#else
#define JSONB_UNROLL
#endif

namespace sydelta {
namespace jsonb {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kCopyTile = 256;        // Copy ops per tile: one per thread
constexpr uint32_t kChunk = 4096;          // literal bytes per Data tile (the single-file writer's kJsonChunk)
constexpr uint32_t kMaxGrid = 1u << 20;    // a workgroup per tile up to here, then grid-strided
constexpr uint32_t kSliceTiles = 8192;     // per slice: 256 KiB of tiles ...
constexpr uint32_t kSlicePairs = 49152;    // ... and 768 KiB of pairs
constexpr uint32_t kRing = 8;              // pinned slices kept per thread: two halves, one filled while one uploads
constexpr uint32_t kHeadLen = 8;           // {"ops":[
constexpr uint32_t kCopySkel = 28;         // {"Copy":{"offset":,"size":}}
constexpr uint32_t kCopyMax = 1 + kCopySkel + 40;  // with its separator and two 20-digit fields
constexpr uint32_t kTailSkel = 31;         // ],"source_size":,"block_size":}
constexpr uint32_t kTailMax = kTailSkel + 40;
// LDS text staging of one tile: up to 15 bytes of phase, the head, the larger of a full Copy
// run and a full chunk (,{"Data":[ + 4 characters per byte + ]}), the tail.
constexpr uint32_t kStage = 17760;
static_assert(kStage % 16 == 0 && kStage >= 15 + kHeadLen + kCopyTile * kCopyMax + kTailMax &&
                  kStage >= 15 + kHeadLen + 1 + 9 + 4 * kChunk + 2 + kTailMax, "a tile's text fits the staging");

constexpr uint32_t kData = 1, kFirst = 2, kLast = 4, kSep = 8, kHead = 16, kTail = 32;
struct Tile {
    uint64_t src;    // Data: the chunk's first byte in d_lit (absolute); Copy: its first pair
    uint64_t tail;   // kTail: the pair {source_size, block_size}
    uint32_t n;      // Copy: ops of the run (0 for a file without ops); Data: bytes of the chunk
    uint32_t flags;  // kData; kFirst / kLast: the op's first / last chunk; kSep: a ',' before
                     // the tile's first op; kHead / kTail: the file's first / last tile
    uint32_t fixed;  // the characters that depend on no digit count of a Copy field or a
                     // literal byte: head, tail, skeletons, separators
    uint32_t file;
};
struct Pair {
    uint64_t a, b;
};
static_assert(sizeof(Tile) == 32 && sizeof(Pair) == 16, "table layout");
constexpr uint64_t kSliceBytes = kSliceTiles * sizeof(Tile) + kSlicePairs * sizeof(Pair);

struct Q16 {
    uint32_t w[4];
};

JSONB_HD uint32_t funnel(uint32_t hi, uint32_t lo, uint32_t r) {  // bytes [r, r + 4) of lo | hi << 32
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, r);
#else
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * r));
#endif
}

JSONB_HD uint32_t dec_digits(uint64_t v) {
    uint32_t n = 1;
    uint64_t p = 10;
    while (v >= p) {
        ++n;
        if (n == 20) break;  // 10^19 <= v: p * 10 would wrap
        p *= 10;
    }
    return n;
}
// Decimal digits of v at p (no terminator); returns their count.
JSONB_HD uint32_t put_dec(uint8_t* p, uint64_t v) {
    const uint32_t n = dec_digits(v);
    uint32_t i = n;
    while (v >> 32) {
        p[--i] = (uint8_t)('0' + v % 10);
        v /= 10;
    }
    uint32_t x = (uint32_t)v;
    while (i > 0) {
        p[--i] = (uint8_t)('0' + x % 10);
        x /= 10;
    }
    return n;
}
JSONB_HD uint32_t put_str(uint8_t* p, const char* s) {
    uint32_t i = 0;
    for (; s[i]; ++i) p[i] = (uint8_t)s[i];
    return i;
}
JSONB_HD uint32_t byte_chars(uint32_t v) { return 2u + (v >= 10) + (v >= 100); }  // digits and a comma

JSONB_HD uint32_t head_len(const Tile& T) {  // what thread 0 writes in front of the threads' texts
    uint32_t h = T.flags & kHead ? kHeadLen : 0u;
    if (T.flags & kData) h += (T.flags & kSep ? 1u : 0u) + (T.flags & kFirst ? 9u : 0u);
    return h;
}

// ---------------------------------------------------------------------------
// Sizing: lane `lane` of the wave that sizes tile T returns its share of the digits; their
// sum over the 64 lanes plus T.fixed is the tile's text length.  Mem: ld16 / ld4 on aligned
// addresses, ldb on bytes (every granule loaded holds at least one byte of the chunk).
// ---------------------------------------------------------------------------
template <class Mem>
JSONB_HD uint32_t size_lane(Mem& m, const Tile& T, const Pair* pairs, uintptr_t lit, uint32_t lane) {
    uint32_t c = 0;
    if (!(T.flags & kData)) {
        static_assert(kCopyTile == 4 * 64, "four ops per lane");
        for (uint32_t i = lane; i < T.n; i += 64) {
            const Pair P = pairs[T.src + i];
            c += dec_digits(P.a) + dec_digits(P.b);
        }
        return c;
    }
    static_assert(kChunk == 64 * 64, "one lane per 64 literal bytes");
    const uint32_t b0 = 64 * lane;
    const uint32_t cnt = b0 < T.n ? (T.n - b0 < 64u ? T.n - b0 : 64u) : 0u;
    const uintptr_t u = lit + T.src + b0;
    if (cnt == 64 && (u & 15) == 0) {
        JSONB_UNROLL
        for (int k = 0; k < 4; ++k) {
            const Q16 v = m.ld16(u + 16 * k);
            JSONB_UNROLL
            for (int j = 0; j < 16; ++j) c += byte_chars((v.w[j >> 2] >> (8 * (j & 3))) & 0xFF) - 1;
        }
    } else if (cnt == 64) {  // unaligned: the 17 dwords holding the 64 bytes
        const uint32_t sh = (uint32_t)(u & 3);
        const uintptr_t q = u & ~(uintptr_t)3;
        uint32_t lo = m.ld4(q);
        JSONB_UNROLL
        for (int k = 0; k < 16; ++k) {
            const uint32_t hi = (k < 15 || sh) ? m.ld4(q + 4 * (k + 1)) : 0u;
            const uint32_t x = funnel(hi, lo, sh);
            JSONB_UNROLL
            for (int j = 0; j < 4; ++j) c += byte_chars((x >> (8 * j)) & 0xFF) - 1;
            lo = hi;
        }
    } else {
        for (uint32_t j = 0; j < cnt; ++j) c += byte_chars(m.ldb(u + j)) - 1;
    }
    return c;
}

// ---------------------------------------------------------------------------
// Writing, per thread of the tile's workgroup of kThreads:
//   1. thread_len: what the thread will write (its Copy op with its separator, or its 16
//      literal bytes each with a comma), loaded into `th`;
//   2. an exclusive scan over the workgroup gives `pre`, and the sum `body`;
//   3. thread_format writes the thread's text into the staging (thread 0 the head too);
//   4. after a barrier thread 0 closes the tile (tile_close: ]} and the tail);
//   5. after a barrier thread_store moves the staging to d_out.
// Staging byte k stands for the byte at (address of the tile's first character & ~15) + k.
// ---------------------------------------------------------------------------
struct Thread {
    uint32_t w[4];  // Data: the thread's literal bytes
    Pair p;         // Copy: the thread's op
    uint32_t cnt;   // Data: how many of the 16 bytes exist; Copy: 1 when the thread has an op
};

template <class Mem>
JSONB_HD uint32_t thread_len(Mem& m, const Tile& T, const Pair* pairs, uintptr_t lit, uint32_t tid, Thread& th) {
    th.w[0] = th.w[1] = th.w[2] = th.w[3] = 0;
    th.p = Pair{0, 0};
    if (!(T.flags & kData)) {
        th.cnt = tid < T.n ? 1u : 0u;
        if (!th.cnt) return 0;
        th.p = pairs[T.src + tid];
        return ((tid || (T.flags & kSep)) ? 1u : 0u) + kCopySkel + dec_digits(th.p.a) + dec_digits(th.p.b);
    }
    static_assert(kChunk == 16 * kThreads, "one thread per 16 literal bytes");
    const uint32_t b0 = 16 * tid;
    th.cnt = b0 < T.n ? (T.n - b0 < 16u ? T.n - b0 : 16u) : 0u;
    const uintptr_t u = lit + T.src + b0;
    if (th.cnt == 16) {
        if ((u & 15) == 0) {
            const Q16 v = m.ld16(u);
            th.w[0] = v.w[0], th.w[1] = v.w[1], th.w[2] = v.w[2], th.w[3] = v.w[3];
        } else {  // the dwords holding the 16 bytes (never past the granule of a byte of the chunk)
            const uint32_t sh = (uint32_t)(u & 3);
            const uintptr_t q = u & ~(uintptr_t)3;
            const uint32_t d0 = m.ld4(q), d1 = m.ld4(q + 4), d2 = m.ld4(q + 8), d3 = m.ld4(q + 12);
            const uint32_t d4 = sh ? m.ld4(q + 16) : 0u;
            th.w[0] = funnel(d1, d0, sh), th.w[1] = funnel(d2, d1, sh);
            th.w[2] = funnel(d3, d2, sh), th.w[3] = funnel(d4, d3, sh);
        }
    } else {
        JSONB_UNROLL
        for (uint32_t j = 0; j < 16; ++j)
            if (j < th.cnt) th.w[j >> 2] |= (uint32_t)m.ldb(u + j) << (8 * (j & 3));
    }
    uint32_t mine = 0;
    JSONB_UNROLL
    for (uint32_t j = 0; j < 16; ++j)
        mine += j < th.cnt ? byte_chars((th.w[j >> 2] >> (8 * (j & 3))) & 0xFF) : 0u;
    return mine;
}

JSONB_HD void thread_format(uint8_t* js, const Tile& T, uint32_t ph, uint32_t pre, uint32_t tid, const Thread& th) {
    if (tid == 0) {
        uint32_t k = ph;
        if (T.flags & kHead) k += put_str(js + k, "{\"ops\":[");
        if (T.flags & kData) {
            if (T.flags & kSep) js[k++] = ',';
            if (T.flags & kFirst) k += put_str(js + k, "{\"Data\":[");
        }
    }
    uint32_t k = ph + head_len(T) + pre;
    if (!(T.flags & kData)) {
        if (!th.cnt) return;
        if (tid || (T.flags & kSep)) js[k++] = ',';
        k += put_str(js + k, "{\"Copy\":{\"offset\":");
        k += put_dec(js + k, th.p.a);
        k += put_str(js + k, ",\"size\":");
        k += put_dec(js + k, th.p.b);
        js[k] = '}';
        js[k + 1] = '}';
        return;
    }
    JSONB_UNROLL
    for (uint32_t j = 0; j < 16; ++j) {
        const uint32_t v = (th.w[j >> 2] >> (8 * (j & 3))) & 0xFF;
        const uint32_t h = v / 100, t = (v / 10) % 10, o = v % 10;
        const uint32_t nd = 1 + (v >= 10) + (v >= 100);
        // characters: [h] [t] o ','  (leading digits only when present)
        const uint32_t c0 = nd == 3 ? '0' + h : (nd == 2 ? '0' + t : '0' + o);
        const uint32_t c1 = nd == 3 ? '0' + t : (nd == 2 ? '0' + o : ',');
        const uint32_t c2 = nd == 3 ? '0' + o : ',';
        if (j < th.cnt) {
            js[k] = (uint8_t)c0;
            js[k + 1] = (uint8_t)c1;
            if (nd >= 2) js[k + 2] = (uint8_t)c2;
            if (nd == 3) js[k + 3] = ',';
            k += nd + 1;
        }
    }
}

// Thread 0, after every thread's text is in the staging: the op's ]} over the comma of its
// last byte, then the file's tail.  Returns the staging's end (ph + the tile's text length).
JSONB_HD uint32_t tile_close(uint8_t* js, const Tile& T, const Pair* pairs, uint32_t ph, uint32_t body) {
    uint32_t k = ph + head_len(T) + body;
    if (T.flags & kData) {
        if ((T.flags & kLast) && T.n) k -= 1;  // no comma after the op's last byte
        if (T.flags & kLast) {
            js[k] = ']';
            js[k + 1] = '}';
            k += 2;
        }
    }
    if (T.flags & kTail) {
        const Pair P = pairs[T.tail];
        k += put_str(js + k, "],\"source_size\":");
        k += put_dec(js + k, P.a);
        k += put_str(js + k, ",\"block_size\":");
        k += put_dec(js + k, P.b);
        js[k++] = '}';
    }
    return k;
}

// Staging [ph, end) -> [g + ph, g + end), g 16-byte aligned: whole granules with st16, the
// partial ones at the two ends byte by byte.
template <class Mem>
JSONB_HD void thread_store(Mem& m, const uint8_t* js, uint32_t ph, uint32_t end, uintptr_t g, uint32_t tid,
                           uint32_t nthr) {
    for (uint32_t c = 16 * tid; c < end; c += 16 * nthr) {
        if (c >= ph && c + 16 <= end) {
            m.st16(g + c, js + c);
        } else {
            const uint32_t lo = c > ph ? c : ph, hi = c + 16 < end ? c + 16 : end;
            for (uint32_t x = lo; x < hi; ++x) m.stb(g + x, js[x]);
        }
    }
}

// ---------------------------------------------------------------------------
// The host plan
// ---------------------------------------------------------------------------
struct FileIn {
    const sydelta_op* ops;  // nullptr with nops == 0 is a delta without ops
    uint64_t nops;
    bool has_delta;         // false: deltas[f] was NULL
    uint64_t source_size, block_size, lit_off, lit_len;
};
struct Err {
    int code = SYDELTA_OK;
    std::string msg;
};

inline int plan_fail(Err* e, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
inline int plan_fail(Err* e, int code, const char* fmt, ...) {
    char buf[320];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    e->code = code;
    e->msg = buf;
    return code;
}

inline uint32_t tail_len(uint64_t source_size, uint64_t block_size) {
    return kTailSkel + dec_digits(source_size) + dec_digits(block_size);
}

// Bounds of one delta's text from its ops alone: a literal byte is 1 to 3 digits.  False on
// an unknown op kind or when the upper bound does not fit 64 bits.
inline bool text_bounds(const sydelta_op* ops, uint64_t nops, uint64_t source_size, uint64_t block_size, uint64_t* lo,
                        uint64_t* hi) {
    uint64_t l = kHeadLen + tail_len(source_size, block_size), h = l;
    for (uint64_t i = 0; i < nops; ++i) {
        const sydelta_op& o = ops[i];
        uint64_t ol, oh;
        if (o.kind == SYDELTA_OP_COPY) {
            ol = oh = kCopySkel + dec_digits(o.a) + dec_digits(o.b);
        } else if (o.kind == SYDELTA_OP_DATA) {
            if (o.b > (UINT64_MAX >> 3)) return false;
            ol = 11 + (o.b ? 2 * o.b - 1 : 0);  // {"Data":[]} and the commas
            oh = 11 + (o.b ? 4 * o.b - 1 : 0);
        } else {
            return false;
        }
        l += ol + (i ? 1 : 0);  // l <= h
        if (__builtin_add_overflow(h, oh + (i ? 1 : 0), &h)) return false;
    }
    *lo = l;
    *hi = h;
    return true;
}

struct Count {
    uint64_t tiles = 0, pairs = 0;
    uint64_t lo = 0, hi = 0;  // bounds of the text from the ops alone (hi saturates)
};
// Validate file f (its literal range, then every op, overflow-checked); *c receives its tiles,
// its pairs and loose bounds of its text (a Copy field is 1 to 20 digits, a literal byte 1 to
// 3), *literal grows by its Data ops' bytes.
inline int count_file(uint64_t f, const FileIn& in, uint64_t lit_arena, Count* c, uint64_t* literal, Err* e) {
    typedef unsigned long long ull;
    if (in.lit_len > lit_arena || in.lit_off > lit_arena - in.lit_len)
        return plan_fail(e, SYDELTA_E_INVAL, "file %llu: literal range [%llu, +%llu) leaves its arena of %llu bytes", (ull)f,
                         (ull)in.lit_off, (ull)in.lit_len, (ull)lit_arena);
    if (!in.has_delta) return plan_fail(e, SYDELTA_E_INVAL, "file %llu: NULL delta", (ull)f);
    uint64_t tiles = 0, run = 0, copies = 0, bytes = 0;
    for (uint64_t i = 0; i < in.nops; ++i) {
        const sydelta_op& o = in.ops[i];
        if (o.kind == SYDELTA_OP_COPY) {
            if (run++ % kCopyTile == 0) ++tiles;
            ++copies;
            continue;
        }
        run = 0;
        if (o.kind != SYDELTA_OP_DATA)
            return plan_fail(e, SYDELTA_E_INVAL, "file %llu: op %llu: unknown kind %u", (ull)f, (ull)i, (unsigned)o.kind);
        if (o.a > in.lit_len || o.b > in.lit_len - o.a)
            return plan_fail(e, SYDELTA_E_INVAL, "file %llu: op %llu: Data [%llu, +%llu) outside the literal range "
                             "(%llu bytes)", (ull)f, (ull)i, (ull)o.a, (ull)o.b, (ull)in.lit_len);
        tiles += o.b ? (o.b + kChunk - 1) / kChunk : 1;
        if (__builtin_add_overflow(bytes, o.b, &bytes)) bytes = UINT64_MAX;  // ops may overlap: a count, not a size
    }
    c->tiles = in.nops ? tiles : 1;
    c->pairs = copies + 1;  // a pair per Copy op and the tail's
    // head, tail and per op its separator and skeleton; digits and commas on top
    const uint64_t nd = in.nops - copies, skel = kHeadLen + tail_len(in.source_size, in.block_size) +
                                                 (in.nops ? in.nops - 1 : 0) + copies * kCopySkel + nd * 11;
    c->lo = skel + copies * 2 + (bytes >= nd ? 2 * bytes - nd : 0);  // a Data op of b bytes: 2b - 1, or 0
    c->hi = bytes > (UINT64_MAX >> 3) ? UINT64_MAX : skel + copies * 40 + 4 * bytes;
    if (c->lo > c->hi) c->lo = 0;  // a saturated byte count
    if (__builtin_add_overflow(*literal, bytes, literal)) *literal = UINT64_MAX;
    return SYDELTA_OK;
}

// The slices are cut from the files in order; a tile never straddles two, and a file that
// fits a slice never does either (it starts a new slice when the current one has no room for
// all of it), so where the slices start follows from the files' counts alone, without a
// second look at the ops, except inside a file larger than a slice.
struct Cursor {
    uint64_t file = 0, op = 0, chunk = 0;
};
struct Slice {
    uint32_t ntiles = 0, npairs = 0;
};
// The tile at c (the cursor moves past it): its pairs go to po from *npairs on, their indices
// counted from pair_base (po nullptr: counted only).
inline Tile next_tile(const FileIn* files, Cursor& c, uint64_t pair_base, Pair* po, uint32_t* npairs) {
    const FileIn& F = files[c.file];
    Tile T{};
    T.file = (uint32_t)c.file;
    if (c.op == 0 && c.chunk == 0) T.flags |= kHead, T.fixed += kHeadLen;
    bool last;  // the file's last tile
    if (!F.nops) {
        last = true;
    } else if (F.ops[c.op].kind == SYDELTA_OP_COPY) {
        if (c.op) T.flags |= kSep;
        T.src = pair_base + *npairs;
        while (T.n < kCopyTile && c.op < F.nops && F.ops[c.op].kind == SYDELTA_OP_COPY) {
            if (po) po[*npairs] = Pair{F.ops[c.op].a, F.ops[c.op].b};
            ++*npairs, ++T.n, ++c.op;
        }
        T.fixed += T.n * (kCopySkel + 1) - (T.flags & kSep ? 0 : 1);
        last = c.op == F.nops;
    } else {
        const sydelta_op& o = F.ops[c.op];
        const uint64_t nch = o.b ? (o.b + kChunk - 1) / kChunk : 1, at = c.chunk * kChunk;
        T.flags |= kData;
        T.src = F.lit_off + o.a + at;
        T.n = (uint32_t)(o.b - at < kChunk ? o.b - at : kChunk);
        if (c.chunk == 0) {
            T.flags |= kFirst, T.fixed += 9;                  // {"Data":[
            if (c.op) T.flags |= kSep, T.fixed += 1;
        }
        const bool end = c.chunk + 1 == nch;
        if (end) T.flags |= kLast, T.fixed += 2;              // ]}
        T.fixed += T.n ? T.n - (end ? 1 : 0) : 0;             // the commas, the one before the next chunk included
        if (end) ++c.op, c.chunk = 0; else ++c.chunk;
        last = end && c.op == F.nops;
    }
    if (last) {
        T.flags |= kTail;
        T.fixed += tail_len(F.source_size, F.block_size);
        T.tail = pair_base + *npairs;
        if (po) po[*npairs] = Pair{F.source_size, F.block_size};
        ++*npairs;
        ++c.file, c.op = 0, c.chunk = 0;
    }
    return T;
}
// The next slice from c on: to[kSliceTiles] / po[kSlicePairs] filled (both nullptr: counted
// only, whole files from fc without a look at their ops), the tiles' pair indices counted
// from pair_base (the pairs of the slices before).  False when nothing is left.  fc: the
// files' counts from count_file.
inline bool next_slice(const FileIn* files, const Count* fc, uint64_t nfiles, Cursor& c, uint64_t pair_base, Tile* to,
                       Pair* po, Slice* sl) {
    *sl = Slice();
    // a tile needs room for a full Copy run and a tail
    while (c.file < nfiles && sl->ntiles < kSliceTiles && kSlicePairs - sl->npairs > kCopyTile) {
        if (c.op == 0 && c.chunk == 0) {
            const Count& F = fc[c.file];
            const bool fits = F.tiles <= kSliceTiles - sl->ntiles && F.pairs + kCopyTile <= kSlicePairs - sl->npairs;
            if (!fits && sl->ntiles) break;  // the file starts the next slice
            if (fits && !to) {
                sl->ntiles += (uint32_t)F.tiles, sl->npairs += (uint32_t)F.pairs;
                ++c.file;
                continue;
            }
        }
        const Tile T = next_tile(files, c, pair_base, po, &sl->npairs);
        if (to) to[sl->ntiles] = T;
        ++sl->ntiles;
    }
    return sl->ntiles > 0;
}

}  // namespace jsonb

struct Profiler;
// Tiles [t0, t0 + nt) sized (k_jsonb_len): d_len[t] = the tile's text length.
hipError_t launch_jsonb_len(const jsonb::Tile* d_tiles, const jsonb::Pair* d_pairs, uint64_t t0, uint64_t nt,
                            const uint8_t* d_lit, uint64_t* d_len, hipStream_t s, Profiler* prof);
// With d_off the exclusive scan of d_len: d_fstart[f] = where file f's first tile starts,
// d_fstart[nfiles] = the end of the last tile (k_jsonb_files); then d_tlen[f] = file f's
// text length and d_pad[f] the same rounded up to 16 (k_jsonb_flen).
hipError_t launch_jsonb_files(const jsonb::Tile* d_tiles, const uint64_t* d_off, const uint64_t* d_len, uint64_t ntiles,
                              uint64_t nfiles, uint64_t* d_fstart, uint64_t* d_tlen, uint64_t* d_pad, hipStream_t s,
                              Profiler* prof);
// With d_toff the exclusive scan of d_pad: every tile's text at d_out + d_toff[file] + (d_off[t]
// - d_fstart[file]), when d_toff[nfiles - 1] + d_tlen[nfiles - 1] <= out_cap (decided on the
// device); nothing is written otherwise.
hipError_t launch_jsonb_write(const jsonb::Tile* d_tiles, const jsonb::Pair* d_pairs, uint64_t ntiles,
                              const uint8_t* d_lit, const uint64_t* d_off, const uint64_t* d_len,
                              const uint64_t* d_fstart, const uint64_t* d_toff, const uint64_t* d_tlen, uint64_t nfiles,
                              uint8_t* d_out, uint64_t out_cap, hipStream_t s, Profiler* prof);

}  // namespace sydelta
