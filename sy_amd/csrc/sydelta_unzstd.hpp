// sydelta_unzstd.hpp — per-thread bodies of the zstd frame decoder (RFC 8878; K7u), the
// inverse of sydelta_zstd.hpp for any writer's frames: what sy-remote.rs:160-166 does
// with compress::decompress before it parses the Delta JSON.  The kernels of
// sydelta_unzstd.hip call these bodies; tests/csrc/unzstd_check.cpp drives the same
// bodies on the CPU, thread by thread, under the sanitizers.
//
// Stages: scan (frame header, Block_Header chain, section headers, table
// provenance, scratch prefix sums) -> tables (Huffman / FSE decode tables a block
// defines) -> decode (literal streams, sequences with a symbolic repeat-offset history)
// -> stitch (entry histories, output positions, the regenerated size) -> resolve
// (offsets made concrete and checked) -> place (literal bytes and the parent array) ->
// pointer doubling -> gather.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sydelta_zstd.hpp"  // kLLBase / kLLBits / kMLBase / kMLBits, highbit32

namespace sydelta {
namespace unz {

#define UNZ_HD __host__ __device__ inline

constexpr uint32_t kBlockMax = 128u << 10;
constexpr uint32_t kMaxSeq = kBlockMax / 3;  // a match has at least 3 bytes
constexpr uint32_t kHufLogMax = 12;          // libzstd reads trees up to 12 bits (the RFC writes 11)
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint64_t kNoErr = ~0ull;           // status word: (block << 32) | Err, the lowest wins

enum Err : uint32_t {
    kOk = 0,
    kMagic,      // not a zstd frame
    kTrunc,      // the frame ends early
    kReserved,   // reserved Frame_Header_Descriptor bit
    kDict,       // non-zero Dictionary_ID
    kChecksum,   // Content_Checksum flag
    kWindow,     // window above 2^31
    kTrailing,   // bytes behind the last block
    kBlockType,  // reserved block type 3
    kBlockBig,   // a block regenerating more than 128 KiB
    kBlockSize,  // a Compressed block of less than 3 or at least 128 Ki bytes
    kLitHeader,  // literals section header
    kHufDesc,    // Huffman tree description
    kFseDesc,    // FSE table description
    kNoPrev,     // Treeless / Repeat_Mode without a predecessor
    kLitStream,  // a literal stream does not end where its symbols do
    kSeqHeader,  // sequences section header
    kSeqStream,  // the sequence bitstream does not end where its sequences do
    kLitOver,    // more literals consumed than present
    kOffset,     // an offset reaching before the start of the output
    kFcs,        // Frame_Content_Size differs from the regenerated size
    kTooBig,     // 4 GiB or more of output
    kErrCount
};

UNZ_HD uint64_t ekey(uint64_t block, uint32_t e) { return block << 32 | e; }

struct Block {
    uint64_t off;       // the block's content in the frame
    uint64_t lit_off;   // literals payload (behind the literals section header)
    uint64_t seq_off;   // first byte behind the modes byte
    uint64_t lit_base;  // the block's literals in the literal scratch
    uint64_t seq_base;  // the block's sequences in the sequence scratch
    uint32_t type;      // 0 Raw, 1 RLE, 2 Compressed
    uint32_t size;      // content bytes in the frame (RLE: 1)
    uint32_t regen;     // regenerated size (Compressed: set by the decode stage)
    uint32_t lit_type, lit_regen, lit_csize, lit_streams;
    uint32_t nseq, modes;
    uint32_t huf_slot;     // Huffman table to use (its own or a predecessor's)
    uint32_t fse_slot[3];  // LL, OF, ML tables to use
    uint32_t huf_desc;     // bytes of its tree description (tables stage)
    uint32_t bits_off;     // sequence bitstream, from seq_off (tables stage)
    int32_t seq_left;      // with kSeqStream: bits left when the sequences ended (< 0: read past the start)
    int32_t lit_before;    // with kLitStream: bits a refused stream had left before its last symbol (-1: other)
};

struct Totals {
    uint64_t nb, nlit, nseq, nhuf, nfse, out_len, fcs;
    uint64_t least;  // a lower bound of the regenerated size, from the headers alone
    uint32_t has_fcs, pad;
};

struct HufTab {
    uint32_t log, pad[3];
    uint16_t e[1u << kHufLogMax];  // symbol | bits << 8, indexed by the next `log` bits
};
struct FseTab {
    uint32_t log, pad[3];
    uint32_t e[512];  // symbol | bits << 8 | baseline << 16
};

// One sequence: its literals lits[lit, lit + ll) go to block-relative position out, its
// match behind them.  sym 0: off is the offset; sym k + 1: max(1, entry rep k - off).
struct Seq {
    uint32_t out, lit, ll, ml, off, sym;
};
// Repeat-offset history in the same symbolic form.
struct Hist {
    uint32_t sym[3], val[3];
};

UNZ_HD uint32_t le16(const uint8_t* p) { return p[0] | (uint32_t)p[1] << 8; }
UNZ_HD uint32_t le24(const uint8_t* p) { return p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16; }
UNZ_HD uint32_t le32(const uint8_t* p) { return le24(p) | (uint32_t)p[3] << 24; }

// Frame header: *pos = its size.
UNZ_HD uint32_t parse_header(const uint8_t* in, uint64_t len, uint64_t& pos, uint64_t& fcs, uint32_t& has_fcs) {
    if (len < 4) return kTrunc;
    if (le32(in) != 0xFD2FB528u) return kMagic;
    if (len < 5) return kTrunc;
    const uint32_t fhd = in[4], did = fhd & 3, single = (fhd >> 5) & 1, fid = fhd >> 6;
    const uint32_t dbytes = did == 3 ? 4 : did, fbytes = fid == 0 ? single : 1u << fid;
    const uint64_t hs = 5 + (single ? 0 : 1) + dbytes + fbytes;
    if (len < hs) return kTrunc;
    if (fhd & 8) return kReserved;
    if (fhd & 4) return kChecksum;
    uint64_t p = 5;
    if (!single && (in[p++] >> 3) + 10u > 31u) return kWindow;
    uint32_t dict = 0;
    for (uint32_t i = 0; i < dbytes; ++i) dict |= (uint32_t)in[p++] << (8 * i);
    if (dict) return kDict;
    fcs = 0;
    for (uint32_t i = 0; i < fbytes; ++i) fcs |= (uint64_t)in[p++] << (8 * i);
    if (fbytes == 2) fcs += 256;
    has_fcs = fbytes != 0;
    pos = hs;
    return kOk;
}

// Stage 1.  out == nullptr: count only (t sizes the scratch); else blocks [0, cap) written.
UNZ_HD uint64_t scan(const uint8_t* in, uint64_t len, Block* out, uint64_t cap, Totals& t) {
    t = Totals{};
    uint64_t pos = 0;
    if (const uint32_t e = parse_header(in, len, pos, t.fcs, t.has_fcs)) return ekey(0, e);
    uint32_t cur_huf = kNone, cur_fse[3] = {kNone, kNone, kNone};
    uint64_t b = 0;
    for (;; ++b) {
        if (len - pos < 3) return ekey(b, kTrunc);
        const uint32_t h = le24(in + pos);
        pos += 3;
        const uint32_t last = h & 1, type = (h >> 1) & 3, size = h >> 3;
        if (type == 3) return ekey(b, kBlockType);
        Block k{};
        k.lit_before = -1;
        k.type = type;
        k.off = pos;
        if (type == 1) {
            if (size > kBlockMax) return ekey(b, kBlockBig);
            if (len - pos < 1) return ekey(b, kTrunc);
            k.size = 1, k.regen = size;
            t.least += size;
            pos += 1;
        } else if (type == 0) {
            if (size > kBlockMax) return ekey(b, kBlockBig);
            if (len - pos < size) return ekey(b, kTrunc);
            k.size = k.regen = size;
            t.least += size;
            pos += size;
        } else {
            if (len - pos < size) return ekey(b, kTrunc);
            if (size < 3 || size >= kBlockMax) return ekey(b, kBlockSize);
            k.size = size;
            const uint8_t* p = in + pos;  // size >= 3 bytes readable
            const uint32_t lt = p[0] & 3, sf = (p[0] >> 2) & 3;
            uint32_t lh, regen, csize, streams = 0;
            if (lt < 2) {
                if (sf == 1) lh = 2, regen = le16(p) >> 4;
                else if (sf == 3) lh = 3, regen = le24(p) >> 4;
                else lh = 1, regen = p[0] >> 3;
                csize = lt == 0 ? regen : 1;
            } else {
                if (size < 5) return ekey(b, kLitHeader);
                const uint32_t lhc = le32(p);
                if (sf < 2) lh = 3, streams = sf ? 4 : 1, regen = (lhc >> 4) & 0x3FF, csize = (lhc >> 14) & 0x3FF;
                else if (sf == 2) lh = 4, streams = 4, regen = (lhc >> 4) & 0x3FFF, csize = lhc >> 18;
                else lh = 5, streams = 4, regen = (lhc >> 4) & 0x3FFFF, csize = (lhc >> 22) + ((uint32_t)p[4] << 10);
                if (!regen || !csize) return ekey(b, kLitHeader);
            }
            if (regen > kBlockMax || (uint64_t)lh + csize > size) return ekey(b, kLitHeader);
            if (lt == 2) k.huf_slot = cur_huf = (uint32_t)t.nhuf++;
            else if (lt == 3) {
                if (cur_huf == kNone) return ekey(b, kNoPrev);
                k.huf_slot = cur_huf;
            }
            k.lit_type = lt, k.lit_regen = regen, k.lit_csize = csize, k.lit_streams = streams;
            k.lit_off = pos + lh;
            uint32_t q = lh + csize;  // the sequences section
            if (q >= size) return ekey(b, kSeqHeader);
            uint32_t n = p[q++];
            if (n == 0) {
                if (q != size) return ekey(b, kSeqHeader);
            } else {
                if (n == 255) {
                    if (q + 2 > size) return ekey(b, kSeqHeader);
                    n = le16(p + q) + 0x7F00, q += 2;
                } else if (n >= 128) {
                    if (q >= size) return ekey(b, kSeqHeader);
                    n = ((n - 128) << 8) + p[q++];
                }
                if (q >= size || n == 0) return ekey(b, kSeqHeader);
                if (n > kMaxSeq) return ekey(b, kBlockBig);
                k.modes = p[q++];
                if (k.modes & 3) return ekey(b, kSeqHeader);  // reserved bits
                for (uint32_t j = 0; j < 3; ++j) {
                    if (((k.modes >> (6 - 2 * j)) & 3) == 3) {
                        if (cur_fse[j] == kNone) return ekey(b, kNoPrev);
                    } else {
                        cur_fse[j] = (uint32_t)t.nfse++;
                    }
                    k.fse_slot[j] = cur_fse[j];
                }
            }
            k.nseq = n;
            k.seq_off = pos + q;
            k.lit_base = t.nlit, t.nlit += regen;
            k.seq_base = t.nseq, t.nseq += n;
            t.least += regen + 3ull * n;  // every literal, and 3 bytes a match
            pos += size;
        }
        // before any scratch is sized by these sums
        if (t.least >> 32) return ekey(b, kTooBig);
        if (out) {
            if (b >= cap) return ekey(b, kTrunc);
            out[b] = k;
        }
        if (last) break;
    }
    if (pos != len) return ekey(b, kTrailing);
    t.nb = b + 1;
    return kNoErr;
}

// ---- stage 2: tables ----------------------------------------------------------------
// Bits [pos, pos + n) of p[0, size), LSB first; zero past the end.
UNZ_HD uint32_t fwd_bits(const uint8_t* p, uint32_t size, uint64_t pos, uint32_t n) {
    uint64_t w = 0;
    const uint64_t b0 = pos >> 3;
    for (uint32_t i = 0; i < 4; ++i)
        if (b0 + i < size) w |= (uint64_t)p[b0 + i] << (8 * i);
    return (uint32_t)(w >> (pos & 7)) & ((1u << n) - 1);
}

// FSE table description (FSE_readNCount): bytes used, 0 = malformed.  norm holds maxsym + 1 entries.
UNZ_HD uint32_t read_ncount(const uint8_t* p, uint32_t size, int16_t* norm, uint32_t& maxsym, uint32_t& log) {
    if (!size) return 0;
    const uint64_t end = (uint64_t)size * 8;
    log = fwd_bits(p, size, 0, 4) + 5;
    if (log > 15) return 0;
    uint64_t pos = 4;
    int32_t remaining = (1 << log) + 1, threshold = 1 << log;
    uint32_t nb = log + 1, sym = 0;
    bool prev0 = false;
    while (remaining > 1 && sym <= maxsym) {
        if (prev0) {
            uint32_t n0 = sym;
            while (pos < end && fwd_bits(p, size, pos, 16) == 0xFFFF) n0 += 24, pos += 16;
            while (pos < end && fwd_bits(p, size, pos, 2) == 3) n0 += 3, pos += 2;
            n0 += fwd_bits(p, size, pos, 2), pos += 2;
            if (n0 > maxsym) return 0;
            while (sym < n0) norm[sym++] = 0;
        }
        const int32_t max = (2 * threshold - 1) - remaining;
        int32_t count = (int32_t)fwd_bits(p, size, pos, nb - 1);
        if (count < max) {
            pos += nb - 1;
        } else {
            count = (int32_t)fwd_bits(p, size, pos, nb);
            if (count >= threshold) count -= max;
            pos += nb;
        }
        --count;
        remaining -= count < 0 ? -count : count;
        norm[sym++] = (int16_t)count;
        prev0 = !count;
        while (remaining < threshold) --nb, threshold >>= 1;
    }
    if (remaining != 1 || pos > end) return 0;
    maxsym = sym - 1;
    return (uint32_t)((pos + 7) >> 3);
}

// FSE decode table of a normalized distribution (FSE_buildDTable / ZSTD_buildFSETable).
// next: nsym entries of work space.
UNZ_HD bool fse_table(const int16_t* norm, uint32_t nsym, uint32_t log, uint32_t* e, uint16_t* next) {
    const uint32_t size = 1u << log, mask = size - 1, step = (size >> 1) + (size >> 3) + 3;
    uint32_t high = size - 1;
    for (uint32_t s = 0; s < nsym; ++s) {
        if (norm[s] == -1) e[high--] = s, next[s] = 1;
        else next[s] = (uint16_t)norm[s];
    }
    uint32_t pos = 0;
    for (uint32_t s = 0; s < nsym; ++s)
        for (int32_t i = 0; i < norm[s]; ++i) {
            e[pos] = s;
            do pos = (pos + step) & mask;
            while (pos > high);
        }
    if (pos != 0) return false;
    for (uint32_t u = 0; u < size; ++u) {
        const uint32_t s = e[u], ns = next[s]++, nbits = log - zstd::highbit32(ns);
        e[u] = s | nbits << 8 | ((ns << nbits) - size) << 16;
    }
    return true;
}

// Backward bit reader over p[0, n): t bits remain (negative: read past the start, as zeros).
// (A reader that kept sixteen 8-byte words of the stream in registers and loaded eight
// ahead was measured and was slower, 28.5 against 17.1 ms of k_unz_decode: DESIGN.md §11.)
struct BitR {
    const uint8_t* p;
    int64_t t;
    uint64_t w;  // the next bits, from the top
    int32_t v;   // of which valid
    // false: an empty stream or one without its end mark
    __host__ __device__ bool init(const uint8_t* p_, uint32_t n) {
        p = p_, w = 0, v = 0, t = 0;
        if (!n || !p_[n - 1]) return false;
        t = (int64_t)(n - 1) * 8 + zstd::highbit32(p_[n - 1]);
        return true;
    }
    __host__ __device__ void fill() {
        if (t <= 0) {
            w = 0, v = 64;
            return;
        }
        const int64_t top = (t - 1) >> 3, s = top - 7;  // the 8 bytes ending at the one that holds bit t - 1
        uint64_t x = 0;
        if (s >= 0) __builtin_memcpy(&x, p + s, 8);
        else
            for (int64_t i = 0; i <= top; ++i) x |= (uint64_t)p[i] << (8 * (i - s));
        const uint32_t sh = 7 - (uint32_t)((t - 1) & 7);
        w = x << sh, v = 64 - (int32_t)sh;
    }
    __host__ __device__ uint32_t peek(uint32_t n) {  // 1 <= n <= 32
        if (v < (int32_t)n) fill();
        return (uint32_t)(w >> (64 - n));
    }
    __host__ __device__ void skip(uint32_t n) { w <<= n, v -= (int32_t)n, t -= n; }
    __host__ __device__ uint32_t read(uint32_t n) {  // n <= 32
        if (!n) return 0;
        const uint32_t r = peek(n);
        skip(n);
        return r;
    }
};

// Huffman weights coded with FSE (FSE_decompress with two interleaved states): count, 0 = malformed.
UNZ_HD uint32_t fse_weights(const uint8_t* p, uint32_t size, uint8_t* wt) {
    int16_t norm[256];
    uint16_t next[256];
    uint32_t e[64];
    uint32_t maxsym = 255, log = 0;
    const uint32_t used = read_ncount(p, size, norm, maxsym, log);
    if (!used || log > 6 || used >= size) return 0;
    if (!fse_table(norm, maxsym + 1, log, e, next)) return 0;
    BitR r;
    if (!r.init(p + used, size - used)) return 0;
    uint32_t s1 = r.read(log), s2 = r.read(log), n = 0;
    for (;;) {
        if (n > 253) return 0;
        wt[n++] = (uint8_t)e[s1];
        s1 = (e[s1] >> 16) + r.read((e[s1] >> 8) & 255);
        if (r.t < 0) {
            wt[n++] = (uint8_t)e[s2];
            break;
        }
        if (n > 253) return 0;
        wt[n++] = (uint8_t)e[s2];
        s2 = (e[s2] >> 16) + r.read((e[s2] >> 8) & 255);
        if (r.t < 0) {
            wt[n++] = (uint8_t)e[s1];
            break;
        }
    }
    return n;
}

// Huffman decode table from a tree description at p (avail bytes): its size, 0 = malformed.
UNZ_HD uint32_t huf_table(const uint8_t* p, uint32_t avail, HufTab& T) {
    if (!avail) return 0;
    uint8_t wt[256];
    uint32_t n, desc;
    const uint32_t hb = p[0];
    if (hb >= 128) {
        n = hb - 127;
        desc = 1 + (n + 1) / 2;
        if (desc > avail) return 0;
        for (uint32_t i = 0; i < n; ++i) wt[i] = (i & 1) ? p[1 + i / 2] & 15 : p[1 + i / 2] >> 4;
    } else {
        desc = 1 + hb;
        if (!hb || desc > avail) return 0;
        n = fse_weights(p + 1, hb, wt);
        if (!n) return 0;
    }
    uint32_t rank[kHufLogMax + 1] = {}, total = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (wt[i] >= kHufLogMax) return 0;
        rank[wt[i]]++;
        total += (1u << wt[i]) >> 1;
    }
    if (!total) return 0;
    const uint32_t log = zstd::highbit32(total) + 1;
    if (log > kHufLogMax) return 0;
    const uint32_t rest = (1u << log) - total;
    if (rest & (rest - 1)) return 0;  // the last weight completes a power of two
    wt[n] = (uint8_t)(zstd::highbit32(rest) + 1);
    rank[wt[n++]]++;
    if (rank[1] < 2 || (rank[1] & 1)) return 0;
    uint32_t start[kHufLogMax + 1], nx = 0;
    for (uint32_t w = 1; w <= log; ++w) start[w] = nx, nx += rank[w] << (w - 1);
    for (uint32_t s = 0; s < n; ++s) {
        const uint32_t w = wt[s];
        if (!w) continue;
        const uint32_t length = (1u << w) >> 1, ent = s | (log + 1 - w) << 8;
        for (uint32_t u = start[w]; u < start[w] + length; ++u) T.e[u] = (uint16_t)ent;
        start[w] += length;
    }
    T.log = log;
    return desc;
}

constexpr int16_t kLLNorm[36] = {4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2,
                                 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1};
constexpr int16_t kOFNorm[29] = {1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1};
constexpr int16_t kMLNorm[53] = {1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                                 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1};

// What block k defines: its Huffman table and the sequence tables whose mode is not
// Repeat, into their slots; k.huf_desc and k.bits_off.
UNZ_HD uint32_t build_tables(const uint8_t* in, Block& k, HufTab* huf, FseTab* fse) {
    if (k.type != 2) return kOk;
    if (k.lit_type == 2) {
        const uint32_t d = huf_table(in + k.lit_off, k.lit_csize, huf[k.huf_slot]);
        if (!d || d >= k.lit_csize) return kHufDesc;
        k.huf_desc = d;
    }
    if (!k.nseq) return kOk;
    const uint32_t end = (uint32_t)(k.off + k.size - k.seq_off);
    const uint8_t* p = in + k.seq_off;
    uint32_t q = 0;
    int16_t norm[53];
    uint16_t next[53];
    for (uint32_t j = 0; j < 3; ++j) {
        const uint32_t mode = (k.modes >> (6 - 2 * j)) & 3;
        if (mode == 3) continue;
        FseTab& T = fse[k.fse_slot[j]];
        const uint32_t maxsym = j == 0 ? 35 : j == 1 ? 31 : 52;
        if (mode == 0) {
            const int16_t* d = j == 0 ? kLLNorm : j == 1 ? kOFNorm : kMLNorm;
            const uint32_t ns = j == 0 ? 36 : j == 1 ? 29 : 53;
            for (uint32_t s = 0; s < ns; ++s) norm[s] = d[s];
            T.log = j == 1 ? 5 : 6;
            if (!fse_table(norm, ns, T.log, T.e, next)) return kFseDesc;
        } else if (mode == 1) {
            if (q >= end || p[q] > maxsym) return kFseDesc;
            T.log = 0;
            T.e[0] = p[q++];
        } else {
            uint32_t ms = maxsym, log = 0;
            const uint32_t used = read_ncount(p + q, end - q, norm, ms, log);
            if (!used || log > (j == 1 ? 8u : 9u)) return kFseDesc;
            T.log = log;
            if (!fse_table(norm, ms + 1, log, T.e, next)) return kFseDesc;
            q += used;
        }
    }
    if (q >= end || !p[end - 1]) return kSeqStream;
    k.bits_off = q;
    return kOk;
}

// ---- stage 3: entropy decode --------------------------------------------------------
// Raw / RLE literals: thread tid of nt.
UNZ_HD void lit_fill(const uint8_t* in, const Block& k, uint8_t* lits, uint32_t tid, uint32_t nt) {
    uint8_t* o = lits + k.lit_base;
    const uint8_t* p = in + k.lit_off;
    if (k.lit_type == 0)
        for (uint32_t i = tid; i < k.lit_regen; i += nt) o[i] = p[i];
    else
        for (uint32_t i = tid; i < k.lit_regen; i += nt) o[i] = p[0];
}

// Huffman stream j of block k (table e of `log` bits).
UNZ_HD uint32_t lit_stream(const uint8_t* in, Block& k, const uint16_t* e, uint32_t log, uint32_t j,
                           uint8_t* lits) {
    const uint32_t desc = k.lit_type == 2 ? k.huf_desc : 0;
    const uint8_t* p = in + k.lit_off + desc;
    uint32_t n = k.lit_csize - desc, o0 = 0, o1 = k.lit_regen;
    if (k.lit_streams == 4) {
        if (n < 10) return kLitStream;
        const uint32_t s[3] = {le16(p), le16(p + 2), le16(p + 4)};
        if (6 + s[0] + s[1] + s[2] > n) return kLitStream;
        const uint32_t seg = (k.lit_regen + 3) / 4;
        if (3 * seg > k.lit_regen) return kLitStream;
        uint32_t at = 6;
        for (uint32_t i = 0; i < j; ++i) at += s[i];
        n = j < 3 ? s[j] : n - at;
        p += at;
        o0 = j * seg;
        if (j < 3) o1 = o0 + seg;
    }
    BitR r;
    if (!r.init(p, n)) return kLitStream;
    uint8_t* o = lits + k.lit_base;
    int64_t before = 0;  // bits left before the last symbol
    uint32_t last_bits = 0;
    for (uint32_t i = o0; i < o1; ++i) {
        const uint32_t x = e[r.peek(log)];
        before = r.t, last_bits = x >> 8;
        r.skip(x >> 8);
        o[i] = (uint8_t)x;
    }
    if (r.t == 0) return kOk;
    // libzstd's double-symbol decoder is lenient about a stream's last symbol
    // (HUF_decodeLastSymbolX2: a table entry that holds two symbols, 12 bits wide at most,
    // may stand for the last one, and what it consumes is cut off at the stream's start).
    // Following it keeps the bytes equal to libzstd's wherever it accepts: a last code that runs past the start is
    // read with zeros for the missing bits, and up to one more code may lie between the last
    // symbol and the start when both codes fit one entry.  The symbols are the same either way.
    if (o1 == o0 || before <= 0) {
        k.lit_before = o1 > o0 && before == 0 ? 0 : -1;
        return kLitStream;
    }
    if (r.t < 0) return kOk;
    {
        const uint32_t more = e[r.peek(log)] >> 8;
        if ((int64_t)more >= r.t && last_bits + more <= kHufLogMax) return kOk;
    }
    k.lit_before = -1;
    return kLitStream;
}

UNZ_HD void hist_dec(uint32_t& sym, uint32_t& val) {  // rep1 - 1 (0 reads as 1, as libzstd)
    if (sym) ++val;
    else if (--val == 0) val = 1;
}

// The block's sequences from the interleaved bitstream; out[0, nseq); exit = its history.
UNZ_HD uint32_t seq_decode(const uint8_t* in, Block& k, const uint32_t* ell, uint32_t lll, const uint32_t* eof,
                           uint32_t lof, const uint32_t* eml, uint32_t lml, Seq* out, Hist& exit) {
    Hist h = {{1, 2, 3}, {0, 0, 0}};
    if (!k.nseq) {
        k.regen = k.lit_regen;
        exit = h;
        return kOk;
    }
    BitR r;
    if (!r.init(in + k.seq_off + k.bits_off, (uint32_t)(k.off + k.size - k.seq_off) - k.bits_off)) return kSeqStream;
    uint32_t sl = r.read(lll), so = r.read(lof), sm = r.read(lml);
    uint32_t pos = 0, lit = 0;
    for (uint32_t i = 0; i < k.nseq; ++i) {
        const uint32_t el = ell[sl], eo = eof[so], em = eml[sm];
        const uint32_t lc = el & 255, oc = eo & 255, mc = em & 255;
        const uint32_t offv = (1u << oc) + r.read(oc);
        const uint32_t ml = (mc < 32 ? mc + 3 : zstd::kMLBase[mc - 32]) + r.read(mc < 32 ? 0 : zstd::kMLBits[mc - 32]);
        const uint32_t ll = zstd::kLLBase[lc] + r.read(zstd::kLLBits[lc]);
        uint32_t cs, cv;
        if (offv > 3) {
            cs = 0, cv = offv - 3;
            h.sym[2] = h.sym[1], h.val[2] = h.val[1], h.sym[1] = h.sym[0], h.val[1] = h.val[0];
        } else {
            const uint32_t idx = offv - 1 + (ll == 0);
            if (idx == 0) {
                cs = h.sym[0], cv = h.val[0];
            } else {
                const uint32_t src = idx == 3 ? 0 : idx;
                cs = h.sym[src], cv = h.val[src];
                if (idx == 3) hist_dec(cs, cv);
                if (idx != 1) h.sym[2] = h.sym[1], h.val[2] = h.val[1];
                h.sym[1] = h.sym[0], h.val[1] = h.val[0];
            }
        }
        h.sym[0] = cs, h.val[0] = cv;
        if (ll > k.lit_regen - lit) return kLitOver;
        if ((uint64_t)pos + ll + ml > kBlockMax) return kBlockBig;
        out[i] = Seq{pos, lit, ll, ml, cv, cs};
        pos += ll + ml, lit += ll;
        if (i + 1 < k.nseq) {
            sl = (el >> 16) + r.read((el >> 8) & 255);
            sm = (em >> 16) + r.read((em >> 8) & 255);
            so = (eo >> 16) + r.read((eo >> 8) & 255);
        }
    }
    if (r.t != 0) {
        k.seq_left = (int32_t)(r.t < -(1 << 30) ? -(1 << 30) : r.t);
        return kSeqStream;
    }
    if (pos + (k.lit_regen - lit) > kBlockMax) return kBlockBig;
    k.regen = pos + (k.lit_regen - lit);
    exit = h;
    return kOk;
}

// ---- stage 4: stitch ----------------------------------------------------------------
UNZ_HD uint32_t hist_value(const uint32_t* entry, uint32_t sym, uint32_t val) {
    if (!sym) return val;
    const int64_t x = (int64_t)entry[sym - 1] - (int64_t)val;
    return x < 1 ? 1u : (uint32_t)x;
}

// entry: 3 per block; bpos: nb + 1 output positions.
UNZ_HD uint64_t stitch(const Block* blocks, uint64_t nb, const Hist* exit, uint32_t* entry, uint64_t* bpos, Totals& t) {
    uint32_t e[3] = {1, 4, 8};
    uint64_t pos = 0;
    for (uint64_t b = 0; b < nb; ++b) {
        for (int j = 0; j < 3; ++j) entry[3 * b + j] = e[j];
        bpos[b] = pos;
        pos += blocks[b].regen;
        if (blocks[b].type == 2 && blocks[b].nseq) {
            uint32_t x[3];
            for (int j = 0; j < 3; ++j) x[j] = hist_value(e, exit[b].sym[j], exit[b].val[j]);
            for (int j = 0; j < 3; ++j) e[j] = x[j];
        }
    }
    bpos[nb] = pos;
    t.out_len = pos;
    if (t.has_fcs && t.fcs != pos) return ekey(nb - 1, kFcs);
    if (pos >> 32) return ekey(nb - 1, kTooBig);
    return kNoErr;
}

// ---- stage 4b: offsets made concrete and checked, one sequence -----------------------
UNZ_HD uint32_t resolve(uint64_t block_pos, const uint32_t* entry, Seq& q) {
    const uint32_t off = hist_value(entry, q.sym, q.off);
    q.off = off, q.sym = 0;
#ifndef UNZSTD_PLANT_BUG
    if (off > block_pos + q.out + q.ll) return kOffset;
#endif
    return kOk;
}

// ---- stage 5: place, output byte i ---------------------------------------------------
UNZ_HD void place(uint64_t i, const uint8_t* in, const Block* blocks, uint64_t nb, const uint64_t* bpos,
                  const Seq* seqs, const uint8_t* lits, uint8_t* out, uint32_t* parent) {
    uint64_t lo = 0, hi = nb;  // the last block with bpos <= i (it is not empty: bpos[b + 1] > i)
    while (hi - lo > 1) {
        const uint64_t m = (lo + hi) / 2;
        if (bpos[m] <= i) lo = m;
        else hi = m;
    }
    const Block& k = blocks[lo];
    const uint32_t r = (uint32_t)(i - bpos[lo]);
    parent[i] = (uint32_t)i;
    if (k.type == 0) {
        out[i] = in[k.off + r];
    } else if (k.type == 1) {
        out[i] = in[k.off];
    } else if (!k.nseq) {
        out[i] = lits[k.lit_base + r];
    } else {
        const Seq* S = seqs + k.seq_base;
        uint32_t a = 0, z = k.nseq;  // the last sequence with out <= r
        while (z - a > 1) {
            const uint32_t m = (a + z) / 2;
            if (S[m].out <= r) a = m;
            else z = m;
        }
        const Seq q = S[a];
        const uint32_t d = r - q.out;
        if (d < q.ll) out[i] = lits[k.lit_base + q.lit + d];
        else if (d < q.ll + q.ml) parent[i] = (uint32_t)(i - q.off);
        else out[i] = lits[k.lit_base + q.lit + q.ll + (d - q.ll - q.ml)];
    }
}

// ---- stage 6: pointer jumping and gather --------------------------------------------
// true: the parent of i moved (another round is needed).  In place: whatever another thread
// has already written to an entry is an ancestor of it, so every value read is one.
UNZ_HD bool jump(uint64_t i, uint32_t* parent) {
    const uint32_t p = parent[i];
    if (p == i) return false;
    const uint32_t g = parent[p];
    if (g == p) return false;
    parent[i] = parent[parent[g]];  // four hops a round (a root is its own parent)
    return true;
}
UNZ_HD void gather(uint64_t i, const uint32_t* parent, uint8_t* out) {
    const uint32_t p = parent[i];
    if (p != i) out[i] = out[p];
}

UNZ_HD const char* err_text(uint32_t e) {
    switch (e) {
        case kMagic: return "not a zstd frame (bad magic)";
        case kTrunc: return "truncated frame";
        case kReserved: return "reserved Frame_Header_Descriptor bit set";
        case kDict: return "frame needs a dictionary (non-zero Dictionary_ID)";
        case kChecksum: return "Content_Checksum flag set (XXH64 is not computed here)";
        case kWindow: return "window larger than 2 GiB";
        case kTrailing: return "bytes behind the last block (trailing data or a second frame)";
        case kBlockType: return "reserved block type 3";
        case kBlockBig: return "block regenerates more than 128 KiB";
        case kBlockSize: return "Compressed block of an impossible size";
        case kLitHeader: return "bad literals section header";
        case kHufDesc: return "Huffman tree description does not add up";
        case kFseDesc: return "FSE table description does not add up";
        case kNoPrev: return "Treeless literals or Repeat_Mode with no earlier table";
        case kLitStream: return "literal stream does not end with its symbols";
        case kSeqHeader: return "bad sequences section header";
        case kSeqStream: return "sequence bitstream does not end with its sequences";
        case kLitOver: return "sequences consume more literals than present";
        case kOffset: return "offset reaches before the start of the output";
        case kFcs: return "Frame_Content_Size differs from the regenerated size";
        case kTooBig: return "regenerated size of 4 GiB or more";
        default: return "unknown";
    }
}

#undef UNZ_HD
}  // namespace unz

// The launches (sydelta_unzstd.hip).  All pointers are device memory.
struct Profiler;
constexpr uint32_t kUnzRounds = 32;  // pointer-doubling rounds: chains are shorter than 2^32
struct UnzArgs {
    const uint8_t* in;
    unz::Block* blocks;  // nb
    uint64_t nb;
    unz::HufTab* huf;    // Totals::nhuf slots
    unz::FseTab* fse;    // Totals::nfse slots
    uint8_t* lits;       // Totals::nlit bytes
    unz::Seq* seqs;      // Totals::nseq
    unz::Hist* exit;     // nb
    uint32_t* entry;     // 3 nb
    uint64_t* bpos;      // nb + 1
    unz::Totals* tot;
    unsigned long long* status;
};
// The decode scratch behind UnzArgs / UnzbArgs for these counts, every region on a 256-byte
// boundary; bpos holds nb + bpos_extra words (1 for a frame, nfiles for a batch).
struct UnzScratch {
    uint64_t blocks, huf, fse, lits, seqs, exit, entry, bpos, changed, total;
    UnzScratch(uint64_t nb, uint64_t nhuf, uint64_t nfse, uint64_t nlit, uint64_t nseq, uint64_t bpos_extra) {
        uint64_t at = 0;
        auto take = [&at](uint64_t bytes) {
            const uint64_t o = at;
            at += (bytes + 255) & ~(uint64_t)255;
            return o;
        };
        blocks = take(nb * sizeof(unz::Block)), huf = take(nhuf * sizeof(unz::HufTab)), fse = take(nfse * sizeof(unz::FseTab));
        lits = take(nlit), seqs = take(nseq * sizeof(unz::Seq)), exit = take(nb * sizeof(unz::Hist)), entry = take(nb * 12);
        bpos = take((nb + bpos_extra) * 8), changed = take(4 * kUnzRounds), total = at;
    }
    template <class Args>
    void point(Args& a, uint8_t* W) const {
        a.blocks = (unz::Block*)(W + blocks);
        a.huf = (unz::HufTab*)(W + huf);
        a.fse = (unz::FseTab*)(W + fse);
        a.lits = W + lits;
        a.seqs = (unz::Seq*)(W + seqs);
        a.exit = (unz::Hist*)(W + exit);
        a.entry = (uint32_t*)(W + entry);
        a.bpos = (uint64_t*)(W + bpos);
    }
};
// Stage 1 (d_blocks NULL: the counts alone).
hipError_t launch_unz_scan(const uint8_t* d_in, uint64_t len, unz::Block* d_blocks, uint64_t cap, unz::Totals* d_tot,
                           unsigned long long* d_status, hipStream_t s, Profiler* prof);
// Stages 2-4b: tables, entropy decode, stitch (a.tot->out_len), offsets resolved and checked.
hipError_t launch_unz_decode(const UnzArgs& a, hipStream_t s, Profiler* prof);
// Stages 5-6: n = out_len bytes into d_out; d_parent: n words, d_changed: kUnzRounds words.
hipError_t launch_unz_place(const UnzArgs& a, uint64_t n, uint8_t* d_out, uint32_t* d_parent, uint32_t* d_changed,
                            hipStream_t s, Profiler* prof);
}  // namespace sydelta
