// sydelta_sigbatch.hpp — sydelta_checksums_batch_to_json_device (K7sb) and
// sydelta_checksums_batch_from_json_device (K7pb): the signature texts of a whole batch
// (`sy-remote checksums`, sy-remote.rs:145-147, once per file) written and parsed in one call
// each, the two steps of the remote exchange between sydelta_signature_batch_device (receiver)
// and sydelta_index_create_batch + sydelta_match_batch_device (sender).
//
// The text and its grammar are sydelta_sigjson.hpp's: entry_len / entry_write / store_chunk and
// parse_entry / chunk_entries are called here, not copied.  What a batch adds is where a file's
// things lie.
//
// Writer.  The signature is the concatenated SoA of sydelta_signature_batch_device: file f's
// entries at ebase[f] = the sum of the earlier nblocks.  A tile is up to kTile entries of one
// file (a file without blocks has the one tile that writes "[]"); one workgroup per tile.
// k_sigb_len sums the tiles' lengths, one exclusive scan (with a trailing entry) places the
// tiles, a lane per file takes text_len[f] from the scan at its first tile and at the next
// file's, a second scan over the lengths rounded up to 16 gives text_off, and k_sigb_write
// composes each tile in LDS and stores it.  One wait.
//
// Parser.  The 64-byte chunks of all texts share one chunk table (file f's at cbase[f]) with one
// trailing entry; one exclusive scan over the '{' counts ranks the entries of the whole batch,
// so file f's entry i is rank R[cbase[f]] + i = sig_off[f] + i and nblocks[f] = R[cbase[f + 1]] -
// R[cbase[f]].  A tile is up to 64 chunks of one file: one wave.  Beside the grammar the parser
// holds every entry to the layout compute_checksums (checksum.rs:46-76) produces for the block
// size the sender chose: index == i, offset == i * bs, size == bs but for the last entry, whose
// size lies in (0, bs].  That is what makes the result the SoA sydelta_index_create_batch takes.
// Stages: count (wave per tile) -> scan -> sizes (lane per file) -> parse (wave per tile).  One
// wait.
//
// The plan (host) and the per-file bodies are shared with tests/csrc/sig_batch_check.cpp, which
// runs them on host memory.
#pragma once
#include <stdarg.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "../../include/sydelta.h"
#include "sydelta_sigjson.hpp"

#define SIGB_HD __host__ __device__ inline

namespace sydelta {
namespace sigb {

constexpr uint32_t kLanes = 64;               // files per workgroup of the lane-per-file kernels
constexpr uint32_t kTileChunks = 64;          // parser: chunks per tile, one wave
constexpr uint32_t kStageBytes = 640u << 10;  // a pinned upload slot: 20 480 files
constexpr uint32_t kStageSlots = 2;
constexpr uint64_t kNoBad = UINT64_MAX;
constexpr uint64_t kLayoutBit = 1ull << 63;

// The parser's staged span of a tile: the tile's 4 KiB, the two bytes parse_entry looks at
// before a '{' on the tile's first byte, and behind the tile the rest of an entry that starts on
// its last byte with the two bytes of look-ahead (kMaxEntry counts the separator before the '{'
// and a ']' behind the '}': 136 bytes from '{' to '}', then ",{" or "]").
constexpr uint32_t kBefore = 2;
constexpr uint32_t kAfter = sigjson::kMaxEntry;
constexpr uint32_t kSpan = kBefore + kTileChunks * sigjson::kParseChunk + kAfter;
constexpr uint32_t kRow = 68;  // LDS bytes per staged 64-byte row: lanes 64 bytes apart hit 64 banks
// staged from the 16-byte granule of the span's first byte: up to 15 bytes in front
constexpr uint32_t kRows = (kSpan + 15 + 15 + 63) / 64;

SIGB_HD uint64_t pad16(uint64_t n) { return (n + 15) & ~(uint64_t)15; }
template <class I>
SIGB_HD I stage_off(I d) { return (d >> 6) * kRow + (d & 63); }

// ---------------------------------------------------------------------------
// Writer
// ---------------------------------------------------------------------------
struct WFile {
    uint64_t ebase;  // its first entry of the SoA
    uint64_t n;      // entries
    uint64_t last;   // size of its last block
    uint64_t tbase;  // its first tile
};
static_assert(sizeof(WFile) == 32, "table layout");

SIGB_HD uint64_t wtiles_of(uint64_t n) { return n ? (n + sigjson::kTile - 1) / sigjson::kTile : 1; }

// The file of a tile: the last f with tbase <= tile.  Every writer file has a tile, so the bases
// are strictly increasing; the parser's files may have none and then share their tbase with the
// next file that has some, which stands behind them (tile < the total: never a trailing one).
template <class F>
SIGB_HD uint64_t file_of_tile(const F* files, uint64_t nfiles, uint64_t tile) {
    uint64_t lo = 0, hi = nfiles;
    while (hi - lo > 1) {
        const uint64_t m = (lo + hi) / 2;
        if (files[m].tbase <= tile) lo = m;
        else hi = m;
    }
    return lo;
}

// File F as the single writer sees it: its own arrays, entries 0 .. n - 1.
SIGB_HD sigjson::SigArgs wargs_of(const uint32_t* weak, const uint64_t* strong, const WFile& F, uint64_t bs) {
    return sigjson::SigArgs{weak + F.ebase, strong + F.ebase, F.n, bs, F.last};
}
// Length of the text of entry slot k (0 .. kTile - 1) of the file's tile `lt`.
SIGB_HD uint32_t wslot_len(const sigjson::SigArgs& a, uint64_t lt, uint32_t k) {
    if (a.n == 0) return k == 0 ? 2u : 0u;  // []
    const uint64_t i = lt * sigjson::kTile + k;
    return i < a.n ? sigjson::entry_len(a, i) : 0u;
}
SIGB_HD void wslot_write(const sigjson::SigArgs& a, uint64_t lt, uint32_t k, uint8_t* p) {
    if (a.n == 0) {
        if (k == 0) p[0] = '[', p[1] = ']';
        return;
    }
    const uint64_t i = lt * sigjson::kTile + k;
    if (i < a.n) sigjson::entry_write(a, i, p);
}
// Lane-per-file: the text's length from the scan of the tile lengths (toff: ntiles + 1 entries).
SIGB_HD uint64_t wfile_len(const WFile* files, uint64_t nfiles, uint64_t ntiles, const uint64_t* toff, uint64_t f) {
    const uint64_t t1 = f + 1 < nfiles ? files[f + 1].tbase : ntiles;
    return toff[t1] - toff[files[f].tbase];
}

// ---------------------------------------------------------------------------
// Parser
// ---------------------------------------------------------------------------
struct PFile {
    uint64_t off, len;  // the text: d_text[off, +len)
    uint64_t cbase;     // its first entry of the chunk table
    uint64_t tbase;     // its first tile
};
static_assert(sizeof(PFile) == 32, "table layout");

// A text shorter than "[]" has no chunks: it is refused at byte 0 by the sizes stage.
SIGB_HD uint64_t chunks_of(uint64_t len) {
    return len < 2 ? 0 : (len + sigjson::kParseChunk - 1) / sigjson::kParseChunk;
}
SIGB_HD uint64_t ptiles_of(uint64_t len) { return (chunks_of(len) + kTileChunks - 1) / kTileChunks; }

// The staged span of the tile whose first chunk is c0, as text positions [p0, p0 + n), clipped
// to the text.
SIGB_HD uint64_t span_p0(uint64_t c0) {
    const uint64_t b = c0 * sigjson::kParseChunk;
    return b < kBefore ? 0 : b - kBefore;
}
SIGB_HD uint32_t span_len(uint64_t len, uint64_t c0, uint64_t p0) {
    const uint64_t hi = (c0 + kTileChunks) * sigjson::kParseChunk + kAfter;
    return (uint32_t)((hi < len ? hi : len) - p0);
}

// The device's status word of a file: kNoBad, the first byte that breaks the grammar, or
// kLayoutBit | the '{' of the first entry that breaks the layout.  One unsigned minimum keeps
// the smallest byte of a kind and lets a grammar refusal win over a layout one.
SIGB_HD uint64_t status_spelling(uint64_t p) { return p; }
SIGB_HD uint64_t status_layout(uint64_t p) { return kLayoutBit | p; }
// ... and what the caller gets: 0, 1 + P, or (1 << 63) | (1 + P).  P < 2^58.
SIGB_HD uint64_t status_out(uint64_t w) { return w == kNoBad ? 0 : w + 1; }

// Entry i of n of a signature with block size bs, as compute_checksums lays it out.
SIGB_HD bool layout_ok(const sydelta_block_checksum& r, uint64_t i, uint64_t n, uint64_t bs) {
    uint64_t off;
    if (r.index != i || __builtin_mul_overflow(i, bs, &off) || r.offset != off) return false;
    return i + 1 == n ? (r.size > 0 && r.size <= bs) : r.size == bs;
}

// Count stage, chunk c of a file's text t (a pointer or a staged accessor).
template <class T>
SIGB_HD uint64_t count_chunk(const T& t, uint64_t len, uint64_t c) { return sigjson::chunk_entries(t, len, c); }

// Sizes stage, file F (rank: the scan of the whole chunk table, nchunks + 1 entries).
SIGB_HD void sizes_file(const PFile& F, const uint64_t* rank, uint64_t& sig_off, uint64_t& nblocks, uint64_t& last,
                        uint64_t& status, uint64_t& lay_i) {
    sig_off = rank[F.cbase];
    nblocks = rank[F.cbase + chunks_of(F.len)] - sig_off;
    last = 0;
    status = F.len < 2 ? status_spelling(0) : kNoBad;
    lay_i = kNoBad;
}

// Parse stage, chunk c of file F: its entries are i0, i0 + 1, ... of the file's n (both from the
// ranks), and go to weak / strong [sig_off + i] (NULL: checked only).  Returns the chunk's status
// word; *last gets the size of the file's last entry if this chunk holds it, *lay_i the number
// of the chunk's first entry that breaks the layout (the refusal message names it).
template <class T>
SIGB_HD uint64_t parse_chunk(const T& t, uint64_t len, uint64_t c, uint64_t i0, uint64_t n, uint64_t bs,
                             uint64_t sig_off, uint32_t* weak, uint64_t* strong, uint64_t* last, uint64_t* lay_i) {
    if (c == 0 && !sigjson::head_ok(t, len)) return status_spelling(0);
    uint64_t st = kNoBad, i = i0;
    const uint64_t lo = c * sigjson::kParseChunk, hi = lo + sigjson::kParseChunk < len ? lo + sigjson::kParseChunk : len;
    // The chunk's '{' first, as a mask, then one entry per round: the lanes of a wave find their
    // '{' on different bytes, and a parse started inside the byte loop would run once per
    // distinct byte, the other lanes idle.  A chunk of well-formed text holds two at the most.
    static_assert(sigjson::kParseChunk == 64, "one mask bit per byte of the chunk");
    uint64_t m = 0;
    for (uint64_t p = lo; p < hi; ++p) m |= (uint64_t)(t[p] == '{') << (p - lo);
    for (; m; m &= m - 1) {
        const uint64_t p = lo + (uint64_t)__builtin_ctzll(m);
        sydelta_block_checksum r;
        if (!sigjson::parse_entry(t, len, p, r)) return status_spelling(p);  // below any layout word
        if (!layout_ok(r, i, n, bs)) {
            if (st == kNoBad) st = status_layout(p), *lay_i = i;
        } else {
#ifdef SIGB_PLANT_BUG
            (void)sig_off;  // entries left batch-relative from 0: right for the first file only
            const uint64_t at = i;
#else
            const uint64_t at = sig_off + i;
#endif
            if (weak) weak[at] = r.weak, strong[at] = r.strong;
            if (i + 1 == n) *last = r.size;
        }
        ++i;
    }
    return st;
}

// ---------------------------------------------------------------------------
// The host plans: every argument validated (overflow-checked) before a device is touched
// ---------------------------------------------------------------------------
struct PlanErr {
    int code = SYDELTA_OK;
    std::string msg;
};
inline int plan_fail(PlanErr* e, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
inline int plan_fail(PlanErr* e, int code, const char* fmt, ...) {
    char buf[320];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    e->code = code;
    e->msg = buf;
    return code;
}
inline int check_block_size(uint64_t bs, PlanErr* e) {
    if (bs == 0 || bs > (1ull << 32))
        return plan_fail(e, SYDELTA_E_INVAL, "block_size %llu out of range (1 .. 2^32)", (unsigned long long)bs);
    return SYDELTA_OK;
}

// Writer: the file table with every file's entry base and first tile, the totals, and the bounds
// of every text (sigjson::text_bounds).
inline int wplan(bool have_soa, const uint64_t* nblocks, const uint64_t* last_size, uint64_t nfiles, uint64_t bs,
                 std::vector<WFile>* files, std::vector<uint64_t>* lo, std::vector<uint64_t>* hi, uint64_t* nentries,
                 uint64_t* ntiles, PlanErr* e) {
    typedef unsigned long long ull;
    if (!nblocks || !last_size) return plan_fail(e, SYDELTA_E_INVAL, "NULL table");
    if (nfiles > UINT32_MAX) return plan_fail(e, SYDELTA_E_INVAL, "more than 2^32 - 1 files");
    if (check_block_size(bs, e)) return e->code;
    files->resize(nfiles);
    lo->resize(nfiles);
    hi->resize(nfiles);
    uint64_t ne = 0, nt = 0;
    for (uint64_t f = 0; f < nfiles; ++f) {
        const uint64_t n = nblocks[f], last = last_size[f];
        if (n) {
            if (last == 0 || last > bs)
                return plan_fail(e, SYDELTA_E_INVAL, "file %llu: last_size %llu outside (0, %llu]", (ull)f, (ull)last,
                                 (ull)bs);
            if (n - 1 > (UINT64_MAX - last) / bs)
                return plan_fail(e, SYDELTA_E_INVAL, "file %llu: offsets of %llu blocks overflow", (ull)f, (ull)n);
        }
        (*files)[f] = WFile{ne, n, n ? last : 0, nt};
        if (__builtin_add_overflow(ne, n, &ne))
            return plan_fail(e, SYDELTA_E_INVAL, "file %llu: the batch's block count overflows", (ull)f);
        // the scans count their entries in an int (each file's tiles below 2^56, nfiles below 2^32)
        nt += wtiles_of(n);
        if (nt >= 0x7FFFFFFFull)
            return plan_fail(e, SYDELTA_E_INVAL, "file %llu: the batch holds more than 2^31 tiles of 256 blocks: split it",
                             (ull)f);
        sigjson::text_bounds(n, bs, last, (*lo)[f], (*hi)[f]);  // n < 2^39: no overflow
    }
    if (ne && !have_soa) return plan_fail(e, SYDELTA_E_INVAL, "NULL signature arrays");
    *nentries = ne;
    *ntiles = nt;
    return SYDELTA_OK;
}

// The arena that always holds the texts: every file's upper bound, rounded up to 16.
inline uint64_t wbound(const uint64_t* nblocks, const uint64_t* last_size, uint64_t nfiles, uint64_t bs) {
    if (!nfiles) return 0;
    if (!nblocks || !last_size || bs == 0 || bs > (1ull << 32)) return UINT64_MAX;
    uint64_t total = 0;
    for (uint64_t f = 0; f < nfiles; ++f) {
        const uint64_t n = nblocks[f];
        // 138 bytes per entry at the most, and n * bs is part of the bound's arithmetic
        if (n > (UINT64_MAX >> 9) || (n && n - 1 > (UINT64_MAX - bs) / bs)) return UINT64_MAX;
        uint64_t lo, hi;
        sigjson::text_bounds(n, bs, n ? (last_size[f] && last_size[f] <= bs ? last_size[f] : bs) : 0, lo, hi);
        if (__builtin_add_overflow(total, pad16(hi), &total)) return UINT64_MAX;
    }
    return total;
}

// Parser: the file table with the files' places in the chunk table and the tile grid.
inline int pplan(bool have_text, uint64_t text_buf_len, const uint64_t* text_off, const uint64_t* text_len,
                 uint64_t nfiles, uint64_t bs, std::vector<PFile>* files, uint64_t* nchunks, uint64_t* ntiles,
                 PlanErr* e) {
    typedef unsigned long long ull;
    if (!text_off || !text_len) return plan_fail(e, SYDELTA_E_INVAL, "NULL table");
    if (nfiles > UINT32_MAX) return plan_fail(e, SYDELTA_E_INVAL, "more than 2^32 - 1 files");
    if (check_block_size(bs, e)) return e->code;
    files->resize(nfiles);
    uint64_t nc = 0, nt = 0;
    for (uint64_t f = 0; f < nfiles; ++f) {
        const uint64_t off = text_off[f], len = text_len[f];
        if (len > text_buf_len || off > text_buf_len - len)
            return plan_fail(e, SYDELTA_E_INVAL, "file %llu: text [%llu, +%llu) leaves its arena of %llu bytes", (ull)f,
                             (ull)off, (ull)len, (ull)text_buf_len);
        if (len && !have_text) return plan_fail(e, SYDELTA_E_INVAL, "file %llu: NULL text arena", (ull)f);
        (*files)[f] = PFile{off, len, nc, nt};
        nc += chunks_of(len);  // each below 2^58, nfiles below 2^32: checked below before it can wrap
        nt += ptiles_of(len);
        if (nc >= 0x7FFFFFFFull)
            return plan_fail(e, SYDELTA_E_INVAL, "the batch holds more than 2^31 chunks of text at file %llu: split it",
                             (ull)f);
    }
    *nchunks = nc;
    *ntiles = nt;
    return SYDELTA_OK;
}

// "file F: checksum JSON: not serde's compact form at byte P" /
// "file F: checksum JSON: entry at byte P is not block I of a signature with block size B"
// (w: the device's status word; entry: the file's first entry off the layout, which the parse
// stage reports beside the status word).
inline std::string refusal_message(uint64_t f, uint64_t w, uint64_t entry, uint64_t bs) {
    typedef unsigned long long ull;
    char buf[200];
    if (w & kLayoutBit)
        snprintf(buf, sizeof buf, "file %llu: checksum JSON: entry at byte %llu is not block %llu of a signature with block size %llu",
                 (ull)f, (ull)(w & ~kLayoutBit), (ull)entry, (ull)bs);
    else
        snprintf(buf, sizeof buf, "file %llu: checksum JSON: not serde's compact form at byte %llu", (ull)f, (ull)w);
    return buf;
}

}  // namespace sigb

// The launches (sydelta_sigbatch.hip).  All pointers are device memory.
struct Profiler;
struct SigbWArgs {
    const uint32_t* weak;
    const uint64_t* strong;
    const sigb::WFile* files;  // nfiles
    uint64_t nfiles, ntiles, bs;
    uint64_t* tlen;            // ntiles + 1: the tiles' lengths (the trailing one 0), then their scan
    uint64_t* toff;
    uint64_t* pad;             // nfiles: text_len rounded up to 16
    uint64_t* text_off;        // nfiles, then text_len (nfiles): one copy back
    uint64_t* text_len;
};
// tlen, toff, text_len, text_off of every file.
hipError_t launch_sigb_len(const SigbWArgs& a, hipStream_t s, Profiler* prof);
// The texts, if out_cap holds them (decided on the device from text_off / text_len).
hipError_t launch_sigb_write(const SigbWArgs& a, uint8_t* d_out, uint64_t out_cap, hipStream_t s, Profiler* prof);

struct SigbPArgs {
    const uint8_t* text;       // the text arena
    const sigb::PFile* files;  // nfiles
    uint64_t nfiles, nchunks, ntiles, bs;
    uint64_t* cnt;             // nchunks + 1: '{' per chunk (the trailing one 0), then their scan
    uint64_t* rank;
    uint64_t* sig_off;         // nfiles each, then one entry (the sum of nblocks): one copy back
    uint64_t* nblocks;
    uint64_t* last;
    uint64_t* status;
    uint64_t* lay_i;           // the first entry of a file that breaks the layout
    uint64_t* need;
};
// staged: the waves read their tile from LDS; else from global memory (kept for measuring one
// against the other, tools/sig_batch_bench.py).
hipError_t launch_sigpb_count(const SigbPArgs& a, bool staged, hipStream_t s, Profiler* prof);
// The SoA, if cap holds the batch's entries (decided on the device from *need); the statuses and
// last sizes in either case.
hipError_t launch_sigpb_parse(const SigbPArgs& a, uint32_t* d_weak, uint64_t* d_strong, uint64_t cap, bool staged,
                              hipStream_t s, Profiler* prof);
}  // namespace sydelta
