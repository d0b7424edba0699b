// sydelta_dparsebatch.hpp — sydelta_delta_batch_from_json_device (K7db): the Delta JSON texts
// of a whole batch parsed in one call, the receiver's step between
// sydelta_zstd_decompress_batch_device's text arena and sydelta_apply_delta_batch_device.
//
// The parser is sydelta_dparse.hpp's: its chunk bodies and the wave bodies around them
// (sydelta_kernels.hip: dp_count_wave / dp_place_wave / dp_parse_wave) are called here, not
// copied.  What a batch adds is where a file's things lie.  The chunks of all files share one
// chunk table (file f's at cbase[f], room for chunk_bound(text_len[f]) of them: the chunks at
// or behind the file's ops region count nothing, so the table is sized on the host without a
// wait), and one exclusive scan over it, with one trailing entry, ranks the ops and the
// literals of the whole batch: the ops of all files lie back to back in one op table, and file
// f's literal k is rank lbase[f] + k.  The entry behind a file's last chunk is the next file's
// first (or the trailing one): the file's total, which lits_before reads at lrank[nc].  A
// file's literals go to d_lit + lit_off[f] + (rank - lbase[f]) (lit_off: a second scan, over
// the per-file counts rounded up to 16), and a Data op's a = rank - lbase[f] (DArgs::lbase).
//
// Stages: tail (lane per file: head, tail, the per-file record) -> count (a
// wave per tile of up to 64 chunks of one file) -> two scans -> sizes (lane per file) -> scan
// of the padded literal counts (lit_off) -> [first wait: the counts size the op table and
// decide whether the arena holds the literals] -> place, parse (waves over the same tiles) ->
// [second wait: the records and the op table].
//
// The plan (host) and the per-file bodies are shared with tests/csrc/dparse_batch_check.cpp,
// which runs them on host memory.
#pragma once
#include <stdarg.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "../../include/sydelta.h"
#include "sydelta_dparse.hpp"

#define DPB_HD __host__ __device__ inline

namespace sydelta {
namespace dpb {

constexpr uint32_t kLanes = 64;               // files per workgroup of the lane-per-file kernels
constexpr uint32_t kTileChunks = 64;          // chunks per tile: one wave
constexpr uint32_t kStageBytes = 640u << 10;  // a pinned upload slot: 20 480 files
constexpr uint32_t kStageSlots = 2;
constexpr uint64_t kTailMax = 96;             // the tail is < 80 bytes: two u64 and the keys
// the shortest text: {"ops":[],"source_size":0,"block_size":0}
constexpr uint64_t kMinText = dparse::kHead + 16 + 17;
constexpr uint64_t kNoBad = dparse::kNoBad;

struct File {
    uint64_t off, len;  // the text: d_text[off, +len)
    uint64_t cbase;     // its first entry of the chunk table
    uint64_t tbase;     // its first tile
};
// What the tail stage finds; status: kNoBad, or the first byte that breaks the form (the tail
// stage's, then the smallest any chunk reports).  A file refused by the tail stage has e =
// kHead: no chunks.
struct Rec {
    uint64_t e;  // the ']' of the ops region
    uint64_t n, b;  // source_size, block_size
    uint64_t status;
};
static_assert(sizeof(File) == 32 && sizeof(Rec) == 32, "table layout");

DPB_HD uint64_t pad16(uint64_t n) { return (n + 15) & ~(uint64_t)15; }
DPB_HD uint64_t chunks_of(uint64_t e) { return (e - dparse::kHead + dparse::kChunk - 1) / dparse::kChunk; }
// The most chunks a text of len bytes can have: its ops region ends at least 33 bytes (the
// shortest tail) before the text does.
DPB_HD uint64_t chunk_bound(uint64_t len) { return len < kMinText ? 0 : chunks_of(len - (kMinText - dparse::kHead)); }
DPB_HD uint64_t tile_bound(uint64_t len) { return (chunk_bound(len) + kTileChunks - 1) / kTileChunks; }

// A u64 in serde's compact spelling at t[p, e): digits, no leading zero; returns the digits
// consumed or 0.
DPB_HD uint64_t tail_dec(const uint8_t* t, uint64_t p, uint64_t e, uint64_t& v) {
    uint64_t x = 0, k = 0;
    while (p + k < e && t[p + k] >= '0' && t[p + k] <= '9') {
        const uint64_t d = (uint64_t)(t[p + k] - '0');
        if (x > (UINT64_MAX - d) / 10) return 0;
        x = x * 10 + d;
        ++k;
    }
    if (!k || (k > 1 && t[p] == '0')) return 0;
    v = x;
    return k;
}
DPB_HD bool tail_is(const uint8_t* t, uint64_t p, uint64_t e, const char* key, uint64_t n) {
    if (e - p < n) return false;
    for (uint64_t i = 0; i < n; ++i)
        if (t[p + i] != (uint8_t)key[i]) return false;
    return true;
}
// The head and the tail of a text of len >= kMinText bytes: head = its first kHead bytes, tail
// = its last tl = min(len - kHead, kTailMax).  Both the single call (from two small copies) and
// the batch's tail stage (on the text itself) run this, so they accept the same texts and name
// the same byte.  Positions are the text's.
DPB_HD Rec tail_parse(const uint8_t* head, const uint8_t* tail, uint64_t len, uint64_t tl) {
    const char kHeadKey[] = "{\"ops\":[";
    const char kTailKey[] = "],\"source_size\":";
    const char kBs[] = ",\"block_size\":";
    const uint64_t nk = sizeof kTailKey - 1, nb = sizeof kBs - 1;
    Rec r{dparse::kHead, 0, 0, 0};
    if (!tail_is(head, 0, dparse::kHead, kHeadKey, dparse::kHead)) return r;  // status 0
    const uint64_t w0 = len - tl;
    uint64_t at = UINT64_MAX;  // the last "],\"source_size\":" in the tail
    for (uint64_t i = 0; i + nk <= tl; ++i)
        if (tail_is(tail, i, tl, kTailKey, nk)) at = i;
    if (at == UINT64_MAX) return r.status = w0, r;
    uint64_t q = at + nk, k;
    if (!(k = tail_dec(tail, q, tl, r.n))) return r.status = w0 + q, r;
    q += k;
    if (!tail_is(tail, q, tl, kBs, nb)) return r.status = w0 + q, r;
    q += nb;
    if (!(k = tail_dec(tail, q, tl, r.b))) return r.status = w0 + q, r;
    q += k;
    if (!(q + 1 == tl && tail[q] == '}')) return r.status = w0 + q, r;
    r.e = w0 + at;  // >= kHead: the tail starts at or behind the head's end
    r.status = kNoBad;
    return r;
}

// Stage 1, file F: its record.  A text shorter than the shortest Delta is refused at byte 0.
// Reads the text's first 8 and last <= 96 bytes only.
DPB_HD Rec tail_file(const uint8_t* arena, const File& F) {
    if (F.len < kMinText) return Rec{dparse::kHead, 0, 0, 0};
    const uint8_t* t = arena + F.off;
    const uint64_t tl = F.len - dparse::kHead < kTailMax ? F.len - dparse::kHead : kTailMax;
    Rec r = tail_parse(t, t + F.len - tl, F.len, tl);
    if (r.status != kNoBad) r.e = dparse::kHead;
    return r;
}

// The file of a tile: the last f with tbase <= tile (a file without tiles shares its tbase with
// the next one that has some, which stands behind it; tile < the total, so never a trailing one).
DPB_HD uint64_t file_of_tile(const File* files, uint64_t nfiles, uint64_t tile) {
    uint64_t lo = 0, hi = nfiles;
    while (hi - lo > 1) {
        const uint64_t m = (lo + hi) / 2;
        if (files[m].tbase <= tile) lo = m;
        else hi = m;
    }
    return lo;
}

// File F as the single parser sees it: its text alone, its own chunk grid (8 + 64c), and the
// rank of its first literal, which chunk_parse takes off a Data op's a.
DPB_HD dparse::DArgs args_of(const uint8_t* arena, const File& F, const Rec& R, uint64_t lbase) {
    dparse::DArgs a{arena + F.off, R.e, chunks_of(R.e)};
#ifdef DPARSEB_PLANT_BUG
    (void)lbase;  // op.a left arena-relative: right for the first file with literals only
#else
    a.lbase = lbase;
#endif
    return a;
}
// Where rank r of the batch's literals goes, as a base pointer for the file's waves: the file's
// rank lbase lands on d_lit + lit_off.  lit_off >= lbase (it sums the same counts, rounded up),
// so the pointer stays inside the arena.  dparse::lit_split phases on the absolute address
// (lit + rank), which is what this base keeps: the whole dwords of a wave's range are aligned
// stores wherever the file's range starts.
DPB_HD uint8_t* lit_base(uint8_t* d_lit, uint64_t lit_off, uint64_t lbase) {
    return d_lit ? d_lit + (lit_off - lbase) : nullptr;
}

// Stage 3, file F (orank / lrank: the scans of the whole chunk table): its ops, its literals
// and what they take in the arena.  A non-empty ops region without an op is refused at its
// first byte, as the single call does before it places anything.
DPB_HD void sizes_file(const File& F, const uint64_t* orank, const uint64_t* lrank, Rec& R, uint64_t& nops,
                       uint64_t& nlit) {
    const uint64_t c1 = F.cbase + chunk_bound(F.len);
    nops = orank[c1] - orank[F.cbase];
    nlit = lrank[c1] - lrank[F.cbase];
    if (R.status == kNoBad && R.e > dparse::kHead && nops == 0) R.status = dparse::kHead;
}

// ---------------------------------------------------------------------------
// The host plan
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

// Every argument validated (overflow-checked) before a device is touched; the file table with
// the files' places in the chunk table and the tile grid, and their totals.
inline int plan(bool have_text, uint64_t text_buf_len, const uint64_t* text_off, const uint64_t* text_len, uint64_t nfiles,
                bool have_lit, uint64_t lit_buf_len, const uint64_t* lit_off, const uint64_t* lit_len,
                std::vector<File>* files, uint64_t* nchunks, uint64_t* ntiles, PlanErr* e) {
    typedef unsigned long long ull;
    if (!text_off || !text_len || !lit_off || !lit_len) return plan_fail(e, SYDELTA_E_INVAL, "NULL table");
    if (nfiles > UINT32_MAX) return plan_fail(e, SYDELTA_E_INVAL, "more than 2^32 - 1 files");
    if (!have_lit && lit_buf_len)
        return plan_fail(e, SYDELTA_E_INVAL, "NULL literal arena of %llu bytes", (ull)lit_buf_len);
    files->resize(nfiles);
    uint64_t nc = 0, nt = 0;
    for (uint64_t f = 0; f < nfiles; ++f) {
        const uint64_t off = text_off[f], len = text_len[f];
        if (len > text_buf_len || off > text_buf_len - len)
            return plan_fail(e, SYDELTA_E_INVAL, "file %llu: text [%llu, +%llu) leaves its arena of %llu bytes", (ull)f,
                             (ull)off, (ull)len, (ull)text_buf_len);
        if (len && !have_text) return plan_fail(e, SYDELTA_E_INVAL, "file %llu: NULL text arena", (ull)f);
        (*files)[f] = File{off, len, nc, nt};
        nc += chunk_bound(len);  // each below 2^58, nfiles below 2^32: checked below before it can wrap
        nt += tile_bound(len);
        // the scans count their entries in an int, and a tile is a wave of a 4-wave workgroup
        if (nc >= 0x7FFFFFFFull)
            return plan_fail(e, SYDELTA_E_INVAL, "the batch holds more than 2^31 chunks of text at file %llu: split it", (ull)f);
    }
    *nchunks = nc;
    *ntiles = nt;
    return SYDELTA_OK;
}

// "file F: Delta JSON: not serde's compact form at byte P"
inline std::string refusal_message(uint64_t f, uint64_t at) {
    char buf[160];
    snprintf(buf, sizeof buf, "file %llu: Delta JSON: not serde's compact form at byte %llu", (unsigned long long)f,
             (unsigned long long)at);
    return buf;
}

}  // namespace dpb

// The launches (sydelta_kernels.hip, beside the single call's).  All pointers are device memory.
struct Profiler;
struct DpbArgs {
    const uint8_t* text;     // the text arena
    const dpb::File* files;  // nfiles
    uint64_t nfiles, nchunks, ntiles;
    dpb::Rec* recs;          // nfiles
    uint64_t* ocnt;          // nchunks + 1 each: op / literal starts per chunk, their exclusive scans
    uint64_t* lcnt;
    uint64_t* orank;
    uint64_t* lrank;
    uint64_t* lit_off;       // nfiles, then lit_len (nfiles) and nops (nfiles): one copy back
    uint64_t* lit_len;
    uint64_t* nops;
    uint64_t* pad;           // nfiles: lit_len rounded up to 16
};
// Stages 1-3: recs, the ranks, lit_off / lit_len / nops of every file.
hipError_t launch_dpb_count(const DpbArgs& a, hipStream_t s, Profiler* prof);
// Stages 4-5: d_pos and d_ops hold the batch's ops (the sum of nops); d_lit NULL: checked only.
hipError_t launch_dpb_parse(const DpbArgs& a, uint64_t* d_pos, sydelta_op* d_ops, uint8_t* d_lit, hipStream_t s,
                            Profiler* prof);
}  // namespace sydelta
