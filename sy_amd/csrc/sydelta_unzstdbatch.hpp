// sydelta_unzstdbatch.hpp — sydelta_zstd_decompress_batch_device (K7ub): the zstd frames of a
// whole batch decoded in one call, the texts packed into one arena (every text at a multiple
// of 16, the layout of sydelta_delta_batch_to_json_device).
//
// The decoder is sydelta_unzstd.hpp's: its stage bodies are called here, not copied.  What a
// batch adds is where a file's things lie.  The blocks of all files share one block table, one
// set of Huffman / FSE slots, one literal and one sequence scratch; a file's share of each
// starts at its Base (an exclusive sum of the per-file counts of the counting pass).  A block's
// `off` stays relative to its frame, and the frame's base is added where a body takes `in`; a
// block's file stands in an array beside the block table (bfile).  Every file has a status word
// of its own, with block numbers counted inside the file.
//
// Stages: count (lane per file) -> bases (host, from the one copy of the
// totals that sizes the scratch) -> scan (lane per file, the shared block table) -> tables,
// decode (per block, all files at once) -> stitch (lane per file) -> resolve (per block) ->
// sizes (lane per file: text_len, 0 for a refused file) -> exclusive sum of the padded lengths
// (text_off) -> arena positions of the blocks -> place, pointer doubling, gather over the
// arena's bytes, once per batch.
//
// The plan (host) and the bodies are shared with tests/csrc/unzstd_batch_check.cpp, which
// runs them on host memory.
#pragma once
#include <stdarg.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "../../include/sydelta.h"
#include "sydelta_unzstd.hpp"

#define UNZB_HD __host__ __device__ inline

namespace sydelta {
namespace unzb {

using namespace unz;

constexpr uint32_t kLanes = 64;               // files per workgroup of the lane-per-file kernels
constexpr uint32_t kStageBytes = 640u << 10;  // a pinned upload slot: 40 960 frames, 16 384 bases
constexpr uint32_t kStageSlots = 2;
constexpr uint64_t kArenaMax = 1ull << 32;    // parents are 32-bit arena positions

struct File {
    uint64_t off, len;  // the frame: d_in[off, +len)
};
// Where a file's share of the shared scratch starts.
struct Base {
    uint64_t nb, nhuf, nfse, nlit, nseq;
};
static_assert(sizeof(File) == 16 && sizeof(Base) == 40, "table layout");

UNZB_HD uint64_t pad16(uint64_t n) { return (n + 15) & ~(uint64_t)15; }

UNZB_HD const uint8_t* frame_of(const uint8_t* arena, const File& F) { return F.len ? arena + F.off : nullptr; }

// Stage 1, file F: its counts and its status.  A refused file counts as nothing.
UNZB_HD void count_file(const uint8_t* arena, const File& F, Totals& t, uint64_t& status) {
    status = scan(frame_of(arena, F), F.len, nullptr, 0, t);
    if (status != kNoErr) t = Totals{};
}

// Stage 1b, file f (not refused, t its counts): its blocks into the shared table behind B.nb,
// still in the frame's own numbering (adopt makes them absolute), and their file.
UNZB_HD uint64_t scan_file(const uint8_t* arena, const File& F, const Base& B, const Totals& t, uint32_t f, Block* blocks,
                           uint32_t* bfile) {
    Totals again;
    const uint64_t st = scan(frame_of(arena, F), F.len, blocks + B.nb, t.nb, again);
    for (uint64_t b = 0; b < t.nb; ++b) bfile[B.nb + b] = f;
    return st;
}

// Slot numbers, lit_base and seq_base of a block made absolute (once, by the tables stage).
UNZB_HD void adopt(Block& k, const Base& B) {
    if (k.type != 2) return;
    k.lit_base += B.nlit;
    k.seq_base += B.nseq;
    if (k.lit_type >= 2) k.huf_slot += (uint32_t)B.nhuf;
    if (k.nseq)
        for (uint32_t j = 0; j < 3; ++j) k.fse_slot[j] += (uint32_t)B.nfse;
}

// Stage 4, file f: entry histories from 1, 4, 8, block positions inside its own text (nb + 1
// of them, so the file's start at B.nb + f), t.out_len and the content size check.
UNZB_HD uint64_t stitch_file(const Block* blocks, const Hist* exit, uint32_t* entry, uint64_t* bpos, const Base& B,
                             uint64_t f, Totals& t) {
    return stitch(blocks + B.nb, t.nb, exit + B.nb, entry + 3 * B.nb, bpos + B.nb + f, t);
}

// Stage 4b, one sequence of block b of file f.
// INVARIANT (what lets parents be arena positions): text_pos is the block's position inside
// its own text, so resolve() refuses every offset that reaches before the text's first byte.
// A match byte at text position p >= text_pos + q.out + q.ll then has its parent at p - off >=
// 0 of the same text, i.e. at arena position text_off[f] + p - off >= text_off[f]: a chain
// never leaves [text_off[f], text_off[f] + text_len[f]), so it ends at a literal of its own
// file and never reads a pad byte or another file's text.
UNZB_HD uint32_t resolve_in_text(uint64_t text_pos, uint64_t f, const uint32_t* entry, Seq& q) {
#ifdef UNZSTDB_PLANT_BUG
    text_pos += 16 * f;  // as if measured from the arena's start (every text before it non-empty)
#else
    (void)f;
#endif
    return resolve(text_pos, entry, q);
}

// Stage 4c, file f: what it takes in the arena.
UNZB_HD uint64_t text_len_of(const Totals& t, uint64_t status) { return status == kNoErr ? t.out_len : 0; }

// Stage 4d, block b: its arena position.  The blocks of a refused file all stand at their
// file's (empty) place, so the table stays sorted and the bisection never ends in one.
UNZB_HD uint64_t arena_pos(uint64_t b, const uint32_t* bfile, const uint64_t* bpos, const uint64_t* text_off,
                           const uint64_t* status) {
    const uint32_t f = bfile[b];
    return text_off[f] + (status[f] == kNoErr ? bpos[b + f] : 0);
}

// Stage 5, arena byte i < out_need: the last block with apos <= i, and place() on that block
// alone with its frame as `in`.  A pad byte belongs to no block: it is neither read nor
// written, and its parent is itself, so that the doubling and the gather pass over it.
UNZB_HD void place_at(uint64_t i, const uint8_t* arena, const File* files, const uint32_t* bfile, const Block* blocks,
                      uint64_t nb, const uint64_t* apos, const Seq* seqs, const uint8_t* lits, uint8_t* out,
                      uint32_t* parent) {
    uint64_t lo = 0, hi = nb;
    while (hi - lo > 1) {
        const uint64_t m = (lo + hi) / 2;
        if (apos[m] <= i) lo = m;
        else hi = m;
    }
    if (apos[lo] > i || i - apos[lo] >= blocks[lo].regen) {
        parent[i] = (uint32_t)i;
        return;
    }
    place(i, frame_of(arena, files[bfile[lo]]), blocks + lo, 1, apos + lo, seqs, lits, out, parent);
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

// Every argument validated (overflow-checked) before a device is touched; the file table.
inline int plan(bool have_in, uint64_t in_buf_len, const uint64_t* frame_off, const uint64_t* frame_len, uint64_t nfiles,
                bool have_out, uint64_t out_buf_len, const uint64_t* text_off, const uint64_t* text_len,
                std::vector<File>* files, PlanErr* e) {
    typedef unsigned long long ull;
    if (!frame_off || !frame_len || !text_off || !text_len) return plan_fail(e, SYDELTA_E_INVAL, "NULL table");
    if (nfiles > UINT32_MAX) return plan_fail(e, SYDELTA_E_INVAL, "more than 2^32 - 1 files");
    if (!have_out && out_buf_len)
        return plan_fail(e, SYDELTA_E_INVAL, "NULL output arena of %llu bytes", (ull)out_buf_len);
    files->resize(nfiles);
    for (uint64_t f = 0; f < nfiles; ++f) {
        const uint64_t off = frame_off[f], len = frame_len[f];
        if (len > in_buf_len || off > in_buf_len - len)
            return plan_fail(e, SYDELTA_E_INVAL, "file %llu: frame [%llu, +%llu) leaves its arena of %llu bytes", (ull)f,
                             (ull)off, (ull)len, (ull)in_buf_len);
        if (len && !have_in) return plan_fail(e, SYDELTA_E_INVAL, "file %llu: NULL input arena", (ull)f);
        (*files)[f] = File{off, len};
    }
    return SYDELTA_OK;
}

// "file F: zstd frame: block B: <reason>"
inline std::string frame_message(uint64_t f, uint64_t status) {
    char buf[200];
    snprintf(buf, sizeof buf, "file %llu: zstd frame: block %llu: %s", (unsigned long long)f,
             (unsigned long long)(status >> 32), err_text((uint32_t)status));
    return buf;
}

// From the one copy of the per-file totals (refused files hold zeros): every file's bases,
// their sums, and a lower bound of the arena the batch needs (the headers' `least`, packed).
// The 4 GiB refusal comes here, before any scratch is sized from these sums.
inline int bases(const Totals* tot, uint64_t nfiles, std::vector<Base>* out, Base* sum, PlanErr* e) {
    typedef unsigned long long ull;
    out->resize(nfiles);
    Base s{};
    uint64_t least = 0;
    for (uint64_t f = 0; f < nfiles; ++f) {
        (*out)[f] = s;
        const Totals& t = tot[f];
        s.nb += t.nb, s.nhuf += t.nhuf, s.nfse += t.nfse, s.nlit += t.nlit, s.nseq += t.nseq;
        least = pad16(least) + t.least;  // each below 2^32 (scan), nfiles below 2^32: no overflow
    }
    if (least >= kArenaMax)
        return plan_fail(e, SYDELTA_E_INVAL, "the batch regenerates at least %llu bytes; split it below 4 GiB", (ull)least);
    if (s.nb > 0x7FFFFFFFull || s.nhuf > UINT32_MAX || s.nfse > UINT32_MAX)
        return plan_fail(e, SYDELTA_E_INVAL, "the batch holds %llu blocks: split it", (ull)s.nb);
    *sum = s;
    return SYDELTA_OK;
}

// After the second wait: the statuses, the tables and the total, in that order of precedence.
// status_out NULL: the lowest refused file is the call's error.
inline int finish(const uint64_t* toff, const uint64_t* tlen, const uint64_t* status, uint64_t need, uint64_t nfiles,
                  uint64_t* text_off, uint64_t* text_len, uint64_t* status_out, uint64_t* out_need, PlanErr* e) {
    for (uint64_t f = 0; f < nfiles; ++f) {
        text_off[f] = toff[f], text_len[f] = tlen[f];
        if (status_out) status_out[f] = status[f] == kNoErr ? 0 : status[f];
    }
    *out_need = need;
    if (!status_out)
        for (uint64_t f = 0; f < nfiles; ++f)
            if (status[f] != kNoErr) return plan_fail(e, SYDELTA_E_INVAL, "%s", frame_message(f, status[f]).c_str());
    if (need >= kArenaMax)
        return plan_fail(e, SYDELTA_E_INVAL, "the batch regenerates %llu bytes; split it below 4 GiB",
                         (unsigned long long)need);
    return SYDELTA_OK;
}

}  // namespace unzb

// The launches (sydelta_unzstdbatch.hip).  All pointers are device memory.
struct Profiler;
struct UnzbArgs {
    const uint8_t* in;         // the frame arena
    const unzb::File* files;   // nfiles
    const unzb::Base* bases;   // nfiles
    uint64_t nfiles;
    unz::Totals* tot;          // nfiles
    unsigned long long* status;  // nfiles
    unz::Block* blocks;        // nb
    uint32_t* bfile;           // nb
    uint64_t nb;
    unz::HufTab* huf;
    unz::FseTab* fse;
    uint8_t* lits;
    unz::Seq* seqs;
    unz::Hist* exit;           // nb
    uint32_t* entry;           // 3 nb
    uint64_t* bpos;            // nb + nfiles: positions inside the file's text
    uint64_t* apos;            // nb: arena positions
    uint64_t* text_off;        // nfiles, then text_len (nfiles), status, and the total: one copy back
    uint64_t* text_len;
    uint64_t* pad;             // nfiles: text_len rounded up to 16
    uint64_t* need;
};
// Stage 1: tot[f] and status[f] of every file.
hipError_t launch_unzb_count(const UnzbArgs& a, hipStream_t s, Profiler* prof);
// Stages 1b-4d: the block table, tables, entropy decode, stitch, offsets, sizes, positions.
hipError_t launch_unzb_decode(const UnzbArgs& a, hipStream_t s, Profiler* prof);
// Stages 5-6 over n = *need arena bytes; d_parent: n words, d_changed: kUnzRounds words.
hipError_t launch_unzb_place(const UnzbArgs& a, uint64_t n, uint8_t* d_out, uint32_t* d_parent, uint32_t* d_changed,
                             hipStream_t s, Profiler* prof);
}  // namespace sydelta
