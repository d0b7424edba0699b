// sydelta_zstdbatch.hpp — sydelta_zstd_compress_batch_device (K7zb): the zstd frames
// (sydelta_zstd.hpp; ssh.rs:1009-1017) of a whole batch of texts in one call, the frames
// packed back to back.
//
// The unit of work is a 128 KiB block of some file; an empty text is one block of 0 bytes.
// Host: every text is validated and the per-file table {text_off, text_len, first_block} is
// made, first_block a prefix sum of the files' block counts.  Device: the blocks go through in
// rounds of at most N.  A workgroup per block finds its file by bisection (block_at) and codes
// the block with k_zstd_block's body (k_zstdb_block); a block's placed length is 3 + its
// content, plus the 14-byte frame header when it is its file's first (placed_len); an exclusive
// scan of those on top of a running base kept in device memory places the round, and a
// workgroup per block writes its headers and content straight into the arena (place_block,
// k_zstdb_frame), nothing at or past the arena's end.  The host reads nothing between rounds.
//
// The plan (host) and the per-thread bodies (host and device, over a memory policy) are
// shared with tests/csrc/zstd_batch_check.cpp, which runs them on host memory.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../../include/sydelta.h"
#include "sydelta_zstd.hpp"

#define ZSTDB_HD __host__ __device__ inline
#if defined(__clang__)
#define ZSTDB_UNROLL _Pragma("unroll")
#else
#define ZSTDB_UNROLL
#endif

namespace sydelta {
namespace zstdb {

constexpr uint32_t kThreads = 256;
constexpr uint64_t kRoundDefault = 4096;  // blocks per round (sydelta_zstd_compress_device's batch)
constexpr uint64_t kRoundMin = 64;        // a device short of memory: halved down to here
constexpr uint64_t kRoundMax = 1 << 20;
constexpr uint32_t kStageFiles = 32768;   // files per pinned upload slot (768 KiB)
constexpr uint32_t kStageSlots = 2;
constexpr uint32_t kFrameMin = zstd::kFrameHeader + 3;  // the frame of an empty text

struct File {
    uint64_t off, len;     // the text: d_in[off, +len)
    uint64_t first_block;  // the blocks of the files before it
};
static_assert(sizeof(File) == 24, "table layout");

ZSTDB_HD uint64_t blocks_of(uint64_t len) {  // any len: no sum that could wrap
    return len ? len / zstd::kBlockMax + (len % zstd::kBlockMax != 0) : 1;
}

// What a block takes in the arena: its header and content, behind the frame header when it is
// its file's first.
__host__ __device__ constexpr uint64_t placed_len(bool first, uint32_t size) {
    return (first ? zstd::kFrameHeader : 0u) + 3ull + size;
}

struct Block {
    uint64_t file;
    uint64_t at;        // its first byte in d_in
    uint64_t text_len;  // its file's
    uint32_t n;         // its bytes
    bool first, last;   // in its file
};
// Block b of the batch (b < files[nfiles - 1].first_block + blocks_of(files[nfiles - 1].len)):
// the last file with first_block <= b, by bisection.
ZSTDB_HD Block block_at(const File* files, uint64_t nfiles, uint64_t b) {
    uint64_t lo = 0, hi = nfiles;  // files[lo].first_block <= b < files[hi].first_block
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (files[mid].first_block <= b) lo = mid; else hi = mid;
    }
    const File F = files[lo];
    const uint64_t k = b - F.first_block, nb = blocks_of(F.len), at = k * zstd::kBlockMax;
    Block B;
    B.file = lo;
    B.at = F.off + at;
    B.text_len = F.len;
    B.n = (uint32_t)(F.len - at < zstd::kBlockMax ? F.len - at : zstd::kBlockMax);
    B.first = k == 0;
    B.last = k + 1 == nb;
    return B;
}

// Thread tid of nthr places block B at arena offset o (the round's base + the block's scan):
// the frame header when it is its file's first, the block header, and `size` content bytes
// from src (Raw: the text; RLE: its first byte; Compressed: the slot).  A byte at or past cap
// is not written.  Mem: ldb / stb on absolute addresses.
template <class Mem>
ZSTDB_HD void place_block(Mem& m, const Block& B, uint32_t type, uint32_t size, uintptr_t src, uintptr_t out, uint64_t o,
                          uint64_t cap, uint32_t tid, uint32_t nthr) {
    if (tid == 0) {
        uint8_t h[zstd::kFrameHeader + 3];
        uint32_t k = 0;
        if (B.first) {
            zstd::frame_header(h, B.text_len);
            k = zstd::kFrameHeader;
        }
        zstd::block_header(h + k, B.last, type, type == 2 ? size : B.n);
        k += 3;
        for (uint32_t i = 0; i < k; ++i)
            if (o + i < cap) m.stb(out + o + i, h[i]);
    }
    const uint64_t c = o + placed_len(B.first, 0);
    const uint32_t lim = c >= cap ? 0u : (cap - c < size ? (uint32_t)(cap - c) : size);  // the bytes the arena holds
    const uintptr_t dst = out + c;
    for (uint32_t i = tid; i < lim; i += 8 * nthr) {  // eight loads in flight per thread, then their stores
        uint8_t v[8];
        ZSTDB_UNROLL
        for (uint32_t k = 0; k < 8; ++k) v[k] = i + k * nthr < lim ? m.ldb(src + i + k * nthr) : (uint8_t)0;
        ZSTDB_UNROLL
        for (uint32_t k = 0; k < 8; ++k)
            if (i + k * nthr < lim) m.stb(dst + i + k * nthr, v[k]);
    }
}

// ---------------------------------------------------------------------------
// The host plan
// ---------------------------------------------------------------------------
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

// Σ zstd::frame_bound(text_len[f]); UINT64_MAX on overflow or a NULL table with nfiles > 0.
inline uint64_t batch_bound(const uint64_t* text_len, uint64_t nfiles) {
    if (!nfiles) return 0;
    if (!text_len) return UINT64_MAX;
    uint64_t total = 0;
    for (uint64_t f = 0; f < nfiles; ++f) {
        const uint64_t len = text_len[f], over = zstd::kFrameHeader + 3 * blocks_of(len);
        uint64_t b;
        if (__builtin_add_overflow(len, over, &b) || __builtin_add_overflow(total, b, &total)) return UINT64_MAX;
    }
    return total;
}

// Validate the tables (overflow-checked) and make the per-file table; *nblocks = the batch's
// blocks.  in_addr: d_in as an integer.
inline int plan(uintptr_t in_addr, uint64_t in_buf_len, const uint64_t* text_off, const uint64_t* text_len, uint64_t nfiles,
                std::vector<File>* files, uint64_t* nblocks, Err* e) {
    typedef unsigned long long ull;
    if (in_addr & 15) return plan_fail(e, SYDELTA_E_INVAL, "the input arena must be 16-byte aligned");
    files->resize(nfiles);
    uint64_t nb = 0;
    for (uint64_t f = 0; f < nfiles; ++f) {
        const uint64_t off = text_off[f], len = text_len[f];
        if (off & 15)
            return plan_fail(e, SYDELTA_E_INVAL, "file %llu: text offset %llu is not a multiple of 16", (ull)f, (ull)off);
        if (len > in_buf_len || off > in_buf_len - len)
            return plan_fail(e, SYDELTA_E_INVAL, "file %llu: text [%llu, +%llu) leaves its arena of %llu bytes", (ull)f,
                             (ull)off, (ull)len, (ull)in_buf_len);
        if (len && !in_addr) return plan_fail(e, SYDELTA_E_INVAL, "file %llu: NULL input arena", (ull)f);
        (*files)[f] = File{off, len, nb};
        nb += blocks_of(len);  // <= nfiles + in_buf_len * nfiles / 2^17: no overflow below 2^32 files
    }
    *nblocks = nb;
    return SYDELTA_OK;
}

// Blocks per round: the default, or the SYDELTA_ZSTD_BATCH knob's value.
inline uint64_t round_blocks(const char* knob) {
    uint64_t n = kRoundDefault;
    if (knob)
        if (const uint64_t v = strtoull(knob, nullptr, 10)) n = v < kRoundMax ? v : kRoundMax;
    return n;
}

}  // namespace zstdb

struct Profiler;
// Round [b0, b0 + nb) of the batch's blocks coded (k_zstdb_block, sydelta_kernels.hip): slot i
// of d_slots (zstd::kBlockMax bytes each) gets block b0 + i's content, d_size[i] its size,
// d_type[i] its type, d_len64[i] its placed length; d_lz holds nb * zstd::kSeqScratchBytes.
hipError_t launch_zstdb_blocks(const uint8_t* d_in, const zstdb::File* d_files, uint64_t nfiles, uint64_t b0, uint32_t nb,
                               uint8_t* d_slots, uint8_t* d_lz, uint32_t* d_size, uint32_t* d_type, uint64_t* d_len64,
                               hipStream_t s, Profiler* prof);
// With d_off the exclusive scan of d_len64: block b0 + i placed at d_out + *d_base_in + d_off[i]
// (k_zstdb_frame), nothing at or past out_cap; a file's first block stores its offset to
// d_foff[file]; *d_base_out = *d_base_in + the round's total (d_base_out != d_base_in).
hipError_t launch_zstdb_frame(const uint8_t* d_in, const zstdb::File* d_files, uint64_t nfiles, uint64_t b0, uint32_t nb,
                              const uint8_t* d_slots, const uint32_t* d_size, const uint32_t* d_type,
                              const uint64_t* d_off, const uint64_t* d_len64, const uint64_t* d_base_in,
                              uint64_t* d_base_out, uint64_t* d_foff, uint8_t* d_out, uint64_t out_cap, hipStream_t s,
                              Profiler* prof);

}  // namespace sydelta
