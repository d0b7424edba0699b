// sydelta_applybatch.hpp — sydelta_apply_delta_batch_device (K12): applier.rs:22-56 for a
// whole batch of (basis, delta) pairs in a few launches.
//
// Host: every file's ops are validated and, while they are flattened, merged: consecutive
// ops of one kind whose sources are contiguous become one run (the reference emits one Copy
// per matched block, generator.rs, so an edited file is a few runs, not a Copy per block).
// The runs reach the device in slices (kSliceRuns runs, kSliceSegs segments, one launch
// each); a segment is the part of one file's output that a slice's runs cover.
// Device: the destination is tiled, not the ops.  A workgroup takes a span of kSpan output
// bytes of one segment (spans are cut at 16-byte boundaries of the absolute address), finds
// the first run that overlaps it by binary search over the runs' destination offsets, and
// copies run by run: whole 16-byte destination granules are assembled from two aligned
// 16-byte source loads (the misalignment of source against destination is uniform per
// run), the partial granules at the two ends of a run's part are written byte by byte, so
// neighbouring runs, segments and files never race.
//
// The plan (host) and the span copy (host and device, over a memory policy) are shared
// with tests/csrc/apply_batch_check.cpp, which runs them on host memory.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/sydelta.h"

#define APPLYB_HD __host__ __device__ inline

namespace sydelta {
namespace applyb {

constexpr uint64_t kSpan = 16 * 1024;     // output bytes per workgroup and step (measured: DESIGN.md §11)
constexpr uint32_t kThreads = 256;
constexpr uint32_t kMaxGrid = 1u << 20;   // a workgroup per span up to here, then grid-strided
constexpr uint32_t kSliceRuns = 16384;    // per slice: 512 KiB of runs ...
constexpr uint32_t kSliceSegs = 16384;    // ... and 512 KiB of segments
constexpr uint32_t kRing = 4;             // pinned slices kept per thread

// out[dst, dst + len) = (from_basis ? basis : lit)[src, src + len); len > 0.
struct Run {
    uint64_t dst;  // absolute in d_out
    uint64_t src;  // absolute in its arena
    uint64_t len;
    uint64_t from_basis;
};
// The destination range of the runs [run0, run0 + nruns) of a slice: they belong to one
// file and their destinations are contiguous.  Its spans are tiles [tile0, next tile0).
struct Seg {
    uint64_t dst, len;
    uint64_t tile0;
    uint32_t run0, nruns;
};
constexpr uint64_t kSliceBytes = kSliceRuns * sizeof(Run) + kSliceSegs * sizeof(Seg);
static_assert(sizeof(Run) == 32 && sizeof(Seg) == 32, "table layout");

struct Q16 {
    uint32_t w[4];
};

APPLYB_HD uint32_t funnel(uint32_t hi, uint32_t lo, uint32_t r) {  // bytes [r, r + 4) of lo | hi << 32
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, r);
#else
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * r));
#endif
}

APPLYB_HD uint64_t seg_tiles(uintptr_t out_base, uint64_t dst, uint64_t len) {
    const uintptr_t a0 = out_base + dst;
    return (uint64_t)((a0 + len - (a0 & ~(uintptr_t)15) + kSpan - 1) / kSpan);
}

// Destination bytes [p0, p1) (absolute addresses, p0 < p1) from p + delta.  Mem: ld16 / st16
// on 16-byte aligned addresses, ldb / stb on bytes; ld16 is told the source bytes the piece
// needs (every granule it loads holds at least one of them).
template <class Mem>
APPLYB_HD void copy_piece(Mem& m, uint32_t tid, uint32_t nthr, uintptr_t p0, uintptr_t p1, uintptr_t delta) {
    const uintptr_t b0 = (p0 + 15) & ~(uintptr_t)15, b1 = p1 & ~(uintptr_t)15;
    if (b0 >= b1) {  // no whole granule
        for (uintptr_t x = p0 + tid; x < p1; x += nthr) m.stb(x, m.ldb(x + delta));
        return;
    }
    // the partial granules at the two ends: at most 15 bytes each
    for (uintptr_t x = p0 + tid; x < b0; x += nthr) m.stb(x, m.ldb(x + delta));
    for (uintptr_t x = b1 + tid; x < p1; x += nthr) m.stb(x, m.ldb(x + delta));
    const uint32_t sh = (uint32_t)(delta & 15), dq = sh >> 2, r = sh & 3;
    const uintptr_t need0 = p0 + delta, need1 = p1 + delta;
    for (uintptr_t c = b0 + 16ull * tid; c < b1; c += 16ull * nthr) {
        const uintptr_t sa = (c + delta) & ~(uintptr_t)15;
        const Q16 A = m.ld16(sa, need0, need1);
        Q16 B = {{0, 0, 0, 0}};
        if (sh) B = m.ld16(sa + 16, need0, need1);
        const uint32_t w[8] = {A.w[0], A.w[1], A.w[2], A.w[3], B.w[0], B.w[1], B.w[2], B.w[3]};
        Q16 o;
        // dword k of the output = bytes [sh + 4k, +4) of A|B
        switch (dq) {
            case 0: o = {{funnel(w[1], w[0], r), funnel(w[2], w[1], r), funnel(w[3], w[2], r), funnel(w[4], w[3], r)}}; break;
            case 1: o = {{funnel(w[2], w[1], r), funnel(w[3], w[2], r), funnel(w[4], w[3], r), funnel(w[5], w[4], r)}}; break;
            case 2: o = {{funnel(w[3], w[2], r), funnel(w[4], w[3], r), funnel(w[5], w[4], r), funnel(w[6], w[5], r)}}; break;
            default: o = {{funnel(w[4], w[3], r), funnel(w[5], w[4], r), funnel(w[6], w[5], r), funnel(w[7], w[6], r)}}; break;
        }
        m.st16(c, o);
    }
}

// Tile t of a slice (segs[0, nsegs), runs indexed by the segments), by nthr threads.
template <class Mem>
APPLYB_HD void copy_tile(Mem& m, uint32_t tid, uint32_t nthr, uint64_t t, const Run* runs, const Seg* segs,
                         uint32_t nsegs, uintptr_t basis, uintptr_t lit, uintptr_t out) {
    uint32_t lo = 0, hi = nsegs;  // the last segment with tile0 <= t
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (segs[mid].tile0 <= t) lo = mid; else hi = mid;
    }
    const Seg S = segs[lo];
    const uintptr_t a0 = out + S.dst, a1 = a0 + S.len;
    uintptr_t s0 = (a0 & ~(uintptr_t)15) + (uintptr_t)((t - S.tile0) * kSpan), s1 = s0 + kSpan;
    if (s0 < a0) s0 = a0;
    if (s1 > a1) s1 = a1;
    if (s0 >= s1) return;
    uint32_t rl = S.run0, rh = S.run0 + S.nruns;  // the last run that starts at or before s0
    while (rh - rl > 1) {
        const uint32_t mid = rl + (rh - rl) / 2;
        if (out + runs[mid].dst <= s0) rl = mid; else rh = mid;
    }
    for (uint32_t i = rl; i < S.run0 + S.nruns; ++i) {
        const Run R = runs[i];
        const uintptr_t r0 = out + R.dst, r1 = r0 + R.len;
        if (r0 >= s1) break;
        const uintptr_t p0 = r0 < s0 ? s0 : r0, p1 = r1 > s1 ? s1 : r1;
        if (p0 < p1) copy_piece(m, tid, nthr, p0, p1, (R.from_basis ? basis : lit) + R.src - r0);
    }
}

// ---------------------------------------------------------------------------
// The host plan
// ---------------------------------------------------------------------------
struct FileIn {
    const sydelta_op* ops;  // nullptr with nops == 0 is an empty delta
    uint64_t nops;
    bool has_delta;         // false: deltas[f] was NULL
    uint64_t basis_off, basis_len, lit_off, lit_len, out_off, out_cap;
};
struct Arenas {
    uint64_t basis_len, lit_len, out_len;
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

// Validate file f (its table entries, then every op, overflow-checked) and append its merged
// runs to `runs`; st receives what the single-file call reports.  On an error `runs` may hold
// runs of this file: nothing is applied after an error.
inline int plan_file(uint64_t f, const FileIn& in, const Arenas& A, std::vector<Run>& runs, sydelta_apply_stats* st,
                     Err* e) {
    typedef unsigned long long ull;
    if (in.basis_len > A.basis_len || in.basis_off > A.basis_len - in.basis_len)
        return plan_fail(e, SYDELTA_E_INVAL, "file %llu: basis range [%llu, +%llu) leaves its arena of %llu bytes", (ull)f,
                         (ull)in.basis_off, (ull)in.basis_len, (ull)A.basis_len);
    if (in.lit_len > A.lit_len || in.lit_off > A.lit_len - in.lit_len)
        return plan_fail(e, SYDELTA_E_INVAL, "file %llu: literal range [%llu, +%llu) leaves its arena of %llu bytes", (ull)f,
                         (ull)in.lit_off, (ull)in.lit_len, (ull)A.lit_len);
    if (in.out_cap > A.out_len || in.out_off > A.out_len - in.out_cap)
        return plan_fail(e, SYDELTA_E_INVAL, "file %llu: output range [%llu, +%llu) leaves its arena of %llu bytes", (ull)f,
                         (ull)in.out_off, (ull)in.out_cap, (ull)A.out_len);
    if (!in.has_delta) return plan_fail(e, SYDELTA_E_INVAL, "file %llu: NULL delta", (ull)f);
    const size_t first = runs.size();
    uint64_t pos = 0, literal = 0;
    for (uint64_t i = 0; i < in.nops; ++i) {
        const sydelta_op& o = in.ops[i];
        const bool cp = o.kind == SYDELTA_OP_COPY;
        if (o.kind != SYDELTA_OP_COPY && o.kind != SYDELTA_OP_DATA)
            return plan_fail(e, SYDELTA_E_INVAL, "file %llu: op %llu: unknown kind %u", (ull)f, (ull)i, (unsigned)o.kind);
        if (cp && (o.a > in.basis_len || o.b > in.basis_len - o.a))
            return plan_fail(e, SYDELTA_E_IO, "file %llu: op %llu: Copy{offset %llu, size %llu} past the end of the basis "
                             "(%llu bytes): failed to fill whole buffer", (ull)f, (ull)i, (ull)o.a, (ull)o.b,
                             (ull)in.basis_len);
        if (!cp && (o.a > in.lit_len || o.b > in.lit_len - o.a))
            return plan_fail(e, SYDELTA_E_INVAL, "file %llu: op %llu: Data [%llu, +%llu) outside the literal range "
                             "(%llu bytes)", (ull)f, (ull)i, (ull)o.a, (ull)o.b, (ull)in.lit_len);
        if (o.b > in.out_cap - pos)  // pos <= out_cap
            return plan_fail(e, SYDELTA_E_INVAL, "file %llu: op %llu: output needs more than its capacity of %llu bytes",
                             (ull)f, (ull)i, (ull)in.out_cap);
        if (o.b) {
            // inside their arenas (checked above): no overflow
            const uint64_t src = (cp ? in.basis_off : in.lit_off) + o.a;
            if (runs.size() > first && runs.back().from_basis == (uint64_t)cp && runs.back().src + runs.back().len == src)
                runs.back().len += o.b;
            else
                runs.push_back(Run{in.out_off + pos, src, o.b, (uint64_t)cp});
            pos += o.b;
            if (!cp) literal += o.b;
        }
    }
    st->operations_count = in.nops;
    st->literal_bytes = literal;
    st->bytes_written = pos;
    return SYDELTA_OK;
}

// A file's merged runs; the slices are cut from the files in order.
struct FileRuns {
    const Run* runs;
    uint64_t nruns;
};
struct Cursor {
    uint64_t file = 0, run = 0;
};
struct Slice {
    uint32_t nruns = 0, nsegs = 0;
    uint64_t ntiles = 0;
};
// The next slice from c on: ro[kSliceRuns] / so[kSliceSegs] filled (both nullptr: counted
// only).  False when nothing is left.
inline bool next_slice(const FileRuns* files, uint64_t nfiles, uintptr_t out_base, Cursor& c, Run* ro, Seg* so,
                       Slice* sl) {
    *sl = Slice();
    while (c.file < nfiles && sl->nruns < kSliceRuns && sl->nsegs < kSliceSegs) {
        const FileRuns& F = files[c.file];
        if (c.run >= F.nruns) {
            ++c.file;
            c.run = 0;
            continue;
        }
        const uint32_t n = (uint32_t)(F.nruns - c.run < kSliceRuns - sl->nruns ? F.nruns - c.run : kSliceRuns - sl->nruns);
        const Run &a = F.runs[c.run], &z = F.runs[c.run + n - 1];
        Seg s{a.dst, z.dst + z.len - a.dst, sl->ntiles, sl->nruns, n};
        if (ro) {
            memcpy(ro + sl->nruns, F.runs + c.run, n * sizeof(Run));
            so[sl->nsegs] = s;
        }
        sl->ntiles += seg_tiles(out_base, s.dst, s.len);
        sl->nruns += n;
        sl->nsegs += 1;
        c.run += n;
    }
    return sl->nsegs > 0;
}

}  // namespace applyb

struct Profiler;
// One slice (k_applyb): d_runs / d_segs as next_slice filled them.
hipError_t launch_applyb(const applyb::Run* d_runs, const applyb::Seg* d_segs, uint32_t nsegs, uint64_t ntiles,
                         const uint8_t* d_basis, const uint8_t* d_lit, uint8_t* d_out, hipStream_t s, Profiler* prof);

}  // namespace sydelta
