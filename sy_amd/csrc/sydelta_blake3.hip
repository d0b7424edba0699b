// sydelta_blake3.hip — BLAKE3-256 of files resident in HBM (integrity/blake3.rs:16-36, the
// `Cryptographic` arm of IntegrityVerifier::compute_file_checksum, integrity/mod.rs:100-112).
//
// k_b3_chunks: one lane per 1 KiB chunk (its 16 block compressions in registers), the
// chunks' bytes staged through LDS by coalesced 16-byte loads, then six levels of the tree
// inside the wave.  k_b3_tree: six more levels per launch over the chaining values the
// launch before it left.  Files of up to 64 chunks finish in k_b3_chunks.
#include <hip/hip_runtime.h>

#include "sydelta_blake3.hpp"

namespace sydelta {
namespace {
using namespace b3;

// LDS row of one chunk's current block: 5 granules of 16 bytes (64 bytes that start at
// any byte of the first granule) + 1 dword, so that the row stride is odd and the lanes'
// dword reads of their own rows fall on 32 different banks.
constexpr uint32_t kRowDw = 21;

// entry of slot t: the last one with start <= t (segs[0].start == 0)
__device__ __forceinline__ uint64_t find_seg(const B3Seg* __restrict__ segs, uint64_t nsegs, uint64_t t) {
    uint64_t lo = 0, hi = nsegs;
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (segs[mid].start <= t)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// Six levels of the tree inside the wave.  On entry every active lane holds node i (of n)
// of one level; on exit the lanes with i % 64 == 0 hold the nodes six levels up (i / 64 of
// ceil(n / 64)).  At level l the lanes with i % 2^(l+1) == 0 hold the left nodes; a left
// node with a right sibling takes it from lane ^ 2^l (B3Seg: start is aligned so that this
// is the lane of node i + 2^l) and becomes their parent, one without moves up unchanged.
__device__ __forceinline__ void wave_levels(uint32_t (&cv)[8], uint64_t i, uint64_t n, bool act, bool root) {
#pragma unroll 1
    for (uint32_t l = 0; l < 6; ++l) {
        uint32_t r[8], p[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            r[k] = (uint32_t)__shfl_xor((int)cv[k], 1 << l);
            p[k] = cv[k];
        }
        const uint64_t cnt = (n + (1ull << l) - 1) >> l;  // nodes of this level
        const bool join = act && (i & ((2ull << l) - 1)) == 0 && (i >> l) + 1 < cnt;
        parent(p, r, root && cnt == 2);
        if (join) {
#pragma unroll
            for (int k = 0; k < 8; ++k) cv[k] = p[k];
        }
    }
}

// after wave_levels: the result of a file of <= 64 nodes, or a node of the next launch
__device__ __forceinline__ void put_node(const uint32_t (&cv)[8], uint64_t i, const B3Seg& sg, bool act,
                                         uint32_t* __restrict__ cv_next, uint8_t* __restrict__ out) {
    if (!act || (i & 63)) return;
    uint4* dst = sg.n <= 64 ? (uint4*)(out + 32 * sg.out) : (uint4*)(cv_next + 8 * (sg.out + (i >> 6)));
    dst[0] = make_uint4(cv[0], cv[1], cv[2], cv[3]);
    dst[1] = make_uint4(cv[4], cv[5], cv[6], cv[7]);
}

// One wave per workgroup, lane = slot = chunk (B3Seg).  Block b of the wave's 64 chunks is
// 64 rows of 64 bytes, 1 KiB apart: four lanes load a row's four (16-byte aligned) granules,
// so an instruction reads 16 rows of 64 contiguous bytes; a row that starts off a 16-byte
// boundary needs a fifth granule, which its own lane loads.  Only granules that hold a byte
// of the chunk are loaded from the buffer (so no load leaves its pages).
// The granules of block b + 1 are in flight in registers while block b is compressed:
// a lane copies its message words out of LDS before it compresses, which frees the rows.
__global__ __launch_bounds__(64) void k_b3_chunks(const uint8_t* __restrict__ buf, const B3Seg* __restrict__ segs,
                                                  uint64_t nsegs, uint64_t first_chunk, uint32_t root,
                                                  uint32_t* __restrict__ cv_next, uint8_t* __restrict__ out) {
    __shared__ uint32_t rows[64 * kRowDw];
    __shared__ uint4 rowinfo[64];  // {first granule's offset from buf lo, hi, bytes from it to the chunk's end (0: none), -}
    const uint32_t lane = threadIdx.x;
    const uint64_t t = (uint64_t)blockIdx.x * 64 + lane;
    const B3Seg sg = segs[find_seg(segs, nsegs, t)];
    const uint64_t i = t - sg.start;
    const bool act = i < sg.n;
    const uint64_t left = act ? sg.len - (i << 10) : 0;  // act: i < chunks_of(len), so i * 1024 <= len
    const uint32_t clen = (uint32_t)(left < kChunkLen ? left : kChunkLen);
    const uint32_t nblk = act ? (clen ? (clen + 63) >> 6 : 1) : 0;
    const uint64_t poff = act ? sg.off + (i << 10) : 0;
    const uint32_t sh = (uint32_t)(((uintptr_t)buf + poff) & 15);
    const int64_t aoff = (int64_t)poff - sh;  // the first granule, from buf (global address space)
    const uint32_t vbytes = clen ? sh + clen : 0;
    rowinfo[lane] = make_uint4((uint32_t)aoff, (uint32_t)((uint64_t)aoff >> 32), vbytes, 0);
    __syncthreads();

    const uint32_t prow = lane >> 2, pcol = (lane & 3) << 4;
    // Every lane loads every time: a granule outside the chunk is replaced by one of the
    // table's (always mapped), so the loads sit in straight-line code and none waits for
    // another.  What such a granule holds never matters: it only feeds bytes past the
    // chunk's end, which the last block's mask clears (or a block no lane compresses).
    uint4 pf[5];
    const uint8_t* const safe = (const uint8_t*)segs;
    auto issue = [&](uint32_t b) {
        uint4 ri[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) ri[q] = rowinfo[q * 16 + prow];
        const uint32_t o = b * 64 + pcol;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            pf[q] = *(const uint4*)(o < ri[q].z ? buf + (int64_t)((uint64_t)ri[q].y << 32 | ri[q].x) + o : safe);
        pf[4] = *(const uint4*)(sh && b * 64 + 64 < vbytes ? buf + aoff + (b * 64 + 64) : safe);
    };
    auto commit = [&]() {
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            uint32_t* w = q < 4 ? rows + (q * 16 + prow) * kRowDw + (pcol >> 2) : rows + lane * kRowDw + 16;
            w[0] = pf[q].x, w[1] = pf[q].y, w[2] = pf[q].z, w[3] = pf[q].w;
        }
    };

    uint32_t cv[8];
    iv(cv);
    const uint64_t counter = first_chunk + i;
    const uint32_t last_flags = kChunkEnd | ((root && sg.n == 1) ? kRoot : 0u);
    const uint32_t* mine = rows + lane * kRowDw + (sh >> 2);
    issue(0);
    for (uint32_t b = 0;; ++b) {
        commit();
        __syncthreads();
        uint32_t d[17], m[16];
#pragma unroll
        for (int k = 0; k < 17; ++k) d[k] = mine[k];
#pragma unroll
        for (int k = 0; k < 16; ++k) m[k] = __builtin_amdgcn_alignbyte(d[k + 1], d[k], sh & 3);
        __syncthreads();
        const bool more = __ballot(b + 1 < nblk) != 0;
        if (more) issue(b + 1);
        if (b < nblk) {
            const uint32_t rest = clen - b * 64;  // an empty chunk: 0
            const uint32_t bl = rest < 64 ? rest : 64;
            if (bl < 64) {  // the input's last block: zero past its end
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    const int keep = (int)bl - 4 * k;
                    m[k] = keep >= 4 ? m[k] : keep <= 0 ? 0u : m[k] & ((1u << (8 * keep)) - 1);
                }
            }
            compress(cv, m, counter, bl, (b == 0 ? kChunkStart : 0u) | (b + 1 == nblk ? last_flags : 0u));
        }
        if (!more) break;
    }
    wave_levels(cv, i, sg.n, act, root != 0);
    put_node(cv, i, sg, act, cv_next, out);
}

// lane = slot = node of the array cv_in (slot-indexed, 8 words each)
__global__ __launch_bounds__(256) void k_b3_tree(const uint32_t* __restrict__ cv_in, const B3Seg* __restrict__ segs,
                                                 uint64_t nsegs, uint32_t root, uint32_t* __restrict__ cv_next,
                                                 uint8_t* __restrict__ out) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const B3Seg sg = segs[find_seg(segs, nsegs, t)];
    const uint64_t i = t - sg.start;
    const bool act = i < sg.n;
    uint32_t cv[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (act) {
        const uint4 a = ((const uint4*)(cv_in + 8 * t))[0], b = ((const uint4*)(cv_in + 8 * t))[1];
        cv[0] = a.x, cv[1] = a.y, cv[2] = a.z, cv[3] = a.w;
        cv[4] = b.x, cv[5] = b.y, cv[6] = b.z, cv[7] = b.w;
    }
    wave_levels(cv, i, sg.n, act, root != 0);
    put_node(cv, i, sg, act, cv_next, out);
}

}  // namespace

hipError_t launch_blake3(const uint8_t* d_buf, const B3Seg* segs, uint64_t nsegs, uint64_t total0,
                         const B3Seg* const* lv_segs, const uint64_t* lv_nsegs, const uint64_t* lv_total, int nlevels,
                         uint32_t* const d_cv[2], uint64_t first_chunk, bool root, uint8_t* d_out, hipStream_t s,
                         Profiler* prof) {
    if (!nsegs) return hipSuccess;
    if ((total0 + 63) / 64 > 0x7FFFFFFFull) return hipErrorInvalidValue;
    {
        ProfScope ps(prof, s, "k_b3_chunks");
        hipLaunchKernelGGL(k_b3_chunks, dim3((unsigned)((total0 + 63) / 64)), dim3(64), 0, s, d_buf, segs, nsegs,
                           first_chunk, root ? 1u : 0u, d_cv[0], d_out);
    }
    for (int j = 0; j < nlevels; ++j) {
        ProfScope ps(prof, s, "k_b3_tree");
        hipLaunchKernelGGL(k_b3_tree, dim3((unsigned)((lv_total[j] + 255) / 256)), dim3(256), 0, s, d_cv[j & 1],
                           lv_segs[j], lv_nsegs[j], root ? 1u : 0u, d_cv[(j + 1) & 1], d_out);
    }
    return hipGetLastError();
}

}  // namespace sydelta
