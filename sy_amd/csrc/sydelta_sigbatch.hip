// sydelta_sigbatch.hip — K7sb / K7pb: the kernels of the batched signature JSON writer and
// parser (sydelta_sigbatch.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "sydelta_sigbatch.hpp"
#include "sydelta_internal.hpp"

namespace sydelta {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) u32x4 g_u32x4;
typedef __attribute__((address_space(3))) uint8_t lds_u8;
typedef __attribute__((address_space(3))) uint32_t lds_u32;

__device__ __forceinline__ void lds_fence() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// The tile of this wave / workgroup is wave-uniform: say so, and the bisection over the file
// table and the file's record are scalar loads.
__device__ __forceinline__ uint64_t uniform(uint64_t v) {
    return (uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)v) |
           ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(v >> 32)) << 32);
}

// Sum over the workgroup's 256 threads; valid in every thread.  wsum: 4 words of LDS.
__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t* wsum) {
#pragma unroll
    for (int k = 32; k > 0; k >>= 1) v += (uint32_t)__shfl_xor((int)v, k, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    return wsum[0] + wsum[1] + wsum[2] + wsum[3];
}
// Exclusive scan over the workgroup's 256 threads and the total.
__device__ __forceinline__ uint32_t block_scan_excl(uint32_t v, uint32_t* wsum, uint32_t& total) {
    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)inc, k, 64);
        if (lane >= (uint32_t)k) inc += o;
    }
    if (lane == 63) wsum[wid] = inc;
    __syncthreads();
    uint32_t pre = inc - v;
    for (uint32_t q = 0; q < wid; ++q) pre += wsum[q];
    total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    return pre;
}

}  // namespace

// ---------------------------------------------------------------------------
// Writer: k_sigjson_len / k_sigjson_write's bodies per tile of one file
// ---------------------------------------------------------------------------
static_assert(sigjson::kTile == 256, "one entry per thread of a 256-thread workgroup");

__global__ __launch_bounds__(256) void k_sigb_len(SigbWArgs a) {
    __shared__ uint32_t wsum[4];
    const uint64_t tile = blockIdx.x;
    const uint64_t f = sigb::file_of_tile(a.files, a.nfiles, tile);
    const sigb::WFile F = a.files[f];
    const sigjson::SigArgs A = sigb::wargs_of(a.weak, a.strong, F, a.bs);
    const uint32_t tot = block_sum(sigb::wslot_len(A, tile - F.tbase, threadIdx.x), wsum);
    if (threadIdx.x == 0) {
        a.tlen[tile] = tot;
        if (tile == 0) a.tlen[a.ntiles] = 0;  // the trailing entry: its scan is the batch's total
    }
}

__global__ __launch_bounds__(256) void k_sigb_files(SigbWArgs a) {
    const uint64_t f = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= a.nfiles) return;
    const uint64_t l = sigb::wfile_len(a.files, a.nfiles, a.ntiles, a.toff, f);
    a.text_len[f] = l;
    a.pad[f] = sigb::pad16(l);
}

__global__ __launch_bounds__(256) void k_sigb_write(SigbWArgs a, uint8_t* out, uint64_t out_cap) {
    __shared__ uint32_t wsum[4];
    __shared__ __attribute__((aligned(16))) uint8_t stage[sigjson::kStage];
    if (a.text_off[a.nfiles - 1] + a.text_len[a.nfiles - 1] > out_cap) return;  // sizing only
    const uint64_t tile = blockIdx.x;
    const uint64_t f = sigb::file_of_tile(a.files, a.nfiles, tile);
    const sigb::WFile F = a.files[f];
    const sigjson::SigArgs A = sigb::wargs_of(a.weak, a.strong, F, a.bs);
    const uint32_t len = sigb::wslot_len(A, tile - F.tbase, threadIdx.x);
    uint32_t tot;
    const uint32_t off = block_scan_excl(len, wsum, tot);
    if (len) sigb::wslot_write(A, tile - F.tbase, threadIdx.x, stage + off);
    __syncthreads();
    // the length from the sizing pass placed the next tile: store exactly that
    tot = (uint32_t)a.tlen[tile];
    uint8_t* dst = out + a.text_off[f] + (a.toff[tile] - a.toff[F.tbase]);
    const uintptr_t c0 = (uintptr_t)dst & ~(uintptr_t)15, c1 = ((uintptr_t)dst + tot + 15) & ~(uintptr_t)15;
    for (uintptr_t c = c0 + 16ull * threadIdx.x; c < c1; c += 16ull * 256) sigjson::store_chunk(stage, tot, dst, c);
}

hipError_t launch_sigb_len(const SigbWArgs& a, hipStream_t s, Profiler* prof) {
    if (!a.nfiles) return hipSuccess;
    {
        ProfScope ps(prof, s, "k_sigb_len");
        hipLaunchKernelGGL(k_sigb_len, dim3((unsigned)a.ntiles), dim3(256), 0, s, a);
        if (hipError_t e = hipGetLastError()) return e;
    }
    if (hipError_t e = launch_exclusive_sum_u64(a.tlen, a.toff, a.ntiles + 1, s)) return e;
    {
        ProfScope ps(prof, s, "k_sigb_files");
        hipLaunchKernelGGL(k_sigb_files, dim3((unsigned)((a.nfiles + 255) / 256)), dim3(256), 0, s, a);
        if (hipError_t e = hipGetLastError()) return e;
    }
    return launch_exclusive_sum_u64(a.pad, a.text_off, a.nfiles, s);
}

hipError_t launch_sigb_write(const SigbWArgs& a, uint8_t* d_out, uint64_t out_cap, hipStream_t s, Profiler* prof) {
    if (!a.nfiles || !d_out) return hipSuccess;
    ProfScope ps(prof, s, "k_sigb_write");
    hipLaunchKernelGGL(k_sigb_write, dim3((unsigned)a.ntiles), dim3(256), 0, s, a, d_out, out_cap);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Parser
// ---------------------------------------------------------------------------
namespace {

// The text outside the staged span (not reached by well-formed text).  Not inlined, so that the
// compiler cannot turn the accessor's branch into a select that issues this load for every byte.
__device__ __noinline__ uint8_t sp_gload(const uint8_t* g, uint64_t p) { return g[p]; }

// A file's text with the wave's span [p0, p0 + n) in LDS: byte p0 at LDS byte ph of the rows.
struct SigText {
    const uint8_t* g;
    const lds_u8* l;
    uint64_t p0;
    uint32_t n, ph;
    __device__ __forceinline__ uint8_t operator[](uint64_t p) const {
        const uint64_t d = p - p0;
        if (__builtin_expect(d < n, 1)) return l[sigb::stage_off((uint32_t)d + ph)];
        return sp_gload(g, p);
    }
};

// Stage the span of the tile whose first chunk is c0 with aligned 16-byte loads: the granules
// from the one that holds the span's first byte to the one that holds its last, so nothing
// outside the granules of the text's first and last byte is read.  Granule k goes to LDS bytes
// stage_off(16 k) ..: a row of 64 bytes takes four, 4-byte aligned in rows of kRow = 68 bytes.
__device__ __forceinline__ SigText sp_stage(const uint8_t* t, uint64_t len, uint64_t c0, uint8_t* rows) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t p0 = sigb::span_p0(c0);
    const uint32_t n = sigb::span_len(len, c0, p0);
    const uintptr_t a0 = (uintptr_t)(t + p0);
    const uint32_t ph = (uint32_t)(a0 & 15);
    const uintptr_t A = a0 - ph;
    const uint32_t bytes = (ph + n + 15) & ~15u;  // <= kRows * 64
    for (uint32_t d = 16 * lane; d < bytes; d += 16 * 64) {
        const u32x4 v = *(const g_u32x4*)(A + d);
        lds_u32* w = (lds_u32*)(rows + sigb::stage_off(d));
        w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
    }
    lds_fence();
    return SigText{t, (const lds_u8*)rows, p0, n, ph};
}
static_assert(sigb::kRows * 64 >= ((15 + sigb::kSpan + 15) & ~15u), "the staged granules fit the rows");

struct PTile {
    uint64_t f, c0, nc;
    sigb::PFile F;
};
__device__ __forceinline__ bool tile_of_wave(const SigbPArgs& a, PTile& T) {
    const uint64_t tile = uniform((uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6));
    if (tile >= a.ntiles) return false;
    T.f = sigb::file_of_tile(a.files, a.nfiles, tile);
    T.F = a.files[T.f];
    T.c0 = (tile - T.F.tbase) * sigb::kTileChunks;
    T.nc = sigb::chunks_of(T.F.len);
    return true;
}

}  // namespace

template <bool kStaged>
__global__ __launch_bounds__(256) void k_sigpb_count(SigbPArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t st[kStaged ? 4 : 1][sigb::kRows * sigb::kRow];
    PTile T;
    if (!tile_of_wave(a, T)) return;  // whole waves only
    const uint8_t* t = a.text + T.F.off;
    const uint64_t c = T.c0 + (threadIdx.x & 63);
    if (kStaged) {
        const SigText x = sp_stage(t, T.F.len, T.c0, st[threadIdx.x >> 6]);
        if (c < T.nc) a.cnt[T.F.cbase + c] = sigb::count_chunk(x, T.F.len, c);
    } else {
        if (c < T.nc) a.cnt[T.F.cbase + c] = sigb::count_chunk(t, T.F.len, c);
    }
}

__global__ __launch_bounds__(256) void k_sigpb_sizes(SigbPArgs a) {
    const uint64_t f = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (f == 0) *a.need = a.rank[a.nchunks];
    if (f >= a.nfiles) return;
    sigb::sizes_file(a.files[f], a.rank, a.sig_off[f], a.nblocks[f], a.last[f], a.status[f], a.lay_i[f]);
}

template <bool kStaged>
__global__ __launch_bounds__(256) void k_sigpb_parse(SigbPArgs a, uint32_t* weak, uint64_t* strong, uint64_t cap) {
    __shared__ __attribute__((aligned(16))) uint8_t st[kStaged ? 4 : 1][sigb::kRows * sigb::kRow];
    PTile T;
    if (!tile_of_wave(a, T)) return;
    const uint64_t* rank = a.rank + T.F.cbase;
    const uint64_t c1 = T.c0 + sigb::kTileChunks < T.nc ? T.c0 + sigb::kTileChunks : T.nc;
    // a tile without a '{' has nothing to parse; the head is chunk 0's
    if (T.c0 && rank[c1] == rank[T.c0]) return;  // wave-uniform
    if (!(weak && strong && cap >= *a.need)) weak = nullptr, strong = nullptr;  // the size query
    const uint8_t* t = a.text + T.F.off;
    const uint64_t c = T.c0 + (threadIdx.x & 63);
    const uint64_t sig_off = a.sig_off[T.f], n = a.nblocks[T.f];
    uint64_t last = UINT64_MAX, lay_i = sigb::kNoBad, w = sigb::kNoBad;
    if (kStaged) {
        const SigText x = sp_stage(t, T.F.len, T.c0, st[threadIdx.x >> 6]);
        if (c < T.nc) w = sigb::parse_chunk(x, T.F.len, c, rank[c] - sig_off, n, a.bs, sig_off, weak, strong, &last, &lay_i);
    } else {
        if (c < T.nc) w = sigb::parse_chunk(t, T.F.len, c, rank[c] - sig_off, n, a.bs, sig_off, weak, strong, &last, &lay_i);
    }
    if (last != UINT64_MAX) a.last[T.f] = last;
    if (w != sigb::kNoBad) atomicMin((unsigned long long*)&a.status[T.f], (unsigned long long)w);
    if (lay_i != sigb::kNoBad) atomicMin((unsigned long long*)&a.lay_i[T.f], (unsigned long long)lay_i);
}

hipError_t launch_sigpb_count(const SigbPArgs& a, bool staged, hipStream_t s, Profiler* prof) {
    if (!a.nfiles) return hipSuccess;
    if (hipError_t e = hipMemsetAsync(a.cnt + a.nchunks, 0, 8, s)) return e;  // the trailing entry
    if (a.ntiles) {
        ProfScope ps(prof, s, "k_sigpb_count");
        const dim3 grid((unsigned)((a.ntiles + 3) / 4));
        if (staged) hipLaunchKernelGGL(k_sigpb_count<true>, grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL(k_sigpb_count<false>, grid, dim3(256), 0, s, a);
        if (hipError_t e = hipGetLastError()) return e;
    }
    if (hipError_t e = launch_exclusive_sum_u64(a.cnt, a.rank, a.nchunks + 1, s)) return e;
    ProfScope ps(prof, s, "k_sigpb_sizes");
    hipLaunchKernelGGL(k_sigpb_sizes, dim3((unsigned)((a.nfiles + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_sigpb_parse(const SigbPArgs& a, uint32_t* d_weak, uint64_t* d_strong, uint64_t cap, bool staged,
                              hipStream_t s, Profiler* prof) {
    if (!a.nfiles || !a.ntiles) return hipSuccess;
    ProfScope ps(prof, s, "k_sigpb_parse");
    const dim3 grid((unsigned)((a.ntiles + 3) / 4));
    if (staged) hipLaunchKernelGGL(k_sigpb_parse<true>, grid, dim3(256), 0, s, a, d_weak, d_strong, cap);
    else hipLaunchKernelGGL(k_sigpb_parse<false>, grid, dim3(256), 0, s, a, d_weak, d_strong, cap);
    return hipGetLastError();
}

}  // namespace sydelta
