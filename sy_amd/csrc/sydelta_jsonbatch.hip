// sydelta_jsonbatch.hip — K7b: the batched Delta JSON writer's kernels (sydelta_jsonbatch.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "sydelta_jsonbatch.hpp"
#include "sydelta_internal.hpp"

namespace sydelta {

namespace {

// The addresses are integers (absolute, so that any buffer alignment works): name the global
// address space, or the accesses compile to flat ones.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) u32x4 g_u32x4;
typedef __attribute__((address_space(1))) uint32_t g_u32;
typedef __attribute__((address_space(1))) uint8_t g_u8;

struct DevMem {
    __device__ __forceinline__ jsonb::Q16 ld16(uintptr_t p) const {
        const u32x4 v = *(const g_u32x4*)p;
        return jsonb::Q16{{v.x, v.y, v.z, v.w}};
    }
    __device__ __forceinline__ uint32_t ld4(uintptr_t p) const { return *(const g_u32*)p; }
    __device__ __forceinline__ uint8_t ldb(uintptr_t p) const { return *(const g_u8*)p; }
    __device__ __forceinline__ void st16(uintptr_t p, const uint8_t* js) const { *(g_u32x4*)p = *(const u32x4*)js; }
    __device__ __forceinline__ void stb(uintptr_t p, uint8_t b) const { *(g_u8*)p = b; }
};

}  // namespace

// One wave per tile.
__global__ __launch_bounds__(jsonb::kThreads) void k_jsonb_len(const jsonb::Tile* __restrict__ tiles,
                                                              const jsonb::Pair* __restrict__ pairs, uint64_t t0,
                                                              uint64_t nt, const uint8_t* lit,
                                                              uint64_t* __restrict__ len) {
    const uint64_t w = ((uint64_t)blockIdx.x * jsonb::kThreads + threadIdx.x) >> 6;
    if (w >= nt) return;  // wave-uniform
    const jsonb::Tile T = tiles[t0 + w];
    DevMem m;
    uint32_t c = jsonb::size_lane(m, T, pairs, (uintptr_t)lit, threadIdx.x & 63);
#pragma unroll
    for (int k = 32; k > 0; k >>= 1) c += (uint32_t)__shfl_xor((int)c, k, 64);
    if ((threadIdx.x & 63) == 0) len[t0 + w] = (uint64_t)T.fixed + c;
}

__global__ __launch_bounds__(256) void k_jsonb_files(const jsonb::Tile* __restrict__ tiles,
                                                     const uint64_t* __restrict__ off, const uint64_t* __restrict__ len,
                                                     uint64_t ntiles, uint64_t nfiles, uint64_t* __restrict__ fstart) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= ntiles) return;
    if (tiles[t].flags & jsonb::kHead) fstart[tiles[t].file] = off[t];
    if (t + 1 == ntiles) fstart[nfiles] = off[t] + len[t];
}

__global__ __launch_bounds__(256) void k_jsonb_flen(const uint64_t* __restrict__ fstart, uint64_t nfiles,
                                                    uint64_t* __restrict__ tlen, uint64_t* __restrict__ pad) {
    const uint64_t f = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= nfiles) return;
    const uint64_t l = fstart[f + 1] - fstart[f];
    tlen[f] = l;
    pad[f] = (l + 15) & ~(uint64_t)15;
}

// One workgroup per tile, grid-strided.
__global__ __launch_bounds__(jsonb::kThreads) void k_jsonb_write(
    const jsonb::Tile* __restrict__ tiles, const jsonb::Pair* __restrict__ pairs, uint64_t ntiles, const uint8_t* lit,
    const uint64_t* __restrict__ off, const uint64_t* __restrict__ len, const uint64_t* __restrict__ fstart,
    const uint64_t* __restrict__ toff, const uint64_t* __restrict__ tlen, uint64_t nfiles, uint8_t* out,
    uint64_t out_cap) {
    __shared__ __attribute__((aligned(16))) uint8_t js[jsonb::kStage];
    __shared__ uint32_t wsum[4];
    if (toff[nfiles - 1] + tlen[nfiles - 1] > out_cap) return;  // the arena does not hold the texts: sizing only
    DevMem m;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const jsonb::Tile T = tiles[t];
        const uintptr_t oaddr = (uintptr_t)out + toff[T.file] + (off[t] - fstart[T.file]);
        const uint32_t ph = (uint32_t)(oaddr & 15);
        jsonb::Thread th;
        const uint32_t mine = jsonb::thread_len(m, T, pairs, (uintptr_t)lit, tid, th);
        // exclusive scan of `mine` over the workgroup
        uint32_t inc = mine;
#pragma unroll
        for (int k = 1; k < 64; k <<= 1) {
            const uint32_t o = (uint32_t)__shfl_up((int)inc, k, 64);
            if (lane >= (uint32_t)k) inc += o;
        }
        if (lane == 63) wsum[wid] = inc;
        __syncthreads();
        uint32_t pre = inc - mine;
        for (uint32_t q = 0; q < wid; ++q) pre += wsum[q];
        const uint32_t body = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        jsonb::thread_format(js, T, ph, pre, tid, th);
        __syncthreads();
        if (tid == 0) (void)jsonb::tile_close(js, T, pairs, ph, body);
        __syncthreads();
        // the end from the sizing pass: what placed the next tile
        jsonb::thread_store(m, js, ph, ph + (uint32_t)len[t], oaddr - ph, tid, jsonb::kThreads);
        __syncthreads();  // the staging and wsum are reused
    }
}

hipError_t launch_jsonb_len(const jsonb::Tile* d_tiles, const jsonb::Pair* d_pairs, uint64_t t0, uint64_t nt,
                            const uint8_t* d_lit, uint64_t* d_len, hipStream_t s, Profiler* prof) {
    if (!nt) return hipSuccess;
    ProfScope ps(prof, s, "k_jsonb_len");
    hipLaunchKernelGGL(k_jsonb_len, dim3((unsigned)((nt + 3) / 4)), dim3(jsonb::kThreads), 0, s, d_tiles, d_pairs, t0, nt,
                       d_lit, d_len);
    return hipGetLastError();
}

hipError_t launch_jsonb_files(const jsonb::Tile* d_tiles, const uint64_t* d_off, const uint64_t* d_len, uint64_t ntiles,
                              uint64_t nfiles, uint64_t* d_fstart, uint64_t* d_tlen, uint64_t* d_pad, hipStream_t s,
                              Profiler* prof) {
    if (!ntiles || !nfiles) return hipSuccess;
    {
        ProfScope ps(prof, s, "k_jsonb_files");
        hipLaunchKernelGGL(k_jsonb_files, dim3((unsigned)((ntiles + 255) / 256)), dim3(256), 0, s, d_tiles, d_off, d_len,
                           ntiles, nfiles, d_fstart);
        if (hipError_t e = hipGetLastError()) return e;
    }
    ProfScope ps(prof, s, "k_jsonb_flen");
    hipLaunchKernelGGL(k_jsonb_flen, dim3((unsigned)((nfiles + 255) / 256)), dim3(256), 0, s, d_fstart, nfiles, d_tlen,
                       d_pad);
    return hipGetLastError();
}

hipError_t launch_jsonb_write(const jsonb::Tile* d_tiles, const jsonb::Pair* d_pairs, uint64_t ntiles,
                              const uint8_t* d_lit, const uint64_t* d_off, const uint64_t* d_len,
                              const uint64_t* d_fstart, const uint64_t* d_toff, const uint64_t* d_tlen, uint64_t nfiles,
                              uint8_t* d_out, uint64_t out_cap, hipStream_t s, Profiler* prof) {
    if (!ntiles || !nfiles || !d_out) return hipSuccess;
    ProfScope ps(prof, s, "k_jsonb_write");
    const unsigned grid = (unsigned)std::min<uint64_t>(ntiles, jsonb::kMaxGrid);
    hipLaunchKernelGGL(k_jsonb_write, dim3(grid), dim3(jsonb::kThreads), 0, s, d_tiles, d_pairs, ntiles, d_lit, d_off,
                       d_len, d_fstart, d_toff, d_tlen, nfiles, d_out, out_cap);
    return hipGetLastError();
}

}  // namespace sydelta
