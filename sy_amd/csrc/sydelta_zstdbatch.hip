// sydelta_zstdbatch.hip — K7zb: the batched zstd compressor's placement kernel
// (sydelta_zstdbatch.hpp).  The block coder's kernel, k_zstdb_block, stands beside
// k_zstd_block in sydelta_kernels.hip: both call the one coder there.
#include <hip/hip_runtime.h>

#include "sydelta_zstdbatch.hpp"
#include "sydelta_internal.hpp"

namespace sydelta {

namespace {

typedef __attribute__((address_space(1))) uint8_t g_u8;

struct DevMem {
    __device__ __forceinline__ uint8_t ldb(uintptr_t p) const { return *(const g_u8*)p; }
    __device__ __forceinline__ void stb(uintptr_t p, uint8_t b) const { *(g_u8*)p = b; }
};

}  // namespace

// One workgroup per block of the round.  The round's last workgroup also hands the next round
// its base: base_out is another word than base_in, so no workgroup of this launch reads it.
__global__ __launch_bounds__(zstdb::kThreads) void k_zstdb_frame(
    const uint8_t* arena, const zstdb::File* __restrict__ files, uint64_t nfiles, uint64_t b0,
    const uint8_t* slots, const uint32_t* __restrict__ size_in, const uint32_t* __restrict__ type_in,
    const uint64_t* __restrict__ off, const uint64_t* __restrict__ len64, const uint64_t* __restrict__ base_in,
    uint64_t* __restrict__ base_out, uint64_t* __restrict__ foff, uint8_t* out, uint64_t out_cap) {
    const uint32_t i = blockIdx.x;
    const zstdb::Block B = zstdb::block_at(files, nfiles, b0 + i);
    const uint32_t t = type_in[i], size = size_in[i];
    const uint64_t o = *base_in + off[i];
    if (threadIdx.x == 0) {
        if (B.first) foff[B.file] = o;
        if (i + 1 == gridDim.x) *base_out = o + len64[i];
    }
    const uintptr_t src = t == 2 ? (uintptr_t)slots + (uint64_t)i * zstd::kBlockMax : (uintptr_t)arena + B.at;
    DevMem m;
    zstdb::place_block(m, B, t, size, src, (uintptr_t)out, o, out_cap, threadIdx.x, zstdb::kThreads);
}

hipError_t launch_zstdb_frame(const uint8_t* d_in, const zstdb::File* d_files, uint64_t nfiles, uint64_t b0, uint32_t nb,
                              const uint8_t* d_slots, const uint32_t* d_size, const uint32_t* d_type,
                              const uint64_t* d_off, const uint64_t* d_len64, const uint64_t* d_base_in,
                              uint64_t* d_base_out, uint64_t* d_foff, uint8_t* d_out, uint64_t out_cap, hipStream_t s,
                              Profiler* prof) {
    if (!nb) return hipSuccess;
    if (!nfiles || d_base_in == d_base_out) return hipErrorInvalidValue;
    ProfScope ps(prof, s, "k_zstdb_frame");
    hipLaunchKernelGGL(k_zstdb_frame, dim3(nb), dim3(zstdb::kThreads), 0, s, d_in, d_files, nfiles, b0, d_slots, d_size,
                       d_type, d_off, d_len64, d_base_in, d_base_out, d_foff, d_out, out_cap);
    return hipGetLastError();
}

}  // namespace sydelta
