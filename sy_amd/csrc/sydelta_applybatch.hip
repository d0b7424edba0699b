// sydelta_applybatch.hip — K12: the batched device apply's span copy (sydelta_applybatch.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "sydelta_applybatch.hpp"
#include "sydelta_internal.hpp"

namespace sydelta {

namespace {

// The addresses are integers (absolute, so that any buffer alignment works): name the global
// address space, or the accesses compile to flat ones.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) u32x4 g_u32x4;
typedef __attribute__((address_space(1))) uint8_t g_u8;

struct DevMem {
    __device__ __forceinline__ applyb::Q16 ld16(uintptr_t p, uintptr_t, uintptr_t) const {
        const u32x4 v = *(const g_u32x4*)p;
        return applyb::Q16{{v.x, v.y, v.z, v.w}};
    }
    __device__ __forceinline__ void st16(uintptr_t p, const applyb::Q16& q) const {
        const u32x4 v = {q.w[0], q.w[1], q.w[2], q.w[3]};
        *(g_u32x4*)p = v;
    }
    __device__ __forceinline__ uint8_t ldb(uintptr_t p) const { return *(const g_u8*)p; }
    __device__ __forceinline__ void stb(uintptr_t p, uint8_t b) const { *(g_u8*)p = b; }
};

}  // namespace

// One workgroup per span of kSpan output bytes, grid-strided over the slice's tiles.
__global__ __launch_bounds__(applyb::kThreads) void k_applyb(const applyb::Run* __restrict__ runs,
                                                            const applyb::Seg* __restrict__ segs, uint32_t nsegs,
                                                            uint64_t ntiles, const uint8_t* basis, const uint8_t* lit,
                                                            uint8_t* out) {
    DevMem m;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x)
        applyb::copy_tile(m, threadIdx.x, applyb::kThreads, t, runs, segs, nsegs, (uintptr_t)basis, (uintptr_t)lit,
                          (uintptr_t)out);
}

hipError_t launch_applyb(const applyb::Run* d_runs, const applyb::Seg* d_segs, uint32_t nsegs, uint64_t ntiles,
                         const uint8_t* d_basis, const uint8_t* d_lit, uint8_t* d_out, hipStream_t s, Profiler* prof) {
    if (!nsegs || !ntiles) return hipSuccess;
    ProfScope ps(prof, s, "k_applyb");
    const unsigned grid = (unsigned)std::min<uint64_t>(ntiles, applyb::kMaxGrid);
    hipLaunchKernelGGL(k_applyb, dim3(grid), dim3(applyb::kThreads), 0, s, d_runs, d_segs, nsegs, ntiles, d_basis, d_lit,
                       d_out);
    return hipGetLastError();
}

}  // namespace sydelta
