// micro_b3_alu.hip — the ALU ceiling of BLAKE3 on this box (calibration, not product code).
// Every lane runs the compression function of sy_amd/csrc/sydelta_blake3.hpp on registers
// only (no loads, no LDS), at 1, 2, 4 and 8 waves per SIMD, and the program prints the
// cycles a SIMD spends per vector instruction of a 64-byte block (672: 7 rounds x 8 G x 12)
// and the bytes per second that rate would hash on the whole device, as one JSON line.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I sy_amd/csrc tools/micro_b3_alu.hip -o tools/micro_b3_alu
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "sydelta_blake3.hpp"

#define CK(x) do { hipError_t e = (x); if (e) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)

using namespace sydelta;

__global__ __launch_bounds__(64) void k_alu(uint32_t iters, uint32_t* out) {
    const uint32_t t = blockIdx.x * 64 + threadIdx.x;
    uint32_t cv[8], m[16];
    b3::iv(cv);
#pragma unroll
    for (int k = 0; k < 16; ++k) m[k] = t * (2 * k + 1);
    for (uint32_t i = 0; i < iters; ++i) {
        b3::compress(cv, m, i, 64, 0);
        m[0] ^= cv[7];
    }
    out[t] = cv[0] ^ cv[3];
}

int main() {
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount;
    const double ghz = prop.clockRate / 1e6;
    uint32_t* out;
    CK(hipMalloc(&out, (size_t)cus * 4 * 8 * 64 * 4));
    hipEvent_t a, b;
    CK(hipEventCreate(&a));
    CK(hipEventCreate(&b));
    const uint32_t iters = 2048;
    printf("{\"tool\": \"micro_b3_alu\", \"cus\": %d, \"clock_ghz\": %.3f, \"iters\": %u, \"runs\": [", cus, ghz, iters);
    for (int w = 1; w <= 8; w *= 2) {
        const unsigned grid = (unsigned)cus * 4 * w;  // w single-wave workgroups per SIMD
        hipLaunchKernelGGL(k_alu, dim3(grid), dim3(64), 0, 0, 64u, out);  // warm-up
        CK(hipDeviceSynchronize());
        float best = 1e30f;
        for (int r = 0; r < 3; ++r) {
            CK(hipEventRecord(a, 0));
            hipLaunchKernelGGL(k_alu, dim3(grid), dim3(64), 0, 0, iters, out);
            CK(hipEventRecord(b, 0));
            CK(hipEventSynchronize(b));
            float ms;
            CK(hipEventElapsedTime(&ms, a, b));
            if (ms < best) best = ms;
        }
        const double blocks = (double)grid * 64 * iters;          // 64-byte blocks compressed
        const double bytes_per_s = blocks * 64 / (best * 1e-3);
        const double simd_cycles = best * 1e-3 * ghz * 1e9;       // at the nominal clock
        const double cyc_per_inst = simd_cycles / ((double)w * iters * 672);
        printf("%s{\"waves_per_simd\": %d, \"ms\": %.4f, \"GBps\": %.1f, \"cycles_per_wave_instruction\": %.3f}",
               w == 1 ? "" : ", ", w, best, bytes_per_s / 1e9, cyc_per_inst);
    }
    printf("]}\n");
    CK(hipFree(out));
    return 0;
}
