// sydelta_unzstd.hip — K7u: the zstd frame decoder's kernels (bodies in sydelta_unzstd.hpp),
// separate launches on the caller's stream, no waits between workgroups inside a launch.
// Every kernel behind the scan leaves at once when the status word already names an error.
#include <algorithm>

#include "sydelta_internal.hpp"
#include "sydelta_unzstd.hpp"

namespace sydelta {
namespace {

using namespace unz;

__device__ __forceinline__ void report(unsigned long long* status, uint64_t block, uint32_t e) {
    if (e) atomicMin(status, (unsigned long long)ekey(block, e));
}

// Stage 1: one lane walks the Block_Header chain (blocks == nullptr: counts only).
__global__ __launch_bounds__(64) void k_unz_scan(const uint8_t* __restrict__ in, uint64_t len, Block* blocks,
                                                 uint64_t cap, Totals* tot, unsigned long long* status) {
    if (threadIdx.x) return;
    Totals t;
    const uint64_t st = scan(in, len, blocks, cap, t);
    *tot = t;
    if (st != kNoErr) atomicMin(status, (unsigned long long)st);
}

// Stage 2: what each block defines, one lane per block.
__global__ __launch_bounds__(64) void k_unz_tables(const uint8_t* __restrict__ in, Block* blocks, HufTab* huf,
                                                   FseTab* fse, unsigned long long* status) {
    if (threadIdx.x || *status != kNoErr) return;
    report(status, blockIdx.x, build_tables(in, blocks[blockIdx.x], huf, fse));
}

// Stage 3: one workgroup per Compressed block, tables in LDS.  Wave 0: the literals (a lane
// per Huffman stream, or every lane for Raw / RLE literals); wave 1, lane 0: the sequences.
__global__ __launch_bounds__(128) void k_unz_decode(const uint8_t* __restrict__ in, Block* blocks,
                                                    const HufTab* __restrict__ huf, const FseTab* __restrict__ fse,
                                                    uint8_t* lits, Seq* seqs, Hist* exit, unsigned long long* status) {
    __shared__ uint16_t s_huf[1u << kHufLogMax];
    __shared__ uint32_t s_fse[3][512];
    // one reading of the status word for the whole workgroup: other workgroups of this launch
    // may report while this one starts, and both waves must take the same way to the barrier
    __shared__ uint32_t s_skip;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) s_skip = *status != kNoErr;
    __syncthreads();
    if (s_skip) return;
    Block& k = blocks[blockIdx.x];
    if (k.type != 2) return;
    uint32_t hlog = 0, flog[3] = {0, 0, 0};
    if (k.lit_type >= 2) {
        const HufTab& T = huf[k.huf_slot];
        hlog = T.log;
        for (uint32_t i = tid; i < (1u << hlog); i += 128) s_huf[i] = T.e[i];
    }
    if (k.nseq) {
        for (uint32_t j = 0; j < 3; ++j) {
            const FseTab& T = fse[k.fse_slot[j]];
            flog[j] = T.log;
            for (uint32_t i = tid; i < (1u << flog[j]); i += 128) s_fse[j][i] = T.e[i];
        }
    }
    __syncthreads();
    if (tid < 64) {
        if (k.lit_type < 2) lit_fill(in, k, lits, tid, 64);
        else if (tid < k.lit_streams) report(status, blockIdx.x, lit_stream(in, k, s_huf, hlog, tid, lits));
    } else if (tid == 64) {
        report(status, blockIdx.x,
               seq_decode(in, k, s_fse[0], flog[0], s_fse[1], flog[1], s_fse[2], flog[2], seqs + k.seq_base,
                          exit[blockIdx.x]));
    }
}

// Stage 4: serial over blocks.
__global__ __launch_bounds__(64) void k_unz_stitch(const Block* __restrict__ blocks, uint64_t nb,
                                                   const Hist* __restrict__ exit, uint32_t* entry, uint64_t* bpos,
                                                   Totals* tot, unsigned long long* status) {
    if (threadIdx.x || *status != kNoErr) return;
    Totals t = *tot;
    const uint64_t st = stitch(blocks, nb, exit, entry, bpos, t);
    tot->out_len = t.out_len;
    if (st != kNoErr) atomicMin(status, (unsigned long long)st);
}

// Stage 4b: a workgroup per block over its sequences.
__global__ __launch_bounds__(256) void k_unz_resolve(const Block* __restrict__ blocks, const uint32_t* __restrict__ entry,
                                                     const uint64_t* __restrict__ bpos, Seq* seqs,
                                                     unsigned long long* status) {
    if (*status != kNoErr) return;
    const Block& k = blocks[blockIdx.x];
    if (k.type != 2) return;
    uint32_t bad = 0;
    for (uint32_t i = threadIdx.x; i < k.nseq; i += 256)
        if (const uint32_t e = resolve(bpos[blockIdx.x], entry + 3 * (uint64_t)blockIdx.x, seqs[k.seq_base + i])) bad = e;
    report(status, blockIdx.x, bad);
}

__global__ __launch_bounds__(256) void k_unz_place(uint64_t n, const uint8_t* __restrict__ in,
                                                   const Block* __restrict__ blocks, uint64_t nb,
                                                   const uint64_t* __restrict__ bpos, const Seq* __restrict__ seqs,
                                                   const uint8_t* __restrict__ lits, uint8_t* out, uint32_t* parent) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256)
        place(i, in, blocks, nb, bpos, seqs, lits, out, parent);
}

// Round r of the pointer doubling; changed[r] set when a parent moved.  A round behind one
// that moved nothing leaves at once.
__global__ __launch_bounds__(256) void k_unz_jump(uint64_t n, uint32_t* parent, uint32_t* changed, uint32_t r) {
    if (r && !changed[r - 1]) return;
    // a workgroup walks its own contiguous share upwards: the parents of a byte are mostly
    // bytes its workgroup has just shortened
    const uint64_t per = ((n + gridDim.x - 1) / gridDim.x + 255) & ~(uint64_t)255;
    const uint64_t b0 = blockIdx.x * per, b1 = b0 + per < n ? b0 + per : n;
    bool any = false;
    for (uint64_t i = b0 + threadIdx.x; i < b1; i += 256) any |= jump(i, parent);
    if (any) changed[r] = 1;
}

__global__ __launch_bounds__(256) void k_unz_gather(uint64_t n, const uint32_t* __restrict__ parent, uint8_t* out) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256)
        gather(i, parent, out);
}

unsigned grid_for(uint64_t n) { return (unsigned)std::min<uint64_t>((n + 255) / 256, 1u << 20); }
// The jump rounds loop over the bytes from a fixed grid (32 workgroups per CU): most of the 32
// launches find nothing left to do, and a launch that leaves at once costs its grid.
unsigned jump_grid(uint64_t n) { return (unsigned)std::min<uint64_t>((n + 255) / 256, 8192); }

}  // namespace

hipError_t launch_unz_scan(const uint8_t* d_in, uint64_t len, unz::Block* d_blocks, uint64_t cap, unz::Totals* d_tot,
                           unsigned long long* d_status, hipStream_t s, Profiler* prof) {
    ProfScope ps(prof, s, "k_unz_scan");
    hipLaunchKernelGGL(k_unz_scan, dim3(1), dim3(64), 0, s, d_in, len, d_blocks, cap, d_tot, d_status);
    return hipGetLastError();
}

hipError_t launch_unz_decode(const UnzArgs& a, hipStream_t s, Profiler* prof) {
    const unsigned nb = (unsigned)a.nb;
    {
        ProfScope ps(prof, s, "k_unz_tables");
        hipLaunchKernelGGL(k_unz_tables, dim3(nb), dim3(64), 0, s, a.in, a.blocks, a.huf, a.fse, a.status);
    }
    {
        ProfScope ps(prof, s, "k_unz_decode");
        hipLaunchKernelGGL(k_unz_decode, dim3(nb), dim3(128), 0, s, a.in, a.blocks, a.huf, a.fse, a.lits, a.seqs,
                           a.exit, a.status);
    }
    {
        ProfScope ps(prof, s, "k_unz_stitch");
        hipLaunchKernelGGL(k_unz_stitch, dim3(1), dim3(64), 0, s, a.blocks, a.nb, a.exit, a.entry, a.bpos, a.tot,
                           a.status);
    }
    {
        ProfScope ps(prof, s, "k_unz_resolve");
        hipLaunchKernelGGL(k_unz_resolve, dim3(nb), dim3(256), 0, s, a.blocks, a.entry, a.bpos, a.seqs, a.status);
    }
    return hipGetLastError();
}

hipError_t launch_unz_place(const UnzArgs& a, uint64_t n, uint8_t* d_out, uint32_t* d_parent, uint32_t* d_changed,
                            hipStream_t s, Profiler* prof) {
    if (!n) return hipSuccess;
    if (hipError_t e = hipMemsetAsync(d_changed, 0, 4 * kUnzRounds, s)) return e;
    {
        ProfScope ps(prof, s, "k_unz_place");
        hipLaunchKernelGGL(k_unz_place, dim3(grid_for(n)), dim3(256), 0, s, n, a.in, a.blocks, a.nb, a.bpos, a.seqs,
                           a.lits, d_out, d_parent);
    }
    {
        ProfScope ps(prof, s, "k_unz_jump");
        for (uint32_t r = 0; r < kUnzRounds; ++r)
            hipLaunchKernelGGL(k_unz_jump, dim3(jump_grid(n)), dim3(256), 0, s, n, d_parent, d_changed, r);
    }
    {
        ProfScope ps(prof, s, "k_unz_gather");
        hipLaunchKernelGGL(k_unz_gather, dim3(grid_for(n)), dim3(256), 0, s, n, d_parent, d_out);
    }
    return hipGetLastError();
}

}  // namespace sydelta
