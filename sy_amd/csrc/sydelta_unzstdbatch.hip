// sydelta_unzstdbatch.hip — K7ub: the batched zstd decoder's kernels (sydelta_unzstdbatch.hpp
// over the stage bodies of sydelta_unzstd.hpp), separate launches on the caller's stream, no
// waits between workgroups inside a launch.  A kernel behind the scan leaves a block, or a
// file, at once when that file's status word already names an error; other files go on.
#include <algorithm>

#include "sydelta_internal.hpp"
#include "sydelta_unzstdbatch.hpp"

namespace sydelta {
namespace {

using namespace unzb;

__device__ __forceinline__ void report(unsigned long long* status, uint64_t block, uint32_t e) {
    if (e) atomicMin(status, (unsigned long long)ekey(block, e));
}

// Stage 1: a lane per file walks its Block_Header chain for the counts.
__global__ __launch_bounds__(kLanes) void k_unzb_count(const uint8_t* __restrict__ in, const File* __restrict__ files,
                                                       uint64_t nfiles, Totals* tot, unsigned long long* status) {
    const uint64_t f = (uint64_t)blockIdx.x * kLanes + threadIdx.x;
    if (f >= nfiles) return;
    Totals t;
    uint64_t st;
    count_file(in, files[f], t, st);
    tot[f] = t;
    status[f] = st;
}

// Stage 1b: a lane per file writes its blocks into the shared table.
__global__ __launch_bounds__(kLanes) void k_unzb_scan(const uint8_t* __restrict__ in, const File* __restrict__ files,
                                                      const Base* __restrict__ bases, uint64_t nfiles,
                                                      const Totals* __restrict__ tot, Block* blocks, uint32_t* bfile,
                                                      unsigned long long* status) {
    const uint64_t f = (uint64_t)blockIdx.x * kLanes + threadIdx.x;
    if (f >= nfiles || status[f] != kNoErr) return;
    const uint64_t st = scan_file(in, files[f], bases[f], tot[f], (uint32_t)f, blocks, bfile);
    if (st != kNoErr) atomicMin(status + f, (unsigned long long)st);
}

// Stage 2: what each block defines, one lane per block.
__global__ __launch_bounds__(64) void k_unzb_tables(const uint8_t* __restrict__ in, const File* __restrict__ files,
                                                    const Base* __restrict__ bases, const uint32_t* __restrict__ bfile,
                                                    Block* blocks, HufTab* huf, FseTab* fse, unsigned long long* status) {
    if (threadIdx.x) return;
    const uint32_t f = bfile[blockIdx.x];
    if (status[f] != kNoErr) return;
    const Base B = bases[f];
    Block& k = blocks[blockIdx.x];
    adopt(k, B);
    report(status + f, blockIdx.x - B.nb, build_tables(frame_of(in, files[f]), k, huf, fse));
}

// Stage 3: one workgroup per Compressed block, as k_unz_decode: tables in LDS; wave 0 the
// literals, wave 1's lane 0 the sequences.
__global__ __launch_bounds__(128) void k_unzb_decode(const uint8_t* __restrict__ arena, const File* __restrict__ files,
                                                     const Base* __restrict__ bases, const uint32_t* __restrict__ bfile,
                                                     Block* blocks, const HufTab* __restrict__ huf,
                                                     const FseTab* __restrict__ fse, uint8_t* lits, Seq* seqs, Hist* exit,
                                                     unsigned long long* status) {
    __shared__ uint16_t s_huf[1u << kHufLogMax];
    __shared__ uint32_t s_fse[3][512];
    // one reading of the file's status word for the whole workgroup: other workgroups of this
    // launch may report while this one starts, and both waves must take the same way to the barrier
    __shared__ uint32_t s_skip;
    const uint32_t tid = threadIdx.x;
    const uint32_t f = bfile[blockIdx.x];
    if (tid == 0) s_skip = status[f] != kNoErr;
    __syncthreads();
    if (s_skip) return;
    Block& k = blocks[blockIdx.x];
    if (k.type != 2) return;
    const uint8_t* in = frame_of(arena, files[f]);
    const uint64_t b = blockIdx.x - bases[f].nb;
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
        else if (tid < k.lit_streams) report(status + f, b, lit_stream(in, k, s_huf, hlog, tid, lits));
    } else if (tid == 64) {
        report(status + f, b,
               seq_decode(in, k, s_fse[0], flog[0], s_fse[1], flog[1], s_fse[2], flog[2], seqs + k.seq_base,
                          exit[blockIdx.x]));
    }
}

// Stage 4: a lane per file, serial over that file's blocks.
__global__ __launch_bounds__(kLanes) void k_unzb_stitch(const Block* __restrict__ blocks, const Hist* __restrict__ exit,
                                                        const Base* __restrict__ bases, uint64_t nfiles, uint32_t* entry,
                                                        uint64_t* bpos, Totals* tot, unsigned long long* status) {
    const uint64_t f = (uint64_t)blockIdx.x * kLanes + threadIdx.x;
    if (f >= nfiles || status[f] != kNoErr) return;
    Totals t = tot[f];
    const uint64_t st = stitch_file(blocks, exit, entry, bpos, bases[f], f, t);
    tot[f].out_len = t.out_len;
    if (st != kNoErr) atomicMin(status + f, (unsigned long long)st);
}

// Stage 4b: a workgroup per block over its sequences.
__global__ __launch_bounds__(256) void k_unzb_resolve(const Block* __restrict__ blocks, const uint32_t* __restrict__ bfile,
                                                      const Base* __restrict__ bases, const uint32_t* __restrict__ entry,
                                                      const uint64_t* __restrict__ bpos, Seq* seqs,
                                                      unsigned long long* status) {
    const uint32_t f = bfile[blockIdx.x];
    if (status[f] != kNoErr) return;
    const Block& k = blocks[blockIdx.x];
    if (k.type != 2) return;
    const uint64_t at = bpos[(uint64_t)blockIdx.x + f];
    uint32_t bad = 0;
    for (uint32_t i = threadIdx.x; i < k.nseq; i += 256)
        if (const uint32_t e = resolve_in_text(at, f, entry + 3 * (uint64_t)blockIdx.x, seqs[k.seq_base + i])) bad = e;
    report(status + f, blockIdx.x - bases[f].nb, bad);
}

// Stage 4c: a lane per file: what it takes in the arena.
__global__ __launch_bounds__(kLanes) void k_unzb_sizes(const Totals* __restrict__ tot,
                                                       const unsigned long long* __restrict__ status, uint64_t nfiles,
                                                       uint64_t* text_len, uint64_t* pad) {
    const uint64_t f = (uint64_t)blockIdx.x * kLanes + threadIdx.x;
    if (f >= nfiles) return;
    const uint64_t n = text_len_of(tot[f], status[f]);
    text_len[f] = n;
    pad[f] = pad16(n);
}

// Stage 4d: a thread per block: its arena position; the first thread also leaves the total.
__global__ __launch_bounds__(256) void k_unzb_arena(uint64_t nb, const uint32_t* __restrict__ bfile,
                                                    const uint64_t* __restrict__ bpos,
                                                    const uint64_t* __restrict__ text_off,
                                                    const uint64_t* __restrict__ text_len,
                                                    const unsigned long long* __restrict__ status, uint64_t nfiles,
                                                    uint64_t* apos, uint64_t* need) {
    const uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (b == 0) *need = text_off[nfiles - 1] + text_len[nfiles - 1];
    if (b < nb) apos[b] = arena_pos(b, bfile, bpos, text_off, (const uint64_t*)status);
}

__global__ __launch_bounds__(256) void k_unzb_place(uint64_t n, const uint8_t* __restrict__ in,
                                                    const File* __restrict__ files, const uint32_t* __restrict__ bfile,
                                                    const Block* __restrict__ blocks, uint64_t nb,
                                                    const uint64_t* __restrict__ apos, const Seq* __restrict__ seqs,
                                                    const uint8_t* __restrict__ lits, uint8_t* out, uint32_t* parent) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256)
        place_at(i, in, files, bfile, blocks, nb, apos, seqs, lits, out, parent);
}

// Round r of the pointer doubling over the arena, as k_unz_jump.
__global__ __launch_bounds__(256) void k_unzb_jump(uint64_t n, uint32_t* parent, uint32_t* changed, uint32_t r) {
    if (r && !changed[r - 1]) return;
    const uint64_t per = ((n + gridDim.x - 1) / gridDim.x + 255) & ~(uint64_t)255;
    const uint64_t b0 = blockIdx.x * per, b1 = b0 + per < n ? b0 + per : n;
    bool any = false;
    for (uint64_t i = b0 + threadIdx.x; i < b1; i += 256) any |= jump(i, parent);
    if (any) changed[r] = 1;
}

__global__ __launch_bounds__(256) void k_unzb_gather(uint64_t n, const uint32_t* __restrict__ parent, uint8_t* out) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256)
        gather(i, parent, out);
}

unsigned grid_for(uint64_t n) { return (unsigned)std::min<uint64_t>((n + 255) / 256, 1u << 20); }
unsigned jump_grid(uint64_t n) { return (unsigned)std::min<uint64_t>((n + 255) / 256, 8192); }
unsigned file_grid(uint64_t nfiles) { return (unsigned)((nfiles + kLanes - 1) / kLanes); }

}  // namespace

hipError_t launch_unzb_count(const UnzbArgs& a, hipStream_t s, Profiler* prof) {
    ProfScope ps(prof, s, "k_unzb_count");
    hipLaunchKernelGGL(k_unzb_count, dim3(file_grid(a.nfiles)), dim3(kLanes), 0, s, a.in, a.files, a.nfiles, a.tot,
                       a.status);
    return hipGetLastError();
}

hipError_t launch_unzb_decode(const UnzbArgs& a, hipStream_t s, Profiler* prof) {
    const unsigned nb = (unsigned)a.nb, nf = file_grid(a.nfiles);
    if (nb) {
        {
            ProfScope ps(prof, s, "k_unzb_scan");
            hipLaunchKernelGGL(k_unzb_scan, dim3(nf), dim3(kLanes), 0, s, a.in, a.files, a.bases, a.nfiles, a.tot, a.blocks,
                               a.bfile, a.status);
        }
        {
            ProfScope ps(prof, s, "k_unzb_tables");
            hipLaunchKernelGGL(k_unzb_tables, dim3(nb), dim3(64), 0, s, a.in, a.files, a.bases, a.bfile, a.blocks, a.huf,
                               a.fse, a.status);
        }
        {
            ProfScope ps(prof, s, "k_unzb_decode");
            hipLaunchKernelGGL(k_unzb_decode, dim3(nb), dim3(128), 0, s, a.in, a.files, a.bases, a.bfile, a.blocks, a.huf,
                               a.fse, a.lits, a.seqs, a.exit, a.status);
        }
        {
            ProfScope ps(prof, s, "k_unzb_stitch");
            hipLaunchKernelGGL(k_unzb_stitch, dim3(nf), dim3(kLanes), 0, s, a.blocks, a.exit, a.bases, a.nfiles, a.entry,
                               a.bpos, a.tot, a.status);
        }
        {
            ProfScope ps(prof, s, "k_unzb_resolve");
            hipLaunchKernelGGL(k_unzb_resolve, dim3(nb), dim3(256), 0, s, a.blocks, a.bfile, a.bases, a.entry, a.bpos,
                               a.seqs, a.status);
        }
    }
    {
        ProfScope ps(prof, s, "k_unzb_sizes");
        hipLaunchKernelGGL(k_unzb_sizes, dim3(nf), dim3(kLanes), 0, s, a.tot, a.status, a.nfiles, a.text_len, a.pad);
    }
    if (hipError_t e = launch_exclusive_sum_u64(a.pad, a.text_off, a.nfiles, s)) return e;
    {
        ProfScope ps(prof, s, "k_unzb_arena");
        hipLaunchKernelGGL(k_unzb_arena, dim3(std::max(1u, grid_for(a.nb))), dim3(256), 0, s, a.nb, a.bfile, a.bpos,
                           a.text_off, a.text_len, a.status, a.nfiles, a.apos, a.need);
    }
    return hipGetLastError();
}

hipError_t launch_unzb_place(const UnzbArgs& a, uint64_t n, uint8_t* d_out, uint32_t* d_parent, uint32_t* d_changed,
                             hipStream_t s, Profiler* prof) {
    if (!n) return hipSuccess;
    if (!a.nb) return hipErrorInvalidValue;
    if (hipError_t e = hipMemsetAsync(d_changed, 0, 4 * kUnzRounds, s)) return e;
    {
        ProfScope ps(prof, s, "k_unzb_place");
        hipLaunchKernelGGL(k_unzb_place, dim3(grid_for(n)), dim3(256), 0, s, n, a.in, a.files, a.bfile, a.blocks, a.nb,
                           a.apos, a.seqs, a.lits, d_out, d_parent);
    }
    {
        ProfScope ps(prof, s, "k_unzb_jump");
        for (uint32_t r = 0; r < kUnzRounds; ++r)
            hipLaunchKernelGGL(k_unzb_jump, dim3(jump_grid(n)), dim3(256), 0, s, n, d_parent, d_changed, r);
    }
    {
        ProfScope ps(prof, s, "k_unzb_gather");
        hipLaunchKernelGGL(k_unzb_gather, dim3(grid_for(n)), dim3(256), 0, s, n, d_parent, d_out);
    }
    return hipGetLastError();
}

}  // namespace sydelta
