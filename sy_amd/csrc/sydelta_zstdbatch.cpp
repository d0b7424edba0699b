// sydelta_zstdbatch.cpp — sydelta_zstd_compress_batch_device: compress(delta_json,
// Compression::Zstd) (ssh.rs:1009-1017) for a batch of texts.  The host validates the tables
// and makes the per-file table (sydelta_zstdbatch.hpp), uploads it through pinned staging, and
// queues the rounds: blocks coded, placed by a scan on top of a base that stays on the device,
// written.  Nothing is read back between rounds; the call waits for the stream once, at its
// end, for the frames' offsets and the total.
#include <algorithm>

#include "sydelta_host.hpp"
#include "sydelta_stage.hpp"
#include "sydelta_zstdbatch.hpp"

using namespace sydelta;

namespace {

// The calling thread's pinned staging (sydelta_stage.hpp): kStageSlots slots of kStageFiles
// table entries, whatever the batch.
thread_local StageRing t_stage(zstdb::kStageSlots);
}  // namespace

extern "C" uint64_t sydelta_zstd_batch_bound(const uint64_t* text_len, uint64_t nfiles) {
    return zstdb::batch_bound(text_len, nfiles);
}

extern "C" int sydelta_zstd_compress_batch_device(int device, const uint8_t* d_in, uint64_t in_buf_len,
                                                  const uint64_t* text_off, const uint64_t* text_len, uint64_t nfiles,
                                                  uint8_t* d_out, uint64_t out_buf_len, uint64_t* frame_off,
                                                  uint64_t* frame_len, uint64_t* out_need, void* stream) try {
    typedef unsigned long long ull;
    if (!out_need) return fail(SYDELTA_E_INVAL, "NULL out_need");
    *out_need = 0;
    if (!nfiles) return SYDELTA_OK;
    if (!text_off || !text_len || !frame_off || !frame_len) return fail(SYDELTA_E_INVAL, "NULL table");
    if (nfiles > UINT32_MAX) return fail(SYDELTA_E_INVAL, "more than 2^32 - 1 files");
    if (!d_out && out_buf_len) return fail(SYDELTA_E_INVAL, "NULL output arena of %llu bytes", (ull)out_buf_len);
    static const bool host_timing = getenv("SYDELTA_HOST_TIMING") != nullptr;
    const auto t_start = std::chrono::steady_clock::now();

    // 1. the plan: every table entry validated before anything is queued
    std::vector<zstdb::File> files;
    uint64_t nblocks = 0;
    zstdb::Err err;
    if (zstdb::plan((uintptr_t)d_in, in_buf_len, text_off, text_len, nfiles, &files, &nblocks, &err))
        return fail(err.code, "%s", err.msg.c_str());
    SYDELTA_ENTER_DEVICE(device);
    int dev;
    hipStream_t s = call_stream(device, stream, &dev);
    const double t_plan = ms_since(t_start);

    // 2. one allocation: a round's slots and scratch, its tables, the file table, the frames'
    // offsets with the running base behind them
    uint64_t round = zstdb::round_blocks(getenv("SYDELTA_ZSTD_BATCH"));
    const size_t b_files = up256(nfiles * sizeof(zstdb::File)), b_foff = up256((nfiles + 3) * 8);
    uint64_t nb_max;
    size_t o_lz, o_size, o_type, o_len, o_off, o_files, o_foff;
    DevBuf buf;
    for (;;) {  // a device short of memory gets smaller rounds
        nb_max = std::min<uint64_t>(nblocks, round);
        o_lz = up256(nb_max * zstd::kBlockMax);
        o_size = o_lz + up256(nb_max * zstd::kSeqScratchBytes);
        o_type = o_size + up256(4 * nb_max);
        o_len = o_type + up256(4 * nb_max);
        o_off = o_len + up256(8 * nb_max);
        o_files = o_off + up256(8 * nb_max);
        o_foff = o_files + b_files;
        const hipError_t e = buf.alloc(o_foff + b_foff, s);
        if (e == hipSuccess) break;
        if (e != hipErrorOutOfMemory || round <= zstdb::kRoundMin) HIP_TRY(e);
        (void)hipGetLastError();
        round /= 2;
    }
    uint8_t* const B = buf.at<uint8_t>();
    uint8_t* const d_lz = B + o_lz;
    uint32_t* const d_size = (uint32_t*)(B + o_size);
    uint32_t* const d_type = (uint32_t*)(B + o_type);
    uint64_t* const d_len = (uint64_t*)(B + o_len);
    uint64_t* const d_off = (uint64_t*)(B + o_off);
    zstdb::File* const d_files = (zstdb::File*)(B + o_files);
    uint64_t* const d_foff = (uint64_t*)(B + o_foff);  // nfiles offsets, the total, two words of running base
    uint64_t* const d_total = d_foff + nfiles;
    uint64_t* const d_base = d_total + 1;

    // On an error after the first upload was queued the stream is drained before the scratch
    // (device) and the staging (host, reused by the next call) go away.
    StreamDrain drain(s);

    // 3. the file table, a staging slot at a time
    HIP_TRY(t_stage.open(dev, (size_t)zstdb::kStageSlots * zstdb::kStageFiles * sizeof(zstdb::File)));
    uint64_t slot_uses = 0;
    drain.armed = true;
    HIP_TRY(t_stage.upload(files.data(), files.size(), d_files, &slot_uses, s));
    HIP_TRY(hipMemsetAsync(d_base, 0, 16, s));

    // 4. the rounds: round r reads its base from word r % 2 and leaves the next one's in the
    // other word, the last round's in d_total
    CallProf cp;
    uint64_t rounds = 0;
    for (uint64_t b0 = 0; b0 < nblocks; b0 += round, ++rounds) {
        const uint32_t nb = (uint32_t)std::min<uint64_t>(round, nblocks - b0);
        const bool last = b0 + nb == nblocks;
        HIP_TRY(launch_zstdb_blocks(d_in, d_files, nfiles, b0, nb, B, d_lz, d_size, d_type, d_len, s, cp.get()));
        HIP_TRY(launch_exclusive_sum_u64(d_len, d_off, nb, s));
        HIP_TRY(launch_zstdb_frame(d_in, d_files, nfiles, b0, nb, B, d_size, d_type, d_off, d_len, d_base + rounds % 2,
                                   last ? d_total : d_base + (rounds + 1) % 2, d_foff, d_out, out_buf_len, s, cp.get()));
    }
    std::vector<uint64_t> res(nfiles + 1);
    HIP_TRY(hipMemcpyAsync(res.data(), d_foff, (nfiles + 1) * 8, hipMemcpyDeviceToHost, s));
    const double t_enq = ms_since(t_start);
    HIP_TRY(hipStreamSynchronize(s));  // the staging is reused by the next call
    drain.armed = false;
    if (host_timing)
        fprintf(stderr, "sydelta zstd batch: %llu files, %llu blocks, %llu rounds of %llu, plan %.3f ms, all queued %.3f ms, "
                "total %.3f ms\n", (ull)nfiles, (ull)nblocks, (ull)rounds, (ull)round, t_plan, t_enq, ms_since(t_start));

    // 5. the offsets must run up to the total in steps that a frame of that text can take: a
    // length outside means a sizing fault (the kernels wrote inside [0, total) or not at all)
    for (uint64_t f = 0; f < nfiles; ++f) {
        const uint64_t len = res[f + 1] - res[f], hi = zstd::frame_bound(text_len[f]);
        if (res[f + 1] < res[f] || len < zstdb::kFrameMin || len > hi || (f == 0 && res[0] != 0))
            return fail(SYDELTA_E_KERNEL, "file %llu: zstd frame sizing out of bounds (%llu not in [%u, %llu])", (ull)f,
                        (ull)len, zstdb::kFrameMin, (ull)hi);
    }
    for (uint64_t f = 0; f < nfiles; ++f) frame_off[f] = res[f], frame_len[f] = res[f + 1] - res[f];
    *out_need = res[nfiles];
    if (out_buf_len < *out_need && (d_out || out_buf_len))
        return fail(SYDELTA_E_INVAL, "arena holds %llu, the batch needs %llu", (ull)out_buf_len, (ull)*out_need);
    return SYDELTA_OK;
} catch (...) {
    return sydelta::host_exception();
}
