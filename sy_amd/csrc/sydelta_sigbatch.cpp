// sydelta_sigbatch.cpp — sydelta_checksums_batch_to_json_device and
// sydelta_checksums_batch_from_json_device: `sy-remote checksums` (sy-remote.rs:145-147) and the
// sender's parse of its line (ssh.rs:967-973) for a batch of files, the two steps between
// sydelta_signature_batch_device and sydelta_index_create_batch.  The host validates the tables,
// uploads the file table through pinned staging, queues every stage and waits once: the decision
// whether the caller's buffers hold the result is taken on the device.
#include <stdlib.h>

#include <algorithm>

#include "sydelta_sigbatch.hpp"
#include "sydelta_host.hpp"
#include "sydelta_stage.hpp"

using namespace sydelta;

namespace {
// The calling thread's pinned staging (sydelta_stage.hpp): kStageSlots slots of kStageBytes,
// whatever the batch.
thread_local StageRing t_wstage(sigb::kStageSlots);
thread_local StageRing t_pstage(sigb::kStageSlots);

// SYDELTA_SIGB_STAGE=0: the parser's waves read their text from global memory, not through LDS
// (the form tools/sig_batch_bench.py measures the staged one against; read per call).
bool parser_staged() {
    const char* e = getenv("SYDELTA_SIGB_STAGE");
    return !(e && e[0] == '0');
}
}  // namespace

#define ALLOC_TRY(buf, bytes, s)                                                                          \
    do {                                                                                                  \
        const hipError_t e_ = (buf).alloc((bytes), (s));                                                  \
        if (e_ != hipSuccess) {                                                                           \
            (void)hipGetLastError();                                                                      \
            return fail(e_ == hipErrorOutOfMemory ? SYDELTA_E_OOM : SYDELTA_E_KERNEL,                     \
                        "signature JSON batch: device allocation of %llu bytes failed: %s", (ull)(bytes), \
                        hipGetErrorString(e_));                                                           \
        }                                                                                                 \
    } while (0)

extern "C" uint64_t sydelta_checksums_batch_to_json_bound(const uint64_t* nblocks, const uint64_t* last_size,
                                                          uint64_t nfiles, uint64_t block_size) try {
    return sigb::wbound(nblocks, last_size, nfiles, block_size);
} catch (...) {
    return UINT64_MAX;
}

extern "C" int sydelta_checksums_batch_to_json_device(int device, const uint32_t* d_weak, const uint64_t* d_strong,
                                                      const uint64_t* nblocks, const uint64_t* last_size, uint64_t nfiles,
                                                      uint64_t block_size, uint8_t* d_out, uint64_t out_buf_len,
                                                      uint64_t* text_off, uint64_t* text_len, uint64_t* out_need,
                                                      void* stream) try {
    typedef unsigned long long ull;
    if (!out_need) return fail(SYDELTA_E_INVAL, "NULL out_need");
    *out_need = 0;
    if (!nfiles) return SYDELTA_OK;
    if (!text_off || !text_len) return fail(SYDELTA_E_INVAL, "NULL table");

    // 1. every table entry validated before a device is touched
    std::vector<sigb::WFile> files;
    std::vector<uint64_t> lo, hi;
    uint64_t nentries = 0, ntiles = 0;
    sigb::PlanErr err;
    if (sigb::wplan(d_weak && d_strong, nblocks, last_size, nfiles, block_size, &files, &lo, &hi, &nentries, &ntiles, &err))
        return fail(err.code, "%s", err.msg.c_str());
    SYDELTA_ENTER_DEVICE(device);
    int dev;
    hipStream_t s = call_stream(device, stream, &dev);
    CallProf cp;

    // 2. the tables: files, the tile lengths and their scan, the padded lengths, and what comes
    // back (text_off, text_len: one copy)
    const size_t nte = ntiles + 1;
    const size_t o_files = 0, o_tlen = o_files + up256(nfiles * sizeof(sigb::WFile)), o_toff = o_tlen + up256(nte * 8),
                 o_pad = o_toff + up256(nte * 8), o_res = o_pad + up256(nfiles * 8), b_all = o_res + up256(2 * nfiles * 8);
    DevBuf tab;
    // On an error after the first upload was queued the stream is drained before the scratch
    // (device) and the staging (host, reused by the next call) go away.
    StreamDrain drain(s);
    ALLOC_TRY(tab, b_all, s);
    uint8_t* const H = tab.at<uint8_t>();
    SigbWArgs a{};
    a.weak = d_weak, a.strong = d_strong;
    a.files = (sigb::WFile*)(H + o_files);
    a.nfiles = nfiles, a.ntiles = ntiles, a.bs = block_size;
    a.tlen = (uint64_t*)(H + o_tlen);
    a.toff = (uint64_t*)(H + o_toff);
    a.pad = (uint64_t*)(H + o_pad);
    a.text_off = (uint64_t*)(H + o_res);
    a.text_len = a.text_off + nfiles;

    HIP_TRY(t_wstage.open(dev, (size_t)sigb::kStageSlots * sigb::kStageBytes));
    uint64_t slot_uses = 0;
    drain.armed = true;
    HIP_TRY(t_wstage.upload(files.data(), files.size(), (sigb::WFile*)a.files, &slot_uses, s));

    // 3. size, place, write (the kernel decides whether the arena holds the texts), and the
    // offsets and lengths back: the one wait
    HIP_TRY(launch_sigb_len(a, s, cp.get()));
    HIP_TRY(launch_sigb_write(a, d_out, d_out ? out_buf_len : 0, s, cp.get()));
    std::vector<uint64_t> res(2 * nfiles);
    HIP_TRY(hipMemcpyAsync(res.data(), a.text_off, res.size() * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    drain.armed = false;

    // every text is bounded from both sides by its implied fields; a length outside the bounds
    // means a sizing fault (the kernel wrote inside [0, need) or not at all)
    for (uint64_t f = 0; f < nfiles; ++f)
        if (res[nfiles + f] < lo[f] || res[nfiles + f] > hi[f])
            return fail(SYDELTA_E_KERNEL, "file %llu: signature JSON sizing out of bounds (%llu not in [%llu, %llu])", (ull)f,
                        (ull)res[nfiles + f], (ull)lo[f], (ull)hi[f]);
    std::copy(res.begin(), res.begin() + nfiles, text_off);
    std::copy(res.begin() + nfiles, res.end(), text_len);
    *out_need = text_off[nfiles - 1] + text_len[nfiles - 1];
    return SYDELTA_OK;
} catch (...) {
    return sydelta::host_exception();
}

extern "C" int sydelta_checksums_batch_from_json_device(int device, const uint8_t* d_text, uint64_t text_buf_len,
                                                        const uint64_t* text_off, const uint64_t* text_len,
                                                        uint64_t nfiles, uint64_t block_size, uint32_t* d_weak,
                                                        uint64_t* d_strong, uint64_t sig_cap, uint64_t* sig_off,
                                                        uint64_t* nblocks, uint64_t* last_size, uint64_t* file_status,
                                                        uint64_t* sig_need, void* stream) try {
    typedef unsigned long long ull;
    if (!sig_need) return fail(SYDELTA_E_INVAL, "NULL sig_need");
    *sig_need = 0;
    if (!nfiles) return SYDELTA_OK;
    if (!sig_off || !nblocks || !last_size) return fail(SYDELTA_E_INVAL, "NULL table");

    // 1. every table entry validated before a device is touched
    std::vector<sigb::PFile> files;
    uint64_t nchunks = 0, ntiles = 0;
    sigb::PlanErr err;
    if (sigb::pplan(d_text != nullptr, text_buf_len, text_off, text_len, nfiles, block_size, &files, &nchunks, &ntiles,
                    &err))
        return fail(err.code, "%s", err.msg.c_str());
    SYDELTA_ENTER_DEVICE(device);
    int dev;
    hipStream_t s = call_stream(device, stream, &dev);
    CallProf cp;

    // 2. the tables: files, the chunk table (counts and ranks), and what comes back (sig_off,
    // nblocks, last_size, the status words, the first off-layout entries, the total: one copy)
    const size_t nce = nchunks + 1, nres = 5 * nfiles + 1;
    const size_t o_files = 0, o_cnt = o_files + up256(nfiles * sizeof(sigb::PFile)), o_rank = o_cnt + up256(nce * 8),
                 o_res = o_rank + up256(nce * 8), b_all = o_res + up256(nres * 8);
    DevBuf tab;
    StreamDrain drain(s);
    ALLOC_TRY(tab, b_all, s);
    uint8_t* const H = tab.at<uint8_t>();
    SigbPArgs a{};
    a.text = d_text;
    a.files = (sigb::PFile*)(H + o_files);
    a.nfiles = nfiles, a.nchunks = nchunks, a.ntiles = ntiles, a.bs = block_size;
    a.cnt = (uint64_t*)(H + o_cnt);
    a.rank = (uint64_t*)(H + o_rank);
    a.sig_off = (uint64_t*)(H + o_res);
    a.nblocks = a.sig_off + nfiles;
    a.last = a.nblocks + nfiles;
    a.status = a.last + nfiles;
    a.lay_i = a.status + nfiles;
    a.need = a.lay_i + nfiles;

    HIP_TRY(t_pstage.open(dev, (size_t)sigb::kStageSlots * sigb::kStageBytes));
    uint64_t slot_uses = 0;
    drain.armed = true;
    HIP_TRY(t_pstage.upload(files.data(), files.size(), (sigb::PFile*)a.files, &slot_uses, s));

    // 3. count, rank, sizes, parse (the kernel decides whether the SoA holds the entries), and
    // the tables back: the one wait
    const bool staged = parser_staged();
    HIP_TRY(launch_sigpb_count(a, staged, s, cp.get()));
    HIP_TRY(launch_sigpb_parse(a, d_weak, d_strong, d_weak && d_strong ? sig_cap : 0, staged, s, cp.get()));
    std::vector<uint64_t> res(nres);
    HIP_TRY(hipMemcpyAsync(res.data(), a.sig_off, nres * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    drain.armed = false;

    const uint64_t *r_off = res.data(), *r_n = r_off + nfiles, *r_last = r_n + nfiles, *r_st = r_last + nfiles,
                   *r_i = r_st + nfiles;
    std::copy(r_off, r_off + nfiles, sig_off);
    std::copy(r_n, r_n + nfiles, nblocks);
    std::copy(r_last, r_last + nfiles, last_size);
    *sig_need = res[5 * nfiles];
    // a refused file keeps its place; a last size sydelta_index_create_batch takes for its count
    for (uint64_t f = 0; f < nfiles; ++f)
        if (r_st[f] != sigb::kNoBad) last_size[f] = r_n[f] ? block_size : 0;
    for (uint64_t f = 0; f < nfiles; ++f) {
        if (file_status) file_status[f] = sigb::status_out(r_st[f]);
        else if (r_st[f] != sigb::kNoBad)
            return fail(SYDELTA_E_INVAL, "%s", sigb::refusal_message(f, r_st[f], r_i[f], block_size).c_str());
    }
    return SYDELTA_OK;
} catch (...) {
    return sydelta::host_exception();
}
