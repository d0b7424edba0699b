// sydelta_unzstdbatch.cpp — sydelta_zstd_decompress_batch_device: compress::decompress
// (sy-remote.rs:160-166) for a batch of frames, the receiver's first step behind
// sydelta_zstd_compress_batch_device's arena.  The host validates the tables, uploads the file
// table through pinned staging and waits three times whatever the batch: for the per-file
// counts (they size the shared scratch, and their exclusive sums, made here from that one copy,
// go back up as the files' bases), for the sizes and statuses, and at the end.
#include <algorithm>

#include "sydelta_host.hpp"
#include "sydelta_stage.hpp"
#include "sydelta_unzstdbatch.hpp"

using namespace sydelta;

namespace {

// The calling thread's pinned staging (sydelta_stage.hpp): kStageSlots slots of kStageBytes,
// whatever the batch.
thread_local StageRing t_stage(unzb::kStageSlots);
}  // namespace

#define ALLOC_TRY(buf, bytes, s)                                                                          \
    do {                                                                                                  \
        const hipError_t e_ = (buf).alloc((bytes), (s));                                                  \
        if (e_ != hipSuccess) {                                                                           \
            (void)hipGetLastError();                                                                      \
            return fail(e_ == hipErrorOutOfMemory ? SYDELTA_E_OOM : SYDELTA_E_KERNEL,                     \
                        "zstd batch decode: device allocation of %llu bytes failed: %s", (ull)(bytes),    \
                        hipGetErrorString(e_));                                                           \
        }                                                                                                 \
    } while (0)

extern "C" int sydelta_zstd_decompress_batch_device(int device, const uint8_t* d_in, uint64_t in_buf_len,
                                                    const uint64_t* frame_off, const uint64_t* frame_len,
                                                    uint64_t nfiles, uint8_t* d_out, uint64_t out_buf_len,
                                                    uint64_t* text_off, uint64_t* text_len, uint64_t* file_status,
                                                    uint64_t* out_need, void* stream) try {
    typedef unsigned long long ull;
    if (!out_need) return fail(SYDELTA_E_INVAL, "NULL out_need");
    *out_need = 0;
    if (!nfiles) return SYDELTA_OK;

    // 1. every table entry validated before a device is touched
    static const bool host_timing = getenv("SYDELTA_HOST_TIMING") != nullptr;
    const auto t_start = std::chrono::steady_clock::now();
    std::vector<unzb::File> files;
    unzb::PlanErr err;
    if (unzb::plan(d_in != nullptr, in_buf_len, frame_off, frame_len, nfiles, d_out != nullptr, out_buf_len, text_off,
                   text_len, &files, &err))
        return fail(err.code, "%s", err.msg.c_str());
    SYDELTA_ENTER_DEVICE(device);
    int dev;
    hipStream_t s = call_stream(device, stream, &dev);
    CallProf cp;

    // 2. the per-file tables: frames, counts, bases, and what comes back (text_off, text_len,
    // the statuses and the total, one copy)
    const size_t o_files = 0, o_tot = o_files + up256(nfiles * sizeof(unzb::File)),
                 o_bases = o_tot + up256(nfiles * sizeof(unz::Totals)), o_pad = o_bases + up256(nfiles * sizeof(unzb::Base)),
                 o_res = o_pad + up256(nfiles * 8), b_head = o_res + up256((3 * nfiles + 1) * 8);
    DevBuf head;
    // On an error after the first upload was queued the stream is drained before the scratch
    // (device) and the staging (host, reused by the next call) go away.
    StreamDrain drain(s);
    ALLOC_TRY(head, b_head, s);
    uint8_t* const H = head.at<uint8_t>();
    UnzbArgs a{};
    a.in = d_in;
    a.files = (unzb::File*)(H + o_files);
    a.bases = (unzb::Base*)(H + o_bases);
    a.nfiles = nfiles;
    a.tot = (unz::Totals*)(H + o_tot);
    a.pad = (uint64_t*)(H + o_pad);
    a.text_off = (uint64_t*)(H + o_res);
    a.text_len = a.text_off + nfiles;
    a.status = (unsigned long long*)(a.text_len + nfiles);
    a.need = (uint64_t*)(a.status + nfiles);

    HIP_TRY(t_stage.open(dev, (size_t)unzb::kStageSlots * unzb::kStageBytes));
    uint64_t slot_uses = 0;
    drain.armed = true;
    HIP_TRY(t_stage.upload(files.data(), files.size(), (unzb::File*)a.files, &slot_uses, s));

    // 3. the counts: first wait
    HIP_TRY(launch_unzb_count(a, s, cp.get()));
    std::vector<unz::Totals> tot(nfiles);
    HIP_TRY(hipMemcpyAsync(tot.data(), a.tot, nfiles * sizeof(unz::Totals), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const double t_counts = ms_since(t_start);
    std::vector<unzb::Base> bases;
    unzb::Base c;
    if (unzb::bases(tot.data(), nfiles, &bases, &c, &err)) return fail(err.code, "%s", err.msg.c_str());

    // 4. the shared scratch, the block table, tables, entropy decode, stitch, offsets, sizes
    // and positions: second wait
    const UnzScratch L(c.nb, c.nhuf, c.nfse, c.nlit, c.nseq, nfiles);
    const uint64_t o_bfile = L.total, o_apos = o_bfile + up256(c.nb * 4), total = o_apos + up256(c.nb * 8);
    DevBuf ws;
    ALLOC_TRY(ws, total, s);
    const double t_scratch = ms_since(t_start);
    L.point(a, ws.at<uint8_t>());
    a.bfile = ws.at<uint32_t>(o_bfile);
    a.nb = c.nb;
    a.apos = ws.at<uint64_t>(o_apos);
    HIP_TRY(t_stage.upload(bases.data(), bases.size(), (unzb::Base*)a.bases, &slot_uses, s));
    HIP_TRY(launch_unzb_decode(a, s, cp.get()));
    std::vector<uint64_t> res(3 * nfiles + 1);
    HIP_TRY(hipMemcpyAsync(res.data(), a.text_off, res.size() * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    drain.armed = false;
    const double t_sizes = ms_since(t_start);
    if (unzb::finish(res.data(), res.data() + nfiles, res.data() + 2 * nfiles, res[3 * nfiles], nfiles, text_off, text_len,
                     file_status, out_need, &err))
        return fail(err.code, "%s", err.msg.c_str());
    const uint64_t n = *out_need;
    if (!d_out || out_buf_len < n || !n) return SYDELTA_OK;

    // 5. place, pointer doubling, gather over the arena: third wait
    DevBuf par;
    ALLOC_TRY(par, n * 4, s);
    const double t_parent = ms_since(t_start);
    drain.armed = true;
    HIP_TRY(launch_unzb_place(a, n, d_out, par.at<uint32_t>(), ws.at<uint32_t>(L.changed), s, cp.get()));
    const double t_enq = ms_since(t_start);
    HIP_TRY(hipStreamSynchronize(s));
    drain.armed = false;
    if (host_timing)
        fprintf(stderr, "sydelta unzstd batch: %llu files, %llu blocks, %llu bytes; counts back %.3f ms, scratch of %llu "
                "bytes %.3f ms, sizes back %.3f ms, parents %.3f ms, all queued %.3f ms, total %.3f ms\n", (ull)nfiles,
                (ull)c.nb, (ull)n, t_counts, (ull)total, t_scratch, t_sizes, t_parent, t_enq, ms_since(t_start));
    return SYDELTA_OK;
} catch (...) {
    return sydelta::host_exception();
}
