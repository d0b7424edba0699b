// sydelta_dparsebatch.cpp — sydelta_delta_batch_from_json_device: serde_json::from_str::<Delta>
// (sy-remote.rs:175) for a batch of texts, the receiver's step between
// sydelta_zstd_decompress_batch_device and sydelta_apply_delta_batch_device.  The host validates
// the tables, uploads the file table through pinned staging and waits twice whatever the batch:
// for the per-file counts (they size the op table and say whether the arena holds the literals),
// and at the end, for the records and the op table, which it splits into the batch's deltas.
#include <algorithm>

#include "sydelta_dparsebatch.hpp"
#include "sydelta_host.hpp"
#include "sydelta_stage.hpp"

using namespace sydelta;

namespace {
// The calling thread's pinned staging (sydelta_stage.hpp): kStageSlots slots of kStageBytes,
// whatever the batch.
thread_local StageRing t_stage(dpb::kStageSlots);
}  // namespace

#define ALLOC_TRY(buf, bytes, s)                                                                          \
    do {                                                                                                  \
        const hipError_t e_ = (buf).alloc((bytes), (s));                                                  \
        if (e_ != hipSuccess) {                                                                           \
            (void)hipGetLastError();                                                                      \
            return fail(e_ == hipErrorOutOfMemory ? SYDELTA_E_OOM : SYDELTA_E_KERNEL,                     \
                        "Delta JSON batch: device allocation of %llu bytes failed: %s", (ull)(bytes),     \
                        hipGetErrorString(e_));                                                           \
        }                                                                                                 \
    } while (0)

extern "C" int sydelta_delta_batch_from_json_device(int device, const uint8_t* d_text, uint64_t text_buf_len,
                                                    const uint64_t* text_off, const uint64_t* text_len, uint64_t nfiles,
                                                    uint8_t* d_lit, uint64_t lit_buf_len, uint64_t* lit_off,
                                                    uint64_t* lit_len, uint64_t* file_status, uint64_t* lit_need,
                                                    sydelta_delta_batch** out, void* stream) try {
    typedef unsigned long long ull;
    if (out) *out = nullptr;
    if (!lit_need) return fail(SYDELTA_E_INVAL, "NULL lit_need");
    *lit_need = 0;
    if (!nfiles) {
        if (out) *out = new sydelta_delta_batch();
        return SYDELTA_OK;
    }

    // 1. every table entry validated before a device is touched
    static const bool host_timing = getenv("SYDELTA_HOST_TIMING") != nullptr;
    const auto t_start = std::chrono::steady_clock::now();
    std::vector<dpb::File> files;
    uint64_t nchunks = 0, ntiles = 0;
    dpb::PlanErr err;
    if (dpb::plan(d_text != nullptr, text_buf_len, text_off, text_len, nfiles, d_lit != nullptr, lit_buf_len, lit_off,
                  lit_len, &files, &nchunks, &ntiles, &err))
        return fail(err.code, "%s", err.msg.c_str());
    SYDELTA_ENTER_DEVICE(device);
    int dev;
    hipStream_t s = call_stream(device, stream, &dev);
    CallProf cp;

    // 2. the tables: files, records, the chunk table (counts and ranks), and what comes back
    // first (lit_off, lit_len, nops: one copy)
    const size_t nce = nchunks + 1;
    const size_t o_files = 0, o_recs = o_files + up256(nfiles * sizeof(dpb::File)),
                 o_cnt = o_recs + up256(nfiles * sizeof(dpb::Rec)), o_rank = o_cnt + up256(2 * nce * 8),
                 o_res = o_rank + up256(2 * nce * 8), o_pad = o_res + up256(3 * nfiles * 8),
                 b_head = o_pad + up256(nfiles * 8);
    DevBuf head, ob;
    // On an error after the first upload was queued the stream is drained before the scratch
    // (device) and the staging (host, reused by the next call) go away.
    StreamDrain drain(s);
    ALLOC_TRY(head, b_head, s);
    uint8_t* const H = head.at<uint8_t>();
    DpbArgs a{};
    a.text = d_text;
    a.files = (dpb::File*)(H + o_files);
    a.nfiles = nfiles, a.nchunks = nchunks, a.ntiles = ntiles;
    a.recs = (dpb::Rec*)(H + o_recs);
    a.ocnt = (uint64_t*)(H + o_cnt);
    a.lcnt = a.ocnt + nce;
    a.orank = (uint64_t*)(H + o_rank);
    a.lrank = a.orank + nce;
    a.lit_off = (uint64_t*)(H + o_res);
    a.lit_len = a.lit_off + nfiles;
    a.nops = a.lit_len + nfiles;
    a.pad = (uint64_t*)(H + o_pad);

    HIP_TRY(t_stage.open(dev, (size_t)dpb::kStageSlots * dpb::kStageBytes));
    uint64_t slot_uses = 0;
    drain.armed = true;
    HIP_TRY(t_stage.upload(files.data(), files.size(), (dpb::File*)a.files, &slot_uses, s));

    // 3. tail, count, ranks, sizes, lit_off: first wait
    HIP_TRY(launch_dpb_count(a, s, cp.get()));
    std::vector<uint64_t> res(3 * nfiles);
    HIP_TRY(hipMemcpyAsync(res.data(), a.lit_off, res.size() * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const double t_counts = ms_since(t_start);
    const uint64_t *r_off = res.data(), *r_len = r_off + nfiles, *r_nops = r_len + nfiles;
    uint64_t total_ops = 0;
    for (uint64_t f = 0; f < nfiles; ++f) {
        lit_off[f] = r_off[f], lit_len[f] = r_len[f];
        total_ops += r_nops[f];
    }
    const uint64_t need = r_off[nfiles - 1] + r_len[nfiles - 1];
    *lit_need = need;
    uint8_t* const lit = d_lit && lit_buf_len >= need ? d_lit : nullptr;  // else: the size query

    // 4. place and parse (with or without the literal bytes), the records and the op table back:
    // second wait
    uint64_t* d_pos = nullptr;
    sydelta_op* d_ops = nullptr;
    // the whole op table, plain memory without a zero fill (not an OpVec: an array of this size
    // would come from the op arena that the deltas of the match calls live in)
    std::unique_ptr<sydelta_op[]> ops(out && total_ops ? new sydelta_op[total_ops] : nullptr);
    if (total_ops) {
        ALLOC_TRY(ob, total_ops * (8 + sizeof(sydelta_op)), s);
        d_ops = ob.at<sydelta_op>();
        d_pos = (uint64_t*)(d_ops + total_ops);
        HIP_TRY(launch_dpb_parse(a, d_pos, d_ops, lit, s, cp.get()));
        if (out)
            HIP_TRY(hipMemcpyAsync(ops.get(), d_ops, total_ops * sizeof(sydelta_op), hipMemcpyDeviceToHost, s));
    }
    std::vector<dpb::Rec> recs(nfiles);
    HIP_TRY(hipMemcpyAsync(recs.data(), a.recs, nfiles * sizeof(dpb::Rec), hipMemcpyDeviceToHost, s));
    const double t_enq = ms_since(t_start);
    HIP_TRY(hipStreamSynchronize(s));
    drain.armed = false;
    const double t_ops = ms_since(t_start);

    // 5. the statuses, then the batch's deltas from the op table (file f's ops behind those of
    // the files before it)
    for (uint64_t f = 0; f < nfiles; ++f) {
        const uint64_t st = recs[f].status;
        if (file_status) file_status[f] = st == dpb::kNoBad ? 0 : 1 + st;
        else if (st != dpb::kNoBad) return fail(SYDELTA_E_INVAL, "%s", dpb::refusal_message(f, st).c_str());
    }
    if (!out) return SYDELTA_OK;
    std::unique_ptr<sydelta_delta_batch> b(new sydelta_delta_batch());
    b->d.resize(nfiles);
    uint64_t o0 = 0;
    for (uint64_t f = 0; f < nfiles; o0 += r_nops[f], ++f) {
        if (recs[f].status != dpb::kNoBad) continue;  // a refused file: no ops
        sydelta_delta& d = b->d[f];
        d.source_size = recs[f].n;
        d.block_size = recs[f].b;
        d.ops.assign(ops.get() + o0, ops.get() + o0 + r_nops[f]);
        for (const sydelta_op& o : d.ops) {  // the stats the single call fills
            if (o.kind == SYDELTA_OP_COPY) ++d.stats.copy_ops;
            else { ++d.stats.data_ops; d.stats.literal_bytes += o.b; }
        }
        b->total.copy_ops += d.stats.copy_ops;
        b->total.data_ops += d.stats.data_ops;
        b->total.literal_bytes += d.stats.literal_bytes;
    }
    *out = b.release();
    if (host_timing)
        fprintf(stderr, "sydelta dparse batch: %llu files, %llu chunks, %llu ops; counts back %.3f ms, all queued %.3f ms, "
                "op table back %.3f ms, deltas split %.3f ms\n", (ull)nfiles, (ull)nchunks, (ull)total_ops, t_counts, t_enq,
                t_ops, ms_since(t_start));
    return SYDELTA_OK;
} catch (...) {
    return sydelta::host_exception();
}
