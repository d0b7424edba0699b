// sydelta_applybatch.cpp — sydelta_apply_delta_batch_device: applier.rs:22-56 for a batch
// of (basis, delta) pairs.  The host validates and merges every file's ops
// (sydelta_applybatch.hpp; on the shared host pool when the batch is large), then feeds the
// merged table to the device in slices through the calling thread's pinned ring
// (sydelta_stage.hpp; kRing slices of kSliceBytes, whatever the batch): slice j is filled
// while slice j-1 is uploaded on the ring's copy stream and slice j-2 is copied by k_applyb.
#include <algorithm>

#include "sydelta_host.hpp"
#include "sydelta_stage.hpp"
#include "sydelta_applybatch.hpp"

using namespace sydelta;

namespace {
thread_local StageRing t_ring(applyb::kRing);
}  // namespace

extern "C" int sydelta_apply_delta_batch_device(int device, const uint8_t* d_basis, uint64_t basis_buf_len,
                                                const uint64_t* basis_off, const uint64_t* basis_len,
                                                const sydelta_delta* const* deltas, const uint8_t* d_lit,
                                                uint64_t lit_buf_len, const uint64_t* lit_off, const uint64_t* lit_len,
                                                uint8_t* d_out, uint64_t out_buf_len, const uint64_t* out_off,
                                                const uint64_t* out_cap, uint64_t nfiles, void* stream,
                                                sydelta_apply_stats* per_file, sydelta_apply_stats* total) try {
    if (total) *total = sydelta_apply_stats{};
    if (!nfiles) return SYDELTA_OK;
    if (!deltas || !basis_off || !basis_len || !lit_off || !lit_len || !out_off || !out_cap)
        return fail(SYDELTA_E_INVAL, "NULL table");
    SYDELTA_ENTER_DEVICE(device);
    static const bool host_timing = getenv("SYDELTA_HOST_TIMING") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();

    // 1. validate and merge: parts of about equal op counts, each with its own run list
    uint64_t nops = 0;
    for (uint64_t f = 0; f < nfiles; ++f) nops += deltas[f] ? deltas[f]->ops.size() : 0;
    const int nparts = batch_parts(nops, nfiles);
    struct Part {
        uint64_t f0 = 0, f1 = 0;
        std::vector<applyb::Run> runs;
        applyb::Err err;
    };
    std::vector<Part> parts(nparts);
    const auto ranges = split_by_ops(deltas, nfiles, nparts, nops);
    for (int t = 0; t < nparts; ++t) parts[t].f0 = ranges[t].first, parts[t].f1 = ranges[t].second;
    std::vector<sydelta_apply_stats> stats(nfiles);  // handed to the caller once the batch is valid
    std::vector<applyb::FileRuns> files(nfiles);  // runs: first the index into the part's list
    const applyb::Arenas arenas{basis_buf_len, lit_buf_len, out_buf_len};
    const bool ok = walk::run_parallel(nparts, [&](int t) {
        Part& P = parts[t];
        for (uint64_t f = P.f0; f < P.f1; ++f) {
            const sydelta_delta* d = deltas[f];
            const applyb::FileIn in{d && !d->ops.empty() ? d->ops.data() : nullptr, d ? d->ops.size() : 0, d != nullptr,
                                    basis_off[f], basis_len[f], lit_off[f], lit_len[f], out_off[f], out_cap[f]};
            const size_t first = P.runs.size();
            if (applyb::plan_file(f, in, arenas, P.runs, &stats[f], &P.err)) return;
            files[f] = applyb::FileRuns{(const applyb::Run*)(uintptr_t)first, P.runs.size() - first};
        }
    });
    if (!ok) return fail(SYDELTA_E_OOM, "out of host memory");
    for (const Part& P : parts)  // the first file in error
        if (P.err.code) return fail(P.err.code, "%s", P.err.msg.c_str());
    sydelta_apply_stats sum{};
    bool from_basis = false, from_lit = false;
    for (const Part& P : parts) {
        for (uint64_t f = P.f0; f < P.f1; ++f) {
            files[f].runs = P.runs.data() + (uintptr_t)files[f].runs;
            sum.operations_count += stats[f].operations_count;
            sum.literal_bytes += stats[f].literal_bytes;
            sum.bytes_written += stats[f].bytes_written;  // <= out_buf_len each; the ranges are disjoint
        }
        for (const applyb::Run& r : P.runs) (r.from_basis ? from_basis : from_lit) = true;
    }
    if (sum.bytes_written && !d_out) return fail(SYDELTA_E_INVAL, "NULL output");
    if ((from_basis && !d_basis) || (from_lit && !d_lit)) return fail(SYDELTA_E_INVAL, "NULL input arena");
    if (per_file) std::copy(stats.begin(), stats.end(), per_file);
    if (total) *total = sum;
    if (!sum.bytes_written) return SYDELTA_OK;
    const double t_plan = ms_since(t0);

    // 2. the slices
    uint64_t nslices = 0, nruns = 0;
    {
        applyb::Cursor c;
        applyb::Slice sl;
        while (applyb::next_slice(files.data(), nfiles, (uintptr_t)d_out, c, nullptr, nullptr, &sl)) ++nslices, nruns += sl.nruns;
    }
    int dev;
    hipStream_t s = call_stream(device, stream, &dev), copy;
    CallProf cp;
    HIP_TRY(t_ring.open(dev, applyb::kRing * applyb::kSliceBytes));
    // On an error after the first upload was queued: both streams are drained before the
    // table (device) and the ring (host, reused by the next call) go away.
    DevBuf tab;
    HIP_TRY(tab.alloc(nslices * applyb::kSliceBytes, s));
    HIP_TRY(t_ring.copy_stream(s, &copy));  // the table allocation is ordered before the uploads
    StreamDrain drain(copy, s);
    drain.armed = true;
    applyb::Cursor c;
    applyb::Slice sl;
    for (uint64_t j = 0; j < nslices; ++j) {
        void* slot;
        HIP_TRY(t_ring.acquire(j, &slot));
        applyb::Seg* hs = (applyb::Seg*)slot;
        applyb::Run* hr = (applyb::Run*)(hs + applyb::kSliceSegs);
        if (!applyb::next_slice(files.data(), nfiles, (uintptr_t)d_out, c, hr, hs, &sl))
            return fail(SYDELTA_E_INVAL, "internal: slice count");
        applyb::Seg* ds = tab.at<applyb::Seg>(j * applyb::kSliceBytes);
        applyb::Run* dr = (applyb::Run*)(ds + applyb::kSliceSegs);
        HIP_TRY(hipMemcpyAsync(ds, hs, sl.nsegs * sizeof(applyb::Seg), hipMemcpyHostToDevice, copy));
        HIP_TRY(hipMemcpyAsync(dr, hr, sl.nruns * sizeof(applyb::Run), hipMemcpyHostToDevice, copy));
        HIP_TRY(t_ring.uploaded(j, copy, s));
        HIP_TRY(launch_applyb(dr, ds, sl.nsegs, sl.ntiles, d_basis, d_lit, d_out, s, cp.get()));
    }
    const double t_enq = ms_since(t0);
    HIP_TRY(hipStreamSynchronize(s));  // the ring is reused by the next call
    drain.armed = false;
    if (host_timing)
        fprintf(stderr, "sydelta apply batch: %llu files, %llu ops, %llu runs, %llu slices, plan %.3f ms, enqueued %.3f ms, "
                "total %.3f ms\n", (unsigned long long)nfiles, (unsigned long long)nops, (unsigned long long)nruns,
                (unsigned long long)nslices, t_plan, t_enq, ms_since(t0));
    return SYDELTA_OK;
} catch (...) {
    return sydelta::host_exception();
}
