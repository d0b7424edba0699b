// sydelta_applybatch.cpp — sydelta_apply_delta_batch_device: applier.rs:22-56 for a batch
// of (basis, delta) pairs.  The host validates and merges every file's ops
// (sydelta_applybatch.hpp; on the shared host pool when the batch is large), then feeds the
// merged table to the device in slices through a ring of pinned buffers: slice j is filled
// while slice j-1 is uploaded on a copy stream and slice j-2 is copied by k_applyb.
#include <algorithm>
#include <chrono>
#include <map>

#include "sydelta_host.hpp"
#include "sydelta_applybatch.hpp"

using namespace sydelta;

namespace {

struct FreeAsync {
    void* p = nullptr;
    hipStream_t s = nullptr;
    ~FreeAsync() {
        if (p) (void)hipFreeAsync(p, s);
    }
};

// The calling thread's pinned ring (kRing slices of kSliceBytes, whatever the batch), and
// per device its copy stream and the events of the slices' uploads (never destroyed, like
// thread_stream).
struct Ring {
    uint8_t* p = nullptr;
    ~Ring() {
        if (p) (void)hipHostFree(p);
    }
};
struct CopyStream {
    hipStream_t s = nullptr;
    hipEvent_t ready = nullptr, up[applyb::kRing] = {};
};
thread_local Ring t_ring;
thread_local std::map<int, CopyStream> t_copy;

constexpr uint64_t kParallelOps = 1ull << 17;  // below: the plan stays on the calling thread

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

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
    const int nparts = nops < kParallelOps ? 1 : (int)std::min<uint64_t>(std::max(1, walk::HostPool::get().size()), nfiles);
    struct Part {
        uint64_t f0 = 0, f1 = 0;
        std::vector<applyb::Run> runs;
        applyb::Err err;
    };
    std::vector<Part> parts(nparts);
    {
        uint64_t f = 0, seen = 0;
        for (int t = 0; t < nparts; ++t) {
            parts[t].f0 = f;
            const uint64_t goal = nops / nparts * (t + 1);
            while (f < nfiles && (t + 1 == nparts || seen < goal)) seen += deltas[f] ? deltas[f]->ops.size() : 0, ++f;
            parts[t].f1 = f;
        }
    }
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
    const int dev = device < 0 ? 0 : device;
    hipStream_t s = stream ? (hipStream_t)stream : thread_stream(dev);
    CallProf cp;
    if (!t_ring.p) HIP_TRY(hipHostMalloc((void**)&t_ring.p, applyb::kRing * applyb::kSliceBytes, hipHostMallocDefault));
    CopyStream& cs = t_copy[dev];
    if (!cs.s) HIP_TRY(hipStreamCreateWithFlags(&cs.s, hipStreamNonBlocking));
    if (!cs.ready) HIP_TRY(hipEventCreateWithFlags(&cs.ready, hipEventDisableTiming));
    for (hipEvent_t& e : cs.up)
        if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    // On an error after the first upload was queued: both streams are drained before the
    // table (device) and the ring (host, reused by the next call) go away (drain is declared
    // after tab, so it runs first).
    FreeAsync tab;
    struct Drain {
        hipStream_t a, b;
        bool armed = false;
        ~Drain() {
            if (armed) { (void)hipStreamSynchronize(a); (void)hipStreamSynchronize(b); }
        }
    } drain{cs.s, s};
    HIP_TRY(dev_malloc_async(&tab.p, nslices * applyb::kSliceBytes, s));
    tab.s = s;
    HIP_TRY(hipEventRecord(cs.ready, s));  // the table allocation is ordered before the uploads
    HIP_TRY(hipStreamWaitEvent(cs.s, cs.ready, 0));
    drain.armed = true;
    applyb::Cursor c;
    applyb::Slice sl;
    for (uint64_t j = 0; j < nslices; ++j) {
        const uint32_t slot = (uint32_t)(j % applyb::kRing);
        if (j >= applyb::kRing) HIP_TRY(hipEventSynchronize(cs.up[slot]));  // the slot's previous upload
        applyb::Seg* hs = (applyb::Seg*)(t_ring.p + slot * applyb::kSliceBytes);
        applyb::Run* hr = (applyb::Run*)(hs + applyb::kSliceSegs);
        if (!applyb::next_slice(files.data(), nfiles, (uintptr_t)d_out, c, hr, hs, &sl))
            return fail(SYDELTA_E_INVAL, "internal: slice count");
        applyb::Seg* ds = (applyb::Seg*)((uint8_t*)tab.p + j * applyb::kSliceBytes);
        applyb::Run* dr = (applyb::Run*)(ds + applyb::kSliceSegs);
        HIP_TRY(hipMemcpyAsync(ds, hs, sl.nsegs * sizeof(applyb::Seg), hipMemcpyHostToDevice, cs.s));
        HIP_TRY(hipMemcpyAsync(dr, hr, sl.nruns * sizeof(applyb::Run), hipMemcpyHostToDevice, cs.s));
        HIP_TRY(hipEventRecord(cs.up[slot], cs.s));
        HIP_TRY(hipStreamWaitEvent(s, cs.up[slot], 0));
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
