// sydelta_unzstdbatch.cpp — sydelta_zstd_decompress_batch_device: compress::decompress
// (sy-remote.rs:160-166) for a batch of frames, the receiver's first step behind
// sydelta_zstd_compress_batch_device's arena.  The host validates the tables, uploads the file
// table through pinned staging and waits three times whatever the batch: for the per-file
// counts (they size the shared scratch, and their exclusive sums, made here from that one copy,
// go back up as the files' bases), for the sizes and statuses, and at the end.
#include <algorithm>
#include <chrono>
#include <map>

#include "sydelta_host.hpp"
#include "sydelta_unzstdbatch.hpp"

using namespace sydelta;

namespace {

struct FreeAsync {
    void* p = nullptr;
    hipStream_t s = nullptr;
    ~FreeAsync() {
        if (p) (void)hipFreeAsync(p, s);
    }
};

// The calling thread's pinned staging (kStageSlots slots of kStageBytes, whatever the batch),
// and per device the events of the slots' uploads (never destroyed, like thread_stream).
struct Stage {
    uint8_t* p = nullptr;
    ~Stage() {
        if (p) (void)hipHostFree(p);
    }
};
struct Uploads {
    hipEvent_t up[unzb::kStageSlots] = {};
};
thread_local Stage t_stage;
thread_local std::map<int, Uploads> t_up;

size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// A host table to the device, a staging slot at a time; *k counts the call's slot uses.
template <class T>
hipError_t upload(const std::vector<T>& src, T* d_dst, Uploads& ups, uint64_t* k, hipStream_t s) {
    const size_t per = unzb::kStageBytes / sizeof(T);
    for (size_t i0 = 0; i0 < src.size(); i0 += per, ++*k) {
        const size_t n = std::min(per, src.size() - i0);
        const uint32_t slot = (uint32_t)(*k % unzb::kStageSlots);
        if (*k >= unzb::kStageSlots)
            if (hipError_t e = hipEventSynchronize(ups.up[slot])) return e;  // the slot's previous upload
        T* h = (T*)(t_stage.p + (size_t)slot * unzb::kStageBytes);
        std::copy(src.begin() + i0, src.begin() + i0 + n, h);
        if (hipError_t e = hipMemcpyAsync(d_dst + i0, h, n * sizeof(T), hipMemcpyHostToDevice, s)) return e;
        if (hipError_t e = hipEventRecord(ups.up[slot], s)) return e;
    }
    return hipSuccess;
}

}  // namespace

#define ALLOC_TRY(ptr, bytes, s)                                                                          \
    do {                                                                                                  \
        const hipError_t e_ = dev_malloc_async(&(ptr), (bytes), (s));                                     \
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
    const int dev = device < 0 ? 0 : device;
    hipStream_t s = stream ? (hipStream_t)stream : thread_stream(dev);
    CallProf cp;

    // 2. the per-file tables: frames, counts, bases, and what comes back (text_off, text_len,
    // the statuses and the total, one copy)
    const size_t o_files = 0, o_tot = o_files + up256(nfiles * sizeof(unzb::File)),
                 o_bases = o_tot + up256(nfiles * sizeof(unz::Totals)), o_pad = o_bases + up256(nfiles * sizeof(unzb::Base)),
                 o_res = o_pad + up256(nfiles * 8), b_head = o_res + up256((3 * nfiles + 1) * 8);
    FreeAsync head;
    // On an error after the first upload was queued the stream is drained before the scratch
    // (device) and the staging (host, reused by the next call) go away.
    struct Drain {
        hipStream_t s;
        bool armed = false;
        ~Drain() {
            if (armed) (void)hipStreamSynchronize(s);
        }
    } drain{s};
    ALLOC_TRY(head.p, b_head, s);
    head.s = s;
    uint8_t* const H = (uint8_t*)head.p;
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

    if (!t_stage.p)
        HIP_TRY(hipHostMalloc((void**)&t_stage.p, (size_t)unzb::kStageSlots * unzb::kStageBytes, hipHostMallocDefault));
    Uploads& ups = t_up[dev];
    for (hipEvent_t& e : ups.up)
        if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    uint64_t slot_uses = 0;
    drain.armed = true;
    HIP_TRY(upload(files, (unzb::File*)a.files, ups, &slot_uses, s));

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
    const uint64_t o_blocks = 0, o_bfile = o_blocks + up256(c.nb * sizeof(unz::Block)), o_huf = o_bfile + up256(c.nb * 4),
                   o_fse = o_huf + up256(c.nhuf * sizeof(unz::HufTab)), o_lits = o_fse + up256(c.nfse * sizeof(unz::FseTab)),
                   o_seqs = o_lits + up256(c.nlit), o_exit = o_seqs + up256(c.nseq * sizeof(unz::Seq)),
                   o_entry = o_exit + up256(c.nb * sizeof(unz::Hist)), o_bpos = o_entry + up256(c.nb * 12),
                   o_apos = o_bpos + up256((c.nb + nfiles) * 8), o_changed = o_apos + up256(c.nb * 8),
                   total = o_changed + up256(4 * kUnzRounds);
    FreeAsync ws;
    ALLOC_TRY(ws.p, total, s);
    ws.s = s;
    const double t_scratch = ms_since(t_start);
    uint8_t* const W = (uint8_t*)ws.p;
    a.blocks = (unz::Block*)(W + o_blocks);
    a.bfile = (uint32_t*)(W + o_bfile);
    a.nb = c.nb;
    a.huf = (unz::HufTab*)(W + o_huf);
    a.fse = (unz::FseTab*)(W + o_fse);
    a.lits = W + o_lits;
    a.seqs = (unz::Seq*)(W + o_seqs);
    a.exit = (unz::Hist*)(W + o_exit);
    a.entry = (uint32_t*)(W + o_entry);
    a.bpos = (uint64_t*)(W + o_bpos);
    a.apos = (uint64_t*)(W + o_apos);
    HIP_TRY(upload(bases, (unzb::Base*)a.bases, ups, &slot_uses, s));
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
    FreeAsync par;
    ALLOC_TRY(par.p, n * 4, s);
    par.s = s;
    const double t_parent = ms_since(t_start);
    drain.armed = true;
    HIP_TRY(launch_unzb_place(a, n, d_out, (uint32_t*)par.p, (uint32_t*)(W + o_changed), s, cp.get()));
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
