// sydelta_unzstd_api.cpp — sydelta_zstd_decompress_device: step 2 of sy-remote's
// apply-delta (sy-remote.rs:160-166: the zstd magic sniffed, compress::decompress), on a
// frame in HBM.  Two host round trips: the scan's counts (they size the scratch), then the
// regenerated size and the status word before anything is written to d_out.
#include <algorithm>

#include "sydelta_host.hpp"
#include "sydelta_unzstd.hpp"

using namespace sydelta;

namespace {

struct FreeAsync {
    void* p = nullptr;
    hipStream_t s = nullptr;
    ~FreeAsync() {
        if (p) (void)hipFreeAsync(p, s);
    }
};

int frame_error(uint64_t status) {
    return fail(SYDELTA_E_INVAL, "zstd frame: block %llu: %s", (unsigned long long)(status >> 32),
                unz::err_text((uint32_t)status));
}

}  // namespace

extern "C" int sydelta_zstd_decompress_device(int device, const uint8_t* d_in, uint64_t len, uint8_t* d_out,
                                              uint64_t out_cap, uint64_t* out_len, void* stream) try {
    if (!out_len) return fail(SYDELTA_E_INVAL, "NULL argument");
    *out_len = 0;
    if (len < 4) return frame_error(unz::ekey(0, unz::kTrunc));
    if (!d_in) return fail(SYDELTA_E_INVAL, "NULL input");
    SYDELTA_ENTER_DEVICE(device);
    hipStream_t s = stream ? (hipStream_t)stream : thread_stream(device < 0 ? 0 : device);
    CallProf cp;
    auto al = [](uint64_t b) { return (b + 255) & ~(uint64_t)255; };

    // the counts
    FreeAsync head;
    HIP_TRY(dev_malloc_async(&head.p, 512, s));
    head.s = s;
    unz::Totals* d_tot = (unz::Totals*)head.p;
    unsigned long long* d_status = (unsigned long long*)((uint8_t*)head.p + 256);
    struct {
        unz::Totals t;
        unsigned long long status;
    } h;
    HIP_TRY(hipMemsetAsync(d_status, 0xFF, 8, s));
    HIP_TRY(launch_unz_scan(d_in, len, nullptr, 0, d_tot, d_status, s, cp.get()));
    HIP_TRY(hipMemcpyAsync(&h.t, d_tot, sizeof h.t, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&h.status, d_status, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (h.status != unz::kNoErr) return frame_error(h.status);
    const unz::Totals c = h.t;
    if (c.nb > 0x7FFFFFFFull) return fail(SYDELTA_E_INVAL, "zstd frame: too many blocks");

    // tables, entropy decode, stitch, offsets
    const uint64_t o_blocks = 0, o_huf = o_blocks + al(c.nb * sizeof(unz::Block)),
                   o_fse = o_huf + al(c.nhuf * sizeof(unz::HufTab)), o_lits = o_fse + al(c.nfse * sizeof(unz::FseTab)),
                   o_seqs = o_lits + al(c.nlit), o_exit = o_seqs + al(c.nseq * sizeof(unz::Seq)),
                   o_entry = o_exit + al(c.nb * sizeof(unz::Hist)), o_bpos = o_entry + al(c.nb * 12),
                   o_changed = o_bpos + al((c.nb + 1) * 8), total = o_changed + al(4 * kUnzRounds);
    FreeAsync ws;
    HIP_TRY(dev_malloc_async(&ws.p, total, s));
    ws.s = s;
    uint8_t* W = (uint8_t*)ws.p;
    UnzArgs a{};
    a.in = d_in;
    a.blocks = (unz::Block*)(W + o_blocks);
    a.nb = c.nb;
    a.huf = (unz::HufTab*)(W + o_huf);
    a.fse = (unz::FseTab*)(W + o_fse);
    a.lits = W + o_lits;
    a.seqs = (unz::Seq*)(W + o_seqs);
    a.exit = (unz::Hist*)(W + o_exit);
    a.entry = (uint32_t*)(W + o_entry);
    a.bpos = (uint64_t*)(W + o_bpos);
    a.tot = d_tot;
    a.status = d_status;
    HIP_TRY(launch_unz_scan(d_in, len, a.blocks, c.nb, d_tot, d_status, s, cp.get()));
    HIP_TRY(launch_unz_decode(a, s, cp.get()));
    HIP_TRY(hipMemcpyAsync(&h.t, d_tot, sizeof h.t, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&h.status, d_status, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (h.status != unz::kNoErr) return frame_error(h.status);
    const uint64_t n = h.t.out_len;
    *out_len = n;
    if (!d_out || out_cap < n || !n) return SYDELTA_OK;

    // place, pointer doubling, gather
    FreeAsync par;
    HIP_TRY(dev_malloc_async(&par.p, n * 4, s));
    par.s = s;
    HIP_TRY(launch_unz_place(a, n, d_out, (uint32_t*)par.p, (uint32_t*)(W + o_changed), s, cp.get()));
    HIP_TRY(hipStreamSynchronize(s));
    return SYDELTA_OK;
} catch (...) {
    return sydelta::host_exception();
}
