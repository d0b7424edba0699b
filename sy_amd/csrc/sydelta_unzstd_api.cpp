// sydelta_unzstd_api.cpp — sydelta_zstd_decompress_device: step 2 of sy-remote's
// apply-delta (sy-remote.rs:160-166: the zstd magic sniffed, compress::decompress), on a
// frame in HBM.  Two host round trips: the scan's counts (they size the scratch), then the
// regenerated size and the status word before anything is written to d_out.
#include <algorithm>

#include "sydelta_host.hpp"
#include "sydelta_unzstd.hpp"

using namespace sydelta;

namespace {

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
    hipStream_t s = call_stream(device, stream);
    CallProf cp;

    // the counts
    DevBuf head;
    HIP_TRY(head.alloc(512, s));
    unz::Totals* d_tot = head.at<unz::Totals>();
    unsigned long long* d_status = head.at<unsigned long long>(256);
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
    const UnzScratch L(c.nb, c.nhuf, c.nfse, c.nlit, c.nseq, 1);
    DevBuf ws;
    HIP_TRY(ws.alloc(L.total, s));
    UnzArgs a{};
    a.in = d_in;
    L.point(a, ws.at<uint8_t>());
    a.nb = c.nb;
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
    DevBuf par;
    HIP_TRY(par.alloc(n * 4, s));
    HIP_TRY(launch_unz_place(a, n, d_out, par.at<uint32_t>(), ws.at<uint32_t>(L.changed), s, cp.get()));
    HIP_TRY(hipStreamSynchronize(s));
    return SYDELTA_OK;
} catch (...) {
    return sydelta::host_exception();
}
