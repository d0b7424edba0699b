// sydelta_jsonbatch.cpp — sydelta_delta_batch_to_json_device: serde_json::to_string(&Delta)
// (ssh.rs:1003) for a batch of deltas.  The host validates every file and cuts its ops into
// tiles (sydelta_jsonbatch.hpp; on the shared host pool when the batch is large), then feeds
// the tile and pair tables to the device in slices through the calling thread's pinned ring
// (sydelta_stage.hpp; kRing slices of kSliceBytes, whatever the batch): half a ring of slices
// is filled while the half before it is uploaded and sized.
// Placing the texts, the decision whether the arena holds them, and the writing are queued
// behind the last slice without a wait; the call waits for the stream once, at the end.
#include <limits.h>

#include <algorithm>

#include "sydelta_host.hpp"
#include "sydelta_stage.hpp"
#include "sydelta_jsonbatch.hpp"

using namespace sydelta;

namespace {

thread_local StageRing t_ring(jsonb::kRing);

jsonb::FileIn file_in(const sydelta_delta* d, uint64_t lit_off, uint64_t lit_len) {
    return jsonb::FileIn{d && !d->ops.empty() ? d->ops.data() : nullptr, d ? d->ops.size() : 0, d != nullptr,
                         d ? d->source_size : 0, d ? d->block_size : 0, lit_off, lit_len};
}

}  // namespace

extern "C" uint64_t sydelta_delta_batch_to_json_bound(const sydelta_delta* const* deltas, uint64_t nfiles) try {
    if (!nfiles) return 0;
    if (!deltas) return UINT64_MAX;
    uint64_t total = 0;
    for (uint64_t f = 0; f < nfiles; ++f) {
        const sydelta_delta* d = deltas[f];
        uint64_t lo, hi;
        if (!d || !jsonb::text_bounds(d->ops.data(), d->ops.size(), d->source_size, d->block_size, &lo, &hi) ||
            hi > UINT64_MAX - 15)
            return UINT64_MAX;
        if (__builtin_add_overflow(total, (hi + 15) & ~(uint64_t)15, &total)) return UINT64_MAX;
    }
    return total;
} catch (...) {
    return UINT64_MAX;
}

extern "C" int sydelta_delta_batch_to_json_device(int device, const sydelta_delta* const* deltas, uint64_t nfiles,
                                                  const uint8_t* d_lit, uint64_t lit_buf_len, const uint64_t* lit_off,
                                                  const uint64_t* lit_len, uint8_t* d_out, uint64_t out_buf_len,
                                                  uint64_t* text_off, uint64_t* text_len, uint64_t* out_need,
                                                  void* stream) try {
    if (out_need) *out_need = 0;
    if (!nfiles) return SYDELTA_OK;
    if (!deltas || !lit_off || !lit_len || !text_off || !text_len || !out_need) return fail(SYDELTA_E_INVAL, "NULL table");
    if (nfiles > UINT32_MAX) return fail(SYDELTA_E_INVAL, "more than 2^32 - 1 files");
    SYDELTA_ENTER_DEVICE(device);
    static const bool host_timing = getenv("SYDELTA_HOST_TIMING") != nullptr;
    const auto t_start = std::chrono::steady_clock::now();

    // 1. validate every file and count its tiles and pairs: parts of about equal op counts
    uint64_t nops = 0;
    for (uint64_t f = 0; f < nfiles; ++f) nops += deltas[f] ? deltas[f]->ops.size() : 0;
    const int nparts = batch_parts(nops, nfiles);
    struct Part {
        uint64_t f0 = 0, f1 = 0, literal = 0;
        jsonb::Err err;
    };
    std::vector<Part> parts(nparts);
    const auto ranges = split_by_ops(deltas, nfiles, nparts, nops);
    for (int t = 0; t < nparts; ++t) parts[t].f0 = ranges[t].first, parts[t].f1 = ranges[t].second;
    std::vector<jsonb::FileIn> files(nfiles);
    std::vector<jsonb::Count> fc(nfiles);
    if (!walk::run_parallel(nparts, [&](int t) {
            Part& P = parts[t];
            for (uint64_t f = P.f0; f < P.f1; ++f) {
                files[f] = file_in(deltas[f], lit_off[f], lit_len[f]);
                if (jsonb::count_file(f, files[f], lit_buf_len, &fc[f], &P.literal, &P.err)) return;
            }
        }))
        return fail(SYDELTA_E_OOM, "out of host memory");
    jsonb::Count cnt;
    uint64_t literal = 0;
    for (const Part& P : parts) {  // the first file in error
        if (P.err.code) return fail(P.err.code, "%s", P.err.msg.c_str());
        literal |= P.literal;
    }
    for (const jsonb::Count& c : fc) cnt.tiles += c.tiles, cnt.pairs += c.pairs;
    if (literal && !d_lit) return fail(SYDELTA_E_INVAL, "NULL literal arena");
    if (cnt.tiles > INT_MAX) return fail(SYDELTA_E_INVAL, "the batch needs %llu tiles: split it", (unsigned long long)cnt.tiles);
    // where the slices start: from the counts, without a second look at the ops of a file
    // that fits a slice
    struct SliceAt {
        jsonb::Cursor c;
        uint64_t t0, p0;
        jsonb::Slice sl;
    };
    std::vector<SliceAt> slices;
    {
        jsonb::Cursor c;
        uint64_t t0 = 0, p0 = 0;
        for (;;) {
            SliceAt a{c, t0, p0, {}};
            if (!jsonb::next_slice(files.data(), fc.data(), nfiles, c, p0, nullptr, nullptr, &a.sl)) break;
            slices.push_back(a);
            t0 += a.sl.ntiles, p0 += a.sl.npairs;
        }
        if (t0 != cnt.tiles || p0 != cnt.pairs) return fail(SYDELTA_E_INVAL, "internal: slice count");
    }

    const double t_plan = ms_since(t_start);

    // 2. the device tables
    int dev;
    hipStream_t s = call_stream(device, stream, &dev);
    CallProf cp;
    HIP_TRY(t_ring.open(dev, jsonb::kRing * jsonb::kSliceBytes));
    const size_t b_tiles = up256(cnt.tiles * sizeof(jsonb::Tile)), b_pairs = up256(cnt.pairs * sizeof(jsonb::Pair)),
                 b_t8 = up256(cnt.tiles * 8), b_f8 = up256((nfiles + 1) * 8);
    // On an error after the first upload was queued: the stream is drained before the tables
    // (device) and the ring (host, reused by the next call) go away.
    DevBuf tab;
    StreamDrain drain(s);
    HIP_TRY(tab.alloc(b_tiles + b_pairs + 2 * b_t8 + 2 * b_f8 + up256(2 * nfiles * 8), s));
    uint8_t* at = tab.at<uint8_t>();
    jsonb::Tile* d_tiles = (jsonb::Tile*)at;
    jsonb::Pair* d_pairs = (jsonb::Pair*)(at += b_tiles);
    uint64_t* d_len = (uint64_t*)(at += b_pairs);
    uint64_t* d_off = (uint64_t*)(at += b_t8);
    uint64_t* d_fstart = (uint64_t*)(at += b_t8);
    uint64_t* d_pad = (uint64_t*)(at += b_f8);
    uint64_t* d_toff = (uint64_t*)(at += b_f8);  // text_off, then text_len: one copy back
    uint64_t* d_tlen = d_toff + nfiles;

    // 3. the slices, half a ring of them at a time: filled (in parallel when the batch is
    // large) while the other half uploads, then uploaded and sized in order
    constexpr uint32_t kGroup = jsonb::kRing / 2;
    const uint64_t nslices = slices.size();
    for (uint64_t j0 = 0; j0 < nslices; j0 += kGroup) {
        const int n = (int)std::min<uint64_t>(kGroup, nslices - j0);
        void* slot[kGroup];  // of the calling thread's ring: the pool's threads have their own t_ring
        for (int k = 0; k < n; ++k) HIP_TRY(t_ring.acquire(j0 + k, &slot[k]));
        int bad[kGroup] = {};
        const int par = nparts > 1 ? n : 1;
        if (!walk::run_parallel(par, [&](int k) {
                for (int i = k; i < n; i += par) {
                    const SliceAt& a = slices[j0 + i];
                    jsonb::Tile* ht = (jsonb::Tile*)slot[i];
                    jsonb::Cursor c = a.c;
                    jsonb::Slice sl;
                    jsonb::next_slice(files.data(), fc.data(), nfiles, c, a.p0, ht, (jsonb::Pair*)(ht + jsonb::kSliceTiles), &sl);
                    bad[i] = sl.ntiles != a.sl.ntiles || sl.npairs != a.sl.npairs;
                }
            }))
            return fail(SYDELTA_E_OOM, "out of host memory");
        for (int k = 0; k < n; ++k) {
            const SliceAt& a = slices[j0 + k];
            if (bad[k]) return fail(SYDELTA_E_INVAL, "internal: slice count");
            jsonb::Tile* ht = (jsonb::Tile*)slot[k];
            jsonb::Pair* hp = (jsonb::Pair*)(ht + jsonb::kSliceTiles);
            drain.armed = true;
            HIP_TRY(hipMemcpyAsync(d_tiles + a.t0, ht, a.sl.ntiles * sizeof(jsonb::Tile), hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemcpyAsync(d_pairs + a.p0, hp, a.sl.npairs * sizeof(jsonb::Pair), hipMemcpyHostToDevice, s));
            HIP_TRY(t_ring.uploaded(j0 + k, s));
            HIP_TRY(launch_jsonb_len(d_tiles, d_pairs, a.t0, a.sl.ntiles, d_lit, d_len, s, cp.get()));
        }
    }
    const double t_slices = ms_since(t_start);

    // 4. place the tiles and the texts, write, and bring the offsets and lengths back
    HIP_TRY(launch_exclusive_sum_u64(d_len, d_off, cnt.tiles, s));
    HIP_TRY(launch_jsonb_files(d_tiles, d_off, d_len, cnt.tiles, nfiles, d_fstart, d_tlen, d_pad, s, cp.get()));
    HIP_TRY(launch_exclusive_sum_u64(d_pad, d_toff, nfiles, s));
    HIP_TRY(launch_jsonb_write(d_tiles, d_pairs, cnt.tiles, d_lit, d_off, d_len, d_fstart, d_toff, d_tlen, nfiles, d_out,
                               out_buf_len, s, cp.get()));
    std::vector<uint64_t> res(2 * nfiles);
    HIP_TRY(hipMemcpyAsync(res.data(), d_toff, 2 * nfiles * 8, hipMemcpyDeviceToHost, s));
    const double t_enq = ms_since(t_start);
    HIP_TRY(hipStreamSynchronize(s));  // the ring is reused by the next call
    drain.armed = false;
    if (host_timing)
        fprintf(stderr, "sydelta json batch: %llu files, %llu ops, %llu tiles, %llu pairs, %llu slices, plan %.3f ms, slices "
                "queued %.3f ms, all queued %.3f ms, total %.3f ms\n", (unsigned long long)nfiles, (unsigned long long)nops,
                (unsigned long long)cnt.tiles, (unsigned long long)cnt.pairs, (unsigned long long)nslices, t_plan, t_slices,
                t_enq, ms_since(t_start));
    // every text is bounded from both sides by its ops; a length outside the bounds means a
    // sizing fault (the kernel wrote inside [0, need) or not at all)
    for (uint64_t f = 0; f < nfiles; ++f)
        if (res[nfiles + f] < fc[f].lo || res[nfiles + f] > fc[f].hi)
            return fail(SYDELTA_E_KERNEL, "file %llu: delta JSON sizing out of bounds (%llu not in [%llu, %llu])",
                        (unsigned long long)f, (unsigned long long)res[nfiles + f], (unsigned long long)fc[f].lo,
                        (unsigned long long)fc[f].hi);
    std::copy(res.begin(), res.begin() + nfiles, text_off);
    std::copy(res.begin() + nfiles, res.end(), text_len);
    *out_need = text_off[nfiles - 1] + text_len[nfiles - 1];
    return SYDELTA_OK;
} catch (...) {
    return sydelta::host_exception();
}
