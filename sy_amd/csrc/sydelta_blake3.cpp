// sydelta_blake3.cpp — BLAKE3-256 whole-file hashes (the `Cryptographic` arm of
// IntegrityVerifier::compute_file_checksum, integrity/mod.rs:100-112): Blake3Hasher::hash_data
// (integrity/blake3.rs:32-36) of bytes in HBM, one file, a batch or an aligned piece of a
// sharded file, the host-side join of the pieces' chaining values, and
// Blake3Hasher::hash_file (blake3.rs:16-29) streamed through the device.
#include <errno.h>
#include <fcntl.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <vector>

#include "sydelta_blake3.hpp"
#include "sydelta_host.hpp"

using namespace sydelta;

namespace {

constexpr uint64_t kFilePiece = 64ull << 20;  // hash_file's piece: 2^16 chunks

// start alignment of n nodes (B3Seg)
uint64_t seg_align(uint64_t n) {
    uint64_t a = 1;
    while (a < n && a < 64) a <<= 1;
    return a;
}

// Enqueue the hashes of files (offs, lens) of d_buf on s: d_out (device) + 32 f.  The
// scratch is released in stream order; the caller synchronizes.
int b3_enqueue(const uint8_t* d_buf, const uint64_t* offs, const uint64_t* lens, uint64_t nfiles, uint64_t first_chunk,
               bool root, uint8_t* d_out, hipStream_t s, Profiler* prof) {
    // level 0: the files' chunks; level j + 1: the nodes six levels up of the files still open
    struct Open {
        uint64_t file, n, start;
    };
    std::vector<B3Seg> tab;
    std::vector<uint64_t> lv_first, lv_count, lv_total;
    std::vector<Open> cur(nfiles), next;
    uint64_t pos = 0;
    for (uint64_t f = 0; f < nfiles; ++f) {
        const uint64_t n = b3::chunks_of(lens[f]), a = seg_align(n);
        pos = (pos + a - 1) / a * a;
        cur[f] = {f, n, pos};
        pos += n;
    }
    uint64_t total = pos;
    while (!cur.empty()) {
        lv_first.push_back(tab.size());
        lv_count.push_back(cur.size());
        lv_total.push_back(total);
        next.clear();
        uint64_t npos = 0;
        const bool chunks = lv_first.size() == 1;
        for (const Open& o : cur) {
            B3Seg sg{o.start, o.n, o.file, chunks ? offs[o.file] : 0, chunks ? lens[o.file] : 0};
            if (o.n > 64) {
                const uint64_t m = (o.n + 63) / 64, a = seg_align(m);
                npos = (npos + a - 1) / a * a;
                sg.out = npos;
                next.push_back({o.file, m, npos});
                npos += m;
            }
            tab.push_back(sg);
        }
        cur.swap(next);
        total = npos;
    }
    const int nlevels = (int)lv_first.size() - 1;
    const uint64_t cv0 = nlevels >= 1 ? lv_total[1] : 0, cv1 = nlevels >= 2 ? lv_total[2] : 0;
    const uint64_t tab_bytes = (tab.size() * sizeof(B3Seg) + 255) / 256 * 256;
    DevBuf ws;
    HIP_TRY(ws.alloc(tab_bytes + (cv0 + cv1) * 32 + 256, s));
    B3Seg* d_tab = (B3Seg*)ws.p;
    uint32_t* d_cv[2] = {(uint32_t*)((uint8_t*)ws.p + tab_bytes), (uint32_t*)((uint8_t*)ws.p + tab_bytes + cv0 * 32)};
    HIP_TRY(hipMemcpyAsync(d_tab, tab.data(), tab.size() * sizeof(B3Seg), hipMemcpyHostToDevice, s));
    std::vector<const B3Seg*> lv_segs;
    for (int j = 1; j <= nlevels; ++j) lv_segs.push_back(d_tab + lv_first[j]);
    HIP_TRY(launch_blake3(d_buf, d_tab, lv_count[0], lv_total[0], lv_segs.data(), lv_count.data() + 1, lv_total.data() + 1,
                          nlevels, d_cv, first_chunk, root, d_out, s, prof));
    return SYDELTA_OK;
}

// checked arguments -> host results
int b3_run(int device, const uint8_t* d_buf, const uint64_t* offs, const uint64_t* lens, uint64_t nfiles,
           uint64_t first_chunk, bool root, void* stream, uint8_t* out) {
    SYDELTA_ENTER_DEVICE(device);
    hipStream_t s = call_stream(device, stream);
    DevBuf d_out;
    HIP_TRY(d_out.alloc(nfiles * 32, s));
    CallProf cp;
    if (int r = b3_enqueue(d_buf, offs, lens, nfiles, first_chunk, root, (uint8_t*)d_out.p, s, cp.get())) return r;
    HIP_TRY(hipMemcpyAsync(out, d_out.p, nfiles * 32, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return SYDELTA_OK;
}

void empty_hash(uint8_t out[32]) {
    uint32_t w[8];
    b3::hash_host(nullptr, 0, 0, true, w);
    b3::words_to_bytes(w, out);
}

}  // namespace

extern "C" int sydelta_blake3_batch_device(int device, const uint8_t* d_buf, uint64_t buf_len, const uint64_t* offs,
                                           const uint64_t* lens, uint64_t nfiles, void* stream, uint8_t* out) try {
    if (!nfiles) return SYDELTA_OK;
    if (!offs || !lens || !out) return fail(SYDELTA_E_INVAL, "NULL offs/lens/out");
    if (nfiles > 0xFFFFFFFFull) return fail(SYDELTA_E_INVAL, "too many files");
    uint64_t total = 0;
    for (uint64_t f = 0; f < nfiles; ++f) {
        if (offs[f] > buf_len || lens[f] > buf_len - offs[f]) return fail(SYDELTA_E_INVAL, "file range outside the buffer");
        total |= lens[f];
    }
    if (total && !d_buf) return fail(SYDELTA_E_INVAL, "NULL buffer");
    return b3_run(device, d_buf, offs, lens, nfiles, 0, true, stream, out);
} catch (...) {
    return sydelta::host_exception();
}

extern "C" int sydelta_blake3_device(int device, const uint8_t* d_buf, uint64_t len, void* stream, uint8_t out[32]) try {
    if (!out) return fail(SYDELTA_E_INVAL, "NULL out");
    if (!len) {  // a constant: no device needed
        empty_hash(out);
        return SYDELTA_OK;
    }
    const uint64_t off = 0;
    return sydelta_blake3_batch_device(device, d_buf, len, &off, &len, 1, stream, out);
} catch (...) {
    return sydelta::host_exception();
}

extern "C" int sydelta_blake3_subtree_device(int device, const uint8_t* d_buf, uint64_t len, uint64_t first_chunk,
                                             void* stream, uint8_t out_cv[32]) try {
    if (!out_cv) return fail(SYDELTA_E_INVAL, "NULL out_cv");
    if (!len || !d_buf) return fail(SYDELTA_E_INVAL, "an empty piece has no chaining value");
    const uint64_t n = b3::chunks_of(len);
    if (first_chunk + n < first_chunk) return fail(SYDELTA_E_INVAL, "chunk counter overflow");
    const uint64_t off = 0;
    return b3_run(device, d_buf, &off, &len, 1, first_chunk, false, stream, out_cv);
} catch (...) {
    return sydelta::host_exception();
}

extern "C" int sydelta_blake3_join(const uint8_t* cvs, const uint64_t* piece_chunks, uint64_t npieces, uint8_t out[32]) try {
    if (!cvs || !piece_chunks || !out) return fail(SYDELTA_E_INVAL, "NULL argument");
    if (npieces < 2)
        return fail(SYDELTA_E_INVAL, "join needs at least two pieces (a single piece is sydelta_blake3_device's)");
    if (npieces > (1ull << 40)) return fail(SYDELTA_E_INVAL, "too many pieces");
    if (!b3::pieces_ok(piece_chunks, npieces))
        return fail(SYDELTA_E_INVAL, "pieces must be equal powers of two of chunks, the last one 1 to that many");
    b3::join(cvs, npieces, out);
    return SYDELTA_OK;
} catch (...) {
    return sydelta::host_exception();
}

namespace {
struct Fd {
    int fd = -1;
    ~Fd() {
        if (fd >= 0) close(fd);
    }
};
struct Pinned {
    uint8_t* p = nullptr;
    ~Pinned() {
        if (p) (void)hipHostFree(p);
    }
};
struct Event {
    hipEvent_t e = nullptr;
    ~Event() {
        if (e) (void)hipEventDestroy(e);
    }
};

int read_exact(int fd, const char* path, uint64_t off, uint8_t* dst, uint64_t n) {
    uint64_t got = 0;
    while (got < n) {
        const ssize_t r = pread(fd, dst + got, n - got, (off_t)(off + got));
        if (r < 0) {
            if (errno == EINTR) continue;
            return fail(SYDELTA_E_IO, "%s: %s", path, strerror(errno));
        }
        if (r == 0) return fail(SYDELTA_E_IO, "%s: short read at %llu", path, (unsigned long long)(off + got));
        got += (uint64_t)r;
    }
    return SYDELTA_OK;
}
}  // namespace

// Files above one piece: piece k is read into one of two pinned buffers while the device
// still uploads and hashes piece k - 1 from the other; the pieces' chaining values are
// joined on the host.
extern "C" int sydelta_blake3_file(const char* path, uint8_t out[32]) try {
    if (!path || !out) return fail(SYDELTA_E_INVAL, "NULL argument");
    Fd f;
    f.fd = open(path, O_RDONLY | O_CLOEXEC);
    if (f.fd < 0) return fail(SYDELTA_E_IO, "%s: %s", path, strerror(errno));
    struct stat st;
    if (fstat(f.fd, &st) != 0) return fail(SYDELTA_E_IO, "%s: %s", path, strerror(errno));
    const uint64_t len = (uint64_t)st.st_size;
    if (!len) {
        empty_hash(out);
        return SYDELTA_OK;
    }
    int dev = 0;
    if (int r = path_device(&dev)) return r;
    SYDELTA_ENTER_DEVICE(dev);
    hipStream_t s = thread_stream(dev);
    const uint64_t piece = std::min(len, kFilePiece), npieces = (len + kFilePiece - 1) / kFilePiece;
    const int nbuf = npieces > 1 ? 2 : 1;
    Pinned pin[2];
    DevBuf dbuf[2], d_cvs;
    Event ev[2];
    for (int b = 0; b < nbuf; ++b) {
        HIP_TRY(hipHostMalloc((void**)&pin[b].p, piece, hipHostMallocDefault));
        HIP_TRY(dbuf[b].alloc(piece, s));
        HIP_TRY(hipEventCreateWithFlags(&ev[b].e, hipEventDisableTiming));
    }
    HIP_TRY(d_cvs.alloc(npieces * 32, s));
    CallProf cp;
    for (uint64_t k = 0; k < npieces; ++k) {
        const int b = (int)(k & 1);
        const uint64_t off = k * kFilePiece, n = std::min(kFilePiece, len - off), zero = 0;
        if (k >= 2) HIP_TRY(hipEventSynchronize(ev[b].e));  // piece k - 2 has left this pinned buffer
        if (int r = read_exact(f.fd, path, off, pin[b].p, n)) {
            (void)hipStreamSynchronize(s);
            return r;
        }
        HIP_TRY(hipMemcpyAsync(dbuf[b].p, pin[b].p, n, hipMemcpyHostToDevice, s));
        HIP_TRY(hipEventRecord(ev[b].e, s));
        if (int r = b3_enqueue((const uint8_t*)dbuf[b].p, &zero, &n, 1, k << 16, npieces == 1,
                               (uint8_t*)d_cvs.p + 32 * k, s, cp.get())) {
            (void)hipStreamSynchronize(s);
            return r;
        }
    }
    std::vector<uint8_t> cvs(npieces * 32);
    HIP_TRY(hipMemcpyAsync(cvs.data(), d_cvs.p, cvs.size(), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (npieces == 1) {
        memcpy(out, cvs.data(), 32);
        return SYDELTA_OK;
    }
    std::vector<uint64_t> pc(npieces, kFilePiece / b3::kChunkLen);
    pc.back() = b3::chunks_of(len - (npieces - 1) * kFilePiece);
    return sydelta_blake3_join(cvs.data(), pc.data(), npieces, out);
} catch (...) {
    return sydelta::host_exception();
}
