// apply_batch_check.cpp — the batched apply's host plan (validation, merging, slices, tile
// table) and its span copy body (sy_amd/csrc/sydelta_applybatch.hpp) on host memory, under
// ASan + UBSan.  Seeded random batches are planned, cut into slices and copied tile by tile,
// thread by thread, through a memory policy that holds the three arenas at their exact
// sizes: a byte access outside its arena, a 16-byte load of a granule that holds no byte the
// piece needs, an unaligned 16-byte access and any store outside the output arena fail the
// run, and the arena is compared with a byte loop over the ops (every byte outside the
// outputs still the sentinel).  Then every refusal of the contract, each naming its file
// and op.
//
//   apply_batch_check <batches> <seed>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "sydelta_applybatch.hpp"

using namespace sydelta::applyb;

namespace {

uint64_t g_rng = 1;
uint64_t rnd() {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return g_rng;
}
uint64_t below(uint64_t n) { return n ? rnd() % n : 0; }

[[noreturn]] void die(const char* what, uint64_t batch) {
    printf("FAIL batch %llu: %s\n", (unsigned long long)batch, what);
    exit(1);
}

// An arena of exactly `len` bytes that ends where its allocation ends and starts at a
// random alignment.
struct Arena {
    uint8_t* raw = nullptr;
    uint8_t* p = nullptr;
    uint64_t len = 0, slack = 0;
    void make(uint64_t n, uint8_t fill) {
        slack = below(16);
        raw = (uint8_t*)malloc(n + slack + 1);
        // + 1: malloc(0) stays valid; the byte is kept in front so the end is exact
        memset(raw, 0xA5, slack + 1);
        p = raw + slack + 1;
        len = n;
        memset(p, fill, n);
    }
    bool front_clean() const {
        for (uint64_t i = 0; i < slack + 1; ++i)
            if (raw[i] != 0xA5) return false;
        return true;
    }
    ~Arena() { free(raw); }
    bool holds(uintptr_t x) const { return x >= (uintptr_t)p && x < (uintptr_t)p + len; }
};

uint64_t g_batch = 0;
struct HostMem {
    const Arena *basis, *lit, *out;
    uint8_t ldb(uintptr_t x) const {
        if (!basis->holds(x) && !lit->holds(x)) die("byte load outside the arenas", g_batch);
        return *(const uint8_t*)x;
    }
    void stb(uintptr_t x, uint8_t b) const {
        if (!out->holds(x)) die("byte store outside the output arena", g_batch);
        *(uint8_t*)x = b;
    }
    Q16 ld16(uintptr_t p, uintptr_t need0, uintptr_t need1) const {
        if (p & 15) die("unaligned 16-byte load", g_batch);
        if (!(p < need1 && p + 16 > need0)) die("16-byte load of a granule the piece does not need", g_batch);
        uint8_t b[16];
        for (int i = 0; i < 16; ++i)  // the granule rule: bytes outside the arena are never looked at
            b[i] = (basis->holds(p + i) || lit->holds(p + i)) ? *(const uint8_t*)(p + i) : 0;
        Q16 q;
        memcpy(q.w, b, 16);
        return q;
    }
    void st16(uintptr_t p, const Q16& q) const {
        if (p & 15) die("unaligned 16-byte store", g_batch);
        if (!out->holds(p) || !out->holds(p + 15)) die("16-byte store outside the output arena", g_batch);
        memcpy((void*)p, q.w, 16);
    }
};

struct File {
    std::vector<sydelta_op> ops;
    uint64_t basis_off, basis_len, lit_off, lit_len, out_off, out_cap, bytes;
};

uint64_t op_size() {
    const uint64_t k = below(100);
    if (k < 10) return 0;
    if (k < 50) return 1 + below(40);
    if (k < 85) return 41 + below(5000);
    if (k < 97) return below(70000);
    return below(200 * 1024 + 1);
}

// ops of one file: contiguous and non-contiguous neighbours of both kinds
void make_ops(File& F, uint64_t nops, bool tiny) {
    uint64_t end[2] = {0, 0};  // where the previous op of each kind ended
    uint32_t prev = 2;
    for (uint64_t i = 0; i < nops; ++i) {
        sydelta_op o{};
        o.kind = (prev < 2 && below(3) == 0) ? prev : (uint32_t)below(2);
        const uint64_t range = o.kind == SYDELTA_OP_COPY ? F.basis_len : F.lit_len;
        o.a = (prev == o.kind && below(2)) ? end[o.kind] : below(range + 1);
        o.b = tiny ? 1 + below(3) : op_size();
        if (o.a > range) o.a = range;
        if (o.b > range - o.a) o.b = range - o.a;
        end[o.kind] = o.a + o.b;
        prev = o.kind;
        F.bytes += o.b;
        F.ops.push_back(o);
    }
}

int plan_all(const std::vector<File>& files, const Arenas& A, std::vector<std::vector<Run>>& runs,
             std::vector<sydelta_apply_stats>& st, Err* e, const std::vector<bool>* null_delta = nullptr) {
    runs.assign(files.size(), {});
    st.assign(files.size(), sydelta_apply_stats{});
    for (size_t f = 0; f < files.size(); ++f) {
        const File& F = files[f];
        const FileIn in{F.ops.empty() ? nullptr : F.ops.data(), F.ops.size(), !(null_delta && (*null_delta)[f]),
                        F.basis_off, F.basis_len, F.lit_off, F.lit_len, F.out_off, F.out_cap};
        if (int rc = plan_file(f, in, A, runs[f], &st[f], e)) return rc;
    }
    return 0;
}

void one_batch(uint64_t batch) {
    g_batch = batch;
    const bool many = batch % 400 == 399;  // more runs than a slice holds: a file cut between slices
    const uint64_t nfiles = 1 + below(40);
    std::vector<File> files(nfiles);
    uint64_t bpos = below(20), lpos = below(20), opos = below(20);
    const bool packed = below(2);
    for (uint64_t f = 0; f < nfiles; ++f) {
        File& F = files[f];
        F.bytes = 0;
        auto len = [&]() -> uint64_t {
            const uint64_t k = below(10);
            return k == 0 ? 0 : k < 6 ? below(300) : k < 9 ? below(20000) : below(300 * 1024);
        };
        F.basis_len = len();
        F.lit_len = len();
        F.basis_off = bpos;
        F.lit_off = lpos;
        bpos += F.basis_len + (below(2) ? 0 : below(40));
        lpos += F.lit_len + (below(2) ? 0 : below(40));
        if (many && f == nfiles / 2) {
            if (F.basis_len < 64) F.basis_len = 64, bpos += 64;
            if (F.lit_len < 64) F.lit_len = 64, lpos += 64;
            make_ops(F, 3 * kSliceRuns + below(3000), true);  // about a third of the neighbours merge
        } else {
            const uint64_t k = below(20);
            make_ops(F, k == 0 ? 0 : k < 15 ? below(30) : k < 19 ? below(300) : below(3000), k == 19);
        }
        F.out_off = opos;
        F.out_cap = F.bytes + (packed ? 0 : below(3) ? 0 : below(50));
        opos += F.out_cap + (packed ? 0 : below(3) ? 0 : below(40));
    }
    Arena basis, lit, out;
    basis.make(bpos, 0);
    lit.make(lpos, 0);
    out.make(opos + (packed ? 0 : below(20)), 0xEE);
    for (uint64_t i = 0; i < basis.len; ++i) basis.p[i] = (uint8_t)rnd();
    for (uint64_t i = 0; i < lit.len; ++i) lit.p[i] = (uint8_t)rnd();
    std::vector<uint8_t> want(out.len, 0xEE);
    std::vector<sydelta_apply_stats> wst(nfiles);
    for (uint64_t f = 0; f < nfiles; ++f) {  // the byte loop
        const File& F = files[f];
        uint64_t at = F.out_off;
        wst[f] = sydelta_apply_stats{F.ops.size(), 0, 0};
        for (const sydelta_op& o : F.ops) {
            const uint8_t* src = o.kind == SYDELTA_OP_COPY ? basis.p + F.basis_off : lit.p + F.lit_off;
            for (uint64_t i = 0; i < o.b; ++i) want[at + i] = src[o.a + i];
            at += o.b;
            if (o.kind == SYDELTA_OP_DATA) wst[f].literal_bytes += o.b;
        }
        wst[f].bytes_written = at - F.out_off;
    }

    const Arenas A{basis.len, lit.len, out.len};
    std::vector<std::vector<Run>> runs;
    std::vector<sydelta_apply_stats> st;
    Err e;
    if (plan_all(files, A, runs, st, &e)) die(e.msg.c_str(), batch);
    for (uint64_t f = 0; f < nfiles; ++f) {
        if (memcmp(&st[f], &wst[f], sizeof st[f])) die("stats differ", batch);
        for (size_t i = 1; i < runs[f].size(); ++i) {  // merged: no two neighbours contiguous in one source
            const Run &a = runs[f][i - 1], &b = runs[f][i];
            if (a.dst + a.len != b.dst) die("runs leave a gap in the output", batch);
            if (a.from_basis == b.from_basis && a.src + a.len == b.src) die("unmerged neighbours", batch);
        }
    }
    std::vector<FileRuns> fr(nfiles);
    for (uint64_t f = 0; f < nfiles; ++f) fr[f] = FileRuns{runs[f].data(), runs[f].size()};
    std::vector<Run> sr(kSliceRuns);
    std::vector<Seg> ss(kSliceSegs);
    Cursor c, c2;
    Slice sl, sl2;
    HostMem m{&basis, &lit, &out};
    static const uint32_t kThr[4] = {1, 5, 64, 256};
    const uint32_t nthr = many ? 16 : kThr[below(4)];
    uint64_t nslices = 0;
    while (next_slice(fr.data(), nfiles, (uintptr_t)out.p, c, sr.data(), ss.data(), &sl)) {
        if (!next_slice(fr.data(), nfiles, (uintptr_t)out.p, c2, nullptr, nullptr, &sl2) || sl2.nruns != sl.nruns ||
            sl2.nsegs != sl.nsegs || sl2.ntiles != sl.ntiles)
            die("the counting pass disagrees with the filling pass", batch);
        // a slice's tables at their exact sizes
        std::vector<Run> xr(sr.begin(), sr.begin() + sl.nruns);
        std::vector<Seg> xs(ss.begin(), ss.begin() + sl.nsegs);
        for (uint64_t t = 0; t < sl.ntiles; ++t)
            for (uint32_t tid = 0; tid < nthr; ++tid)
                copy_tile(m, tid, nthr, t, xr.data(), xs.data(), sl.nsegs, (uintptr_t)basis.p, (uintptr_t)lit.p,
                          (uintptr_t)out.p);
        ++nslices;
    }
    if (many && nslices < 2) die("the large file did not span slices", batch);
    if (memcmp(out.p, want.data(), out.len)) {
        uint64_t i = 0;
        while (out.p[i] == want[i]) ++i;
        printf("first difference at output byte %llu\n", (unsigned long long)i);
        die("output differs from the byte loop", batch);
    }
    if (!out.front_clean()) die("bytes in front of the output arena changed", batch);
}

// --- refusals ---------------------------------------------------------------
int g_refusals = 0;
void expect(std::vector<File> files, const Arenas& A, int code, const char* where, const char* what,
            const std::vector<bool>* nulls = nullptr) {
    std::vector<std::vector<Run>> runs;
    std::vector<sydelta_apply_stats> st;
    Err e;
    const int rc = plan_all(files, A, runs, st, &e, nulls);
    if (rc != code || e.code != code || e.msg.find(where) != 0 || e.msg.find(what) == std::string::npos) {
        printf("FAIL refusal: wanted %d '%s' ... '%s', got %d '%s'\n", code, where, what, rc, e.msg.c_str());
        exit(1);
    }
    printf("reject %s\n", e.msg.c_str());
    ++g_refusals;
}

void refusals() {
    // 20 good files of 100 ops; file 13's op 77 is replaced
    const uint64_t N = 20, L = 5000;
    std::vector<File> good(N);
    for (uint64_t f = 0; f < N; ++f) {
        File& F = good[f];
        F.basis_off = f * L, F.basis_len = L, F.lit_off = f * L + 3, F.lit_len = L - 3;
        F.bytes = 0;
        for (int i = 0; i < 100; ++i) {
            sydelta_op o{};
            o.kind = i & 1;
            o.a = below(L - 200);
            o.b = 1 + below(100);
            F.ops.push_back(o);
            F.bytes += o.b;
        }
        F.out_off = f ? good[f - 1].out_off + good[f - 1].out_cap : 7;
        F.out_cap = F.bytes;
    }
    const Arenas A{N * L, N * L, good[N - 1].out_off + good[N - 1].out_cap};
    {
        std::vector<std::vector<Run>> runs;
        std::vector<sydelta_apply_stats> st;
        Err e;
        if (plan_all(good, A, runs, st, &e)) die("the good batch was refused", 0);
    }
    auto with = [&](uint64_t f, uint64_t i, uint32_t kind, uint64_t a, uint64_t b) {
        std::vector<File> v = good;
        v[f].ops[i].kind = kind, v[f].ops[i].a = a, v[f].ops[i].b = b;
        return v;
    };
    const char* at = "file 13: op 77:";
    // one byte past file 13's basis, still inside the arena
    expect(with(13, 77, SYDELTA_OP_COPY, L - 9, 10), A, SYDELTA_E_IO, at, "past the end of the basis");
    expect(with(13, 77, SYDELTA_OP_COPY, L + 1, 0), A, SYDELTA_E_IO, at, "past the end of the basis");
    expect(with(13, 77, SYDELTA_OP_COPY, UINT64_MAX, 2), A, SYDELTA_E_IO, at, "past the end of the basis");
    expect(with(13, 77, SYDELTA_OP_COPY, 2, UINT64_MAX), A, SYDELTA_E_IO, at, "past the end of the basis");
    expect(with(13, 77, SYDELTA_OP_DATA, L - 3 - 9, 10), A, SYDELTA_E_INVAL, at, "outside the literal range");
    expect(with(13, 77, SYDELTA_OP_DATA, UINT64_MAX - 1, 5), A, SYDELTA_E_INVAL, at, "outside the literal range");
    expect(with(13, 77, SYDELTA_OP_DATA, 5, UINT64_MAX - 1), A, SYDELTA_E_INVAL, at, "outside the literal range");
    expect(with(13, 77, 2, 0, 1), A, SYDELTA_E_INVAL, at, "unknown kind");
    {  // the output one byte above its capacity: the op that crosses it is named
        std::vector<File> v = good;
        v[13].out_cap -= 1;
        expect(v, A, SYDELTA_E_INVAL, "file 13: op 99:", "more than its capacity");
        v = good;
        v[13].ops[77].b += 1;  // (a + b stays inside the ranges)
        expect(v, A, SYDELTA_E_INVAL, "file 13: op 99:", "more than its capacity");
    }
    {  // ranges that leave their arena, wrapping ones included
        std::vector<File> v = good;
        v[19].basis_len += 1;
        expect(v, A, SYDELTA_E_INVAL, "file 19:", "basis range");
        v = good;
        v[4].basis_off = UINT64_MAX - 10;
        expect(v, A, SYDELTA_E_INVAL, "file 4:", "basis range");
        v = good;
        v[19].lit_len += 1;
        expect(v, A, SYDELTA_E_INVAL, "file 19:", "literal range");
        v = good;
        v[6].lit_off = UINT64_MAX, v[6].lit_len = 2;
        expect(v, A, SYDELTA_E_INVAL, "file 6:", "literal range");
        v = good;
        v[19].out_cap += 1;
        expect(v, A, SYDELTA_E_INVAL, "file 19:", "output range");
        v = good;
        v[0].out_off = UINT64_MAX - 3;
        expect(v, A, SYDELTA_E_INVAL, "file 0:", "output range");
    }
    {
        std::vector<bool> nulls(N, false);
        nulls[9] = true;
        expect(good, A, SYDELTA_E_INVAL, "file 9:", "NULL delta", &nulls);
    }
    {  // two bad files: the first is reported
        std::vector<File> v = with(13, 77, SYDELTA_OP_COPY, L - 9, 10);
        v[5].ops[3] = sydelta_op{SYDELTA_OP_DATA, 0, L, 1};
        expect(v, A, SYDELTA_E_INVAL, "file 5: op 3:", "outside the literal range");
    }
}

}  // namespace

int main(int argc, char** argv) {
    const uint64_t batches = argc > 1 ? strtoull(argv[1], nullptr, 10) : 2000;
    g_rng = (argc > 2 ? strtoull(argv[2], nullptr, 10) : 7) * 0x9E3779B97F4A7C15ull + 1;
    refusals();
    for (uint64_t b = 0; b < batches; ++b) one_batch(b);
    printf("apply_batch_check ok: %llu batches, %d refusals\n", (unsigned long long)batches, g_refusals);
    return 0;
}
