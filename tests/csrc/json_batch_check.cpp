// json_batch_check.cpp — the batched Delta JSON writer's host plan (validation, tiles, slices)
// and its per-thread bodies (sy_amd/csrc/sydelta_jsonbatch.hpp) on host memory, under ASan +
// UBSan.  Seeded random batches are planned, cut into slices, sized lane by lane, placed by
// the scans the entry point queues and written tile by tile, thread by thread, through a
// memory policy that holds the literal arena and the output arena at their exact sizes: a
// load of a granule that holds no byte of the tile's chunk, an unaligned wide access and any
// store outside the tile's own text fail the run.  Every text is compared with a plain writer
// (snprintf over the ops, the literal bytes digit by digit), every byte outside the texts must still be the sentinel.  Then
// every refusal of the contract, each naming its file and op.
//
//   json_batch_check <batches> <seed>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "sydelta_jsonbatch.hpp"

using namespace sydelta::jsonb;

namespace {

uint64_t g_rng = 1;
uint64_t rnd() {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return g_rng;
}
uint64_t below(uint64_t n) { return n ? rnd() % n : 0; }

uint64_t g_batch = 0;
[[noreturn]] void die(const char* what) {
    printf("FAIL batch %llu: %s\n", (unsigned long long)g_batch, what);
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
        memset(raw, 0xA5, slack + 1);  // + 1: malloc(0) stays valid; the byte is kept in front
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

struct HostMem {
    const Arena *lit, *out;
    uintptr_t need0 = 0, need1 = 0;  // the chunk's literal bytes
    uintptr_t d0 = 0, d1 = 0;        // the tile's text
    void wide_load(uintptr_t p, uint32_t n, uint8_t* b) const {
        if (p % n) die("unaligned wide load");
        if (!(p < need1 && p + n > need0)) die("wide load that holds no byte of the chunk");
        for (uint32_t i = 0; i < n; ++i)  // the granule rule: bytes outside the arena are never looked at
            b[i] = lit->holds(p + i) ? *(const uint8_t*)(p + i) : 0;
    }
    Q16 ld16(uintptr_t p) const {
        Q16 q;
        uint8_t b[16];
        wide_load(p, 16, b);
        memcpy(q.w, b, 16);
        return q;
    }
    uint32_t ld4(uintptr_t p) const {
        uint32_t v;
        uint8_t b[4];
        wide_load(p, 4, b);
        memcpy(&v, b, 4);
        return v;
    }
    uint8_t ldb(uintptr_t p) const {
        if (p < need0 || p >= need1) die("byte load outside the chunk");
        return *(const uint8_t*)p;
    }
    void st16(uintptr_t p, const uint8_t* js) const {
        if (p & 15) die("unaligned 16-byte store");
        if (p < d0 || p + 16 > d1 || !out->holds(p) || !out->holds(p + 15)) die("16-byte store outside the tile's text");
        memcpy((void*)p, js, 16);
    }
    void stb(uintptr_t p, uint8_t b) const {
        if (p < d0 || p >= d1 || !out->holds(p)) die("byte store outside the tile's text");
        *(uint8_t*)p = b;
    }
};

struct File {
    std::vector<sydelta_op> ops;
    uint64_t source_size, block_size, lit_off, lit_len;
};

// digit-class edges: 0, 9, 10, 99, 100, ..., 2^32 and its neighbours, 2^64 - 1
uint64_t edge() {
    const uint64_t k = below(44);
    if (k == 0) return 0;
    if (k == 41) return 1ull << 32;
    if (k == 42) return (1ull << 32) - 1;
    if (k == 43) return UINT64_MAX;
    uint64_t p = 1;  // 10^((k + 1) / 2), k = 1..40
    for (uint64_t i = 0; i < (k + 1) / 2; ++i) p *= 10;
    if ((k + 1) / 2 == 20) return UINT64_MAX - below(3);
    return (k & 1) ? p - 1 : p;
}
uint64_t field() { return below(4) ? edge() : rnd() >> below(64); }

uint64_t data_size() {
    const uint64_t k = below(200);
    if (k < 20) return 0;
    if (k < 130) return 1 + below(40);
    if (k < 190) return 41 + below(300);
    if (k < 198) return below(4200);  // around one chunk
    return below(20001);
}

void make_ops(File& F, uint64_t nops, int mode) {  // mode 0: mixed, 1: Copies, 2: tiny Data
    uint32_t prev = 0;
    for (uint64_t i = 0; i < nops; ++i) {
        sydelta_op o{};
        o.kind = mode == 1 ? SYDELTA_OP_COPY : mode == 2 ? SYDELTA_OP_DATA : below(4) ? prev : (uint32_t)below(2);
        prev = o.kind;
        if (o.kind == SYDELTA_OP_COPY) {
            o.a = field(), o.b = field();
        } else {
            o.b = mode == 2 ? below(3) : data_size();
            if (o.b > F.lit_len) o.b = F.lit_len;
            o.a = below(F.lit_len - o.b + 1);
        }
        F.ops.push_back(o);
    }
}

std::string plain(const File& F, const uint8_t* lit) {  // the independent writer
    std::string s = "{\"ops\":[";
    char t[96];
    for (size_t i = 0; i < F.ops.size(); ++i) {
        const sydelta_op& o = F.ops[i];
        if (i) s += ',';
        if (o.kind == SYDELTA_OP_COPY) {
            snprintf(t, sizeof t, "{\"Copy\":{\"offset\":%llu,\"size\":%llu}}", (unsigned long long)o.a, (unsigned long long)o.b);
            s += t;
        } else {
            s += "{\"Data\":[";
            for (uint64_t k = 0; k < o.b; ++k) {
                const unsigned v = lit[F.lit_off + o.a + k];
                if (k) s += ',';
                if (v >= 100) s += (char)('0' + v / 100);
                if (v >= 10) s += (char)('0' + v / 10 % 10);
                s += (char)('0' + v % 10);
            }
            s += "]}";
        }
    }
    snprintf(t, sizeof t, "],\"source_size\":%llu,\"block_size\":%llu}", (unsigned long long)F.source_size,
             (unsigned long long)F.block_size);
    return s + t;
}

FileIn file_in(const File& F, bool has = true) {
    return FileIn{F.ops.empty() ? nullptr : F.ops.data(), F.ops.size(), has, F.source_size, F.block_size, F.lit_off, F.lit_len};
}

uint64_t g_tiles = 0, g_slices = 0, g_bytes = 0;

void one_batch(uint64_t batch) {
    g_batch = batch;
    const int big = batch % 400 == 399 ? 1 : batch % 400 == 199 ? 2 : 0;  // a file cut between slices
    const uint64_t nfiles = 1 + below(40);
    std::vector<File> files(nfiles);
    uint64_t lpos = below(20);
    for (uint64_t f = 0; f < nfiles; ++f) {
        File& F = files[f];
        F.source_size = field(), F.block_size = field();
        const uint64_t k = below(10);
        F.lit_len = k == 0 ? 0 : k < 5 ? below(300) : k < 9 ? below(6000) : below(30000);
        F.lit_off = lpos;
        lpos += F.lit_len + (below(2) ? 0 : below(40));
        if (big && f == nfiles / 2) {
            if (F.lit_len < 2) F.lit_len = 2, lpos += 2;
            make_ops(F, big == 1 ? kSlicePairs + 300 + below(3000) : kSliceTiles + 100 + below(1000), big);
        } else {
            const uint64_t q = below(40);
            make_ops(F, q < 4 ? 0 : q < 32 ? below(12) : q < 39 ? below(80) : below(601), below(8) == 0 ? 1 : 0);
        }
    }
    Arena lit;
    lit.make(lpos, 0);
    const uint64_t fill = below(8);  // all 0, all 255, small values, or random bytes
    for (uint64_t i = 0; i < lit.len; ++i)
        lit.p[i] = fill == 0 ? 0 : fill == 1 ? 255 : fill == 2 ? (uint8_t)below(12) : fill == 3 ? (uint8_t)(90 + below(20)) : (uint8_t)rnd();

    // plan
    std::vector<FileIn> in(nfiles);
    std::vector<Count> fc(nfiles);
    Count cnt;
    Err e;
    uint64_t literal = 0, lit_sum = 0;
    for (uint64_t f = 0; f < nfiles; ++f) {
        in[f] = file_in(files[f]);
        if (count_file(f, in[f], lit.len, &fc[f], &literal, &e)) die(e.msg.c_str());
        cnt.tiles += fc[f].tiles, cnt.pairs += fc[f].pairs;
        for (const sydelta_op& o : files[f].ops)
            if (o.kind == SYDELTA_OP_DATA) lit_sum += o.b;
    }
    if (literal != lit_sum) die("literal bytes miscounted");
    // the device tables at their exact sizes; a slice's tables at the ring's
    std::vector<Tile> tiles(cnt.tiles), st(kSliceTiles);
    std::vector<Pair> pairs(cnt.pairs), sp(kSlicePairs);
    Cursor c, c2;
    Slice sl, sl2;
    uint64_t t0 = 0, p0 = 0, nslices = 0;
    while (next_slice(in.data(), fc.data(), nfiles, c, p0, st.data(), sp.data(), &sl)) {
        if (!next_slice(in.data(), fc.data(), nfiles, c2, p0, nullptr, nullptr, &sl2) || sl2.ntiles != sl.ntiles ||
            sl2.npairs != sl.npairs || c2.file != c.file || c2.op != c.op || c2.chunk != c.chunk)
            die("the counting pass disagrees with the filling pass");
        if (sl.ntiles > kSliceTiles || sl.npairs > kSlicePairs) die("a slice larger than the ring's");
        if (t0 + sl.ntiles > cnt.tiles || p0 + sl.npairs > cnt.pairs) die("more tiles or pairs than counted");
        memcpy(tiles.data() + t0, st.data(), sl.ntiles * sizeof(Tile));
        memcpy(pairs.data() + p0, sp.data(), sl.npairs * sizeof(Pair));
        t0 += sl.ntiles, p0 += sl.npairs, ++nslices;
    }
    if (t0 != cnt.tiles || p0 != cnt.pairs) die("fewer tiles or pairs than counted");
    if (big && nslices < 2) die("the large file did not span slices");
    g_tiles += cnt.tiles, g_slices += nslices;

    // sizing: a wave per tile
    HostMem m{&lit, nullptr};
    std::vector<uint64_t> len(cnt.tiles), off(cnt.tiles), fstart(nfiles + 1, UINT64_MAX), tlen(nfiles), toff(nfiles);
    for (uint64_t t = 0; t < cnt.tiles; ++t) {
        const Tile& T = tiles[t];
        if (T.file >= nfiles) die("a tile of no file");
        if (T.flags & kData) m.need0 = (uintptr_t)lit.p + T.src, m.need1 = m.need0 + T.n;
        uint32_t sum = 0;
        for (uint32_t lane = 0; lane < 64; ++lane) sum += size_lane(m, T, pairs.data(), (uintptr_t)lit.p, lane);
        len[t] = (uint64_t)T.fixed + sum;
    }
    uint64_t acc = 0;
    for (uint64_t t = 0; t < cnt.tiles; ++t) off[t] = acc, acc += len[t];
    for (uint64_t t = 0; t < cnt.tiles; ++t)
        if (tiles[t].flags & kHead) fstart[tiles[t].file] = off[t];
    fstart[nfiles] = acc;
    uint64_t need = 0;
    for (uint64_t f = 0; f < nfiles; ++f) {
        if (fstart[f] == UINT64_MAX) die("a file without a first tile");
        tlen[f] = fstart[f + 1] - fstart[f];
        toff[f] = need;
        need += (tlen[f] + 15) & ~15ull;
    }
    need = toff[nfiles - 1] + tlen[nfiles - 1];

    // the expected texts, and the bounds from the ops alone
    std::vector<std::string> want(nfiles);
    uint64_t bound = 0;
    for (uint64_t f = 0; f < nfiles; ++f) {
        want[f] = plain(files[f], lit.p);
        uint64_t lo, hi;
        if (!text_bounds(in[f].ops, in[f].nops, in[f].source_size, in[f].block_size, &lo, &hi)) die("no bounds");
        if (want[f].size() < lo || want[f].size() > hi) die("the text is outside its bounds");
        if (tlen[f] != want[f].size()) die("sized length differs from the plain writer's");
        if (fc[f].lo > lo || fc[f].hi < hi) die("the plan's loose bounds are inside the exact ones");
        bound += (hi + 15) & ~15ull;
    }
    if (need > bound) die("the packed size is above the bound");

    // writing: a workgroup per tile
    Arena out;
    out.make(need + (below(2) ? 0 : below(20)), 0xA5);
    m.out = &out;
    uint8_t* js = (uint8_t*)malloc(kStage);
    std::vector<Thread> th(kThreads);
    std::vector<uint32_t> pre(kThreads);
    static const uint32_t kThr[3] = {kThreads, 64, 1};  // the store loop is strided: any thread count
    const uint32_t nthr = kThr[below(3)];
    for (uint64_t t = 0; t < cnt.tiles; ++t) {
        const Tile& T = tiles[t];
        const uintptr_t oaddr = (uintptr_t)out.p + toff[T.file] + (off[t] - fstart[T.file]);
        const uint32_t ph = (uint32_t)(oaddr & 15);
        if (T.flags & kData) m.need0 = (uintptr_t)lit.p + T.src, m.need1 = m.need0 + T.n;
        m.d0 = oaddr, m.d1 = oaddr + len[t];
        memset(js, 0xEE, ph + len[t] + 32 < kStage ? ph + len[t] + 32 : kStage);
        uint32_t body = 0;
        for (uint32_t tid = 0; tid < kThreads; ++tid) {
            pre[tid] = body;
            body += thread_len(m, T, pairs.data(), (uintptr_t)lit.p, tid, th[tid]);
        }
        for (uint32_t tid = 0; tid < kThreads; ++tid) thread_format(js, T, ph, pre[tid], tid, th[tid]);
        const uint32_t end = tile_close(js, T, pairs.data(), ph, body);
        if (end != ph + len[t]) die("the written length differs from the sized one");
        if (end > kStage) die("staging overflow");
        for (uint32_t tid = 0; tid < nthr; ++tid) thread_store(m, js, ph, end, oaddr - ph, tid, nthr);
    }
    free(js);

    std::vector<uint8_t> img(out.len, 0xA5);
    for (uint64_t f = 0; f < nfiles; ++f) memcpy(img.data() + toff[f], want[f].data(), want[f].size());
    if (out.len && memcmp(out.p, img.data(), out.len)) {
        uint64_t i = 0;
        while (out.p[i] == img[i]) ++i;
        printf("first difference at output byte %llu\n", (unsigned long long)i);
        die("output differs from the plain writer's (texts, or a byte outside them)");
    }
    if (!out.front_clean()) die("bytes in front of the output arena changed");
    g_bytes += need;
}

// --- refusals ---------------------------------------------------------------
int g_refusals = 0;
void expect(const std::vector<File>& files, uint64_t arena, const char* where, const char* what,
            const std::vector<bool>* nulls = nullptr) {
    Err e;
    Count cnt;
    uint64_t literal = 0;
    int rc = 0;
    for (size_t f = 0; f < files.size() && !rc; ++f)
        rc = count_file(f, file_in(files[f], !(nulls && (*nulls)[f])), arena, &cnt, &literal, &e);
    if (rc != SYDELTA_E_INVAL || e.code != rc || e.msg.find(where) != 0 || e.msg.find(what) == std::string::npos) {
        printf("FAIL refusal: wanted '%s' ... '%s', got %d '%s'\n", where, what, rc, e.msg.c_str());
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
        F.source_size = 1 << 20, F.block_size = 4096, F.lit_off = f * L + 3, F.lit_len = L - 3;
        for (int i = 0; i < 100; ++i) {
            sydelta_op o{};
            o.kind = i & 1;
            o.a = below(L - 200);
            o.b = 1 + below(100);
            F.ops.push_back(o);
        }
    }
    const uint64_t A = N * L;
    {
        Err e;
        Count cnt;
        uint64_t literal = 0;
        for (uint64_t f = 0; f < N; ++f)
            if (count_file(f, file_in(good[f]), A, &cnt, &literal, &e)) die("the good batch was refused");
    }
    auto with = [&](uint64_t f, uint64_t i, uint32_t kind, uint64_t a, uint64_t b) {
        std::vector<File> v = good;
        v[f].ops[i].kind = kind, v[f].ops[i].a = a, v[f].ops[i].b = b;
        return v;
    };
    const char* at = "file 13: op 77:";
    // one byte past file 13's literal range, still inside the arena
    expect(with(13, 77, SYDELTA_OP_DATA, L - 3 - 9, 10), A, at, "outside the literal range");
    expect(with(13, 77, SYDELTA_OP_DATA, L - 2, 0), A, at, "outside the literal range");
    expect(with(13, 77, SYDELTA_OP_DATA, UINT64_MAX - 1, 5), A, at, "outside the literal range");
    expect(with(13, 77, SYDELTA_OP_DATA, 5, UINT64_MAX - 1), A, at, "outside the literal range");
    expect(with(13, 77, 2, 0, 1), A, at, "unknown kind");
    {  // literal ranges that leave the arena, a wrapping one included
        std::vector<File> v = good;
        v[19].lit_len += 1;
        expect(v, A, "file 19:", "literal range");
        v = good;
        v[6].lit_off = UINT64_MAX, v[6].lit_len = 2;
        expect(v, A, "file 6:", "literal range");
    }
    {
        std::vector<bool> nulls(N, false);
        nulls[9] = true;
        expect(good, A, "file 9:", "NULL delta", &nulls);
    }
    {  // two bad files: the first is reported
        std::vector<File> v = with(13, 77, 2, 0, 1);
        v[5].ops[3] = sydelta_op{SYDELTA_OP_DATA, 0, L, 1};
        expect(v, A, "file 5: op 3:", "outside the literal range");
    }
    // a Copy op is never refused: its fields are only printed
    {
        Err e;
        Count cnt;
        uint64_t literal = 0;
        std::vector<File> v = with(13, 76, SYDELTA_OP_COPY, UINT64_MAX, UINT64_MAX);
        for (uint64_t f = 0; f < N; ++f)
            if (count_file(f, file_in(v[f]), A, &cnt, &literal, &e)) die("a Copy op was refused");
    }
}

void digits() {
    uint64_t p = 1;
    for (uint32_t n = 1; n <= 20; ++n) {  // 10^(n-1) has n digits, one less has n - 1
        if (dec_digits(p) != n || (n > 1 && dec_digits(p - 1) != n - 1)) die("dec_digits");
        uint8_t b[24];
        char t[24];
        const int k = snprintf(t, sizeof t, "%llu", (unsigned long long)(p - 1));
        if (put_dec(b, p - 1) != (uint32_t)k || memcmp(b, t, k)) die("put_dec");
        if (n < 20) p *= 10;
    }
    if (dec_digits(UINT64_MAX) != 20 || dec_digits(0) != 1) die("dec_digits at the ends");
}

}  // namespace

int main(int argc, char** argv) {
    const uint64_t batches = argc > 1 ? strtoull(argv[1], nullptr, 10) : 2000;
    g_rng = (argc > 2 ? strtoull(argv[2], nullptr, 10) : 7) * 0x9E3779B97F4A7C15ull + 1;
    digits();
    refusals();
    for (uint64_t b = 0; b < batches; ++b) one_batch(b);
    printf("json_batch_check ok: %llu batches, %llu tiles, %llu slices, %llu text bytes, %d refusals\n",
           (unsigned long long)batches, (unsigned long long)g_tiles, (unsigned long long)g_slices,
           (unsigned long long)g_bytes, g_refusals);
    return 0;
}
