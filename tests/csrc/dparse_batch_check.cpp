// dparse_batch_check.cpp — the batched Delta JSON parse (sy_amd/csrc/sydelta_dparsebatch.hpp
// over the chunk bodies of sydelta_dparse.hpp and the wave replica of dparse_wave.hpp) on the
// CPU under ASan + UBSan: what sydelta_delta_batch_from_json_device and its kernels run -- the
// plan, the tail body per file, count / place / parse per file on the shared chunk table with
// the batch's ranks, the sizes, the literal arena -- on host memory with every array at its
// exact size, the files' stages in shuffled order, the text arena at byte offsets 0, 1 and 7
// with its pad bytes spelling digits and commas, the literal arena at phases 0, 1 and 3 inside
// a 0xA5 guard.
//
//   dparse_batch_check <dir> <seed>
//
// <dir>/manifest.txt lists "<name> ok|reject"; <name>.json holds the text
// (tests/test_dparse_batch_host.py writes them from tests/delta_json_cases.py).  The reference
// for every file is the parse of its text alone (parse_alone: the single call's steps, no
// batch code).
#include <sanitizer/asan_interface.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <fstream>
#include <iterator>
#include <numeric>
#include <random>
#include <string>
#include <vector>

#include "dparse_wave.hpp"
#include "sydelta_dparsebatch.hpp"

using namespace sydelta;

namespace {

typedef std::vector<uint8_t> Bytes;
int g_fails = 0;

#define CHECK(cond, ...)                            \
    do {                                            \
        if (!(cond)) {                              \
            printf("FAIL " __VA_ARGS__);            \
            printf("  [%s:%d]\n", #cond, __LINE__); \
            ++g_fails;                              \
        }                                           \
    } while (0)

template <class T>
struct Arr {  // exactly n elements (malloc: the sanitizer's red zones on both sides)
    T* p;
    size_t n;
    explicit Arr(size_t n_) : p((T*)malloc(n_ ? n_ * sizeof(T) : 1)), n(n_) {
        if (!n) ASAN_POISON_MEMORY_REGION(p, 1);
    }
    ~Arr() {
        ASAN_UNPOISON_MEMORY_REGION(p, 1);
        free(p);
    }
    Arr(const Arr&) = delete;
};

// n bytes whose address is k mod 16, the bytes before and behind them poisoned
struct Exact {
    uint8_t* block = nullptr;
    uint8_t* p = nullptr;
    size_t pad = 0, total = 0;
    Exact(size_t n, unsigned k) {
        pad = k ? k : 16;
        total = (pad + n + 15) / 16 * 16 + 16;
        block = (uint8_t*)aligned_alloc(16, total);
        p = block + pad;
        ASAN_POISON_MEMORY_REGION(block, pad);
        ASAN_POISON_MEMORY_REGION(p + n, total - pad - n);
    }
    ~Exact() {
        ASAN_UNPOISON_MEMORY_REGION(block, total);
        free(block);
    }
    Exact(const Exact&) = delete;
};

std::vector<uint64_t> shuffled(uint64_t n, std::mt19937_64& rng) {
    std::vector<uint64_t> v(n);
    std::iota(v.begin(), v.end(), 0);
    std::shuffle(v.begin(), v.end(), rng);
    return v;
}

void exclusive(const uint64_t* in, uint64_t* out, uint64_t n) {
    uint64_t s = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t v = in[i];
        out[i] = s;
        s += v;
    }
}

// ---- the reference: one text alone, the steps of sydelta_delta_from_json_device
struct Alone {
    uint64_t status = dpb::kNoBad;  // or the byte the single call names
    uint64_t n = 0, b = 0, nlit = 0;
    std::vector<sydelta_op> ops;
    Bytes lit;
};
Alone parse_alone(const Bytes& text) {
    Alone r;
    const uint64_t len = text.size();
    if (len < dpb::kMinText) return r.status = 0, r;
    Exact t(len, 0);
    memcpy(t.p, text.data(), len);
    const uint64_t tl = std::min<uint64_t>(len - dparse::kHead, dpb::kTailMax);
    uint8_t head[dparse::kHead], tail[dpb::kTailMax];
    memcpy(head, t.p, dparse::kHead);
    memcpy(tail, t.p + len - tl, tl);
    const dpb::Rec rec = dpb::tail_parse(head, tail, len, tl);
    if (rec.status != dpb::kNoBad) return r.status = rec.status, r;
    r.n = rec.n, r.b = rec.b;
    const dparse::DArgs a{t.p, rec.e, dpb::chunks_of(rec.e)};
    if (!a.nc) return r;
    Arr<uint64_t> ocnt(a.nc + 1), lcnt(a.nc + 1), orank(a.nc + 1), lrank(a.nc + 1);
    ocnt.p[a.nc] = lcnt.p[a.nc] = 0;
    dparse_wave::count(a, ocnt.p, lcnt.p);
    exclusive(ocnt.p, orank.p, a.nc + 1);
    exclusive(lcnt.p, lrank.p, a.nc + 1);
    const uint64_t nops = orank.p[a.nc];
    r.nlit = lrank.p[a.nc];
    if (!nops) return r.status = dparse::kHead, r;
    Arr<uint64_t> pos(nops);
    Arr<sydelta_op> ops(nops);
    Arr<uint8_t> lit(r.nlit);
    unsigned long long bad = dparse::kNoBad;
    dparse_wave::place(a, orank.p, pos.p);
    dparse_wave::parse(a, orank.p, lrank.p, pos.p, nops, ops.p, r.nlit ? lit.p : nullptr, &bad);
    // (a delta without literals: the single call may be handed a NULL buffer; checked only)
    r.status = bad;
    if (bad != dparse::kNoBad) return r;
    r.ops.assign(ops.p, ops.p + nops);
    r.lit.assign(lit.p, lit.p + r.nlit);
    return r;
}

// ---- the batch
struct Batch {
    std::vector<const Bytes*> texts;  // file f's text (a pointer may repeat: the same arena range)
};
struct Result {
    std::vector<uint64_t> status, n, b, lit_off, lit_len;
    std::vector<std::vector<sydelta_op>> ops;
    std::vector<Bytes> lit;
    uint64_t need = 0;
};

// Every (file, wave) with chunks is the tile of exactly one wave of the grid, and no other tile
// finds a file it does not belong to.
void check_tiles(const std::vector<dpb::File>& files, uint64_t ntiles, const char* what) {
    uint64_t seen = 0;
    for (uint64_t t = 0; t < ntiles; ++t) {
        const uint64_t f = dpb::file_of_tile(files.data(), files.size(), t);
        CHECK(f < files.size() && files[f].tbase <= t && t - files[f].tbase < dpb::tile_bound(files[f].len),
              "%s: tile %llu -> file %llu", what, (unsigned long long)t, (unsigned long long)f);
        ++seen;
    }
    uint64_t want = 0;
    for (const dpb::File& F : files) want += dpb::tile_bound(F.len);
    CHECK(seen == want, "%s: %llu tiles for %llu", what, (unsigned long long)seen, (unsigned long long)want);
}

// The stages of sydelta_delta_batch_from_json_device.  text_phase: the text arena's address mod
// 16; lit_phase: the literal arena's; odd: the texts packed back to back behind one poison byte
// each (odd offsets) instead of at multiples of 16.
Result run_batch(const Batch& B, unsigned text_phase, unsigned lit_phase, bool odd, std::mt19937_64& rng,
                 const char* what) {
    const uint64_t nf = B.texts.size();
    // the text arena: each distinct text once, pads spelling literals ("7,8,9,...")
    std::vector<uint64_t> toff(nf), tlen(nf);
    uint64_t arena_len = 0;
    std::vector<std::pair<const Bytes*, uint64_t>> placed;
    for (uint64_t f = 0; f < nf; ++f) {
        tlen[f] = B.texts[f]->size();
        auto it = std::find_if(placed.begin(), placed.end(), [&](auto& x) { return x.first == B.texts[f]; });
        if (it != placed.end()) {
            toff[f] = it->second;
            continue;
        }
        arena_len = odd ? arena_len + 1 : dpb::pad16(arena_len);
        toff[f] = arena_len;
        placed.push_back({B.texts[f], arena_len});
        arena_len += tlen[f];
    }
    Exact arena(arena_len, text_phase);
    static const char kPoison[] = "7,88,199,{1,2],";
    for (uint64_t i = 0; i < arena_len; ++i) arena.p[i] = (uint8_t)kPoison[i % (sizeof kPoison - 1)];
    for (auto& x : placed)
        if (!x.first->empty()) memcpy(arena.p + x.second, x.first->data(), x.first->size());

    Result R;
    R.status.assign(nf, 0), R.n.assign(nf, 0), R.b.assign(nf, 0), R.lit_off.assign(nf, 0), R.lit_len.assign(nf, 0);
    R.ops.resize(nf), R.lit.resize(nf);
    std::vector<dpb::File> files;
    uint64_t nchunks = 0, ntiles = 0;
    dpb::PlanErr err;
    const int rc = dpb::plan(true, arena_len, toff.data(), tlen.data(), nf, true, 0, R.lit_off.data(), R.lit_len.data(),
                             &files, &nchunks, &ntiles, &err);
    CHECK(rc == 0, "%s: plan: %s", what, err.msg.c_str());
    if (rc) return R;
    check_tiles(files, ntiles, what);

    // stage 1: the tail, a lane per file
    Arr<dpb::Rec> recs(nf);
    for (uint64_t f : shuffled(nf, rng)) recs.p[f] = dpb::tail_file(arena.p, files[f]);
    // stage 2: the counts on the shared chunk table (zeroed: a file's spare entries stay 0)
    const uint64_t nce = nchunks + 1;
    Arr<uint64_t> ocnt(nce), lcnt(nce), orank(nce), lrank(nce);
    memset(ocnt.p, 0, nce * 8);
    memset(lcnt.p, 0, nce * 8);
    for (uint64_t f : shuffled(nf, rng)) {
        const dparse::DArgs a = dpb::args_of(arena.p, files[f], recs.p[f], 0);
        CHECK(a.nc <= dpb::chunk_bound(files[f].len), "%s: file %llu has more chunks than its bound", what,
              (unsigned long long)f);
        if (a.nc) dparse_wave::count(a, ocnt.p + files[f].cbase, lcnt.p + files[f].cbase);
    }
    exclusive(ocnt.p, orank.p, nce);
    exclusive(lcnt.p, lrank.p, nce);
    // stage 3: the sizes, lit_off
    Arr<uint64_t> nops(nf), pad(nf);
    for (uint64_t f : shuffled(nf, rng)) {
        dpb::sizes_file(files[f], orank.p, lrank.p, recs.p[f], nops.p[f], R.lit_len[f]);
        pad.p[f] = dpb::pad16(R.lit_len[f]);
    }
    exclusive(pad.p, R.lit_off.data(), nf);
    R.need = R.lit_off[nf - 1] + R.lit_len[nf - 1];
    const uint64_t total_ops = std::accumulate(nops.p, nops.p + nf, (uint64_t)0);
    CHECK(total_ops == orank.p[nchunks], "%s: the op counts do not add up", what);

    // stages 4-5: place and parse, the literal arena inside a guard
    const uint64_t G = 64;
    Exact guard(R.need + 2 * G, (lit_phase + 16 - G % 16) % 16);
    memset(guard.p, 0xA5, R.need + 2 * G);
    uint8_t* const lit = guard.p + G;
    CHECK(((uintptr_t)lit & 15) == lit_phase, "%s: literal phase", what);
    Arr<uint64_t> pos(total_ops);
    Arr<sydelta_op> ops(total_ops);
    if (total_ops) {
        for (uint64_t f : shuffled(nf, rng)) {
            const dpb::File& F = files[f];
            const dparse::DArgs a = dpb::args_of(arena.p, F, recs.p[f], lrank.p[F.cbase]);
            if (a.nc) dparse_wave::place(a, orank.p + F.cbase, pos.p);
        }
        for (uint64_t f : shuffled(nf, rng)) {
            const dpb::File& F = files[f];
            const dparse::DArgs a = dpb::args_of(arena.p, F, recs.p[f], lrank.p[F.cbase]);
            if (!a.nc) continue;
            dparse_wave::parse(a, orank.p + F.cbase, lrank.p + F.cbase, pos.p, orank.p[F.cbase + a.nc], ops.p,
                               dpb::lit_base(lit, R.lit_off[f], lrank.p[F.cbase]),
                               (unsigned long long*)&recs.p[f].status);
        }
    }
    // back on the host
    uint64_t o0 = 0;
    for (uint64_t f = 0; f < nf; o0 += nops.p[f], ++f) {
        R.status[f] = recs.p[f].status == dpb::kNoBad ? 0 : 1 + recs.p[f].status;
        if (R.status[f]) continue;
        R.n[f] = recs.p[f].n, R.b[f] = recs.p[f].b;
        R.ops[f].assign(ops.p + o0, ops.p + o0 + nops.p[f]);
        R.lit[f].assign(lit + R.lit_off[f], lit + R.lit_off[f] + R.lit_len[f]);
    }
    // the packing rule; guards and pads intact
    uint64_t at = 0;
    for (uint64_t f = 0; f < nf; ++f) {
        CHECK(R.lit_off[f] == at, "%s: file %llu at %llu, the packing rule says %llu", what, (unsigned long long)f,
              (unsigned long long)R.lit_off[f], (unsigned long long)at);
        at += dpb::pad16(R.lit_len[f]);
    }
    std::vector<uint8_t> own(R.need + 2 * G, 0);
    for (uint64_t f = 0; f < nf; ++f) std::fill_n(own.begin() + G + R.lit_off[f], R.lit_len[f], 1);
    for (uint64_t i = 0; i < own.size(); ++i)
        if (!own[i] && guard.p[i] != 0xA5) {
            CHECK(false, "%s: byte %lld outside every file's literal range was written", what, (long long)i - (long long)G);
            break;
        }
    return R;
}

bool same_ops(const std::vector<sydelta_op>& x, const std::vector<sydelta_op>& y) {
    if (x.size() != y.size()) return false;
    for (size_t i = 0; i < x.size(); ++i)
        if (x[i].kind != y[i].kind || x[i].a != y[i].a || x[i].b != y[i].b) return false;
    return true;
}

void compare(const Batch& B, const Result& R, const std::vector<Alone>& alone, const std::vector<size_t>& which,
             const char* what) {
    for (size_t f = 0; f < B.texts.size(); ++f) {
        const Alone& A = alone[which[f]];
        const uint64_t want = A.status == dpb::kNoBad ? 0 : 1 + A.status;
        CHECK(R.status[f] == want, "%s: file %zu: status %llu, alone %llu", what, f, (unsigned long long)R.status[f],
              (unsigned long long)want);
        CHECK(R.lit_len[f] == A.nlit, "%s: file %zu: %llu literals, alone %llu", what, f, (unsigned long long)R.lit_len[f],
              (unsigned long long)A.nlit);
        if (want || R.status[f]) continue;
        CHECK(R.n[f] == A.n && R.b[f] == A.b, "%s: file %zu: source_size / block_size", what, f);
        CHECK(same_ops(R.ops[f], A.ops), "%s: file %zu: ops differ from the text's alone", what, f);
        CHECK(R.lit[f] == A.lit, "%s: file %zu: literal bytes differ from the text's alone", what, f);
    }
}

Bytes slurp(const std::string& path) {
    std::ifstream in(path, std::ios::binary);
    return Bytes(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) return fprintf(stderr, "usage: dparse_batch_check <dir> <seed>\n"), 2;
    const std::string dir = argv[1];
    std::mt19937_64 rng(strtoull(argv[2], nullptr, 10));
    std::vector<std::string> names;
    std::vector<Bytes> texts;
    std::vector<bool> ok;
    {
        std::ifstream man(dir + "/manifest.txt");
        std::string name, kind;
        while (man >> name >> kind) {
            names.push_back(name);
            texts.push_back(slurp(dir + "/" + name + ".json"));
            ok.push_back(kind == "ok");
        }
    }
    if (texts.empty()) return fprintf(stderr, "no corpus in %s\n", dir.c_str()), 2;
    std::vector<Alone> alone;
    for (size_t i = 0; i < texts.size(); ++i) {
        alone.push_back(parse_alone(texts[i]));
        CHECK((alone[i].status == dpb::kNoBad) == ok[i], "%s: alone: status %llu", names[i].c_str(),
              (unsigned long long)alone[i].status);
    }
    auto find = [&](const char* n) {
        const size_t i = std::find(names.begin(), names.end(), n) - names.begin();
        if (i == names.size()) fprintf(stderr, "no %s in the corpus\n", n), exit(2);
        return i;
    };
    auto run = [&](const std::vector<size_t>& which, unsigned tp, unsigned lp, bool odd, const char* what) {
        Batch B;
        for (size_t i : which) B.texts.push_back(&texts[i]);
        const Result R = run_batch(B, tp, lp, odd, rng, what);
        compare(B, R, alone, which, what);
        return R;
    };
    std::vector<size_t> good, bad;
    for (size_t i = 0; i < texts.size(); ++i) (ok[i] ? good : bad).push_back(i);

    // 1. every accepted text in one batch: forward, reversed, shuffled; text arena at 0, 1, 7;
    // literal arena at phases 0, 1, 3; at multiples of 16 and at odd offsets; one text twice
    unsigned runs = 0;
    for (int order = 0; order < 3; ++order) {
        std::vector<size_t> which = good;
        if (order == 1) std::reverse(which.begin(), which.end());
        if (order == 2) std::shuffle(which.begin(), which.end(), rng);
        which.push_back(which[1]);  // a repeated text: the same arena range
        static const unsigned tps[] = {0, 1, 7}, lps[] = {0, 1, 3};
        for (int k = 0; k < 3; ++k) {
            char what[64];
            snprintf(what, sizeof what, "all order %d text+%u lit+%u", order, tps[k], lps[(k + order) % 3]);
            run(which, tps[k], lps[(k + order) % 3], (k + order) & 1, what);
            ++runs;
        }
    }
    printf("all: %zu texts, %u runs\n", good.size(), runs);

    // 2. every refused text between two good files
    const size_t g0 = find("acc-3"), g1 = find("acc-4");
    for (size_t i : bad) {
        char what[96];
        snprintf(what, sizeof what, "reject %s", names[i].c_str());
        const Result R = run({g0, i, g1}, 1, 3, true, what);
        printf("reject %s: %s\n", names[i].c_str(), dpb::refusal_message(1, R.status[1] - 1).c_str());
    }

    // 3. a file ending in a Data op directly before one starting with a Data op; empty-ops texts
    // first, last and adjacent
    const size_t td = find("tail-data"), hd = find("head-data"), em = find("acc-0"), dn = find("dense");
    run({td, hd}, 0, 0, true, "data-data");
    run({td, hd, td, hd}, 7, 1, true, "data-data twice");
    run({em, td, em, em, dn, hd, em}, 0, 1, false, "empties");
    run({em}, 0, 0, false, "one empty");
    run({em, em, em}, 1, 3, true, "only empties");

    if (g_fails) return printf("dparse_batch_check: %d failures\n", g_fails), 1;
    printf("dparse_batch_check ok\n");
    return 0;
}
