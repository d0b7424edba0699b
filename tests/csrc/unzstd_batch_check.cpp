// unzstd_batch_check.cpp — the batched zstd decoder (sy_amd/csrc/sydelta_unzstdbatch.hpp over
// the stage bodies of sydelta_unzstd.hpp) on the CPU under ASan + UBSan: what
// sydelta_zstd_decompress_batch_device and its kernels run, thread by thread in shuffled
// orders, on host memory with every array at its exact size, the frame arena at its exact
// size and at byte offsets 0, 1 and 7, the text arena inside a guard buffer with its pad
// bytes poisoned while the stages run.
//
//   unzstd_batch_check <dir> <mutants per frame> <seed>
//
// <dir>/manifest.txt lists "<name> ok|valid|reject"; <name>.frame, and unless reject <name>.out
// (the corpus directory of tests/test_unzstd_host.py).  The reference for every file is the
// decode of its frame alone (decode_alone: the single decoder's bodies, no batch code).
#include <sanitizer/asan_interface.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <fstream>
#include <iterator>
#include <map>
#include <numeric>
#include <random>
#include <string>
#include <vector>

#include "sydelta_unzstdbatch.hpp"

using namespace sydelta;
using namespace sydelta::unzb;

namespace {

typedef std::vector<uint8_t> Bytes;
int g_fails = 0;

#define CHECK(cond, ...)                          \
    do {                                          \
        if (!(cond)) {                            \
            printf("FAIL " __VA_ARGS__);          \
            printf("  [%s:%d]\n", #cond, __LINE__); \
            ++g_fails;                            \
        }                                         \
    } while (0)

template <class T>
struct Arr {  // exactly n elements (malloc: the sanitizer's red zones on both sides)
    T* p;
    explicit Arr(size_t n) : p((T*)malloc(n ? n * sizeof(T) : 1)) {
        if (!n) ASAN_POISON_MEMORY_REGION(p, 1);
    }
    ~Arr() {
        ASAN_UNPOISON_MEMORY_REGION(p, 1);
        free(p);
    }
    Arr(const Arr&) = delete;
};

// n bytes whose address is k mod 16, the bytes before them poisoned, the heap's red zone behind
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

struct Perm {  // i -> a permutation of [0, n)
    uint64_t n, mul, add;
    Perm(uint64_t n_, std::mt19937_64& rng) : n(n_) {
        static const uint64_t primes[] = {1000003, 7919, 104729, 15485863, 2147483647};
        mul = 1;
        for (uint64_t q : primes)
            if (n % q) {
                mul = q % n ? q % n : 1;
                break;
            }
        if (n && std::gcd(mul, n) != 1) mul = 1;
        add = n ? rng() % n : 0;
    }
    uint64_t at(uint64_t j) const { return (uint64_t)(((unsigned __int128)j * mul + add) % n); }
};

void lds_tables(const Block& k, const HufTab* huf, const FseTab* fse, std::vector<uint16_t>& s_huf,
                std::vector<uint32_t> s_fse[3], uint32_t& hlog, uint32_t flog[3]) {
    hlog = 0, flog[0] = flog[1] = flog[2] = 0;
    s_huf.clear();
    if (k.lit_type >= 2) {
        hlog = huf[k.huf_slot].log;
        s_huf.assign(huf[k.huf_slot].e, huf[k.huf_slot].e + ((size_t)1 << hlog));
        s_huf.shrink_to_fit();
    }
    for (int j = 0; j < 3; ++j) {
        s_fse[j].clear();
        if (!k.nseq) continue;
        const FseTab& T = fse[k.fse_slot[j]];
        flog[j] = T.log;
        s_fse[j].assign(T.e, T.e + ((size_t)1 << T.log));
        s_fse[j].shrink_to_fit();
    }
}

// The reference: one frame alone, the single decoder's stages in their plain order.
uint64_t decode_alone(const Bytes& frame, Bytes& result, bool size_only = false, uint64_t* out_len = nullptr) {
    result.clear();
    Exact in(frame.size(), 3);
    if (!frame.empty()) memcpy(in.p, frame.data(), frame.size());
    Totals t;
    uint64_t st = scan(in.p, frame.size(), nullptr, 0, t);
    if (st != kNoErr) return st;
    const Totals c = t;
    Arr<Block> blocks(c.nb);
    if ((st = scan(in.p, frame.size(), blocks.p, c.nb, t)) != kNoErr) return st;
    Arr<HufTab> huf(c.nhuf);
    Arr<FseTab> fse(c.nfse);
    Arr<uint8_t> lits(c.nlit);
    Arr<Seq> seqs(c.nseq);
    Arr<Hist> hexit(c.nb);
    Arr<uint32_t> entry(3 * c.nb);
    Arr<uint64_t> bpos(c.nb + 1);
    uint64_t status = kNoErr;
    auto report = [&](uint64_t b, uint32_t e) {
        if (e) status = std::min(status, ekey(b, e));
    };
    for (uint64_t b = 0; b < c.nb; ++b) report(b, build_tables(in.p, blocks.p[b], huf.p, fse.p));
    if (status != kNoErr) return status;
    for (uint64_t b = 0; b < c.nb; ++b) {
        Block& k = blocks.p[b];
        if (k.type != 2) continue;
        std::vector<uint16_t> s_huf;
        std::vector<uint32_t> s_fse[3];
        uint32_t hlog, flog[3];
        lds_tables(k, huf.p, fse.p, s_huf, s_fse, hlog, flog);
        for (uint32_t tid = 0; tid < 64; ++tid) {
            if (k.lit_type < 2) lit_fill(in.p, k, lits.p, tid, 64);
            else if (tid < k.lit_streams) report(b, lit_stream(in.p, k, s_huf.data(), hlog, tid, lits.p));
        }
        report(b, seq_decode(in.p, k, s_fse[0].data(), flog[0], s_fse[1].data(), flog[1], s_fse[2].data(), flog[2],
                             seqs.p + k.seq_base, hexit.p[b]));
    }
    if (status != kNoErr) return status;
    if ((st = stitch(blocks.p, c.nb, hexit.p, entry.p, bpos.p, t)) != kNoErr) return st;
    for (uint64_t b = 0; b < c.nb; ++b) {
        const Block& k = blocks.p[b];
        if (k.type != 2) continue;
        for (uint32_t i = 0; i < k.nseq; ++i) report(b, resolve(bpos.p[b], entry.p + 3 * b, seqs.p[k.seq_base + i]));
    }
    if (status != kNoErr) return status;
    const uint64_t n = t.out_len;
    if (out_len) *out_len = n;
    if (size_only) return kNoErr;
    Arr<uint8_t> out(n);
    Arr<uint32_t> parent(n);
    for (uint64_t i = 0; i < n; ++i) place(i, in.p, blocks.p, c.nb, bpos.p, seqs.p, lits.p, out.p, parent.p);
    for (uint32_t r = 0; r < kUnzRounds; ++r) {
        bool any = false;
        for (uint64_t i = 0; i < n; ++i) any |= jump(i, parent.p);
        if (!any) break;
    }
    for (uint64_t i = 0; i < n; ++i) gather(i, parent.p, out.p);
    result.assign(out.p, out.p + n);
    return kNoErr;
}

struct Result {
    int rc = SYDELTA_OK;
    std::string msg;
    std::vector<uint64_t> toff, tlen, status;
    uint64_t need = 0;
    bool sized_scratch = false;  // the shared scratch was allocated
};

// sydelta_zstd_decompress_batch_device on host memory.  d_out: out_cap bytes (or NULL).
Result decode_batch(const uint8_t* d_in, uint64_t in_len, const std::vector<uint64_t>& foff,
                    const std::vector<uint64_t>& flen, uint8_t* d_out, uint64_t out_cap, bool want_status,
                    std::mt19937_64& rng) {
    Result R;
    const uint64_t nfiles = foff.size();
    R.toff.assign(nfiles, 77), R.tlen.assign(nfiles, 77), R.status.assign(nfiles, 77);
    if (!nfiles) return R;
    std::vector<File> files_h;
    PlanErr err;
    if (plan(d_in != nullptr, in_len, foff.data(), flen.data(), nfiles, d_out != nullptr, out_cap, R.toff.data(),
             R.tlen.data(), &files_h, &err)) {
        R.rc = err.code, R.msg = err.msg;
        return R;
    }
    Arr<File> files(nfiles);
    std::copy(files_h.begin(), files_h.end(), files.p);
    Arr<Totals> tot(nfiles);
    Arr<uint64_t> status(nfiles);
    // k_unzb_count
    for (uint64_t f : shuffled(nfiles, rng)) count_file(d_in, files.p[f], tot.p[f], status.p[f]);
    std::vector<Base> bases_h;
    Base c;
    if (bases(tot.p, nfiles, &bases_h, &c, &err)) {
        R.rc = err.code, R.msg = err.msg;
        return R;
    }
    R.sized_scratch = true;
    Arr<Base> bs(nfiles);
    std::copy(bases_h.begin(), bases_h.end(), bs.p);
    Arr<Block> blocks(c.nb);
    Arr<uint32_t> bfile(c.nb);
    Arr<HufTab> huf(c.nhuf);
    Arr<FseTab> fse(c.nfse);
    Arr<uint8_t> lits(c.nlit);
    Arr<Seq> seqs(c.nseq);
    Arr<Hist> hexit(c.nb);
    Arr<uint32_t> entry(3 * c.nb);
    Arr<uint64_t> bpos(c.nb + nfiles);
    Arr<uint64_t> apos(c.nb);
    Arr<uint64_t> toff(nfiles), tlen(nfiles), pad(nfiles);
    auto report = [&](uint32_t f, uint64_t b, uint32_t e) {
        if (e) status.p[f] = std::min(status.p[f], ekey(b, e));
    };
    // k_unzb_scan
    for (uint64_t f : shuffled(nfiles, rng)) {
        if (status.p[f] != kNoErr) continue;
        const uint64_t st = scan_file(d_in, files.p[f], bs.p[f], tot.p[f], (uint32_t)f, blocks.p, bfile.p);
        if (st != kNoErr) status.p[f] = std::min(status.p[f], st);
    }
    const std::vector<uint64_t> order = shuffled(c.nb, rng);
    // Within a launch every workgroup reads its file's status as the launch found it (the
    // schedule in which all of them start before any reports): the lowest key then wins as in
    // the reference, whatever the order.
    std::vector<uint64_t> at_launch(status.p, status.p + nfiles);
    // k_unzb_tables
    for (uint64_t b : order) {
        const uint32_t f = bfile.p[b];
        if (at_launch[f] != kNoErr) continue;
        adopt(blocks.p[b], bs.p[f]);
        report(f, b - bs.p[f].nb, build_tables(frame_of(d_in, files.p[f]), blocks.p[b], huf.p, fse.p));
    }
    // k_unzb_decode (a file's status is read once per workgroup, before its work)
    at_launch.assign(status.p, status.p + nfiles);
    for (uint64_t b : order) {
        const uint32_t f = bfile.p[b];
        if (at_launch[f] != kNoErr) continue;
        Block& k = blocks.p[b];
        if (k.type != 2) continue;
        const uint8_t* in = frame_of(d_in, files.p[f]);
        const uint64_t rb = b - bs.p[f].nb;
        std::vector<uint16_t> s_huf;
        std::vector<uint32_t> s_fse[3];
        uint32_t hlog, flog[3];
        lds_tables(k, huf.p, fse.p, s_huf, s_fse, hlog, flog);
        const bool seq_first = rng() & 1;
        uint32_t e_seq = 0;
        auto run_seq = [&] {
            e_seq = seq_decode(in, k, s_fse[0].data(), flog[0], s_fse[1].data(), flog[1], s_fse[2].data(), flog[2],
                               seqs.p + k.seq_base, hexit.p[b]);
        };
        if (seq_first) run_seq();
        uint32_t e_lit[64] = {};
        for (uint64_t tid : shuffled(64, rng)) {
            if (k.lit_type < 2) lit_fill(in, k, lits.p, (uint32_t)tid, 64);
            else if (tid < k.lit_streams) e_lit[tid] = lit_stream(in, k, s_huf.data(), hlog, (uint32_t)tid, lits.p);
        }
        if (!seq_first) run_seq();
        for (uint32_t e : e_lit) report(f, rb, e);
        report(f, rb, e_seq);
    }
    // k_unzb_stitch
    for (uint64_t f : shuffled(nfiles, rng)) {
        if (status.p[f] != kNoErr) continue;
        const uint64_t st = stitch_file(blocks.p, hexit.p, entry.p, bpos.p, bs.p[f], f, tot.p[f]);
        if (st != kNoErr) status.p[f] = std::min(status.p[f], st);
    }
    // k_unzb_resolve
    at_launch.assign(status.p, status.p + nfiles);
    for (uint64_t b : order) {
        const uint32_t f = bfile.p[b];
        if (at_launch[f] != kNoErr) continue;
        const Block& k = blocks.p[b];
        if (k.type != 2) continue;
        uint32_t bad = 0;
        for (uint64_t i : shuffled(k.nseq, rng))
            if (const uint32_t e = resolve_in_text(bpos.p[b + f], f, entry.p + 3 * b, seqs.p[k.seq_base + i])) bad = e;
        report(f, b - bs.p[f].nb, bad);
    }
    // k_unzb_sizes, the exclusive sum, k_unzb_arena
    for (uint64_t f = 0; f < nfiles; ++f) tlen.p[f] = text_len_of(tot.p[f], status.p[f]), pad.p[f] = pad16(tlen.p[f]);
    uint64_t run = 0;
    for (uint64_t f = 0; f < nfiles; ++f) toff.p[f] = run, run += pad.p[f];
    const uint64_t need = toff.p[nfiles - 1] + tlen.p[nfiles - 1];
    for (uint64_t b : order) apos.p[b] = arena_pos(b, bfile.p, bpos.p, toff.p, status.p);
    if (finish(toff.p, tlen.p, status.p, need, nfiles, R.toff.data(), R.tlen.data(), want_status ? R.status.data() : nullptr,
               &R.need, &err)) {
        R.rc = err.code, R.msg = err.msg;
        return R;
    }
    const uint64_t n = R.need;
    if (!d_out || out_cap < n || !n) return R;
    Arr<uint32_t> parent(n);
    const Perm pm(n, rng);
    for (uint64_t j = 0; j < n; ++j)
        place_at(pm.at(j), d_in, files.p, bfile.p, blocks.p, c.nb, apos.p, seqs.p, lits.p, d_out, parent.p);
    for (uint32_t r = 0; r < kUnzRounds; ++r) {
        bool any = false;
        for (uint64_t j = 0; j < n; ++j) any |= jump(pm.at(j), parent.p);
        if (!any) break;
        if (r + 1 == kUnzRounds) {
            fprintf(stderr, "pointer doubling did not settle\n");
            exit(3);
        }
    }
    for (uint64_t j = 0; j < n; ++j) gather(pm.at(j), parent.p, d_out);
    return R;
}

Bytes slurp(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) {
        fprintf(stderr, "cannot read %s\n", path.c_str());
        exit(2);
    }
    return Bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

struct Item {
    std::string name;
    Bytes frame;
    uint64_t st = kNoErr;  // of the frame alone
    Bytes text;            // of the frame alone
};

Item alone(const std::string& name, const Bytes& frame) {
    Item it;
    it.name = name, it.frame = frame;
    it.st = decode_alone(frame, it.text);
    return it;
}

constexpr unsigned kGuard = 64;

// The batch `items` through both forms of the call: the size query, then the decode into a
// guard buffer (0xA5 everywhere; the pads and guards poisoned when out_align is 0).  With
// want_status the refused files are reported per file; without, a batch with a refused file is
// an error that writes nothing.  Every file against its frame alone.
void run_batch(const char* what, const std::vector<const Item*>& items, unsigned in_off, unsigned out_align,
               bool want_status, std::mt19937_64& rng) {
    const uint64_t n = items.size();
    std::vector<uint64_t> foff(n), flen(n);
    uint64_t total = 0;
    for (uint64_t f = 0; f < n; ++f) foff[f] = total, flen[f] = items[f]->frame.size(), total += flen[f];
    Exact in(total, in_off);
    for (uint64_t f = 0; f < n; ++f)
        if (flen[f]) memcpy(in.p + foff[f], items[f]->frame.data(), flen[f]);
    // what the contract promises
    std::vector<uint64_t> want_off(n), want_len(n);
    uint64_t run = 0, first_bad = n;
    for (uint64_t f = 0; f < n; ++f) {
        const bool ok = items[f]->st == kNoErr;
        if (!ok && first_bad == n) first_bad = f;
        want_len[f] = ok ? items[f]->text.size() : 0;
        want_off[f] = run;
        run += pad16(want_len[f]);
    }
    const uint64_t want_need = n ? want_off[n - 1] + want_len[n - 1] : 0;

    const Result Q = decode_batch(in.p, total, foff, flen, nullptr, 0, want_status, rng);
    if (!want_status && first_bad < n) {
        const std::string msg = frame_message(first_bad, items[first_bad]->st);
        CHECK(Q.rc == SYDELTA_E_INVAL && Q.msg == msg, "%s: size query: rc %d \"%s\", want \"%s\"\n", what, Q.rc,
              Q.msg.c_str(), msg.c_str());
        // nothing may be written: the whole arena is poisoned
        Exact out(want_need + kGuard, 0);
        ASAN_POISON_MEMORY_REGION(out.p, want_need + kGuard);
        const Result W = decode_batch(in.p, total, foff, flen, out.p, want_need + kGuard, false, rng);
        CHECK(W.rc == SYDELTA_E_INVAL && W.msg == msg, "%s: rc %d \"%s\"\n", what, W.rc, W.msg.c_str());
        ASAN_UNPOISON_MEMORY_REGION(out.p, want_need + kGuard);
        return;
    }
    CHECK(Q.rc == SYDELTA_OK, "%s: size query: rc %d %s\n", what, Q.rc, Q.msg.c_str());
    CHECK(Q.need == want_need && Q.toff == want_off && Q.tlen == want_len, "%s: size query: need %llu for %llu\n", what,
          (unsigned long long)Q.need, (unsigned long long)want_need);
    if (g_fails) return;

    const uint64_t cap = want_need + kGuard;
    Exact out(cap, out_align);
    memset(out.p, 0xA5, cap);
    if (out_align == 0) {
        for (uint64_t f = 0; f + 1 < n; ++f)
            ASAN_POISON_MEMORY_REGION(out.p + want_off[f] + want_len[f], want_off[f + 1] - want_off[f] - want_len[f]);
        ASAN_POISON_MEMORY_REGION(out.p + (want_need + 7) / 8 * 8, cap - (want_need + 7) / 8 * 8);
    }
    // one byte short: nothing written, the same sizes
    if (want_need) {
        const Result S = decode_batch(in.p, total, foff, flen, out.p, want_need - 1, want_status, rng);
        CHECK(S.rc == SYDELTA_OK && S.need == want_need && S.toff == want_off && S.tlen == want_len, "%s: short arena\n", what);
        ASAN_UNPOISON_MEMORY_REGION(out.p, cap);
        for (uint64_t i = 0; i < cap; ++i)
            if (out.p[i] != 0xA5) {
                CHECK(false, "%s: short arena: byte %llu written\n", what, (unsigned long long)i);
                break;
            }
        if (out_align == 0) {
            for (uint64_t f = 0; f + 1 < n; ++f)
                ASAN_POISON_MEMORY_REGION(out.p + want_off[f] + want_len[f], want_off[f + 1] - want_off[f] - want_len[f]);
            ASAN_POISON_MEMORY_REGION(out.p + (want_need + 7) / 8 * 8, cap - (want_need + 7) / 8 * 8);
        }
    }
    const Result W = decode_batch(in.p, total, foff, flen, out.p, cap, want_status, rng);
    ASAN_UNPOISON_MEMORY_REGION(out.p, cap);
    CHECK(W.rc == SYDELTA_OK, "%s: rc %d %s\n", what, W.rc, W.msg.c_str());
    CHECK(W.need == want_need && W.toff == want_off && W.tlen == want_len, "%s: tables\n", what);
    if (g_fails) return;
    std::vector<uint8_t> is_text(cap, 0);
    for (uint64_t f = 0; f < n; ++f) {
        if (want_status) {
            const uint64_t ws = items[f]->st == kNoErr ? 0 : items[f]->st;
            CHECK(W.status[f] == ws, "%s: file %llu (%s): status %llx for %llx\n", what, (unsigned long long)f,
                  items[f]->name.c_str(), (unsigned long long)W.status[f], (unsigned long long)ws);
        }
        if (!want_len[f]) continue;
        std::fill(is_text.begin() + want_off[f], is_text.begin() + want_off[f] + want_len[f], 1);
        if (memcmp(out.p + want_off[f], items[f]->text.data(), want_len[f])) {
            uint64_t d = 0;
            while (out.p[want_off[f] + d] == items[f]->text[d]) ++d;
            CHECK(false, "%s: file %llu (%s): first difference at %llu of %llu\n", what, (unsigned long long)f,
                  items[f]->name.c_str(), (unsigned long long)d, (unsigned long long)want_len[f]);
        }
    }
    for (uint64_t i = 0; i < cap; ++i)
        if (!is_text[i] && out.p[i] != 0xA5) {
            CHECK(false, "%s: byte %llu outside the texts was written\n", what, (unsigned long long)i);
            break;
        }
}

// A frame of `nblocks` RLE blocks of 128 KiB each.
Bytes rle_frame(uint32_t nblocks) {
    Bytes f = {0x28, 0xB5, 0x2F, 0xFD, 0x00, 0x38};
    for (uint32_t b = 0; b < nblocks; ++b) {
        const uint32_t h = kBlockMax << 3 | 1 << 1 | (b + 1 == nblocks);
        f.push_back((uint8_t)h), f.push_back((uint8_t)(h >> 8)), f.push_back((uint8_t)(h >> 16)), f.push_back(0x55);
    }
    return f;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    const std::string dir = argv[1];
    const int nmut = atoi(argv[2]);
    std::mt19937_64 rng(strtoull(argv[3], nullptr, 10));
    std::ifstream man(dir + "/manifest.txt");
    std::string name, kind;
    std::vector<Item> good, bad;
    std::map<std::string, size_t> bad_at;
    while (man >> name >> kind) {
        Item it = alone(name, slurp(dir + "/" + name + ".frame"));
        if (kind == "reject") {
            CHECK(it.st != kNoErr, "%s: accepted alone\n", name.c_str());
            bad_at[name] = bad.size();
            bad.push_back(std::move(it));
        } else {
            CHECK(it.st == kNoErr && it.text == slurp(dir + "/" + name + ".out"), "%s: alone\n", name.c_str());
            good.push_back(std::move(it));
        }
    }
    if (g_fails || good.size() < 8 || bad.empty()) {
        printf("unzstd_batch_check: the corpus does not decode alone\n");
        return 1;
    }
    auto find_good = [&](const char* nm) -> const Item* {
        for (const Item& it : good)
            if (it.name == nm) return &it;
        fprintf(stderr, "no frame %s in the corpus\n", nm);
        exit(2);
    };
    const Item* small = find_good("json-small-s1");
    const Item* empty = find_good("empty-s3");
    const Item* one = find_good("one-s3");
    const Item* two = find_good("hand-two-blocks");
    int batches = 0;

    // 1. the whole corpus in one batch: file order, reversed, shuffled; the frame arena at 0, 1, 7
    {
        std::vector<const Item*> all;
        for (const Item& it : good) all.push_back(&it);
        std::vector<const Item*> orders[3] = {all, all, all};
        std::reverse(orders[1].begin(), orders[1].end());
        std::shuffle(orders[2].begin(), orders[2].end(), rng);
        const unsigned offs[3] = {0, 1, 7};
        // every order and every offset, five of the nine pairs (a pass over the 22 MB of text
        // takes the better part of a minute under the sanitizers)
        const int pairs[5][2] = {{0, 0}, {1, 1}, {2, 2}, {0, 1}, {0, 2}};
        for (const auto& pr : pairs) {
            const int o = pr[0], k = pr[1];
            char what[64];
            snprintf(what, sizeof what, "corpus order %d, frames at %u", o, offs[k]);
            // the text arena aligned with its pads poisoned, or at an odd address
            run_batch(what, orders[o], offs[k], k == o ? 0 : (unsigned)(1 + 2 * o + k), true, rng);
            ++batches;
        }
    }

    // 2. every malformed frame in the middle of three good frames
    for (const Item& b : bad) {
        const std::vector<const Item*> files = {small, &b, two, one};
        run_batch(("malformed " + b.name).c_str(), files, 1, 0, true, rng);
        run_batch(("malformed " + b.name + ", no status table").c_str(), files, 1, 0, false, rng);
        printf("reject %s: %s\n", b.name.c_str(), frame_message(1, b.st).c_str());
        batches += 2;
    }

    // 3. no table, repeat offset or match from the file before
    {
        const Item* with_huf = nullptr;
        const Item* with_fse = nullptr;
        for (const Item& it : good) {
            Totals t;
            if (scan(it.frame.data(), it.frame.size(), nullptr, 0, t) != kNoErr) continue;
            // the last block defines the tables a first block of the next file would find
            if (t.nhuf && !with_huf && it.name.find("json-literals") == 0) with_huf = &it;
            if (t.nfse && !with_fse && it.name.find("json-copies") == 0) with_fse = &it;
        }
        CHECK(with_huf && with_fse, "no frame with tables in the corpus\n");
        if (with_huf && with_fse) {
            const Item* treeless = &bad[bad_at.at("first-block-treeless")];
            const Item* repeat = &bad[bad_at.at("first-block-repeat-mode")];
            const Item* ll0 = &bad[bad_at.at("ll0-offset-before-start")];
            run_batch("treeless behind a Huffman table", {with_huf, treeless, small}, 0, 0, true, rng);
            run_batch("repeat mode behind FSE tables", {with_fse, repeat, small}, 7, 0, true, rng);
            run_batch("offset before the start behind a text", {two, ll0, small}, 0, 0, true, rng);
            run_batch("offset before the start behind a text, no status table", {two, ll0, small}, 0, 0, false, rng);
            batches += 4;
        }
    }

    // 4. empty texts first, last and adjacent; 1, 64, 65 and 200 files
    run_batch("empty texts", {empty, empty, small, empty, empty, one, empty}, 1, 0, true, rng);
    run_batch("only empty texts", {empty, empty, empty}, 0, 0, true, rng);
    ++batches, ++batches;
    for (unsigned n : {1u, 64u, 65u, 200u}) {
        const Item* cyc[5] = {small, one, empty, two, &bad[0]};
        std::vector<const Item*> files;
        for (unsigned f = 0; f < n; ++f) files.push_back(cyc[n == 1 ? 0 : (f * 7 + f / 5) % 5]);
        char what[32];
        snprintf(what, sizeof what, "%u files", n);
        run_batch(what, files, 7, n % 2 ? 5 : 0, true, rng);
        ++batches;
    }

    // 5. the 4 GiB arena limit, as a size query: 2 GiB regenerated from 64 KiB of frame
    {
        Item big;
        big.name = "rle-2GiB", big.frame = rle_frame(16384);
        uint64_t len = 0;
        big.st = decode_alone(big.frame, big.text, true, &len);
        CHECK(big.st == kNoErr && len == 2ull << 30, "rle-2GiB alone: %llu bytes\n", (unsigned long long)len);
        Exact in(2 * big.frame.size(), 1);
        memcpy(in.p, big.frame.data(), big.frame.size());
        memcpy(in.p + big.frame.size(), big.frame.data(), big.frame.size());
        const uint64_t L = big.frame.size();
        Result A = decode_batch(in.p, 2 * L, {L}, {L}, nullptr, 0, true, rng);
        CHECK(A.rc == SYDELTA_OK && A.need == 2ull << 30 && A.tlen[0] == 2ull << 30 && A.status[0] == 0, "rle-2GiB in a batch of one\n");
        Result B = decode_batch(in.p, 2 * L, {0, L}, {L, L}, nullptr, 0, true, rng);
        CHECK(B.rc == SYDELTA_E_INVAL && !B.sized_scratch && B.msg.find("the batch regenerates") == 0 &&
                  B.msg.find("split it below 4 GiB") != std::string::npos && B.msg.find("file") == std::string::npos,
              "two of rle-2GiB: rc %d \"%s\"\n", B.rc, B.msg.c_str());
        printf("limit: %s\n", B.msg.c_str());
        batches += 2;
    }

    // 6. the host refusals
    {
        uint8_t byte = 0;
        const uint64_t big = ~0ull;
        struct {
            const uint8_t* in;
            uint64_t in_len;
            std::vector<uint64_t> off, len;
            uint8_t* out;
            uint64_t out_cap;
        } cases[] = {{&byte, 100, {0, 16, 96}, {10, 10, 5}, nullptr, 0},
                     {&byte, 100, {0, big - 15}, {10, 32}, nullptr, 0},
                     {&byte, 100, {0, 16}, {10, big}, nullptr, 0},
                     {nullptr, 100, {0, 16}, {0, 4}, nullptr, 0},
                     {&byte, 100, {0}, {10}, nullptr, 64}};
        for (auto& c : cases) {
            const Result r = decode_batch(c.in, c.in_len, c.off, c.len, c.out, c.out_cap, true, rng);
            CHECK(r.rc == SYDELTA_E_INVAL && !r.sized_scratch, "a bad table entry was accepted\n");
            printf("refuse %s\n", r.msg.c_str());
        }
    }

    // 7. seeded mutants between two good frames: a file's result in the batch is its result alone
    uint64_t mutants = 0, refused = 0;
    for (const Item& it : good) {
        for (int m = 0; m < nmut && !it.frame.empty(); ++m) {
            Bytes f = it.frame;
            if (rng() % 8 == 0) {
                f.resize(f.size() > 1 ? 1 + rng() % (f.size() - 1) : 1);
            } else {
                const int flips = 1 + (int)(rng() % 3);
                for (int i = 0; i < flips; ++i)
                    f[(rng() & 1) ? rng() % std::min<size_t>(f.size(), 64) : rng() % f.size()] ^= (uint8_t)(1u << (rng() % 8));
            }
            const Item mut = alone(it.name + " mutant", f);
            ++mutants, refused += mut.st != kNoErr;
            run_batch(mut.name.c_str(), {two, &mut, small}, (unsigned)(rng() % 16), (unsigned)(rng() % 16), true, rng);
            if (g_fails) break;
        }
        if (g_fails) break;
    }
    printf("batches: %d; mutants: %llu (%llu refused)\n", batches, (unsigned long long)mutants, (unsigned long long)refused);
    if (g_fails) {
        printf("unzstd_batch_check: %d failures\n", g_fails);
        return 1;
    }
    printf("unzstd_batch_check ok\n");
    return 0;
}
