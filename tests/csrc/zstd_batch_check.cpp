// zstd_batch_check.cpp — the batched zstd compressor's host plan and its shared bodies
// (sy_amd/csrc/sydelta_zstdbatch.hpp) on host memory, under ASan + UBSan.  A batch of texts is
// planned; every block of the batch is found by the bisection the kernels use and coded with
// zstd::block_content_seq (the sequential form of the device coder); the blocks then go through
// in rounds as the entry point queues them: placed lengths, an exclusive scan, a carried base,
// and the placement body run thread by thread through a memory policy that holds the input
// arena, the slots and the output arena at their exact sizes: a load outside the block's text
// or its slot, and a store outside the block's own place or at or past the arena's end, fail
// the run.  The arena must equal, byte for byte, the frames of tests/csrc/zstd_ref.cpp (linked
// in) built file by file and laid back to back, for rounds of 1, 3 and all blocks.  Then the
// too-small arena (a guard region behind it must stay intact), every refusal of the contract
// and the bound's overflow.
//
//   zstd_batch_check <random batches> <seed>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "sydelta_zstdbatch.hpp"

using namespace sydelta;
using namespace sydelta::zstdb;

extern "C" size_t zstd_ref_compress(const uint8_t* in, size_t len, uint8_t* out, size_t cap);

namespace {

uint64_t g_rng = 1;
uint64_t rnd() {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return g_rng;
}
uint64_t below(uint64_t n) { return n ? rnd() % n : 0; }

const char* g_batch = "";
[[noreturn]] void die(const char* what) {
    printf("FAIL %s: %s\n", g_batch, what);
    exit(1);
}

// Exactly `len` bytes, 16-byte aligned (len 0: one byte that nobody may touch).
struct Buf {
    uint8_t* p = nullptr;
    uint64_t len = 0;
    void make(uint64_t n, uint8_t fill) {
        void* q = nullptr;
        if (posix_memalign(&q, 16, n ? n : 1)) die("out of memory");
        p = (uint8_t*)q;
        len = n;
        memset(p, fill, n);
    }
    Buf() = default;
    Buf(const Buf&) = delete;
    ~Buf() { free(p); }
};

struct HostMem {
    uintptr_t s0 = 0, s1 = 0;  // what the block may read: its text, or its content in the slot
    uintptr_t d0 = 0, d1 = 0;  // where the block may write: its place, cut at the arena's end
    uint8_t ldb(uintptr_t p) const {
        if (p < s0 || p >= s1) die("load outside the block's source");
        return *(const uint8_t*)p;
    }
    void stb(uintptr_t p, uint8_t b) const {
        if (p < d0 || p >= d1) die("store outside the block's place or past the arena's end");
        *(uint8_t*)p = b;
    }
};

// Texts of the kinds the sender meets: Delta JSON heavy in Copy ops (literals + sequences),
// heavy in literal bytes (entropy-only), random bytes (Raw), one repeated byte (RLE).
enum Kind { kCopyJson, kDataJson, kRandom, kRle };
std::string make_text(Kind kind, uint64_t len) {
    std::string t;
    if (kind == kRle) return std::string(len, '7');
    if (kind == kRandom) {
        t.resize(len);
        for (uint64_t i = 0; i < len; ++i) t[i] = (char)rnd();
        return t;
    }
    t = "{\"ops\":[";
    uint64_t off = below(1 << 20);
    char buf[96];
    while (t.size() < len + 64) {
        if (kind == kCopyJson && below(8)) {
            snprintf(buf, sizeof buf, "{\"Copy\":{\"offset\":%llu,\"size\":4096}},", (unsigned long long)off);
            t += buf;
            off += 4096 * (1 + below(3));
        } else {
            t += "{\"Data\":[";
            for (uint64_t k = 0, n = 1 + below(kind == kDataJson ? 600 : 12); k < n; ++k) {
                snprintf(buf, sizeof buf, "%u,", (unsigned)below(256));
                t += buf;
            }
            t.back() = ']';
            t += "},";
        }
    }
    t.resize(len);  // cut anywhere: the coder takes any bytes
    return t;
}

struct Coded {
    uint32_t type = 0, size = 0;
    std::vector<uint8_t> slot;  // exactly `size` bytes of a Compressed block
};

// One batch: texts at multiples of 16 of an arena of exact size, through the plan, the coder and
// the rounds of each size in `rounds` (0: all blocks in one).
void run_batch(const std::vector<std::string>& texts, const std::vector<uint64_t>& rounds) {
    const uint64_t nfiles = texts.size();
    std::vector<uint64_t> toff(nfiles), tlen(nfiles);
    uint64_t in_len = 0;
    for (uint64_t f = 0; f < nfiles; ++f) {
        toff[f] = (in_len + 15) & ~(uint64_t)15;
        tlen[f] = texts[f].size();
        in_len = toff[f] + tlen[f];
    }
    Buf in;
    in.make(in_len, 0xEE);
    for (uint64_t f = 0; f < nfiles; ++f) memcpy(in.p + toff[f], texts[f].data(), tlen[f]);

    // the reference: the frames built file by file
    std::vector<uint8_t> want;
    std::vector<uint64_t> want_off(nfiles), want_len(nfiles);
    for (uint64_t f = 0; f < nfiles; ++f) {
        std::vector<uint8_t> fr(zstd::frame_bound(tlen[f]));
        const size_t n = zstd_ref_compress((const uint8_t*)texts[f].data(), tlen[f], fr.data(), fr.size());
        if (n < kFrameMin) die("reference frame");
        want_off[f] = want.size(), want_len[f] = n;
        want.insert(want.end(), fr.begin(), fr.begin() + n);
    }
    const uint64_t bound = batch_bound(tlen.data(), nfiles);
    if (bound == UINT64_MAX || bound < want.size()) die("the bound does not cover the frames");
    uint64_t sum = 0;
    for (uint64_t f = 0; f < nfiles; ++f) sum += zstd::frame_bound(tlen[f]);
    if (sum != bound) die("bound != sum of the frames' bounds");

    // the plan and every block's content
    std::vector<File> files;
    uint64_t nblocks = 0;
    Err err;
    if (plan((uintptr_t)in.p, in_len, toff.data(), tlen.data(), nfiles, &files, &nblocks, &err)) die(err.msg.c_str());
    if (files.size() != nfiles) die("file table size");
    std::vector<Coded> coded(nblocks);
    {
        std::vector<uint8_t> slot(zstd::kBlockMax), lz(zstd::kSeqScratchBytes);
        const zstd::SeqScratch sc = zstd::seq_scratch_at(lz.data(), 1, 0);
        uint64_t seen_file = UINT64_MAX;
        for (uint64_t b = 0; b < nblocks; ++b) {
            const Block B = block_at(files.data(), nfiles, b);
            if (B.file >= nfiles || B.at + B.n > in_len || B.text_len != tlen[B.file]) die("block lookup");
            if (B.first != (B.file != seen_file)) die("block lookup: first");
            if (B.last != (b + 1 == nblocks || block_at(files.data(), nfiles, b + 1).file != B.file)) die("block lookup: last");
            seen_file = B.file;
            Coded& C = coded[b];
            C.size = B.n ? zstd::block_content_seq(in.p + B.at, B.n, slot.data(), sc, &C.type) : 0;
            if (C.type == 2) C.slot.assign(slot.begin(), slot.begin() + C.size);
        }
    }

    // the rounds, into an arena of `cap` bytes with a guard behind it
    auto place_all = [&](uint64_t round, uint64_t cap, std::vector<uint64_t>* foff, Buf* out) -> uint64_t {
        constexpr uint64_t kGuard = 64;
        out->make(cap + kGuard, 0xA5);
        foff->assign(nfiles, UINT64_MAX);
        uint64_t base = 0;  // the device word: only ever advanced by a round's total
        for (uint64_t b0 = 0; b0 < nblocks; b0 += round) {
            const uint64_t nb = round < nblocks - b0 ? round : nblocks - b0;
            std::vector<uint64_t> len64(nb), off(nb);
            for (uint64_t i = 0; i < nb; ++i)
                len64[i] = placed_len(block_at(files.data(), nfiles, b0 + i).first, coded[b0 + i].size);
            uint64_t run = 0;
            for (uint64_t i = 0; i < nb; ++i) off[i] = run, run += len64[i];  // the exclusive scan
            for (uint64_t i = 0; i < nb; ++i) {
                const Block B = block_at(files.data(), nfiles, b0 + i);
                const Coded& C = coded[b0 + i];
                const uint64_t o = base + off[i];
                if (B.first) (*foff)[B.file] = o;
                HostMem m;
                m.s0 = C.type == 2 ? (uintptr_t)C.slot.data() : (uintptr_t)in.p + B.at;
                m.s1 = m.s0 + (C.type == 2 ? C.size : B.n);
                m.d0 = (uintptr_t)out->p + (o < cap ? o : cap);
                m.d1 = (uintptr_t)out->p + (o + len64[i] < cap ? o + len64[i] : cap);
                for (uint32_t tid = 0; tid < kThreads; ++tid)
                    place_block(m, B, C.type, C.size, m.s0, (uintptr_t)out->p, o, cap, tid, kThreads);
            }
            base += run;
        }
        for (uint64_t i = 0; i < kGuard; ++i)
            if (out->p[cap + i] != 0xA5) die("the guard behind the arena was written");
        return base;
    };
    for (uint64_t r : rounds) {
        const uint64_t round = r ? r : nblocks;
        std::vector<uint64_t> foff;
        Buf out;
        const uint64_t total = place_all(round, want.size(), &foff, &out);  // an arena of exactly the need
        if (total != want.size()) die("total differs from the frames' sizes");
        if (memcmp(out.p, want.data(), want.size())) die("arena differs from the frames built file by file");
        for (uint64_t f = 0; f < nfiles; ++f) {
            const uint64_t len = (f + 1 < nfiles ? foff[f + 1] : total) - foff[f];
            if (foff[f] != want_off[f] || len != want_len[f]) die("frame offset or length");
            if (len < kFrameMin || len > zstd::frame_bound(tlen[f])) die("frame length outside its bounds");
        }
        // too small: one byte short, cut inside a header, cut to nothing
        for (uint64_t cap : {total - 1, total > 20 ? total - 20 : 0, want_len[0] - 5, (uint64_t)0}) {
            std::vector<uint64_t> foff2;
            Buf out2;
            if (place_all(round, cap, &foff2, &out2) != total || foff2 != foff) die("sizes change with the arena");
            if (memcmp(out2.p, want.data(), cap)) die("a too-small arena's bytes differ");  // stricter than the contract
        }
    }
}

void refusals() {
    g_batch = "refusals";
    std::vector<File> files;
    uint64_t nb = 0;
    auto refuse = [&](uintptr_t in, uint64_t in_len, std::vector<uint64_t> off, std::vector<uint64_t> len) {
        Err e;
        if (plan(in, in_len, off.data(), len.data(), off.size(), &files, &nb, &e) != SYDELTA_E_INVAL) die("not refused");
        printf("reject %s\n", e.msg.c_str());
    };
    refuse(0x1008, 100, {0}, {10});                                             // the arena itself
    refuse(0x1000, 100, {0, 16, 40}, {10, 10, 10});                             // file 2: offset
    refuse(0x1000, 100, {0, 16, 96}, {10, 10, 5});                              // file 2: one byte past
    refuse(0x1000, 100, {0, 112}, {10, 0});                                     // file 1: empty, but outside
    refuse(0x1000, 100, {0, UINT64_MAX - 15}, {10, 32});                        // file 1: wraps
    refuse(0x1000, 100, {0, 16, 32, 48}, {10, 10, 10, UINT64_MAX});             // file 3: wraps
    refuse(0, 100, {0, 16}, {0, 1});                                            // file 1: NULL arena
    Err e;
    const std::vector<uint64_t> off{0, 16, 96}, len{16, 0, 4};
    if (plan(0x1000, 100, off.data(), len.data(), 3, &files, &nb, &e) || nb != 3) die("a text that ends with the arena");
    const std::vector<uint64_t> z{0, 0};
    if (plan(0, 0, z.data(), z.data(), 2, &files, &nb, &e) || nb != 2) die("empty texts need no arena");

    if (batch_bound(nullptr, 0) != 0 || batch_bound(nullptr, 3) != UINT64_MAX) die("bound of a NULL table");
    const std::vector<uint64_t> big{UINT64_MAX - 100, 5}, two{UINT64_MAX / 2, UINT64_MAX / 2, 1 << 20};
    if (batch_bound(big.data(), 2) != UINT64_MAX || batch_bound(two.data(), 3) != UINT64_MAX) die("bound overflow");
    const std::vector<uint64_t> ok{0, 1, 131072, 131073};
    if (batch_bound(ok.data(), 4) != 17 + 18 + (17 + 131072) + (20 + 131073)) die("bound value");
    if (round_blocks(nullptr) != 4096 || round_blocks("3") != 3 || round_blocks("0") != 4096 ||
        round_blocks("x") != 4096 || round_blocks("99999999999") != kRoundMax)
        die("round knob");
}

}  // namespace

int main(int argc, char** argv) {
    const uint64_t nrandom = argc > 1 ? strtoull(argv[1], nullptr, 10) : 8;
    g_rng = argc > 2 ? strtoull(argv[2], nullptr, 10) * 0x9E3779B97F4A7C15ull + 1 : 1;
    constexpr uint64_t K = zstd::kBlockMax;

    // empty texts first, last and adjacent; the lengths where the coder or the block count
    // changes; with rounds of 3 the files of 2 and 3 blocks straddle rounds
    g_batch = "edges";
    run_batch({"", "", make_text(kCopyJson, 1), make_text(kCopyJson, 1023), make_text(kCopyJson, 1024), "",
               make_text(kCopyJson, K - 1), make_text(kDataJson, K), make_text(kCopyJson, K + 1), make_text(kRle, 300000),
               make_text(kRandom, 5000), make_text(kCopyJson, 3 * K), ""},
              {1, 3, 0});
    g_batch = "one empty";
    run_batch({""}, {1, 3, 0});

    uint64_t nbatches = 2;
    for (uint64_t t = 0; t < nrandom; ++t, ++nbatches) {
        char name[32];
        snprintf(name, sizeof name, "random %llu", (unsigned long long)t);
        g_batch = name;
        std::vector<std::string> texts;
        for (uint64_t f = 0, n = 1 + below(12); f < n; ++f) {
            const uint64_t pick = below(10);
            const uint64_t len = pick == 0 ? 0 : pick == 1 ? K + below(3) - 1 : pick == 2 ? 1 + below(3) : below(20000);
            texts.push_back(make_text((Kind)below(4), len));
        }
        run_batch(texts, {1, 3, 0});
    }
    refusals();
    printf("zstd_batch_check ok: %llu batches\n", (unsigned long long)nbatches);
    return 0;
}
