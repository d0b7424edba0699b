// unzstd_check.cpp — the zstd decoder's stage bodies (sy_amd/csrc/sydelta_unzstd.hpp) on the
// CPU under ASan + UBSan, driven the way the kernels of sydelta_unzstd.hip drive them: one
// call per GPU thread, the data-parallel stages in a shuffled order, every array allocated
// at exactly the size the kernels assume, the tables copied into arrays of exactly their
// size (the kernels' LDS copies), the frame and the output at exact sizes and at every
// alignment 0-15.
//
//   unzstd_check <dir> <mutants per frame> <seed>
//
// <dir>/manifest.txt lists "<name> ok|valid|reject"; <name>.frame, and unless reject <name>.out.
// 1. every ok / valid frame decodes to its bytes; 2. every reject frame returns an error and
// writes nothing; 3. every ok frame is mutated (1-3 byte flips or a truncation): an error or some
// bytes, and whenever libzstd (linked) accepts the mutant, either the same bytes, or one of
// the refusals that are stricter than libzstd 1.4.8 by design, each established from the
// frame's bytes by a reader of its own (excused()); any other refusal is a failure.
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
#include <sstream>
#include <string>
#include <vector>

#include "sydelta_unzstd.hpp"

extern "C" {
size_t ZSTD_decompress(void* dst, size_t cap, const void* src, size_t n);
unsigned ZSTD_isError(size_t code);
}

using namespace sydelta;
using namespace sydelta::unz;

namespace {

// n bytes whose address is k mod 16, the bytes before and behind them poisoned
struct Exact {
    uint8_t* block = nullptr;
    uint8_t* p = nullptr;
    size_t pad = 0;
    Exact(size_t n, unsigned k) {
        pad = k ? k : 16;
        block = (uint8_t*)malloc(pad + n);
        p = block + pad;
        ASAN_POISON_MEMORY_REGION(block, pad);
    }
    ~Exact() {
        ASAN_UNPOISON_MEMORY_REGION(block, pad);
        free(block);
    }
    Exact(const Exact&) = delete;
};

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

std::vector<uint64_t> shuffled(uint64_t n, std::mt19937_64& rng) {
    std::vector<uint64_t> v(n);
    std::iota(v.begin(), v.end(), 0);
    std::shuffle(v.begin(), v.end(), rng);
    return v;
}

// i -> a permutation of [0, n): the shuffled order of the per-byte stages
struct Perm {
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

// The whole decode as sydelta_zstd_decompress_device runs it.  Returns the status word;
// out (exact size, alignment out_align) receives the bytes.
uint64_t decode(const uint8_t* in, uint64_t len, std::vector<uint8_t>& result, unsigned out_align, std::mt19937_64& rng,
                int32_t* seq_left) {
    result.clear();
    *seq_left = 0;
    Totals t;
    uint64_t st = scan(in, len, nullptr, 0, t);
    if (st != kNoErr) return st;
    const Totals c = t;
    Arr<Block> blocks(c.nb);
    st = scan(in, len, blocks.p, c.nb, t);
    if (st != kNoErr) return st;
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
    const std::vector<uint64_t> order = shuffled(c.nb, rng);
    for (uint64_t b : order) report(b, build_tables(in, blocks.p[b], huf.p, fse.p));
    if (status != kNoErr) return status;
    for (uint64_t b : order) {
        Block& k = blocks.p[b];
        if (k.type != 2) continue;
        uint32_t hlog = 0, flog[3] = {0, 0, 0};
        Arr<uint16_t> s_huf(k.lit_type >= 2 ? (size_t)1 << huf.p[k.huf_slot].log : 0);
        if (k.lit_type >= 2) {
            hlog = huf.p[k.huf_slot].log;
            memcpy(s_huf.p, huf.p[k.huf_slot].e, sizeof(uint16_t) << hlog);
        }
        std::vector<std::vector<uint32_t>> s_fse(3);
        if (k.nseq)
            for (int j = 0; j < 3; ++j) {
                const FseTab& T = fse.p[k.fse_slot[j]];
                flog[j] = T.log;
                s_fse[j].assign(T.e, T.e + ((size_t)1 << T.log));
                s_fse[j].shrink_to_fit();
            }
        // wave 1's lane first or last, the literal lanes in a shuffled order
        const bool seq_first = rng() & 1;
        auto run_seq = [&] {
            report(b, seq_decode(in, k, s_fse[0].data(), flog[0], s_fse[1].data(), flog[1], s_fse[2].data(), flog[2],
                                 seqs.p + k.seq_base, hexit.p[b]));
        };
        if (seq_first) run_seq();
        for (uint64_t tid : shuffled(64, rng)) {
            if (k.lit_type < 2) lit_fill(in, k, lits.p, (uint32_t)tid, 64);
            else if (tid < k.lit_streams) report(b, lit_stream(in, k, s_huf.p, hlog, (uint32_t)tid, lits.p));
        }
        if (!seq_first) run_seq();
    }
    if (status != kNoErr) {
        *seq_left = (uint32_t)status == kLitStream ? blocks.p[status >> 32].lit_before : blocks.p[status >> 32].seq_left;
        return status;
    }
    st = stitch(blocks.p, c.nb, hexit.p, entry.p, bpos.p, t);
    if (st != kNoErr) return st;
    for (uint64_t b : order) {
        const Block& k = blocks.p[b];
        if (k.type != 2) continue;
        for (uint64_t i : shuffled(k.nseq, rng)) report(b, resolve(bpos.p[b], entry.p + 3 * b, seqs.p[k.seq_base + i]));
    }
    if (status != kNoErr) return status;
    const uint64_t n = t.out_len;
    Exact out(n, out_align);
    Arr<uint32_t> parent(n);
    const Perm pm(n, rng);
    for (uint64_t j = 0; j < n; ++j) place(pm.at(j), in, blocks.p, c.nb, bpos.p, seqs.p, lits.p, out.p, parent.p);
    for (uint32_t r = 0; r < kUnzRounds; ++r) {
        bool any = false;
        for (uint64_t j = 0; j < n; ++j) any |= jump(pm.at(j), parent.p);
        if (!any) break;
        if (r + 1 == kUnzRounds) {
            fprintf(stderr, "pointer doubling did not settle\n");
            exit(3);
        }
    }
    for (uint64_t j = 0; j < n; ++j) gather(pm.at(j), parent.p, out.p);
    result.assign(out.p, out.p + n);
    return kNoErr;
}

std::vector<uint8_t> slurp(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) {
        fprintf(stderr, "cannot read %s\n", path.c_str());
        exit(2);
    }
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

uint64_t decode_at(const std::vector<uint8_t>& frame, unsigned in_align, unsigned out_align, std::vector<uint8_t>& got,
                   std::mt19937_64& rng, int32_t* seq_left = nullptr) {
    int32_t left = 0;
    if (!seq_left) seq_left = &left;
    Exact in(frame.size(), in_align);
    if (!frame.empty()) memcpy(in.p, frame.data(), frame.size());
    return decode(in.p, frame.size(), got, out_align, rng, seq_left);
}

// A refusal of a frame that libzstd 1.4.8 accepts passes only when this reader, which shares
// no code with the decoder and goes by the frame's bytes, finds the condition that the issue
// or RFC 8878 makes a refusal and libzstd 1.4.8 does not enforce:
//   kChecksum / kDict: the flag, a non-zero Dictionary_ID (unsupported by design);
//   kBlockBig: a Raw or RLE Block_Size above 128 KiB; for a Compressed block the issue's own
//     rule (a block regenerating more than 128 KiB), which no header shows;
//   kTooBig: the issue's 4 GiB rule;
//   kLitStream: four Huffman streams for fewer literals than three segments hold (libzstd
//     1.4.8 writes past the literals there); or the decoder's reader had used the stream up
//     exactly when one symbol was still to come (Block::lit_before == 0: libzstd's
//     double-symbol decoder then reads the stream's first bits a second time and accepts);
//   kSeqHeader: the long form of a zero Number_of_Sequences, or reserved bits in the modes byte;
//   kSeqStream: the decoder's reader ended `left` bits off (Block::seq_left): past the start
//     (libzstd reads on and accepts), or short by no more than the 26 bits of the state update
//     that libzstd 1.4.8 still performs after the last sequence.
// Anything else is a failure.
bool excused(const std::vector<uint8_t>& f, uint64_t st, int32_t left) {
    const uint32_t e = (uint32_t)st;
    const uint64_t b = st >> 32;
    if (e == kTooBig) return true;
    if (f.size() < 6) return false;
    const uint32_t fhd = f[4], did = fhd & 3, single = (fhd >> 5) & 1, fid = fhd >> 6;
    const size_t dbytes = did == 3 ? 4 : did, dpos = 5 + (single ? 0 : 1);
    size_t pos = dpos + dbytes + (fid ? (size_t)1 << fid : single);
    if (e == kChecksum) return (fhd & 4) != 0;
    if (e == kDict) {
        for (size_t i = 0; i < dbytes && dpos + i < f.size(); ++i)
            if (f[dpos + i]) return true;
        return false;
    }
    uint32_t type = 0, size = 0;
    for (uint64_t k = 0;; ++k) {  // to block b
        if (pos + 3 > f.size()) return false;
        const uint32_t h = f[pos] | f[pos + 1] << 8 | f[pos + 2] << 16;
        pos += 3;
        type = (h >> 1) & 3, size = h >> 3;
        if (k == b) break;
        pos += type == 1 ? 1 : size;
    }
    if (e == kBlockBig) return type == 2 || ((type == 0 || type == 1) && size > (128u << 10));
    if (type != 2 || pos + size > f.size() || size < 3) return false;
    const uint8_t* p = f.data() + pos;
    const uint32_t lt = p[0] & 3, sf = (p[0] >> 2) & 3;
    uint32_t lh, regen, csize;
    if (lt < 2) {
        lh = sf == 1 ? 2 : sf == 3 ? 3 : 1;
        regen = lh == 1 ? p[0] >> 3 : (p[0] | p[1] << 8 | (lh == 3 ? p[2] << 16 : 0)) >> 4;
        csize = lt == 0 ? regen : 1;
    } else {
        if (size < 5) return false;
        const uint64_t v = (p[0] | (uint64_t)p[1] << 8 | (uint64_t)p[2] << 16 | (uint64_t)p[3] << 24 | (uint64_t)p[4] << 32) >> 4;
        const uint32_t bits = sf < 2 ? 10 : sf == 2 ? 14 : 18;
        lh = sf < 2 ? 3 : sf == 2 ? 4 : 5;
        regen = (uint32_t)(v & ((1u << bits) - 1)), csize = (uint32_t)((v >> bits) & ((1u << bits) - 1));
        if (e == kLitStream) return (sf != 0 && 3 * ((regen + 3) / 4) > regen) || left == 0;
    }
    if (e == kLitStream) return false;
    if (e == kSeqStream) return left < 0 || (left > 0 && left <= 26);
    if (e == kSeqHeader) {
        const uint32_t q = lh + csize;
        if (q + 1 >= size) return false;
        const uint32_t n = p[q];
        if (n == 128 && p[q + 1] == 0) return true;  // the long form of zero
        const uint32_t m = n == 255 ? q + 3 : n >= 128 ? q + 2 : q + 1;  // the modes byte
        return n != 0 && m < size && (p[m] & 3) != 0;
    }
    return false;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    const std::string dir = argv[1];
    const int nmut = atoi(argv[2]);
    std::mt19937_64 rng(strtoull(argv[3], nullptr, 10));
    std::ifstream man(dir + "/manifest.txt");
    std::string name, kind;
    int fails = 0, nok = 0, nrej = 0;
    uint64_t mutants = 0, both = 0, we_only = 0, strict = 0, rejected = 0, by_code[kErrCount] = {};
    std::vector<uint8_t> zbuf(8u << 20);
    unsigned idx = 0;
    while (man >> name >> kind) {
        const std::vector<uint8_t> frame = slurp(dir + "/" + name + ".frame");
        std::vector<uint8_t> got;
        ++idx;
        if (kind == "reject") {
            const uint64_t st = decode_at(frame, idx % 16, 0, got, rng);
            if (st == kNoErr) printf("FAIL %s: accepted (%zu bytes)\n", name.c_str(), got.size()), ++fails;
            else printf("reject %s: block %llu: %s\n", name.c_str(), (unsigned long long)(st >> 32), err_text((uint32_t)st));
            ++nrej;
            continue;
        }
        const std::vector<uint8_t> want = slurp(dir + "/" + name + ".out");
        for (unsigned rep = 0; rep < 2; ++rep) {
            const unsigned ia = (idx * 5 + rep * 7) % 16, oa = (idx * 3 + rep * 11 + 1) % 16;
            const uint64_t st = decode_at(frame, ia, oa, got, rng);
            if (st != kNoErr)
                printf("FAIL %s: block %llu: %s\n", name.c_str(), (unsigned long long)(st >> 32), err_text((uint32_t)st)), ++fails;
            else if (got != want) {
                size_t d = 0;
                while (d < got.size() && d < want.size() && got[d] == want[d]) ++d;
                printf("FAIL %s: %zu bytes for %zu, first difference at %zu\n", name.c_str(), got.size(), want.size(), d);
                ++fails;
            }
        }
        ++nok;
        for (int m = 0; m < nmut && kind == "ok"; ++m) {
            std::vector<uint8_t> f = frame;
            if (f.empty()) break;
            if (rng() % 8 == 0) {
                f.resize(f.size() > 1 ? 1 + rng() % (f.size() - 1) : 1);  // not to nothing: no bytes are no frame, and libzstd reads them as zero frames
            } else {
                const int flips = 1 + (int)(rng() % 3);
                // half of the flips land in the first 64 bytes, where the headers are
                for (int i = 0; i < flips; ++i) f[(rng() & 1) ? rng() % std::min<size_t>(f.size(), 64) : rng() % f.size()] ^= (uint8_t)(1u << (rng() % 8));
            }
            ++mutants;
            int32_t left = 0;
            const uint64_t st = decode_at(f, (unsigned)(rng() % 16), (unsigned)(rng() % 16), got, rng, &left);
            const size_t zr = ZSTD_decompress(zbuf.data(), zbuf.size(), f.data(), f.size());
            const bool zok = !ZSTD_isError(zr);
            if (st != kNoErr) ++rejected;
            if (zok && st == kNoErr) {
                ++both;
                if (got.size() != zr || (zr && memcmp(got.data(), zbuf.data(), zr))) {
                    printf("FAIL %s mutant %d: libzstd regenerates %zu bytes, we %zu, and they differ\n", name.c_str(), m, zr, got.size());
                    ++fails;
                }
            } else if (zok) {
                if (excused(f, st, left)) ++strict, ++by_code[(uint32_t)st];
                else {
                    printf("FAIL %s mutant %d: libzstd accepts (%zu bytes), we refuse: block %llu: %s\n", name.c_str(), m, zr,
                           (unsigned long long)(st >> 32), err_text((uint32_t)st));
                    ++fails;
                }
            } else if (st == kNoErr) {
                ++we_only;
            }
        }
    }
    printf("frames: %d ok, %d reject; mutants: %llu (%llu refused by us, %llu accepted by both, %llu accepted by us and "
           "refused by libzstd, %llu accepted by libzstd and refused here as stricter by design)\n",
           nok, nrej, (unsigned long long)mutants, (unsigned long long)rejected, (unsigned long long)both,
           (unsigned long long)we_only, (unsigned long long)strict);
    for (uint32_t e = 0; e < kErrCount; ++e)
        if (by_code[e]) printf("  stricter by design: %llu x %s\n", (unsigned long long)by_code[e], err_text(e));
    if (fails) {
        printf("unzstd_check: %d failures\n", fails);
        return 1;
    }
    printf("unzstd_check ok\n");
    return 0;
}
