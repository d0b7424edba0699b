// blake3_host_check.cpp — the portable part of sy_amd/csrc/sydelta_blake3.hpp (compress, the
// level-wise tree, the join of pieces) under AddressSanitizer + UndefinedBehaviorSanitizer,
// as a program of its own (tests/test_blake3_host.py builds it with g++ and runs it).
//
//   blake3_host_check CASES
//
// CASES is a text file, one case per line, inputs are bytes(i % 251 for i in range(len)):
//   hash LEN HEX                   BLAKE3 of the input
//   cv LEN FIRST_CHUNK HEX         chaining value of the input as a piece that starts at FIRST_CHUNK
//   join LEN PIECE_CHUNKS HEX      the input cut into pieces of PIECE_CHUNKS chunks, joined
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "sydelta_blake3.hpp"

using namespace sydelta;

static std::string hex(const uint8_t* p, size_t n) {
    static const char* d = "0123456789abcdef";
    std::string s;
    for (size_t i = 0; i < n; ++i) {
        s += d[p[i] >> 4];
        s += d[p[i] & 15];
    }
    return s;
}

static std::vector<uint8_t> pattern(uint64_t n) {
    std::vector<uint8_t> v(n);
    for (uint64_t i = 0; i < n; ++i) v[i] = (uint8_t)(i % 251);
    return v;
}

static int fails = 0;
static void expect(const char* what, unsigned long long a, unsigned long long b, const std::string& got, const char* want) {
    if (got != want) {
        ++fails;
        fprintf(stderr, "%s %llu %llu: got %s, expected %s\n", what, a, b, got.c_str(), want);
    }
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    char kind[16], want[80];
    unsigned long long a, b;
    int ncases = 0;
    while (fscanf(f, "%15s", kind) == 1) {
        uint8_t out[32];
        uint32_t w[8];
        if (!strcmp(kind, "hash")) {
            if (fscanf(f, "%llu %79s", &a, want) != 2) return 2;
            const std::vector<uint8_t> d = pattern(a);
            b3::hash_host(d.data(), d.size(), 0, true, w);
            b3::words_to_bytes(w, out);
            expect(kind, a, 0, hex(out, 32), want);
        } else if (!strcmp(kind, "cv")) {
            if (fscanf(f, "%llu %llu %79s", &a, &b, want) != 3) return 2;
            const std::vector<uint8_t> d = pattern(a);
            b3::hash_host(d.data(), d.size(), b, false, w);
            b3::words_to_bytes(w, out);
            expect(kind, a, b, hex(out, 32), want);
        } else if (!strcmp(kind, "join")) {
            if (fscanf(f, "%llu %llu %79s", &a, &b, want) != 3) return 2;
            const std::vector<uint8_t> d = pattern(a);
            const uint64_t step = b * 1024;
            std::vector<uint8_t> cvs;
            std::vector<uint64_t> pc;
            for (uint64_t o = 0; o < a; o += step) {
                const uint64_t n = a - o < step ? a - o : step;
                b3::hash_host(d.data() + o, n, o / 1024, false, w);
                cvs.resize(cvs.size() + 32);
                b3::words_to_bytes(w, cvs.data() + cvs.size() - 32);
                pc.push_back(b3::chunks_of(n));
            }
            if (!b3::pieces_ok(pc.data(), pc.size())) {
                ++fails;
                fprintf(stderr, "join %llu %llu: pieces refused\n", a, b);
                continue;
            }
            b3::join(cvs.data(), pc.size(), out);
            expect(kind, a, b, hex(out, 32), want);
        } else {
            return 2;
        }
        ++ncases;
    }
    fclose(f);
    // the piece contract
    const uint64_t bad1[] = {3, 3, 1}, bad2[] = {4, 2, 4}, bad3[] = {4, 4, 5}, bad4[] = {4}, bad5[] = {0, 0}, ok1[] = {4, 4, 1};
    if (b3::pieces_ok(bad1, 3) || b3::pieces_ok(bad2, 3) || b3::pieces_ok(bad3, 3) || b3::pieces_ok(bad4, 1) ||
        b3::pieces_ok(bad5, 2) || b3::pieces_ok(ok1, 0) || !b3::pieces_ok(ok1, 3)) {
        ++fails;
        fprintf(stderr, "pieces_ok\n");
    }
    // the first compression of the empty input by hand: IV, a zero block, CHUNK_START | CHUNK_END | ROOT
    {
        uint32_t cv[8];
        const uint32_t m[16] = {0};
        uint8_t out[32];
        b3::iv(cv);
        b3::compress(cv, m, 0, 0, b3::kChunkStart | b3::kChunkEnd | b3::kRoot);
        b3::words_to_bytes(cv, out);
        expect("compress", 0, 0, hex(out, 32), "af1349b9f5f9a1a6a0404dea36dcc9499bcb25c9adc112b7cc9a93cae41f3262");
    }
    if (fails) return 1;
    printf("blake3_host_check ok: %d cases\n", ncases);
    return 0;
}
