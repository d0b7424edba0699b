// xxh_scratch_check.cpp — TEST INFRASTRUCTURE, never part of libsydelta.  A stand-alone
// program (g++ -fsanitize=address,undefined, tests/test_xxh_scratch_host.py) that proves on
// the host that k_xxh_chain's unchecked batch prefetch stays inside the scratch that
// sydelta_xxh3_batch_device allocates.
//
// For a batch of file lengths it rebuilds the host tables exactly as
// sydelta_xxh3_batch_device does (nb, pfx, the stable descending order, waves of eight),
// walks the kernel's two loops for every wave to find the last index of Cn that a lane loads
// (which must equal xxh_chain_last_load of sydelta_internal.hpp, the constexpr the sizing is
// derived from), and requires for every lane group, inactive ones with the base the kernel
// gives them, that row 7's last loaded record lies inside the allocation:
//     7 * cstride + fpfx[f] + 1 + last_load < allocated records.
// The scratch is then really allocated and those records are read, so AddressSanitizer
// sees the same accesses.
//
// Batches: the named ones of the file given as argv[1] (one per line: name, then lengths),
// every non-increasing batch of 1 to 9 files with block counts from {0, 1, 2, 63, 64, 65, 66,
// 129} (small files last: the highest fpfx) and each of them reversed, and 2000 seeded random
// batches.  Each named batch prints its excess, the distance of the worst load beyond the last
// record of the eight rows (8 * cstride - 1); negative means inside the rows.
//
// -DXXH_SCRATCH_ROWS_ONLY sizes the allocation as eight rows without the tail, the sizing
// before xxh_scratch_records: the program must then fail (the test builds it both ways).
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <numeric>
#include <sstream>
#include <string>
#include <vector>

#include "sydelta_internal.hpp"

using namespace sydelta;

static uint64_t allocated_records(uint64_t npieces, uint64_t nb_max) {
#ifdef XXH_SCRATCH_ROWS_ONLY
    (void)nb_max;
    return 8 * xxh_chain_records(npieces);
#else
    return xxh_scratch_records(npieces, nb_max);
#endif
}

// The last index of Cn loaded by k_xxh_chain's loops, walked as the kernel walks them.
static uint64_t walk_last_load(uint64_t nmin, uint64_t nmax) {
    uint64_t last = kChainBatch - 1;  // prologue: ba = Cn[0, kChainBatch)
    uint64_t k = 0;
    for (; k + 2 * kChainBatch <= nmin; k += 2 * kChainBatch) last = k + 3 * kChainBatch - 1;
    for (; k < nmax; k += 2 * kChainBatch) last = k + 3 * kChainBatch - 1;
    return last;
}

static uint64_t g_batches = 0, g_waves = 0, g_failures = 0;
static volatile uint64_t g_sink = 0;

// Returns the excess of the batch's worst load over the last record of the eight rows.
static int64_t check_batch(const std::vector<uint64_t>& lens, const char* name) {
    const uint64_t nfiles = lens.size();
    std::vector<uint64_t> pfx(nfiles + 1, 0), nb(nfiles);
    for (uint64_t f = 0; f < nfiles; ++f) {
        nb[f] = lens[f] > 240 ? (lens[f] - 1) >> 10 : 0;
        pfx[f + 1] = pfx[f] + nb[f];
    }
    const uint64_t npieces = pfx[nfiles];
    std::vector<uint32_t> order(nfiles);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return nb[a] > nb[b]; });
    const uint64_t nb_max = *std::max_element(nb.begin(), nb.end());
    const uint64_t cstride = xxh_chain_records(npieces);
    const uint64_t alloc = allocated_records(npieces, nb_max);
    std::vector<uint64_t> scratch(alloc, 1);
    int64_t worst = INT64_MIN;
    ++g_batches;
    for (uint64_t w = 0; w < (nfiles + 7) / 8; ++w) {
        uint64_t base[8], nmin = ~0ull, nmax = 0;
        for (uint64_t g = 0; g < 8; ++g) {
            const uint64_t slot = 8 * w + g;
            const bool act = slot < nfiles;
            const uint32_t f = act ? order[slot] : 0;
            const uint64_t len = act ? lens[f] : 0;
            const uint64_t b = len > 240 ? (len - 1) >> 10 : 0;
            const uint64_t steps = b ? b - 1 : 0;
            base[g] = act ? pfx[f] : 0;
            if (act) nmin = std::min(nmin, steps);
            nmax = std::max(nmax, steps);
        }
        const uint64_t last = walk_last_load(nmin, nmax);
        if (last != xxh_chain_last_load(nmin, nmax)) {
            printf("FAIL %s: wave %" PRIu64 " nmin %" PRIu64 " nmax %" PRIu64 ": loops load Cn[%" PRIu64
                   "], xxh_chain_last_load says %" PRIu64 "\n",
                   name, w, nmin, nmax, last, xxh_chain_last_load(nmin, nmax));
            ++g_failures;
        }
        ++g_waves;
        for (uint64_t g = 0; g < 8; ++g) {
            const uint64_t rec = 7 * cstride + base[g] + 1 + last;
            worst = std::max(worst, (int64_t)rec - (int64_t)(8 * cstride - 1));
            if (rec >= alloc) {
                if (g_failures < 20)
                    printf("FAIL %s: wave %" PRIu64 " group %" PRIu64 " (nmax %" PRIu64 ") loads record %" PRIu64
                           " of %" PRIu64 " allocated\n",
                           name, w, g, nmax, rec, alloc);
                ++g_failures;
                continue;
            }
            for (uint64_t i = 0; i < 8; ++i) g_sink += scratch[i * cstride + base[g] + 1 + last];
        }
    }
    return worst;
}

static uint64_t len_of_blocks(uint64_t nb) { return nb ? nb * 1024 + 1 : 5; }

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // splitmix64
    uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static void enumerate(std::vector<uint64_t>& blocks, size_t n, size_t from) {
    static const uint64_t kCounts[8] = {129, 66, 65, 64, 63, 2, 1, 0};  // descending
    if (blocks.size() == n) {
        std::vector<uint64_t> lens;
        for (uint64_t b : blocks) lens.push_back(len_of_blocks(b));
        check_batch(lens, "enumerated");
        std::reverse(lens.begin(), lens.end());
        check_batch(lens, "enumerated-reversed");
        return;
    }
    for (size_t c = from; c < 8; ++c) {
        blocks.push_back(kCounts[c]);
        enumerate(blocks, n, c);
        blocks.pop_back();
    }
}

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: xxh_scratch_check CASES\n");
        return 2;
    }
    std::ifstream in(argv[1]);
    std::string line;
    uint64_t named = 0;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string name;
        if (!(ss >> name)) continue;
        std::vector<uint64_t> lens;
        uint64_t v;
        while (ss >> v) lens.push_back(v);
        if (lens.empty()) {
            fprintf(stderr, "empty batch %s\n", name.c_str());
            return 2;
        }
        printf("%s excess=%" PRId64 "\n", name.c_str(), check_batch(lens, name.c_str()));
        ++named;
    }
    for (size_t n = 1; n <= 9; ++n) {
        std::vector<uint64_t> blocks;
        enumerate(blocks, n, 0);
    }
    for (int t = 0; t < 2000; ++t) {
        const uint64_t nfiles = 1 + rnd() % 40;
        std::vector<uint64_t> lens;
        for (uint64_t f = 0; f < nfiles; ++f) {
            const uint64_t kind = rnd() % 8;
            uint64_t len;
            if (kind == 0) len = rnd() % 241;                          // no chain
            else if (kind == 1) len = 241 + rnd() % 2000;               // 0 or 1 block
            else if (kind == 2) len = len_of_blocks(60 + rnd() % 12);   // around one round
            else if (kind == 3) len = len_of_blocks(120 + rnd() % 20);  // around two rounds
            else if (kind == 4) len = 1 + rnd() % (4u << 20);
            else len = 1 + rnd() % (300u << 10);
            lens.push_back(len);
        }
        check_batch(lens, "random");
    }
    if (g_failures) {
        printf("xxh_scratch_check FAILED: %" PRIu64 " loads outside the allocation or off the helper\n", g_failures);
        return 1;
    }
    printf("xxh_scratch_check ok: %" PRIu64 " named, %" PRIu64 " batches, %" PRIu64 " waves\n", named, g_batches, g_waves);
    return 0;
}
