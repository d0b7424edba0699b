// dparse_wave.hpp — TEST INFRASTRUCTURE.  A wave-by-wave, lane-by-lane replica on the CPU
// of k_dparse_count, k_dparse_place and k_dparse (sy_amd/csrc/sydelta_kernels.hip) built
// from the same arithmetic the kernels use (sydelta_dparse.hpp: stage_off / stage_p0 /
// stage_len, fast_chunk / fast_classify / fast_values, lit_split) and the same chunk
// bodies.  What is LDS on the device is an array of exactly the kernel's size here, so an
// index outside it is an AddressSanitizer report (tests/csrc/kernel_bodies_fuzz.cpp):
//
//   * the wave's rows: kDpRows * kDpRow bytes, filled by the dword copy or the byte copy
//     as the text's address decides, 64 lanes each with the kernel's loop.  The rows are
//     first filled with '5': a fast path that read a byte nobody staged would see a digit
//     and disagree with the bodies on plain memory;
//   * the text outside the staged span: read from the text itself (its own array);
//   * the wave's literal slab: kDpLitMax bytes;
//   * the literal output: the head / dword / tail split; a dword store has to be 4-byte
//     aligned and inside [l0, l1).
//
// The lanes of a wave and the waves run in descending order (one schedule of many).  Used
// by the emulated device (fake_device.cpp) and by kernel_bodies_fuzz.cpp.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>

#include "sydelta_dparse.hpp"

namespace dparse_wave {
using namespace sydelta;

#define DPW_CHECK(c)                                                                      \
    do {                                                                                  \
        if (!(c)) {                                                                       \
            fprintf(stderr, "dparse_wave: CHECK failed: %s (%s:%d)\n", #c, __FILE__, __LINE__); \
            abort();                                                                      \
        }                                                                                 \
    } while (0)

// LdsText's twin: staged bytes from the rows, the rest from the text.
struct RowText {
    const uint8_t* g;
    const uint8_t* l;
    uint64_t p0, n;
    uint8_t operator[](uint64_t p) const {
        const uint64_t d = p - p0;
        if (d < n) return l[dparse::stage_off(d)];
        return g[p];
    }
};
// LdsLit's twin.
struct SlabLit {
    uint8_t* l;
    uint64_t base;
    explicit operator bool() const { return true; }
    uint8_t& operator[](uint64_t i) const {
        DPW_CHECK(i - base < dparse::kDpLitMax);
        return l[i - base];
    }
};

struct Wave {
    std::unique_ptr<uint8_t[]> rows{new uint8_t[dparse::kDpRows * dparse::kDpRow]};
    RowText t{};

    // dp_stage
    void stage(const dparse::DArgs& a, uint64_t c0) {
        memset(rows.get(), '5', dparse::kDpRows * dparse::kDpRow);
        const uint64_t p0 = dparse::stage_p0(a, c0);
        const uint32_t n = dparse::stage_len(a, p0);
        const uint8_t* g = a.t + p0;
        uint8_t* r = rows.get();
        for (uint32_t lane = 64; lane-- > 0;) {
            if (((uintptr_t)g & 3) == 0) {
                for (uint32_t i = 4 * lane; i < n; i += 256) {
                    if (i + 4 <= n) {
                        DPW_CHECK((dparse::stage_off(i) & 3) == 0);
                        memcpy(r + dparse::stage_off(i), g + i, 4);  // one aligned dword, inside one row
                        DPW_CHECK(dparse::stage_off(i + 3) == dparse::stage_off(i) + 3);
                    } else {
                        for (uint32_t j = i; j < n; ++j) r[dparse::stage_off(j)] = g[j];
                    }
                }
            } else {
                for (uint32_t i = lane; i < n; i += 64) r[dparse::stage_off(i)] = g[i];
            }
        }
        t = RowText{a.t, r, p0, n};
    }
    // dp_fast
    bool fast(const dparse::DArgs& a, uint64_t c, uint32_t* x, uint64_t& lits) const {
        lits = 0;
        uint32_t d0;
        if (!dparse::fast_chunk(a, c, t.p0, t.n, d0)) return false;
        DPW_CHECK(d0 >= 4 && (d0 & 3) == 0);
        for (int k = 0; k < 18; ++k) {
            const uint32_t o = dparse::stage_off(d0 + 4 * k);
            DPW_CHECK(dparse::stage_off(d0 + 4 * k + 3) == o + 3 && d0 + 4 * k + 3 < t.n);
            memcpy(&x[k], t.l + o, 4);
        }
        uint32_t prevw;
        memcpy(&prevw, t.l + dparse::stage_off(d0 - 4), 4);
        return dparse::fast_classify(x, prevw >> 24, lits);
    }
};

inline uint32_t lanes_of(const dparse::DArgs& a, uint64_t c0) { return (uint32_t)(a.nc - c0 < 64 ? a.nc - c0 : 64); }

// k_dparse_count.  fast_chunks (optional): how many chunks took the fast path.
inline void count(const dparse::DArgs& a, uint64_t* ocnt, uint64_t* lcnt, uint64_t* fast_chunks = nullptr) {
    Wave w;
    for (uint64_t c0 = (a.nc + 63) & ~63ull; c0 > 0;) {
        c0 -= 64;
        w.stage(a, c0);
        for (uint32_t lane = lanes_of(a, c0); lane-- > 0;) {
            const uint64_t c = c0 + lane;
            uint32_t x[18];
            uint64_t lits, no, nl;
            if (w.fast(a, c, x, lits)) {
                no = 0;
                nl = (uint64_t)__builtin_popcountll(lits);
                if (fast_chunks) ++*fast_chunks;
            } else {
                dparse::chunk_count(a, w.t, c, no, nl);
            }
            ocnt[c] = no;
            lcnt[c] = nl;
        }
    }
}

// k_dparse_place.  orank: nc + 1 entries.
inline void place(const dparse::DArgs& a, const uint64_t* orank, uint64_t* pos) {
    Wave w;
    for (uint64_t c0 = (a.nc + 63) & ~63ull; c0 > 0;) {
        c0 -= 64;
        if (orank[c0 + 64 < a.nc ? c0 + 64 : a.nc] == orank[c0]) continue;  // no op start in the wave
        w.stage(a, c0);
        for (uint32_t lane = lanes_of(a, c0); lane-- > 0;) {
            const uint64_t c = c0 + lane;
            uint32_t x[18];
            uint64_t lits;
            if (!w.fast(a, c, x, lits)) dparse::chunk_place(a, w.t, c, orank[c], pos);
        }
    }
}

// k_dparse.  lit: the literal output (any alignment; NULL: validate only); *bad: the
// smallest bad position (kNoBad to begin with).
inline void parse(const dparse::DArgs& a, const uint64_t* orank, const uint64_t* lrank, const uint64_t* pos,
                  uint64_t nops, sydelta_op* ops, uint8_t* lit, unsigned long long* bad) {
    Wave w;
    std::unique_ptr<uint8_t[]> slab(new uint8_t[dparse::kDpLitMax]);
    for (uint64_t c0 = (a.nc + 63) & ~63ull; c0 > 0;) {
        c0 -= 64;
        w.stage(a, c0);
        memset(slab.get(), 0xA5, dparse::kDpLitMax);  // a slab byte nobody wrote shows in the output
        const uint64_t l0 = lrank[c0], l1 = lrank[c0 + 64 < a.nc ? c0 + 64 : a.nc];
        const bool staged = lit && l1 - l0 <= dparse::kDpLitMax;
        const SlabLit sl{slab.get(), l0};
        for (uint32_t lane = lanes_of(a, c0); lane-- > 0;) {
            const uint64_t c = c0 + lane;
            uint32_t x[18];
            uint64_t lits;
            bool ok = w.fast(a, c, x, lits);
            if (ok)
                ok = dparse::fast_values(x, lits, lrank[c], [&](uint64_t r, uint32_t v) {
                    if (lit) {
                        if (staged) sl[r] = (uint8_t)v;
                        else lit[r] = (uint8_t)v;
                    }
                });
            if (!ok) {
                const uint64_t b = staged ? dparse::chunk_parse(a, w.t, c, orank, lrank, pos, nops, ops, sl)
                                          : dparse::chunk_parse(a, w.t, c, orank, lrank, pos, nops, ops, lit);
                if (b < *bad) *bad = b;
            }
        }
        if (!lit || l1 - l0 > dparse::kDpLitMax || l1 == l0) continue;
        const uint8_t* src = slab.get();
        uint64_t a0, a1;
        dparse::lit_split(l0, l1, (uint32_t)((uintptr_t)lit & 3), a0, a1);
        for (uint32_t lane = 64; lane-- > 0;) {
            if (a0 >= a1) {
                for (uint64_t i = l0 + lane; i < l1; i += 64) lit[i] = src[i - l0];
                continue;
            }
            DPW_CHECK(l0 <= a0 && a0 - l0 < 4 && a1 <= l1 && l1 - a1 < 4);
            if (lane < a0 - l0) lit[l0 + lane] = src[lane];
            if (lane < l1 - a1) lit[a1 + lane] = src[a1 - l0 + lane];
            for (uint64_t i = a0 + 4ull * lane; i < a1; i += 256) {
                const uint64_t k = i - l0;
                DPW_CHECK(((uintptr_t)(lit + i) & 3) == 0 && i + 4 <= a1 && k + 4 <= dparse::kDpLitMax);
                memcpy(lit + i, src + k, 4);  // one aligned dword store
            }
        }
    }
}

}  // namespace dparse_wave
