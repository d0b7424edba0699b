// sig_batch_check.cpp — the batched signature JSON writer and parser
// (sy_amd/csrc/sydelta_sigbatch.hpp over the bodies of sydelta_sigjson.hpp) on the CPU under
// ASan + UBSan: what sydelta_checksums_batch_to_json_device, sydelta_checksums_batch_from_json_device
// and their kernels run -- the plans, the tile's file, the per-tile and per-file bodies, the
// staged span's geometry -- on host memory with every array at its exact size and the stages'
// tiles and files in shuffled order.
//
//   sig_batch_check <seed>
//
// The reference of every text is the single writer's bodies run on the file alone; the
// reference of every parse is the single parser's bodies (chunk_entries / chunk_parse) run on
// the text alone, and for a layout refusal the '{' the text was built with.
#include <sanitizer/asan_interface.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <numeric>
#include <random>
#include <string>
#include <vector>

#include "sydelta_sigbatch.hpp"

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

// ---- signatures and their texts
struct Sig {
    std::vector<uint32_t> w;
    std::vector<uint64_t> s;
    uint64_t last = 0;
};

// The single writer's bodies on the file alone (sydelta_checksums_to_json_device's text).
Bytes text_alone(const Sig& g, uint64_t bs) {
    if (g.w.empty()) return Bytes{'[', ']'};
    const sigjson::SigArgs a{g.w.data(), g.s.data(), g.w.size(), bs, g.last};
    Bytes t;
    for (uint64_t i = 0; i < a.n; ++i) {
        uint8_t e[sigjson::kMaxEntry];
        const uint32_t k = sigjson::entry_write(a, i, e);
        CHECK(k == sigjson::entry_len(a, i), "entry_len %llu\n", (unsigned long long)i);
        t.insert(t.end(), e, e + k);
    }
    return t;
}

uint64_t rand_digits(std::mt19937_64& rng, uint64_t maxv) {  // a value with a random number of digits
    const uint64_t v = rng() >> (rng() % 64);
    return v > maxv ? v % (maxv + 1) : v;
}

Sig make_sig(uint64_t n, uint64_t bs, uint64_t last, std::mt19937_64& rng, bool extremes) {
    Sig g;
    g.last = n ? last : 0;
    static const uint32_t ew[] = {0, 9, 10, 0xFFFFFFFFu};
    static const uint64_t es[] = {0, UINT64_MAX};
    for (uint64_t i = 0; i < n; ++i) {
        g.w.push_back(extremes ? ew[i % 4] : (uint32_t)rand_digits(rng, 0xFFFFFFFFu));
        g.s.push_back(extremes ? es[(i / 4) % 2] : rand_digits(rng, UINT64_MAX));
    }
    (void)bs;
    return g;
}

// ---- the writer, as the kernels run it
void run_writer(const std::vector<Sig>& sigs, uint64_t bs, unsigned phase, std::mt19937_64& rng) {
    const uint64_t nf = sigs.size();
    std::vector<uint64_t> nblocks(nf), lasts(nf);
    uint64_t ne = 0;
    for (uint64_t f = 0; f < nf; ++f) nblocks[f] = sigs[f].w.size(), lasts[f] = sigs[f].last, ne += nblocks[f];
    Arr<uint32_t> weak(ne);
    Arr<uint64_t> strong(ne);
    for (uint64_t f = 0, at = 0; f < nf; at += nblocks[f], ++f) {
        std::copy(sigs[f].w.begin(), sigs[f].w.end(), weak.p + at);
        std::copy(sigs[f].s.begin(), sigs[f].s.end(), strong.p + at);
    }
    std::vector<sigb::WFile> files;
    std::vector<uint64_t> lo, hi;
    uint64_t nent = 0, ntiles = 0;
    sigb::PlanErr err;
    const int rc = sigb::wplan(true, nblocks.data(), lasts.data(), nf, bs, &files, &lo, &hi, &nent, &ntiles, &err);
    CHECK(rc == 0 && nent == ne, "wplan: %s\n", err.msg.c_str());
    if (rc) return;
    Arr<sigb::WFile> F(nf);
    std::copy(files.begin(), files.end(), F.p);

    // k_sigb_len, the scan, k_sigb_files, the scan
    Arr<uint64_t> tlen(ntiles + 1), toff(ntiles + 1), tl(nf), pad(nf), to(nf);
    for (uint64_t tile : shuffled(ntiles, rng)) {
        const uint64_t f = sigb::file_of_tile(F.p, nf, tile);
        CHECK(F.p[f].tbase <= tile && tile < F.p[f].tbase + sigb::wtiles_of(F.p[f].n), "file_of_tile %llu\n",
              (unsigned long long)tile);
        const sigjson::SigArgs A = sigb::wargs_of(weak.p, strong.p, F.p[f], bs);
        uint64_t s = 0;
        for (uint32_t k = 0; k < sigjson::kTile; ++k) s += sigb::wslot_len(A, tile - F.p[f].tbase, k);
        tlen.p[tile] = s;
    }
    tlen.p[ntiles] = 0;
    exclusive(tlen.p, toff.p, ntiles + 1);
    for (uint64_t f : shuffled(nf, rng)) {
        tl.p[f] = sigb::wfile_len(F.p, nf, ntiles, toff.p, f);
        pad.p[f] = sigb::pad16(tl.p[f]);
    }
    exclusive(pad.p, to.p, nf);
    const uint64_t need = to.p[nf - 1] + tl.p[nf - 1];
    const uint64_t bound = sigb::wbound(nblocks.data(), lasts.data(), nf, bs);
    CHECK(need <= bound && bound != UINT64_MAX, "bound %llu < need %llu\n", (unsigned long long)bound, (unsigned long long)need);
    for (uint64_t f = 0; f < nf; ++f)
        CHECK(tl.p[f] >= lo[f] && tl.p[f] <= hi[f], "file %llu: length outside text_bounds\n", (unsigned long long)f);

    // k_sigb_write into an arena at `phase`, inside a 0xA5 guard
    const uint64_t G = 48;
    Exact arena(need + 2 * G, phase);
    memset(arena.p, 0xA5, need + 2 * G);
    uint8_t* out = arena.p + G;
    std::vector<uint8_t> stage(sigjson::kStage);
    for (uint64_t tile : shuffled(ntiles, rng)) {
        const uint64_t f = sigb::file_of_tile(F.p, nf, tile);
        const sigjson::SigArgs A = sigb::wargs_of(weak.p, strong.p, F.p[f], bs);
        uint32_t off = 0;
        for (uint32_t k = 0; k < sigjson::kTile; ++k) {
            const uint32_t l = sigb::wslot_len(A, tile - F.p[f].tbase, k);
            if (l) sigb::wslot_write(A, tile - F.p[f].tbase, k, stage.data() + off);
            off += l;
        }
        CHECK(off == tlen.p[tile], "tile %llu: composed %u bytes, sized %llu\n", (unsigned long long)tile, off,
              (unsigned long long)tlen.p[tile]);
        uint8_t* dst = out + to.p[f] + (toff.p[tile] - toff.p[F.p[f].tbase]);
        const uintptr_t c0 = (uintptr_t)dst & ~(uintptr_t)15, c1 = ((uintptr_t)dst + off + 15) & ~(uintptr_t)15;
        for (uintptr_t c = c0; c < c1; c += 16) sigjson::store_chunk(stage.data(), off, dst, c);
    }
    // every text equals the single writer's; the packing rule; pads and guards intact
    std::vector<uint8_t> seen(need + 2 * G, 0);
    uint64_t at = 0;
    for (uint64_t f = 0; f < nf; ++f) {
        const Bytes ref = text_alone(sigs[f], bs);
        CHECK(to.p[f] == at, "file %llu: text_off %llu, packing says %llu\n", (unsigned long long)f,
              (unsigned long long)to.p[f], (unsigned long long)at);
        CHECK(tl.p[f] == ref.size() && !memcmp(out + to.p[f], ref.data(), ref.size()), "file %llu (%llu blocks, bs %llu): text differs\n",
              (unsigned long long)f, (unsigned long long)nblocks[f], (unsigned long long)bs);
        std::fill(seen.begin() + G + to.p[f], seen.begin() + G + to.p[f] + tl.p[f], 1);
        at += sigb::pad16(tl.p[f]);
    }
    for (uint64_t i = 0; i < need + 2 * G; ++i)
        if (!seen[i] && arena.p[i] != 0xA5) {
            CHECK(false, "byte %lld outside the texts was written (phase %u)\n", (long long)i - (long long)G, phase);
            break;
        }
}

// ---- the parser's staged span, replicated on host memory: the accessor of the kernels' waves
struct Staged {
    const uint8_t* g;
    const uint8_t* rows;
    uint64_t p0;
    uint32_t n, ph;
    uint64_t* misses;
    uint8_t operator[](uint64_t p) const {
        const uint64_t d = p - p0;
        if (d < n) return rows[sigb::stage_off((uint32_t)d + ph)];
        ++*misses;
        return g[p];
    }
};
struct StageBuf {
    Arr<uint8_t> rows{sigb::kRows * sigb::kRow};
    Staged stage(const uint8_t* t, uint64_t len, uint64_t c0, uint64_t* misses) {
        const uint64_t p0 = sigb::span_p0(c0);
        const uint32_t n = sigb::span_len(len, c0, p0);
        const uint32_t ph = (uint32_t)((uintptr_t)(t + p0) & 15);
        CHECK(((ph + n + 15) & ~15u) <= sigb::kRows * 64, "span of %u bytes at phase %u leaves the rows\n", n, ph);
        memset(rows.p, 0x7B, rows.n);  // '{' wherever the granules' edge bytes would lie
        for (uint32_t d = 0; d < n; ++d) rows.p[sigb::stage_off(ph + d)] = t[p0 + d];
        return Staged{t, rows.p, p0, n, ph, misses};
    }
};

// ---- the single parser on one text alone (sydelta_checksums_from_json_device's steps)
struct Alone {
    uint64_t bad = UINT64_MAX;
    std::vector<sydelta_block_checksum> e;
};
Alone parse_alone(const Bytes& text) {
    Alone r;
    const uint64_t len = text.size();
    if (len < 2) return r.bad = 0, r;
    Exact t(len, 0);
    memcpy(t.p, text.data(), len);
    const uint64_t nc = (len + sigjson::kParseChunk - 1) / sigjson::kParseChunk;
    std::vector<uint64_t> cnt(nc), rank(nc);
    for (uint64_t c = 0; c < nc; ++c) cnt[c] = sigjson::chunk_entries((const uint8_t*)t.p, len, c);
    exclusive(cnt.data(), rank.data(), nc);
    r.e.resize(rank[nc - 1] + cnt[nc - 1]);
    for (uint64_t c = 0; c < nc; ++c)
        r.bad = std::min(r.bad, sigjson::chunk_parse((const uint8_t*)t.p, len, c, rank[c], r.e.data(), r.e.size()));
    return r;
}

struct PCase {
    std::string name;
    Bytes text;
    uint64_t want = 0;         // the status word the caller gets
    const Sig* sig = nullptr;  // a good file's values
};

struct Layout {
    std::vector<uint64_t> off;
    uint64_t total = 0;
};
enum Pack { kPack16, kOdd };
Layout layout_of(const std::vector<const PCase*>& order, Pack how) {
    Layout L;
    uint64_t at = how == kOdd ? 3 : 0;
    for (const PCase* c : order) {
        L.off.push_back(at);
        at += how == kOdd ? c->text.size() + 1 + (c->text.size() & 3) : sigb::pad16(c->text.size());
    }
    L.total = at + (how == kOdd ? 5 : 0);
    return L;
}

// The batch `order` (a case may stand in it twice), at the given places of an arena at `phase`.
void run_parser(const std::vector<const PCase*>& order, const std::vector<uint64_t>& toff, uint64_t arena_len,
                uint64_t bs, unsigned phase, std::mt19937_64& rng, const char* what, bool report) {
    const uint64_t nf = order.size();
    Exact arena(arena_len, phase);
    static const char kPadText[] = "{1,{\"index\":2,";
    for (uint64_t i = 0; i < arena_len; ++i) arena.p[i] = (uint8_t)kPadText[i % (sizeof kPadText - 1)];
    std::vector<uint64_t> tlen(nf);
    for (uint64_t f = 0; f < nf; ++f) {
        tlen[f] = order[f]->text.size();
        if (tlen[f]) memcpy(arena.p + toff[f], order[f]->text.data(), tlen[f]);
    }
    std::vector<sigb::PFile> files;
    uint64_t nchunks = 0, ntiles = 0;
    sigb::PlanErr err;
    const int rc = sigb::pplan(true, arena_len, toff.data(), tlen.data(), nf, bs, &files, &nchunks, &ntiles, &err);
    CHECK(rc == 0, "%s: pplan: %s\n", what, err.msg.c_str());
    if (rc) return;
    Arr<sigb::PFile> F(nf);
    std::copy(files.begin(), files.end(), F.p);

    // k_sigpb_count (staged and plain must agree), the scan, k_sigpb_sizes
    Arr<uint64_t> cnt(nchunks + 1), rank(nchunks + 1), sig_off(nf), nblocks(nf), last(nf), status(nf), lay_i(nf);
    StageBuf sb;
    uint64_t misses = 0;
    for (uint64_t tile : shuffled(ntiles, rng)) {
        const uint64_t f = sigb::file_of_tile(F.p, nf, tile);
        const sigb::PFile& P = F.p[f];
        const uint64_t nc = sigb::chunks_of(P.len), c0 = (tile - P.tbase) * sigb::kTileChunks;
        CHECK(P.tbase <= tile && c0 < nc, "%s: file_of_tile %llu\n", what, (unsigned long long)tile);
        const uint8_t* t = arena.p + P.off;
        const Staged x = sb.stage(t, P.len, c0, &misses);
        for (uint64_t c = c0; c < nc && c < c0 + sigb::kTileChunks; ++c) {
            cnt.p[P.cbase + c] = sigb::count_chunk(x, P.len, c);
            CHECK(cnt.p[P.cbase + c] == sigb::count_chunk(t, P.len, c), "%s: staged count differs\n", what);
        }
    }
    CHECK(misses == 0, "%s: the count left its span %llu times\n", what, (unsigned long long)misses);
    cnt.p[nchunks] = 0;
    exclusive(cnt.p, rank.p, nchunks + 1);
    for (uint64_t f : shuffled(nf, rng))
        sigb::sizes_file(F.p[f], rank.p, sig_off.p[f], nblocks.p[f], last.p[f], status.p[f], lay_i.p[f]);
    const uint64_t need = rank.p[nchunks];

    // k_sigpb_parse into an SoA of exactly `need` entries
    Arr<uint32_t> weak(need);
    Arr<uint64_t> strong(need);
    memset(weak.p, 0xCD, need * 4);
    memset(strong.p, 0xCD, need * 8);
    uint64_t good_misses = 0;
    for (uint64_t tile : shuffled(ntiles, rng)) {
        const uint64_t f = sigb::file_of_tile(F.p, nf, tile);
        const sigb::PFile& P = F.p[f];
        const uint64_t nc = sigb::chunks_of(P.len), c0 = (tile - P.tbase) * sigb::kTileChunks;
        const uint8_t* t = arena.p + P.off;
        uint64_t m = 0;
        const Staged x = sb.stage(t, P.len, c0, &m);
        for (uint64_t c = c0; c < nc && c < c0 + sigb::kTileChunks; ++c) {
            uint64_t l = UINT64_MAX, li = sigb::kNoBad;
            const uint64_t w = sigb::parse_chunk(x, P.len, c, rank.p[P.cbase + c] - sig_off.p[f], nblocks.p[f], bs,
                                                 sig_off.p[f], weak.p, strong.p, &l, &li);
            uint64_t l2 = UINT64_MAX, li2 = sigb::kNoBad;  // the plain form: checked only
            const uint64_t w2 = sigb::parse_chunk(t, P.len, c, rank.p[P.cbase + c] - sig_off.p[f], nblocks.p[f], bs,
                                                  sig_off.p[f], (uint32_t*)nullptr, (uint64_t*)nullptr, &l2, &li2);
            CHECK(w == w2 && l == l2 && li == li2, "%s: staged and plain parse differ\n", what);
            if (l != UINT64_MAX) last.p[f] = l;
            status.p[f] = std::min(status.p[f], w);
            lay_i.p[f] = std::min(lay_i.p[f], li);
        }
        if (order[f]->want == 0) good_misses += m;
    }
    CHECK(good_misses == 0, "%s: a well-formed text left its span %llu times\n", what, (unsigned long long)good_misses);

    // every file against its text alone
    uint64_t at = 0;
    for (uint64_t f = 0; f < nf; ++f) {
        const PCase& c = *order[f];
        const uint64_t st = sigb::status_out(status.p[f]);
        CHECK(sig_off.p[f] == at, "%s: file %llu: sig_off\n", what, (unsigned long long)f);
        at += nblocks.p[f];
        CHECK(st == c.want, "%s: file %llu (%s): status %llx, want %llx\n", what, (unsigned long long)f, c.name.c_str(),
              (unsigned long long)st, (unsigned long long)c.want);
        const Alone a = parse_alone(c.text);
        if (!(c.want >> 63)) CHECK((a.bad == UINT64_MAX ? 0 : 1 + a.bad) == c.want, "%s: %s: the single parser says %llu\n", what,
                                   c.name.c_str(), (unsigned long long)a.bad);
        if (c.text.size() >= 2) CHECK(nblocks.p[f] == a.e.size(), "%s: file %llu: nblocks\n", what, (unsigned long long)f);
        if (report && st)
            printf("reject %s: %s\n", c.name.c_str(), sigb::refusal_message(f, status.p[f], lay_i.p[f], bs).c_str());
        if (c.want) continue;
        CHECK(c.sig && nblocks.p[f] == c.sig->w.size() && last.p[f] == c.sig->last, "%s: file %llu (%s): tables\n", what,
              (unsigned long long)f, c.name.c_str());
        for (uint64_t i = 0; i < nblocks.p[f] && c.sig && i < c.sig->w.size(); ++i)
            if (weak.p[sig_off.p[f] + i] != c.sig->w[i] || strong.p[sig_off.p[f] + i] != c.sig->s[i] ||
                a.e[i].weak != c.sig->w[i] || a.e[i].strong != c.sig->s[i]) {
                CHECK(false, "%s: file %llu (%s): entry %llu differs\n", what, (unsigned long long)f, c.name.c_str(),
                      (unsigned long long)i);
                break;
            }
    }
    CHECK(at == need, "%s: sig_need\n", what);
}

void run_orders(const std::vector<PCase>& cases, uint64_t bs, std::mt19937_64& rng, const char* what) {
    std::vector<const PCase*> fwd, rev, shuf;
    for (const PCase& c : cases) fwd.push_back(&c);
    rev.assign(fwd.rbegin(), fwd.rend());
    shuf = fwd;
    std::shuffle(shuf.begin(), shuf.end(), rng);
    for (unsigned phase : {0u, 1u, 7u})
        for (Pack how : {kPack16, kOdd})
            for (const auto* order : {&fwd, &rev, &shuf}) {
                const Layout L = layout_of(*order, how);
                run_parser(*order, L.off, L.total, bs, phase, rng, what, false);
            }
    // one text listed twice: the same place, two files
    std::vector<const PCase*> twice = fwd;
    Layout L = layout_of(twice, kPack16);
    twice.push_back(fwd[fwd.size() / 2]);
    L.off.push_back(L.off[fwd.size() / 2]);
    run_parser(twice, L.off, L.total, bs, 1, rng, what, false);
}

// ---- texts built entry by entry, for the refusals
struct Ent {
    std::string index, offset, size, weak, strong;
};
std::string u64s(uint64_t v) { return std::to_string((unsigned long long)v); }
std::vector<Ent> good_entries(uint64_t n, uint64_t bs, uint64_t last) {
    std::vector<Ent> e;
    for (uint64_t i = 0; i < n; ++i)
        e.push_back(Ent{u64s(i), u64s(i * bs), u64s(i + 1 == n ? last : bs), u64s(1000 + 37 * i), u64s(0x9E3779B97F4A7C15ull * (i + 1))});
    return e;
}
// The text and the '{' of every entry.
Bytes text_of(const std::vector<Ent>& e, std::vector<uint64_t>* brace) {
    std::string t = "[";
    for (size_t i = 0; i < e.size(); ++i) {
        if (i) t += ",";
        brace->push_back(t.size());
        t += "{\"index\":" + e[i].index + ",\"offset\":" + e[i].offset + ",\"size\":" + e[i].size + ",\"weak\":" + e[i].weak +
             ",\"strong\":" + e[i].strong + "}";
    }
    t += "]";
    return Bytes(t.begin(), t.end());
}
Bytes replace_first(const Bytes& t, const std::string& a, const std::string& b) {
    std::string s(t.begin(), t.end());
    const size_t at = s.find(a);
    if (at != std::string::npos) s.replace(at, a.size(), b);
    return Bytes(s.begin(), s.end());
}

void run_refusals(uint64_t bs, std::mt19937_64& rng) {
    const uint64_t n = 5, last = bs > 1 ? bs - 1 : 1;
    const std::vector<Ent> E = good_entries(n, bs, last);
    std::vector<uint64_t> br;
    const Bytes good = text_of(E, &br);
    std::vector<PCase> bad;
    auto spelling = [&](const char* name, const Bytes& t) {
        const Alone a = parse_alone(t);
        CHECK(a.bad != UINT64_MAX, "%s: the single parser accepts it\n", name);
        bad.push_back(PCase{name, t, 1 + a.bad, nullptr});
    };
    auto with = [&](size_t i, void (*edit)(Ent&, uint64_t), std::vector<uint64_t>* b) {
        std::vector<Ent> e = E;
        edit(e[i], bs);
        return text_of(e, b);
    };
    auto layout = [&](const char* name, size_t i, void (*edit)(Ent&, uint64_t)) {
        std::vector<uint64_t> b;
        const Bytes t = with(i, edit, &b);
        bad.push_back(PCase{name, t, sigb::kLayoutBit | (1 + b[i]), nullptr});
    };
    std::vector<uint64_t> scratch;
    spelling("space-after-comma", replace_first(good, ",", ", "));
    spelling("missing-bracket", Bytes(good.begin(), good.end() - 1));
    spelling("Weak", replace_first(good, "\"weak\"", "\"Weak\""));
    spelling("leading-zero", with(1, [](Ent& e, uint64_t) { e.weak = "0" + e.weak; }, &scratch));
    spelling("weak-2^32", with(2, [](Ent& e, uint64_t) { e.weak = "4294967296"; }, &scratch));
    spelling("above-u64", with(2, [](Ent& e, uint64_t) { e.strong = "18446744073709551616"; }, &scratch));
    spelling("one-byte", Bytes{'['});
    spelling("no-bytes", Bytes{});
    layout("index-off-by-one", 2, [](Ent& e, uint64_t) { e.index = "3"; });
    layout("offset", 3, [](Ent& e, uint64_t b) { e.offset = u64s(3 * b + 1); });
    layout("size-not-bs", 1, [](Ent& e, uint64_t b) { e.size = u64s(b + 1); });
    layout("last-size-0", 4, [](Ent& e, uint64_t) { e.size = "0"; });
    layout("last-size-bs+1", 4, [](Ent& e, uint64_t b) { e.size = u64s(b + 1); });
    {  // both kinds in one file: the spelling one is reported
        std::vector<Ent> e = E;
        e[1].size = u64s(bs + 7);
        e[3].weak = "00";
        std::vector<uint64_t> b;
        spelling("both-kinds", text_of(e, &b));
    }
    // each between two good files that must stay exact
    Sig g1 = make_sig(3, bs, bs, rng, false), g2 = make_sig(70, bs, 1, rng, true);
    const PCase A{"good-a", text_alone(g1, bs), 0, &g1}, B{"good-b", text_alone(g2, bs), 0, &g2};
    for (const PCase& c : bad) {
        const std::vector<const PCase*> order{&A, &c, &B};
        for (Pack how : {kPack16, kOdd}) {
            const Layout L = layout_of(order, how);
            run_parser(order, L.off, L.total, bs, how == kOdd ? 7 : 0, rng, c.name.c_str(), how == kPack16 && bs == 4096);
        }
    }
}

// A signature one of whose '{' stands on byte `want` mod `mod` of its text.
bool brace_at(const Bytes& t, uint64_t mod, uint64_t want) {
    for (uint64_t p = 0; p < t.size(); ++p)
        if (t[p] == '{' && p % mod == want) return true;
    return false;
}

void run_all(uint64_t bs, uint64_t seed) {
    std::mt19937_64 rng(seed ^ bs);
    // the file set: neighbouring empty files, tile edges, last_size 1 and bs, the extremes
    std::vector<Sig> sigs;
    const uint64_t counts[] = {1, 0, 2, 0, 0, 255, 256, 257, 513, 0};
    for (uint64_t n : counts) sigs.push_back(make_sig(n, bs, n % 2 ? 1 : bs, rng, false));
    sigs.push_back(make_sig(257, bs, bs, rng, true));
    sigs.push_back(make_sig(9, bs, 1, rng, true));
    // a '{' on the last byte of a chunk and on the last byte of a 4 KiB tile
    bool found = false;
    for (int k = 0; k < 4000 && !found; ++k) {
        Sig g = make_sig(513, bs, bs, rng, false);
        const Bytes t = text_alone(g, bs);
        if (brace_at(t, 4096, 4095) && brace_at(t, 64, 63)) sigs.push_back(g), found = true;
    }
    CHECK(found, "no signature with a '{' on a tile's last byte\n");
    for (unsigned phase : {0u, 1u, 7u}) run_writer(sigs, bs, phase, rng);

    std::vector<PCase> cases;
    for (size_t f = 0; f < sigs.size(); ++f) cases.push_back(PCase{"sig-" + std::to_string(f), text_alone(sigs[f], bs), 0, &sigs[f]});
    run_orders(cases, bs, rng, "good");
    run_refusals(bs, rng);
}

}  // namespace

int main(int argc, char** argv) {
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    run_all(4096, seed);
    run_all(1007, seed);
    // the host refusals of the plans
    {
        std::vector<sigb::WFile> wf;
        std::vector<sigb::PFile> pf;
        std::vector<uint64_t> lo, hi;
        uint64_t a = 0, b = 0;
        sigb::PlanErr e;
        const uint64_t nb[2] = {3, 2}, l0[2] = {5, 0}, l1[2] = {5, 4097};
        CHECK(sigb::wplan(true, nb, l0, 2, 4096, &wf, &lo, &hi, &a, &b, &e) == SYDELTA_E_INVAL && e.msg.find("file 1: last_size 0") == 0,
              "last_size 0: %s\n", e.msg.c_str());
        CHECK(sigb::wplan(true, nb, l1, 2, 4096, &wf, &lo, &hi, &a, &b, &e) == SYDELTA_E_INVAL && e.msg.find("file 1: last_size 4097") == 0,
              "last_size bs + 1: %s\n", e.msg.c_str());
        const uint64_t to[2] = {0, 90}, tl[2] = {10, 11};
        CHECK(sigb::pplan(true, 100, to, tl, 2, 4096, &pf, &a, &b, &e) == SYDELTA_E_INVAL &&
                  e.msg == "file 1: text [90, +11) leaves its arena of 100 bytes", "arena: %s\n", e.msg.c_str());
    }
    if (g_fails) {
        printf("sig_batch_check: %d failures\n", g_fails);
        return 1;
    }
    printf("sig_batch_check ok\n");
    return 0;
}
