// zstd_ref.cpp — TEST INFRASTRUCTURE: the sequential host form of the device zstd
// encoder (sy_amd/csrc/sydelta_zstd.hpp: block_content_seq, the block code builder and
// header writers that k_zstd_block shares), built by tests/test_zstd.py.  The device
// output must equal this byte for byte, and libzstd's decoder must give the input back.
#include <stdint.h>
#include <string.h>

#include <memory>
#include <vector>

#include "sydelta_zstd.hpp"

using namespace sydelta::zstd;

// The frame for in[0, len) into out (cap >= frame_bound(len)); returns its size or 0.
extern "C" size_t zstd_ref_compress(const uint8_t* in, size_t len, uint8_t* out, size_t cap) {
    if (cap < frame_bound(len)) return 0;
    std::vector<uint8_t> slot(kBlockMax), lz(kSeqScratchBytes);
    const SeqScratch scratch = seq_scratch_at(lz.data(), 1, 0);
    frame_header(out, len);
    size_t o = kFrameHeader;
    const size_t nb = len ? (len + kBlockMax - 1) / kBlockMax : 1;
    for (size_t b = 0; b < nb; ++b) {
        const size_t p = b * kBlockMax;
        const uint32_t n = (uint32_t)(len - p < kBlockMax ? len - p : kBlockMax);
        uint32_t type = 0;
        const uint32_t size = n ? block_content_seq(in + p, n, slot.data(), scratch, &type) : 0;
        block_header(out + o, b + 1 == nb, type, type == 2 ? size : n);
        const uint8_t* src = type == 2 ? slot.data() : in + p;
        if (size) memcpy(out + o + 3, src, size);
        o += 3 + size;
    }
    return o;
}

// What the literals + sequences blocks of a text hold (tests/test_zstd_corpus.py): the forms
// that the device's parallel parse, repeat-history scan, literals section and sequence
// bitstream treat apart.  Counters in the order of tests/test_zstd_corpus.py SHAPE_NAMES; the
// kMax* ones keep the largest value, the others add up, so one array takes a whole corpus.
enum Shape : uint32_t {
    kBlocksWon, kSeqs, kMaxSeqsInBlock,
    kOv1Ll0, kOv2Ll0, kOv3Ll0, kOv1LlN, kOv2LlN, kOv3LlN,
    kMaxRepRun, kMaxRepRunBlockSeqs, kMaxRepRunOver64,
    kLl0AtRep0, kMaxMatch, kMatchOver512, kEndOn512, kLastEndsAtN,
    kLitRaw, kLitOne, kLitFour,
    kRleBlocks, kRleOver1, kRleOver64, kOneSeqBlocks, kDistOver4096, kDupHistoryTurns,
    kShapeCount
};

// Adds the shape of in[0, len) to c[0, kShapeCount); returns kShapeCount, 0 when nc differs.
// A block counts where its literals + sequences content is what the frame holds: the block
// is Compressed, lz_worth holds and lz_content, run again over the bests that
// block_content_seq left in the scratch, gives the slot's bytes.
extern "C" size_t zstd_ref_shape(const uint8_t* in, size_t len, uint64_t* c, size_t nc) {
    if (nc != kShapeCount) return 0;
    std::vector<uint8_t> slot(kBlockMax), lz(kSeqScratchBytes), lsec(kBlockMax + 8);
    std::vector<uint32_t> hh(256);
    std::unique_ptr<HufCode> code(new HufCode);
    std::unique_ptr<HufWork> work(new HufWork);
    const SeqScratch sc = seq_scratch_at(lz.data(), 1, 0);
    auto top = [&](uint32_t k, uint64_t v) { if (v > c[k]) c[k] = v; };
    for (size_t p0 = 0; p0 < len; p0 += kBlockMax) {
        const uint8_t* b = in + p0;
        const uint32_t n = (uint32_t)(len - p0 < kBlockMax ? len - p0 : kBlockMax);
        uint32_t type = 0;
        const uint32_t size = block_content_seq(b, n, slot.data(), sc, &type);
        if (type != 2) continue;
        uint32_t nbest = 0;
        for (uint32_t p = 0; p < n; ++p) nbest += sc.best[p] != 0;
        if (!lz_worth(nbest, n)) continue;
        uint32_t cand[kCands] = {0};  // greedy_parse does not read it
        const uint32_t z = lz_content(b, n, cand, sc, hh.data(), *code, *work);
        if (z != size || memcmp(sc.body, slot.data(), size) != 0) continue;
        uint32_t nl = 0, cov = 0;
        const uint32_t ns = greedy_parse(b, n, sc.best, cand, sc.seq, sc.lit, &nl, &cov);
        ++c[kBlocksWon];
        c[kSeqs] += ns;
        top(kMaxSeqsInBlock, ns);
        c[kOneSeqBlocks] += ns == 1;
        // the literals section's kind from its header, the table modes from the sequences header
        const uint32_t lt = slot[0] & 3u, sf = (slot[0] >> 2) & 3u;
        ++c[lt == 0 ? kLitRaw : sf == 0 ? kLitOne : kLitFour];
        const uint32_t lsz = lit_section_seq(sc.lit, nl, lsec.data(), sc.streams, hh.data(), *code, *work);
        const uint8_t modes = slot[lsz + (ns < 128 ? 1 : ns < 0x7F00 ? 2 : 3)];
        const bool rle = ((modes >> 6) & 3u) == 1 || ((modes >> 4) & 3u) == 1 || ((modes >> 2) & 3u) == 1;
        c[kRleBlocks] += rle;
        c[kRleOver1] += rle && ns > 1;
        c[kRleOver64] += rle && ns > 64;
        uint32_t rep[3] = {0, 0, 0}, pos = 0, run = 0, best_run = 0;
        uint32_t mtf[3] = {0, 0, 0};  // the three latest distinct distances, latest first
        for (uint32_t k = 0; k < ns; ++k) {
            const Seq& q = sc.seq[k];
            const uint32_t start = pos + q.ll, end = start + q.ml;
            const uint32_t ll0 = q.ll == 0;
            if (q.ov <= 3) ++c[(ll0 ? kOv1Ll0 : kOv1LlN) + q.ov - 1];
            run = q.off != (sc.best[start] & 0xFFFFFFu) ? run + 1 : 0;
            if (run > best_run) best_run = run;
            c[kLl0AtRep0] += ll0 && rep[0] && q.off == rep[0];
            top(kMaxMatch, q.ml);
            c[kMatchOver512] += q.ml > 512;
            c[kEndOn512] += end % 512 == 0 && end < n;
            c[kDistOver4096] += q.off >= 4096;
            {   // the Offset_Value differs when the history is taken as the three latest distinct
                // distances: a value stands twice in rep[] (after a literal length of 0 at rep[0])
                // and a later sequence reaches past it.  The device's wave scan assumes distinct
                // values, so only its sequential fallback codes these.
                uint32_t t0 = mtf[0], t1 = mtf[1], t2 = mtf[2];
                c[kDupHistoryTurns] += rep_code3(t0, t1, t2, q.ll, q.off) != q.ov;
                if (q.off == mtf[1]) { mtf[1] = mtf[0]; mtf[0] = q.off; }
                else if (q.off != mtf[0]) { mtf[2] = mtf[1]; mtf[1] = mtf[0]; mtf[0] = q.off; }
            }
            rep_code(rep, q.ll, q.off);
            pos = end;
        }
        c[kLastEndsAtN] += pos == n;
        if (best_run > c[kMaxRepRun]) { c[kMaxRepRun] = best_run; c[kMaxRepRunBlockSeqs] = ns; }
        if (ns > 64) top(kMaxRepRunOver64, best_run);
    }
    return kShapeCount;
}
