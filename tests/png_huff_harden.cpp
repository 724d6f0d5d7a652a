// Host program over ccedit_amd/csrc/png_huff.h, the plain C++ the PNG kernels run serially (the LZ77 walk of a chunk, Huffman code
// lengths with the repair to 15 / 7 bits, canonical codes, the run-coded block header, a token's bits).  Built by tests/test_png.py with
// -fsanitize=address,undefined; the cases and what tests/_png_numpy.py gives for them come in one file:
//   png_huff_harden CASES
// "PNH1", int32 count; per case int32 kind (0: a chunk's bytes, 1: histograms only), int32 final;
//   kind 0: int32 n, n bytes, int32 ntok, ntok uint32 tokens;
//   both:   uint32 hist[320], uint32 codes[320], int32 header_bits, uint32 header[144], int32 chunk_bits, int32 unlimited depth of the
//           literal/length tree and of the distance tree;
//   kind 0: int32 nbytes, the chunk's coded bytes (its bits zero-padded to a byte).
// Exit 0 and "<count> cases, 0 mismatches" when every word agrees.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../ccedit_amd/csrc/png_huff.h"

using namespace pnghuff;

static bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    char magic[4];
    int32_t count = 0;
    if (!rd(f, magic, 4) || memcmp(magic, "PNH1", 4) || !rd(f, &count, 4)) return 2;
    int bad = 0;
    for (int32_t c = 0; c < count; ++c) {
        int32_t kind, final_block, n = 0, ntok = 0;
        if (!rd(f, &kind, 4) || !rd(f, &final_block, 4)) return 2;
        std::vector<uint8_t> bytes;
        std::vector<uint32_t> want_tok;
        if (kind == 0) {
            if (!rd(f, &n, 4) || n < 1 || n > kChunk) return 2;
            bytes.resize(n);                                   // exactly n: a read past the chunk's end is a heap overflow the sanitizer sees
            if (!rd(f, bytes.data(), n) || !rd(f, &ntok, 4) || ntok < 1 || ntok > n) return 2;
            want_tok.resize(ntok);
            if (!rd(f, want_tok.data(), 4 * (size_t)ntok)) return 2;
        }
        std::vector<uint32_t> want_hist(kHistWords), want_codes(kHistWords), want_header(kHeaderWords);
        int32_t want_hbits, want_bits, want_unl[2], nbytes = 0;
        if (!rd(f, want_hist.data(), 4 * kHistWords) || !rd(f, want_codes.data(), 4 * kHistWords) || !rd(f, &want_hbits, 4) ||
            !rd(f, want_header.data(), 4 * kHeaderWords) || !rd(f, &want_bits, 4) || !rd(f, want_unl, 8))
            return 2;
        std::vector<uint8_t> want_bytes;
        if (kind == 0) {
            if (!rd(f, &nbytes, 4) || nbytes < 1) return 2;
            want_bytes.resize(nbytes);
            if (!rd(f, want_bytes.data(), nbytes)) return 2;
        }
        int miss = 0;
        std::vector<uint32_t> hist(kHistWords, 0), tok(n > 0 ? n : 1);
        if (kind == 0) {
            std::vector<uint16_t> table(kHashSize, kEmpty);
            const int got = lz77_tokens(bytes.data(), n, table.data(), hist.data(), tok.data());
            miss += got != ntok || memcmp(tok.data(), want_tok.data(), 4 * (size_t)ntok) != 0;
            miss += memcmp(hist.data(), want_hist.data(), 4 * kHistWords) != 0;
        } else {
            hist = want_hist;
        }
        std::vector<Work> work(1);
        std::vector<uint8_t> len(kHistWords, 0), run_sym(kLitSyms + kDistSyms), run_val(kLitSyms + kDistSyms);
        std::vector<uint32_t> codes(kHistWords, 0), header(kHeaderWords);
        int nl = rank_symbols(hist.data(), kLitSyms, work.data(), 0, 1);
        const int unl_lit = code_lengths(work.data(), nl, kLitSyms, kMaxBits, len.data());
        nl = rank_symbols(hist.data() + kDistAt, kDistSyms, work.data(), 0, 1);
        const int unl_dist = code_lengths(work.data(), nl, kDistSyms, kMaxBits, len.data() + kDistAt);
        canonical_codes(len.data(), kLitSyms, kMaxBits, codes.data());
        canonical_codes(len.data() + kDistAt, kDistSyms, kMaxBits, codes.data() + kDistAt);
        const int hbits = block_header(len.data(), len.data() + kDistAt, final_block, work.data(), run_sym.data(), run_val.data(), header.data());
        uint32_t bits = (uint32_t)hbits;
        for (int s = 0; s < kLitSyms; ++s) bits += hist[s] * (len[s] + (s > kEob ? length_extra_bits(s) : 0u));
        for (int s = 0; s < kDistSyms; ++s) bits += hist[kDistAt + s] * (len[kDistAt + s] + dist_extra_bits(s));
        miss += memcmp(codes.data(), want_codes.data(), 4 * kHistWords) != 0;
        miss += hbits != want_hbits || memcmp(header.data(), want_header.data(), 4 * kHeaderWords) != 0;
        miss += (int32_t)bits != want_bits || unl_lit != want_unl[0] || unl_dist != want_unl[1];
        if (kind == 0) {
            std::vector<uint8_t> out(((size_t)bits + 7) / 8 + 16, 0);
            size_t at = 0;
            auto put = [&](uint64_t v, uint32_t nb) {
                for (uint32_t b = 0; b < nb; ++b, ++at)
                    if ((v >> b) & 1u) out[at >> 3] |= (uint8_t)(1u << (at & 7));
            };
            for (int w = 0; w < kHeaderWords && (int)at < hbits; ++w) put(header[w], hbits - w * 32 < 32 ? hbits - w * 32 : 32);
            for (int t = 0; t <= ntok; ++t) {
                uint64_t v = codes[kEob] & 0xffffu;
                uint32_t nb = codes[kEob] >> 16;
                if (t < ntok) token_bits(tok[t], codes.data(), v, nb);
                put(v, nb);
            }
            miss += at != bits || (int32_t)((at + 7) / 8) != nbytes || memcmp(out.data(), want_bytes.data(), nbytes) != 0;
        }
        if (miss) {
            printf("case %d (kind %d): %d mismatches\n", c, kind, miss);
            ++bad;
        }
    }
    fclose(f);
    printf("%d cases, %d mismatches\n", count, bad);
    return bad ? 1 : 0;
}
