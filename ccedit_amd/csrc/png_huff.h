// The serial parts of the PNG encoder's deflate blocks (png.hip; ccedit_amd/png.py) as plain C++: the greedy LZ77
// walk of a chunk, Huffman code lengths from a histogram with the repair that limits them to max_bits, canonical codes, the run-coded
// block header, a token's bits.  No intrinsics and nothing of HIP: the kernel and a host program (tests/png_huff_harden.cpp, built with the host's sanitizers) compile the
// SAME text, and tests/_png_numpy.py states the rules it follows.  Integer arithmetic only; ties are broken by symbol number.
//
// Bounded by construction: every histogram has at most kMaxSyms entries and every array here holds kMaxSyms; lengths are <= max_bits <=
// 15; the repair loop is counted; the header writer refuses words past kHeaderWords (the worst case fits: kHeaderMaxBits).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PNG_HD __host__ __device__
#else
#define PNG_HD
#endif

namespace pnghuff {

// ccedit_amd/png.py
constexpr int kLitSyms = 286, kDistSyms = 30, kClSyms = 19, kEob = 256, kMaxBits = 15, kClMaxBits = 7;
constexpr int kDistAt = 288, kHistWords = 320, kMaxSyms = 288;
constexpr int kChunk = 16384;                    // filtered bytes per chunk
constexpr int kHashBits = 12, kHashSize = 1 << kHashBits;
constexpr uint32_t kHashMul = 2654435761u;
constexpr uint16_t kEmpty = 0xffff;              // no position: positions are < kChunk
constexpr int kMinMatch = 3, kMaxMatch = 258;
constexpr uint32_t kTokenMatch = 0x80000000u;    // a token: a literal's byte, or kTokenMatch | (length - 3) << 16 | (distance - 1)
constexpr int kHeaderMaxBits = 3 + 5 + 5 + 4 + 3 * kClSyms + (kLitSyms + kDistSyms) * (kClMaxBits + 7);
constexpr int kHeaderWords = ((kHeaderMaxBits + 31) / 32 + 3) / 4 * 4;

struct Work {                     // scratch of one construction
    uint32_t w[kMaxSyms], iw[kMaxSyms];              // weights of the sorted leaves, of the internal nodes in creation order
    uint16_t order[kMaxSyms], leaf_parent[kMaxSyms], int_parent[kMaxSyms], depth[kMaxSyms];
};

// The used symbols sorted by (count, symbol) ascending -> work.order / work.w; returns how many are used.  Symbols lane, lane + nlanes,
// ... are placed by this caller (a wave shares the work; a host caller passes 0, 1): a symbol's place is the number of used symbols
// before it in that order.
PNG_HD inline int rank_symbols(const uint32_t* counts, int nsym, Work* k, int lane, int nlanes) {
    int n = 0;
    for (int t = 0; t < nsym; ++t) n += counts[t] != 0;
    for (int s = lane; s < nsym; s += nlanes) {
        const uint32_t c = counts[s];
        if (!c) continue;
        int r = 0;
        for (int t = 0; t < nsym; ++t) {
            const uint32_t ct = counts[t];
            r += (ct != 0 && (ct < c || (ct == c && t < s))) ? 1 : 0;
        }
        k->order[r] = (uint16_t)s;
        k->w[r] = c;
    }
    return n;
}

// work.order / work.w of n used symbols -> lengths[nsym] limited to max_bits; returns the depth of the unlimited Huffman tree.
PNG_HD inline int code_lengths(Work* k, int n, int nsym, int max_bits, uint8_t* lengths) {
    for (int s = 0; s < nsym; ++s) lengths[s] = 0;
    if (n <= 0) return 0;
    if (n == 1) {
        lengths[k->order[0]] = 1;
        return 1;
    }
    int li = 0, ii = 0;
    for (int made = 0; made < n - 1; ++made) {                                    // two queues: sorted leaves, internal nodes as they were made
        uint32_t total = 0;
        for (int j = 0; j < 2; ++j) {
            if (li < n && (ii >= made || k->w[li] < k->iw[ii])) {              // equal weights: the internal node first
                k->leaf_parent[li] = (uint16_t)made;
                total += k->w[li++];
            } else {
                k->int_parent[ii] = (uint16_t)made;
                total += k->iw[ii++];
            }
        }
        k->iw[made] = total;
    }
    k->depth[n - 2] = 0;                                                           // the root was made last
    for (int j = n - 3; j >= 0; --j) k->depth[j] = (uint16_t)(k->depth[k->int_parent[j]] + 1);
    int per[kMaxBits + 1] = {0};
    int unlimited = 0;
    for (int i = 0; i < n; ++i) {
        const int d = k->depth[k->leaf_parent[i]] + 1;
        unlimited = d > unlimited ? d : unlimited;
        ++per[d < max_bits ? d : max_bits];
    }
    uint32_t total = 0;                                                            // the Kraft sum in units of 2^-max_bits
    for (int l = 1; l <= max_bits; ++l) total += (uint32_t)per[l] << (max_bits - l);
    for (int it = 0; it < n && total > (1u << max_bits); ++it) {                    // every clamped leaf adds less than one unit: < n rounds
        --per[max_bits];
        for (int l = max_bits - 1; l > 0; --l)
            if (per[l]) {
                --per[l];
                per[l + 1] += 2;
                break;
            }
        --total;
    }
    int at = 0;
    for (int l = max_bits; l > 0; --l)
        for (int c = 0; c < per[l] && at < n; ++c) lengths[k->order[at++]] = (uint8_t)l;
    return unlimited;
}

// lengths -> table[s] = length << 16 | the canonical code with its bits reversed (a Huffman code is sent most significant bit first,
// the stream is filled from the least significant bit); 0 for an unused symbol.
PNG_HD inline void canonical_codes(const uint8_t* lengths, int nsym, int max_bits, uint32_t* table) {
    uint32_t per[kMaxBits + 2] = {0}, next[kMaxBits + 2] = {0};
    for (int s = 0; s < nsym; ++s) ++per[lengths[s] <= max_bits ? lengths[s] : 0];
    per[0] = 0;
    for (int l = 1; l <= max_bits; ++l) next[l] = (next[l - 1] + per[l - 1]) << 1;
    for (int s = 0; s < nsym; ++s) {
        const uint32_t l = lengths[s] <= max_bits ? lengths[s] : 0;
        if (!l) {
            table[s] = 0;
            continue;
        }
        const uint32_t c = next[l]++;
        uint32_t r = 0;
        for (uint32_t b = 0; b < l; ++b) r |= ((c >> b) & 1u) << (l - 1 - b);
        table[s] = l << 16 | r;
    }
}

struct BitWriter {                 // LSB first into 32-bit words; words past `cap` are dropped (cannot happen: see the callers' bounds)
    uint32_t* words;
    uint32_t cap;
    uint64_t acc = 0;
    uint32_t n = 0, wi = 0, bits = 0;
    PNG_HD BitWriter(uint32_t* w, uint32_t cap_words) : words(w), cap(cap_words) {}
    PNG_HD void put(uint32_t value, uint32_t width) {                               // width <= 16, n < 32
        acc |= (uint64_t)(value & ((1u << width) - 1u)) << n;
        n += width;
        bits += width;
        if (n >= 32u) {
            if (wi < cap) words[wi] = (uint32_t)acc;
            ++wi;
            acc >>= 32;
            n -= 32u;
        }
    }
    PNG_HD void finish() {
        if (n && wi < cap) words[wi] = (uint32_t)acc;
    }
};

PNG_HD inline int cl_order(int k) {
    constexpr uint8_t order[kClSyms] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    return order[k < kClSyms ? k : 0];
}

// The header of a dynamic-Huffman block from the two alphabets' lengths -> header_words[kHeaderWords] (every word written: zeros after
// the last bit); returns its bit count.  run_sym / run_val: scratch of kLitSyms + kDistSyms entries each.
PNG_HD inline int block_header(const uint8_t* lit_len, const uint8_t* dist_len, int final_block, Work* k, uint8_t* run_sym, uint8_t* run_val,
                               uint32_t* header_words) {
    int hlit = kEob + 1, hdist = 1;
    for (int s = kEob + 1; s < kLitSyms; ++s)
        if (lit_len[s]) hlit = s + 1;
    for (int s = 1; s < kDistSyms; ++s)
        if (dist_len[s]) hdist = s + 1;
    const int nseq = hlit + hdist;
    uint32_t cl_hist[kClSyms] = {0};
    int nrun = 0;
    for (int i = 0; i < nseq;) {
        const int v = i < hlit ? lit_len[i] : dist_len[i - hlit];
        int run = 1;
        while (i + run < nseq && (i + run < hlit ? lit_len[i + run] : dist_len[i + run - hlit]) == v) ++run;
        if (v == 0 && run >= 3) {
            const int r = run < 138 ? run : 138;
            run_sym[nrun] = r <= 10 ? 17 : 18;
            run_val[nrun++] = (uint8_t)(r <= 10 ? r - 3 : r - 11);
            i += r;
        } else if (v != 0 && run >= 4) {
            const int r = run - 1 < 6 ? run - 1 : 6;
            run_sym[nrun] = (uint8_t)v;
            run_val[nrun++] = 0;
            run_sym[nrun] = 16;
            run_val[nrun++] = (uint8_t)(r - 3);
            i += 1 + r;
        } else {
            run_sym[nrun] = (uint8_t)v;
            run_val[nrun++] = 0;
            i += 1;
        }
    }
    for (int j = 0; j < nrun; ++j) ++cl_hist[run_sym[j] < kClSyms ? run_sym[j] : 0];
    uint8_t cl_len[kClSyms];
    uint32_t cl_table[kClSyms];
    const int n = rank_symbols(cl_hist, kClSyms, k, 0, 1);
    code_lengths(k, n, kClSyms, kClMaxBits, cl_len);
    canonical_codes(cl_len, kClSyms, kClMaxBits, cl_table);
    int hclen = 4;
    for (int j = 4; j < kClSyms; ++j)
        if (cl_len[cl_order(j)]) hclen = j + 1;
    for (int j = 0; j < kHeaderWords; ++j) header_words[j] = 0;
    BitWriter out(header_words, kHeaderWords);
    out.put(final_block ? 1u : 0u, 1);
    out.put(2u, 2);
    out.put((uint32_t)(hlit - 257), 5);
    out.put((uint32_t)(hdist - 1), 5);
    out.put((uint32_t)(hclen - 4), 4);
    for (int j = 0; j < hclen; ++j) out.put(cl_len[cl_order(j)], 3);
    for (int j = 0; j < nrun; ++j) {
        const int s = run_sym[j] < kClSyms ? run_sym[j] : 0;
        out.put(cl_table[s] & 0xffffu, cl_table[s] >> 16);
        if (s == 16) out.put(run_val[j], 2);
        if (s == 17) out.put(run_val[j], 3);
        if (s == 18) out.put(run_val[j], 7);
    }
    out.finish();
    return (int)out.bits;
}

// length - 3 (0 ... 255) -> literal/length symbol, its extra bits and their value
PNG_HD inline void length_symbol(uint32_t l, uint32_t& sym, uint32_t& eb, uint32_t& ev) {
    if (l >= 255u) {
        sym = 285, eb = 0, ev = 0;
    } else if (l < 8u) {
        sym = 257 + l, eb = 0, ev = 0;
    } else {
        const uint32_t top = 31u - (uint32_t)__builtin_clz(l);                      // floor(log2 l) >= 3
        eb = top - 2;
        sym = 257 + 4 * eb + 4 + ((l >> eb) & 3u);
        ev = l & ((1u << eb) - 1u);
    }
}

// distance - 1 (0 ... 32767) -> distance symbol, its extra bits and their value
PNG_HD inline void dist_symbol(uint32_t d, uint32_t& sym, uint32_t& eb, uint32_t& ev) {
    d &= 32767u;
    if (d < 4u) {
        sym = d, eb = 0, ev = 0;
    } else {
        const uint32_t top = 31u - (uint32_t)__builtin_clz(d);                      // floor(log2 d) >= 2
        eb = top - 1;
        sym = 2 * eb + 2 + ((d >> eb) & 1u);
        ev = d & ((1u << eb) - 1u);
    }
}

PNG_HD inline uint32_t hash3(const uint8_t* b, int i) {
    return (((uint32_t)b[i] | (uint32_t)b[i + 1] << 8 | (uint32_t)b[i + 2] << 16) * kHashMul) >> (32 - kHashBits);
}

// The greedy walk of one chunk b[0 .. n), n <= kChunk: table[kHashSize] all kEmpty and hist[kHistWords] all zero on entry, out holds n
// words.  Returns the number of tokens (<= n).  Every read of b is at an index < n, every table entry a position < the current one.
PNG_HD inline int lz77_tokens(const uint8_t* b, int n, uint16_t* table, uint32_t* hist, uint32_t* out) {
    int nt = 0;
    for (int i = 0; i < n;) {
        int len = 0, cand = 0;
        if (i + 3 <= n) {
            const uint32_t k = hash3(b, i);
            cand = table[k];
            table[k] = (uint16_t)i;
            if (cand != kEmpty && cand < i) {                                       // (cand < i always: an earlier position of this chunk)
                const int top = n - i < kMaxMatch ? n - i : kMaxMatch;
                while (len < top && b[cand + len] == b[i + len]) ++len;
            }
        }
        if (len >= kMinMatch) {
            uint32_t sym, eb, ev;
            out[nt++] = kTokenMatch | (uint32_t)(len - 3) << 16 | (uint32_t)(i - cand - 1);
            length_symbol((uint32_t)(len - 3), sym, eb, ev);
            ++hist[sym];
            dist_symbol((uint32_t)(i - cand - 1), sym, eb, ev);
            ++hist[kDistAt + sym];
            const int end = i + len < n - 2 ? i + len : n - 2;
            for (int j = i + 1; j < end; ++j) table[hash3(b, j)] = (uint16_t)j;      // the positions inside the match that still have three bytes
            i += len;
        } else {
            out[nt++] = b[i];
            ++hist[b[i]];
            ++i;
        }
    }
    ++hist[kEob];
    return nt;
}

// One token's bits (LSB first, at most 15 + 5 + 15 + 13 = 48) under the code table of canonical_codes (literal/length at 0, distance at
// kDistAt); symbols are masked into their tables.
PNG_HD inline void token_bits(uint32_t t, const uint32_t* table, uint64_t& bits, uint32_t& nb) {
    if (t & kTokenMatch) {
        uint32_t sym, eb, ev;
        length_symbol((t >> 16) & 255u, sym, eb, ev);
        uint32_t e = table[sym];
        bits = e & 0xffffu, nb = e >> 16;
        bits |= (uint64_t)ev << nb, nb += eb;
        dist_symbol(t & 0xffffu, sym, eb, ev);
        e = table[kDistAt + sym];
        bits |= (uint64_t)(e & 0xffffu) << nb, nb += e >> 16;
        bits |= (uint64_t)ev << nb, nb += eb;
    } else {
        const uint32_t e = table[t & 255u];
        bits = e & 0xffffu, nb = e >> 16;
    }
}

PNG_HD inline uint32_t length_extra_bits(int sym) {                                // of literal/length symbol 257 ... 285
    const int k = sym - 257;
    return (k < 8 || k >= 28) ? 0u : (uint32_t)(k - 4) >> 2;
}

PNG_HD inline uint32_t dist_extra_bits(int sym) { return sym < 4 ? 0u : (uint32_t)(sym - 2) >> 1; }

}  // namespace pnghuff
