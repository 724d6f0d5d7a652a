// The serial heart of the PNG decoder (pngdec.hip; ccedit_amd/pngdec.py) as plain C++: the LSB-first bit reader,
// the construction of a canonical Huffman code table from code lengths, the symbol decoder, the walk over a zlib stream's stored,
// fixed and dynamic blocks, Adler-32 by position weights, and the five PNG row filters undone.  No intrinsics and nothing of HIP: the
// kernels and a host program (tests/pngdec_harden.cpp, built with the host's sanitizers) compile the SAME text.
//
// Who executes it.  inflate() is written for a GROUP of lanes that all run it on the same stream and therefore hold the same state: the
// symbol walk is serial, but a match is copied by the whole group (copy_match: for distance < length lane j reads
// out[pos - d + (j mod d)], every source lies before pos, so the lanes are independent) and the checksum is summed by the whole group.
// What only ONE lane may do (a store to the tables, a literal's store) and what the group has to agree on goes through the executor E:
//   bool lead()                      this lane writes the shared tables
//   int32_t share(int32_t v)         the leader's v, in every lane
//   void sync()                      what the group wrote so far is visible to all of it
//   void put(out, pos, byte)         one literal
//   void copy(out, pos, d, len)      one match (pos - d >= 0 and pos + len <= n_out were checked)
//   void copy_in(out, pos, src, n)   a stored block's bytes
//   uint32_t adler(p, n)             Adler-32 of p[0, n)
//   uint8_t byte(data, pos, end)     the input byte data[pos], 0 <= pos < end (the kernel stages the input in LDS, 1 KiB at a time)
// The kernel's executor is a wave of 64 lanes; the host's is one lane, or 64 lanes emulated one after the other.
//
// Safe on hostile input, by construction:
//   - an input byte is read only at data[pos] with 0 <= pos < n_in: the reader checks before every read; behind the last byte it pads
//     with zeros and refuses to consume a bit that is not there;
//   - an output byte is written only at out[pos] with pos < n_out, and a match reads only out[pos - d ...] with d <= pos: both are
//     checked before the executor is asked to copy;
//   - code lengths are masked to 0 ... 15 where they index, the sorted-symbol index is clamped into its table, symbols that index the
//     base / extra tables are checked against 29 and 30 first, the count of code lengths is checked against HLIT + HDIST before a run is
//     written;
//   - every turn of every loop consumes at least one input bit or counts an index up: there is no state in which it can spin.
// Anything wrong STOPS the stream with a status and the input byte position; the output behind what was written so far stays as it was.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PNGDEC_HD __host__ __device__
#else
#define PNGDEC_HD
#endif

namespace pngdec {

// (ccedit_amd/pngdec.py STATUS_TEXT)
enum Status : int32_t {
    kOk = 0,
    kBadHeader = 1,     // zlib header: CM != 8, a window above 32 KiB, FDICT, or FCHECK wrong
    kInputEnds = 2,     // the stream runs past its input
    kBadBlockType = 3,  // BTYPE 3
    kStoredLength = 4,  // a stored block whose LEN and NLEN disagree
    kBadCode = 5,       // an over-subscribed or incomplete code, more than 286 / 30 symbols, or no end-of-block code
    kBadLengths = 6,    // a repeat without a previous length, or a run past HLIT + HDIST
    kBadSymbol = 7,     // bits that are no code, literal/length symbol 286 / 287, distance code 30 / 31
    kDistance = 8,      // a distance that reaches before the stream's start
    kOutputLong = 9,    // the output would pass the expected size
    kOutputShort = 10,  // the stream ends short of the expected size
    kAdler = 11,        // the trailing Adler-32 is not the output's
    kBadFilter = 12,    // a row's filter byte above 4 (unfilter)
    kStatusCount = 13
};

constexpr int kLutBits = 10, kMaxBits = 15;
constexpr int kLitLenSyms = 288, kDistSyms = 32, kClSyms = 19;
constexpr uint32_t kAdlerMod = 65521u;

// One code: codes of up to kLutBits bits by one lookup (entry = length << 9 | symbol, 0: longer or no code), longer ones by the
// canonical walk over count / symbol (symbols sorted by length, then by value).
struct Table {
    uint16_t lut[1 << kLutBits];
    uint16_t count[kMaxBits + 1];
    uint16_t symbol[kLitLenSyms];
};

struct Work {
    Table lit, dist;
    uint8_t lens[kLitLenSyms + kDistSyms];
    uint8_t cl[32];
};

// LSB-first bit reader over data[0, end).  `n` counts the REAL bits held in the low end of `acc`.
struct BitReader {
    const uint8_t* data;
    int64_t pos, end;
    uint64_t acc;
    int n;

    template <class E>
    PNGDEC_HD inline void fill(E& ex) {
        while (n <= 56 && pos < end) {
            acc |= (uint64_t)ex.byte(data, pos, end) << n;
            ++pos;
            n += 8;
        }
    }
    // the next k <= 16 bits, zeros behind the last real one
    template <class E>
    PNGDEC_HD inline uint32_t peek(E& ex, int k) {
        if (n < k) fill(ex);
        return (uint32_t)acc & ((1u << k) - 1u);
    }
    PNGDEC_HD inline bool skip(int k) {
        if (k > n) return false;
        acc >>= k;
        n -= k;
        return true;
    }
    template <class E>
    PNGDEC_HD inline bool bits(E& ex, int k, uint32_t* v) {
        *v = peek(ex, k);
        return skip(k);
    }
    // input bytes touched so far
    PNGDEC_HD inline int64_t byte_pos() const { return pos - (n >> 3); }
    // back to whole bytes: the rest of the current byte is dropped, whole bytes held in acc are handed back
    PNGDEC_HD inline void align() {
        pos -= n >> 3;
        acc = 0;
        n = 0;
    }
};

// Code lengths lens[0, n) (n <= 288) -> t.  Returns what is left of the code space: 0 a complete code, > 0 an incomplete one (the
// caller decides; `codes` and `longest` tell it whether this is the one-code case zlib accepts), < 0 an over-subscribed one (t is
// then not usable).
PNGDEC_HD inline int build_table(const uint8_t* lens, int n, Table& t, int* codes, int* longest) {
    uint16_t count[kMaxBits + 1], offs[kMaxBits + 1], next[kMaxBits + 1];
    for (int l = 0; l <= kMaxBits; ++l) count[l] = 0;
    for (int s = 0; s < n; ++s) ++count[lens[s] & 15];
    *codes = n - count[0];
    *longest = 0;
    int left = 1;
    for (int l = 1; l <= kMaxBits; ++l) {
        left <<= 1;
        left -= count[l];
        if (left < 0) return left;
        if (count[l]) *longest = l;
    }
    for (int i = 0; i < (1 << kLutBits); ++i) t.lut[i] = 0;
    t.count[0] = 0;
    offs[1] = 0;
    next[0] = next[1] = 0;
    for (int l = 1; l <= kMaxBits; ++l) t.count[l] = count[l];
    for (int l = 1; l < kMaxBits; ++l) {
        offs[l + 1] = (uint16_t)(offs[l] + count[l]);
        next[l + 1] = (uint16_t)((next[l] + count[l]) << 1);
    }
    for (int s = 0; s < n; ++s) {
        const int l = lens[s] & 15;
        if (l == 0) continue;
        const int at = offs[l]++;
        t.symbol[at < kLitLenSyms ? at : kLitLenSyms - 1] = (uint16_t)s;
        const uint32_t code = next[l]++;
        if (l <= kLutBits) {
            uint32_t rev = 0;
            for (int b = 0; b < l; ++b) rev |= ((code >> b) & 1u) << (l - 1 - b);
            for (uint32_t k = rev; k < (1u << kLutBits); k += 1u << l) t.lut[k] = (uint16_t)(l << 9 | s);
        }
    }
    return left;
}

// One symbol of code t.
template <class E>
PNGDEC_HD inline int32_t decode_symbol(E& ex, BitReader& br, const Table& t, int* sym) {
    const uint32_t v = br.peek(ex, kMaxBits);
    const uint32_t e = t.lut[v & ((1u << kLutBits) - 1u)];
    int len = (int)(e >> 9);
    if (len) {
        *sym = (int)(e & 511u);
    } else {
        int code = 0, first = 0, index = 0;
        for (int l = 1; l <= kMaxBits; ++l) {
            code |= (int)((v >> (l - 1)) & 1u);
            const int count = t.count[l];
            if (code - count < first) {
                const int at = index + (code - first);
                *sym = t.symbol[at < 0 ? 0 : (at < kLitLenSyms ? at : kLitLenSyms - 1)];
                len = l;
                break;
            }
            index += count;
            first += count;
            first <<= 1;
            code <<= 1;
        }
        if (len == 0) return kBadSymbol;
    }
    return br.skip(len) ? kOk : kInputEnds;
}

// Lane `lane` of `lanes` copies its bytes of a match of `len` bytes at distance d to out[pos ...]: every source lies before pos.
PNGDEC_HD inline void copy_match(uint8_t* out, int64_t pos, int d, int len, int lane, int lanes) {
    for (int j = lane; j < len; j += lanes) out[pos + j] = out[pos - d + (j < d ? j : j % d)];
}

// Adler-32 by position weights: s1 = 1 + sum b[i], s2 = n + sum (n - i) b[i].  A lane sums the bytes lane, lane + lanes, ...
PNGDEC_HD inline void adler_partial(const uint8_t* p, int64_t n, int lane, int lanes, uint32_t* s1, uint32_t* s2) {
    uint64_t a = 0, b = 0;                      // b <= (n / lanes + 1) * n * 255: below 2^64 for every n < 2^27 bytes
    for (int64_t i = lane; i < n; i += lanes) {
        a += p[i];
        b += (uint64_t)(n - i) * p[i];
    }
    *s1 = (uint32_t)(a % kAdlerMod);
    *s2 = (uint32_t)(b % kAdlerMod);
}

// (s1, s2: the lanes' partials, each below the modulus, summed over at most 65536 lanes)
PNGDEC_HD inline uint32_t adler_finish(uint32_t s1, uint32_t s2, int64_t n) {
    const uint32_t a = (1u + s1) % kAdlerMod;
    const uint32_t b = (uint32_t)(((uint64_t)(n % kAdlerMod) + s2) % kAdlerMod);
    return b << 16 | a;
}

// RFC 1951's tables of base values and extra bits in closed form (a table in memory would be a load on the path of every match):
// length symbol s = 0 ... 28 (the symbol - 257): 3 ... 10 without extra bits, then four symbols per extra bit, 258 for the last;
// distance symbol s = 0 ... 29: 1 ... 4 without extra bits, then two symbols per extra bit.  tests/test_pngdec.py holds them to the tables.
PNGDEC_HD inline int length_extra(int s) { return (s < 8 || s >= 28) ? 0 : (s - 4) >> 2; }
PNGDEC_HD inline int length_base(int s) { return s < 8 ? 3 + s : (s >= 28 ? 258 : 3 + ((4 + (s & 3)) << ((s - 4) >> 2))); }
PNGDEC_HD inline int distance_extra(int s) { return s < 4 ? 0 : (s >> 1) - 1; }
PNGDEC_HD inline int distance_base(int s) { return s < 4 ? 1 + s : 1 + ((2 + (s & 1)) << ((s >> 1) - 1)); }

template <class E>
PNGDEC_HD inline int32_t make_table(E& ex, const uint8_t* lens, int n, Table& t, bool one_code_ok) {
    int32_t st = kOk;
    if (ex.lead()) {
        int codes = 0, longest = 0;
        const int left = build_table(lens, n, t, &codes, &longest);
        if (left < 0) st = kBadCode;
        if (left > 0 && !(one_code_ok && (codes == 0 || (codes == 1 && longest == 1)))) st = kBadCode;
    }
    st = ex.share(st);
    ex.sync();
    return st;
}

// One zlib stream data[0, n_in) -> exactly n_out bytes at out.  Returns the status; *where: the input byte position that goes with it
// (kInputEnds: n_in; kAdler: where the trailer begins; kBadHeader: 0; else the bytes touched when the stream stopped).
template <class E>
PNGDEC_HD inline int32_t inflate(E& ex, const uint8_t* data, int64_t n_in, uint8_t* out, int64_t n_out, Work& wk, int64_t* where) {
    constexpr uint8_t cl_order[kClSyms] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
#define PNGDEC_STOP(code)            \
    do {                             \
        *where = (code) == kInputEnds ? n_in : br.byte_pos(); \
        return (code);               \
    } while (0)

    BitReader br{data, 0, n_in < 0 ? 0 : n_in, 0, 0};
    *where = 0;
    if (n_in < 2) PNGDEC_STOP(kInputEnds);
    {
        const uint32_t cmf = data[0], flg = data[1];
        if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) | flg) % 31u != 0u || (flg & 0x20u)) return kBadHeader;
        br.pos = 2;
    }
    int64_t opos = 0;
    bool fixed_built = false;
    for (uint32_t final = 0; !final;) {
        uint32_t type;
        if (!br.bits(ex, 1, &final) || !br.bits(ex, 2, &type)) PNGDEC_STOP(kInputEnds);
        if (type == 3) PNGDEC_STOP(kBadBlockType);
        if (type == 0) {
            br.skip(br.n & 7);
            uint32_t len, nlen;
            if (!br.bits(ex, 16, &len) || !br.bits(ex, 16, &nlen)) PNGDEC_STOP(kInputEnds);
            if ((len ^ 0xffffu) != nlen) PNGDEC_STOP(kStoredLength);
            br.align();
            if ((int64_t)len > br.end - br.pos) PNGDEC_STOP(kInputEnds);
            if ((int64_t)len > n_out - opos) PNGDEC_STOP(kOutputLong);
            ex.copy_in(out, opos, data + br.pos, (int)len);
            br.pos += len;
            opos += len;
            continue;
        }
        if (type == 1) {
            if (!fixed_built) {
                if (ex.lead()) {
                    for (int s = 0; s < kLitLenSyms; ++s) wk.lens[s] = (uint8_t)(s < 144 ? 8 : (s < 256 ? 9 : (s < 280 ? 7 : 8)));
                    for (int s = 0; s < kDistSyms; ++s) wk.lens[kLitLenSyms + s] = 5;
                }
                ex.sync();
                if (int32_t st = make_table(ex, wk.lens, kLitLenSyms, wk.lit, false)) PNGDEC_STOP(st);
                if (int32_t st = make_table(ex, wk.lens + kLitLenSyms, kDistSyms, wk.dist, false)) PNGDEC_STOP(st);
                fixed_built = true;
            }
        } else {
            fixed_built = false;
            uint32_t hlit, hdist, hclen;
            if (!br.bits(ex, 5, &hlit) || !br.bits(ex, 5, &hdist) || !br.bits(ex, 4, &hclen)) PNGDEC_STOP(kInputEnds);
            hlit += 257, hdist += 1, hclen += 4;
            if (hlit > 286 || hdist > 30) PNGDEC_STOP(kBadCode);
            for (int i = 0; i < kClSyms; ++i) {
                uint32_t v = 0;
                if (i < (int)hclen && !br.bits(ex, 3, &v)) PNGDEC_STOP(kInputEnds);
                if (ex.lead()) wk.cl[cl_order[i]] = (uint8_t)v;
            }
            ex.sync();
            if (int32_t st = make_table(ex, wk.cl, kClSyms, wk.lit, false)) PNGDEC_STOP(st);
            const int total = (int)(hlit + hdist);
            int i = 0, prev = 0, eob = 0;
            while (i < total) {
                int sym = 0;
                if (int32_t st = decode_symbol(ex, br, wk.lit, &sym)) PNGDEC_STOP(st);
                int rep = 1, val = sym;
                uint32_t extra;
                if (sym == 16) {
                    if (i == 0) PNGDEC_STOP(kBadLengths);
                    if (!br.bits(ex, 2, &extra)) PNGDEC_STOP(kInputEnds);
                    rep = 3 + (int)extra, val = prev;
                } else if (sym == 17) {
                    if (!br.bits(ex, 3, &extra)) PNGDEC_STOP(kInputEnds);
                    rep = 3 + (int)extra, val = 0;
                } else if (sym == 18) {
                    if (!br.bits(ex, 7, &extra)) PNGDEC_STOP(kInputEnds);
                    rep = 11 + (int)extra, val = 0;
                } else if (sym > 18) {
                    PNGDEC_STOP(kBadSymbol);
                }
                if (rep > total - i) PNGDEC_STOP(kBadLengths);
                if (i <= 256 && 256 < i + rep) eob = val;
                if (ex.lead())
                    for (int k = 0; k < rep; ++k) wk.lens[i + k] = (uint8_t)val;
                i += rep;
                prev = val;
            }
            ex.sync();
            if (eob == 0) PNGDEC_STOP(kBadCode);
            if (int32_t st = make_table(ex, wk.lens, (int)hlit, wk.lit, true)) PNGDEC_STOP(st);
            if (int32_t st = make_table(ex, wk.lens + hlit, (int)hdist, wk.dist, true)) PNGDEC_STOP(st);
        }
        for (;;) {
            int sym = 0;
            if (int32_t st = decode_symbol(ex, br, wk.lit, &sym)) PNGDEC_STOP(st);
            if (sym < 256) {
                if (opos >= n_out) PNGDEC_STOP(kOutputLong);
                ex.put(out, opos, (uint8_t)sym);
                ++opos;
                continue;
            }
            if (sym == 256) break;
            sym -= 257;
            if (sym >= 29) PNGDEC_STOP(kBadSymbol);
            uint32_t extra;
            if (!br.bits(ex, length_extra(sym), &extra)) PNGDEC_STOP(kInputEnds);
            const int len = length_base(sym) + (int)extra;
            int dsym = 0;
            if (int32_t st = decode_symbol(ex, br, wk.dist, &dsym)) PNGDEC_STOP(st);
            if (dsym >= 30) PNGDEC_STOP(kBadSymbol);
            if (!br.bits(ex, distance_extra(dsym), &extra)) PNGDEC_STOP(kInputEnds);
            const int d = distance_base(dsym) + (int)extra;
            if ((int64_t)d > opos) PNGDEC_STOP(kDistance);
            if ((int64_t)len > n_out - opos) PNGDEC_STOP(kOutputLong);
            ex.copy(out, opos, d, len);
            opos += len;
        }
    }
    if (opos != n_out) PNGDEC_STOP(kOutputShort);
    br.skip(br.n & 7);
    br.align();
    if (br.end - br.pos < 4) PNGDEC_STOP(kInputEnds);
    const uint32_t want = (uint32_t)data[br.pos] << 24 | (uint32_t)data[br.pos + 1] << 16 | (uint32_t)data[br.pos + 2] << 8 | data[br.pos + 3];
    ex.sync();
    if (ex.adler(out, n_out) != want) PNGDEC_STOP(kAdler);
    return kOk;
#undef PNGDEC_STOP
}

// ---- the row filters undone (PNG 1.2 section 6): x the filtered byte, a the byte 3 to the left, b the byte above, c above-left
PNGDEC_HD inline int paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

PNGDEC_HD inline uint8_t unfilter_byte(int ft, int x, int a, int b, int c) {
    const int pred = ft == 1 ? a : (ft == 2 ? b : (ft == 3 ? (a + b) >> 1 : (ft == 4 ? paeth(a, b, c) : 0)));
    return (uint8_t)((x + pred) & 255);
}

// One row, serially: in[0, n) the filtered bytes behind the filter byte ft <= 4, up the row above (nullptr: zeros), bpp = 3.
PNGDEC_HD inline void unfilter_row(int ft, const uint8_t* in, const uint8_t* up, uint8_t* out, int64_t n) {
    for (int64_t i = 0; i < n; ++i) {
        const int a = i >= 3 ? out[i - 3] : 0, b = up ? up[i] : 0, c = (up && i >= 3) ? up[i - 3] : 0;
        out[i] = unfilter_byte(ft, in[i], a, b, c);
    }
}

}  // namespace pngdec
