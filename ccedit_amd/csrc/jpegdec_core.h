// The entropy stage of the JPEG decoder (jpegdec.hip; ccedit_amd/jpegdec.py) as plain C++: the bit reader with
// FF 00 unstuffing, the Huffman lookup, the run / size expansion, EOB and ZRL, the DC prediction inside one restart interval.  No
// intrinsics and nothing of HIP: the kernel and a host program (tests/jpegdec_harden.cpp, built with the host's sanitizers) compile
// the SAME text, and tests/_jpegdec_numpy.py restates it.
//
// Safe on hostile input, by construction:
//   - a byte is read only at an address in [data + start, data + end): the reader checks before every read;
//   - a coefficient is written only at index natural[k] with k checked to be <= 63, into one of the n_mcus * blocks_per_mcu blocks
//     the caller gave the interval; the loops over MCUs and blocks are counted, nothing in the data can lengthen them;
//   - every table value that becomes an index is masked to its table (the table is device data the host cannot check per launch);
//   - every loop consumes input bits or counts a coefficient index up: there is no state in which it can spin.
// On an invalid code, on data that ends before the interval's blocks do (a marker inside the data ends it too) or on a coefficient
// index past 63 the interval STOPS and the status says why; its remaining coefficients stay as the caller zeroed them.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define JPEGDEC_HD __host__ __device__
#else
#define JPEGDEC_HD
#endif

namespace jpegdec {

// layout of the int32 table (ccedit_amd/jpegdec.py TAB_* / HUFF_*)
constexpr int kLutBits = 9;
constexpr int kHuffLut = 0, kHuffMaxcode = 512, kHuffValoff = 530, kHuffVals = 548, kHuffStride = 804;
constexpr int kTabQuant = 0, kTabSel = 192, kTabHuff = 200, kTabSize = 200 + 4 * kHuffStride;

enum Status : int32_t { kOk = 0, kBadCode = 1, kDataEnds = 2, kCoefIndex = 3, kBadDcSize = 4 };

// position in the scan -> row-major index
JPEGDEC_HD inline int natural_order(int k) {
    constexpr uint8_t zz[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return zz[k & 63];
}

// MSB-first bit reader over [p, end).  `n` counts the REAL bits held in the low end of `acc`; once the data has ended (its last byte,
// or an FF that is not followed by 00: a marker) peek pads with zeros and skip refuses to pass the last real bit.
struct BitReader {
    const uint8_t* p;
    const uint8_t* end;
    uint64_t acc;
    int n;

    JPEGDEC_HD inline void fill() {
        while (n <= 48 && p < end) {
            uint32_t b = *p;
            if (b == 0xFFu) {
                if (p + 1 < end && p[1] == 0u) {
                    p += 2;
                } else {
                    end = p;                    // a marker (or a lone FF at the end): the data ends here
                    break;
                }
            } else {
                ++p;
            }
            acc = (acc << 8) | b;
            n += 8;
        }
    }
    // the next 16 bits, zeros behind the last real one
    JPEGDEC_HD inline uint32_t peek16() {
        if (n < 16) fill();
        return n >= 16 ? (uint32_t)(acc >> (n - 16)) & 0xFFFFu : (uint32_t)(acc << (16 - n)) & 0xFFFFu;
    }
    JPEGDEC_HD inline bool skip(int k) {
        if (k > n) return false;
        n -= k;
        return true;
    }
};

// One Huffman symbol from table `t` (kHuffStride int32): codes of up to 9 bits by one lookup, longer ones by the Annex F.2.2.3 walk.
JPEGDEC_HD inline int32_t decode_symbol(BitReader& br, const int32_t* t, int* sym) {
    const uint32_t v = br.peek16();
    const uint32_t e = (uint32_t)t[kHuffLut + (v >> (16 - kLutBits))];
    int len = (int)((e >> 8) & 255u);
    if (len >= 1 && len <= kLutBits) {
        *sym = (int)(e & 255u);
    } else {
        len = 0;
        for (int l = kLutBits + 1; l <= 16; ++l) {
            const int32_t code = (int32_t)(v >> (16 - l));
            const int32_t mc = t[kHuffMaxcode + l];
            if (mc >= 0 && code <= mc) {
                *sym = t[kHuffVals + ((t[kHuffValoff + l] + code) & 255)] & 255;
                len = l;
                break;
            }
        }
        if (len == 0) return kBadCode;
    }
    return br.skip(len) ? kOk : kDataEnds;
}

// s (1 ... 15) more bits as the signed value of size category s (F.2.2.1 EXTEND)
JPEGDEC_HD inline bool receive_extend(BitReader& br, int s, int* value) {
    const int v = (int)(br.peek16() >> (16 - s));
    if (!br.skip(s)) return false;
    *value = v >= (1 << (s - 1)) ? v : v - (1 << s) + 1;
    return true;
}

// One restart interval: bytes [start, end) of `data` -> n_mcus * blocks_per_mcu blocks of 64 int16 at `coef` (zero on entry), natural
// order inside a block.  ncomp 1: one block per MCU; ncomp 3: luma_blocks of component 0, then one of component 1, one of component 2.
JPEGDEC_HD inline int32_t decode_interval(const uint8_t* data, int64_t start, int64_t end, const int32_t* tab, int ncomp, int luma_blocks,
                                          int64_t n_mcus, int16_t* coef) {
    BitReader br{data + start, data + end, 0, 0};
    int pred[3] = {0, 0, 0};
    const int bpm = ncomp == 1 ? 1 : luma_blocks + 2;
    for (int64_t m = 0; m < n_mcus; ++m) {
        for (int j = 0; j < bpm; ++j) {
            const int c = (ncomp == 1 || j < luma_blocks) ? 0 : j - luma_blocks + 1;
            const int32_t* dc = tab + kTabHuff + (tab[kTabSel + c] & 1) * kHuffStride;
            const int32_t* ac = tab + kTabHuff + (2 + (tab[kTabSel + 3 + c] & 1)) * kHuffStride;
            int16_t* out = coef + (m * bpm + j) * 64;
            int sym = 0, val = 0;
            if (int32_t st = decode_symbol(br, dc, &sym)) return st;
            if (sym > 11) return kBadDcSize;
            if (sym) {
                if (!receive_extend(br, sym, &val)) return kDataEnds;
            }
            pred[c] = (int)(int16_t)(uint16_t)((uint32_t)pred[c] + (uint32_t)val);           // (wraps at 16 bits: only hostile data gets there)
            out[0] = (int16_t)pred[c];
            int k = 1;
            while (k < 64) {
                if (int32_t st = decode_symbol(br, ac, &sym)) return st;
                const int r = sym >> 4, s = sym & 15;
                if (s == 0) {
                    if (r != 15) break;             // EOB
                    k += 16;                        // ZRL
                    continue;
                }
                k += r;
                if (k > 63) return kCoefIndex;
                if (!receive_extend(br, s, &val)) return kDataEnds;
                out[natural_order(k)] = (int16_t)val;
                ++k;
            }
        }
    }
    return kOk;
}

}  // namespace jpegdec
