// Stand-alone hardening program of the JPEG decoder's entropy core (ccedit_amd/csrc/jpegdec_core.h): the SAME text the kernel compiles,
// built here with the host compiler and -fsanitize=address,undefined and run directly (tests/test_jpegdec.py writes the case file,
// builds and runs it; it is never loaded into Python).
//
//   jpegdec_harden CASES
//
// CASES (little endian): "JDH1", int32 number of cases; per case
//   int32 ncomp, int32 luma_blocks, int64 mcus_frame, int64 mcus_interval, int64 n_intervals, int64 data_bytes, int32 has_coef,
//   int32 tables[kTabSize], uint8 data[data_bytes], int64 intervals[n_intervals][2], int32 status[n_intervals],
//   has_coef: int16 coef[mcus_frame * blocks_per_mcu * 64]
// Every interval's bytes are copied into a heap block of exactly their length, so that a read past the interval's end is a sanitizer
// report, and decoded into a zeroed buffer of exactly its blocks.  Each status must be a defined one and equal the expected word; the
// coefficients, where given, must equal the dump.  Exit 0: all cases as expected (and, by running to the end, no report).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../ccedit_amd/csrc/jpegdec_core.h"

static bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s CASES\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    char magic[4];
    int32_t n_cases = 0;
    if (!f || !rd(f, magic, 4) || memcmp(magic, "JDH1", 4) != 0 || !rd(f, &n_cases, 4)) {
        fprintf(stderr, "%s: not a case file\n", argv[1]);
        return 2;
    }
    long bad = 0, intervals_run = 0, stopped = 0;
    for (int32_t c = 0; c < n_cases; ++c) {
        int32_t ncomp, luma, has_coef;
        int64_t mcus_frame, mcus_interval, n_iv, data_bytes;
        if (!rd(f, &ncomp, 4) || !rd(f, &luma, 4) || !rd(f, &mcus_frame, 8) || !rd(f, &mcus_interval, 8) || !rd(f, &n_iv, 8) ||
            !rd(f, &data_bytes, 8) || !rd(f, &has_coef, 4)) {
            fprintf(stderr, "case %d: truncated case file\n", c);
            return 2;
        }
        std::vector<int32_t> tab(jpegdec::kTabSize);
        std::vector<uint8_t> data((size_t)data_bytes);
        std::vector<int64_t> iv((size_t)n_iv * 2);
        std::vector<int32_t> want((size_t)n_iv);
        const int bpm = ncomp == 1 ? 1 : luma + 2;
        std::vector<int16_t> want_coef(has_coef ? (size_t)(mcus_frame * bpm * 64) : 0);
        if (!rd(f, tab.data(), tab.size() * 4) || !rd(f, data.data(), data.size()) || !rd(f, iv.data(), iv.size() * 8) ||
            !rd(f, want.data(), want.size() * 4) || !rd(f, want_coef.data(), want_coef.size() * 2)) {
            fprintf(stderr, "case %d: truncated case file\n", c);
            return 2;
        }
        for (int64_t i = 0; i < n_iv; ++i) {
            const int64_t lo = iv[2 * i], hi = iv[2 * i + 1];
            const int64_t first = i * mcus_interval;
            if (lo < 0 || hi < lo || hi > data_bytes || first >= mcus_frame) {
                fprintf(stderr, "case %d interval %lld: bad case file\n", c, (long long)i);
                return 2;
            }
            const int64_t n = mcus_frame - first < mcus_interval ? mcus_frame - first : mcus_interval;
            uint8_t* seg = (uint8_t*)malloc((size_t)(hi - lo) ? (size_t)(hi - lo) : 1);      // exactly the interval: reads past it are reports
            int16_t* coef = (int16_t*)calloc((size_t)(n * bpm * 64), sizeof(int16_t));
            if (hi > lo) memcpy(seg, data.data() + lo, (size_t)(hi - lo));
            const int32_t st = jpegdec::decode_interval(seg, 0, hi - lo, tab.data(), ncomp, luma, n, coef);
            ++intervals_run;
            stopped += st != 0;
            if (st < 0 || st > 4 || st != want[(size_t)i]) {
                fprintf(stderr, "case %d interval %lld: status %d, expected %d\n", c, (long long)i, st, want[(size_t)i]);
                ++bad;
            }
            if (has_coef && memcmp(coef, want_coef.data() + first * bpm * 64, (size_t)(n * bpm * 64) * 2) != 0) {
                fprintf(stderr, "case %d interval %lld: coefficients differ from the dump\n", c, (long long)i);
                ++bad;
            }
            free(seg);
            free(coef);
        }
    }
    fclose(f);
    printf("%d cases, %ld intervals (%ld stopped with a status), %ld mismatches\n", n_cases, intervals_run, stopped, bad);
    return bad ? 1 : 0;
}
