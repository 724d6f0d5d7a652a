// Stand-alone hardening program of the PNG decoder's core (ccedit_amd/csrc/pngdec_core.h): the SAME text the kernels compile, built here
// with the host compiler and -fsanitize=address,undefined and run directly (tests/_pngdec_cases.py writes the case file, builds and
// runs it; it is never loaded into Python).
//
//   pngdec_harden CASES RESULT
//
// CASES (little endian): "PDH1", int32 number of cases; per case
//   int32 H, int32 W, int64 stream_bytes (-1: no stream), int32 has_filtered, int32 has_rgb,
//   uint8 stream[stream_bytes], has_filtered: uint8 filtered[H * (1 + 3 W)], has_rgb: uint8 rgb[H * W * 3]
// With a stream: it is copied into a heap block of exactly its length and inflated into a heap block of exactly H * (1 + 3 W) bytes, so
// that any access outside either is a sanitizer report.  It is inflated TWICE: by one lane, and by 64 emulated lanes that take their
// turns in descending order (a match's bytes must not depend on the order of the lanes); status, position and bytes must agree.
// has_filtered: the status must be 0 and the bytes equal; else the stream must stop with a defined non-zero status.  On status 0 the
// rows are unfiltered, and must equal rgb where given.  Without a stream the given filtered bytes are unfiltered.
// RESULT: one line "status position" per case.  Exit 0: all cases as expected (and, by running to the end, no report).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../ccedit_amd/csrc/pngdec_core.h"

using namespace pngdec;

static bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

template <int LANES>
struct Exec {
    bool lead() const { return true; }
    int32_t share(int32_t v) const { return v; }
    void sync() const {}
    uint8_t byte(const uint8_t* data, int64_t pos, int64_t) const { return data[pos]; }
    void put(uint8_t* out, int64_t pos, uint8_t b) const { out[pos] = b; }
    void copy(uint8_t* out, int64_t pos, int d, int len) const {
        for (int lane = LANES - 1; lane >= 0; --lane) copy_match(out, pos, d, len, lane, LANES);
    }
    void copy_in(uint8_t* out, int64_t pos, const uint8_t* src, int n) const {
        for (int j = 0; j < n; ++j) out[pos + j] = src[j];
    }
    uint32_t adler(const uint8_t* p, int64_t n) const {
        uint32_t s1 = 0, s2 = 0;
        for (int lane = 0; lane < LANES; ++lane) {
            uint32_t a, b;
            adler_partial(p, n, lane, LANES, &a, &b);
            s1 += a, s2 += b;
        }
        return adler_finish(s1, s2, n);
    }
};

// The whole image, serially: a filter byte above 4 stops it with its offset.
static int32_t unfilter_image(const uint8_t* filtered, int H, int W, uint8_t* rgb, int64_t* where) {
    const int64_t rb = 1 + 3 * (int64_t)W, ob = 3 * (int64_t)W;
    for (int r = 0; r < H; ++r) {
        const int ft = filtered[r * rb];
        if (ft > 4) {
            *where = r * rb;
            return kBadFilter;
        }
        unfilter_row(ft, filtered + r * rb + 1, r ? rgb + (r - 1) * ob : nullptr, rgb + r * ob, ob);
    }
    *where = 0;
    return kOk;
}

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s CASES RESULT\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    FILE* res = fopen(argv[2], "w");
    char magic[4];
    int32_t n_cases = 0;
    if (!f || !res || !rd(f, magic, 4) || memcmp(magic, "PDH1", 4) != 0 || !rd(f, &n_cases, 4)) {
        fprintf(stderr, "%s: not a case file (or %s cannot be written)\n", argv[1], argv[2]);
        return 2;
    }
    long bad = 0, stopped = 0;
    {   // the closed forms of the core against RFC 1951's tables
        const int lb[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
        const int le[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
        const int db[30] = {1,   2,   3,   4,   5,   7,    9,    13,   17,   25,   33,   49,   65,    97,    129,
                            193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
        const int de[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
        for (int s = 0; s < 29; ++s) bad += length_base(s) != lb[s] || length_extra(s) != le[s];
        for (int s = 0; s < 30; ++s) bad += distance_base(s) != db[s] || distance_extra(s) != de[s];
        if (bad) fprintf(stderr, "the closed forms of the length / distance tables differ from RFC 1951's\n");
    }
    Work* wk = (Work*)malloc(sizeof(Work));
    for (int32_t c = 0; c < n_cases; ++c) {
        int32_t H, W, has_filtered, has_rgb;
        int64_t n_in;
        if (!rd(f, &H, 4) || !rd(f, &W, 4) || !rd(f, &n_in, 8) || !rd(f, &has_filtered, 4) || !rd(f, &has_rgb, 4) || H < 1 || W < 1) {
            fprintf(stderr, "case %d: truncated case file\n", c);
            return 2;
        }
        const int64_t L = (int64_t)H * (1 + 3 * (int64_t)W), R = (int64_t)H * W * 3;
        std::vector<uint8_t> stream((size_t)(n_in > 0 ? n_in : 0)), want(has_filtered ? (size_t)L : 0), want_rgb(has_rgb ? (size_t)R : 0);
        if (!rd(f, stream.data(), stream.size()) || !rd(f, want.data(), want.size()) || !rd(f, want_rgb.data(), want_rgb.size())) {
            fprintf(stderr, "case %d: truncated case file\n", c);
            return 2;
        }
        int32_t st = kOk;
        int64_t where = 0;
        uint8_t* filtered = (uint8_t*)malloc((size_t)L);
        if (n_in >= 0) {
            uint8_t* in = (uint8_t*)malloc(n_in ? (size_t)n_in : 1);              // exactly the stream: reads past it are reports
            uint8_t* again = (uint8_t*)malloc((size_t)L);
            if (n_in) memcpy(in, stream.data(), (size_t)n_in);
            memset(filtered, 0xA5, (size_t)L);
            memset(again, 0xA5, (size_t)L);
            Exec<1> one;
            Exec<64> wave;
            int64_t where2 = 0;
            st = inflate(one, in, n_in, filtered, L, *wk, &where);
            const int32_t st2 = inflate(wave, in, n_in, again, L, *wk, &where2);
            if (st != st2 || where != where2 || memcmp(filtered, again, (size_t)L) != 0) {
                fprintf(stderr, "case %d: one lane gives status %d at %lld, 64 lanes %d at %lld (or other bytes)\n", c, st, (long long)where, st2,
                        (long long)where2);
                ++bad;
            }
            if (st < 0 || st >= kStatusCount || st == kBadFilter || where < 0 || where > n_in) {
                fprintf(stderr, "case %d: status %d at %lld is not defined\n", c, st, (long long)where);
                ++bad;
            }
            if (has_filtered ? (st != kOk || memcmp(filtered, want.data(), (size_t)L) != 0) : st == kOk) {
                fprintf(stderr, "case %d: status %d at %lld, expected %s\n", c, st, (long long)where, has_filtered ? "0 and the reference's bytes" : "a stop");
                ++bad;
            }
            free(in);
            free(again);
        } else if (has_filtered) {
            memcpy(filtered, want.data(), (size_t)L);
        } else {
            fprintf(stderr, "case %d: neither a stream nor filtered bytes\n", c);
            return 2;
        }
        if (st == kOk) {
            uint8_t* rgb = (uint8_t*)malloc((size_t)R);
            st = unfilter_image(filtered, H, W, rgb, &where);
            if (has_rgb && (st != kOk || memcmp(rgb, want_rgb.data(), (size_t)R) != 0)) {
                fprintf(stderr, "case %d: the unfiltered rows differ from the reference (status %d)\n", c, st);
                ++bad;
            }
            free(rgb);
        }
        stopped += st != kOk;
        fprintf(res, "%d %lld\n", st, (long long)where);
        free(filtered);
    }
    free(wk);
    fclose(f);
    fclose(res);
    printf("%d cases (%ld stopped with a status), %ld mismatches\n", n_cases, stopped, bad);
    return bad ? 1 : 0;
}
