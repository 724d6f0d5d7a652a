// Stand-alone hardening program of the GIF decoder's core (ccedit_amd/csrc/gifdec_core.h): the SAME text the kernels compile, built here
// with the host compiler and -fsanitize=address,undefined and run directly (tests/_gifdec_cases.py writes the case file, builds and
// runs it; it is never loaded into Python).
//
//   gifdec_harden CASES RESULT
//
// CASES (little endian): "GDH1", int32 number of cases; per case
//   int32 min_code, int64 npix, int64 stream_bytes, int32 has_indices, uint8 stream[stream_bytes], has_indices: uint8 indices[npix]
// The stream is copied into a heap block of exactly its length, the code table has exactly the entries the host bound gives
// (min(npix, 8 * stream_bytes / (min_code + 1)) + 1) and the plane exactly npix bytes, so that any access outside them is a sanitizer
// report.  The table is built TWICE: by one lane, and by 64 emulated lanes that take their turns in descending order (a step must not
// depend on what another lane wrote in the same step); status, position, count and every table entry must agree.  On status 0 every
// code's pixels are written (codes in descending order: they are independent) and must equal indices where given; has_indices with a
// non-zero status is a mismatch.  Without indices any defined status will do.
// RESULT: one line "status position codes" per case.  Exit 0: all cases as expected (and, by running to the end, no report).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../ccedit_amd/csrc/gifdec_core.h"

using namespace gifdec;

static bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

template <int LANES>
struct Exec {
    template <class T>
    struct Var {
        T v[LANES];
        T& operator[](int l) { return v[l]; }
    };
    int lanes() const { return LANES; }
    int hi() const { return LANES - 1; }
    int lo() const { return 0; }
    uint64_t ballot(Var<int32_t>& p) const {
        uint64_t m = 0;
        for (int l = 0; l < LANES; ++l) m |= (uint64_t)(p.v[l] != 0) << l;
        return m;
    }
    void gather(Var<int32_t>& dst, Var<int32_t>& src, Var<int32_t>& idx) const {
        int32_t old[LANES];
        for (int l = 0; l < LANES; ++l) old[l] = src.v[l];
        for (int l = LANES - 1; l >= 0; --l) dst.v[l] = old[idx.v[l] & (LANES - 1)];
    }
    void scan(Var<int32_t>& dst, Var<int32_t>& src) const {
        int32_t sum = 0;
        for (int l = 0; l < LANES; ++l) {
            const int32_t x = src.v[l];
            dst.v[l] = sum;
            sum += x;
        }
    }
    template <class T>
    T get(Var<T>& p, int l) const { return p.v[l & (LANES - 1)]; }
    void sync() const {}
};

struct Table {
    int64_t cap;
    int32_t *parent, *len, *off;
    uint8_t *first, *last;
    explicit Table(int64_t n) : cap(n), parent(new int32_t[n]), len(new int32_t[n]), off(new int32_t[n]), first(new uint8_t[n]), last(new uint8_t[n]) {}
    ~Table() { delete[] parent, delete[] len, delete[] off, delete[] first, delete[] last; }
    Codes codes() const { return Codes{parent, len, off, first, last}; }
};

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s CASES RESULT\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    FILE* res = fopen(argv[2], "w");
    char magic[4];
    int32_t n_cases = 0;
    if (!f || !res || !rd(f, magic, 4) || memcmp(magic, "GDH1", 4) != 0 || !rd(f, &n_cases, 4)) {
        fprintf(stderr, "%s: not a case file (or %s cannot be written)\n", argv[1], argv[2]);
        return 2;
    }
    int mismatches = 0;
    for (int32_t i = 0; i < n_cases; ++i) {
        int32_t m = 0, has_indices = 0;
        int64_t npix = 0, n_in = 0;
        if (!rd(f, &m, 4) || !rd(f, &npix, 8) || !rd(f, &n_in, 8) || !rd(f, &has_indices, 4) || npix < 1 || n_in < 0) {
            fprintf(stderr, "case %d: bad header\n", i);
            return 2;
        }
        uint8_t* stream = new uint8_t[n_in];
        uint8_t* want = has_indices ? new uint8_t[npix] : nullptr;
        if (!rd(f, stream, (size_t)n_in) || (has_indices && !rd(f, want, (size_t)npix))) {
            fprintf(stderr, "case %d: short file\n", i);
            return 2;
        }
        const int64_t by_bits = 8 * n_in / ((m >= 2 && m <= 8 ? m : 8) + 1);
        const int64_t cap = (npix < by_bits ? npix : by_bits) + 1;
        Table one(cap), wave(cap);
        Exec<1> e1;
        Exec<64> e64;
        int64_t n1 = 0, n64 = 0, w1 = 0, w64 = 0;
        const int32_t s1 = build_codes(e1, stream, n_in, m, npix, cap, one.codes(), &n1, &w1);
        const int32_t s64 = build_codes(e64, stream, n_in, m, npix, cap, wave.codes(), &n64, &w64);
        bool ok = s1 == s64 && n1 == n64 && w1 == w64 && s1 >= 0 && s1 <= kBadMinCode && n1 >= 0 && n1 <= cap;
        for (int64_t k = 0; ok && k < n1; ++k)
            ok = one.parent[k] == wave.parent[k] && one.len[k] == wave.len[k] && one.off[k] == wave.off[k] && one.first[k] == wave.first[k] &&
                 one.last[k] == wave.last[k] && one.parent[k] >= -1 && one.parent[k] < k;
        if (ok && s1 == kOk) {
            uint8_t* plane = new uint8_t[npix];
            memset(plane, 0xff, (size_t)npix);
            for (int64_t k = n64 - 1; k >= 0; --k) write_code(wave.parent, wave.len, wave.off, wave.last, n64, k, plane, npix);
            if (has_indices) ok = memcmp(plane, want, (size_t)npix) == 0;
            delete[] plane;
        } else if (has_indices) {
            ok = false;
        }
        if (!ok) {
            ++mismatches;
            printf("case %d: MISMATCH one lane (%d, %lld, %lld) 64 lanes (%d, %lld, %lld)\n", i, s1, (long long)w1, (long long)n1, s64, (long long)w64,
                   (long long)n64);
        }
        fprintf(res, "%d %lld %lld\n", s1, (long long)w1, (long long)n1);
        delete[] stream;
        delete[] want;
    }
    fclose(f);
    fclose(res);
    printf("%d cases, %d mismatches\n", n_cases, mismatches);
    return mismatches ? 1 : 0;
}
