// PNG output (include/ccedit_hip.h, "PNG"; ccedit_amd/png.py; `--save_type png`): uint8 RGB frames on the device -> per frame the zlib
// stream of its filtered rows, coded as independent dynamic-Huffman deflate blocks of 16 KiB of filtered bytes (a deflate block may end
// anywhere and a match need not leave it: the trick of gif.hip's Clear codes and mjpeg.hip's restart intervals).
//   png_filter      ONE WAVE PER ROW: the five filters' costs (sum of min(v, 256 - v)) summed across the lanes, the cheapest (lowest
//                   number on a tie) applied in a second pass.  Filters read source pixels, so rows are independent.
//   png_tokens      ONE LANE PER CHUNK, two chunks per workgroup: the wave first copies the chunks' bytes into LDS, then the lane walks
//                   them greedily with a single-entry hash table of 4096 16-bit positions in LDS (no chains, no lazy evaluation) and
//                   writes one 32-bit token per literal or match; the histograms of the 286 + 30 symbols are kept in LDS and written
//                   out by the wave.
//   png_codes       ONE WAVE PER CHUNK: the used symbols are ranked by (count, symbol) across the lanes; lane 0 then runs the plain C++
//                   of png_huff.h (two-queue Huffman, the repair to 15 bits, canonical codes, the run-coded header with a code-length
//                   code of at most 7 bits); the wave writes the code table and sums the chunk's bit count.
//   png_emit        ONE WAVE PER CHUNK: 64 tokens at a time, each lane its token's bits (at most 48), a wave scan of the bit counts,
//                   the bits OR-ed into the chunk's zeroed slot.
//   png_pack_scan / png_pack   bitpack.h, shared with gif.hip, at this file's slot size.
//   png_adler       a wave per chunk: (sum d[k], sum (n - k) d[k]) mod 65521; then a thread per frame combines its chunks in order.
// Every byte equals tests/_png_numpy.py; integer arithmetic only.
//
// Nothing can overflow by construction: a chunk holds at most kChunk tokens and its token buffer holds that; a token costs at most 16
// bits per byte it covers and the slot holds header + 16 kChunk + 15 bits; positions in the hash table are < kChunk <= 0xffff.  Token
// words, histograms and bit lengths are device data when the later stages read them: symbols are masked into their tables, words
// outside a slot are dropped, lengths are clamped into the slot.  The argument checks live with the exported entry points in core.cpp.
#include "common.h"
#include "bitpack.h"
#include "png_huff.h"

namespace {

using namespace pnghuff;

constexpr int kThreads = 256;
constexpr int kTokChunks = 2;                    // chunks (= live lanes) per workgroup of the token stage: 2 x (16 + 8 + 1.25) KB of LDS
constexpr int kSlotWords = ((kHeaderMaxBits + 16 * kChunk + kMaxBits + 31) / 32 + 3) / 4 * 4;      // = png.py SLOT_BYTES / 4
constexpr int kSlotBits = kSlotWords * 32;
constexpr uint32_t kAdlerMod = 65521u;

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
}

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, 64);
        v += (uint64_t)hi << 32 | lo;
    }
    return v;
}

__device__ __forceinline__ int paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__device__ __forceinline__ uint32_t cost_of(int v) {
    v &= 255;
    return (uint32_t)(v < 256 - v ? v : 256 - v);
}

// ---- filter: a wave per row, four rows per workgroup
__global__ __launch_bounds__(kThreads) void png_filter_kernel(const uint8_t* __restrict__ frames, uint8_t* __restrict__ filtered, int H, int W, int64_t rows) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (row >= rows) return;                                                       // (whole waves leave together)
    const int R = 3 * W;
    const int y = (int)(row % H);
    const uint8_t* cur = frames + row * R;
    const uint8_t* up = cur - R;                                                     // read only when y > 0
    uint32_t sum[5] = {0, 0, 0, 0, 0};
    for (int i = lane; i < R; i += 64) {
        const int x = cur[i], a = i >= 3 ? cur[i - 3] : 0, b = y ? up[i] : 0, c = (y && i >= 3) ? up[i - 3] : 0;
        sum[0] += cost_of(x);
        sum[1] += cost_of(x - a);
        sum[2] += cost_of(x - b);
        sum[3] += cost_of(x - ((a + b) >> 1));
        sum[4] += cost_of(x - paeth(a, b, c));
    }
    int t = 0;
    uint32_t best = wave_sum_u32(sum[0]);
#pragma unroll
    for (int k = 1; k < 5; ++k) {
        const uint32_t s = wave_sum_u32(sum[k]);
        if (s < best) best = s, t = k;                                               // a tie keeps the lower filter number
    }
    uint8_t* dst = filtered + row * (R + 1);
    if (lane == 0) dst[0] = (uint8_t)t;
    for (int i = lane; i < R; i += 64) {
        const int x = cur[i], a = i >= 3 ? cur[i - 3] : 0, b = y ? up[i] : 0, c = (y && i >= 3) ? up[i - 3] : 0;
        const int pred = t == 0 ? 0 : (t == 1 ? a : (t == 2 ? b : (t == 3 ? (a + b) >> 1 : paeth(a, b, c))));
        dst[1 + i] = (uint8_t)(x - pred);
    }
}

// ---- tokens: a lane per chunk (the walk itself: png_huff.h lz77_tokens)
__global__ __launch_bounds__(64) void png_tokens_kernel(const uint8_t* __restrict__ filtered, uint32_t* __restrict__ tokens, int32_t* __restrict__ ntok,
                                                        uint32_t* __restrict__ hist, int64_t L, int C, int64_t total) {
    __shared__ uint8_t s_bytes[kTokChunks][kChunk];
    __shared__ uint16_t s_hash[kTokChunks][kHashSize];
    __shared__ uint32_t s_hist[kTokChunks][kHistWords];
    const int lane = threadIdx.x;
    const int64_t id0 = (int64_t)blockIdx.x * kTokChunks;
    for (int i = lane; i < kTokChunks * kHashSize; i += 64) (&s_hash[0][0])[i] = kEmpty;
    for (int i = lane; i < kTokChunks * kHistWords; i += 64) (&s_hist[0][0])[i] = 0;
    for (int q = 0; q < kTokChunks; ++q) {
        const int64_t id = id0 + q;
        if (id >= total) break;
        const int64_t f = id / C, p0 = (id - f * C) * kChunk;
        const int n = (int)(L - p0 < kChunk ? L - p0 : kChunk);
        const uint8_t* src = filtered + f * L + p0;
        for (int i = lane; i < n; i += 64) s_bytes[q][i] = src[i];
    }
    __syncthreads();
    const int64_t id = id0 + lane;
    if (lane < kTokChunks && id < total) {
        const int64_t f = id / C, p0 = (id - f * C) * kChunk;
        const int n = (int)(L - p0 < kChunk ? L - p0 : kChunk);
        ntok[id] = lz77_tokens(s_bytes[lane], n, s_hash[lane], s_hist[lane], tokens + id * kChunk);
    }
    __syncthreads();
    for (int q = 0; q < kTokChunks && id0 + q < total; ++q)
        for (int i = lane; i < kHistWords; i += 64) hist[(id0 + q) * kHistWords + i] = s_hist[q][i];
}

// ---- codes: a wave per chunk
__global__ __launch_bounds__(64) void png_codes_kernel(const uint32_t* __restrict__ hist, uint32_t* __restrict__ codes, uint32_t* __restrict__ header,
                                                       int32_t* __restrict__ header_bits, int32_t* __restrict__ chunk_bits, int C) {
    __shared__ uint32_t s_count[kHistWords], s_table[kHistWords], s_header[kHeaderWords];
    __shared__ uint8_t s_len[kHistWords], s_run_sym[kHistWords], s_run_val[kHistWords];
    __shared__ Work s_work;
    __shared__ int s_hbits;
    const int lane = threadIdx.x;
    const int64_t id = blockIdx.x;
    for (int i = lane; i < kHistWords; i += 64) {
        const bool real = i < kLitSyms || (i >= kDistAt && i < kDistAt + kDistSyms);
        s_count[i] = real ? hist[id * kHistWords + i] : 0u;
        s_table[i] = 0;
        s_len[i] = 0;
    }
    __syncthreads();
    const int n_lit = rank_symbols(s_count, kLitSyms, &s_work, lane, 64);
    __syncthreads();
    if (lane == 0) code_lengths(&s_work, n_lit, kLitSyms, kMaxBits, s_len);
    __syncthreads();
    const int n_dist = rank_symbols(s_count + kDistAt, kDistSyms, &s_work, lane, 64);
    __syncthreads();
    if (lane == 0) {
        code_lengths(&s_work, n_dist, kDistSyms, kMaxBits, s_len + kDistAt);
        canonical_codes(s_len, kLitSyms, kMaxBits, s_table);
        canonical_codes(s_len + kDistAt, kDistSyms, kMaxBits, s_table + kDistAt);
        s_hbits = block_header(s_len, s_len + kDistAt, (int)(id % C) == C - 1, &s_work, s_run_sym, s_run_val, s_header);
    }
    __syncthreads();
    uint32_t bits = 0;
    for (int i = lane; i < kHistWords; i += 64) {
        codes[id * kHistWords + i] = s_table[i];
        if (i < kLitSyms) bits += s_count[i] * (s_len[i] + (i > kEob ? length_extra_bits(i) : 0u));
        if (i >= kDistAt && i < kDistAt + kDistSyms) bits += s_count[i] * (s_len[i] + dist_extra_bits(i - kDistAt));
    }
    for (int i = lane; i < kHeaderWords; i += 64) header[id * kHeaderWords + i] = s_header[i];
    bits = wave_sum_u32(bits);
    if (lane == 0) {
        header_bits[id] = s_hbits;
        chunk_bits[id] = (int32_t)(bits + (uint32_t)s_hbits < (uint32_t)kSlotBits ? bits + (uint32_t)s_hbits : (uint32_t)kSlotBits);
    }
}

// ---- emit: a wave per chunk, 64 tokens at a time
__device__ __forceinline__ void or_bits(uint32_t* __restrict__ slot, uint32_t off, uint64_t bits, uint32_t nb) {
    if (!nb) return;
    const uint32_t w = off >> 5, sh = off & 31u;
    const uint64_t lo = bits << sh;
    const uint32_t hi = sh ? (uint32_t)(bits >> (64u - sh)) : 0u;
    if ((uint32_t)lo && w < (uint32_t)kSlotWords) atomicOr(slot + w, (uint32_t)lo);
    if ((uint32_t)(lo >> 32) && w + 1 < (uint32_t)kSlotWords) atomicOr(slot + w + 1, (uint32_t)(lo >> 32));
    if (hi && w + 2 < (uint32_t)kSlotWords) atomicOr(slot + w + 2, hi);
}

__global__ __launch_bounds__(64) void png_emit_kernel(const uint32_t* __restrict__ tokens, const int32_t* __restrict__ ntok, const uint32_t* __restrict__ codes,
                                                      const uint32_t* __restrict__ header, const int32_t* __restrict__ header_bits,
                                                      uint32_t* __restrict__ slots) {
    __shared__ uint32_t s_table[kHistWords];
    const int lane = threadIdx.x;
    const int64_t id = blockIdx.x;
    uint32_t* slot = slots + id * kSlotWords;                                       // zeroed by the launcher
    for (int i = lane; i < kHistWords; i += 64) s_table[i] = codes[id * kHistWords + i];
    const int hb = cc_clampi(header_bits[id], 0, kHeaderMaxBits);
    const int nt = cc_clampi(ntok[id], 0, kChunk);
    for (int i = lane; i < (hb + 31) >> 5; i += 64) {
        const uint32_t keep = (i == (hb >> 5)) ? (1u << (hb & 31)) - 1u : 0xffffffffu;     // only the header's own bits of its last word
        const uint32_t v = header[id * kHeaderWords + i] & keep;
        if (v) atomicOr(slot + i, v);
    }
    __syncthreads();
    const uint32_t* tok = tokens + id * kChunk;
    uint32_t base = (uint32_t)hb;
    for (int t0 = 0; t0 <= nt; t0 += 64) {                                           // token nt is end-of-block
        const int idx = t0 + lane;
        uint64_t bits = 0;
        uint32_t nb = 0;
        if (idx < nt)
            token_bits(tok[idx], s_table, bits, nb);
        else if (idx == nt)
            bits = s_table[kEob] & 0xffffu, nb = s_table[kEob] >> 16;
        nb = nb < 48u ? nb : 48u;                                                    // (15 + 5 + 15 + 13: cannot be more)
        uint32_t incl = nb;                                                          // inclusive scan of the bit counts across the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t v = (uint32_t)__shfl_up((int)incl, o, 64);
            if (lane >= o) incl += v;
        }
        or_bits(slot, base + incl - nb, bits, nb);
        base += (uint32_t)__shfl((int)incl, 63, 64);
    }
}

__global__ __launch_bounds__(kThreads) void png_pack_scan_kernel(const int32_t* __restrict__ chunk_bits, int64_t* __restrict__ chunk_off,
                                                                 int32_t* __restrict__ frame_bytes, int C) {
    cc_pack_scan<kThreads, kSlotBits>(chunk_bits, chunk_off, frame_bytes, C);
}

__global__ __launch_bounds__(kThreads) void png_pack_kernel(const uint32_t* __restrict__ slots, const int32_t* __restrict__ chunk_bits,
                                                            const int64_t* __restrict__ chunk_off, uint32_t* __restrict__ out, int64_t out_bits) {
    cc_pack_chunk<kThreads, kSlotWords>(slots, chunk_bits, chunk_off, out, out_bits);
}

// ---- Adler-32: a wave per chunk, then a thread per frame
__global__ __launch_bounds__(64) void png_adler_chunk_kernel(const uint8_t* __restrict__ filtered, uint32_t* __restrict__ partials, int64_t L, int C) {
    const int lane = threadIdx.x;
    const int64_t id = blockIdx.x;
    const int64_t f = id / C, p0 = (id - f * C) * kChunk;
    const int n = (int)(L - p0 < kChunk ? L - p0 : kChunk);
    const uint8_t* src = filtered + f * L + p0;
    uint64_t a = 0, b = 0;
    for (int k = lane; k < n; k += 64) {
        const uint32_t d = src[k];
        a += d;
        b += (uint64_t)(uint32_t)(n - k) * d;
    }
    a = wave_sum_u64(a);
    b = wave_sum_u64(b);
    if (lane == 0) {
        partials[id * 2] = (uint32_t)(a % kAdlerMod);
        partials[id * 2 + 1] = (uint32_t)(b % kAdlerMod);
    }
}

__global__ __launch_bounds__(kThreads) void png_adler_frame_kernel(const uint32_t* __restrict__ partials, uint32_t* __restrict__ adler, int64_t L, int C,
                                                                   int N) {
    const int f = blockIdx.x * kThreads + threadIdx.x;
    if (f >= N) return;
    uint64_t s1 = 1, s2 = 0;
    for (int c = 0; c < C; ++c) {
        const int64_t p0 = (int64_t)c * kChunk;
        const uint64_t n = (uint64_t)(L - p0 < kChunk ? L - p0 : kChunk);
        const int64_t id = (int64_t)f * C + c;
        s2 = (s2 + n * s1 + partials[id * 2 + 1] % kAdlerMod) % kAdlerMod;
        s1 = (s1 + partials[id * 2] % kAdlerMod) % kAdlerMod;
    }
    adler[f] = (uint32_t)(s2 << 16 | s1);
}

}  // namespace

// ------------------------------------------------------------------------------------------
// launchers (arguments validated by the entry points in core.cpp)
// ------------------------------------------------------------------------------------------
int64_t cc_png_slot_bytes() { return (int64_t)kSlotWords * 4; }
int64_t cc_png_chunk_bytes() { return kChunk; }

int cc_png_filter(const uint8_t* frames, uint8_t* filtered, int32_t N, int32_t H, int32_t W, hipStream_t s) {
    const int64_t rows = (int64_t)N * H;
    hipLaunchKernelGGL(png_filter_kernel, dim3((unsigned)((rows + kThreads / 64 - 1) / (kThreads / 64))), dim3(kThreads), 0, s, frames, filtered, (int)H,
                       (int)W, rows);
    return cc_launch_status("png_filter");
}

int cc_png_tokens(const uint8_t* filtered, uint32_t* tokens, int32_t* ntok, uint32_t* hist, int32_t N, int64_t L, hipStream_t s) {
    const int64_t C = (L + kChunk - 1) / kChunk, total = (int64_t)N * C;
    hipLaunchKernelGGL(png_tokens_kernel, dim3((unsigned)((total + kTokChunks - 1) / kTokChunks)), dim3(64), 0, s, filtered, tokens, ntok, hist, L, (int)C,
                       total);
    return cc_launch_status("png_tokens");
}

int cc_png_codes(const uint32_t* hist, uint32_t* codes, uint32_t* header, int32_t* header_bits, int32_t* chunk_bits, int32_t N, int32_t C, hipStream_t s) {
    hipLaunchKernelGGL(png_codes_kernel, dim3((unsigned)((int64_t)N * C)), dim3(64), 0, s, hist, codes, header, header_bits, chunk_bits, (int)C);
    return cc_launch_status("png_codes");
}

int cc_png_emit(const uint32_t* tokens, const int32_t* ntok, const uint32_t* codes, const uint32_t* header, const int32_t* header_bits, uint8_t* slots,
                int64_t total, hipStream_t s) {
    hipError_t e = hipMemsetAsync(slots, 0, (size_t)total * kSlotWords * 4, s);
    if (e != hipSuccess) {
        cc_set_error("png_emit: hipMemsetAsync: %s", hipGetErrorString(e));
        return (int)e;
    }
    hipLaunchKernelGGL(png_emit_kernel, dim3((unsigned)total), dim3(64), 0, s, tokens, ntok, codes, header, header_bits, (uint32_t*)slots);
    return cc_launch_status("png_emit");
}

int cc_png_pack_scan(const int32_t* chunk_bits, int64_t* chunk_off, int32_t* frame_bytes, int32_t N, int32_t C, hipStream_t s) {
    hipLaunchKernelGGL(png_pack_scan_kernel, dim3((unsigned)N), dim3(kThreads), 0, s, chunk_bits, chunk_off, frame_bytes, (int)C);
    return cc_launch_status("png_pack_scan");
}

int cc_png_pack(const uint8_t* slots, const int32_t* chunk_bits, const int64_t* chunk_off, uint8_t* out, int32_t N, int32_t C, int64_t out_bytes,
                hipStream_t s) {
    const int64_t words = (out_bytes + 3) / 4;
    hipError_t e = hipMemsetAsync(out, 0, (size_t)words * 4, s);
    if (e != hipSuccess) {
        cc_set_error("png_pack: hipMemsetAsync: %s", hipGetErrorString(e));
        return (int)e;
    }
    hipLaunchKernelGGL(png_pack_kernel, dim3((unsigned)((int64_t)N * C)), dim3(kThreads), 0, s, (const uint32_t*)slots, chunk_bits, chunk_off, (uint32_t*)out,
                       out_bytes * 8);
    return cc_launch_status("png_pack");
}

int cc_png_adler(const uint8_t* filtered, uint32_t* partials, uint32_t* adler, int32_t N, int64_t L, hipStream_t s) {
    const int64_t C = (L + kChunk - 1) / kChunk;
    hipLaunchKernelGGL(png_adler_chunk_kernel, dim3((unsigned)((int64_t)N * C)), dim3(64), 0, s, filtered, partials, L, (int)C);
    if (int rc = cc_launch_status("png_adler_chunk")) return rc;
    hipLaunchKernelGGL(png_adler_frame_kernel, dim3((unsigned)((N + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, (const uint32_t*)partials, adler, L,
                       (int)C, (int)N);
    return cc_launch_status("png_adler");
}
