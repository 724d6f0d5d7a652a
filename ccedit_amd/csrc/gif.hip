// GIF output (include/ccedit_hip.h, "GIF"; ccedit_amd/gif.py; `--gif_encoder device`): uint8 RGB frames on the device -> per frame a
// palette of 256 colours (Wu's variance-minimising quantiser on a 32^3 grid of cells), the pixels' indices and their LZW byte stream,
// coded in independent chunks of 3072 pixels (GIF allows a Clear code anywhere: the trick of mjpeg.hip's restart intervals).
//   gif_histogram   a thread per pixel: count, sum r, sum g, sum b and sum r^2 + g^2 + b^2 of its cell (r >> 3, g >> 3, b >> 3), added with
//                   64-bit integer atomics into five tables on a 33^3 grid with a zero border.  Lanes of a wave that hold the same cell are
//                   combined first (up to four groups of four or more lanes: a ballot, a wave sum, ONE lane adds): a flat or few-colour
//                   frame would otherwise serialise on one or two addresses.  Integer sums: the result does not depend on the order.
//   gif_palette     two launches: the inclusive 3-D prefix sums of every table in place (a workgroup per table: a thread per line, three
//                   passes), then ONE WAVE PER FRAME for the 255 cuts: the next box is the lowest-indexed one of maximal score (cross-lane
//                   arg-max), its up to 93 cut positions are scored two per lane in float64 from 8-corner lookups in four tables and
//                   reduced per direction (greater score, then lower position); then the 32^3 table cell -> box and the rounded box means.
//   gif_map         a thread per pixel: index = cell table [r >> 3][g >> 3][b >> 3]
//   gif_lzw         ONE LANE PER CHUNK, four chunks per workgroup: the lane walks its pixels with the chunk's dictionary as an open
//                   hash table of 4096 words in LDS (prefix << 20 | byte << 12 | code, linear probing, at most 3071 entries) and writes the
//                   codes LSB first as 32-bit words into the chunk's slot; the chunk's bit length goes to chunk_bits.
//   gif_pack_scan   a workgroup per frame: the byte counts of the frames before it, the exclusive scan of its chunks' bit lengths ->
//                   every chunk's bit offset in the packed output, the frame's byte count
//   gif_pack        a workgroup per chunk: its bits shifted to their offset; the first and last word of a chunk are OR-ed into the
//                   zeroed output (neighbouring chunks share them), the words between are stored
// Every byte equals tests/_gif_numpy.py; the file is compiled with -ffp-contract=off -fno-slp-vectorize like the other bit-exact files:
// the cut scores are float64 products summed left to right and IEEE divisions, rounded as numpy rounds them.
//
// Nothing can overflow by construction: a chunk codes to at most (chunk + 2) codes of at most 12 bits and its slot holds that; a chunk adds
// at most 3071 entries to a table of 4096 words.  Chunk bit lengths and offsets are device data when the pack kernels read them: lengths
// are clamped into the slot, and a chunk whose bits would leave the output is skipped.  The argument checks live with the exported entry
// points in core.cpp.
#include "common.h"
#include "bitpack.h"

namespace {

constexpr int kThreads = 256;
constexpr int kSide = 33, kGrid = 32, kCells = kSide * kSide * kSide, kMoments = 5;      // ccedit_amd/gif.py SIDE, GRID, MOMENTS
constexpr int kColors = 256;
constexpr int kClear = 256, kEoi = 257, kFirstCode = 258, kStartWidth = 9;
constexpr int kChunkMax = 3072;
constexpr int kSlotWords = ((12 * (kChunkMax + 2) + 31) / 32 + 3) / 4 * 4;                 // 1156 words = gif.py SLOT_BYTES
constexpr int kSlotBits = kSlotWords * 32;
constexpr int kHashWords = 4096;
constexpr int kLzwChunks = 4;                    // chunks (= live lanes) per workgroup of the LZW stage: 4 x 16 KB of LDS
constexpr uint32_t kEmpty = 0xffffffffu;         // prefix 4095 is never a code

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
}

__device__ __forceinline__ void add_moments(unsigned long long* __restrict__ m, int cell, uint32_t n, uint32_t r, uint32_t g, uint32_t b, uint32_t sq) {
    atomicAdd(m + cell, (unsigned long long)n);
    atomicAdd(m + kCells + cell, (unsigned long long)r);
    atomicAdd(m + 2 * kCells + cell, (unsigned long long)g);
    atomicAdd(m + 3 * kCells + cell, (unsigned long long)b);
    atomicAdd(m + 4 * kCells + cell, (unsigned long long)sq);
}

// ---- histogram: grid (blocks per frame, N); every wave takes 64 consecutive pixels at a time
__global__ __launch_bounds__(kThreads) void gif_histogram_kernel(const uint8_t* __restrict__ frames, unsigned long long* __restrict__ mom, int64_t P) {
    const int64_t f = blockIdx.y;
    const uint8_t* src = frames + f * P * 3;
    unsigned long long* m = mom + f * (int64_t)(kMoments * kCells);
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    const int64_t rounds = (P + stride - 1) / stride;                          // the same for every thread: the ballots below stay convergent
    for (int64_t k = 0; k < rounds; ++k) {
        const int64_t i = k * stride + (int64_t)blockIdx.x * kThreads + threadIdx.x;
        const bool live = i < P;
        uint32_t r = 0, g = 0, b = 0;
        if (live) r = src[i * 3], g = src[i * 3 + 1], b = src[i * 3 + 2];
        const int cell = live ? (((int)(r >> 3) + 1) * kSide + (int)(g >> 3) + 1) * kSide + (int)(b >> 3) + 1 : -1;
        const uint32_t sq = r * r + g * g + b * b;
        unsigned long long todo = __ballot(live);
        bool mine = live;                                                       // this lane still has to add its own pixel
        for (int it = 0; it < 4 && todo; ++it) {
            const int leader = __builtin_ctzll(todo);
            const int c = __shfl(cell, leader, 64);
            const bool same = live && cell == c;
            const unsigned long long grp = __ballot(same);
            todo &= ~grp;
            if (__builtin_popcountll(grp) >= 4) {                                // (uniform)
                const uint32_t sn = wave_sum_u32(same ? 1u : 0u), sr = wave_sum_u32(same ? r : 0u), sg = wave_sum_u32(same ? g : 0u),
                               sb = wave_sum_u32(same ? b : 0u), ss = wave_sum_u32(same ? sq : 0u);
                if ((int)(threadIdx.x & 63) == leader) add_moments(m, c, sn, sr, sg, sb, ss);
                if (same) mine = false;
            }
        }
        if (mine) add_moments(m, cell, 1u, r, g, b, sq);
    }
}

// ---- prefix sums: a workgroup per table of a frame, a thread per line, one pass per axis
__global__ __launch_bounds__(kThreads) void gif_prefix_kernel(int64_t* __restrict__ mom) {
    int64_t* t = mom + (int64_t)blockIdx.x * kCells;
    const int strides[3] = {1, kSide, kSide * kSide};
#pragma unroll
    for (int axis = 0; axis < 3; ++axis) {
        const int sa = strides[axis], s1 = strides[(axis + 1) % 3], s2 = strides[(axis + 2) % 3];
        for (int line = threadIdx.x; line < kSide * kSide; line += kThreads) {
            int64_t* p = t + (line / kSide) * s2 + (line % kSide) * s1;
            int64_t acc = 0;
            for (int i = 0; i < kSide; ++i) {
                acc += p[i * sa];
                p[i * sa] = acc;
            }
        }
        __syncthreads();
    }
}

// ---- the cuts: one wave per frame
struct Box {
    int r0, r1, g0, g1, b0, b1;
};

__device__ __forceinline__ int64_t vol(const int64_t* __restrict__ t, const Box& x) {
    const int R1 = x.r1 * kSide * kSide, R0 = x.r0 * kSide * kSide, G1 = x.g1 * kSide, G0 = x.g0 * kSide;
    return t[R1 + G1 + x.b1] - t[R1 + G1 + x.b0] - t[R1 + G0 + x.b1] + t[R1 + G0 + x.b0] - t[R0 + G1 + x.b1] + t[R0 + G1 + x.b0] + t[R0 + G0 + x.b1] -
           t[R0 + G0 + x.b0];
}

__device__ __forceinline__ double box_score(const int64_t* __restrict__ p, const Box& x) {
    if ((x.r1 - x.r0) * (x.g1 - x.g0) * (x.b1 - x.b0) <= 1) return 0.0;
    const double w = (double)vol(p, x), dr = (double)vol(p + kCells, x), dg = (double)vol(p + 2 * kCells, x), db = (double)vol(p + 3 * kCells, x),
                 m2 = (double)vol(p + 4 * kCells, x);
    return m2 - (dr * dr + dg * dg + db * db) / w;
}

// the better of two (score, position) pairs: the greater score, then the lower position
__device__ __forceinline__ void take_better(double& s, int& pos, double os, int opos) {
    if (os > s || (os == s && opos < pos)) s = os, pos = opos;
}

__device__ __forceinline__ void wave_argmax(double& s, int& pos) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double os = __shfl_xor(s, o, 64);
        const int opos = __shfl_xor(pos, o, 64);
        take_better(s, pos, os, opos);
    }
}

__global__ __launch_bounds__(64) void gif_cut_kernel(const int64_t* __restrict__ mom, uint8_t* __restrict__ cells, uint8_t* __restrict__ palettes) {
    __shared__ Box s_box[kColors];
    __shared__ double s_score[kColors];
    __shared__ int s_n;
    const int lane = threadIdx.x;
    const int64_t f = blockIdx.x;
    const int64_t* p = mom + f * (int64_t)(kMoments * kCells);
    if (lane == 0) {
        const Box all = {0, kGrid, 0, kGrid, 0, kGrid};
        s_box[0] = all;
        s_score[0] = box_score(p, all);
        s_n = 1;
    }
    __syncthreads();
    for (;;) {
        const int n = s_n;
        double top = -1.0;
        int next = 0x7fffffff;
        for (int k = lane; k < n; k += 64) take_better(top, next, s_score[k], k);
        wave_argmax(top, next);                                                // the lowest-indexed box of maximal score
        if (n >= kColors || !(top > 0.0)) break;
        const Box x = s_box[next];
        const int64_t ww = vol(p, x), wr = vol(p + kCells, x), wg = vol(p + 2 * kCells, x), wb = vol(p + 3 * kCells, x);
        const int nr = x.r1 - x.r0 - 1, ng = x.g1 - x.g0 - 1, nb = x.b1 - x.b0 - 1;      // interior positions per direction, each 0 ... 31
        double best[3] = {-1.0, -1.0, -1.0};
        int at[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff};
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int c = lane + 64 * j;
            if (c >= nr + ng + nb) continue;
            Box h = x;
            int d, pos;
            if (c < nr)
                d = 0, pos = x.r0 + 1 + c, h.r1 = pos;
            else if (c < nr + ng)
                d = 1, pos = x.g0 + 1 + c - nr, h.g1 = pos;
            else
                d = 2, pos = x.b0 + 1 + c - nr - ng, h.b1 = pos;
            const int64_t hw = vol(p, h), hr = vol(p + kCells, h), hg = vol(p + 2 * kCells, h), hb = vol(p + 3 * kCells, h);
            const int64_t ow = ww - hw;
            if (hw <= 0 || ow <= 0) continue;                                      // an empty half
            const double fr = (double)hr, fg = (double)hg, fb = (double)hb, qr = (double)(wr - hr), qg = (double)(wg - hg), qb = (double)(wb - hb);
            const double s = (fr * fr + fg * fg + fb * fb) / (double)hw + (qr * qr + qg * qg + qb * qb) / (double)ow;
            if (d == 0) take_better(best[0], at[0], s, pos);
            if (d == 1) take_better(best[1], at[1], s, pos);
            if (d == 2) take_better(best[2], at[2], s, pos);
        }
#pragma unroll
        for (int d = 0; d < 3; ++d) wave_argmax(best[d], at[d]);
        const int d = (best[0] >= best[1] && best[0] >= best[2]) ? 0 : ((best[1] >= best[0] && best[1] >= best[2]) ? 1 : 2);
        const double sd = d == 0 ? best[0] : (d == 1 ? best[1] : best[2]);
        const int pos = d == 0 ? at[0] : (d == 1 ? at[1] : at[2]);
        if (lane == 0) {
            if (sd < 0.0) {
                s_score[next] = 0.0;                                                // cannot be cut: no palette entry is consumed
            } else {
                Box lo = x, hi = x;
                if (d == 0) lo.r1 = pos, hi.r0 = pos;
                if (d == 1) lo.g1 = pos, hi.g0 = pos;
                if (d == 2) lo.b1 = pos, hi.b0 = pos;
                s_box[next] = lo;
                s_box[n] = hi;
                s_score[next] = box_score(p, lo);
                s_score[n] = box_score(p, hi);
                s_n = n + 1;
            }
        }
        __syncthreads();
    }
    const int n = s_n;
    uint8_t* cell = cells + f * (int64_t)(kGrid * kGrid * kGrid);
    for (int k = 0; k < n; ++k) {                                                   // the boxes tile the grid: every cell is written once
        const Box x = s_box[k];
        const int dg = x.g1 - x.g0, db = x.b1 - x.b0, v = (x.r1 - x.r0) * dg * db;
        for (int i = lane; i < v; i += 64) {
            const int r = x.r0 + i / (dg * db), g = x.g0 + (i / db) % dg, b = x.b0 + i % db;
            cell[(r * kGrid + g) * kGrid + b] = (uint8_t)k;
        }
    }
    uint8_t* pal = palettes + f * (int64_t)(kColors * 3);
    for (int k = lane; k < kColors; k += 64) {
        int64_t w = 0, r = 0, g = 0, b = 0;
        if (k < n) {
            const Box x = s_box[k];
            w = vol(p, x), r = vol(p + kCells, x), g = vol(p + 2 * kCells, x), b = vol(p + 3 * kCells, x);
        }
        pal[k * 3] = (uint8_t)(w > 0 ? (r + w / 2) / w : 0);
        pal[k * 3 + 1] = (uint8_t)(w > 0 ? (g + w / 2) / w : 0);
        pal[k * 3 + 2] = (uint8_t)(w > 0 ? (b + w / 2) / w : 0);
    }
}

// ---- map: grid (blocks per frame, N)
__global__ __launch_bounds__(kThreads) void gif_map_kernel(const uint8_t* __restrict__ frames, const uint8_t* __restrict__ cells,
                                                           uint8_t* __restrict__ indices, int64_t P) {
    const int64_t f = blockIdx.y;
    const uint8_t* src = frames + f * P * 3;
    const uint8_t* cell = cells + f * (int64_t)(kGrid * kGrid * kGrid);
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < P; i += (int64_t)gridDim.x * kThreads) {
        const int r = src[i * 3] >> 3, g = src[i * 3 + 1] >> 3, b = src[i * 3 + 2] >> 3;
        indices[f * P + i] = cell[(r * kGrid + g) * kGrid + b];
    }
}

// ---- LZW: a lane per chunk
struct BitWriter {
    uint32_t* words;
    uint64_t acc = 0;
    uint32_t n = 0, wi = 0, bits = 0;
    __device__ __forceinline__ explicit BitWriter(uint32_t* w) : words(w) {}
    __device__ __forceinline__ void put(uint32_t code, uint32_t width) {           // width <= 12, n < 32
        acc |= (uint64_t)code << n;
        n += width;
        bits += width;
        if (n >= 32u) {
            if (wi < (uint32_t)kSlotWords) words[wi] = (uint32_t)acc;
            ++wi;
            acc >>= 32;
            n -= 32u;
        }
    }
    __device__ __forceinline__ void finish() {
        if (n && wi < (uint32_t)kSlotWords) words[wi] = (uint32_t)acc;
    }
};

__global__ __launch_bounds__(64) void gif_lzw_kernel(const uint8_t* __restrict__ indices, uint32_t* __restrict__ slots, int32_t* __restrict__ chunk_bits,
                                                     int64_t P, int chunk, int C, int64_t total) {
    __shared__ uint32_t s_hash[kLzwChunks][kHashWords];
    const int lane = threadIdx.x;
    for (int i = lane; i < kLzwChunks * kHashWords; i += 64) (&s_hash[0][0])[i] = kEmpty;
    __syncthreads();
    const int64_t id = (int64_t)blockIdx.x * kLzwChunks + lane;                  // chunk number over all frames
    if (lane >= kLzwChunks || id >= total) return;
    const int64_t f = id / C;
    const int c = (int)(id - f * C);
    const int64_t p0 = (int64_t)c * chunk;
    const int len = (int)(P - p0 < chunk ? P - p0 : chunk);
    const uint8_t* src = indices + f * P + p0;
    uint32_t* table = s_hash[lane];
    BitWriter out(slots + id * kSlotWords);
    uint32_t width = kStartWidth, next = kFirstCode;
    if (c == 0) out.put(kClear, width);
    uint32_t prev = src[0];
    for (int k = 1; k < len; ++k) {
        const uint32_t ch = src[k];
        const uint32_t key = (prev << 8) | ch;                                  // 20 bits
        uint32_t h = ((key * 2654435761u) >> 20) & (kHashWords - 1);
        uint32_t found = kEmpty;
        for (int probe = 0; probe < kHashWords; ++probe) {                       // at most 3071 of 4096 words are ever taken: an empty one is met
            const uint32_t e = table[h];
            if (e == kEmpty) break;
            if ((e >> 12) == key) {
                found = e & 4095u;
                break;
            }
            h = (h + 1) & (kHashWords - 1);
        }
        if (found != kEmpty) {
            prev = found;
            continue;
        }
        out.put(prev, width);
        table[h] = (key << 12) | next;
        ++next;
        if (next > (1u << width)) ++width;
        prev = ch;
    }
    out.put(prev, width);
    ++next;
    if (next > (1u << width)) ++width;
    out.put(c == C - 1 ? kEoi : kClear, width);
    out.finish();
    chunk_bits[id] = (int32_t)out.bits;
}

// ---- pack: where every chunk's bits go (a workgroup per frame), then the shifted copy (a workgroup per chunk): bitpack.h, shared with png.hip
__global__ __launch_bounds__(kThreads) void gif_pack_scan_kernel(const int32_t* __restrict__ chunk_bits, int64_t* __restrict__ chunk_off,
                                                                 int32_t* __restrict__ frame_bytes, int C) {
    cc_pack_scan<kThreads, kSlotBits>(chunk_bits, chunk_off, frame_bytes, C);
}

__global__ __launch_bounds__(kThreads) void gif_pack_kernel(const uint32_t* __restrict__ slots, const int32_t* __restrict__ chunk_bits,
                                                            const int64_t* __restrict__ chunk_off, uint32_t* __restrict__ out, int64_t out_bits) {
    cc_pack_chunk<kThreads, kSlotWords>(slots, chunk_bits, chunk_off, out, out_bits);
}

}  // namespace

// ------------------------------------------------------------------------------------------
// launchers (arguments validated by the entry points in core.cpp)
// ------------------------------------------------------------------------------------------
int64_t cc_gif_slot_bytes() { return (int64_t)kSlotWords * 4; }

static unsigned gif_pixel_blocks(int64_t P) {
    const int64_t b = (P + kThreads - 1) / kThreads;
    return (unsigned)(b < 1024 ? b : 1024);
}

int cc_gif_histogram(const uint8_t* frames, int64_t* moments, int32_t N, int32_t H, int32_t W, hipStream_t s) {
    const int64_t P = (int64_t)H * W;
    hipError_t e = hipMemsetAsync(moments, 0, (size_t)N * kMoments * kCells * sizeof(int64_t), s);
    if (e != hipSuccess) {
        cc_set_error("gif_histogram: hipMemsetAsync: %s", hipGetErrorString(e));
        return (int)e;
    }
    hipLaunchKernelGGL(gif_histogram_kernel, dim3(gif_pixel_blocks(P), (unsigned)N), dim3(kThreads), 0, s, frames, (unsigned long long*)moments, P);
    return cc_launch_status("gif_histogram");
}

int cc_gif_palette(int64_t* moments, uint8_t* cells, uint8_t* palettes, int32_t N, hipStream_t s) {
    hipLaunchKernelGGL(gif_prefix_kernel, dim3((unsigned)(N * kMoments)), dim3(kThreads), 0, s, moments);
    if (int rc = cc_launch_status("gif_prefix")) return rc;
    hipLaunchKernelGGL(gif_cut_kernel, dim3((unsigned)N), dim3(64), 0, s, (const int64_t*)moments, cells, palettes);
    return cc_launch_status("gif_palette");
}

int cc_gif_map(const uint8_t* frames, const uint8_t* cells, uint8_t* indices, int32_t N, int32_t H, int32_t W, hipStream_t s) {
    const int64_t P = (int64_t)H * W;
    hipLaunchKernelGGL(gif_map_kernel, dim3(gif_pixel_blocks(P), (unsigned)N), dim3(kThreads), 0, s, frames, cells, indices, P);
    return cc_launch_status("gif_map");
}

int cc_gif_lzw(const uint8_t* indices, uint8_t* slots, int32_t* chunk_bits, int32_t N, int32_t H, int32_t W, int32_t chunk, hipStream_t s) {
    const int64_t P = (int64_t)H * W;
    const int64_t C = (P + chunk - 1) / chunk, total = (int64_t)N * C;
    hipLaunchKernelGGL(gif_lzw_kernel, dim3((unsigned)((total + kLzwChunks - 1) / kLzwChunks)), dim3(64), 0, s, indices, (uint32_t*)slots, chunk_bits, P,
                       (int)chunk, (int)C, total);
    return cc_launch_status("gif_lzw");
}

int cc_gif_pack_scan(const int32_t* chunk_bits, int64_t* chunk_off, int32_t* frame_bytes, int32_t N, int32_t H, int32_t W, int32_t chunk, hipStream_t s) {
    const int64_t C = ((int64_t)H * W + chunk - 1) / chunk;
    hipLaunchKernelGGL(gif_pack_scan_kernel, dim3((unsigned)N), dim3(kThreads), 0, s, chunk_bits, chunk_off, frame_bytes, (int)C);
    return cc_launch_status("gif_pack_scan");
}

int cc_gif_pack(const uint8_t* slots, const int32_t* chunk_bits, const int64_t* chunk_off, uint8_t* out, int32_t N, int32_t H, int32_t W, int32_t chunk,
                int64_t out_bytes, hipStream_t s) {
    const int64_t C = ((int64_t)H * W + chunk - 1) / chunk;
    const int64_t words = (out_bytes + 3) / 4;
    hipError_t e = hipMemsetAsync(out, 0, (size_t)words * 4, s);
    if (e != hipSuccess) {
        cc_set_error("gif_pack: hipMemsetAsync: %s", hipGetErrorString(e));
        return (int)e;
    }
    hipLaunchKernelGGL(gif_pack_kernel, dim3((unsigned)(N * C)), dim3(kThreads), 0, s, (const uint32_t*)slots, chunk_bits, chunk_off, (uint32_t*)out,
                       out_bytes * 8);
    return cc_launch_status("gif_pack");
}
