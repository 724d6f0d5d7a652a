// Motion-JPEG output (include/ccedit_hip.h, "Motion-JPEG"; ccedit_amd/mjpeg.py; `--save_type mjpeg`): uint8 RGB frames on the device ->
// one baseline JPEG (ITU-T T.81: sequential DCT, 8 bit, YCbCr 4:2:0, Annex K tables, restart interval = one MCU row) per frame.
//   mjpeg_transform   per strip of four 16 x 16 MCUs: RGB rows through LDS (16-byte global reads), Y and the 2 x 2-mean Cb / Cr in 16-bit
//                     fixed point, level shift, separable fixed-point 8 x 8 FDCT (row pass, column pass), quantisation by exact integer
//                     division with rounding, zigzag -> int16 coefficients in MCU order, written as 16-byte vectors
//   mjpeg_entropy     ONE WAVE PER RESTART INTERVAL, a lane per block, 64 blocks at a time: every lane walks its block twice — first
//                     the bit count, then, after a prefix sum across the wave gave its bit offset, the code words themselves, OR-ed
//                     into an LDS bit buffer (ds_or on 32-bit words).  The wave then stuffs the finished bytes (FF -> FF 00: count per
//                     lane, a second prefix sum) into the interval's slot of the segment buffer; the last byte is padded with ones.
//   mjpeg_pack_scan   per frame the exclusive scan of its segments' lengths -> where every segment goes, and the frame's byte count
//   mjpeg_pack        header, segments, RSTn markers and EOI copied to their place: the frames lie back to back, complete files
// Every byte equals tests/_mjpeg_numpy.py; the file is compiled with -ffp-contract=off -fno-slp-vectorize like the other bit-exact files
// (there is no floating point in it).
//
// Nothing is truncated and nothing can overflow, by construction: a block needs at most 63 x 26 + 27 bits (AC magnitudes are clamped to
// 10 bits, the DC difference to 11, code lengths to 16 WHATEVER the table holds), the LDS buffer holds 64 such blocks plus the carried
// partial byte, and an interval's slot (cc_mjpeg_segment_bytes) holds all its blocks at that bound with every byte stuffed.
//
// The constants (quantisation base tables, zigzag, FDCT matrix, colour factors, Huffman codes) arrive as ONE int32 table from
// ccedit_amd/mjpeg.py, their one place.  It is device data the host cannot check per launch: every value read from it is held in its
// range (indices masked, divisors >= 1, code lengths <= 16), so that nothing in it can take an access outside a buffer.  So are the
// segment lengths and offsets the pack kernels read.  The argument checks live with the exported entry points in core.cpp.
#include "common.h"

namespace {

constexpr int kTabQuant = 0, kTabZigzag = 128, kTabDct = 192, kTabColor = 256, kTabDc = 272, kTabAc = 304;      // ccedit_amd/mjpeg.py TAB_*
constexpr int kThreads = 256;
constexpr int kStrip = 4;                       // MCUs per workgroup of the transform
constexpr int kStripBlocks = kStrip * 6;
constexpr int kMaxBlockBits = 63 * 26 + 27;      // 63 AC coefficients of 16 + 10 bits, a DC difference of 16 + 11
constexpr int kStageWords = (7 + 64 * kMaxBlockBits + 31) / 32 + 3;        // 64 blocks + the carried partial byte

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- transform: a workgroup per strip of up to four MCUs of one MCU row
__global__ __launch_bounds__(kThreads) void mjpeg_transform_kernel(const uint8_t* __restrict__ frames, const int32_t* __restrict__ tab,
                                                                   int16_t* __restrict__ coef, int H, int W, int quality) {
    __shared__ __attribute__((aligned(16))) uint8_t s_rgb[16][kStrip * 48];
    __shared__ int16_t s_pix[kStripBlocks][64];                              // level-shifted samples, row-major per block
    __shared__ int32_t s_row[kStripBlocks][64];                              // after the row pass: [y][u], 5 fraction bits
    __shared__ __attribute__((aligned(16))) int16_t s_out[kStripBlocks][64];  // quantised, in scan order
    __shared__ int32_t s_q[128], s_dct[64], s_izz[64], s_col[9];
    const int tid = threadIdx.x;
    const int MC = W / 16, MR = H / 16, SC = (MC + kStrip - 1) / kStrip;
    const int sx = (int)(blockIdx.x % (unsigned)SC);
    const int64_t r = blockIdx.x / (unsigned)SC;
    const int my = (int)(r % MR);
    const int64_t f = r / MR;
    const int mcu0 = sx * kStrip;
    const int nm = MC - mcu0 < kStrip ? MC - mcu0 : kStrip;

    if (tid < 128) {
        const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
        s_q[tid] = clampi((clampi(tab[kTabQuant + tid], 1, 255) * s + 50) / 100, 1, 255);
    }
    if (tid < 64) {
        s_dct[tid] = clampi(tab[kTabDct + tid], -4096, 4096);                 // |row sums| < 2^22, |column sums| < 2^30
        s_izz[tid] = 0;
    }
    if (tid < 9) s_col[tid] = clampi(tab[kTabColor + tid], -65536, 65536);
    const int vec_per_row = nm * 3;                                          // 16-byte vectors of one pixel row of the strip
    const uint8_t* src = frames + ((f * H + (int64_t)my * 16) * W + (int64_t)mcu0 * 16) * 3;
    for (int i = tid; i < 16 * vec_per_row; i += kThreads) {
        const int row = i / vec_per_row, c = i - row * vec_per_row;
        *(u32x4*)&s_rgb[row][c * 16] = *(const u32x4*)(src + (int64_t)row * W * 3 + c * 16);
    }
    __syncthreads();
    if (tid < 64) s_izz[tab[kTabZigzag + tid] & 63] = tid;                   // row-major index -> place in the scan

    const int yw = nm * 16;
    for (int i = tid; i < 16 * yw; i += kThreads) {
        const int py = i / yw, px = i - py * yw;
        const uint8_t* p = &s_rgb[py][px * 3];
        const int y = (s_col[0] * p[0] + s_col[1] * p[1] + s_col[2] * p[2] + 32768) >> 16;
        const int b = (px >> 4) * 6 + (py >> 3) * 2 + ((px >> 3) & 1);
        s_pix[b][(py & 7) * 8 + (px & 7)] = (int16_t)(clampi(y, 0, 255) - 128);
    }
    const int cw = nm * 8;
    for (int i = tid; i < 8 * cw; i += kThreads) {
        const int cy = i / cw, cx = i - cy * cw;
        const uint8_t* p0 = &s_rgb[2 * cy][cx * 6];
        const uint8_t* p1 = &s_rgb[2 * cy + 1][cx * 6];
        const int rs = p0[0] + p0[3] + p1[0] + p1[3], gs = p0[1] + p0[4] + p1[1] + p1[4], bs = p0[2] + p0[5] + p1[2] + p1[5];
        const int cb = (s_col[3] * rs + s_col[4] * gs + s_col[5] * bs + (128 << 18) + (1 << 17) - 1) >> 18;
        const int cr = (s_col[6] * rs + s_col[7] * gs + s_col[8] * bs + (128 << 18) + (1 << 17) - 1) >> 18;
        const int b = (cx >> 3) * 6 + 4;
        s_pix[b][cy * 8 + (cx & 7)] = (int16_t)(clampi(cb, 0, 255) - 128);
        s_pix[b + 1][cy * 8 + (cx & 7)] = (int16_t)(clampi(cr, 0, 255) - 128);
    }
    __syncthreads();
    for (int i = tid; i < nm * 48; i += kThreads) {                          // row pass: a thread per row of a block
        const int b = i >> 3, y = i & 7;
        int p[8];
#pragma unroll
        for (int x = 0; x < 8; ++x) p[x] = s_pix[b][y * 8 + x];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            int acc = 0;
#pragma unroll
            for (int x = 0; x < 8; ++x) acc += s_dct[u * 8 + x] * p[x];
            s_row[b][y * 8 + u] = (acc + 128) >> 8;
        }
    }
    __syncthreads();
    for (int i = tid; i < nm * 48; i += kThreads) {                          // column pass, quantisation, zigzag: a thread per column
        const int b = i >> 3, u = i & 7;
        const int qoff = (b % 6) >= 4 ? 64 : 0;
        int t[8];
#pragma unroll
        for (int y = 0; y < 8; ++y) t[y] = s_row[b][y * 8 + u];
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            int acc = 0;
#pragma unroll
            for (int y = 0; y < 8; ++y) acc += s_dct[v * 8 + y] * t[y];
            const int nat = v * 8 + u;
            const uint32_t q = (uint32_t)s_q[qoff + nat];
            const uint32_t a = (uint32_t)(acc < 0 ? -acc : acc);
            uint32_t m = ((a + (q << 17)) >> 18) / q;                         // exact: floor(x / (q 2^18)) = floor(floor(x / 2^18) / q)
            if (nat != 0 && m > 1023u) m = 1023u;
            s_out[b][s_izz[nat]] = (int16_t)(acc < 0 ? -(int)m : (int)m);
        }
    }
    __syncthreads();
    int16_t* dst = coef + (((f * MR + my) * MC + mcu0) * 6) * 64;
    for (int i = tid; i < nm * 48; i += kThreads) ((u32x4*)dst)[i] = ((const u32x4*)&s_out[0][0])[i];
}

// ---- entropy coding: one wave (= one workgroup) per restart interval
struct BitCount {
    uint32_t bits = 0;
    __device__ __forceinline__ void put(uint32_t, uint32_t len) { bits += len; }
};

struct BitMerge {
    uint32_t* words;
    uint64_t acc = 0;
    uint32_t n, wi;
    __device__ __forceinline__ BitMerge(uint32_t* w, uint32_t bit_offset) : words(w), n(bit_offset & 31u), wi(bit_offset >> 5) {}
    __device__ __forceinline__ void put(uint32_t code, uint32_t len) {       // len <= 27, n < 32
        acc = (acc << len) | code;
        n += len;
        if (n >= 32u) {
            n -= 32u;
            atomicOr(&words[wi++], (uint32_t)(acc >> n));
        }
    }
    __device__ __forceinline__ void finish() {
        if (n) atomicOr(&words[wi], (uint32_t)(acc << (32u - n)));
    }
};

// The code words of one block (c: its 64 coefficients in scan order as 32 dwords, pred: the DC predictor).  Table entries: code << 8 | length.
template <class Sink>
__device__ __forceinline__ void code_block(Sink& sink, const uint32_t (&c)[32], int pred, const int32_t* dc_tab, const int32_t* ac_tab) {
    const int d = clampi((int)(int16_t)(c[0] & 0xffffu) - pred, -2047, 2047);
    {
        const uint32_t a = (uint32_t)(d < 0 ? -d : d);
        const uint32_t s = a ? 32u - (uint32_t)__builtin_clz(a) : 0u;             // bit length, 0 for 0
        const uint32_t e = (uint32_t)dc_tab[s];
        sink.put(((e >> 8) << s) | ((uint32_t)(d < 0 ? d - 1 : d) & ((1u << s) - 1u)), (e & 255u) + s);
    }
    uint32_t run = 0;
    const uint32_t zrl = (uint32_t)ac_tab[0xF0], eob = (uint32_t)ac_tab[0];
#pragma unroll
    for (int k = 1; k < 64; ++k) {
        const int v = clampi((int)(int16_t)((c[k >> 1] >> (16 * (k & 1))) & 0xffffu), -1023, 1023);
        if (v == 0) {
            ++run;
        } else {
            while (run >= 16u) {
                sink.put(zrl >> 8, zrl & 255u);
                run -= 16u;
            }
            const uint32_t a = (uint32_t)(v < 0 ? -v : v);
            const uint32_t s = 32u - (uint32_t)__builtin_clz(a);
            const uint32_t e = (uint32_t)ac_tab[(run << 4) | s];
            sink.put(((e >> 8) << s) | ((uint32_t)(v < 0 ? v - 1 : v) & ((1u << s) - 1u)), (e & 255u) + s);
            run = 0;
        }
    }
    if (run) sink.put(eob >> 8, eob & 255u);
}

__device__ __forceinline__ uint32_t wave_scan_inclusive(uint32_t x, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)x, d, 64);
        if (lane >= d) x += y;
    }
    return x;
}

__global__ __launch_bounds__(64) void mjpeg_entropy_kernel(const int16_t* __restrict__ coef, const int32_t* __restrict__ tab,
                                                           uint8_t* __restrict__ scratch, int32_t* __restrict__ seg_len, int MC, int64_t seg_cap) {
    __shared__ uint32_t s_bits[kStageWords];
    __shared__ int32_t s_dc[2 * 16], s_ac[2 * 256];
    const int lane = threadIdx.x;
    const int64_t seg = blockIdx.x;
    for (int i = lane; i < 32 + 512; i += 64) {                              // codes held to their lengths, lengths to 16
        const uint32_t e = (uint32_t)(i < 32 ? tab[kTabDc + i] : tab[kTabAc + i - 32]);
        const uint32_t len = (e & 255u) > 16u ? 16u : (e & 255u);
        const int32_t held = (int32_t)((((e >> 8) & ((1u << len) - 1u)) << 8) | len);
        if (i < 32)
            s_dc[i] = held;
        else
            s_ac[i - 32] = held;
    }
    const int nb = MC * 6;
    const int16_t* c0 = coef + seg * nb * 64;
    uint8_t* out = scratch + seg * seg_cap;
    uint32_t carry_bits = 0, carry_byte = 0;
    int64_t out_pos = 0;
    for (int base = 0; base < nb; base += 64) {
        const int b = base + lane;
        const bool live = b < nb;
        const bool last = base + 64 >= nb;
        uint32_t c[32];
        int pred = 0, comp = 0;
        if (live) {
            const u32x4* p = (const u32x4*)(c0 + (int64_t)b * 64);
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const u32x4 v = p[q];
                c[4 * q] = v[0], c[4 * q + 1] = v[1], c[4 * q + 2] = v[2], c[4 * q + 3] = v[3];
            }
            const int j = b % 6;
            comp = j >= 4;
            const int pb = j == 0 ? b - 3 : (j >= 4 ? b - 6 : b - 1);           // the previous block of the same component in the interval
            if (pb >= 0) pred = c0[(int64_t)pb * 64];
        } else {
#pragma unroll
            for (int q = 0; q < 32; ++q) c[q] = 0;
        }
        const int32_t* dc_tab = &s_dc[comp * 16];
        const int32_t* ac_tab = &s_ac[comp * 256];
        __syncthreads();                                                     // tables written; the previous round's bytes read
        BitCount count;
        if (live) code_block(count, c, pred, dc_tab, ac_tab);
        const uint32_t incl = wave_scan_inclusive(count.bits, lane);
        uint32_t total = carry_bits + (uint32_t)__shfl((int)incl, 63, 64);   // <= 7 + 64 * kMaxBlockBits
        const uint32_t pad = last ? (8u - (total & 7u)) & 7u : 0u;
        const uint32_t nwords = (total + pad + 31u) >> 5;
        for (uint32_t i = lane; i <= nwords && i < (uint32_t)kStageWords; i += 64) s_bits[i] = 0;
        __syncthreads();
        if (lane == 0) {                                                     // the carried bits in front, the padding ones behind
            atomicOr(&s_bits[0], carry_byte << 24);
            if (pad) atomicOr(&s_bits[total >> 5], ((1u << pad) - 1u) << (32u - (total & 31u) - pad));       // inside one byte
        }
        if (live) {
            BitMerge merge(s_bits, carry_bits + incl - count.bits);
            code_block(merge, c, pred, dc_tab, ac_tab);
            merge.finish();
        }
        __syncthreads();
        total += pad;
        const uint32_t nbytes = total >> 3;                                   // finished bytes of this round
        const uint32_t per = (nbytes + 63u) >> 6;
        const uint32_t k0 = lane * per < nbytes ? lane * per : nbytes, k1 = k0 + per < nbytes ? k0 + per : nbytes;
        uint32_t ff = 0;
        for (uint32_t k = k0; k < k1; ++k) ff += ((s_bits[k >> 2] >> (24u - 8u * (k & 3u))) & 255u) == 255u;
        const uint32_t ff_incl = wave_scan_inclusive(ff, lane);
        int64_t at = out_pos + k0 + (ff_incl - ff);
        for (uint32_t k = k0; k < k1; ++k) {
            const uint32_t v = (s_bits[k >> 2] >> (24u - 8u * (k & 3u))) & 255u;
            if (at < seg_cap) out[at] = (uint8_t)v;
            ++at;
            if (v == 255u) {
                if (at < seg_cap) out[at] = 0;
                ++at;
            }
        }
        out_pos += nbytes + (uint32_t)__shfl((int)ff_incl, 63, 64);
        carry_bits = total & 7u;
        carry_byte = carry_bits ? (s_bits[nbytes >> 2] >> (24u - 8u * (nbytes & 3u))) & 255u : 0u;
    }
    if (lane == 0) seg_len[seg] = (int32_t)(out_pos < seg_cap ? out_pos : seg_cap);
}

// ---- pack: where every segment goes (a workgroup per frame), then the copy (a workgroup per segment)
__global__ __launch_bounds__(kThreads) void mjpeg_pack_scan_kernel(const int32_t* __restrict__ seg_len, int64_t* __restrict__ seg_off,
                                                                   int32_t* __restrict__ frame_bytes, int MR, int hdr_len, int seg_cap) {
    __shared__ int64_t s_part[kThreads];
    const int tid = threadIdx.x;
    const int64_t f = blockIdx.x;
    int64_t sum = 0;
    for (int64_t i = tid; i < f * MR; i += kThreads) sum += clampi(seg_len[i], 0, seg_cap);
    s_part[tid] = sum;
    __syncthreads();
    for (int o = kThreads / 2; o > 0; o >>= 1) {
        if (tid < o) s_part[tid] += s_part[tid + o];
        __syncthreads();
    }
    if (tid == 0) {
        int64_t at = s_part[0] + f * ((int64_t)hdr_len + 2 * (int64_t)MR) + hdr_len;          // the frames before this one, this one's header
        const int64_t start = at - hdr_len;
        for (int s = 0; s < MR; ++s) {
            seg_off[f * MR + s] = at;
            at += clampi(seg_len[f * MR + s], 0, seg_cap) + 2;                               // the segment and its RSTn (the last one: EOI)
        }
        const int64_t bytes = at - start;
        frame_bytes[f] = (int32_t)(bytes < 0x7fffffff ? bytes : 0x7fffffff);
    }
}

__global__ __launch_bounds__(kThreads) void mjpeg_pack_kernel(const uint8_t* __restrict__ scratch, const int32_t* __restrict__ seg_len,
                                                              const int64_t* __restrict__ seg_off, const uint8_t* __restrict__ header,
                                                              uint8_t* __restrict__ out, int MR, int hdr_len, int64_t seg_cap, int64_t out_bytes) {
    const int tid = threadIdx.x;
    const int64_t seg = blockIdx.x;
    const int s = (int)(seg % MR);
    const int64_t off = seg_off[seg];
    const int len = clampi(seg_len[seg], 0, (int)seg_cap);
    if (off < hdr_len || off > out_bytes - len - 2) return;                  // (cannot happen with the offsets of mjpeg_pack_scan)
    if (s == 0)
        for (int i = tid; i < hdr_len; i += kThreads) out[off - hdr_len + i] = header[i];
    const uint8_t* src = scratch + seg * seg_cap;
    for (int i = tid; i < len; i += kThreads) out[off + i] = src[i];
    if (tid == 0) {
        out[off + len] = 0xFF;
        out[off + len + 1] = (uint8_t)(s < MR - 1 ? 0xD0 + (s & 7) : 0xD9);
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------
// launchers (arguments validated by the entry points in core.cpp)
// ------------------------------------------------------------------------------------------
int64_t cc_mjpeg_segment_bytes(int32_t W) {
    const int64_t blocks = (int64_t)(W / 16) * 6;
    return (2 * ((blocks * kMaxBlockBits + 7) / 8 + 1) + 15) / 16 * 16;
}

int cc_mjpeg_transform(const uint8_t* frames, const int32_t* tab, int16_t* coef, int32_t N, int32_t H, int32_t W, int32_t quality, hipStream_t s) {
    const int64_t grid = (int64_t)N * (H / 16) * ((W / 16 + kStrip - 1) / kStrip);
    hipLaunchKernelGGL(mjpeg_transform_kernel, dim3((unsigned)grid), dim3(kThreads), 0, s, frames, tab, coef, H, W, quality);
    return cc_launch_status("mjpeg_transform");
}

int cc_mjpeg_entropy(const int16_t* coef, const int32_t* tab, uint8_t* scratch, int32_t* seg_len, int32_t N, int32_t H, int32_t W, hipStream_t s) {
    hipLaunchKernelGGL(mjpeg_entropy_kernel, dim3((unsigned)((int64_t)N * (H / 16))), dim3(64), 0, s, coef, tab, scratch, seg_len, W / 16,
                       cc_mjpeg_segment_bytes(W));
    return cc_launch_status("mjpeg_entropy");
}

int cc_mjpeg_pack_scan(const int32_t* seg_len, int64_t* seg_off, int32_t* frame_bytes, int32_t N, int32_t H, int32_t W, int32_t hdr_len, hipStream_t s) {
    hipLaunchKernelGGL(mjpeg_pack_scan_kernel, dim3((unsigned)N), dim3(kThreads), 0, s, seg_len, seg_off, frame_bytes, H / 16, hdr_len,
                       (int)cc_mjpeg_segment_bytes(W));
    return cc_launch_status("mjpeg_pack_scan");
}

int cc_mjpeg_pack(const uint8_t* scratch, const int32_t* seg_len, const int64_t* seg_off, const uint8_t* header, uint8_t* out, int32_t N, int32_t H,
                  int32_t W, int32_t hdr_len, int64_t out_bytes, hipStream_t s) {
    hipLaunchKernelGGL(mjpeg_pack_kernel, dim3((unsigned)((int64_t)N * (H / 16))), dim3(kThreads), 0, s, scratch, seg_len, seg_off, header, out, H / 16,
                       hdr_len, cc_mjpeg_segment_bytes(W), out_bytes);
    return cc_launch_status("mjpeg_pack");
}
