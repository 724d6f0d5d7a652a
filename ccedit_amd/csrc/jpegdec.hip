// JPEG sources decoded on the device (include/ccedit_hip.h, "JPEG decoding"; ccedit_amd/jpegdec.py): the
// entropy-coded bytes of N baseline JPEG frames of one geometry and one set of tables -> uint8 RGB frames.  The stages of mjpeg.hip
// in reverse:
//   jpegdec_entropy   ONE THREAD PER RESTART INTERVAL (Huffman decoding is serial inside an interval: the DC prediction and every
//                     code's position depend on what came before).  The thread runs jpegdec_core.h — the same text the host-side
//                     hardening program compiles — from the tables in LDS and writes int16 coefficients in natural order plus one
//                     status word.  Few lanes of a wave decode (the launcher picks 1 ... 64 so that the grid still covers the chip):
//                     lanes of one wave walk different code paths, and a wave costs what its slowest lane costs.
//   jpegdec_idct      a thread per 8 x 8 block: dequantisation, libjpeg's accurate integer inverse DCT ("islow": 13-bit constants, two
//                     fraction bits after the column pass, one rounding per pass), the range limit ((x & 1023) as a signed 10-bit value,
//                     + 128, clamp) -> the component's plane, padded to whole MCUs
//   jpegdec_rgb       a thread per pixel: libjpeg's "fancy" chroma up-sampling (triangle filters: h2v1 (3 a + b + 1) >> 2 /
//                     (3 a + c + 2) >> 2, h2v2 3 near + far vertically, then (3 a + b + 8) >> 4 / (3 a + c + 7) >> 4; replication for
//                     planes of one or two columns) over the component's REAL size, YCbCr -> RGB in 16-bit fixed point, clamp
// Every byte equals tests/_jpegdec_numpy.py, which equals Pillow (libjpeg-turbo) on every stream an encoder writes.  All arithmetic is
// integer; the inverse DCT is computed modulo 2^32 (unsigned), so hostile coefficients wrap the same way everywhere instead of
// overflowing.  The file is compiled with -ffp-contract=off -fno-slp-vectorize like the other bit-exact files.
//
// Bounds.  The host checks geometry and buffer sizes (core.cpp).  What lies in device memory it cannot check: interval offsets are
// clamped into [0, data_bytes] here, table values are masked where they index (jpegdec_core.h), and every thread's outputs are its
// own interval's blocks, its own block's 64 samples, its own pixel.
#include "common.h"
#include "jpegdec_core.h"

namespace {

using namespace jpegdec;

struct Geom {
    int H, W, ncomp, hs, vs;
    int mx, my;          // MCUs across and down
    int bpm;             // blocks per MCU
    int yw, yh, cw, ch;  // plane sizes, padded to whole MCUs (luma; chroma)
};

__host__ __device__ inline Geom make_geom(int H, int W, int ncomp, int hs, int vs) {
    Geom g;
    g.H = H, g.W = W, g.ncomp = ncomp;
    g.hs = ncomp == 1 ? 1 : hs, g.vs = ncomp == 1 ? 1 : vs;
    g.mx = (W + 8 * g.hs - 1) / (8 * g.hs), g.my = (H + 8 * g.vs - 1) / (8 * g.vs);
    g.bpm = ncomp == 1 ? 1 : g.hs * g.vs + 2;
    g.yw = g.mx * g.hs * 8, g.yh = g.my * g.vs * 8;
    g.cw = ncomp == 1 ? 0 : g.mx * 8, g.ch = ncomp == 1 ? 0 : g.my * 8;
    return g;
}

__host__ __device__ inline int64_t plane_bytes(const Geom& g) { return (int64_t)g.yw * g.yh + 2 * (int64_t)g.cw * g.ch; }

// ---- entropy: `lanes` threads of every 64-thread workgroup decode one interval each; all 64 copy the tables to LDS
__global__ __launch_bounds__(64) void jpegdec_entropy_kernel(const uint8_t* __restrict__ data, int64_t data_bytes, const int64_t* __restrict__ intervals,
                                                             const int32_t* __restrict__ tab, int16_t* __restrict__ coef,
                                                             int32_t* __restrict__ status, int64_t n_intervals, int per_frame, int64_t mcus_frame,
                                                             int64_t mcus_interval, int ncomp, int luma_blocks, int lanes) {
    __shared__ int32_t s_tab[kTabSize];
    for (int i = threadIdx.x; i < kTabSize; i += 64) s_tab[i] = tab[i];
    __syncthreads();
    if ((int)threadIdx.x >= lanes) return;
    const int64_t iv = (int64_t)blockIdx.x * lanes + threadIdx.x;
    if (iv >= n_intervals) return;
    const int64_t f = iv / per_frame, j = iv - f * per_frame;
    int64_t lo = intervals[2 * iv], hi = intervals[2 * iv + 1];
    lo = lo < 0 ? 0 : (lo > data_bytes ? data_bytes : lo);
    hi = hi < lo ? lo : (hi > data_bytes ? data_bytes : hi);
    const int64_t first = j * mcus_interval;                                  // < mcus_frame: per_frame = ceil(mcus_frame / mcus_interval)
    const int64_t n = mcus_frame - first < mcus_interval ? mcus_frame - first : mcus_interval;
    const int bpm = ncomp == 1 ? 1 : luma_blocks + 2;
    status[iv] = decode_interval(data, lo, hi, s_tab, ncomp, luma_blocks, n, coef + ((f * mcus_frame + first) * bpm) * 64);
}

// ---- reconstruction: a thread per block.  One pass of the islow inverse DCT over 8 values, modulo 2^32.
__device__ __forceinline__ void idct_pass(const uint32_t (&in)[8], int32_t (&out)[8], int shift) {
    constexpr uint32_t F0_298 = 2446, F0_390 = 3196, F0_541 = 4433, F0_765 = 6270, F0_899 = 7373, F1_175 = 9633, F1_501 = 12299,
                       F1_847 = 15137, F1_961 = 16069, F2_053 = 16819, F2_562 = 20995, F3_072 = 25172;
    uint32_t z1 = (in[2] + in[6]) * F0_541;
    uint32_t t2 = z1 - in[6] * F1_847;
    uint32_t t3 = z1 + in[2] * F0_765;
    uint32_t t0 = (in[0] + in[4]) << 13;
    uint32_t t1 = (in[0] - in[4]) << 13;
    const uint32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    t0 = in[7], t1 = in[5], t2 = in[3], t3 = in[1];
    z1 = t0 + t3;
    uint32_t z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
    const uint32_t z5 = (z3 + z4) * F1_175;
    t0 *= F0_298, t1 *= F2_053, t2 *= F3_072, t3 *= F1_501;
    z1 = 0u - z1 * F0_899, z2 = 0u - z2 * F2_562;
    z3 = z5 - z3 * F1_961, z4 = z5 - z4 * F0_390;
    t0 += z1 + z3, t1 += z2 + z4, t2 += z2 + z3, t3 += z1 + z4;
    const uint32_t r = 1u << (shift - 1);
    out[0] = (int32_t)(t10 + t3 + r) >> shift, out[7] = (int32_t)(t10 - t3 + r) >> shift;
    out[1] = (int32_t)(t11 + t2 + r) >> shift, out[6] = (int32_t)(t11 - t2 + r) >> shift;
    out[2] = (int32_t)(t12 + t1 + r) >> shift, out[5] = (int32_t)(t12 - t1 + r) >> shift;
    out[3] = (int32_t)(t13 + t0 + r) >> shift, out[4] = (int32_t)(t13 - t0 + r) >> shift;
}

__global__ __launch_bounds__(256) void jpegdec_idct_kernel(const int16_t* __restrict__ coef, const int32_t* __restrict__ tab,
                                                           uint8_t* __restrict__ planes, Geom g, int64_t n_blocks) {
    __shared__ int32_t s_q[192];
    if (threadIdx.x < 192) s_q[threadIdx.x] = tab[kTabQuant + threadIdx.x] & 255;
    __syncthreads();
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= n_blocks) return;
    const int64_t bpf = (int64_t)g.mx * g.my * g.bpm;
    const int64_t f = b / bpf;
    const int64_t r = b - f * bpf;
    const int mcu = (int)(r / g.bpm), j = (int)(r - (int64_t)mcu * g.bpm);
    const int my = mcu / g.mx, mx = mcu - my * g.mx;
    const int luma = g.ncomp == 1 ? 1 : g.hs * g.vs;
    int comp, x0, y0, pw;
    uint8_t* plane = planes + f * plane_bytes(g);
    if (j < luma) {
        comp = 0, pw = g.yw;
        x0 = (mx * g.hs + j % g.hs) * 8, y0 = (my * g.vs + j / g.hs) * 8;
    } else {
        comp = j - luma + 1, pw = g.cw;
        x0 = mx * 8, y0 = my * 8;
        plane += (int64_t)g.yw * g.yh + (int64_t)(comp - 1) * g.cw * g.ch;
    }
    const int32_t* q = &s_q[comp * 64];
    uint32_t c[32];
    const u32x4* p = (const u32x4*)(coef + b * 64);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const u32x4 v = p[i];
        c[4 * i] = v[0], c[4 * i + 1] = v[1], c[4 * i + 2] = v[2], c[4 * i + 3] = v[3];
    }
    int32_t ws[64];                                                          // [row][col] after the column pass
#pragma unroll
    for (int x = 0; x < 8; ++x) {
        uint32_t in[8];
        int32_t o[8];
#pragma unroll
        for (int y = 0; y < 8; ++y) {
            const int k = y * 8 + x;
            in[y] = (uint32_t)((int32_t)(int16_t)((c[k >> 1] >> (16 * (k & 1))) & 0xffffu) * q[k]);
        }
        idct_pass(in, o, 11);
#pragma unroll
        for (int y = 0; y < 8; ++y) ws[y * 8 + x] = o[y];
    }
#pragma unroll
    for (int y = 0; y < 8; ++y) {
        uint32_t in[8];
        int32_t o[8];
#pragma unroll
        for (int x = 0; x < 8; ++x) in[x] = (uint32_t)ws[y * 8 + x];
        idct_pass(in, o, 18);
        uint32_t w[2] = {0u, 0u};
#pragma unroll
        for (int x = 0; x < 8; ++x) {
            int v = (int)(((uint32_t)o[x] & 1023u) ^ 512u) - 512 + 128;       // the low 10 bits, signed; + 128
            v = v < 0 ? 0 : (v > 255 ? 255 : v);
            w[x >> 2] |= (uint32_t)v << (8 * (x & 3));
        }
        u32x2 st;
        st[0] = w[0], st[1] = w[1];
        *(u32x2*)(plane + (int64_t)(y0 + y) * pw + x0) = st;                  // 8-byte aligned: pw and x0 are multiples of 8, so are the planes
    }
}

// ---- colour: a thread per pixel
__device__ __forceinline__ int chroma_at(const uint8_t* __restrict__ p, int pw, int cw, int ch, int hs, int vs, int x, int y) {
    if (hs == 1) return p[(int64_t)y * pw + x];
    const int i = x >> 1;
    if (cw <= 2) return p[(int64_t)(vs == 2 ? y >> 1 : y) * pw + i];             // libjpeg replicates such narrow planes
    if (vs == 1) {
        const uint8_t* row = p + (int64_t)y * pw;
        const int a = row[i];
        if (x & 1) return i == cw - 1 ? a : (3 * a + row[i + 1] + 2) >> 2;
        return i == 0 ? a : (3 * a + row[i - 1] + 1) >> 2;
    }
    const int r = y >> 1;
    const int far = (y & 1) ? (r + 1 < ch ? r + 1 : r) : (r > 0 ? r - 1 : r);   // the row above the first is the first, below the last the last
    const uint8_t* near_row = p + (int64_t)r * pw;
    const uint8_t* far_row = p + (int64_t)far * pw;
    const int a = 3 * near_row[i] + far_row[i];
    if (x & 1) return i == cw - 1 ? (4 * a + 7) >> 4 : (3 * a + 3 * near_row[i + 1] + far_row[i + 1] + 7) >> 4;
    return i == 0 ? (4 * a + 8) >> 4 : (3 * a + 3 * near_row[i - 1] + far_row[i - 1] + 8) >> 4;
}

__global__ __launch_bounds__(256) void jpegdec_rgb_kernel(const uint8_t* __restrict__ planes, uint8_t* __restrict__ out, Geom g, int64_t n_pixels) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pixels) return;
    const int64_t per = (int64_t)g.H * g.W;
    const int64_t f = i / per;
    const int64_t r = i - f * per;
    const int y = (int)(r / g.W), x = (int)(r - (int64_t)y * g.W);
    const uint8_t* pl = planes + f * plane_bytes(g);
    const int Y = pl[(int64_t)y * g.yw + x];
    int R = Y, G = Y, B = Y;
    if (g.ncomp == 3) {
        const int cwr = (g.W + g.hs - 1) / g.hs, chr = (g.H + g.vs - 1) / g.vs;  // the chroma planes' real size
        const uint8_t* pcb = pl + (int64_t)g.yw * g.yh;
        const uint8_t* pcr = pcb + (int64_t)g.cw * g.ch;
        const int cb = chroma_at(pcb, g.cw, cwr, chr, g.hs, g.vs, x, y) - 128;
        const int cr = chroma_at(pcr, g.cw, cwr, chr, g.hs, g.vs, x, y) - 128;
        R = Y + ((91881 * cr + 32768) >> 16);
        G = Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16);
        B = Y + ((116130 * cb + 32768) >> 16);
        R = R < 0 ? 0 : (R > 255 ? 255 : R);
        G = G < 0 ? 0 : (G > 255 ? 255 : G);
        B = B < 0 ? 0 : (B > 255 ? 255 : B);
    }
    uint8_t* o = out + i * 3;
    o[0] = (uint8_t)R, o[1] = (uint8_t)G, o[2] = (uint8_t)B;
}

}  // namespace

// ------------------------------------------------------------------------------------------
// launchers (arguments validated by the entry points in core.cpp)
// ------------------------------------------------------------------------------------------
int64_t cc_jpegdec_plane_bytes(int32_t H, int32_t W, int32_t ncomp, int32_t hs, int32_t vs) { return plane_bytes(make_geom(H, W, ncomp, hs, vs)); }

int64_t cc_jpegdec_blocks(int32_t H, int32_t W, int32_t ncomp, int32_t hs, int32_t vs) {
    const Geom g = make_geom(H, W, ncomp, hs, vs);
    return (int64_t)g.mx * g.my * g.bpm;
}

int64_t cc_jpegdec_intervals(int32_t H, int32_t W, int32_t ncomp, int32_t hs, int32_t vs, int32_t restart_interval) {
    const Geom g = make_geom(H, W, ncomp, hs, vs);
    const int64_t mcus = (int64_t)g.mx * g.my;
    return restart_interval > 0 ? (mcus + restart_interval - 1) / restart_interval : 1;
}

int cc_jpegdec_entropy(const uint8_t* data, int64_t data_bytes, const int64_t* intervals, const int32_t* tab, int16_t* coef, int32_t* status,
                       int32_t N, int32_t H, int32_t W, int32_t ncomp, int32_t hs, int32_t vs, int32_t restart_interval, hipStream_t s) {
    const Geom g = make_geom(H, W, ncomp, hs, vs);
    const int64_t mcus = (int64_t)g.mx * g.my;
    const int64_t per_frame = cc_jpegdec_intervals(H, W, ncomp, hs, vs, restart_interval);
    const int64_t n_iv = per_frame * N;
    hipError_t e = hipMemsetAsync(coef, 0, (size_t)(N * mcus * g.bpm * 128), s);  // the core writes non-zero coefficients only
    if (e != hipSuccess) {
        cc_set_error("jpegdec_entropy: hipMemsetAsync: %s", hipGetErrorString(e));
        return (int)e;
    }
    // As few decoding lanes per wave as still give <= 2048 waves: lanes of one wave diverge, so the expectation is that a wave costs
    // what its slowest lane costs.  An expectation, not a tuned rule: it was timed only where it puts a 113-frame 512 x 768 clip
    // (4 lanes for 32 intervals per frame, 1 lane for files without restart markers); no other lane count was tried.
    int lanes = 1;
    while (lanes < 64 && (n_iv + lanes - 1) / lanes > 2048) lanes *= 4;
    hipLaunchKernelGGL(jpegdec_entropy_kernel, dim3((unsigned)((n_iv + lanes - 1) / lanes)), dim3(64), 0, s, data, data_bytes, intervals, tab, coef,
                       status, n_iv, (int)per_frame, mcus, restart_interval > 0 ? (int64_t)restart_interval : mcus, ncomp, g.hs * g.vs, lanes);
    return cc_launch_status("jpegdec_entropy");
}

int cc_jpegdec_idct(const int16_t* coef, const int32_t* tab, uint8_t* planes, int32_t N, int32_t H, int32_t W, int32_t ncomp, int32_t hs,
                    int32_t vs, hipStream_t s) {
    const Geom g = make_geom(H, W, ncomp, hs, vs);
    const int64_t n = (int64_t)N * g.mx * g.my * g.bpm;
    hipLaunchKernelGGL(jpegdec_idct_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, coef, tab, planes, g, n);
    return cc_launch_status("jpegdec_idct");
}

int cc_jpegdec_rgb(const uint8_t* planes, uint8_t* out, int32_t N, int32_t H, int32_t W, int32_t ncomp, int32_t hs, int32_t vs, hipStream_t s) {
    const Geom g = make_geom(H, W, ncomp, hs, vs);
    const int64_t n = (int64_t)N * H * W;
    hipLaunchKernelGGL(jpegdec_rgb_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, planes, out, g, n);
    return cc_launch_status("jpegdec_rgb");
}
