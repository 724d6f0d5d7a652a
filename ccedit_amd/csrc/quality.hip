// Quality report (include/ccedit_hip.h, "Quality report"): fidelity of a result to its source and warp error of a clip along the
// source's motion (ccedit_amd/quality.py; `--report_quality`).  Two reductions over uint8 frames into uint64 accumulators:
//   quality_pair   per frame: squared error per channel, luma sums and pixel count over the kept pixels, and the sum of the fixed-point
//                  SSIM quotient q over the 8 x 8 windows at stride 4 all of whose pixels are kept
//   quality_warp   per measurement (f, g): squared error of x_f(p) against x_g(q), q = clamp(p + v(p)), over the selected pixels that
//                  land inside frame g and whose way back r(q) agrees with v(p) within `limit` (the test of masktrack_step)
// Everything is integer arithmetic; the sums do not depend on the order of summation, so the 64-bit atomics leave them exact.  Both
// equal tests/_quality_numpy.py bit for bit; the file is compiled with -ffp-contract=off -fno-slp-vectorize like the other bit-exact
// files (there is no floating point in it).
//
// quality_pair: a workgroup owns a tile of 16 x 16 CELLS of 4 x 4 pixels (64 x 64 pixels).  A window at stride 4 is 2 x 2 cells, so
// the tile's windows need one more cell row and column: 17 x 17 cells are formed, one thread per cell and round, straight from
// global memory (a cell row is 12 bytes of a frame: three aligned dwords; neighbouring threads read neighbouring cells).  A cell
// leaves its five luma sums and "all 16 pixels kept" in LDS; the squared errors, the count and the luma sums of the kept pixels are
// taken from the tile's own 16 x 16 cells only, so every pixel is counted once.  Then a thread per window adds four cells, forms q
// by a 0 / 1 integer part and 32 shift-subtract steps (no floating-point divide), and the eight sums go through the wave by
// cross-lane moves, through LDS across the four waves, and to memory as one 64-bit atomicAdd per accumulator and workgroup.
//
// quality_warp: a thread per four consecutive pixels of a row, grid-stride inside one measurement (blockIdx.y), the same reduction.
// The pair list and the per-pixel vectors are device data: frame numbers are clamped into the clip and q into the frame, so nothing
// read from them can take an access outside a tensor.  The argument checks live with the exported entry points in core.cpp.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTile = 16;                    // cells per tile side
constexpr int kSide = kTile + 1;             // ... plus the cell row / column the last windows reach into
constexpr int kWarpBlocks = 256;             // most workgroups per measurement
constexpr int64_t kC1 = 26634;               // (0.01 * 255)^2 * 4096, rounded   (ccedit_amd/quality.py C1, C2)
constexpr int64_t kC2 = 239708;              // (0.03 * 255)^2 * 4096, rounded

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ uint32_t luma_of(uint32_t r, uint32_t g, uint32_t b) { return (77u * r + 150u * g + 29u * b + 128u) >> 8; }

__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int o) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, 64);
    return (uint64_t)hi << 32 | lo;
}

// the workgroup's sums of v[0 .. K) -> acc[0 .. K): every thread of the workgroup calls it (shuffles and a barrier)
template <int K>
__device__ __forceinline__ void reduce_to(uint64_t (&v)[K], uint64_t (*s_red)[K], unsigned long long* acc) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[k] += shfl_xor64(v[k], o);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) s_red[wave][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < K) {
        uint64_t t = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) t += s_red[w][threadIdx.x];
        if (t) atomicAdd(acc + threadIdx.x, (unsigned long long)t);
    }
}

// q = sign(nw) floor(|nw| 2^32 / dw), |nw| <= dw, 0 < dw < 2^63: the integer part is 0 or 1, the 32 fraction bits by shift and subtract
__device__ __forceinline__ int64_t quotient32(int64_t nw, uint64_t dw) {
    const bool neg = nw < 0;
    uint64_t rem = neg ? (uint64_t)(-nw) : (uint64_t)nw;
    uint64_t q = rem >= dw ? 1u : 0u;
    rem -= q ? dw : 0u;
#pragma unroll 4
    for (int i = 0; i < 32; ++i) {
        rem <<= 1;                                                     // rem < dw < 2^63: no bit is lost
        const bool bit = rem >= dw;
        rem -= bit ? dw : 0u;
        q = q << 1 | (bit ? 1u : 0u);
    }
    return neg ? -(int64_t)q : (int64_t)q;
}

__global__ __launch_bounds__(kThreads) void quality_pair_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                                const uint8_t* __restrict__ mask, unsigned long long* __restrict__ acc, int H, int W,
                                                                int tilesX) {
    __shared__ uint32_t s_cell[kSide * kSide][6];                      // s1, s2, saa, sbb, sab, all kept
    __shared__ uint64_t s_red[kWaves][8];
    const int n = blockIdx.y;
    const int ty = blockIdx.x / tilesX, tx = blockIdx.x - ty * tilesX;
    const int cellsY = H / 4, cellsX = W / 4;
    const int cy0 = ty * kTile, cx0 = tx * kTile;
    const uint8_t* fa = a + (int64_t)n * H * W * 3;
    const uint8_t* fb = b + (int64_t)n * H * W * 3;
    const uint8_t* fm = mask ? mask + (int64_t)n * H * W : nullptr;
    uint32_t sse[3] = {0, 0, 0}, cnt = 0, la = 0, lb = 0;              // per thread at most two cells: 32 pixels
    for (int c = threadIdx.x; c < kSide * kSide; c += kThreads) {
        const int ly = c / kSide, lx = c - ly * kSide;
        const int cy = cy0 + ly, cx = cx0 + lx;
        uint32_t s1 = 0, s2 = 0, saa = 0, sbb = 0, sab = 0, all = 0;
        if (cy < cellsY && cx < cellsX) {
            const bool own = ly < kTile && lx < kTile;
            all = 1;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t px = (int64_t)(cy * 4 + r) * W + cx * 4;
                const uint32_t* pa = (const uint32_t*)(fa + px * 3);
                const uint32_t* pb = (const uint32_t*)(fb + px * 3);
                const uint32_t wa[3] = {pa[0], pa[1], pa[2]}, wb[3] = {pb[0], pb[1], pb[2]};
                const uint32_t m4 = fm ? *(const uint32_t*)(fm + px) : 0u;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    uint32_t ca[3], cb[3];
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        const int byte = 3 * j + ch;
                        ca[ch] = (wa[byte >> 2] >> (8 * (byte & 3))) & 255u;
                        cb[ch] = (wb[byte >> 2] >> (8 * (byte & 3))) & 255u;
                    }
                    const uint32_t ya = luma_of(ca[0], ca[1], ca[2]), yb = luma_of(cb[0], cb[1], cb[2]);
                    s1 += ya, s2 += yb, saa += ya * ya, sbb += yb * yb, sab += ya * yb;
                    const bool kept = ((m4 >> (8 * j)) & 255u) < 128u;
                    all &= kept ? 1u : 0u;
                    if (own && kept) {
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch) {
                            const int d = (int)ca[ch] - (int)cb[ch];
                            sse[ch] += (uint32_t)(d * d);
                        }
                        ++cnt, la += ya, lb += yb;
                    }
                }
            }
        }
        uint32_t* o = s_cell[c];
        o[0] = s1, o[1] = s2, o[2] = saa, o[3] = sbb, o[4] = sab, o[5] = all;
    }
    __syncthreads();
    uint64_t v[8] = {sse[0], sse[1], sse[2], cnt, 0, 0, la, lb};
    {
        const int ly = threadIdx.x / kTile, lx = threadIdx.x - ly * kTile;           // the window whose top-left cell is (ly, lx)
        if (cy0 + ly + 1 < cellsY && cx0 + lx + 1 < cellsX) {
            const uint32_t* c00 = s_cell[ly * kSide + lx];
            const uint32_t* c01 = c00 + 6;
            const uint32_t* c10 = c00 + 6 * kSide;
            const uint32_t* c11 = c10 + 6;
            if (c00[5] & c01[5] & c10[5] & c11[5]) {
                const int64_t s1 = c00[0] + c01[0] + c10[0] + c11[0], s2 = c00[1] + c01[1] + c10[1] + c11[1];
                const int64_t saa = c00[2] + c01[2] + c10[2] + c11[2], sbb = c00[3] + c01[3] + c10[3] + c11[3];
                const int64_t sab = c00[4] + c01[4] + c10[4] + c11[4];
                const int64_t va = 64 * saa - s1 * s1, vb = 64 * sbb - s2 * s2, cov = 64 * sab - s1 * s2;
                const int64_t nw = (2 * s1 * s2 + kC1) * (2 * cov + kC2);
                const uint64_t dw = (uint64_t)((s1 * s1 + s2 * s2 + kC1) * (va + vb + kC2));      // >= c1 c2 > 0
                v[4] = (uint64_t)quotient32(nw, dw);                                           // (two's complement: the sum wraps to the exact int64)
                v[5] = 1;
            }
        }
    }
    reduce_to<8>(v, s_red, acc + (int64_t)n * 8);
}

// x, y: [F][H][W][3]; vsel: packed int16 (dy, dx) [2 P][H][W]; acc [P][4] = (SSE x, SSE y, valid, selected)
__global__ __launch_bounds__(kThreads) void quality_warp_kernel(const uint8_t* __restrict__ x, const uint8_t* __restrict__ y,
                                                                const uint32_t* __restrict__ vsel, const int32_t* __restrict__ pairs,
                                                                const uint8_t* __restrict__ mask, unsigned long long* __restrict__ acc, int F, int H,
                                                                int W, int limit, int sel) {
    __shared__ uint64_t s_red[kWaves][4];
    const int j = blockIdx.y;
    const int f = clampi(pairs[8 * j], 0, F - 1), g = clampi(pairs[8 * j + 1], 0, F - 1);
    const int64_t HW = (int64_t)H * W;
    const uint32_t* v = vsel + (int64_t)(2 * j) * HW;
    const uint32_t* r = v + HW;
    const uint8_t* xf = x + (int64_t)f * HW * 3;
    const uint8_t* xg = x + (int64_t)g * HW * 3;
    const uint8_t* yf = y ? y + (int64_t)f * HW * 3 : nullptr;
    const uint8_t* yg = y ? y + (int64_t)g * HW * 3 : nullptr;
    const uint8_t* mf = sel ? mask + (int64_t)f * HW : nullptr;
    const int G = W / 4;
    const int total = H * G;
    uint64_t s[4] = {0, 0, 0, 0};
    for (int idx = blockIdx.x * kThreads + threadIdx.x; idx < total; idx += gridDim.x * kThreads) {
        const int py = idx / G, x0 = (idx - py * G) * 4;
        const int64_t p0 = (int64_t)py * W + x0;
        const u32x4 v4 = *(const u32x4*)(v + p0);
        const uint32_t m4 = mf ? *(const uint32_t*)(mf + p0) : 0u;
        const uint32_t* px = (const uint32_t*)(xf + p0 * 3);
        const uint32_t wx[3] = {px[0], px[1], px[2]};
        uint32_t wy[3] = {0, 0, 0};
        if (yf) {
            const uint32_t* q = (const uint32_t*)(yf + p0 * 3);
            wy[0] = q[0], wy[1] = q[1], wy[2] = q[2];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool edit = ((m4 >> (8 * k)) & 255u) >= 128u;
            if (sel == 0 || (sel == 1) == edit) {
                ++s[3];
                const int vy = (int)(int16_t)(v4[k] & 0xffffu), vx = (int)(int16_t)(v4[k] >> 16);
                const int qy0 = py + vy, qx0 = x0 + k + vx;
                const bool inside = qy0 >= 0 && qy0 < H && qx0 >= 0 && qx0 < W;
                const int64_t q = (int64_t)clampi(qy0, 0, H - 1) * W + clampi(qx0, 0, W - 1);
                const uint32_t rq = r[q];
                int ey = vy + (int)(int16_t)(rq & 0xffffu), ex = vx + (int)(int16_t)(rq >> 16);
                ey = ey < 0 ? -ey : ey, ex = ex < 0 ? -ex : ex;
                if (inside && ey + ex <= limit) {
                    ++s[2];
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        const int byte = 3 * k + ch;
                        const int d = (int)((wx[byte >> 2] >> (8 * (byte & 3))) & 255u) - (int)xg[q * 3 + ch];
                        s[0] += (uint32_t)(d * d);
                        if (yf) {
                            const int e = (int)((wy[byte >> 2] >> (8 * (byte & 3))) & 255u) - (int)yg[q * 3 + ch];
                            s[1] += (uint32_t)(e * e);
                        }
                    }
                }
            }
        }
    }
    reduce_to<4>(s, s_red, acc + (int64_t)j * 4);
}

int memset_status(const char* what, void* p, size_t bytes, hipStream_t s) {
    const hipError_t e = hipMemsetAsync(p, 0, bytes, s);
    if (e != hipSuccess) {
        cc_set_error("%s: hipMemsetAsync: %s", what, hipGetErrorString(e));
        return (int)e;
    }
    return CCEDIT_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------
// launchers (arguments validated by the entry points in core.cpp); both zero their accumulators on the stream first
// ------------------------------------------------------------------------------------------
int cc_quality_pair(const uint8_t* a, const uint8_t* b, const uint8_t* mask, uint64_t* acc, int64_t N, int32_t H, int32_t W, hipStream_t s) {
    if (int rc = memset_status("quality_pair", acc, (size_t)N * 8 * sizeof(uint64_t), s)) return rc;
    const int tilesY = (H / 4 + kTile - 1) / kTile, tilesX = (W / 4 + kTile - 1) / kTile;
    hipLaunchKernelGGL(quality_pair_kernel, dim3((unsigned)(tilesY * tilesX), (unsigned)N), dim3(kThreads), 0, s, a, b, mask,
                       (unsigned long long*)acc, H, W, tilesX);
    return cc_launch_status("quality_pair");
}

int cc_quality_warp(const uint8_t* x, const uint8_t* y, const uint32_t* vsel, const int32_t* pairs, const uint8_t* mask, uint64_t* acc, int32_t P,
                    int32_t F, int32_t H, int32_t W, int32_t limit, int32_t sel, hipStream_t s) {
    if (int rc = memset_status("quality_warp", acc, (size_t)P * 4 * sizeof(uint64_t), s)) return rc;
    const int64_t groups = ((int64_t)H * (W / 4) + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(quality_warp_kernel, dim3((unsigned)(groups < kWarpBlocks ? groups : kWarpBlocks), (unsigned)P), dim3(kThreads), 0, s, x,
                       y, vsel, pairs, mask, (unsigned long long*)acc, F, H, W, limit, sel);
    return cc_launch_status("quality_warp");
}
