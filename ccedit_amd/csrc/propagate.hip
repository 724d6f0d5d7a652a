// Full-frame-rate output (include/ccedit_hip.h, "Propagation"): the edited keyframes are carried to every source frame between them
// along motion estimated on the SOURCE frames (ccedit_amd/propagate.py; `--propagate`).  All integer work on bytes:
//   prop_pyramid   RGB frames -> luma (77 R + 150 G + 29 B + 128) >> 8 and three rounded 2 x 2 means, all four levels in one pass
//   prop_match     one pyramid level, all pairs of the call: per 8 x 8 block the vector of the minimum (SAD, rank) over the 16 x 16
//                  patch (block + 4-pixel apron, coordinates clamped), searched +-R around twice the parent block's vector
//   prop_warp      per-pixel flow in 1/16 pixel interpolated from the block vectors in the kernel, then a bilinear sample with
//                  4-bit fractions; 3 channels (edited keyframes) or 1 (source luma)
//   prop_blend     |warped luma - frame luma| -> 5 x 5 box mean -> confidence table -> weighted mean of the two warped keyframes
//                  (+ optionally the source put back where the frame's own mask is clear)
// Every kernel equals tests/_propagate_numpy.py bit for bit; the file is compiled with -ffp-contract=off -fno-slp-vectorize like
// the other bit-exact files (there is no floating point in it).
//
// prop_match is the hot path.  A block's key window ((16 + 2R) rows of 28 bytes, clamped at the image border while it is staged) and
// its reference patch live in LDS as bytes; ONE LANE PER CANDIDATE walks the 16 rows: a row of the patch is one 16-byte LDS read that
// all lanes of the block share, the shifted key row is five dwords realigned by v_alignbyte_b32, and v_sad_u8 accumulates four pixels
// per instruction.  The lanes' packed keys (SAD << 16 | rank << 8 | candidate) are reduced with a min across the lanes: no atomics,
// the result independent of evaluation order.  R <= 2 (25 candidates): 32 lanes per block, two blocks per wave; R <= 4: one block per wave.
//
// The pair list, the rank / confidence tables and the parent vectors are device data the host cannot check per launch: frame indices
// are clamped into their tensors, table values into their ranges, vectors into +-32 (matching) / +-4096 (warping), so that nothing
// read from them can take an access outside a tensor.  The argument checks live with the exported entry points in core.cpp.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 256 * 8;          // 256 CUs x 8 workgroups of 4 waves
constexpr int kKeyStride = 7;                // dwords per staged key row: 16 + 2 * 4 bytes + the dword v_alignbyte_b32 shifts in
constexpr int kKeyRows = 24;                 // 16 + 2 * 4

inline unsigned grid_for(int64_t items) {
    const int64_t g = (items + kThreads - 1) / kThreads;
    return (unsigned)(g < 1 ? 1 : (g > kMaxBlocks ? kMaxBlocks : g));
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- pyramid: one thread per 8 x 8 block of level 0 = 4 x 4 of level 1 = 2 x 2 of level 2 = one pixel of level 3.
__global__ __launch_bounds__(kThreads) void prop_pyramid_kernel(const uint8_t* __restrict__ rgb, uint8_t* __restrict__ pyr, int F, int H, int W) {
    const int nbx = W / 8, nby = H / 8;
    const int64_t total = (int64_t)F * nby * nbx;
    const int64_t o1 = (int64_t)F * H * W, o2 = o1 + o1 / 4, o3 = o2 + o1 / 16;
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * kThreads) {
        const int bx = (int)(idx % nbx);
        const int64_t r = idx / nbx;
        const int by = (int)(r % nby), f = (int)(r / nby);
        uint32_t l0[8][8];
        const uint8_t* base = rgb + (((int64_t)f * H + by * 8) * W + bx * 8) * 3;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint32_t* row = (const uint32_t*)(base + (int64_t)i * W * 3);           // 24 bytes, 4-byte aligned (W % 64 == 0)
            uint32_t d[6];
#pragma unroll
            for (int q = 0; q < 6; ++q) d[q] = row[q];
#pragma unroll
            for (int x = 0; x < 8; ++x) {
                uint32_t c[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const int b = x * 3 + k;
                    c[k] = (d[b >> 2] >> (8 * (b & 3))) & 255u;
                }
                l0[i][x] = (77u * c[0] + 150u * c[1] + 29u * c[2] + 128u) >> 8;
            }
            uint8_t* o = pyr + ((int64_t)f * H + by * 8 + i) * W + bx * 8;
            *(u32x2*)o = u32x2{l0[i][0] | (l0[i][1] << 8) | (l0[i][2] << 16) | (l0[i][3] << 24),
                               l0[i][4] | (l0[i][5] << 8) | (l0[i][6] << 16) | (l0[i][7] << 24)};
        }
        uint32_t l1[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int x = 0; x < 4; ++x) l1[i][x] = (l0[2 * i][2 * x] + l0[2 * i][2 * x + 1] + l0[2 * i + 1][2 * x] + l0[2 * i + 1][2 * x + 1] + 2u) >> 2;
            uint8_t* o = pyr + o1 + ((int64_t)f * (H / 2) + by * 4 + i) * (W / 2) + bx * 4;
            *(uint32_t*)o = l1[i][0] | (l1[i][1] << 8) | (l1[i][2] << 16) | (l1[i][3] << 24);
        }
        uint32_t l2[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
            for (int x = 0; x < 2; ++x) l2[i][x] = (l1[2 * i][2 * x] + l1[2 * i][2 * x + 1] + l1[2 * i + 1][2 * x] + l1[2 * i + 1][2 * x + 1] + 2u) >> 2;
            uint8_t* o = pyr + o2 + ((int64_t)f * (H / 4) + by * 2 + i) * (W / 4) + bx * 2;
            *(uint16_t*)o = (uint16_t)(l2[i][0] | (l2[i][1] << 8));
        }
        pyr[o3 + ((int64_t)f * (H / 8) + by) * (W / 8) + bx] = (uint8_t)((l2[0][0] + l2[0][1] + l2[1][0] + l2[1][1] + 2u) >> 2);
    }
}

// ---- block matching on one level (lum: that level of all F frames, h x w each).  Four waves per workgroup, each with its own LDS
// slots; a wave whose blocks lie beyond the last one only takes part in the barrier.
__global__ __launch_bounds__(kThreads) void prop_match_kernel(const uint8_t* __restrict__ lum, const int32_t* __restrict__ pairs,
                                                              const int32_t* __restrict__ rank, const int32_t* __restrict__ parent,
                                                              int32_t* __restrict__ out, int P, int F, int h, int w, int R) {
    __shared__ uint32_t s_key[8][kKeyRows * kKeyStride];
    __shared__ __attribute__((aligned(16))) uint32_t s_ref[8][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lpb = R <= 2 ? 32 : 64;                    // lanes per block
    const int bpw = 64 / lpb;                            // blocks per wave
    const int sub = lane / lpb, sl = lane - sub * lpb;
    const int slot = wave * 2 + sub;
    const int nby = h / 8, nbx = w / 8;
    const int n = 2 * R + 1, ncand = n * n;
    const int64_t NB = (int64_t)P * nby * nbx;
    const int64_t g = ((int64_t)blockIdx.x * 4 + wave) * bpw + sub;
    const bool live = g < NB;
    int py = 0, px = 0;
    if (live) {
        const int bx = (int)(g % nbx);
        const int64_t r = g / nbx;
        const int by = (int)(r % nby), p = (int)(r / nby);
        const int f = clampi(pairs[4 * p], 0, F - 1), k = clampi(pairs[4 * p + 1], 0, F - 1);
        if (parent) {
            const int32_t* pv = parent + (((int64_t)p * (nby / 2) + (by >> 1)) * (nbx / 2) + (bx >> 1)) * 2;
            py = 2 * clampi(pv[0], -32, 32);
            px = 2 * clampi(pv[1], -32, 32);
        }
        const uint8_t* yf = lum + (int64_t)f * h * w;
        const uint8_t* yk = lum + (int64_t)k * h * w;
        const int rows = 16 + 2 * R;
        const int oy = by * 8 - 4 + py - R, ox = bx * 8 - 4 + px - R;
        for (int i = sl; i < rows * kKeyStride; i += lpb) {
            const int rr = i / kKeyStride, c = i - rr * kKeyStride;
            const uint8_t* row = yk + (int64_t)clampi(oy + rr, 0, h - 1) * w;
            uint32_t v = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) v |= (uint32_t)row[clampi(ox + 4 * c + b, 0, w - 1)] << (8 * b);
            s_key[slot][i] = v;
        }
        for (int i = sl; i < 64; i += lpb) {
            const int rr = i >> 2, c = i & 3;
            const uint8_t* row = yf + (int64_t)clampi(by * 8 - 4 + rr, 0, h - 1) * w;
            uint32_t v = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) v |= (uint32_t)row[clampi(bx * 8 - 4 + 4 * c + b, 0, w - 1)] << (8 * b);
            s_ref[slot][i] = v;
        }
    }
    __syncthreads();
    uint32_t best = 0xffffffffu;
    if (live) {
        for (int cand = sl; cand < ncand; cand += lpb) {
            const int cy = cand / n, cx = cand - cy * n;              // dy + R, dx + R
            const int q = cx >> 2;
            const uint32_t sh = (uint32_t)(cx & 3);
            uint32_t sad = 0;
#pragma unroll 4
            for (int r = 0; r < 16; ++r) {
                const uint32_t* kr = &s_key[slot][(cy + r) * kKeyStride + q];
                const u32x4 rf = *(const u32x4*)&s_ref[slot][r * 4];
                const uint32_t k0 = kr[0], k1 = kr[1], k2 = kr[2], k3 = kr[3], k4 = kr[4];
                sad = __builtin_amdgcn_sad_u8(rf[0], __builtin_amdgcn_alignbyte(k1, k0, sh), sad);
                sad = __builtin_amdgcn_sad_u8(rf[1], __builtin_amdgcn_alignbyte(k2, k1, sh), sad);
                sad = __builtin_amdgcn_sad_u8(rf[2], __builtin_amdgcn_alignbyte(k3, k2, sh), sad);
                sad = __builtin_amdgcn_sad_u8(rf[3], __builtin_amdgcn_alignbyte(k4, k3, sh), sad);
            }
            const uint32_t key = (sad << 16) | ((uint32_t)clampi(rank[cand], 0, 255) << 8) | (uint32_t)cand;      // SAD <= 65280
            best = key < best ? key : best;
        }
    }
    for (int o = lpb >> 1; o > 0; o >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)best, o, 64);
        best = other < best ? other : best;
    }
    if (live && sl == 0) {
        const int cand = (int)(best & 127u);
        const int cy = cand / n;
        out[g * 2] = py + cy - R;
        out[g * 2 + 1] = px + (cand - cy * n) - R;
    }
}

// ---- warp: one thread per four consecutive pixels of a row (C dwords stored).  `col` selects the column of the pair row
// that names the source frame.
template <int C>
__global__ __launch_bounds__(kThreads) void prop_warp_kernel(const uint8_t* __restrict__ src, const int32_t* __restrict__ vec,
                                                             const int32_t* __restrict__ pairs, int col, uint8_t* __restrict__ out, int P, int Fsrc,
                                                             int H, int W) {
    const int G = W / 4, nby = H / 8, nbx = W / 8;
    const int64_t total = (int64_t)P * H * G;
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * kThreads) {
        const int x0 = (int)(idx % G) * 4;
        const int64_t r = idx / G;
        const int y = (int)(r % H), p = (int)(r / H);
        const int k = clampi(pairs[4 * p + col], 0, Fsrc - 1);
        const uint8_t* s = src + (int64_t)k * H * W * C;
        const int32_t* v = vec + (int64_t)p * nby * nbx * 2;
        const int ty = 2 * y - 7;
        const int by0 = clampi(ty >> 4, 0, nby - 1), by1 = clampi((ty >> 4) + 1, 0, nby - 1);
        const int wy1 = ty & 15, wy0 = 16 - wy1;
        uint32_t o[4 * C];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int x = x0 + j;
            const int tx = 2 * x - 7;
            const int bx0 = clampi(tx >> 4, 0, nbx - 1), bx1 = clampi((tx >> 4) + 1, 0, nbx - 1);
            const int wx1 = tx & 15, wx0 = 16 - wx1;
            int fl[2];
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                const int v00 = clampi(v[(by0 * nbx + bx0) * 2 + a], -4096, 4096), v01 = clampi(v[(by0 * nbx + bx1) * 2 + a], -4096, 4096);
                const int v10 = clampi(v[(by1 * nbx + bx0) * 2 + a], -4096, 4096), v11 = clampi(v[(by1 * nbx + bx1) * 2 + a], -4096, 4096);
                fl[a] = (wy0 * wx0 * v00 + wy0 * wx1 * v01 + wy1 * wx0 * v10 + wy1 * wx1 * v11 + 8) >> 4;
            }
            const int py = clampi(16 * y + fl[0], 0, 16 * (H - 1)), px = clampi(16 * x + fl[1], 0, 16 * (W - 1));
            const int sy0 = py >> 4, fy = py & 15, sx0 = px >> 4, fx = px & 15;
            const int sy1 = sy0 + 1 > H - 1 ? H - 1 : sy0 + 1, sx1 = sx0 + 1 > W - 1 ? W - 1 : sx0 + 1;
            const uint8_t* p00 = s + ((int64_t)sy0 * W + sx0) * C;
            const uint8_t* p01 = s + ((int64_t)sy0 * W + sx1) * C;
            const uint8_t* p10 = s + ((int64_t)sy1 * W + sx0) * C;
            const uint8_t* p11 = s + ((int64_t)sy1 * W + sx1) * C;
            const uint32_t w00 = (uint32_t)((16 - fy) * (16 - fx)), w01 = (uint32_t)((16 - fy) * fx), w10 = (uint32_t)(fy * (16 - fx)),
                           w11 = (uint32_t)(fy * fx);
#pragma unroll
            for (int c = 0; c < C; ++c) o[j * C + c] = (w00 * p00[c] + w01 * p01[c] + w10 * p10[c] + w11 * p11[c] + 128u) >> 8;
        }
        uint32_t* d = (uint32_t*)(out + (((int64_t)p * H + y) * W + x0) * C);
#pragma unroll
        for (int q = 0; q < C; ++q) d[q] = o[4 * q] | (o[4 * q + 1] << 8) | (o[4 * q + 2] << 16) | (o[4 * q + 3] << 24);
    }
}

// ---- blend: a workgroup per 16 x 64 tile of one in-between frame j (pairs 2 j: towards keyframe a, 2 j + 1: towards b).  The two
// error tiles with their 2-pixel border (coordinates clamped = edge replication) go to LDS, then the horizontal 5-sums, then every
// thread finishes four pixels of a row.
constexpr int kTileH = 16, kTileW = 64;
__global__ __launch_bounds__(kThreads) void prop_blend_kernel(const uint8_t* __restrict__ wE, const uint8_t* __restrict__ wY,
                                                              const uint8_t* __restrict__ lum, const int32_t* __restrict__ pairs,
                                                              const int32_t* __restrict__ gtab, const uint8_t* __restrict__ rgb,
                                                              const uint8_t* __restrict__ mask, uint8_t* __restrict__ out, int F, int H, int W) {
    __shared__ uint8_t s_err[2][kTileH + 4][kTileW + 4];
    __shared__ uint16_t s_h[2][kTileH + 4][kTileW];
    const int j = blockIdx.z, ty0 = blockIdx.y * kTileH, tx0 = blockIdx.x * kTileW, tid = threadIdx.x;
    const int f = clampi(pairs[8 * j], 0, F - 1);
    const uint32_t da = (uint32_t)clampi(pairs[8 * j + 3], 1, 255), db = (uint32_t)clampi(pairs[8 * j + 7], 1, 255);
    const uint8_t* yf = lum + (int64_t)f * H * W;
    constexpr int kE = (kTileH + 4) * (kTileW + 4);
    for (int i = tid; i < 2 * kE; i += kThreads) {
        const int s = i / kE, rem = i - s * kE;
        const int r = rem / (kTileW + 4), c = rem - r * (kTileW + 4);
        const int64_t at = (int64_t)clampi(ty0 - 2 + r, 0, H - 1) * W + clampi(tx0 - 2 + c, 0, W - 1);
        const int d = (int)wY[((int64_t)2 * j + s) * H * W + at] - (int)yf[at];
        s_err[s][r][c] = (uint8_t)(d < 0 ? -d : d);
    }
    __syncthreads();
    constexpr int kS = (kTileH + 4) * kTileW;
    for (int i = tid; i < 2 * kS; i += kThreads) {
        const int s = i / kS, rem = i - s * kS;
        const int r = rem / kTileW, c = rem - r * kTileW;
        const uint8_t* e = &s_err[s][r][c];
        s_h[s][r][c] = (uint16_t)(e[0] + e[1] + e[2] + e[3] + e[4]);
    }
    __syncthreads();
    const int row = tid >> 4, cx = (tid & 15) * 4;
    const int y = ty0 + row;
    const int64_t px0 = (int64_t)y * W + tx0 + cx;                       // first of the thread's four pixels within a frame
    const uint32_t* ea4 = (const uint32_t*)(wE + (((int64_t)2 * j) * H * W + px0) * 3);
    const uint32_t* eb4 = (const uint32_t*)(wE + (((int64_t)2 * j + 1) * H * W + px0) * 3);
    uint32_t A[3], B[3], S[3] = {0, 0, 0}, M = 0xffffffffu;
#pragma unroll
    for (int q = 0; q < 3; ++q) A[q] = ea4[q], B[q] = eb4[q];
    if (mask) {
        M = *(const uint32_t*)(mask + (int64_t)f * H * W + px0);
        const uint32_t* s4 = (const uint32_t*)(rgb + ((int64_t)f * H * W + px0) * 3);
#pragma unroll
        for (int q = 0; q < 3; ++q) S[q] = s4[q];
    }
    uint32_t o[12];
#pragma unroll
    for (int x = 0; x < 4; ++x) {
        uint32_t sa = 0, sb = 0;
#pragma unroll
        for (int i = 0; i < 5; ++i) sa += s_h[0][row + i][cx + x], sb += s_h[1][row + i][cx + x];
        const uint32_t ea = (sa + 12u) / 25u, eb = (sb + 12u) / 25u;
        const uint32_t wa = da * (uint32_t)clampi(gtab[ea > 255u ? 255u : ea], 1, 4096), wb = db * (uint32_t)clampi(gtab[eb > 255u ? 255u : eb], 1, 4096);
        const uint32_t den = wa + wb;
        const bool edit = ((M >> (8 * x)) & 255u) >= 128u;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int b = x * 3 + c;
            const uint32_t a8 = (A[b >> 2] >> (8 * (b & 3))) & 255u, b8 = (B[b >> 2] >> (8 * (b & 3))) & 255u, s8 = (S[b >> 2] >> (8 * (b & 3))) & 255u;
            const uint32_t v = (wa * a8 + wb * b8 + den / 2u) / den;            // <= 2 * 255 * 4096 * 255 + den / 2 < 2^31
            o[b] = edit ? v : s8;
        }
    }
    uint32_t* d = (uint32_t*)(out + ((int64_t)j * H * W + px0) * 3);
#pragma unroll
    for (int q = 0; q < 3; ++q) d[q] = o[4 * q] | (o[4 * q + 1] << 8) | (o[4 * q + 2] << 16) | (o[4 * q + 3] << 24);
}

}  // namespace

// ------------------------------------------------------------------------------------------
// launchers (arguments validated by the entry points in core.cpp)
// ------------------------------------------------------------------------------------------
int cc_prop_pyramid(const uint8_t* rgb, uint8_t* pyr, int32_t F, int32_t H, int32_t W, hipStream_t s) {
    hipLaunchKernelGGL(prop_pyramid_kernel, dim3(grid_for((int64_t)F * (H / 8) * (W / 8))), dim3(kThreads), 0, s, rgb, pyr, F, H, W);
    return cc_launch_status("prop_pyramid");
}

int cc_prop_match(const uint8_t* lum, const int32_t* pairs, const int32_t* rank, const int32_t* parent, int32_t* out, int32_t P, int32_t F,
                  int32_t h, int32_t w, int32_t R, hipStream_t s) {
    const int64_t per_wg = 4 * (R <= 2 ? 2 : 1);
    const int64_t NB = (int64_t)P * (h / 8) * (w / 8);
    hipLaunchKernelGGL(prop_match_kernel, dim3((unsigned)((NB + per_wg - 1) / per_wg)), dim3(kThreads), 0, s, lum, pairs, rank, parent, out, P, F, h, w, R);
    return cc_launch_status("prop_match");
}

int cc_prop_warp(const uint8_t* src, const int32_t* vec, const int32_t* pairs, int32_t col, uint8_t* out, int32_t P, int32_t Fsrc, int32_t H,
                 int32_t W, int32_t C, hipStream_t s) {
    const unsigned grid = grid_for((int64_t)P * H * (W / 4));
    if (C == 3)
        hipLaunchKernelGGL(prop_warp_kernel<3>, dim3(grid), dim3(kThreads), 0, s, src, vec, pairs, col, out, P, Fsrc, H, W);
    else
        hipLaunchKernelGGL(prop_warp_kernel<1>, dim3(grid), dim3(kThreads), 0, s, src, vec, pairs, col, out, P, Fsrc, H, W);
    return cc_launch_status("prop_warp");
}

int cc_prop_blend(const uint8_t* wE, const uint8_t* wY, const uint8_t* lum, const int32_t* pairs, const int32_t* gtab, const uint8_t* rgb,
                  const uint8_t* mask, uint8_t* out, int32_t NF, int32_t F, int32_t H, int32_t W, hipStream_t s) {
    hipLaunchKernelGGL(prop_blend_kernel, dim3(W / kTileW, H / kTileH, NF), dim3(kThreads), 0, s, wE, wY, lum, pairs, gtab, rgb, mask, out, F, H, W);
    return cc_launch_status("prop_blend");
}
