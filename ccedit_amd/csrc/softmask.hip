// Graded edit masks (include/ccedit_hip.h, "Graded edit masks"): a uint8 STRENGTH map in place of a binary mask, byte g = edit strength g / 255.
//   mask_feather          strength map -> its mean over the (2R + 1)^2 square, the window clipped at the frame border, rounded half up:
//                         (2 S + A) / (2 A) of the sum S and the pixel count A of the clipped window; two separable passes, row sums in
//                         uint16 (at most 129 * 255 = 32 895), column sums in uint32
//   mask_latent_graded    pixel strengths -> latent strengths: (sum of the 64 bytes of the 8 x 8 cell + 32) >> 6
//   mask_composite_graded out = g == 255 ? result : g == 0 ? original : original + (result - original) * (float(g) / 255.0f)
// The per-step re-injection of a graded run is mask.hip's mask_select_kernel with the caller's threshold (ccedit_inpaint_blend_level).
// All of them move bytes: grid-stride loops over a grid of at most kMaxBlocks workgroups, 16-byte accesses where sizes and alignment
// allow and a narrower variant otherwise.  Feather and latent strengths are integer arithmetic; the file is compiled with
// -ffp-contract=off: the composite is one correctly rounded divide, one subtract, one multiply and one add, as numpy's float32.
// The argument checks live with the exported entry points in core.cpp; the launchers below trust their arguments.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 256 * 8;          // 256 CUs x 8 workgroups of 4 waves

inline unsigned grid_for(int64_t items) {
    const int64_t g = (items + kThreads - 1) / kThreads;
    return (unsigned)(g < 1 ? 1 : (g > kMaxBlocks ? kMaxBlocks : g));
}
inline bool aligned(const void* p, unsigned a) { return ((uintptr_t)p & (a - 1)) == 0; }

// ---- feather, row pass: tmp[n][y][x] = sum of src[n][y][max(x - R, 0) ... min(x + R, W - 1)]; one thread per PX consecutive pixels of a
// row (W % PX == 0).  The first pixel's window is summed byte by byte, the next ones slide it: one byte in, one byte out.
// PX = 8: the eight sums as one 16-byte store; PX = 4: as two 4-byte stores.
template <int PX>
__global__ __launch_bounds__(kThreads) void feather_rows_kernel(const uint8_t* __restrict__ src, uint16_t* __restrict__ tmp, int64_t N, int H, int W,
                                                                int R) {
    const int G = W / PX;
    const int64_t total = N * H * G;
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * kThreads) {
        const int64_t ny = idx / G;                        // n * H + y
        const int x0 = (int)(idx - ny * G) * PX;
        const uint8_t* row = src + ny * W;
        const int lo = x0 - R < 0 ? 0 : x0 - R, hi = x0 + R > W - 1 ? W - 1 : x0 + R;
        uint32_t s[PX];
        uint32_t acc = 0;
        for (int xx = lo; xx <= hi; ++xx) acc += row[xx];
        s[0] = acc;
#pragma unroll
        for (int j = 1; j < PX; ++j) {
            const int in = x0 + j + R, out = x0 + j - 1 - R;
            if (in <= W - 1) acc += row[in];
            if (out >= 0) acc -= row[out];
            s[j] = acc;
        }
        uint32_t* o = (uint32_t*)(tmp + ny * W + x0);
        if constexpr (PX == 8) {
            *(u32x4*)o = u32x4{s[0] | (s[1] << 16), s[2] | (s[3] << 16), s[4] | (s[5] << 16), s[6] | (s[7] << 16)};
        } else {
            o[0] = s[0] | (s[1] << 16);
            o[1] = s[2] | (s[3] << 16);
        }
    }
}

// ---- feather, column pass: S = sum of tmp[n][max(y - R, 0) ... min(y + R, H - 1)][x] in uint32, A = rows x columns of the clipped window,
// dst = (2 S + A) / (2 A).  PX = 8: a 16-byte load per row and an 8-byte store; PX = 4: two 4-byte loads and a 4-byte store.
template <int PX>
__global__ __launch_bounds__(kThreads) void feather_cols_kernel(const uint16_t* __restrict__ tmp, uint8_t* __restrict__ dst, int64_t N, int H, int W,
                                                                int R) {
    const int G = W / PX;
    const int64_t total = N * H * G;
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * kThreads) {
        const int64_t ny = idx / G;
        const int x0 = (int)(idx - ny * G) * PX;
        const int64_t n = ny / H;
        const int y = (int)(ny - n * H);
        const uint16_t* img = tmp + n * H * W + x0;
        const int lo = y - R < 0 ? 0 : y - R, hi = y + R > H - 1 ? H - 1 : y + R;
        uint32_t s[PX];
#pragma unroll
        for (int j = 0; j < PX; ++j) s[j] = 0;
        for (int yy = lo; yy <= hi; ++yy) {
            const uint32_t* p = (const uint32_t*)(img + (int64_t)yy * W);
            uint32_t w[PX / 2];
            if constexpr (PX == 8) {
                const u32x4 v = *(const u32x4*)p;
                w[0] = v[0], w[1] = v[1], w[2] = v[2], w[3] = v[3];
            } else {
                w[0] = p[0], w[1] = p[1];
            }
#pragma unroll
            for (int j = 0; j < PX / 2; ++j) {
                s[2 * j] += w[j] & 0xffffu;
                s[2 * j + 1] += w[j] >> 16;
            }
        }
        const uint32_t rows = (uint32_t)(hi - lo + 1);
        uint32_t b[PX];
#pragma unroll
        for (int j = 0; j < PX; ++j) {
            const int x = x0 + j;
            const int xl = x - R < 0 ? 0 : x - R, xh = x + R > W - 1 ? W - 1 : x + R;
            const uint32_t A = rows * (uint32_t)(xh - xl + 1);
            b[j] = (2u * s[j] + A) / (2u * A);                      // at most 255: S <= 255 A
        }
        uint32_t* o = (uint32_t*)(dst + ny * W + x0);
        if constexpr (PX == 8) {
            *(u32x2*)o = u32x2{b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24), b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24)};
        } else {
            o[0] = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
        }
    }
}

// the four bytes of a word, summed
__device__ inline uint32_t byte_sum(uint32_t w) {
    const uint32_t t = (w & 0x00ff00ffu) + ((w >> 8) & 0x00ff00ffu);
    return (t & 0xffffu) + (t >> 16);
}

// ---- pixel strengths [N][H][W] -> latent strengths [N][H/8][W/8]: (sum of the cell's 64 bytes + 32) >> 6.  CELLS = 2: a 16-byte load per
// row, two cells and a 2-byte store; CELLS = 1: an 8-byte load per row.
template <int CELLS>
__global__ __launch_bounds__(kThreads) void latent_graded_kernel(const uint8_t* __restrict__ px, uint8_t* __restrict__ lat, int64_t N, int h, int w) {
    const int G = w / CELLS;
    const int64_t W = (int64_t)w * 8;
    const int64_t total = N * h * G;
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * kThreads) {
        const int64_t ny = idx / G;                        // n * h + cell row
        const int cx = (int)(idx - ny * G) * CELLS;
        const uint8_t* p = px + ny * 8 * W + (int64_t)cx * 8;
        uint32_t sum[CELLS];
#pragma unroll
        for (int c = 0; c < CELLS; ++c) sum[c] = 0;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            if constexpr (CELLS == 2) {
                const u32x4 v = *(const u32x4*)(p + r * W);
                sum[0] += byte_sum(v[0]) + byte_sum(v[1]);
                sum[1] += byte_sum(v[2]) + byte_sum(v[3]);
            } else {
                const u32x2 v = *(const u32x2*)(p + r * W);
                sum[0] += byte_sum(v[0]) + byte_sum(v[1]);
            }
        }
        uint8_t* o = lat + ny * w + cx;
        if constexpr (CELLS == 2) {
            *(uint16_t*)o = (uint16_t)(((sum[0] + 32u) >> 6) | (((sum[1] + 32u) >> 6) << 8));
        } else {
            o[0] = (uint8_t)((sum[0] + 32u) >> 6);
        }
    }
}

// ---- out = g == 255 ? r : g == 0 ? o : o + (r - o) * (float(g) / 255.0f) over fp32 [B][3][P] with the strengths uint8 [B][P] broadcast over
// the channels.  V = 4: 16-byte accesses, the four strength bytes as one word; all four 255: `original` is not read, all four 0: `result`
// is not.  out may alias result.
template <int V>
__global__ __launch_bounds__(kThreads) void composite_graded_kernel(const float* result, const float* __restrict__ original,
                                                                    const uint8_t* __restrict__ strength, float* out, int64_t BC, int C, int64_t P) {
    const int64_t PV = P / V;
    const int64_t total = BC * PV;
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * kThreads) {
        const int64_t bc = idx / PV;
        const int64_t p = (idx - bc * PV) * V;
        const int64_t e = bc * P + p;
        const uint8_t* gp = strength + (bc / C) * P + p;
        uint32_t g[V];
        bool all_res = true, all_org = true;
        if constexpr (V == 4) {
            const uint32_t gw = *(const uint32_t*)gp;
#pragma unroll
            for (int j = 0; j < 4; ++j) g[j] = (gw >> (8 * j)) & 255u;
        } else {
            g[0] = gp[0];
        }
#pragma unroll
        for (int j = 0; j < V; ++j) {
            all_res = all_res && g[j] == 255u;
            all_org = all_org && g[j] == 0u;
        }
        float rv[V], ov[V];
#pragma unroll
        for (int j = 0; j < V; ++j) rv[j] = ov[j] = 0.0f;
        if (!all_org) {
            if constexpr (V == 4) {
                const f32x4 q = *(const f32x4*)(result + e);
                rv[0] = q[0], rv[1] = q[1], rv[2] = q[2], rv[3] = q[3];
            } else {
                rv[0] = result[e];
            }
        }
        if (!all_res) {
            if constexpr (V == 4) {
                const f32x4 q = *(const f32x4*)(original + e);
                ov[0] = q[0], ov[1] = q[1], ov[2] = q[2], ov[3] = q[3];
            } else {
                ov[0] = original[e];
            }
        }
        float yv[V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float a = (float)g[j] / 255.0f;          // four roundings, as numpy's float32: IEEE divide, no fma (-ffp-contract=off)
            const float d = rv[j] - ov[j];
            const float t = d * a;
            const float u = ov[j] + t;
            yv[j] = g[j] == 255u ? rv[j] : (g[j] == 0u ? ov[j] : u);
        }
        if constexpr (V == 4) {
            *(f32x4*)(out + e) = f32x4{yv[0], yv[1], yv[2], yv[3]};
        } else {
            out[e] = yv[0];
        }
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------
// launchers (arguments validated by the entry points in core.cpp)
// ------------------------------------------------------------------------------------------
int cc_mask_feather(const uint8_t* src, uint16_t* tmp16, uint8_t* dst, int64_t N, int32_t H, int32_t W, int32_t R, hipStream_t s) {
    if (W % 8 == 0 && aligned(tmp16, 16) && aligned(dst, 8)) {          // every row of tmp16 is 16-byte, every row of dst 8-byte aligned
        const unsigned grid = grid_for(N * H * (W / 8));
        hipLaunchKernelGGL(feather_rows_kernel<8>, dim3(grid), dim3(kThreads), 0, s, src, tmp16, N, H, W, R);
        hipLaunchKernelGGL(feather_cols_kernel<8>, dim3(grid), dim3(kThreads), 0, s, tmp16, dst, N, H, W, R);
    } else {                                                             // (core.cpp: W % 4 == 0, every buffer 4-byte aligned)
        const unsigned grid = grid_for(N * H * (W / 4));
        hipLaunchKernelGGL(feather_rows_kernel<4>, dim3(grid), dim3(kThreads), 0, s, src, tmp16, N, H, W, R);
        hipLaunchKernelGGL(feather_cols_kernel<4>, dim3(grid), dim3(kThreads), 0, s, tmp16, dst, N, H, W, R);
    }
    return cc_launch_status("mask_feather");
}

int cc_mask_latent_graded(const uint8_t* mask_px, uint8_t* strength_lat, int64_t N, int32_t H, int32_t W, hipStream_t s) {
    const int h = H / 8, w = W / 8;
    if (w % 2 == 0 && aligned(mask_px, 16) && aligned(strength_lat, 2))      // W % 16 == 0: every row of a cell pair is 16-byte aligned
        hipLaunchKernelGGL(latent_graded_kernel<2>, dim3(grid_for(N * h * (w / 2))), dim3(kThreads), 0, s, mask_px, strength_lat, N, h, w);
    else                                                                     // (core.cpp: the map is 8-byte aligned, W % 8 == 0)
        hipLaunchKernelGGL(latent_graded_kernel<1>, dim3(grid_for(N * h * w)), dim3(kThreads), 0, s, mask_px, strength_lat, N, h, w);
    return cc_launch_status("mask_latent_graded");
}

int cc_mask_composite_graded(const float* result, const float* original, const uint8_t* strength_px, float* out, int32_t B, int64_t P,
                             hipStream_t st) {
    if (P % 4 == 0 && aligned(result, 16) && aligned(original, 16) && aligned(out, 16) && aligned(strength_px, 4))
        hipLaunchKernelGGL(composite_graded_kernel<4>, dim3(grid_for((int64_t)B * 3 * (P / 4))), dim3(kThreads), 0, st, result, original, strength_px,
                           out, (int64_t)B * 3, 3, P);
    else
        hipLaunchKernelGGL(composite_graded_kernel<1>, dim3(grid_for((int64_t)B * 3 * P)), dim3(kThreads), 0, st, result, original, strength_px, out,
                           (int64_t)B * 3, 3, P);
    return cc_launch_status("mask_composite_graded");
}
