// Region-restricted editing (include/ccedit_hip.h, "Edit masks"): what lies between a user's pixel mask and the samplers' inpainting loops.
//   mask_resize_nearest   uint8 mask -> the clip's size by two index tables (Pillow's NEAREST), a gather
//   mask_latent           pixel mask -> latent mask: an 8 x 8 cell is 1 when MORE than 32 of its pixels are set
//   inpaint_blend         the per-step re-injection y = m ? x : (x0 + noise * sigma) / s, mask broadcast over the channels
//   inpaint_blend_level   the same kernel with the caller's threshold on the byte: the re-injection of a graded run (softmask.hip)
//   mask_composite        out = m ? result : original on the decoded frames
//   mask_dilate           pixel mask -> its (2R + 1)^2 square maximum in two separable passes, optionally inverted (255 - m) on the way out
// Convention everywhere: set (pixel masks: byte >= 128, latent masks: byte != 0) = edit, clear = keep the original.
// All of them move bytes: grid-stride loops over a grid of at most kMaxBlocks workgroups, 16-byte accesses where sizes and alignment
// allow and a one-element variant otherwise; the mask is never expanded to the tensors' shape.  The file is compiled with
// -ffp-contract=off: inpaint_blend is one fp32 multiply, one add and one correctly rounded divide, in the reference's order.
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

// ---- nearest resize: dst[n][y][x] = src[n][ytab[y]][xtab[x]]; PX output bytes per thread (4: one 4-byte store).  Indices are held
// inside the source whatever the tables say.
template <int PX>
__global__ __launch_bounds__(kThreads) void mask_resize_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                               const int32_t* __restrict__ ytab, const int32_t* __restrict__ xtab, int N, int Hs,
                                                               int Ws, int H, int W) {
    const int G = W / PX;
    const int64_t total = (int64_t)N * H * G;
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * kThreads) {
        const int64_t ny = idx / G;
        const int x0 = (int)(idx - ny * G) * PX;
        const int n = (int)(ny / H), y = (int)(ny - (int64_t)n * H);
        int ys = ytab[y];
        ys = ys < 0 ? 0 : (ys > Hs - 1 ? Hs - 1 : ys);
        const uint8_t* srow = src + ((int64_t)n * Hs + ys) * Ws;
        uint32_t b[PX];
#pragma unroll
        for (int p = 0; p < PX; ++p) {
            int xs = xtab[x0 + p];
            xs = xs < 0 ? 0 : (xs > Ws - 1 ? Ws - 1 : xs);
            b[p] = srow[xs];
        }
        uint8_t* d = dst + ny * W + x0;
        if constexpr (PX == 4) {
            *(uint32_t*)d = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
        } else {
            d[0] = (uint8_t)b[0];
        }
    }
}

// ---- pixel mask [N][H][W] -> latent mask [N][H/8][W/8].  A byte is set when its top bit is (>= 128): the set pixels of eight bytes
// are the population count of (word & 0x80808080) twice; a cell is eight such rows.  CELLS = 2: a 16-byte load per row, two cells.
template <int CELLS>
__global__ __launch_bounds__(kThreads) void mask_latent_kernel(const uint8_t* __restrict__ px, uint8_t* __restrict__ lat, int64_t N, int h, int w) {
    const int G = w / CELLS;
    const int64_t W = (int64_t)w * 8;
    const int64_t total = N * h * G;
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * kThreads) {
        const int64_t ny = idx / G;                        // n * h + cell row
        const int cx = (int)(idx - ny * G) * CELLS;
        const uint8_t* p = px + ny * 8 * W + (int64_t)cx * 8;
        int cnt[CELLS];
#pragma unroll
        for (int c = 0; c < CELLS; ++c) cnt[c] = 0;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            if constexpr (CELLS == 2) {
                const u32x4 v = *(const u32x4*)(p + r * W);
                cnt[0] += __popc(v[0] & 0x80808080u) + __popc(v[1] & 0x80808080u);
                cnt[1] += __popc(v[2] & 0x80808080u) + __popc(v[3] & 0x80808080u);
            } else {
                const u32x2 v = *(const u32x2*)(p + r * W);
                cnt[0] += __popc(v[0] & 0x80808080u) + __popc(v[1] & 0x80808080u);
            }
        }
        uint8_t* o = lat + ny * w + cx;
        if constexpr (CELLS == 2) {
            *(uint16_t*)o = (uint16_t)((cnt[0] > 32 ? 1u : 0u) | (cnt[1] > 32 ? 0x100u : 0u));
        } else {
            o[0] = cnt[0] > 32 ? 1 : 0;
        }
    }
}

// ---- y = m ? x : other over fp32 [B][C][P] with the uint8 mask [B][P] broadcast over C; m = (byte >= thr).
//   BLEND: other = (a + noise * sigma) / s   (the known content at the current noise level: sampling.py:150-153, 213-216)
//   else:  other = a                         (the original frames)
// V = 4: 16-byte accesses, the four mask bytes as one word; where all four are set nothing but x is read.  y may alias x.
template <int V, bool BLEND>
__global__ __launch_bounds__(kThreads) void mask_select_kernel(const float* x, const float* __restrict__ a, const float* __restrict__ noise,
                                                               const uint8_t* __restrict__ mask, float* y, int64_t BC, int C, int64_t P,
                                                               uint32_t thr, float sigma, float s) {
    const int64_t PV = P / V;
    const int64_t total = BC * PV;
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * kThreads) {
        const int64_t bc = idx / PV;
        const int64_t p = (idx - bc * PV) * V;
        const int64_t e = bc * P + p;
        const uint8_t* mp = mask + (bc / C) * P + p;
        bool m[V];
        bool all = true;
        if constexpr (V == 4) {
            const uint32_t mw = *(const uint32_t*)mp;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                m[j] = ((mw >> (8 * j)) & 255u) >= thr;
                all = all && m[j];
            }
        } else {
            m[0] = mp[0] >= thr;
            all = m[0];
        }
        float xv[V], ov[V];
        if constexpr (V == 4) {
            const f32x4 q = *(const f32x4*)(x + e);
            xv[0] = q[0], xv[1] = q[1], xv[2] = q[2], xv[3] = q[3];
        } else {
            xv[0] = x[e];
        }
        if (!all) {
            if constexpr (V == 4) {
                const f32x4 q = *(const f32x4*)(a + e);
                ov[0] = q[0], ov[1] = q[1], ov[2] = q[2], ov[3] = q[3];
            } else {
                ov[0] = a[e];
            }
            if constexpr (BLEND) {
                float nv[V];
                if constexpr (V == 4) {
                    const f32x4 q = *(const f32x4*)(noise + e);
                    nv[0] = q[0], nv[1] = q[1], nv[2] = q[2], nv[3] = q[3];
                } else {
                    nv[0] = noise[e];
                }
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const float t = nv[j] * sigma;          // three roundings, as the reference: no fma (-ffp-contract=off), IEEE divide
                    const float u = ov[j] + t;
                    ov[j] = u / s;
                }
            }
#pragma unroll
            for (int j = 0; j < V; ++j) xv[j] = m[j] ? xv[j] : ov[j];
        }
        if constexpr (V == 4) {
            *(f32x4*)(y + e) = f32x4{xv[0], xv[1], xv[2], xv[3]};
        } else {
            y[e] = xv[0];
        }
    }
}

template <bool BLEND>
void launch_select(const float* x, const float* a, const float* noise, const uint8_t* mask, float* y, int64_t B, int C, int64_t P,
                   uint32_t thr, float sigma, float s, hipStream_t st) {
    const bool vec = P % 4 == 0 && aligned(x, 16) && aligned(a, 16) && aligned(y, 16) && aligned(mask, 4) && (!BLEND || aligned(noise, 16));
    if (vec)
        hipLaunchKernelGGL((mask_select_kernel<4, BLEND>), dim3(grid_for(B * C * (P / 4))), dim3(kThreads), 0, st, x, a, noise, mask, y, B * C, C, P,
                           thr, sigma, s);
    else
        hipLaunchKernelGGL((mask_select_kernel<1, BLEND>), dim3(grid_for(B * C * P)), dim3(kThreads), 0, st, x, a, noise, mask, y, B * C, C, P, thr,
                           sigma, s);
}

// ---- dilation: one pass of the separable (2R + 1)^2 square maximum over uint8 masks [N][H][W], the window clipped at the border;
// one thread per four consecutive pixels of a row (W % 4 == 0).  VERT = false: along x, true: along y; `inv`: 255 - m on the way out.
template <bool VERT>
__global__ __launch_bounds__(kThreads) void mask_dilate_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int64_t N, int H, int W,
                                                               int R, uint32_t inv) {
    const int G = W / 4;
    const int64_t total = N * H * G;
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * kThreads) {
        const int64_t ny = idx / G;
        const int x0 = (int)(idx - ny * G) * 4;
        const int64_t n = ny / H;
        const int y = (int)(ny - n * H);
        const uint8_t* img = src + n * H * W;
        uint32_t m[4] = {0, 0, 0, 0};
        if constexpr (VERT) {
            const int lo = y - R < 0 ? 0 : y - R, hi = y + R > H - 1 ? H - 1 : y + R;
            for (int yy = lo; yy <= hi; ++yy) {
                const uint32_t d = *(const uint32_t*)(img + (int64_t)yy * W + x0);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t b = (d >> (8 * j)) & 255u;
                    m[j] = b > m[j] ? b : m[j];
                }
            }
        } else {
            const uint8_t* row = img + (int64_t)y * W;
            const int lo = x0 - R < 0 ? 0 : x0 - R, hi = x0 + 3 + R > W - 1 ? W - 1 : x0 + 3 + R;
            for (int xx = lo; xx <= hi; ++xx) {
                const uint32_t b = row[xx];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int dx = xx - (x0 + j);
                    if (dx >= -R && dx <= R) m[j] = b > m[j] ? b : m[j];
                }
            }
        }
        *(uint32_t*)(dst + ny * W + x0) = (m[0] | (m[1] << 8) | (m[2] << 16) | (m[3] << 24)) ^ inv;
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------
// launchers (arguments validated by the entry points in core.cpp)
// ------------------------------------------------------------------------------------------
int cc_mask_dilate(const uint8_t* src, uint8_t* tmp, uint8_t* dst, int64_t N, int32_t H, int32_t W, int32_t R, int32_t invert, hipStream_t s) {
    const unsigned grid = grid_for(N * H * (W / 4));
    const uint32_t inv = invert ? 0xffffffffu : 0u;                        // 255 - m of every byte
    if (R > 0)
        hipLaunchKernelGGL(mask_dilate_kernel<false>, dim3(grid), dim3(kThreads), 0, s, src, tmp, N, H, W, R, 0u);
    hipLaunchKernelGGL(mask_dilate_kernel<true>, dim3(grid), dim3(kThreads), 0, s, R > 0 ? tmp : src, dst, N, H, W, R, inv);
    return cc_launch_status("mask_dilate");
}

int cc_mask_resize_nearest(const uint8_t* src, uint8_t* dst, const int32_t* ytab, const int32_t* xtab, int32_t N, int32_t Hs, int32_t Ws,
                           int32_t H, int32_t W, hipStream_t s) {
    if (W % 4 == 0 && aligned(dst, 4))
        hipLaunchKernelGGL(mask_resize_kernel<4>, dim3(grid_for((int64_t)N * H * (W / 4))), dim3(kThreads), 0, s, src, dst, ytab, xtab, N, Hs, Ws, H, W);
    else
        hipLaunchKernelGGL(mask_resize_kernel<1>, dim3(grid_for((int64_t)N * H * W)), dim3(kThreads), 0, s, src, dst, ytab, xtab, N, Hs, Ws, H, W);
    return cc_launch_status("mask_resize_nearest");
}

int cc_mask_latent(const uint8_t* mask_px, uint8_t* mask_lat, int64_t N, int32_t H, int32_t W, hipStream_t s) {
    const int h = H / 8, w = W / 8;
    if (w % 2 == 0 && aligned(mask_px, 16) && aligned(mask_lat, 2))          // W % 16 == 0: every row of a cell pair is 16-byte aligned
        hipLaunchKernelGGL(mask_latent_kernel<2>, dim3(grid_for(N * h * (w / 2))), dim3(kThreads), 0, s, mask_px, mask_lat, N, h, w);
    else                                                                     // (core.cpp: the mask is 8-byte aligned, W % 8 == 0)
        hipLaunchKernelGGL(mask_latent_kernel<1>, dim3(grid_for(N * h * w)), dim3(kThreads), 0, s, mask_px, mask_lat, N, h, w);
    return cc_launch_status("mask_latent");
}

int cc_mask_inpaint_blend(const float* x, const float* x0, const float* noise, const uint8_t* mask, float* y, int32_t B, int32_t C, int64_t P,
                          float sigma, float s, hipStream_t st) {
    launch_select<true>(x, x0, noise, mask, y, B, C, P, 1u, sigma, s, st);
    return cc_launch_status("inpaint_blend");
}

// the re-injection of a graded run (softmask.hip): the same kernel, a cell is free where its strength byte is >= the step's threshold
int cc_mask_inpaint_blend_level(const float* x, const float* x0, const float* noise, const uint8_t* strength, float* y, int32_t B, int32_t C,
                                int64_t P, int32_t thr, float sigma, float s, hipStream_t st) {
    launch_select<true>(x, x0, noise, strength, y, B, C, P, (uint32_t)thr, sigma, s, st);
    return cc_launch_status("inpaint_blend_level");
}

int cc_mask_composite(const float* result, const float* original, const uint8_t* mask_px, float* out, int32_t B, int64_t P, hipStream_t st) {
    launch_select<false>(result, original, nullptr, mask_px, out, B, 3, P, 128u, 0.0f, 1.0f, st);
    return cc_launch_status("mask_composite");
}
