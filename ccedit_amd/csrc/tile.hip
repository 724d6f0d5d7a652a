// Large frames (include/ccedit_hip.h, "Tiles"): a frame of h x w latent pixels is evaluated as overlapping tiles of th x tw, and the
// tiles' denoised latents are cross-faded back into one latent at every network evaluation (ccedit_amd/tiles.py).  x is fp32
// [planes][h][w], planes = B C N; tile t starts at (sy_t, sx_t) = starts[t][0], starts[t][1].
//   tile_gather   xt[t][p][i][j] = x[p][sy_t + i][sx_t + j]: all tiles in one launch, a bit copy
//   tile_fuse     out[p][y][x] = sum over the tiles covering (y, x), ascending t, of coef[t][y - sy_t][x - sx_t] * y_t[p][y - sy_t][x - sx_t];
//                 y_t through a device table of tile pointers, every output element written exactly once, no atomics
// Both move bytes: grid-stride loops over at most kMaxBlocks workgroups, 64-bit element indices, one thread per 4 consecutive
// elements of a row where the row length is a multiple of 4 (one element otherwise).  Whether those 4 move as ONE 16-byte access
// is decided per row in the kernel, from the addresses themselves: a tile that starts at a column that is no multiple of 4, or a tile
// tensor that is not 16-byte aligned, is read element by element.  The file is compiled with -ffp-contract=off: the first term of a
// sum is the product alone, every further term one multiply and then one add — the same roundings as the loop in numpy float32, and
// an element that one tile covers (coefficient exactly 1.0f) is a bit copy.  `starts` and `coef` are device tables the host cannot
// read back before the launch, so the kernels hold every index inside its tensor whatever the tables say: a start is clamped to
// 0 ... h - th / 0 ... w - tw, an element no tile covers is 0.
// The argument checks live with the exported entry points in core.cpp; the launchers below trust their arguments.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 256 * 8;          // 256 CUs x 8 workgroups of 4 waves

inline unsigned grid_for(int64_t items) {
    const int64_t g = (items + kThreads - 1) / kThreads;
    return (unsigned)(g < 1 ? 1 : (g > kMaxBlocks ? kMaxBlocks : g));
}

__device__ inline int clamp_start(int s, int n, int t) { return s < 0 ? 0 : (s > n - t ? n - t : s); }
__device__ inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ---- gather: one thread per V consecutive elements of a tile row (V == 4 needs tw % 4 == 0, so the 4 never leave the row).
template <int V>
__global__ __launch_bounds__(kThreads) void tile_gather_kernel(const float* __restrict__ x, float* __restrict__ xt,
                                                               const int32_t* __restrict__ starts, int T, int64_t planes, int h, int w, int th, int tw) {
    const int64_t rowv = tw / V;                                   // items of one tile row
    const int64_t total = (int64_t)T * planes * th * rowv;
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * kThreads) {
        const int64_t row = idx / rowv;                            // (t * planes + p) * th + i
        const int j = (int)(idx - row * rowv) * V;
        const int64_t tp = row / th;                               // t * planes + p
        const int i = (int)(row - tp * th);
        const int t = (int)(tp / planes);
        const int64_t p = tp - (int64_t)t * planes;
        const int sy = clamp_start(starts[2 * t], h, th);
        const int sx = clamp_start(starts[2 * t + 1], w, tw);
        const float* src = x + (p * h + sy + i) * (int64_t)w + sx + j;
        float* dst = xt + row * tw + j;
        if constexpr (V == 4) {
            if (aligned16(src) && aligned16(dst)) {
                *(f32x4*)dst = *(const f32x4*)src;
            } else {
                dst[0] = src[0], dst[1] = src[1], dst[2] = src[2], dst[3] = src[3];
            }
        } else {
            dst[0] = src[0];
        }
    }
}

// ---- fuse: one thread per V consecutive output elements of a frame row (V == 4 needs w % 4 == 0).  The tiles are walked in
// ascending t, the order of the definition.  A tile whose start column is no multiple of 4 may cover only some of the 4 elements: each
// element keeps its own `first`.  The 4 of a tile move as one 16-byte load when all 4 are inside the tile and the address allows it.
template <int V>
__global__ __launch_bounds__(kThreads) void tile_fuse_kernel(const float* const* __restrict__ yt, float* __restrict__ out,
                                                             const int32_t* __restrict__ starts, const float* __restrict__ coef, int T,
                                                             int64_t planes, int h, int w, int th, int tw) {
    const int64_t rowv = w / V;
    const int64_t total = planes * h * rowv;
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * kThreads) {
        const int64_t row = idx / rowv;                            // p * h + y
        const int x0 = (int)(idx - row * rowv) * V;
        const int64_t p = row / h;
        const int y = (int)(row - p * h);
        float acc[V];
        bool first[V];
#pragma unroll
        for (int v = 0; v < V; ++v) acc[v] = 0.0f, first[v] = true;
        for (int t = 0; t < T; ++t) {
            const int i = y - clamp_start(starts[2 * t], h, th);
            if (i < 0 || i >= th) continue;
            const int j0 = x0 - clamp_start(starts[2 * t + 1], w, tw);
            if (j0 + V <= 0 || j0 >= tw) continue;
            const int64_t crow = ((int64_t)t * th + i) * tw;       // this tile row in coef
            const int64_t yrow = (p * th + i) * (int64_t)tw;       // ... and in y_t
            const float* ybase = yt[t];
            float yv[V], cv[V];
            bool in[V];
            if constexpr (V == 4) {
                if (j0 >= 0 && j0 + 4 <= tw && aligned16(ybase + yrow + j0) && aligned16(coef + crow + j0)) {
                    const f32x4 q = *(const f32x4*)(ybase + yrow + j0);
                    const f32x4 c = *(const f32x4*)(coef + crow + j0);
#pragma unroll
                    for (int v = 0; v < 4; ++v) yv[v] = q[v], cv[v] = c[v], in[v] = true;
                } else {
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        const int j = j0 + v;
                        in[v] = j >= 0 && j < tw;
                        yv[v] = in[v] ? ybase[yrow + j] : 0.0f;
                        cv[v] = in[v] ? coef[crow + j] : 0.0f;
                    }
                }
            } else {
                in[0] = true;                                      // 0 <= j0 < tw was checked above
                yv[0] = ybase[yrow + j0];
                cv[0] = coef[crow + j0];
            }
#pragma unroll
            for (int v = 0; v < V; ++v) {
                if (!in[v]) continue;
                const float term = cv[v] * yv[v];                  // one multiply, then one add: no fma (-ffp-contract=off)
                acc[v] = first[v] ? term : acc[v] + term;
                first[v] = false;
            }
        }
        float* dst = out + row * w + x0;
        if constexpr (V == 4) {
            if (aligned16(dst)) {
                *(f32x4*)dst = f32x4{acc[0], acc[1], acc[2], acc[3]};
            } else {
                dst[0] = acc[0], dst[1] = acc[1], dst[2] = acc[2], dst[3] = acc[3];
            }
        } else {
            dst[0] = acc[0];
        }
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------
// launchers (arguments validated by the entry points in core.cpp)
// ------------------------------------------------------------------------------------------
int cc_tile_gather(const float* x, float* xt, const int32_t* starts, int32_t T, int64_t planes, int32_t h, int32_t w, int32_t th, int32_t tw,
                   hipStream_t s) {
    if (tw % 4 == 0)
        hipLaunchKernelGGL(tile_gather_kernel<4>, dim3(grid_for((int64_t)T * planes * th * (tw / 4))), dim3(kThreads), 0, s, x, xt, starts, T, planes,
                           h, w, th, tw);
    else
        hipLaunchKernelGGL(tile_gather_kernel<1>, dim3(grid_for((int64_t)T * planes * th * tw)), dim3(kThreads), 0, s, x, xt, starts, T, planes, h, w,
                           th, tw);
    return cc_launch_status("tile_gather");
}

int cc_tile_fuse(const float* const* yt, float* out, const int32_t* starts, const float* coef, int32_t T, int64_t planes, int32_t h, int32_t w,
                 int32_t th, int32_t tw, hipStream_t s) {
    if (w % 4 == 0)
        hipLaunchKernelGGL(tile_fuse_kernel<4>, dim3(grid_for(planes * h * (w / 4))), dim3(kThreads), 0, s, yt, out, starts, coef, T, planes, h, w, th,
                           tw);
    else
        hipLaunchKernelGGL(tile_fuse_kernel<1>, dim3(grid_for(planes * h * w)), dim3(kThreads), 0, s, yt, out, starts, coef, T, planes, h, w, th, tw);
    return cc_launch_status("tile_fuse");
}
