// Long clips (include/ccedit_hip.h, "Windows"): a clip of N > T keyframes is evaluated as W overlapping windows of T frames, and
// the windows' denoised latents are cross-faded back into one latent of N frames at every network evaluation (ccedit_amd/windows.py).
//   window_gather   xw[w][bc][j][p] = x[bc][starts[w] + j][p]: all W windows in one launch, a bit copy
//   window_fuse     out[bc][f][p] = sum over the windows covering f, ascending w, of coef[w][f - starts[w]] * y_w[bc][f - starts[w]][p];
//                   y_w through a device table of W pointers, every output element written exactly once, no atomics
// Both move bytes: grid-stride loops over at most kMaxBlocks workgroups, 16-byte accesses where P % 4 == 0 and the pointers allow, a
// one-element variant otherwise.  The file is compiled with -ffp-contract=off: the first term of a sum is the product alone, every
// further term one multiply and then one add — the same roundings as the loop in numpy float32, and a frame that one window covers
// (coefficient exactly 1.0f) is a bit copy.  `starts` and `coef` are device tables the host cannot read back before the launch, so the
// kernels hold every index inside its tensor whatever the tables say: a start is clamped to 0 ... N - T, a frame no window covers is 0.
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

__device__ inline int clamp_start(int s, int N, int T) { return s < 0 ? 0 : (s > N - T ? N - T : s); }

// ---- gather: for one (w, bc) the T frames of a window are ONE contiguous run of T * P floats in x and in xw: W * BC straight copies.
template <int V>
__global__ __launch_bounds__(kThreads) void window_gather_kernel(const float* __restrict__ x, float* __restrict__ xw,
                                                                 const int32_t* __restrict__ starts, int W, int BC, int N, int T, int64_t P) {
    const int64_t run = (int64_t)T * P / V;                        // items of one (w, bc) run
    const int64_t total = (int64_t)W * BC * run;
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * kThreads) {
        const int64_t row = idx / run;                             // w * BC + bc
        const int64_t e = (idx - row * run) * V;
        const int w = (int)(row / BC);
        const int64_t bc = row - (int64_t)w * BC;
        const int s = clamp_start(starts[w], N, T);
        const float* src = x + (bc * N + s) * P + e;
        float* dst = xw + row * T * P + e;
        if constexpr (V == 4)
            *(f32x4*)dst = *(const f32x4*)src;
        else
            dst[0] = src[0];
    }
}

// ---- fuse: one thread per V consecutive output elements of a frame; the windows are walked in ascending w (their starts ascend, so
// are the terms of a frame in the order of the definition).  A window's tensor that is not 16-byte aligned is read element by element.
template <int V>
__global__ __launch_bounds__(kThreads) void window_fuse_kernel(const float* const* __restrict__ yw, float* __restrict__ out,
                                                               const int32_t* __restrict__ starts, const float* __restrict__ coef, int W, int BC,
                                                               int N, int T, int64_t P) {
    const int64_t PV = P / V;
    const int64_t total = (int64_t)BC * N * PV;
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * kThreads) {
        const int64_t bf = idx / PV;                               // bc * N + f
        const int64_t p = (idx - bf * PV) * V;
        const int64_t bc = bf / N;
        const int f = (int)(bf - bc * N);
        float acc[V];
#pragma unroll
        for (int v = 0; v < V; ++v) acc[v] = 0.0f;
        bool first = true;
        for (int w = 0; w < W; ++w) {
            const int j = f - clamp_start(starts[w], N, T);
            if (j < 0 || j >= T) continue;
            const float cf = coef[(int64_t)w * T + j];
            const float* src = yw[w] + (bc * T + j) * P + p;
            float yv[V];
            if constexpr (V == 4) {
                if (((uintptr_t)src & 15) == 0) {
                    const f32x4 q = *(const f32x4*)src;
                    yv[0] = q[0], yv[1] = q[1], yv[2] = q[2], yv[3] = q[3];
                } else {
                    yv[0] = src[0], yv[1] = src[1], yv[2] = src[2], yv[3] = src[3];
                }
            } else {
                yv[0] = src[0];
            }
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const float t = cf * yv[v];                        // one multiply, then one add: no fma (-ffp-contract=off)
                acc[v] = first ? t : acc[v] + t;
            }
            first = false;
        }
        float* dst = out + bf * P + p;
        if constexpr (V == 4)
            *(f32x4*)dst = f32x4{acc[0], acc[1], acc[2], acc[3]};
        else
            dst[0] = acc[0];
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------
// launchers (arguments validated by the entry points in core.cpp)
// ------------------------------------------------------------------------------------------
int cc_window_gather(const float* x, float* xw, const int32_t* starts, int32_t W, int32_t BC, int32_t N, int32_t T, int64_t P, hipStream_t s) {
    if (P % 4 == 0 && aligned(x, 16) && aligned(xw, 16))
        hipLaunchKernelGGL(window_gather_kernel<4>, dim3(grid_for((int64_t)W * BC * T * (P / 4))), dim3(kThreads), 0, s, x, xw, starts, W, BC, N, T, P);
    else
        hipLaunchKernelGGL(window_gather_kernel<1>, dim3(grid_for((int64_t)W * BC * T * P)), dim3(kThreads), 0, s, x, xw, starts, W, BC, N, T, P);
    return cc_launch_status("window_gather");
}

int cc_window_fuse(const float* const* yw, float* out, const int32_t* starts, const float* coef, int32_t W, int32_t BC, int32_t N, int32_t T,
                   int64_t P, hipStream_t s) {
    if (P % 4 == 0 && aligned(out, 16))
        hipLaunchKernelGGL(window_fuse_kernel<4>, dim3(grid_for((int64_t)BC * N * (P / 4))), dim3(kThreads), 0, s, yw, out, starts, coef, W, BC, N, T, P);
    else
        hipLaunchKernelGGL(window_fuse_kernel<1>, dim3(grid_for((int64_t)BC * N * P)), dim3(kThreads), 0, s, yw, out, starts, coef, W, BC, N, T, P);
    return cc_launch_status("window_fuse");
}
