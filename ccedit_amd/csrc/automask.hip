// Automatic edit masks (include/ccedit_hip.h, "Automatic masks"): from the two halves of a denoiser output — the source prompt's and the
// target prompt's prediction for the same noised latent — to a clean uint8 pixel mask (ccedit_amd/automask.py; DiffEdit's mask step,
// plus a vote over time).  tests/_automask_numpy.py is the definition; every kernel reproduces it bit for bit.
//   automask_accumulate   y fp32 [2B][C][P] -> acc fp32 [B][P]: s = ((|y[B+b][0] - y[b][0]| + |...[1]|) + |...[2]|) + ..., channels
//                         ascending, one rounding per subtract and per add; acc = s (first) or acc + s
//   automask_binarize     bin[b][p] = acc[b][p] > theta * scale[b] (strictly; one fp32 multiply; scale read from DEVICE memory), 0 / 1
//   automask_vote         out[b][t][y][x] = (sum of bin over dt, dy, dx in {-1, 0, 1}, coordinates clamped into the volume) >= votes
//   automask_expand       latent mask [N][h][w] (!= 0 is set) -> pixel mask [N][8h][8w] in {0, 255}
// All four move bytes: grid-stride loops of 256-thread workgroups, at most 2048 of them.  accumulate reads 16 bytes per lane and
// channel where P % 4 == 0 and y and acc are 16-byte aligned (every channel row then is), one element otherwise; binarize reads 16
// bytes and writes its four mask bytes as one word under the same condition; expand writes the 8 bytes of a cell's pixel row as one
// store, consecutive lanes consecutive cells of a row; vote is one lane per cell with 27 byte loads that stay in cache (a clip's
// latent mask is ~100 KB).  The file is compiled with -ffp-contract=off and without any fast-math flag.  Nothing here is atomic and
// every output element is written exactly once.  The argument checks live with the exported entry points in core.cpp.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 256 * 8;          // 256 CUs x 8 workgroups of 4 waves
constexpr int kMaxChannels = 16;

inline unsigned grid_for(int64_t items) {
    const int64_t g = (items + kThreads - 1) / kThreads;
    return (unsigned)(g < 1 ? 1 : (g > kMaxBlocks ? kMaxBlocks : g));
}
inline bool aligned(const void* p, unsigned a) { return ((uintptr_t)p & (a - 1)) == 0; }

// ---- accumulate: one thread per V consecutive cells of a clip; the channels are walked in ascending order.
template <int V>
__global__ __launch_bounds__(kThreads) void automask_accumulate_kernel(const float* __restrict__ y, float* __restrict__ acc, int B, int C,
                                                                       int64_t P, int first) {
    const int64_t PV = P / V;
    const int64_t total = (int64_t)B * PV;
    const int64_t half = (int64_t)B * C * P;                       // from the source-prompt half to the target-prompt half
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * kThreads) {
        const int64_t b = idx / PV;
        const int64_t p = (idx - b * PV) * V;
        const float* src = y + b * C * P + p;
        float s[V] = {};
        for (int c = 0; c < C; ++c) {
            float u[V], t[V];
            if constexpr (V == 4) {
                const f32x4 qu = *(const f32x4*)(src + (int64_t)c * P);
                const f32x4 qt = *(const f32x4*)(src + half + (int64_t)c * P);
                u[0] = qu[0], u[1] = qu[1], u[2] = qu[2], u[3] = qu[3];
                t[0] = qt[0], t[1] = qt[1], t[2] = qt[2], t[3] = qt[3];
            } else {
                u[0] = src[(int64_t)c * P];
                t[0] = src[half + (int64_t)c * P];
            }
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const float d = fabsf(t[v] - u[v]);
                s[v] = c == 0 ? d : s[v] + d;
            }
        }
        float* dst = acc + b * P + p;
        if constexpr (V == 4) {
            if (first) {
                *(f32x4*)dst = f32x4{s[0], s[1], s[2], s[3]};
            } else {
                const f32x4 a = *(const f32x4*)dst;
                *(f32x4*)dst = f32x4{a[0] + s[0], a[1] + s[1], a[2] + s[2], a[3] + s[3]};
            }
        } else {
            dst[0] = first ? s[0] : dst[0] + s[0];
        }
    }
}

// ---- binarize: strictly greater than theta * scale[b]; a NaN compares false and stays clear.
template <int V>
__global__ __launch_bounds__(kThreads) void automask_binarize_kernel(const float* __restrict__ acc, const float* __restrict__ scale, float theta,
                                                                     uint8_t* __restrict__ bin, int B, int64_t P) {
    const int64_t PV = P / V;
    const int64_t total = (int64_t)B * PV;
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * kThreads) {
        const int64_t b = idx / PV;
        const int64_t p = (idx - b * PV) * V;
        const float thr = theta * scale[b];
        if constexpr (V == 4) {
            const f32x4 a = *(const f32x4*)(acc + b * P + p);
            const uint32_t word = (a[0] > thr ? 1u : 0u) | (a[1] > thr ? 1u << 8 : 0u) | (a[2] > thr ? 1u << 16 : 0u) | (a[3] > thr ? 1u << 24 : 0u);
            *(uint32_t*)(bin + b * P + p) = word;
        } else {
            bin[b * P + p] = acc[b * P + p] > thr ? 1 : 0;
        }
    }
}

// ---- vote: one thread per cell; the 27 neighbours with every coordinate clamped into the volume (a border cell counts itself again).
__global__ __launch_bounds__(kThreads) void automask_vote_kernel(const uint8_t* __restrict__ bin, uint8_t* __restrict__ out, int64_t total, int T,
                                                                 int h, int w, int votes) {
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * kThreads) {
        const int x = (int)(idx % w);
        int64_t r = idx / w;
        const int yy = (int)(r % h);
        r /= h;
        const int t = (int)(r % T);
        const int64_t b = r / T;
        const uint8_t* clip = bin + b * T * h * w;
        int count = 0;
#pragma unroll
        for (int dt = -1; dt <= 1; ++dt) {
            const int tt = min(max(t + dt, 0), T - 1);
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy) {
                const int ny = min(max(yy + dy, 0), h - 1);
                const uint8_t* row = clip + ((int64_t)tt * h + ny) * w;
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) count += row[min(max(x + dx, 0), w - 1)] != 0 ? 1 : 0;
            }
        }
        out[idx] = count >= votes ? 1 : 0;
    }
}

// ---- expand: one thread per (pixel row, latent cell): the 8 bytes of the cell in that row, one store.
__global__ __launch_bounds__(kThreads) void automask_expand_kernel(const uint8_t* __restrict__ lat, uint8_t* __restrict__ px, int64_t total, int h,
                                                                   int w) {
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * kThreads) {
        const int x = (int)(idx % w);
        const int64_t row = idx / w;                               // n * 8h + Y
        const int64_t n = row / (8 * (int64_t)h);
        const int cy = (int)((row - n * 8 * h) >> 3);
        const uint32_t v = lat[(n * h + cy) * w + x] != 0 ? 0xFFFFFFFFu : 0u;
        *(u32x2*)(px + idx * 8) = u32x2{v, v};                     // (row * 8w + 8x) = 8 idx
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------
// launchers (arguments validated by the entry points in core.cpp)
// ------------------------------------------------------------------------------------------
int cc_automask_accumulate(const float* y, float* acc, int32_t B, int32_t C, int64_t P, int32_t first, hipStream_t s) {
    static_assert(kMaxChannels == 16, "core.cpp checks C against 16");
    if (P % 4 == 0 && aligned(y, 16) && aligned(acc, 16))
        hipLaunchKernelGGL(automask_accumulate_kernel<4>, dim3(grid_for((int64_t)B * (P / 4))), dim3(kThreads), 0, s, y, acc, B, C, P, first);
    else
        hipLaunchKernelGGL(automask_accumulate_kernel<1>, dim3(grid_for((int64_t)B * P)), dim3(kThreads), 0, s, y, acc, B, C, P, first);
    return cc_launch_status("automask_accumulate");
}

int cc_automask_binarize(const float* acc, const float* scale, float theta, uint8_t* bin, int32_t B, int64_t P, hipStream_t s) {
    if (P % 4 == 0 && aligned(acc, 16) && aligned(bin, 4))
        hipLaunchKernelGGL(automask_binarize_kernel<4>, dim3(grid_for((int64_t)B * (P / 4))), dim3(kThreads), 0, s, acc, scale, theta, bin, B, P);
    else
        hipLaunchKernelGGL(automask_binarize_kernel<1>, dim3(grid_for((int64_t)B * P)), dim3(kThreads), 0, s, acc, scale, theta, bin, B, P);
    return cc_launch_status("automask_binarize");
}

int cc_automask_vote(const uint8_t* bin, uint8_t* out, int32_t B, int32_t T, int32_t h, int32_t w, int32_t votes, hipStream_t s) {
    const int64_t total = (int64_t)B * T * h * w;
    hipLaunchKernelGGL(automask_vote_kernel, dim3(grid_for(total)), dim3(kThreads), 0, s, bin, out, total, T, h, w, votes);
    return cc_launch_status("automask_vote");
}

int cc_automask_expand(const uint8_t* lat, uint8_t* px, int64_t N, int32_t h, int32_t w, hipStream_t s) {
    const int64_t total = N * 8 * h * w;
    hipLaunchKernelGGL(automask_expand_kernel, dim3(grid_for(total)), dim3(kThreads), 0, s, lat, px, total, h, w);
    return cc_launch_status("automask_expand");
}
