// Weighted prompts (include/ccedit_hip.h, "Prompts"): the emphasis rule of `--prompt_syntax weighted` on the CLIP text encoder's output.
//   prompt_weight   out[b][t][:] = e[t mod 77][:] + w[b][t] * (z[b][t][:] - e[t mod 77][:])
// z is the encoding (B, L = 77 n, C) of the prompt's chunks, e the encoding (77, C) of the EMPTY chunk (BOS, EOS x 76) and w the
// per-token weight: a token moves from where the empty prompt puts its position towards (w < 1), onto (w = 1) or past (w > 1) where
// its own prompt puts it.  No mean over the sequence, no reduction: a row depends on nothing but itself.
// Arithmetic: fp32 subtract, multiply, add, each rounded, in that order (the file is compiled with -ffp-contract=off: no fma).
// A row with w == 1 is a BIT COPY of z: e + (z - e) is not z in floating point, so it is a branch (as region_fuse copies cells with
// one owner) — a prompt without emphasis is encoded exactly as without the rule.  w is data: it is read from device memory, the
// host wrapper refuses NaN / inf before the launch, and the kernel itself has no index that depends on it.
// Mechanics: grid-stride loop over a grid of at most kMaxBlocks workgroups, one thread per V consecutive channels of a row, 16-byte
// accesses where C % 4 == 0 and the pointers allow, a one-element variant otherwise.  The row of e is (row mod 77): in range by
// construction.  out may alias z (every element is read and written by the same thread).
//
// Prompt schedules (include/ccedit_hip.h, "Prompt schedules"): a context per keyframe from P encoded prompts and a per-frame table.
//   prompt_schedule out[f][:][:] = c[k0[f]]                                    where a[f] == 0   (bit copy)
//                                  c[k1[f]]                                    where a[f] == 1   (bit copy)
//                                  c[k0[f]] + a[f] * (c[k1[f]] - c[k0[f]])     otherwise: subtract, multiply, add, each rounded
// The table (k0, k1, a) is HOST data: the entry point range-checks k0 / k1 against P and the launcher hands the table to the kernel BY
// VALUE, kSchedFrames frames to a launch (one launch up to that many frames), so the indices the kernel uses are the ones that were
// checked.  blockIdx.y is the frame: its table entry is uniform over the workgroup.  No reduction; out must not alias c.
// The argument checks live with the exported entry point in core.cpp; the launchers below trust their arguments.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 256 * 8;          // 256 CUs x 8 workgroups of 4 waves
constexpr int kChunk = 77;                   // rows of e: one CLIP chunk

inline unsigned grid_for(int64_t items) {
    const int64_t g = (items + kThreads - 1) / kThreads;
    return (unsigned)(g < 1 ? 1 : (g > kMaxBlocks ? kMaxBlocks : g));
}
inline bool aligned(const void* p, unsigned a) { return ((uintptr_t)p & (a - 1)) == 0; }

template <int V>
__global__ __launch_bounds__(kThreads) void prompt_weight_kernel(const float* z, const float* __restrict__ e, const float* __restrict__ w, float* out,
                                                                 int64_t R, int C) {
    const int CV = C / V;
    const int64_t total = R * CV;
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * kThreads) {
        const int64_t row = idx / CV;                              // b * L + t; L is a multiple of 77, so row mod 77 == t mod 77
        const int c = (int)(idx - row * CV) * V;
        const int64_t at = row * C + c;
        const float wv = w[row];
        float zv[V];
        if constexpr (V == 4) {
            const f32x4 q = *(const f32x4*)(z + at);
            zv[0] = q[0], zv[1] = q[1], zv[2] = q[2], zv[3] = q[3];
        } else {
            zv[0] = z[at];
        }
        if (wv != 1.0f) {                                          // (w == 1: the bits of z go out as they came in)
            const float* er = e + (int64_t)(row % kChunk) * C + c;
            float ev[V];
            if constexpr (V == 4) {
                const f32x4 q = *(const f32x4*)er;
                ev[0] = q[0], ev[1] = q[1], ev[2] = q[2], ev[3] = q[3];
            } else {
                ev[0] = er[0];
            }
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float d = zv[j] - ev[j];                     // three roundings: no fma (-ffp-contract=off)
                const float m = wv * d;
                zv[j] = ev[j] + m;
            }
        }
        if constexpr (V == 4)
            *(f32x4*)(out + at) = f32x4{zv[0], zv[1], zv[2], zv[3]};
        else
            out[at] = zv[0];
    }
}

constexpr int kSchedFrames = 256;            // frames of one launch: the table travels as 3 KiB of kernel arguments
struct SchedTable {
    int32_t k0[kSchedFrames], k1[kSchedFrames];
    float a[kSchedFrames];
};

template <int V>
__global__ __launch_bounds__(kThreads) void prompt_schedule_kernel(const float* __restrict__ c, float* __restrict__ out, const SchedTable tab,
                                                                   int64_t LC) {
    const int f = blockIdx.y;
    const float av = tab.a[f];
    const float* c0 = c + (int64_t)tab.k0[f] * LC;
    const float* c1 = c + (int64_t)tab.k1[f] * LC;
    float* o = out + (int64_t)f * LC;
    const int64_t total = LC / V;
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * kThreads) {
        const int64_t at = idx * V;
        if (av == 0.0f || av == 1.0f) {                            // (the bits of one prompt go out as they came in, -0.0 included)
            const float* src = av == 0.0f ? c0 : c1;
            if constexpr (V == 4)
                *(f32x4*)(o + at) = *(const f32x4*)(src + at);
            else
                o[at] = src[at];
            continue;
        }
        float x0[V], x1[V];
        if constexpr (V == 4) {
            const f32x4 p = *(const f32x4*)(c0 + at), q = *(const f32x4*)(c1 + at);
            x0[0] = p[0], x0[1] = p[1], x0[2] = p[2], x0[3] = p[3];
            x1[0] = q[0], x1[1] = q[1], x1[2] = q[2], x1[3] = q[3];
        } else {
            x0[0] = c0[at], x1[0] = c1[at];
        }
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float d = x1[j] - x0[j];                         // three roundings: no fma (-ffp-contract=off)
            const float m = av * d;
            x0[j] = x0[j] + m;
        }
        if constexpr (V == 4)
            *(f32x4*)(o + at) = f32x4{x0[0], x0[1], x0[2], x0[3]};
        else
            o[at] = x0[0];
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------
// launcher (arguments validated by the entry point in core.cpp)
// ------------------------------------------------------------------------------------------
int cc_prompt_weight(const float* z, const float* e, const float* w, float* out, int64_t R, int32_t C, hipStream_t s) {
    if (C % 4 == 0 && aligned(z, 16) && aligned(e, 16) && aligned(out, 16))
        hipLaunchKernelGGL(prompt_weight_kernel<4>, dim3(grid_for(R * (C / 4))), dim3(kThreads), 0, s, z, e, w, out, R, C);
    else
        hipLaunchKernelGGL(prompt_weight_kernel<1>, dim3(grid_for(R * C)), dim3(kThreads), 0, s, z, e, w, out, R, C);
    return cc_launch_status("prompt_weight");
}

// k0 / k1 / a: HOST tables of N entries, every index already checked against P by the entry point
int cc_prompt_schedule(const float* c, const int32_t* k0, const int32_t* k1, const float* a, float* out, int32_t N, int32_t L, int32_t C,
                       hipStream_t s) {
    const int64_t LC = (int64_t)L * C;
    const bool vec = C % 4 == 0 && aligned(c, 16) && aligned(out, 16);
    for (int32_t f0 = 0; f0 < N; f0 += kSchedFrames) {
        const int32_t n = N - f0 < kSchedFrames ? N - f0 : kSchedFrames;
        SchedTable tab;
        for (int32_t i = 0; i < kSchedFrames; ++i) {
            tab.k0[i] = i < n ? k0[f0 + i] : 0;
            tab.k1[i] = i < n ? k1[f0 + i] : 0;
            tab.a[i] = i < n ? a[f0 + i] : 0.0f;
        }
        float* o = out + (int64_t)f0 * LC;
        const unsigned gx = grid_for(vec ? LC / 4 : LC);
        if (vec)
            hipLaunchKernelGGL(prompt_schedule_kernel<4>, dim3(gx > 64 ? 64 : gx, n), dim3(kThreads), 0, s, c, o, tab, LC);
        else
            hipLaunchKernelGGL(prompt_schedule_kernel<1>, dim3(gx > 64 ? 64 : gx, n), dim3(kThreads), 0, s, c, o, tab, LC);
    }
    return cc_launch_status("prompt_schedule");
}
