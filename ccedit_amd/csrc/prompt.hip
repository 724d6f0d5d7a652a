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
// The argument checks live with the exported entry point in core.cpp; the launcher below trusts its arguments.
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
