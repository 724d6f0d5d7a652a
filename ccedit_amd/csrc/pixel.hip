// Pixel I/O of a clip (include/ccedit_hip.h, "Pixel I/O"): what the sampling entry points did with Pillow / ATen / numpy on the host
// between decoded uint8 frames and the engine's fp32 tensors, and between the decoder's output and the uint8 frames that are written.
//   resize_u8_*      Pillow's 8-bit Image.resize(BICUBIC): two separable integer passes with a uint8 image in between
//   resize_f32       F.interpolate(mode="bicubic", align_corners=False): 4 x 4 fp32 taps, border clamped
//   kth_* / minmax   exact order statistics (radix select) and min / max of fp32 rows
//   depth_hint       raw depth + two device-resident scalars per clip -> 3-channel hint in [-1, 1]
//   frames_to_u8     fp32 planar clip -> uint8 interleaved frames
// All of them move bytes: no LDS staging of pixels, 4- / 16-byte accesses wherever the sizes allow and a one-pixel variant for the
// others.  Every value that the reference computes with one IEEE operation is computed with exactly that operation (__fdiv_rn etc.,
// the file is also compiled with -ffp-contract=off), which is what makes the results bit-identical and not just close.
// The argument checks live with the exported entry points in core.cpp; the launchers below trust their arguments.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPilBits = 22;          // Pillow: PRECISION_BITS = 32 - 8 - 2

inline unsigned blocks_for(int64_t total) { return (unsigned)((total + kThreads - 1) / kThreads); }

// Pillow's clip8: (v >> 22) clamped to 0 ... 255, written as clamp-then-shift (the same value: 0x3FFFFFFF = (256 << 22) - 1).
// The shift-then-clamp form is matched by hipcc to v_ashr_pk_u8_i32 (two results in the low half of a register); on the MI355X the high
// half of its destination came back holding the register's previous contents where the compiler assumes zeros, which OR-ed a stale byte
// into byte 2 of every packed word after the first.  This form compiles to v_med3_i32 + v_lshrrev_b32; tests/test_pixel_io.py checks the object for the other.
__device__ __forceinline__ uint32_t clip8(int v) {
    v = v < 0 ? 0 : (v > 0x3FFFFFFF ? 0x3FFFFFFF : v);
    return (uint32_t)v >> kPilBits;
}

// first tap / tap count of one output coordinate, held inside [0, size) whatever the table says (a wrong table gives wrong pixels, never
// an access outside the image)
__device__ __forceinline__ void tap_window(const int32_t* __restrict__ t, int kmax, int size, int& first, int& cnt) {
    first = t[0];
    first = first < 0 ? 0 : (first > size - 1 ? size - 1 : first);
    cnt = t[1];
    cnt = cnt < 0 ? 0 : (cnt > kmax ? kmax : cnt);
    cnt = cnt > size - first ? size - first : cnt;
}

// ---- Pillow pass 1 (horizontal): src [rows][Ws][3] -> dst [rows][W][3], PX output pixels per thread (PX = 4: W % 4 == 0, three 4-byte stores)
template <int PX>
__global__ __launch_bounds__(kThreads) void resize_u8_h_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                               const int32_t* __restrict__ tab, int kmax, int64_t rows, int Ws, int W) {
    const int G = W / PX;
    const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= rows * G) return;
    const int64_t row = idx / G;
    const int x0 = (int)(idx - row * G) * PX;
    const uint8_t* srow = src + row * Ws * 3;
    uint32_t b[PX * 3];
#pragma unroll
    for (int p = 0; p < PX; ++p) {
        const int32_t* t = tab + (int64_t)(x0 + p) * (kmax + 2);
        int first, cnt;
        tap_window(t, kmax, Ws, first, cnt);
        int a0 = 1 << (kPilBits - 1), a1 = a0, a2 = a0;
        const uint8_t* s = srow + first * 3;
        for (int k = 0; k < cnt; ++k) {
            const int w = t[2 + k];
            a0 += w * s[3 * k];
            a1 += w * s[3 * k + 1];
            a2 += w * s[3 * k + 2];
        }
        b[3 * p] = clip8(a0);
        b[3 * p + 1] = clip8(a1);
        b[3 * p + 2] = clip8(a2);
    }
    uint8_t* d = dst + (row * W + x0) * 3;
    if constexpr (PX == 4) {
#pragma unroll
        for (int j = 0; j < 3; ++j)
            ((uint32_t*)d)[j] = b[4 * j] | (b[4 * j + 1] << 8) | (b[4 * j + 2] << 16) | (b[4 * j + 3] << 24);
    } else {
#pragma unroll
        for (int j = 0; j < 3; ++j) d[j] = (uint8_t)b[j];
    }
}

// ---- Pillow pass 2 (vertical): src [N][Hs][W][3] -> uint8 [N][H][W][3], or (F32) fp32 x / 255 * 2 - 1 into the planar [3][N][H][W]
template <int PX, bool F32>
__global__ __launch_bounds__(kThreads) void resize_u8_v_kernel(const uint8_t* __restrict__ src, void* __restrict__ dst,
                                                               const int32_t* __restrict__ tab, int kmax, int N, int Hs, int H, int W) {
    const int G = W / PX;
    const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= (int64_t)N * H * G) return;
    const int64_t ny = idx / G;
    const int x0 = (int)(idx - ny * G) * PX;
    const int n = (int)(ny / H), yo = (int)(ny - (int64_t)n * H);
    const int32_t* t = tab + (int64_t)yo * (kmax + 2);
    int first, cnt;
    tap_window(t, kmax, Hs, first, cnt);
    int acc[PX * 3];
#pragma unroll
    for (int j = 0; j < PX * 3; ++j) acc[j] = 1 << (kPilBits - 1);
    const uint8_t* s = src + (((int64_t)n * Hs + first) * W + x0) * 3;
    for (int k = 0; k < cnt; ++k, s += (int64_t)W * 3) {
        const int w = t[2 + k];
        if constexpr (PX == 4) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const uint32_t v = ((const uint32_t*)s)[j];
                acc[4 * j] += w * (int)(v & 255u);
                acc[4 * j + 1] += w * (int)((v >> 8) & 255u);
                acc[4 * j + 2] += w * (int)((v >> 16) & 255u);
                acc[4 * j + 3] += w * (int)(v >> 24);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 3; ++j) acc[j] += w * (int)s[j];
        }
    }
    if constexpr (F32) {
        float* o = (float*)dst;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float f[PX];
#pragma unroll
            for (int p = 0; p < PX; ++p)          // the reference: tensor.float() / 255.0, then * 2.0 - 1.0 (the clamp after it never acts)
                f[p] = __fsub_rn(__fmul_rn(__fdiv_rn((float)clip8(acc[3 * p + c]), 255.0f), 2.0f), 1.0f);
            float* oc = o + (((int64_t)c * N + n) * H + yo) * W + x0;
            if constexpr (PX == 4) {
                *(f32x4*)oc = f32x4{f[0], f[1], f[2], f[3]};
            } else {
                oc[0] = f[0];
            }
        }
    } else {
        uint8_t* d = (uint8_t*)dst + (((int64_t)n * H + yo) * W + x0) * 3;
        if constexpr (PX == 4) {
#pragma unroll
            for (int j = 0; j < 3; ++j)
                ((uint32_t*)d)[j] = clip8(acc[4 * j]) | (clip8(acc[4 * j + 1]) << 8) | (clip8(acc[4 * j + 2]) << 16) | (clip8(acc[4 * j + 3]) << 24);
        } else {
#pragma unroll
            for (int j = 0; j < 3; ++j) d[j] = (uint8_t)clip8(acc[j]);
        }
    }
}

// ---- ATen bicubic: src fp32 [planes][Hs][Ws] -> dst [planes][H][W]; out = sum_j wy_j (sum_i wx_i src[y_j][x_i]), taps clamped to the border
template <int PX>
__global__ __launch_bounds__(kThreads) void resize_f32_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                              const int32_t* __restrict__ ytab, const int32_t* __restrict__ xtab,
                                                              int64_t planes, int Hs, int Ws, int H, int W) {
    const int G = W / PX;
    const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= planes * H * G) return;
    const int64_t py = idx / G;
    const int x0 = (int)(idx - py * G) * PX;
    const int64_t pl = py / H;
    const int yo = (int)(py - pl * H);
    const int32_t* ty = ytab + (int64_t)yo * 6;
    const float* sp = src + pl * Hs * Ws;
    float out[PX];
#pragma unroll
    for (int p = 0; p < PX; ++p) out[p] = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int y = ty[0] + j;
        y = y < 0 ? 0 : (y > Hs - 1 ? Hs - 1 : y);
        const float wy = __int_as_float(ty[2 + j]);
        const float* sr = sp + (int64_t)y * Ws;
#pragma unroll
        for (int p = 0; p < PX; ++p) {
            const int32_t* tx = xtab + (int64_t)(x0 + p) * 6;
            float r = 0.0f;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                int x = tx[0] + i;
                x = x < 0 ? 0 : (x > Ws - 1 ? Ws - 1 : x);
                r += __int_as_float(tx[2 + i]) * sr[x];
            }
            out[p] += wy * r;
        }
    }
    float* d = dst + (pl * H + yo) * W + x0;
    if constexpr (PX == 4) {
        *(f32x4*)d = f32x4{out[0], out[1], out[2], out[3]};
    } else {
        d[0] = out[0];
    }
}

// ---- order statistics.  key(): the unsigned integer whose order is the order of the (finite) floats; -0.0 sorts just below +0.0.
__device__ __forceinline__ uint32_t f2key(float f) {
    const uint32_t u = __float_as_uint(f);
    return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float key2f(uint32_t k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu)); }

constexpr int kMaxRanks = 4;
struct KthRanks {
    uint32_t k[kMaxRanks];
};
// workspace (uint32): state [B][4][2] = (key prefix decided so far, rank left inside it), then hist [B][4][256]
__device__ __forceinline__ uint32_t* kth_state(uint32_t* ws, int row) { return ws + (int64_t)row * kMaxRanks * 2; }
__device__ __forceinline__ uint32_t* kth_hist(uint32_t* ws, int B, int row) { return ws + (int64_t)B * kMaxRanks * 2 + (int64_t)row * kMaxRanks * 256; }

__global__ void kth_init_kernel(uint32_t* ws, int B, KthRanks ranks) {
    const int64_t total = (int64_t)B * kMaxRanks * (2 + 256);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        uint32_t v = 0;
        if (i < (int64_t)B * kMaxRanks * 2 && (i & 1)) v = ranks.k[(i >> 1) % kMaxRanks];
        ws[i] = v;
    }
}

// ranks whose decided prefixes agree count the same elements: only the first of them (its "owner") keeps a histogram
__device__ __forceinline__ int kth_owner(const uint32_t* prefix, int r) {
    int o = r;
    for (int q = r - 1; q >= 0; --q)
        if (prefix[q] == prefix[r]) o = q;
    return o;
}

// one 8-bit digit: histogram of digit `shift` over the elements whose higher bits equal a rank's prefix; LDS atomics, merged into the global table
__global__ __launch_bounds__(kThreads) void kth_hist_kernel(const float* __restrict__ x, int64_t n, uint32_t* ws, int B, int nr, int shift) {
    __shared__ uint32_t h[kMaxRanks][256];
    const int row = blockIdx.y;
    const uint32_t* st = kth_state(ws, row);
    uint32_t prefix[kMaxRanks];
    bool own[kMaxRanks];
#pragma unroll
    for (int r = 0; r < kMaxRanks; ++r) prefix[r] = r < nr ? st[2 * r] : 0u;
#pragma unroll
    for (int r = 0; r < kMaxRanks; ++r) own[r] = r < nr && kth_owner(prefix, r) == r;
    for (int j = threadIdx.x; j < kMaxRanks * 256; j += kThreads) (&h[0][0])[j] = 0;
    __syncthreads();
    const uint32_t himask = shift == 24 ? 0u : (0xFFFFFFFFu << (shift + 8));
    const float* xr = x + (int64_t)row * n;
    auto count = [&](float f) {
        const uint32_t key = f2key(f);
#pragma unroll
        for (int r = 0; r < kMaxRanks; ++r)
            if (own[r] && (key & himask) == prefix[r]) atomicAdd(&h[r][(key >> shift) & 255u], 1u);
    };
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    if (((n & 3) == 0) && (((uintptr_t)x & 15) == 0)) {
        const f32x4* x4 = (const f32x4*)xr;
        for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n / 4; i += stride) {
            const f32x4 v = x4[i];
            count(v[0]);
            count(v[1]);
            count(v[2]);
            count(v[3]);
        }
    } else {
        for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) count(xr[i]);
    }
    __syncthreads();
    uint32_t* gh = kth_hist(ws, B, row);
    for (int j = threadIdx.x; j < kMaxRanks * 256; j += kThreads) {
        const uint32_t c = (&h[0][0])[j];
        if (c) atomicAdd(gh + j, c);
    }
}

// after a digit's histogram: per rank the digit whose cumulative count reaches the rank; the prefix grows by it, the rank becomes the rank
// inside that digit, the table is cleared for the next digit; after the last digit the prefix IS the key of the answer
__global__ __launch_bounds__(256) void kth_select_kernel(uint32_t* ws, int B, int nr, int shift, float* __restrict__ out) {
    __shared__ uint32_t s[256];
    __shared__ uint32_t nstate[kMaxRanks][2];
    const int row = blockIdx.x, tid = threadIdx.x;
    uint32_t* st = kth_state(ws, row);
    uint32_t* gh = kth_hist(ws, B, row);
    uint32_t prefix[kMaxRanks];
#pragma unroll
    for (int r = 0; r < kMaxRanks; ++r) prefix[r] = r < nr ? st[2 * r] : 0u;
    for (int r = 0; r < nr; ++r) {
        const uint32_t k = st[2 * r + 1];
        const uint32_t c = gh[kth_owner(prefix, r) * 256 + tid];
        s[tid] = c;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {          // inclusive scan over the 256 bins
            const uint32_t add = tid >= o ? s[tid - o] : 0u;
            __syncthreads();
            s[tid] += add;
            __syncthreads();
        }
        const uint32_t incl = s[tid], excl = incl - c;
        if (excl < k && k <= incl) {                 // exactly one bin (1 <= k <= number of elements under the prefix)
            nstate[r][0] = prefix[r] | ((uint32_t)tid << shift);
            nstate[r][1] = k - excl;
        }
        __syncthreads();
    }
    for (int j = tid; j < kMaxRanks * 256; j += 256) gh[j] = 0;
    if (tid < nr) {
        st[2 * tid] = nstate[tid][0];
        st[2 * tid + 1] = nstate[tid][1];
        if (shift == 0) out[(int64_t)row * nr + tid] = key2f(nstate[tid][0]);
    }
}

// ---- min / max per row, on the keys: out [B][2] holds (min key, max key) while the reduction runs, floats after the last kernel
__global__ void minmax_init_kernel(uint32_t* out, int B) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 2 * B) out[i] = (i & 1) ? 0u : 0xFFFFFFFFu;
}
__global__ __launch_bounds__(kThreads) void minmax_kernel(const float* __restrict__ x, int64_t n, uint32_t* out) {
    const int row = blockIdx.y;
    const float* xr = x + (int64_t)row * n;
    uint32_t lo = 0xFFFFFFFFu, hi = 0u;
    auto take = [&](float f) {
        const uint32_t k = f2key(f);
        lo = k < lo ? k : lo;
        hi = k > hi ? k : hi;
    };
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    if (((n & 3) == 0) && (((uintptr_t)x & 15) == 0)) {
        const f32x4* x4 = (const f32x4*)xr;
        for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n / 4; i += stride) {
            const f32x4 v = x4[i];
            take(v[0]);
            take(v[1]);
            take(v[2]);
            take(v[3]);
        }
    } else {
        for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) take(xr[i]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t l2 = __shfl_xor(lo, o, 64), h2 = __shfl_xor(hi, o, 64);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMin(out + 2 * row, lo);
        atomicMax(out + 2 * row + 1, hi);
    }
}
__global__ void minmax_final_kernel(uint32_t* out, int B) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 2 * B) ((float*)out)[i] = key2f(out[i]);
}

// ---- depth hint: v = (d - lo) / (hi - lo), clamp to [0, 1] (NaN stays NaN, as torch.clamp), v * 2 - 1, optional sign flip, three channels
template <int V>
__global__ __launch_bounds__(kThreads) void depth_hint_kernel(const float* __restrict__ d, float* __restrict__ out,
                                                              const float* __restrict__ stats, int stat_stride, int64_t n, int flip) {
    const int b = blockIdx.y;
    const int64_t i = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * V;
    if (i >= n) return;
    const float lo = stats[(int64_t)b * stat_stride], hi = stats[(int64_t)b * stat_stride + 1];
    const float den = __fsub_rn(hi, lo);
    float v[V];
    if constexpr (V == 4) {
        const f32x4 q = *(const f32x4*)(d + (int64_t)b * n + i);
        v[0] = q[0], v[1] = q[1], v[2] = q[2], v[3] = q[3];
    } else {
        v[0] = d[(int64_t)b * n + i];
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
        float t = __fdiv_rn(__fsub_rn(v[j], lo), den);
        t = t < 0.0f ? 0.0f : (t > 1.0f ? 1.0f : t);
        t = __fsub_rn(__fmul_rn(t, 2.0f), 1.0f);
        v[j] = flip ? -t : t;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float* o = out + ((int64_t)b * 3 + c) * n + i;
        if constexpr (V == 4) {
            *(f32x4*)o = f32x4{v[0], v[1], v[2], v[3]};
        } else {
            o[0] = v[0];
        }
    }
}

// ---- decoder output -> uint8 frames: x fp32 [B][3][P] (P = T H W) -> [B][P][3]; PX pixels per thread (16: three 16-byte stores)
template <int PX>
__global__ __launch_bounds__(kThreads) void frames_to_u8_kernel(const float* __restrict__ x, uint8_t* __restrict__ out, int64_t P, int mode,
                                                                int unit_range) {
    const int b = blockIdx.y;
    const int64_t p0 = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * PX;
    if (p0 >= P) return;
    uint32_t q[3][PX];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* xc = x + ((int64_t)b * 3 + c) * P + p0;
        float f[PX];
        if constexpr (PX % 4 == 0) {
#pragma unroll
            for (int j = 0; j < PX / 4; ++j) {
                const f32x4 v = ((const f32x4*)xc)[j];
                f[4 * j] = v[0], f[4 * j + 1] = v[1], f[4 * j + 2] = v[2], f[4 * j + 3] = v[3];
            }
        } else {
            f[0] = xc[0];
        }
#pragma unroll
        for (int j = 0; j < PX; ++j) {
            float v = unit_range ? f[j] : __fdiv_rn(__fadd_rn(f[j], 1.0f), 2.0f);
            v = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);          // NaN (never produced by the decoder) falls through to 0 below
            v = __fmul_rn(255.0f, v);
            if (mode == 1) {
                v = __fadd_rn(v, 0.5f);
                v = v > 255.0f ? 255.0f : v;
            }
            q[c][j] = v >= 0.0f ? (uint32_t)v : 0u;                // truncation, as astype(uint8) of a value in [0, 255.5)
        }
    }
    uint8_t* o = out + ((int64_t)b * P + p0) * 3;
    if constexpr (PX % 4 == 0) {
        uint32_t w[PX * 3 / 4];
#pragma unroll
        for (int j = 0; j < PX * 3 / 4; ++j) {
            uint32_t acc = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int byte = 4 * j + e;
                acc |= q[byte % 3][byte / 3] << (8 * e);
            }
            w[j] = acc;
        }
#pragma unroll
        for (int j = 0; j < PX * 3 / 16; ++j) ((u32x4*)o)[j] = u32x4{w[4 * j], w[4 * j + 1], w[4 * j + 2], w[4 * j + 3]};
    } else {
        o[0] = (uint8_t)q[0][0];
        o[1] = (uint8_t)q[1][0];
        o[2] = (uint8_t)q[2][0];
    }
}

inline bool aligned(const void* p, unsigned a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

// ------------------------------------------------------------------------------------------
// launchers (arguments validated by the entry points in core.cpp)
// ------------------------------------------------------------------------------------------
int cc_pixel_resize_u8(const uint8_t* src, void* dst, uint8_t* tmp, const int32_t* ytab, int32_t yk, const int32_t* xtab, int32_t xk,
                       int32_t N, int32_t Hs, int32_t Ws, int32_t H, int32_t W, int32_t out_f32, hipStream_t s) {
    const uint8_t* mid = src;
    if (xtab) {                                   // horizontal pass first, over every source row (Pillow's order)
        const int64_t rows = (int64_t)N * Hs;
        if (W % 4 == 0 && aligned(tmp, 4))
            hipLaunchKernelGGL(resize_u8_h_kernel<4>, dim3(blocks_for(rows * (W / 4))), dim3(kThreads), 0, s, src, tmp, xtab, xk, rows, Ws, W);
        else
            hipLaunchKernelGGL(resize_u8_h_kernel<1>, dim3(blocks_for(rows * W)), dim3(kThreads), 0, s, src, tmp, xtab, xk, rows, Ws, W);
        mid = tmp;
    }
    const bool vec = W % 4 == 0 && aligned(mid, 4) && aligned(dst, out_f32 ? 16 : 4);
    const int64_t total = (int64_t)N * H * (vec ? W / 4 : W);
#define CC_V(PX, F) hipLaunchKernelGGL((resize_u8_v_kernel<PX, F>), dim3(blocks_for(total)), dim3(kThreads), 0, s, mid, dst, ytab, yk, N, Hs, H, W)
    if (vec && out_f32) CC_V(4, true);
    else if (vec) CC_V(4, false);
    else if (out_f32) CC_V(1, true);
    else CC_V(1, false);
#undef CC_V
    return cc_launch_status("resize_u8_pil");
}

int cc_pixel_resize_f32(const float* src, float* dst, const int32_t* ytab, const int32_t* xtab, int64_t planes, int32_t Hs, int32_t Ws,
                        int32_t H, int32_t W, hipStream_t s) {
    if (W % 4 == 0 && aligned(dst, 16))
        hipLaunchKernelGGL(resize_f32_kernel<4>, dim3(blocks_for(planes * H * (W / 4))), dim3(kThreads), 0, s, src, dst, ytab, xtab, planes, Hs, Ws, H, W);
    else
        hipLaunchKernelGGL(resize_f32_kernel<1>, dim3(blocks_for(planes * H * W)), dim3(kThreads), 0, s, src, dst, ytab, xtab, planes, Hs, Ws, H, W);
    return cc_launch_status("resize_f32_bicubic");
}

static unsigned stream_blocks(int64_t n) {        // grid-stride readers: ~16 values per thread, at most 2048 workgroups per row
    int64_t g = (n + kThreads * 16 - 1) / (kThreads * 16);
    return (unsigned)(g < 1 ? 1 : (g > 2048 ? 2048 : g));
}

int cc_pixel_kth_values(const float* x, int32_t B, int64_t n, const int64_t* ranks, int32_t nr, float* out, void* workspace, hipStream_t s) {
    KthRanks kr = {};
    for (int r = 0; r < nr; ++r) kr.k[r] = (uint32_t)ranks[r];
    uint32_t* ws = (uint32_t*)workspace;
    hipLaunchKernelGGL(kth_init_kernel, dim3(blocks_for((int64_t)B * kMaxRanks * 258)), dim3(kThreads), 0, s, ws, B, kr);
    for (int shift = 24; shift >= 0; shift -= 8) {
        hipLaunchKernelGGL(kth_hist_kernel, dim3(stream_blocks(n), B), dim3(kThreads), 0, s, x, n, ws, B, nr, shift);
        hipLaunchKernelGGL(kth_select_kernel, dim3(B), dim3(256), 0, s, ws, B, nr, shift, out);
    }
    return cc_launch_status("kth_values");
}

int cc_pixel_minmax(const float* x, int32_t B, int64_t n, float* out, hipStream_t s) {
    hipLaunchKernelGGL(minmax_init_kernel, dim3(blocks_for(2 * (int64_t)B)), dim3(kThreads), 0, s, (uint32_t*)out, B);
    hipLaunchKernelGGL(minmax_kernel, dim3(stream_blocks(n), B), dim3(kThreads), 0, s, x, n, (uint32_t*)out);
    hipLaunchKernelGGL(minmax_final_kernel, dim3(blocks_for(2 * (int64_t)B)), dim3(kThreads), 0, s, (uint32_t*)out, B);
    return cc_launch_status("minmax_f32");
}

int cc_pixel_depth_hint(const float* depth, float* hint, const float* stats, int32_t stat_stride, int32_t B, int64_t n, int32_t flip,
                        hipStream_t s) {
    if (n % 4 == 0 && aligned(depth, 16) && aligned(hint, 16))
        hipLaunchKernelGGL(depth_hint_kernel<4>, dim3(blocks_for(n / 4), B), dim3(kThreads), 0, s, depth, hint, stats, stat_stride, n, flip);
    else
        hipLaunchKernelGGL(depth_hint_kernel<1>, dim3(blocks_for(n), B), dim3(kThreads), 0, s, depth, hint, stats, stat_stride, n, flip);
    return cc_launch_status("depth_hint");
}

int cc_pixel_frames_to_u8(const float* x, uint8_t* out, int32_t B, int64_t P, int32_t mode, int32_t unit_range, hipStream_t s) {
    if (P % 16 == 0 && aligned(x, 16) && aligned(out, 16))
        hipLaunchKernelGGL(frames_to_u8_kernel<16>, dim3(blocks_for(P / 16), B), dim3(kThreads), 0, s, x, out, P, mode, unit_range);
    else
        hipLaunchKernelGGL(frames_to_u8_kernel<1>, dim3(blocks_for(P), B), dim3(kThreads), 0, s, x, out, P, mode, unit_range);
    return cc_launch_status("frames_to_u8");
}
