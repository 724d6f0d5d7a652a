// Region prompts (include/ccedit_hip.h, "Regions"): a prompt per masked region of the frame.  At every network evaluation the network runs
// once per prompt at its usual shape and the K + 1 denoised latents are blended into one by fixed per-cell coefficients
// (ccedit_amd/regions.py; MultiDiffusion along the conditioning axis, as window.hip is along time and tile.hip along space).
//   region_weights   K pixel masks uint8 [K][T][H][W] -> coef fp32 [K + 1][T][h][w], h = H / 8, w = W / 8, in one launch:
//                      a_r = set pixels (byte >= 128) of a latent cell, 0 ... 64
//                      s_r = sum of a_r over the (2F + 1)^2 cells around it, coordinates clamped into the frame, 0 ... S = 64 (2F + 1)^2
//                      tot = sum_r s_r, D = max(S, tot), s_0 = D - tot, coef[r] = float(double(s_r) / double(D)): integers, one quotient
//                      in float64, one conversion — tests/_regions_numpy.py bit for bit
//   region_fuse      out[bc][t][p] = sum over r = 0 ... K, ascending, of coef[r][t][p] * y_r[bc][t][p], terms whose coefficient is exactly 0
//                    SKIPPED (a NaN of a region that does not own a cell never reaches it); y_r through a device table of K + 1 pointers,
//                    every output element written exactly once, no atomics
// region_weights: one workgroup of 256 threads per (frame, tile of 16 x 16 latent cells).  Per region the cell counts of the tile and
// its apron of F cells are staged in LDS — every cell of the frame the apron touches is counted ONCE, from 16-byte row loads where the
// rows allow (two cells per load: popcount of the bytes' top bits), and written to every apron slot that clamps to it — then summed
// along the rows and along the columns in LDS (separable), and the thread of a cell keeps s_r in a register until all K are known.
// LDS row stride of the apron is 48 words (16 mod 32): the two rows a 32-lane group reads in the row pass fall on different banks.
// region_fuse moves bytes like window_fuse: grid-stride loop, 16-byte accesses where P % 4 == 0 and the pointers allow, a one-element
// variant otherwise; a region tensor that is not 16-byte aligned is read element by element, and four elements whose coefficients
// are all 0 are not read at all.  The file is compiled with -ffp-contract=off and without any fast-math flag: the first term of a
// sum is the product alone, every further term one multiply and then one add, and the float64 division is the correctly rounded one.
// The argument checks live with the exported entry points in core.cpp; the launchers below trust their arguments.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 256 * 8;          // 256 CUs x 8 workgroups of 4 waves
constexpr int kMaxRegions = 7;               // K; the fuse walks K + 1 tensors
constexpr int kMaxFeather = 8;               // F
constexpr int kTile = 16;                    // latent cells per tile side: 256 threads, one per cell
constexpr int kApron = kTile + 2 * kMaxFeather;      // 32
constexpr int kApronStride = 48;             // words per apron row in LDS (see above)

inline unsigned grid_for(int64_t items) {
    const int64_t g = (items + kThreads - 1) / kThreads;
    return (unsigned)(g < 1 ? 1 : (g > kMaxBlocks ? kMaxBlocks : g));
}
inline bool aligned(const void* p, unsigned a) { return ((uintptr_t)p & (a - 1)) == 0; }

__device__ inline int popc_top(uint32_t v) { return __popc(v & 0x80808080u); }

// ---- weights.  WIDE: W % 16 == 0 and the masks 16-byte aligned — a 16-byte load is two whole cells of one pixel row.
template <bool WIDE>
__global__ __launch_bounds__(kThreads) void region_weights_kernel(const uint8_t* __restrict__ masks, float* __restrict__ coef, int K, int T, int h,
                                                                  int w, int F, int tiles_y, int tiles_x) {
    __shared__ int apron[kApron * kApronStride];           // counts of the tile and its apron, clamped into the frame
    __shared__ int rows[kApron * kTile];                   // sums along the rows: rows[ai][tj] = sum_d apron[ai][tj + d]
    int blk = (int)blockIdx.x;
    const int bx = blk % tiles_x;
    blk /= tiles_x;
    const int by = blk % tiles_y;
    const int t = blk / tiles_y;
    if (t >= T) return;                                    // (uniform: the grid is exactly T tiles_y tiles_x)
    const int i0 = by * kTile, j0 = bx * kTile;            // first cell of the tile; i0 < h, j0 < w
    const int AH = kTile + 2 * F, AW = kTile + 2 * F;
    // the cells of the frame the apron touches (clamped at both ends: F may exceed h or w)
    const int ilo = max(i0 - F, 0), ihi = min(i0 + kTile - 1 + F, h - 1);
    const int jlo = max(j0 - F, 0), jhi = min(j0 + kTile - 1 + F, w - 1);
    const int R = ihi - ilo + 1;
    const int G = WIDE ? (jhi >> 1) - (jlo >> 1) + 1 : jhi - jlo + 1;          // loads per cell row: cell pairs / cells
    const int64_t Wpx = (int64_t)w * 8;
    const int ti = (int)threadIdx.x / kTile, tj = (int)threadIdx.x % kTile;
    int s[kMaxRegions];
#pragma unroll
    for (int r = 0; r < kMaxRegions; ++r) s[r] = 0;

#pragma unroll
    for (int r = 0; r < kMaxRegions; ++r) {
        if (r < K) {                                       // (uniform)
            const uint8_t* frame = masks + ((int64_t)r * T + t) * (int64_t)h * 8 * Wpx;
            for (int e = (int)threadIdx.x; e < R * G; e += kThreads) {
                const int ci = ilo + e / G;
                const int g = e % G;
                int cnt[2] = {0, 0};
                int cj;
                if constexpr (WIDE) {
                    cj = ((jlo >> 1) + g) * 2;             // an even cell; cj + 1 <= w - 1 because w is even here
                    const uint8_t* p = frame + (int64_t)ci * 8 * Wpx + (int64_t)cj * 8;
#pragma unroll
                    for (int y = 0; y < 8; ++y) {
                        const u32x4 v = *(const u32x4*)(p + y * Wpx);
                        cnt[0] += popc_top(v[0]) + popc_top(v[1]);
                        cnt[1] += popc_top(v[2]) + popc_top(v[3]);
                    }
                } else {
                    cj = jlo + g;
                    const uint8_t* p = frame + (int64_t)ci * 8 * Wpx + (int64_t)cj * 8;
#pragma unroll
                    for (int y = 0; y < 8; ++y) {
                        const u32x2 v = *(const u32x2*)(p + y * Wpx);
                        cnt[0] += popc_top(v[0]) + popc_top(v[1]);
                    }
                }
                // every apron slot that clamps to this cell: its own, and at a border of the frame everything beyond it
                const int a0 = ci == 0 ? 0 : ci - i0 + F, a1 = ci == h - 1 ? AH - 1 : ci - i0 + F;
#pragma unroll
                for (int c = 0; c < (WIDE ? 2 : 1); ++c) {
                    const int cc = cj + c;
                    if (cc < jlo || cc > jhi) continue;
                    const int b0 = cc == 0 ? 0 : cc - j0 + F, b1 = cc == w - 1 ? AW - 1 : cc - j0 + F;
                    for (int a = a0; a <= a1; ++a)
                        for (int b = b0; b <= b1; ++b) apron[a * kApronStride + b] = cnt[c];
                }
            }
            __syncthreads();
            for (int e = (int)threadIdx.x; e < AH * kTile; e += kThreads) {
                const int a = e / kTile, b = e % kTile;
                int acc = 0;
                for (int d = 0; d <= 2 * F; ++d) acc += apron[a * kApronStride + b + d];
                rows[e] = acc;
            }
            __syncthreads();
            int acc = 0;
            for (int d = 0; d <= 2 * F; ++d) acc += rows[(ti + d) * kTile + tj];
            s[r] = acc;
            // (the next region's row pass writes `rows` only after the barrier that follows its staging: every thread is past this read)
        }
    }

    const int i = i0 + ti, j = j0 + tj;
    if (i >= h || j >= w) return;
    int tot = 0;
#pragma unroll
    for (int r = 0; r < kMaxRegions; ++r) tot += s[r];
    const int S = 64 * (2 * F + 1) * (2 * F + 1);
    const int D = tot > S ? tot : S;
    const double dd = (double)D;
    const int64_t plane = (int64_t)T * h * w;
    float* o = coef + ((int64_t)t * h + i) * w + j;
    o[0] = (float)((double)(D - tot) / dd);
#pragma unroll
    for (int r = 0; r < kMaxRegions; ++r)
        if (r < K) o[(int64_t)(r + 1) * plane] = (float)((double)s[r] / dd);
}

// ---- fuse: one thread per V consecutive output elements of a frame; the regions are walked in ascending r.
template <int V>
__global__ __launch_bounds__(kThreads) void region_fuse_kernel(const float* const* __restrict__ yr, float* __restrict__ out,
                                                               const float* __restrict__ coef, int R, int64_t BC, int T, int64_t P) {
    const int64_t PV = P / V;
    const int64_t TP = (int64_t)T * P;
    const int64_t total = BC * T * PV;
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * kThreads) {
        const int64_t bf = idx / PV;                               // bc * T + t
        const int64_t p = (idx - bf * PV) * V;
        const int64_t tp = (bf % T) * P + p;                       // offset inside one region's coefficient plane
        float acc[V];
        bool first[V];
#pragma unroll
        for (int v = 0; v < V; ++v) acc[v] = 0.0f, first[v] = true;
        for (int r = 0; r < R; ++r) {
            float cf[V];
            if constexpr (V == 4) {
                const f32x4 q = *(const f32x4*)(coef + (int64_t)r * TP + tp);
                cf[0] = q[0], cf[1] = q[1], cf[2] = q[2], cf[3] = q[3];
                if (cf[0] == 0.0f && cf[1] == 0.0f && cf[2] == 0.0f && cf[3] == 0.0f) continue;
            } else {
                cf[0] = coef[(int64_t)r * TP + tp];
                if (cf[0] == 0.0f) continue;
            }
            const float* src = yr[r] + bf * P + p;
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
                if (cf[v] == 0.0f) continue;                       // a skipped term: the value is never looked at
                const float tm = cf[v] * yv[v];                    // one multiply, then one add: no fma (-ffp-contract=off)
                acc[v] = first[v] ? tm : acc[v] + tm;
                first[v] = false;
            }
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
int cc_region_weights(const uint8_t* masks, float* coef, int32_t K, int32_t T, int32_t H, int32_t W, int32_t F, hipStream_t s) {
    const int h = H / 8, w = W / 8;
    const int ty = (h + kTile - 1) / kTile, tx = (w + kTile - 1) / kTile;
    const dim3 grid((unsigned)((int64_t)T * ty * tx));
    if (W % 16 == 0 && aligned(masks, 16))
        hipLaunchKernelGGL(region_weights_kernel<true>, grid, dim3(kThreads), 0, s, masks, coef, K, T, h, w, F, ty, tx);
    else
        hipLaunchKernelGGL(region_weights_kernel<false>, grid, dim3(kThreads), 0, s, masks, coef, K, T, h, w, F, ty, tx);
    return cc_launch_status("region_weights");
}

int cc_region_fuse(const float* const* yr, float* out, const float* coef, int32_t K, int64_t BC, int32_t T, int64_t P, hipStream_t s) {
    if (P % 4 == 0 && aligned(out, 16) && aligned(coef, 16))
        hipLaunchKernelGGL(region_fuse_kernel<4>, dim3(grid_for(BC * T * (P / 4))), dim3(kThreads), 0, s, yr, out, coef, K + 1, BC, T, P);
    else
        hipLaunchKernelGGL(region_fuse_kernel<1>, dim3(grid_for(BC * T * P)), dim3(kThreads), 0, s, yr, out, coef, K + 1, BC, T, P);
    return cc_launch_status("region_fuse");
}
