// Mask tracking (include/ccedit_hip.h, "Mask tracking"): a mask painted on one frame follows the source's motion through the clip
// (ccedit_amd/masktrack.py; `--mask_track`).  All integer work on bytes:
//   masktrack_select   all pairs of the call: per pixel the best of the 3 x 3 neighbouring blocks' vectors (from prop_match, level 0) by
//                      the key S * 16 + order, S the 5 x 5 edge-replicated box sum of |Y_f(p) - Y_g(clamp(p + c))|
//   masktrack_step     one frame of the chain: m_f(p) = m_g(q), q = clamp(p + v(p)), or 0 where |v(p) + r(q)|_1 > limit
// Both equal tests/_masktrack_numpy.py bit for bit; the file is compiled with -ffp-contract=off -fno-slp-vectorize like the other
// bit-exact files (there is no floating point in it).
//
// masktrack_select is the hot path.  The candidate set is constant over an 8 x 8 block, so a workgroup owns a tile of four blocks of
// one block row (32 x 8 pixels), ONE WAVE PER BLOCK with its own LDS slots.  A wave stages Y_f of its block plus the 2-pixel apron
// of the box (12 x 12 bytes, coordinates clamped = the box's edge replication) and, per candidate, the 12 x 12 window of Y_g shifted
// by that candidate, clamped while it is staged.  Rows are 16 bytes apart (12 used), so the lanes of a row read the same one or two
// dwords (a broadcast) and the eight rows a 32-lane group touches lie on different banks.  Then the box sum is separable: a lane per
// (row, x) forms the horizontal 5-sum of every candidate — the five bytes are one dword realigned by v_alignbyte_b32 plus one byte,
// two v_sad_u8 — into LDS, and a lane per pixel adds five rows and keeps the minimum key.  Every candidate is evaluated, identical
// ones too: equal vectors give equal sums and the lower order wins, so skipping them could only save time.  No atomics; the
// result does not depend on evaluation order.
//
// The pair list and the block vectors are device data the host cannot check per launch: frame indices are clamped into the
// pyramid, block indices into the table, vectors into +-kVecMax, window coordinates into the frame, so that nothing read from
// them can take an access outside a tensor.  masktrack_step clamps q into the frame.  The argument checks live with the exported
// entry points in core.cpp.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 256 * 8;
constexpr int kCand = 9;                     // 3 x 3 neighbouring blocks
constexpr int kWin = 12;                     // 8 + 2 * 2: a block plus the apron of the 5 x 5 box
constexpr int kRowDw = 4;                    // dwords per staged row: 12 bytes + 4 of padding
constexpr int kVecMax = 64;                  // (ccedit_amd/masktrack.py VEC_MAX; the matcher's own reach is 46)

constexpr uint32_t pack9(int a0, int a1, int a2, int a3, int a4, int a5, int a6, int a7, int a8) {
    return (uint32_t)(a0 + 1) | (uint32_t)(a1 + 1) << 2 | (uint32_t)(a2 + 1) << 4 | (uint32_t)(a3 + 1) << 6 | (uint32_t)(a4 + 1) << 8 |
           (uint32_t)(a5 + 1) << 10 | (uint32_t)(a6 + 1) << 12 | (uint32_t)(a7 + 1) << 14 | (uint32_t)(a8 + 1) << 16;
}
constexpr uint32_t kOrderY = pack9(0, -1, 0, 0, 1, -1, -1, 1, 1);          // dby of candidates 0 ... 8
constexpr uint32_t kOrderX = pack9(0, 0, -1, 1, 0, -1, 1, -1, 1);          // dbx

inline unsigned grid_for(int64_t items) {
    const int64_t g = (items + kThreads - 1) / kThreads;
    return (unsigned)(g < 1 ? 1 : (g > kMaxBlocks ? kMaxBlocks : g));
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// five consecutive bytes starting at byte x of a staged row -> (bytes x .. x + 3, byte x + 4)
__device__ __forceinline__ void five(const uint32_t* row, int x, uint32_t& four, uint32_t& one) {
    const uint32_t lo = row[x >> 2], hi = row[(x >> 2) + 1];
    const uint32_t sh = (uint32_t)(x & 3);
    four = __builtin_amdgcn_alignbyte(hi, lo, sh);
    one = (hi >> (8 * sh)) & 255u;
}

__global__ __launch_bounds__(kThreads) void masktrack_select_kernel(const uint8_t* __restrict__ lum, const int32_t* __restrict__ pairs,
                                                                    const int32_t* __restrict__ vec, uint32_t* __restrict__ out, int P, int F,
                                                                    int H, int W) {
    __shared__ uint32_t s_f[4][kWin * kRowDw];
    __shared__ uint32_t s_g[4][kCand][kWin * kRowDw];
    __shared__ uint16_t s_h[4][kCand][kWin][8];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nby = H / 8, nbx = W / 8;
    const int64_t NB = (int64_t)P * nby * nbx;
    const int64_t g = (int64_t)blockIdx.x * 4 + wave;
    const bool live = g < NB;                // (wave-uniform; a wave beyond the last block only takes part in the barriers)
    int by = 0, bx = 0, p = 0, vy = 0, vx = 0;
    if (live) {
        bx = (int)(g % nbx);
        const int64_t r = g / nbx;
        by = (int)(r % nby), p = (int)(r / nby);
        const int f = clampi(pairs[4 * p], 0, F - 1), k = clampi(pairs[4 * p + 1], 0, F - 1);
        const uint8_t* yf = lum + (int64_t)f * H * W;
        const uint8_t* yk = lum + (int64_t)k * H * W;
        // lane c < 9 holds candidate c: the vector of block (by + dby, bx + dbx), indices clamped, in the order
        // (0,0) (-1,0) (0,-1) (0,1) (1,0) (-1,-1) (-1,1) (1,-1) (1,1) (kOrderY / kOrderX: two bits each, value + 1)
        const int c = lane < kCand ? lane : 0;
        const int dby = (int)((kOrderY >> (2 * c)) & 3u) - 1;
        const int dbx = (int)((kOrderX >> (2 * c)) & 3u) - 1;
        const int32_t* pv = vec + (((int64_t)p * nby + clampi(by + dby, 0, nby - 1)) * nbx + clampi(bx + dbx, 0, nbx - 1)) * 2;
        vy = clampi(pv[0], -kVecMax, kVecMax);
        vx = clampi(pv[1], -kVecMax, kVecMax);
        const int oy = by * 8 - 2, ox = bx * 8 - 2;
        if (lane < kWin * 3) {
            const int rr = lane / 3, cc = lane - rr * 3;
            const uint8_t* row = yf + (int64_t)clampi(oy + rr, 0, H - 1) * W;
            uint32_t v = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) v |= (uint32_t)row[clampi(ox + 4 * cc + b, 0, W - 1)] << (8 * b);
            s_f[wave][rr * kRowDw + cc] = v;
        }
        for (int i0 = 0; i0 < kCand * kWin * 3; i0 += 64) {
            const int i = i0 + lane;
            const int cand = i / (kWin * 3) < kCand ? i / (kWin * 3) : kCand - 1;
            const int cy = __shfl(vy, cand, 64), cx = __shfl(vx, cand, 64);          // (every lane of the wave takes part)
            if (i < kCand * kWin * 3) {
                const int rem = i - cand * (kWin * 3);
                const int rr = rem / 3, cc = rem - rr * 3;
                // the box is edge-replicated: the pixel is clamped first, then the pixel plus the candidate
                const uint8_t* row = yk + (int64_t)clampi(clampi(oy + rr, 0, H - 1) + cy, 0, H - 1) * W;
                uint32_t v = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b) v |= (uint32_t)row[clampi(clampi(ox + 4 * cc + b, 0, W - 1) + cx, 0, W - 1)] << (8 * b);
                s_g[wave][cand][rr * kRowDw + cc] = v;
            }
        }
    }
    __syncthreads();
    if (live) {
        for (int it = lane; it < kWin * 8; it += 64) {
            const int rr = it >> 3, x = it & 7;
            uint32_t f4, f1;
            five(&s_f[wave][rr * kRowDw], x, f4, f1);
#pragma unroll
            for (int c = 0; c < kCand; ++c) {
                uint32_t g4, g1;
                five(&s_g[wave][c][rr * kRowDw], x, g4, g1);
                s_h[wave][c][rr][x] = (uint16_t)__builtin_amdgcn_sad_u8(f1, g1, __builtin_amdgcn_sad_u8(f4, g4, 0u));       // <= 1275
            }
        }
    }
    __syncthreads();
    if (live) {
        const int y = lane >> 3, x = lane & 7;
        uint32_t best = 0xffffffffu;
#pragma unroll
        for (int c = 0; c < kCand; ++c) {
            uint32_t s = 0;
#pragma unroll
            for (int i = 0; i < 5; ++i) s += s_h[wave][c][y + i][x];
            const uint32_t key = s * 16u + (uint32_t)c;                     // S <= 6375
            best = key < best ? key : best;
        }
        const int win = (int)(best & 15u);
        const int wy = __shfl(vy, win, 64), wx = __shfl(vx, win, 64);
        out[((int64_t)p * H + by * 8 + y) * W + bx * 8 + x] = ((uint32_t)wy & 0xffffu) | ((uint32_t)wx << 16);
    }
}

// ---- step: one thread per four consecutive pixels of a row.  v, r: packed int16 (dy, dx) per pixel of ONE pair each.
__global__ __launch_bounds__(kThreads) void masktrack_step_kernel(const uint32_t* __restrict__ v, const uint32_t* __restrict__ r,
                                                                  const uint8_t* __restrict__ mg, uint8_t* __restrict__ mf, int H, int W, int limit) {
    const int G = W / 4;
    const int total = H * G;
    for (int idx = blockIdx.x * kThreads + threadIdx.x; idx < total; idx += gridDim.x * kThreads) {
        const int y = idx / G, x0 = (idx - y * G) * 4;
        const u32x4 v4 = *(const u32x4*)(v + (int64_t)y * W + x0);
        uint32_t o = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int vy = (int)(int16_t)(v4[j] & 0xffffu), vx = (int)(int16_t)(v4[j] >> 16);
            const int64_t q = (int64_t)clampi(y + vy, 0, H - 1) * W + clampi(x0 + j + vx, 0, W - 1);
            const uint32_t rq = r[q];
            int ey = vy + (int)(int16_t)(rq & 0xffffu), ex = vx + (int)(int16_t)(rq >> 16);
            ey = ey < 0 ? -ey : ey, ex = ex < 0 ? -ex : ex;
            const uint32_t m = ey + ex > limit ? 0u : (uint32_t)mg[q];
            o |= m << (8 * j);
        }
        *(uint32_t*)(mf + (int64_t)y * W + x0) = o;
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------
// launchers (arguments validated by the entry points in core.cpp)
// ------------------------------------------------------------------------------------------
int cc_masktrack_select(const uint8_t* lum, const int32_t* pairs, const int32_t* vec, uint32_t* out, int32_t P, int32_t F, int32_t H, int32_t W,
                        hipStream_t s) {
    const int64_t NB = (int64_t)P * (H / 8) * (W / 8);
    hipLaunchKernelGGL(masktrack_select_kernel, dim3((unsigned)((NB + 3) / 4)), dim3(kThreads), 0, s, lum, pairs, vec, out, P, F, H, W);
    return cc_launch_status("masktrack_select");
}

int cc_masktrack_step(const uint32_t* v, const uint32_t* r, const uint8_t* mg, uint8_t* mf, int32_t H, int32_t W, int32_t limit, hipStream_t s) {
    hipLaunchKernelGGL(masktrack_step_kernel, dim3(grid_for((int64_t)H * (W / 4))), dim3(kThreads), 0, s, v, r, mg, mf, H, W, limit);
    return cc_launch_status("masktrack_step");
}
