// Motion-following noise (include/ccedit_hip.h, "Motion-following noise"): once per clip, which noise sample every latent cell (8 x 8
// pixels) of every keyframe inherits from an earlier keyframe along the source's motion (ccedit_amd/noisewarp.py; `--noise_warp`), and
// on every draw of the run the gather that applies it.  All integer work and bit copies:
//   noisewarp_track    one thread per (k >= 1, cell): the cell's centre followed frame by frame from keyframe k back to keyframe k - 1
//                      along the block vectors of prop_match, dropped where it leaves the frame or the way back disagrees
//   noisewarp_claim    keyframe k: every cell that arrives at a sample of an earlier keyframe bids for it, atomicMax of
//                      k * cells + (cells - 1 - idx) + 1 — the smallest cell index is the largest bid
//   noisewarp_resolve  keyframe k: a cell whose bid the table holds inherits (R', P), every other cell is fresh: (k, own centre); writes
//                      the origins, the index map and the count of inherited cells
//   noisewarp_check    any index of a map outside [0, N)?  (the host reads one word back, once per map)
//   noise_warp         out[b][c][n] = raw[b][c][src[b][n]], a 4-byte bit copy
// All equal tests/_noisewarp_numpy.py bit for bit; the file is compiled with -ffp-contract=off -fno-slp-vectorize like the other
// bit-exact files (there is no floating-point arithmetic in it: the noise moves as uint32).
//
// Claim and resolve are two launches per keyframe: the kernel boundary is the ordering, there is no flag protocol between
// workgroups.  The table is zeroed once per clip; bids of keyframe k exceed every bid of an earlier keyframe, so an entry never has
// to be cleared.  atomicMax of distinct values does not depend on arrival order, neither does the integer count.
//
// The pair order of the block vectors is that of ccedit_amd/masktrack.py pair_rows with the anchor at frame 0: for frame f >= 1 row
// 2 (f - 1) is f -> f - 1 and row 2 (f - 1) + 1 is f - 1 -> f.  The keyframe numbers, the block vectors, the tracked positions, the
// origins and the index map are device data the host cannot check per launch: frame numbers are clamped into the clip, vectors into
// +-kVecMax, positions into the frame, keyframe ordinals into 0 ... k - 1 and map indices into the raw noise, so that nothing read from
// them can take an access outside a tensor.  The argument checks live with the exported entry points in core.cpp.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 256 * 8;          // 256 CUs x 8 workgroups of 4 waves
constexpr int kVecMax = 64;                  // (ccedit_amd/noisewarp.py VEC_MAX; the matcher's own reach is 46)

inline unsigned grid_for(int64_t items) {
    const int64_t g = (items + kThreads - 1) / kThreads;
    return (unsigned)(g < 1 ? 1 : (g > kMaxBlocks ? kMaxBlocks : g));
}
inline bool aligned(const void* p, unsigned a) { return ((uintptr_t)p & (a - 1)) == 0; }

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int absi(int v) { return v < 0 ? -v : v; }

// ---- track: trk[k][cell] = (valid, Q_y, Q_x) for k = 1 ... K - 1 (row 0 is the host's: zero).  The loop of a thread runs over at most
// F - 1 frames whatever `key` holds.
__global__ __launch_bounds__(kThreads) void noisewarp_track_kernel(const int32_t* __restrict__ vec, const int32_t* __restrict__ key,
                                                                   int32_t* __restrict__ trk, int K, int F, int H, int W, int limit) {
    const int h = H / 8, w = W / 8;
    const int64_t cells = (int64_t)h * w;
    const int64_t total = (int64_t)(K - 1) * cells;
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * kThreads) {
        const int k = (int)(idx / cells) + 1;
        const int64_t cell = idx - (int64_t)(k - 1) * cells;
        const int ci = (int)(cell / w), cj = (int)(cell - (int64_t)ci * w);
        int py = 8 * ci + 4, px = 8 * cj + 4;
        bool valid = true;
        const int hi = clampi(key[k], 0, F - 1), lo = clampi(key[k - 1], 0, F - 1);
        for (int f = hi; f > lo; --f) {                       // f >= 1: rows 2 (f - 1) and 2 (f - 1) + 1 exist
            const int32_t* v = vec + (((int64_t)2 * (f - 1) * h + (py >> 3)) * w + (px >> 3)) * 2;
            const int vy = clampi(v[0], -kVecMax, kVecMax), vx = clampi(v[1], -kVecMax, kVecMax);
            int qy = py + vy, qx = px + vx;
            const bool inside = qy >= 0 && qy < H && qx >= 0 && qx < W;
            qy = clampi(qy, 0, H - 1), qx = clampi(qx, 0, W - 1);
            const int32_t* r = vec + ((((int64_t)2 * (f - 1) + 1) * h + (qy >> 3)) * w + (qx >> 3)) * 2;
            const int ry = clampi(r[0], -kVecMax, kVecMax), rx = clampi(r[1], -kVecMax, kVecMax);
            valid = valid && inside && absi(vy + ry) + absi(vx + rx) <= limit;
            py = qy, px = qx;
        }
        int32_t* o = trk + ((int64_t)k * cells + cell) * 3;
        o[0] = valid ? 1 : 0, o[1] = py, o[2] = px;
    }
}

// what a cell of keyframe k >= 1 arrives at: the sample (R', P) and its key, or nothing
struct Arrival {
    bool cand;
    int r, py, px;
    uint32_t key;
};

__device__ __forceinline__ Arrival arrive(const int32_t* __restrict__ trk, const int32_t* __restrict__ org, int k, int64_t cell, int64_t cells,
                                          int H, int W) {
    const int w = W / 8;
    const int32_t* t = trk + ((int64_t)k * cells + cell) * 3;
    const int qy = clampi(t[1], 0, H - 1), qx = clampi(t[2], 0, W - 1);
    const int32_t* p = org + ((int64_t)(k - 1) * cells + (int64_t)(qy >> 3) * w + (qx >> 3)) * 3;
    Arrival a;
    a.r = clampi(p[0], 0, k - 1);
    a.py = clampi(p[1], 0, H - 1) + (qy & 7) - 4;             // P' + (Q - centre of Q's cell)
    a.px = clampi(p[2], 0, W - 1) + (qx & 7) - 4;
    a.cand = t[0] != 0 && a.py >= 0 && a.py < H && a.px >= 0 && a.px < W;
    a.key = (uint32_t)((int64_t)a.r * cells + (int64_t)(clampi(a.py, 0, H - 1) >> 3) * w + (clampi(a.px, 0, W - 1) >> 3));      // < k cells
    return a;
}

__global__ __launch_bounds__(kThreads) void noisewarp_claim_kernel(const int32_t* __restrict__ trk, const int32_t* __restrict__ org,
                                                                   uint32_t* __restrict__ table, int k, int H, int W) {
    const int64_t cells = (int64_t)(H / 8) * (W / 8);
    for (int64_t cell = (int64_t)blockIdx.x * kThreads + threadIdx.x; cell < cells; cell += (int64_t)gridDim.x * kThreads) {
        const Arrival a = arrive(trk, org, k, cell, cells, H, W);
        if (a.cand) atomicMax(table + a.key, (uint32_t)((int64_t)k * cells + (cells - 1 - cell) + 1));
    }
}

// k = 0: every cell is its own origin (0, centre), nothing is read.
__global__ __launch_bounds__(kThreads) void noisewarp_resolve_kernel(const int32_t* __restrict__ trk, int32_t* __restrict__ org,
                                                                     const uint32_t* __restrict__ table, int32_t* __restrict__ src,
                                                                     uint32_t* __restrict__ inherited, int k, int H, int W) {
    const int w = W / 8;
    const int64_t cells = (int64_t)(H / 8) * w;
    uint32_t mine = 0;
    for (int64_t cell = (int64_t)blockIdx.x * kThreads + threadIdx.x; cell < cells; cell += (int64_t)gridDim.x * kThreads) {
        const int ci = (int)(cell / w), cj = (int)(cell - (int64_t)ci * w);
        int r = k, py = 8 * ci + 4, px = 8 * cj + 4;
        if (k > 0) {
            const Arrival a = arrive(trk, org, k, cell, cells, H, W);
            if (a.cand && table[a.key] == (uint32_t)((int64_t)k * cells + (cells - 1 - cell) + 1)) {
                r = a.r, py = a.py, px = a.px;
                ++mine;
            }
        }
        int32_t* o = org + ((int64_t)k * cells + cell) * 3;
        o[0] = r, o[1] = py, o[2] = px;
        src[(int64_t)k * cells + cell] = (int32_t)((int64_t)r * cells + (int64_t)(py >> 3) * w + (px >> 3));
    }
    if (k > 0) {                                              // (k is uniform: every lane takes part in the shuffles)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
        if ((threadIdx.x & 63) == 0 && mine) atomicAdd(inherited + k, mine);
    }
}

// ---- check: *flag |= 1 where an index lies outside [0, N)
__global__ __launch_bounds__(kThreads) void noisewarp_check_kernel(const int32_t* __restrict__ src, int64_t total, uint32_t N, uint32_t* flag) {
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads)
        bad = bad || (uint32_t)src[i] >= N;
    if (bad) atomicOr(flag, 1u);
}

// ---- gather: out[b][c][n] = raw[b][c][src[b][n]] over uint32 [B][C][N].  V = 4: four indices as one 16-byte load, four 4-byte
// gathers, one 16-byte store (N % 4 == 0, src and out 16-byte aligned); V = 1: 4-byte accesses.  An index is held inside [0, N).
template <int V>
__global__ __launch_bounds__(kThreads) void noise_warp_kernel(const uint32_t* __restrict__ raw, const int32_t* __restrict__ src,
                                                              uint32_t* __restrict__ out, int64_t BC, int C, uint32_t N) {
    const int64_t NV = N / V;
    const int64_t total = BC * NV;
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * kThreads) {
        const int64_t bc = idx / NV;
        const int64_t n = (idx - bc * NV) * V;
        const uint32_t* plane = raw + bc * N;
        const int32_t* sp = src + (bc / C) * N + n;
        if constexpr (V == 4) {
            const u32x4 s = *(const u32x4*)sp;
            u32x4 y;
#pragma unroll
            for (int j = 0; j < 4; ++j) y[j] = plane[s[j] < N ? s[j] : N - 1];
            *(u32x4*)(out + bc * N + n) = y;
        } else {
            const uint32_t s = (uint32_t)sp[0];
            out[bc * N + n] = plane[s < N ? s : N - 1];
        }
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------
// launchers (arguments validated by the entry points in core.cpp)
// ------------------------------------------------------------------------------------------
int cc_noisewarp_track(const int32_t* vec, const int32_t* key, int32_t* trk, int32_t K, int32_t F, int32_t H, int32_t W, int32_t limit,
                       hipStream_t s) {
    const int64_t total = (int64_t)(K - 1) * (H / 8) * (W / 8);
    hipLaunchKernelGGL(noisewarp_track_kernel, dim3(grid_for(total)), dim3(kThreads), 0, s, vec, key, trk, K, F, H, W, limit);
    return cc_launch_status("noisewarp_track");
}

int cc_noisewarp_claim(const int32_t* trk, const int32_t* org, uint32_t* table, int32_t k, int32_t H, int32_t W, hipStream_t s) {
    hipLaunchKernelGGL(noisewarp_claim_kernel, dim3(grid_for((int64_t)(H / 8) * (W / 8))), dim3(kThreads), 0, s, trk, org, table, k, H, W);
    return cc_launch_status("noisewarp_claim");
}

int cc_noisewarp_resolve(const int32_t* trk, int32_t* org, const uint32_t* table, int32_t* src, uint32_t* inherited, int32_t k, int32_t H,
                         int32_t W, hipStream_t s) {
    hipLaunchKernelGGL(noisewarp_resolve_kernel, dim3(grid_for((int64_t)(H / 8) * (W / 8))), dim3(kThreads), 0, s, trk, org, table, src,
                       inherited, k, H, W);
    return cc_launch_status("noisewarp_resolve");
}

// -> CCEDIT_OK, CCEDIT_EINVAL where an index is out of range, or a HIP error.  Waits for the stream: the one word comes back to the host.
int cc_noisewarp_check(const int32_t* src, int64_t total, int64_t N, uint32_t* flag, hipStream_t s) {
    hipError_t e = hipMemsetAsync(flag, 0, sizeof(uint32_t), s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(noisewarp_check_kernel, dim3(grid_for(total)), dim3(kThreads), 0, s, src, total, (uint32_t)N, flag);
        e = hipGetLastError();
    }
    uint32_t host = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&host, flag, sizeof(uint32_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        cc_set_error("noisewarp_check: %s", hipGetErrorString(e));
        return (int)e;
    }
    if (host) {
        cc_set_error("ccedit_noisewarp_check: the map holds an index outside 0 ... %lld", (long long)N - 1);
        return CCEDIT_EINVAL;
    }
    return CCEDIT_OK;
}

int cc_noise_warp(const float* raw, const int32_t* src, float* out, int32_t B, int32_t C, int64_t N, hipStream_t s) {
    const int64_t BC = (int64_t)B * C;
    if (N % 4 == 0 && aligned(src, 16) && aligned(out, 16))           // every plane of out and every map of src starts 16-byte aligned
        hipLaunchKernelGGL(noise_warp_kernel<4>, dim3(grid_for(BC * (N / 4))), dim3(kThreads), 0, s, (const uint32_t*)raw, src, (uint32_t*)out, BC,
                           C, (uint32_t)N);
    else                                                              // (core.cpp: every buffer 4-byte aligned)
        hipLaunchKernelGGL(noise_warp_kernel<1>, dim3(grid_for(BC * N)), dim3(kThreads), 0, s, (const uint32_t*)raw, src, (uint32_t*)out, BC, C,
                           (uint32_t)N);
    return cc_launch_status("noise_warp");
}
