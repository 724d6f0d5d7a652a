// PNG sources decoded on the device (include/ccedit_hip.h, "PNG decoding"; ccedit_amd/pngdec.py): the zlib
// streams of N 8-bit RGB images of one size -> uint8 RGB frames.  Two stages, the stages of png.hip in reverse:
//   pngdec_inflate    ONE WAVE PER STREAM.  All 64 lanes run pngdec_core.h's inflate() — the same text the host-side hardening program
//                     compiles — on the same bits and so hold the same state; the symbol walk is serial and costs what one lane costs.
//                     The code tables live in LDS and are written by lane 0.  A literal is stored by lane 0; a match is copied by the
//                     whole wave (lane j reads out[pos - d + (j mod d)]: every source lies before the match, so an overlapping copy
//                     needs no order among the lanes); a stored block is copied by the whole wave; the input is staged in LDS 1 KiB at
//                     a time by the whole wave, so the bit reader's refills do not wait for the output's stores in flight; Adler-32 is summed by position
//                     weights, 64 bytes per step, and compared with the trailer.  One status pair per stream.
//   pngdec_unfilter   ONE WAVE PER IMAGE, 64 consecutive rows at a time as a skewed wavefront: lane r undoes row r0 + r and trails
//                     row r0 + r - 1 by one pixel, so at step t it works on pixel t - r.  The pixel above comes from lane r - 1's
//                     previous step through one cross-lane move (the pixel above-left is the one before it, the pixel to the left the
//                     lane's own), only lane 0 reads the row above from memory: the last row of the band before.
// The window of a match and the row above a band are read back from global memory that OTHER lanes of the same wave wrote: between
// such a write and the read stands a fence of wavefront scope, which orders them for the compiler; the hardware performs one wave's
// vector memory operations in order.  Everything is written with ordinary vector stores.  All arithmetic is integer; the file is
// compiled with -ffp-contract=off -fno-slp-vectorize like the other bit-exact files.
//
// Bounds.  The host checks geometry and buffer sizes (core.cpp).  Stream offsets and lengths are device data: they are clamped into
// [0, data_bytes] here.  inflate() checks every input, output and table index before it is used (pngdec_core.h); a thread of the
// unfilter kernel touches only its own row's bytes and, in lane 0, the row above it.
#include "common.h"
#include "pngdec_core.h"

namespace {

using namespace pngdec;

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

constexpr int kStage = 1024;       // input bytes staged in LDS at a time: the bit reader never waits for the stores in flight

struct WaveExec {
    int lane;
    uint8_t* stage;                // kStage bytes of LDS
    int64_t base;                  // stage[j] = data[base + j]; -kStage before the first refill
    __device__ __forceinline__ uint8_t byte(const uint8_t* data, int64_t pos, int64_t end) {
        if (pos < base || pos >= base + kStage) {              // (uniform: every lane reads the same position)
            base = pos;
            wave_sync();
            for (int j = lane; j < kStage; j += 64) stage[j] = base + j < end ? data[base + j] : (uint8_t)0;
            wave_sync();
        }
        return stage[(int)(pos - base) & (kStage - 1)];
    }
    __device__ __forceinline__ bool lead() const { return lane == 0; }
    __device__ __forceinline__ int32_t share(int32_t v) const { return __shfl(v, 0, 64); }
    __device__ __forceinline__ void sync() const { wave_sync(); }
    __device__ __forceinline__ void put(uint8_t* out, int64_t pos, uint8_t b) const {
        if (lane == 0) out[pos] = b;
    }
    __device__ __forceinline__ void copy(uint8_t* out, int64_t pos, int d, int len) const {
        wave_sync();
        copy_match(out, pos, d, len, lane, 64);
        wave_sync();
    }
    __device__ __forceinline__ void copy_in(uint8_t* out, int64_t pos, const uint8_t* src, int n) const {
        for (int j = lane; j < n; j += 64) out[pos + j] = src[j];
    }
    __device__ __forceinline__ uint32_t adler(const uint8_t* p, int64_t n) const {
        uint32_t s1, s2;
        adler_partial(p, n, lane, 64, &s1, &s2);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            s1 += __shfl_xor(s1, o, 64);                   // 64 partials below 65521: no overflow
            s2 += __shfl_xor(s2, o, 64);
        }
        return adler_finish(s1, s2, n);
    }
};

__global__ __launch_bounds__(64) void pngdec_inflate_kernel(const uint8_t* data, int64_t data_bytes, const int64_t* __restrict__ streams,
                                                            uint8_t* filtered, int32_t* __restrict__ status, int64_t L) {
    __shared__ Work wk;
    __shared__ uint8_t stage[kStage];
    const int64_t s = blockIdx.x;
    int64_t lo = streams[2 * s], n = streams[2 * s + 1];
    lo = lo < 0 ? 0 : (lo > data_bytes ? data_bytes : lo);
    n = n < 0 ? 0 : (n > data_bytes - lo ? data_bytes - lo : n);
    WaveExec ex{(int)threadIdx.x, stage, -(int64_t)kStage};
    int64_t where = 0;
    const int32_t st = inflate(ex, data + lo, n, filtered + s * L, L, wk, &where);
    if (threadIdx.x == 0) {
        status[2 * s] = st;
        status[2 * s + 1] = (int32_t)(where > 0x7fffffff ? 0x7fffffff : where);
    }
}

__device__ __forceinline__ uint32_t load3(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16; }

__global__ __launch_bounds__(64) void pngdec_unfilter_kernel(const uint8_t* __restrict__ filtered, uint8_t* rgb, int32_t* __restrict__ status,
                                                             int H, int W) {
    const int lane = threadIdx.x;
    const int64_t img = blockIdx.x;
    const int64_t rb = 1 + 3 * (int64_t)W, ob = 3 * (int64_t)W;
    const uint8_t* in_img = filtered + img * rb * H;
    uint8_t* out_img = rgb + img * ob * H;
    int32_t st = kOk, at = 0;
    for (int r0 = 0; r0 < H; r0 += 64) {
        const int row = r0 + lane;
        const bool active = row < H;
        const uint8_t* in = in_img + (active ? row : 0) * rb;
        uint8_t* out = out_img + (active ? row : 0) * ob;
        const int ft = active ? in[0] : 0;
        const uint64_t bad = __ballot(ft > 4);
        if (bad) {                                              // (uniform: every lane sees the same ballot)
            const int first = __ffsll((unsigned long long)bad) - 1;
            st = kBadFilter;
            const int64_t pos = (int64_t)(r0 + first) * rb;
            at = (int32_t)(pos > 0x7fffffff ? 0x7fffffff : pos);
            break;
        }
        const uint8_t* up = (lane == 0 && r0 > 0) ? out - ob : nullptr;    // lane 0: the last row of the band before, from memory
        uint32_t cur = 0, left = 0, upleft = 0;                              // packed pixels: R | G << 8 | B << 16
        for (int t = 0; t < W + 63; ++t) {
            const uint32_t from_above = __shfl_up(cur, 1, 64);              // lane - 1's pixel of its previous step: this lane's pixel above
            const int x = t - lane;
            if (active && x >= 0 && x < W) {
                const uint32_t above = lane == 0 ? (up ? load3(up + 3 * (int64_t)x) : 0u) : from_above;
                const uint32_t raw = load3(in + 1 + 3 * (int64_t)x);
                uint32_t px = 0;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const int sh = 8 * k;
                    px |= (uint32_t)unfilter_byte(ft, (int)((raw >> sh) & 255u), (int)((left >> sh) & 255u), (int)((above >> sh) & 255u),
                                                  (int)((upleft >> sh) & 255u))
                          << sh;
                }
                uint8_t* o = out + 3 * (int64_t)x;
                o[0] = (uint8_t)px, o[1] = (uint8_t)(px >> 8), o[2] = (uint8_t)(px >> 16);
                left = px, upleft = above, cur = px;
            }
        }
        wave_sync();
    }
    if (lane == 0) {
        status[2 * img] = st;
        status[2 * img + 1] = at;
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------
// launchers (arguments validated by the entry points in core.cpp)
// ------------------------------------------------------------------------------------------
int cc_pngdec_inflate(const uint8_t* data, int64_t data_bytes, const int64_t* streams, uint8_t* filtered, int32_t* status, int32_t N, int32_t H,
                      int32_t W, hipStream_t s) {
    const int64_t L = (int64_t)H * (1 + 3 * (int64_t)W);
    hipLaunchKernelGGL(pngdec_inflate_kernel, dim3((unsigned)N), dim3(64), 0, s, data, data_bytes, streams, filtered, status, L);
    return cc_launch_status("pngdec_inflate");
}

int cc_pngdec_unfilter(const uint8_t* filtered, uint8_t* rgb, int32_t* status, int32_t N, int32_t H, int32_t W, hipStream_t s) {
    hipLaunchKernelGGL(pngdec_unfilter_kernel, dim3((unsigned)N), dim3(64), 0, s, filtered, rgb, status, H, W);
    return cc_launch_status("pngdec_unfilter");
}
