// GIF sources decoded on the device (include/ccedit_hip.h, "GIF decoding"; ccedit_amd/gifdec.py): the LZW streams
// and palettes of N images of one file -> uint8 RGB frames, composited on a canvas that is carried from launch to launch.  Three stages:
//   gifdec_codes     ONE WAVE PER IMAGE.  gifdec_core.h's build_codes() — the same text the host-side hardening program compiles — turns
//                    the bit stream into a TABLE of codes (parent, length, first and last byte, pixel offset) without touching a pixel,
//                    64 codes at a time: the bit positions of a batch are closed-form from the segment's start, a ballot cuts the batch
//                    at its first Clear / EOI, references to codes inside the batch are resolved to a fixed point through cross-lane
//                    moves, the offsets are a wave prefix sum.
//   gifdec_pixels    ONE LANE PER CODE: from the code's last byte up its chain of parents, one hop per pixel.  No lane reads what
//                    another lane wrote; nothing is a serial copy through memory.
//   gifdec_compose   ONE THREAD PER CANVAS PIXEL, looping over the launch's images in order with the pixel's RGB in registers: outside
//                    the image's rectangle nothing, else the index (through the four-pass row order for an interlaced image) and,
//                    unless it is the transparent index, the palette entry; selected images are written to their output, the canvas at
//                    the end.
// The table of a batch is read back, by later batches, from global memory that OTHER lanes of the same wave wrote: between such a write
// and the read stands a fence of wavefront scope.  Everything is written with ordinary vector stores; all arithmetic is integer.
//
// Bounds.  The host checks geometry and buffer sizes (core.cpp).  The descriptors are device data: every kernel checks a descriptor
// against the buffers it points into before it uses it (gifdec_core.h desc_ok) and gives status 6 where it does not fit.
#include "common.h"
#include "gifdec_core.h"

namespace {

using namespace gifdec;

struct WaveExec {
    int lane;
    template <class T>
    struct Var {
        T v;
        __device__ __forceinline__ T& operator[](int) { return v; }
    };
    __device__ __forceinline__ int lanes() const { return 64; }
    __device__ __forceinline__ int hi() const { return lane; }
    __device__ __forceinline__ int lo() const { return lane; }
    __device__ __forceinline__ uint64_t ballot(Var<int32_t>& p) const { return __ballot(p.v != 0); }
    __device__ __forceinline__ void gather(Var<int32_t>& dst, Var<int32_t>& src, Var<int32_t>& idx) const { dst.v = __shfl(src.v, idx.v & 63, 64); }
    __device__ __forceinline__ void scan(Var<int32_t>& dst, Var<int32_t>& src) const {
        int32_t x = src.v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int32_t y = __shfl_up(x, o, 64);
            if (lane >= o) x += y;
        }
        dst.v = x - src.v;
    }
    __device__ __forceinline__ int32_t get(Var<int32_t>& p, int l) const { return __shfl(p.v, l & 63, 64); }
    __device__ __forceinline__ int64_t get(Var<int64_t>& p, int l) const {
        const uint32_t low = (uint32_t)__shfl((int32_t)(uint32_t)p.v, l & 63, 64);
        const uint32_t high = (uint32_t)__shfl((int32_t)(uint32_t)((uint64_t)p.v >> 32), l & 63, 64);
        return (int64_t)((uint64_t)high << 32 | low);
    }
    __device__ __forceinline__ void sync() const {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
};

__global__ __launch_bounds__(64) void gifdec_codes_kernel(const uint8_t* __restrict__ data, int64_t data_bytes, const int64_t* __restrict__ desc,
                                                          int32_t* parent, int32_t* len, int32_t* off, uint8_t* first, uint8_t* last,
                                                          int64_t total_codes, int32_t* __restrict__ ncodes, int32_t* __restrict__ status) {
    const int64_t n = blockIdx.x;
    const int64_t* d = desc + n * kDescWords;
    int32_t st = kBadDescriptor;
    int64_t count = 0, where = 0;
    // (the canvas and the planes are not this stage's: a rectangle of 1 x 1 at 0, 0 on a canvas of 65535 x 65535 stands in for them)
    const bool ok = d[dW] >= 1 && d[dH] >= 1 && d[dW] <= 65535 && d[dH] <= 65535 && d[dPalSize] >= 1 && d[dPalSize] <= 256 && d[dPalOff] >= 0 &&
                    d[dPalOff] <= data_bytes - 3 * d[dPalSize] && d[dStreamLen] >= 0 && d[dStreamOff] >= 0 &&
                    d[dStreamOff] <= data_bytes - d[dStreamLen] && d[dCodeCap] >= 1 && d[dCodeOff] >= 0 && d[dCodeOff] <= total_codes - d[dCodeCap];
    if (ok) {
        WaveExec ex{(int)threadIdx.x};
        const int64_t co = d[dCodeOff];
        const Codes t{parent + co, len + co, off + co, first + co, last + co};
        st = build_codes(ex, data + d[dStreamOff], d[dStreamLen], (int)d[dMinCode], d[dW] * d[dH], d[dCodeCap], t, &count, &where);
    }
    if (threadIdx.x == 0) {
        ncodes[n] = (int32_t)count;
        status[2 * n] = st;
        status[2 * n + 1] = (int32_t)(where > 0x7fffffff ? 0x7fffffff : where);
    }
}

__global__ __launch_bounds__(256) void gifdec_pixels_kernel(const int64_t* __restrict__ desc, const int32_t* __restrict__ parent,
                                                            const int32_t* __restrict__ len, const int32_t* __restrict__ off,
                                                            const uint8_t* __restrict__ last, int64_t total_codes,
                                                            const int32_t* __restrict__ ncodes, uint8_t* planes, int64_t plane_bytes) {
    const int64_t n = blockIdx.y;
    const int64_t* d = desc + n * kDescWords;
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t w = d[dW], h = d[dH], co = d[dCodeOff], cap = d[dCodeCap], po = d[dPlaneOff];
    if (w < 1 || h < 1 || w > 65535 || h > 65535 || cap < 1 || co < 0 || co > total_codes - cap || po < 0 || po > plane_bytes - w * h) return;
    int64_t count = ncodes[n];
    count = count < 0 ? 0 : (count > cap ? cap : count);
    if (k >= count) return;
    write_code(parent + co, len + co, off + co, last + co, count, k, planes + po, w * h);
}

__global__ __launch_bounds__(256) void gifdec_compose_kernel(const uint8_t* __restrict__ data, int64_t data_bytes, const int64_t* __restrict__ desc,
                                                             int32_t N, const uint8_t* __restrict__ planes, int64_t plane_bytes, uint8_t* canvas,
                                                             uint8_t* out, int32_t n_out, int32_t H, int32_t W, int32_t* status) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t npix = (int64_t)H * W;
    const bool mine = p < npix;
    const int y = mine ? (int)(p / W) : 0, x = mine ? (int)(p % W) : 0;
    uint32_t r = 0, g = 0, b = 0;
    if (mine) r = canvas[3 * p], g = canvas[3 * p + 1], b = canvas[3 * p + 2];
    for (int32_t n = 0; n < N; ++n) {
        const int64_t* d = desc + (int64_t)n * kDescWords;
        if (!desc_ok(d, data_bytes, (int64_t)1 << 62, plane_bytes, H, W, n_out) || d[dCodeCap] < 1) {          // (uniform: every thread reads the same words)
            if (p == 0) status[2 * n] = kBadDescriptor, status[2 * n + 1] = 0;
            continue;
        }
        const int fx = (int)d[dX], fy = (int)d[dY], fw = (int)d[dW], fh = (int)d[dH];
        if (mine && x >= fx && x < fx + fw && y >= fy && y < fy + fh) {
            const int row = d[dInterlace] ? interlaced_row(y - fy, fh) : y - fy;
            const int64_t at = (int64_t)row * fw + (x - fx);
            const int idx = planes[d[dPlaneOff] + at];
            if (idx >= (int)d[dPalSize]) {
                status[2 * n] = kBadIndex;                                          // (every thread that stores here stores the same value)
                atomicMin(&status[2 * n + 1], (int32_t)(at > 0x7ffffffe ? 0x7ffffffe : at));
            } else if (idx != (int)d[dTransparent]) {
                const uint8_t* pal = data + d[dPalOff] + 3 * idx;
                r = pal[0], g = pal[1], b = pal[2];
            }
        }
        if (mine && d[dSlot] >= 0) {
            uint8_t* o = out + (d[dSlot] * npix + p) * 3;
            o[0] = (uint8_t)r, o[1] = (uint8_t)g, o[2] = (uint8_t)b;
        }
    }
    if (mine) canvas[3 * p] = (uint8_t)r, canvas[3 * p + 1] = (uint8_t)g, canvas[3 * p + 2] = (uint8_t)b;
}

}  // namespace

// ------------------------------------------------------------------------------------------
// launchers (arguments validated by the entry points in core.cpp)
// ------------------------------------------------------------------------------------------
int cc_gifdec_codes(const uint8_t* data, int64_t data_bytes, const int64_t* desc, int32_t* parent, int32_t* len, int32_t* off, uint8_t* first,
                    uint8_t* last, int64_t total_codes, int32_t* ncodes, int32_t* status, int32_t N, hipStream_t s) {
    hipLaunchKernelGGL(gifdec_codes_kernel, dim3((unsigned)N), dim3(64), 0, s, data, data_bytes, desc, parent, len, off, first, last, total_codes,
                       ncodes, status);
    return cc_launch_status("gifdec_codes");
}

int cc_gifdec_pixels(const int64_t* desc, const int32_t* parent, const int32_t* len, const int32_t* off, const uint8_t* last, int64_t total_codes,
                     const int32_t* ncodes, uint8_t* planes, int64_t plane_bytes, int32_t N, int64_t max_codes, hipStream_t s) {
    hipLaunchKernelGGL(gifdec_pixels_kernel, dim3((unsigned)((max_codes + 255) / 256), (unsigned)N), dim3(256), 0, s, desc, parent, len, off, last,
                       total_codes, ncodes, planes, plane_bytes);
    return cc_launch_status("gifdec_pixels");
}

int cc_gifdec_compose(const uint8_t* data, int64_t data_bytes, const int64_t* desc, const uint8_t* planes, int64_t plane_bytes, uint8_t* canvas,
                      uint8_t* out, int32_t* status, int32_t N, int32_t n_out, int32_t H, int32_t W, hipStream_t s) {
    const int64_t npix = (int64_t)H * W;
    hipLaunchKernelGGL(gifdec_compose_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, s, data, data_bytes, desc, N, planes, plane_bytes,
                       canvas, out, n_out, H, W, status);
    return cc_launch_status("gifdec_compose");
}
