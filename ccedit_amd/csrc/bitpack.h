// Chunks of bits, each coded on its own into a slot of kSlotWords 32-bit words (LSB first), packed into one stream per frame: the scan
// that says where every chunk's bits go and the shifted copy.  Shared by gif.hip (LZW chunks) and png.hip (deflate blocks): the callers
// are kernels of their own that fix the slot size.  Chunk bit lengths and offsets are device data when these read them: lengths are
// clamped into the slot, and a chunk whose bits would leave the output is skipped.
#pragma once
#include "common.h"

__device__ __forceinline__ int cc_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// A workgroup of kThreads per frame (blockIdx.x), C chunks per frame: the byte counts of the frames before it, the exclusive scan of its
// chunks' bit lengths -> every chunk's bit offset in the packed output, the frame's byte count (its bits zero-padded to a byte).
template <int kThreads, int kSlotBits>
__device__ __forceinline__ void cc_pack_scan(const int32_t* __restrict__ chunk_bits, int64_t* __restrict__ chunk_off, int32_t* __restrict__ frame_bytes,
                                             int C) {
    __shared__ int64_t s_part[kThreads];
    const int tid = threadIdx.x;
    const int64_t f = blockIdx.x;
    int64_t sum = 0;
    for (int64_t g = tid; g < f; g += kThreads) {                                // the bytes of the frames before this one
        int64_t bits = 0;
        for (int c = 0; c < C; ++c) bits += cc_clampi(chunk_bits[g * C + c], 0, kSlotBits);
        sum += (bits + 7) >> 3;
    }
    s_part[tid] = sum;
    __syncthreads();
    for (int o = kThreads / 2; o > 0; o >>= 1) {
        if (tid < o) s_part[tid] += s_part[tid + o];
        __syncthreads();
    }
    const int64_t start = s_part[0] * 8;
    __syncthreads();
    const int per = (C + kThreads - 1) / kThreads;                               // chunks per thread, consecutive
    const int c0 = tid * per < C ? tid * per : C, c1 = c0 + per < C ? c0 + per : C;
    int64_t mine = 0;
    for (int c = c0; c < c1; ++c) mine += cc_clampi(chunk_bits[f * C + c], 0, kSlotBits);
    s_part[tid] = mine;
    __syncthreads();
    if (tid == 0) {
        int64_t acc = 0;
        for (int i = 0; i < kThreads; ++i) {
            const int64_t v = s_part[i];
            s_part[i] = acc;
            acc += v;
        }
        const int64_t bytes = (acc + 7) >> 3;
        frame_bytes[f] = (int32_t)(bytes < 0x7fffffff ? bytes : 0x7fffffff);
    }
    __syncthreads();
    int64_t at = start + s_part[tid];
    for (int c = c0; c < c1; ++c) {
        chunk_off[f * C + c] = at;
        at += cc_clampi(chunk_bits[f * C + c], 0, kSlotBits);
    }
}

// A workgroup of kThreads per chunk (blockIdx.x): its bits shifted to their offset; the first and last word of a chunk are OR-ed into the
// zeroed output (neighbouring chunks share them), the words between are stored.
template <int kThreads, int kSlotWords>
__device__ __forceinline__ void cc_pack_chunk(const uint32_t* __restrict__ slots, const int32_t* __restrict__ chunk_bits,
                                              const int64_t* __restrict__ chunk_off, uint32_t* __restrict__ out, int64_t out_bits) {
    const int64_t id = blockIdx.x;
    const int len = cc_clampi(chunk_bits[id], 0, kSlotWords * 32);
    const int64_t off = chunk_off[id];
    if (len == 0 || off < 0 || off > out_bits - len) return;                      // (cannot happen with the offsets of cc_pack_scan)
    const uint32_t* src = slots + id * kSlotWords;
    const int nsrc = (len + 31) >> 5;
    const uint32_t tail = (len & 31) ? (1u << (len & 31)) - 1u : 0xffffffffu;       // what the last source word holds
    const uint32_t sh = (uint32_t)(off & 31);
    const int64_t w0 = off >> 5;
    const int nout = (int)(((off + len - 1) >> 5) - w0) + 1;
    for (int j = threadIdx.x; j < nout; j += kThreads) {
        uint32_t lo = 0, hi = 0;                                                  // source words j - 1 and j
        if (j < nsrc) hi = src[j] & (j == nsrc - 1 ? tail : 0xffffffffu);
        if (j >= 1 && j - 1 < nsrc) lo = src[j - 1] & (j - 1 == nsrc - 1 ? tail : 0xffffffffu);
        const uint32_t v = sh ? (hi << sh) | (lo >> (32u - sh)) : hi;
        if (j == 0 || j == nout - 1)
            atomicOr(out + w0 + j, v);
        else
            out[w0 + j] = v;
    }
}
