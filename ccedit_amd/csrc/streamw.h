// Building blocks of the STREAMING WEIGHT-IN-REGISTER kernels (lin320_kernel / lin320s_kernel: lin320.hip, lin640s_kernel:
// lin640.hip, temp320s_kernel: temp320.hip) — gfx950.  A slice of the weights lives in registers as MFMA A fragments, activation
// tiles stream past it through a DMA ring in LDS, the output leaves one iteration later.  Everything here is force-inlined into
// the kernel that calls it; each kernel keeps its own tile geometry, DMA plan and epilogue.
//
// These loops are bound by INSTRUCTION ISSUE, not by a pipe: a wave issues at most one instruction per four cycles, a step has 30 MFMAs
// (480 cycles) per wave, and the first version of temp320s_kernel spent ~860 instructions per step and wave — 500 of them scalar (ring
// wrap-arounds, 64-bit address products, exec-mask juggling around lane-dependent DMA selects, a 45-way switch for the counted
// wait, SGPR spills) — i.e. 1.5 us per step whatever the memory system or the matrix pipe did (ablation: all of MFMA, DMA and
// stores switched off left 0.56 us per step).  Hence: ring slots as wrap-around counters (three scalar instructions each), running byte
// offsets instead of row x stride products, DMA sources valid for every lane (padding slots copy a neighbouring granule: no
// selects, no exec masks), the same number of loads per tile in every requesting wave (compile-time wait counts).
#pragma once
#include "common.h"

// LDS-only workgroup barrier: __syncthreads() would also drain vmcnt, i.e. wait for the tiles in flight
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
template <int N>
__device__ __forceinline__ void vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// Workgroup b runs on XCD b % 8: the 32 workgroups of an XCD take (32 / nslice) unit lanes x nslice channel slices, so the slices of
// a layer walk the SAME units at the same time and the activation rows come out of that XCD's L2 for all but the first.  The units
// (pixel tiles, columns) of this workgroup are first, first + lanes, ... < end: `count` of them; none when first >= end (count 0).
struct WorkSplit {
    int slice, lanes, first, end, count;
};
__device__ __forceinline__ WorkSplit work_split(unsigned block, int nslice, int n_units) {
    const int xcd = block & 7, j = block >> 3;
    WorkSplit w;
    w.lanes = 32 / nslice;
    w.slice = j % nslice;
    const int plane = j / nslice;
    const int per_xcd = (n_units + 7) >> 3;
    const int lo = xcd * per_xcd;
    w.first = lo + plane;
    w.end = plane < w.lanes ? min(lo + per_xcd, n_units) : 0;
    w.count = w.first < w.end ? (w.end - w.first + w.lanes - 1) / w.lanes : 0;
    return w;
}

// The A-operand fragments of one sixteen-channel tile (channels ch .. ch + 15, ch % 16 == 0), resident for the whole kernel:
// wf[ks] = elements koff(ks) + 8 (lane >> 4) .. + 7 of weight row ch + (lane & 15); koff(ks) % 32 == 0, kKpad = d.Kpad (a constant
// of the kernel: it scales a 64-bit address).  With the fragment-ordered copy (CcGemmDesc.Wfrag) a fragment is one contiguous
// kilobyte per wave (rows are padded to 256: a wave beyond N reads zeros); from row-major W a wave beyond N reads any valid row.
template <int kKpad, int KS, class KOff>
__device__ __forceinline__ void load_wfrags(bf16x8 (&wf)[KS], const CcGemmDesc& d, int ch, int lane, KOff koff) {
    if (d.Wfrag) {
        const bf16* __restrict__ blk = (const bf16*)d.Wfrag + ((size_t)(ch >> 4) * (kKpad / 32) * 64 + lane) * 8;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) wf[ks] = *(const bf16x8*)(blk + (koff(ks) >> 5) * 512);
    } else {
        const bf16* __restrict__ row = (const bf16*)d.W + (size_t)min(ch + (lane & 15), d.N - 1) * d.Kpad + (lane >> 4) * 8;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) wf[ks] = *(const bf16x8*)(row + koff(ks));
    }
}
// p[c .. c + 3] (bias, column sums) of the lane's four channels; zeros without p
__device__ __forceinline__ f32x4 load_quad(const float* p, int c) {
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = p ? p[c + e] : 0.f;
    return v;
}

// ---- the DMA ring ----
// Ring slots are wrap-around counters, never a modulo (see the top of the file).
template <int N>
__device__ __forceinline__ void ring_next(int& slot) { slot = slot == N - 1 ? 0 : slot + 1; }
// The first RX - 1 tiles are requested BEHIND the weight loads, in the same breath — one latency instead of two at the start of
// every launch; the one wait covers both: from here on the queue of a requesting wave holds DMA (and stores) only.
template <int RX, class Stage>
__device__ __forceinline__ void ring_prologue(int& staged, int ntile, Stage stage_next) {
    for (; staged < RX - 1 && staged < ntile; ++staged) stage_next();
    vmcnt<0>();
}
// ... and tile i + RX - 1 at the top of iteration i, right after the barrier that frees its slot
template <class Stage>
__device__ __forceinline__ void ring_step(int& staged, int ntile, Stage stage_next) {
    if (staged < ntile) {
        stage_next();
        ++staged;
    }
}
// The counted wait: loads return in order, so with at most the loads of `later` (<= kMaxLater = ring depth - 2) newer tiles
// outstanding, the awaited tile has landed.  It is exact only for a queue that holds these loads alone, hence:
//  * DMA by waves 0-3, stores and atomics by waves 4-7 (lin640s, temp320s): a store in the same queue has to complete as well
//    before the count can fall to the number of younger loads;
//  * no register-returning load inside the loop: the compiler's wait for it would drain the DMA queue;
//  * every requesting wave issues kPerTile loads per tile, so the counts are compile-time constants.
template <int kPerTile, int kMaxLater>
__device__ __forceinline__ void wait_later(int later) {
    if constexpr (kMaxLater == 0) vmcnt<0>();
    else if (later >= kMaxLater) vmcnt<kMaxLater * kPerTile>();
    else wait_later<kPerTile, kMaxLater - 1>(later);
}

// ---- the K loop ----
// The B fragment of k-step ks + DEPTH - 1 is requested before the MFMAs of k-step ks are issued (hipcc on its own reads, waits,
// multiplies, reads again); the compiler counts the reads still in flight behind a fragment (all issued in order).  frag(ks) reads
// the fragment(s) of a k-step from LDS, mma(ks, x) issues its MFMAs, hook(ks) runs behind them (work for the shadow of the matrix
// pipe; it closes with its own sched_barrier).
template <int KS, int DEPTH, class Frag, class Mma, class Hook>
__device__ __forceinline__ void frag_pipeline(Frag frag, Mma mma, Hook hook) {
    decltype(frag(0)) xq[DEPTH];
#pragma unroll
    for (int ks = 0; ks < DEPTH - 1; ++ks) xq[ks] = frag(ks);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        if (ks + DEPTH - 1 < KS) xq[(ks + DEPTH - 1) % DEPTH] = frag(ks + DEPTH - 1);
        __builtin_amdgcn_sched_barrier(0);
        mma(ks, xq[ks % DEPTH]);
        __builtin_amdgcn_sched_barrier(0);
        hook(ks);
    }
}
template <int KS, int DEPTH, class Frag, class Mma>
__device__ __forceinline__ void frag_pipeline(Frag frag, Mma mma) {
    frag_pipeline<KS, DEPTH>(frag, mma, [](int) {});
}

// ---- the unpadded, XOR-swizzled activation tile (lin640s, temp320s) ----
// 16 rows of kRS bytes (a multiple of 256: a row's position in the banks depends on the swizzle alone), NO padding; granule j of
// row r sits at position j ^ (r & 15) of its 16-granule block (the DMA picks the source granule per destination slot).
// ds_read_b128 is served in the lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, ... (MI355X_MICROARCH.md): lane (c, g) of a
// B fragment reads granule 4 ks + g of row c, so a group holds all sixteen c — half of them with g, half with g + 1 — and both
// halves are closed under c ^ 1 and c ^ 2: the positions ((4 ks + g) ^ c) cover the sixteen 16-byte bank groups exactly once.
// (Rows padded to 1296 B, the usual recipe, put two lanes of every group on the same banks: SQ_LDS_BANK_CONFLICT = 20 % of
// lin640s_kernel's cycles.)
// B fragment of k-step ks, lane (c16, g4): xlane[ks & 3] + (ks >> 2) * 256
template <int kRS>
__device__ __forceinline__ void swizzled_lanes(int (&xlane)[4], int c16, int g4) {
#pragma unroll
    for (int m = 0; m < 4; ++m) xlane[m] = c16 * kRS + (((4 * m + g4) ^ c16) << 4);
}
__device__ __forceinline__ bf16x8 swizzled_frag(const char* tile, const int (&xlane)[4], int ks) {
    return *(const bf16x8*)(tile + xlane[ks & 3] + (ks >> 2) * 256);
}

// ---- statistics that meet across waves in LDS ----
// The waves add their fp32 partials in DOUBLE (exact for these sums, so order-independent) to a (sum, sum of squares) pair at
// `pair` + kOff bytes.  (asm: for an LDS atomic the compiler first drains the vector-memory queue — the DMA writes LDS too.)
template <int kOff = 0>
__device__ __forceinline__ void lds_add_f64_pair(const double* pair, float s, float q) {
    const uint32_t a = (uint32_t)(uintptr_t)(LDS_AS const char*)pair;
    asm volatile("ds_add_f64 %0, %1 offset:%3\n\tds_add_f64 %0, %2 offset:%4" ::"v"(a), "v"((double)s), "v"((double)q), "n"(kOff), "n"(kOff + 8) : "memory");
}
// ... and one lane per slot takes the total to memory one iteration later, leaving the slot zero for its next use
__device__ __forceinline__ void lds_flush_f64(double* slot, double* dst) {
    const double v = *slot;
    *slot = 0.0;
    unsafeAtomicAdd(dst, v);
}
