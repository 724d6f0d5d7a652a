// Cross-attention onto the keys of a LONG prompt (ccedit_amd/prompt.py: 2, 3 or 4 chunks of 77 CLIP tokens) — gfx950.
//
//     O[row, h] = softmax(Q[row, h] K[clip, h]^T * scale) V[clip, h]        Lk = 154 / 231 / 308, K / V shared by all query rows of a clip
//
// attn_text_kernel (attntext.hip) keeps K and V^T of a 320-channel group in LDS for Lk <= 96: 136 KB.  Up to 320 padded keys do not
// fit that way, so here a workgroup owns an 80-CHANNEL group (one head of d = 80) and all keys of it:
//     K     32 KT rows x 176 B  (80 channels + 8 zero pad channels; KT = 5 / 8 / 10 key tiles)     <= 56,320 B
//     V^T   112 rows x (32 KT + 8) keys x 2 B  (80 channels + the rows a last head's padded tiles reach into, zeros)   <= 73,472 B
// Otherwise the structure is attn_text_kernel's: a wave owns 32 query rows and walks the heads of its group; S^T = K Q^T with the query
// fragments straight from global memory in MFMA B layout; ALL keys at once — one max, one exp2 per score, no running rescale; the K
// rows are read in the permuted order that makes a lane's score accumulators the B operand of the second product; row sums on the
// matrix pipe; O^T = V^T P, lane halves exchanged into 8-channel runs and stored as 16 bytes.  KT score tiles are 16 KT accumulator
// registers (160 at 308 keys): one wave per SIMD, 4 waves per workgroup.
//
// Only d = 80 is instantiated.  Measured at the production launches (34 frames, two clips' K / V, tools/prompt_time.py, medians of three
// alternating rounds, arm / the kernel that serves the launch without it, us): d = 80 at 1536 rows per frame 61 / 90 (154 keys,
// attn_kernel), 77 / 104 (231, attn_spatial_kernel), 88 / 111 (308, attn_spatial_kernel) — kept; d = 40 at 6144 rows per frame (two heads
// per group, which the template still expresses) 145 / 148 (within the 11 us between rounds), 181 / 159, 206 / 174 — not kept: with
// 80-channel groups a workgroup reads 160-byte pieces of the 640-byte query rows, and at d = 40 that costs more than the resident keys save.
#include "common.h"
#include <stdlib.h>

namespace {

constexpr int kG = 80;                  // channels per group
constexpr int kKRow = (kG + 8) * 2;     // bytes per K row in LDS: 176
constexpr int kVRows = 112;             // V^T rows: 80 channels + what the padded 32-row tiles of the last head reach into (<= 103)
constexpr int kNT = 256;

__device__ __forceinline__ void atl_swap(float& x, float& y) {      // see g8_swap (gemm8p.hip)
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(y), false, false);
    x = __uint_as_float(r[0]);
    y = __uint_as_float(r[1]);
}

template <int D, int KT>
__global__ __launch_bounds__(kNT, 1) void attn_text_long_kernel(const CcAttnDesc a, int ngroups, int nkvb) {
    constexpr int HPG = kG / D;                     // heads per group
    constexpr int KS = (D + 15) / 16;               // k-steps of Q K^T
    constexpr int DT = (D + 31) / 32;               // 32-row tiles of O^T
    constexpr int kKeys = 32 * KT;                  // padded key count
    constexpr int kVRow = (kKeys + 8) * 2;          // bytes per V^T row
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* const sK = smem;
    char* const sV = smem + kKeys * kKRow;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hi = lane >> 5;

    // workgroup b runs on XCD b % 8; the 32 workgroups of an XCD = (32 / ngroups) row lanes x ngroups channel groups, so the groups
    // of a query row run beside each other on one L2
    const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
    const int group = j % ngroups, qlane = j / ngroups;
    const int nlanes = (int)(gridDim.x >> 3) / ngroups;
    if (qlane >= nlanes) return;
    const int stride = nlanes * 4 * 8;              // 32-row tiles between two tiles of one wave
    const int first = (qlane * 4 + wave) * 8 + xcd;
    const int ch0 = group * kG;
    const float c2 = a.scale * 1.4426950408889634f;
    const int64_t rows_per_kvb = (int64_t)a.kv_div * a.Lq;

    // logical key of MFMA row m of a key tile: m = 8 a + 4 h + i  ->  16 (a >> 1) + 8 h + 4 (a & 1) + i
    const int krow = 16 * (l31 >> 4) + 8 * ((l31 >> 2) & 1) + 4 * ((l31 >> 3) & 1) + (l31 & 3);

    // keys >= Lk lie in the LAST key tile only (32 (KT - 1) < Lk, checked by the launcher): it starts from -1e30 there instead of 0 — the
    // zero K rows of the padding add nothing, exp2 turns it into 0.  Register r of tile kt is key 32 kt + 16 (r >> 3) + 8 hi + (r & 7).
    f32x16 maskl;
#pragma unroll
    for (int r = 0; r < 16; ++r) maskl[r] = (32 * (KT - 1) + 16 * (r >> 3) + 8 * hi + (r & 7)) < a.Lk ? 0.f : -1e30f;
    const bf16x8 ones = {1, 1, 1, 1, 1, 1, 1, 1};

    for (int kvb = 0; kvb < nkvb; ++kvb) {
        // ---- stage K (zero-padded rows / columns) and V^T of (kvb, group) ----
        __syncthreads();
        for (int t = tid; t < kKeys * (kG / 8 + 1); t += kNT) {                 // K: consecutive threads = consecutive channels
            const int key = t / (kG / 8 + 1), g8 = t - key * (kG / 8 + 1);
            bf16x8 kv = {0, 0, 0, 0, 0, 0, 0, 0};
            if (key < a.Lk && g8 < kG / 8) kv = *(const bf16x8*)((const bf16*)a.k + (size_t)((int64_t)kvb * a.kv_outer_rows + key) * a.ldk + ch0 + g8 * 8);
            *(bf16x8*)(sK + key * kKRow + g8 * 16) = kv;
        }
        for (int t = tid; t < kKeys * (kG / 8); t += kNT) {                     // V^T: consecutive threads = consecutive KEYS (attntext.hip)
            const int g8 = t / kKeys, key = t - g8 * kKeys;
            bf16x8 vv = {0, 0, 0, 0, 0, 0, 0, 0};
            if (key < a.Lk) vv = *(const bf16x8*)((const bf16*)a.v + (size_t)((int64_t)kvb * a.kv_outer_rows + key) * a.ldv + ch0 + g8 * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) *(bf16*)(sV + (g8 * 8 + e) * kVRow + key * 2) = vv[e];
        }
        for (int t = tid; t < (kVRows - kG) * (kVRow / 16); t += kNT)          // the V^T rows past the last channel
            *(bf16x8*)(sV + kG * kVRow + t * 16) = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
        for (int t = tid; t < kG; t += kNT)                                     // ... and the 8 pad keys of every row (never read)
            *(bf16x8*)(sV + t * kVRow + kKeys * 2) = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
        __syncthreads();

        const int64_t row0 = (int64_t)kvb * rows_per_kvb;
        const int ntiles = (int)((rows_per_kvb + 31) / 32);
        // Q fragments of head h of tile t (B operand): channels 16 ks + 8 hi .. + 7 of this lane's row
        auto load_q = [&](int t, int h, bf16x8(&q)[KS]) {
            const int64_t rloc = (int64_t)t * 32 + l31;
            const bf16* const qr = (const bf16*)a.q + (size_t)(row0 + (rloc < rows_per_kvb ? rloc : 0)) * a.ldq + ch0 + h * D;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                // always a GLOBAL load from inside the tensor (rows past the end read row 0 of the clip and are never stored)
                const int dofs = 16 * ks + 8 * hi;
                q[ks] = *(const bf16x8*)(qr + (dofs < D ? dofs : D - 8));
                if (16 * ks + 8 >= D && dofs >= D) q[ks] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};        // (D = 40: the upper half of the third k-step)
            }
        };
        // all heads' fragments of a tile are requested a whole tile ahead (attntext.hip)
        bf16x8 qa[HPG][KS];
        if (first < ntiles) {
#pragma unroll
            for (int h = 0; h < HPG; ++h) load_q(first, h, qa[h]);
        }
        for (int t = first; t < ntiles; t += stride) {
            const int64_t rloc = (int64_t)t * 32 + l31;
            const bool rok = rloc < rows_per_kvb;
            // row of (batch, i): contiguous token rows (q_outer_rows == Lq is checked by the launcher)
            bf16* const orow = (bf16*)a.o + (size_t)(row0 + (rok ? rloc : 0)) * a.ldo + ch0;
#pragma unroll
            for (int h = 0; h < HPG; ++h) {
                __builtin_amdgcn_sched_barrier(0);       // one head at a time (register budget)
                bf16x8 qf[KS];
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) qf[ks] = qa[h][ks];
                // ---- S^T = K Q^T, KT key tiles; rows read in permuted order (krow); the fragments of tile kt + 1 are requested
                //      before the MFMAs of tile kt are issued ----
                f32x16 sc[KT];
                bf16x8 kf[2][KS];
                auto read_k = [&](int kt, bf16x8(&f)[KS]) {
                    const char* const kp = sK + (32 * kt + krow) * kKRow + (h * D + 8 * hi) * 2;
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks) f[ks] = *(const bf16x8*)(kp + ks * 32);
                };
                read_k(0, kf[0]);
#pragma unroll
                for (int kt = 0; kt < KT; ++kt) {
                    if (kt + 1 < KT) read_k(kt + 1, kf[(kt + 1) & 1]);
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int r = 0; r < 16; ++r) sc[kt][r] = kt == KT - 1 ? maskl[r] : 0.f;
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks)
                        sc[kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[kt & 1][ks], qf[ks], sc[kt], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
                __builtin_amdgcn_sched_barrier(0);
                if (t + stride < ntiles) load_q(t + stride, h, qa[h]);
                __builtin_amdgcn_sched_barrier(0);
                // ---- softmax over the keys (all of them at once: one max, one exp2 per score) ----
                float mx = -1e30f;
#pragma unroll
                for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sc[kt][r]);
                mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
                const float mc = mx * c2;
                bf16x8 pf[KT][2];
#pragma unroll
                for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) pf[kt][r >> 3][r & 7] = f2bf(__builtin_amdgcn_exp2f(sc[kt][r] * c2 - mc));
                // the row sums on the matrix pipe: 1^T P, of the bf16 values the second product uses
                f32x16 ssum;
#pragma unroll
                for (int r = 0; r < 16; ++r) ssum[r] = 0.f;
#pragma unroll
                for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                    for (int s2 = 0; s2 < 2; ++s2) ssum = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ones, pf[kt][s2], ssum, 0, 0, 0);
                const float inv = 1.0f / ssum[0];
                // ---- O^T = V^T P: two key tiles (four k-steps) of V^T fragments in flight ----
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) {
                    f32x16 o;
#pragma unroll
                    for (int r = 0; r < 16; ++r) o[r] = 0.f;
                    const char* const vp = sV + (h * D + 32 * dt + l31) * kVRow + 8 * hi * 2;
#pragma unroll
                    for (int i0 = 0; i0 < 2 * KT; i0 += 4) {
                        bf16x8 vf[4];
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            if (i0 + i < 2 * KT) vf[i] = *(const bf16x8*)(vp + 16 * (i0 + i) * 2);
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            if (i0 + i < 2 * KT) o = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf[i], pf[(i0 + i) >> 1][(i0 + i) & 1], o, 0, 0, 0);
                    }
                    // register r: channel 32 dt + (r & 3) + 8 (r >> 2) + 4 hi of this lane's row -> 8-channel runs by the half exchange
#pragma unroll
                    for (int tq = 0; tq < 2; ++tq) {
                        float x[4], y[4];
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            x[e] = o[8 * tq + e] * inv;
                            y[e] = o[8 * tq + 4 + e] * inv;
                            atl_swap(x[e], y[e]);
                        }
                        const int dofs = 32 * dt + 16 * tq + 8 * hi;
                        if (rok && dofs < D) {
                            const bf16x8 w = {f2bf(x[0]), f2bf(x[1]), f2bf(x[2]), f2bf(x[3]), f2bf(y[0]), f2bf(y[1]), f2bf(y[2]), f2bf(y[3])};
                            *(bf16x8*)(orow + h * D + dofs) = w;
                        }
                    }
                }
            }
        }
    }
}

template <int D, int KT>
int launch_long(const CcAttnDesc& a, hipStream_t s) {
    constexpr int lds = 32 * KT * kKRow + kVRows * (32 * KT + 8) * 2;
    static_assert(lds <= 160 * 1024, "K and V^T of one 80-channel group must fit the LDS");
    static unsigned long long attr_done = 0;
    if (int rc = cc_max_dynamic_lds((const void*)attn_text_long_kernel<D, KT>, lds, &attr_done, "attn_text_long")) return rc;
    const int ngroups = a.heads * a.d / kG;
    const int nkvb = a.batches / a.kv_div;
    cc_note_kernel("attn_text_long_kernel d=%d", D);
    hipLaunchKernelGGL((attn_text_long_kernel<D, KT>), dim3(256), dim3(kNT), lds, s, a, ngroups, nkvb);
    return cc_launch_status("attn_text_long_kernel");
}

template <int D>
int launch_long_d(const CcAttnDesc& a, hipStream_t s) {
    switch (a.Lk) {
        case 154: return launch_long<D, 5>(a, s);
        case 231: return launch_long<D, 8>(a, s);
        default: return launch_long<D, 10>(a, s);
    }
}

}  // namespace

// the geometry of cc_attn_text_applicable (attntext.hip) with 80-channel groups (whole 320-channel groups of them), d = 80 (see the head
// of the file), and exactly the key counts of 2, 3 and 4 prompt chunks: every one of them ends in the last 32-key tile of its padded count.
// Like that kernel it stages every kv batch in every workgroup: K / V per frame (CCEDIT_ATTN_KV_PER_FRAME) go to the general kernels.
bool cc_attn_text_long_applicable(const CcAttnDesc& a) {
    return !(a.flags & CCEDIT_ATTN_KV_PER_FRAME) && a.d == 80 && (a.Lk == 154 || a.Lk == 231 || a.Lk == 308) && a.seg1_len == 0 && !a.causal &&
           (a.heads * a.d) % 320 == 0 && 32 % (a.heads * a.d / kG) == 0 && a.q_inner == 1 && a.q_seq_rows == 1 && a.q_outer_rows == a.Lq &&
           a.kv_inner == 1 && a.kv_seq_rows == 1 && a.kv_outer_rows >= a.Lk && a.batches % a.kv_div == 0 && a.ldo % 8 == 0 &&
           (int64_t)a.kv_div * a.Lq >= 2048;
}

int cc_attn_text_long_launch(const CcAttnDesc& a, hipStream_t s) {
    return launch_long_d<80>(a, s);
}
