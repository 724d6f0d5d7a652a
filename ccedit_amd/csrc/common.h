// Shared device helpers for the gfx950 kernels of libccedit_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ccedit_hip.h"

typedef __bf16 bf16;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;

#define GLOBAL_AS __attribute__((address_space(1)))
#define LDS_AS __attribute__((address_space(3)))

// 16-byte asynchronous global -> LDS copy (global_load_lds_dwordx4).  The LDS destination is the
// wave-uniform `lds_wave_base` + lane*16; the global source address is per lane.
__device__ __forceinline__ void glds16(const void* gsrc, void* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const GLOBAL_AS void*)gsrc, (LDS_AS void*)lds_wave_base, 16, 0, 0);
}

__device__ __forceinline__ float bf2f(bf16 v) { return (float)v; }
__device__ __forceinline__ bf16 f2bf(float v) { return (bf16)v; }

// SiLU, v * sigmoid(v) (nn.SiLU of openaimodel.py:441-444 etc.).  The reciprocal is v_rcp_f32 (1 ulp), not an IEEE division: hipcc
// expands `v / (1 + exp(-v))` into the ten-instruction v_div_scale / v_div_fmas / v_div_fixup sequence (2984 of them in norm.o), which
// made the GroupNorm + SiLU passes VALU-bound (temporal GroupNorm at 34 x 64 x 96 x 320: 70 us with SiLU, 56 us without, 45 us for a
// copy of the same bytes).  The result is rounded to bf16 (8 bits) right after.
__device__ __forceinline__ float silu_f(float v) { return v * __builtin_amdgcn_rcpf(1.0f + __expf(-v)); }
// GELU, 0.5 v (1 + erf(v / sqrt 2)) = v Phi(v) (GEGLU, attention.py:115-126: F.gelu, the exact-erf form), as v * sigmoid(u(v)) with
// u = v (a + b v^2 + c v^4) fitted to Phi (minimax over |v| <= 9; the argument is clamped there — beyond, Phi is 0 or 1 to 1e-11 and
// the quartic would turn around at |v| = 11).  |error| <= 2.6e-5 ABSOLUTE over all v (tools/exp/gelu_fit.py: fp32 evaluation against
// fp64 erf) — 300 times below the bf16 rounding of the result at |v| ~ 3, where the maximum sits, and the result is rounded to bf16
// right after.  Six plain VALU instructions + v_exp_f32 + v_rcp_f32; rounds 1-5 used Abramowitz & Stegun 7.1.28
// (1 - (1 + a1 x + ... + a6 x^6)^-16: 3e-7, sixteen VALU instructions) — the GELU is the VALU share of ff320 and of the GEGLU
// epilogues (13-16 % of a GEGLU GEMM at the 64x96 and 32x48 levels with the cheaper of the two before), libdevice's erff twice that.
// The coefficients carry -log2(e): v_exp_f32 is 2^x.
#ifdef CCEDIT_GELU_AS71_28          // probe builds only (tools/exp/build_gelu_variant.sh): the formula of rounds 1-5, for the same-box A/B
__device__ __forceinline__ float gelu_erf_f(float v) {
    const float x = fabsf(v) * 0.70710678118654752440f;
    float p = fmaf(x, 0.0000430638f, 0.0002765672f);
    p = fmaf(x, p, 0.0001520143f);
    p = fmaf(x, p, 0.0092705272f);
    p = fmaf(x, p, 0.0422820123f);
    p = fmaf(x, p, 0.0705230784f);
    p = fmaf(x, p, 1.0f);
    p = p * p;
    p = p * p;
    p = p * p;
    p = p * p;
    const float e = 1.0f - __builtin_amdgcn_rcpf(p);          // erf(|v| / sqrt 2)
    return 0.5f * v + 0.5f * fabsf(v) * e;                     // 0.5 v (1 + sign(v) e)
}
#else
__device__ __forceinline__ float gelu_erf_f(float v) {
    const float vc = __builtin_amdgcn_fmed3f(v, -9.0f, 9.0f);
    const float t = vc * vc;
    float p = fmaf(t, 0.00101426306f, -0.106775724f);       // -log2(e) * (c, b, a) = -log2(e) * (-7.03033577e-4, 7.40112921e-2, 1.59501577)
    p = fmaf(t, p, -2.30112134f);
    const float e = __builtin_amdgcn_exp2f(p * vc);          // exp(-u)
    return v * __builtin_amdgcn_rcpf(1.0f + e);
}
#endif

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// The library's dispatch policy: ONE table of named integer switches (core.cpp), all defaulting to the fast path.  Nothing in the
// library reads the environment: the host sets entries through ccedit_policy_set (ccedit_amd/policy.py reads CCEDIT_POLICY once and
// pushes it).  Every switch selects between kernels that compute the same fp32 sums in a different order — A/B and test arms
// ("specialised kernels reproduce the generic ones", tests/test_fullsize_gpu.py), never a change of arithmetic.
struct CcPolicy {
    int conv_halo = 1;      // 3x3 stride-1 convs on the LDS-halo kernel with the four-slot weight ring (2: the two-slot kernel of rounds 2-5; 0: tap-gather)
    int conv_wide = 1;      // ... on 256-pixel (16 x 16) tiles: 1 where it measured faster (convhalo.hip: cc_conv_wide_auto), 2 wherever it applies, 0 never
    int g8 = 1;             // persistent eight-phase GEMM for long Linears (0: the tap_gemm block shapes)
    int g8_conv = 1;        // ... its tap-gather mode for 3x3 convs onto >= 1024 channels
    int g8_temporal = 1;    // ... and for Conv1d k3 over T at >= 640 channels
    int g8_split = -1;      // split-K at the 8x12 level: -1 auto, 0 off, n fixed
    int g8_mfma16 = 1;      // ... its K loop on v_mfma_f32_16x16x32_bf16 (0: 32x32x16; 1 and 2 select the same kernels, 2 is what tests set)
    int lin320 = 1;         // register-resident-weight K = 320 Linears (0: tap_gemm)
    int lin320s = 1;        // ... the streaming deep-ring variant (0: the K-split kernel)
    int lin640 = 1;         // streaming K = 640 Linears (0: g8)
    int temp320 = 1;        // streaming Conv1d k3 at 320 channels (0: tap_gemm)
    int attn_short = 1;     // temporal attention kernel (0: the general flash kernel)
    int attn_text = 1;      // text cross-attention kernel
    int attn_spatial = 1;   // long self-attention kernel with the reference in the MFMA: 1 = d 40 and d 80, 2 = d 40 only, 0 = off
    int attn_pv16 = 1;      // ... its PV product in 16x16x32 tiles (0: 32x32x16)
    int attn_opt = 1;       // ... softmax reference fixed by the first key tile, exact re-run of a workgroup that overflowed (0: tracked on every tile)
    int gn_flat = 1;        // flat thread mapping of the temporal GroupNorm at the two large levels
    int gn_apply_flat = 1;  // column-per-thread, four-rows-in-flight mapping of the spatial GroupNorm apply pass (0: a wave per pixel row)
    int f32_split = 1;      // fp32 first-stage contractions as six exact bf16 products per fp32 product on the bf16 matrix pipe (0: v_mfma_f32_32x32x2_f32)
};
const CcPolicy& cc_policy();

void cc_set_error(const char* fmt, ...);
void cc_note_kernel(const char* fmt, ...);      // which kernel template the entry point dispatched to (ccedit_last_kernel)

#define CC_CHECK_ARG(cond, ...)          \
    do {                                 \
        if (!(cond)) {                   \
            cc_set_error(__VA_ARGS__);   \
            return CCEDIT_EINVAL;        \
        }                                \
    } while (0)

#define CC_UNSUPPORTED(cond, ...)        \
    do {                                 \
        if (cond) {                      \
            cc_set_error(__VA_ARGS__);   \
            return CCEDIT_EUNSUPPORTED;  \
        }                                \
    } while (0)

// Per-device once-guard for hipFuncSetAttribute(MaxDynamicSharedMemorySize): the attribute is a property of the
// (function, device) pair, so a process that drives a second GPU must set it there too.  `done` is a per-call-site
// bitmask over device ordinals (devices >= 64 simply set it every time).
static inline int cc_max_dynamic_lds(const void* fn, int bytes, unsigned long long* done, const char* what) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess && dev < 64 && ((*done >> dev) & 1ull)) return CCEDIT_OK;
    if (e == hipSuccess) e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) {
        cc_set_error("hipFuncSetAttribute(%s): %s", what, hipGetErrorString(e));
        return (int)e;
    }
    if (dev < 64) *done |= 1ull << dev;
    return CCEDIT_OK;
}

// ... for every arm (template instantiation) of a kernel family, once per device at the family's FIRST launch there — not at the
// arm's own first launch, which can fall inside a graph capture.  One `done` word per family.
template <class... Arms>
static inline int cc_family_dynamic_lds(int bytes, unsigned long long* done, const char* what, Arms*... arms) {
    int dev = 0;
    if (hipGetDevice(&dev) == hipSuccess && dev < 64 && ((*done >> dev) & 1ull)) return CCEDIT_OK;
    int rc = CCEDIT_OK;
    for (const void* fn : {(const void*)arms...}) {
        unsigned long long arm_done = 0;
        if (rc == CCEDIT_OK) rc = cc_max_dynamic_lds(fn, bytes, &arm_done, what);
    }
    if (rc == CCEDIT_OK && dev < 64) *done |= 1ull << dev;
    return rc;
}

static inline int cc_launch_status(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        cc_set_error("%s: %s", what, hipGetErrorString(e));
        return (int)e;
    }
    return CCEDIT_OK;
}

// Pixel I/O launchers (pixel.hip); the exported entry points with their argument checks are in core.cpp
int cc_pixel_resize_u8(const uint8_t* src, void* dst, uint8_t* tmp, const int32_t* ytab, int32_t yk, const int32_t* xtab, int32_t xk,
                       int32_t N, int32_t Hs, int32_t Ws, int32_t H, int32_t W, int32_t out_f32, hipStream_t s);
int cc_pixel_resize_f32(const float* src, float* dst, const int32_t* ytab, const int32_t* xtab, int64_t planes, int32_t Hs, int32_t Ws,
                        int32_t H, int32_t W, hipStream_t s);
int cc_pixel_kth_values(const float* x, int32_t B, int64_t n, const int64_t* ranks, int32_t nr, float* out, void* workspace, hipStream_t s);
int cc_pixel_minmax(const float* x, int32_t B, int64_t n, float* out, hipStream_t s);
int cc_pixel_depth_hint(const float* depth, float* hint, const float* stats, int32_t stat_stride, int32_t B, int64_t n, int32_t flip,
                        hipStream_t s);
int cc_pixel_frames_to_u8(const float* x, uint8_t* out, int32_t B, int64_t P, int32_t mode, int32_t unit_range, hipStream_t s);

// Edit-mask launchers (mask.hip); entry points and argument checks in core.cpp
int cc_mask_resize_nearest(const uint8_t* src, uint8_t* dst, const int32_t* ytab, const int32_t* xtab, int32_t N, int32_t Hs, int32_t Ws,
                           int32_t H, int32_t W, hipStream_t s);
int cc_mask_latent(const uint8_t* mask_px, uint8_t* mask_lat, int64_t N, int32_t H, int32_t W, hipStream_t s);
int cc_mask_inpaint_blend(const float* x, const float* x0, const float* noise, const uint8_t* mask, float* y, int32_t B, int32_t C, int64_t P,
                          float sigma, float s, hipStream_t st);
int cc_mask_composite(const float* result, const float* original, const uint8_t* mask_px, float* out, int32_t B, int64_t P, hipStream_t st);
int cc_mask_dilate(const uint8_t* src, uint8_t* tmp, uint8_t* dst, int64_t N, int32_t H, int32_t W, int32_t R, int32_t invert, hipStream_t s);
int cc_mask_inpaint_blend_level(const float* x, const float* x0, const float* noise, const uint8_t* strength, float* y, int32_t B, int32_t C,
                                int64_t P, int32_t thr, float sigma, float s, hipStream_t st);

// Graded edit-mask launchers (softmask.hip); entry points and argument checks in core.cpp
int cc_mask_feather(const uint8_t* src, uint16_t* tmp16, uint8_t* dst, int64_t N, int32_t H, int32_t W, int32_t R, hipStream_t s);
int cc_mask_latent_graded(const uint8_t* mask_px, uint8_t* strength_lat, int64_t N, int32_t H, int32_t W, hipStream_t s);
int cc_mask_composite_graded(const float* result, const float* original, const uint8_t* strength_px, float* out, int32_t B, int64_t P,
                             hipStream_t st);

// Window launchers (window.hip); entry points and argument checks in core.cpp
int cc_window_gather(const float* x, float* xw, const int32_t* starts, int32_t W, int32_t BC, int32_t N, int32_t T, int64_t P, hipStream_t s);
int cc_window_fuse(const float* const* yw, float* out, const int32_t* starts, const float* coef, int32_t W, int32_t BC, int32_t N, int32_t T,
                   int64_t P, hipStream_t s);

// Tile launchers (tile.hip); entry points and argument checks in core.cpp
int cc_tile_gather(const float* x, float* xt, const int32_t* starts, int32_t T, int64_t planes, int32_t h, int32_t w, int32_t th, int32_t tw,
                   hipStream_t s);
int cc_tile_fuse(const float* const* yt, float* out, const int32_t* starts, const float* coef, int32_t T, int64_t planes, int32_t h, int32_t w,
                 int32_t th, int32_t tw, hipStream_t s);

// Region launchers (region.hip); entry points and argument checks in core.cpp
int cc_region_weights(const uint8_t* masks, float* coef, int32_t K, int32_t T, int32_t H, int32_t W, int32_t F, hipStream_t s);
int cc_region_fuse(const float* const* yr, float* out, const float* coef, int32_t K, int64_t BC, int32_t T, int64_t P, hipStream_t s);

// Automatic-mask launchers (automask.hip); entry points and argument checks in core.cpp
int cc_automask_accumulate(const float* y, float* acc, int32_t B, int32_t C, int64_t P, int32_t first, hipStream_t s);
int cc_automask_binarize(const float* acc, const float* scale, float theta, uint8_t* bin, int32_t B, int64_t P, hipStream_t s);
int cc_automask_vote(const uint8_t* bin, uint8_t* out, int32_t B, int32_t T, int32_t h, int32_t w, int32_t votes, hipStream_t s);
int cc_automask_expand(const uint8_t* lat, uint8_t* px, int64_t N, int32_t h, int32_t w, hipStream_t s);

// Weighted prompts (prompt.hip); entry point and argument checks in core.cpp
int cc_prompt_weight(const float* z, const float* e, const float* w, float* out, int64_t R, int32_t C, hipStream_t s);
int cc_prompt_schedule(const float* c, const int32_t* k0, const int32_t* k1, const float* a, float* out, int32_t N, int32_t L, int32_t C,
                       hipStream_t s);

// Propagation launchers (propagate.hip); entry points and argument checks in core.cpp
int cc_prop_pyramid(const uint8_t* rgb, uint8_t* pyr, int32_t F, int32_t H, int32_t W, hipStream_t s);
int cc_prop_match(const uint8_t* lum, const int32_t* pairs, const int32_t* rank, const int32_t* parent, int32_t* out, int32_t P, int32_t F,
                  int32_t h, int32_t w, int32_t R, hipStream_t s);
int cc_prop_warp(const uint8_t* src, const int32_t* vec, const int32_t* pairs, int32_t col, uint8_t* out, int32_t P, int32_t Fsrc, int32_t H,
                 int32_t W, int32_t C, hipStream_t s);
int cc_prop_blend(const uint8_t* wE, const uint8_t* wY, const uint8_t* lum, const int32_t* pairs, const int32_t* gtab, const uint8_t* rgb,
                  const uint8_t* mask, uint8_t* out, int32_t NF, int32_t F, int32_t H, int32_t W, hipStream_t s);

// Mask-tracking launchers (masktrack.hip); entry points and argument checks in core.cpp
int cc_masktrack_select(const uint8_t* lum, const int32_t* pairs, const int32_t* vec, uint32_t* out, int32_t P, int32_t F, int32_t H, int32_t W,
                        hipStream_t s);
int cc_masktrack_step(const uint32_t* v, const uint32_t* r, const uint8_t* mg, uint8_t* mf, int32_t H, int32_t W, int32_t limit, hipStream_t s);

// Motion-following noise launchers (noisewarp.hip); entry points and argument checks in core.cpp
int cc_noisewarp_track(const int32_t* vec, const int32_t* key, int32_t* trk, int32_t K, int32_t F, int32_t H, int32_t W, int32_t limit,
                       hipStream_t s);
int cc_noisewarp_claim(const int32_t* trk, const int32_t* org, uint32_t* table, int32_t k, int32_t H, int32_t W, hipStream_t s);
int cc_noisewarp_resolve(const int32_t* trk, int32_t* org, const uint32_t* table, int32_t* src, uint32_t* inherited, int32_t k, int32_t H,
                         int32_t W, hipStream_t s);
int cc_noisewarp_check(const int32_t* src, int64_t total, int64_t N, uint32_t* flag, hipStream_t s);
int cc_noise_warp(const float* raw, const int32_t* src, float* out, int32_t B, int32_t C, int64_t N, hipStream_t s);

// Quality-report launchers (quality.hip); entry points and argument checks in core.cpp
int cc_quality_pair(const uint8_t* a, const uint8_t* b, const uint8_t* mask, uint64_t* acc, int64_t N, int32_t H, int32_t W, hipStream_t s);
int cc_quality_warp(const uint8_t* x, const uint8_t* y, const uint32_t* vsel, const int32_t* pairs, const uint8_t* mask, uint64_t* acc, int32_t P,
                    int32_t F, int32_t H, int32_t W, int32_t limit, int32_t sel, hipStream_t s);

// Motion-JPEG launchers (mjpeg.hip); entry points and argument checks in core.cpp
int64_t cc_mjpeg_segment_bytes(int32_t W);
int cc_mjpeg_transform(const uint8_t* frames, const int32_t* tab, int16_t* coef, int32_t N, int32_t H, int32_t W, int32_t quality, hipStream_t s);
int cc_mjpeg_entropy(const int16_t* coef, const int32_t* tab, uint8_t* scratch, int32_t* seg_len, int32_t N, int32_t H, int32_t W, hipStream_t s);
int cc_mjpeg_pack_scan(const int32_t* seg_len, int64_t* seg_off, int32_t* frame_bytes, int32_t N, int32_t H, int32_t W, int32_t hdr_len, hipStream_t s);
int cc_mjpeg_pack(const uint8_t* scratch, const int32_t* seg_len, const int64_t* seg_off, const uint8_t* header, uint8_t* out, int32_t N, int32_t H,
                  int32_t W, int32_t hdr_len, int64_t out_bytes, hipStream_t s);

// JPEG decoding launchers (jpegdec.hip); entry points and argument checks in core.cpp
int64_t cc_jpegdec_plane_bytes(int32_t H, int32_t W, int32_t ncomp, int32_t hs, int32_t vs);
int64_t cc_jpegdec_blocks(int32_t H, int32_t W, int32_t ncomp, int32_t hs, int32_t vs);
int64_t cc_jpegdec_intervals(int32_t H, int32_t W, int32_t ncomp, int32_t hs, int32_t vs, int32_t restart_interval);
int cc_jpegdec_entropy(const uint8_t* data, int64_t data_bytes, const int64_t* intervals, const int32_t* tab, int16_t* coef, int32_t* status,
                       int32_t N, int32_t H, int32_t W, int32_t ncomp, int32_t hs, int32_t vs, int32_t restart_interval, hipStream_t s);
int cc_jpegdec_idct(const int16_t* coef, const int32_t* tab, uint8_t* planes, int32_t N, int32_t H, int32_t W, int32_t ncomp, int32_t hs,
                    int32_t vs, hipStream_t s);
int cc_jpegdec_rgb(const uint8_t* planes, uint8_t* out, int32_t N, int32_t H, int32_t W, int32_t ncomp, int32_t hs, int32_t vs, hipStream_t s);

// GIF launchers (gif.hip); entry points and argument checks in core.cpp
int64_t cc_gif_slot_bytes();
int cc_gif_histogram(const uint8_t* frames, int64_t* moments, int32_t N, int32_t H, int32_t W, hipStream_t s);
int cc_gif_palette(int64_t* moments, uint8_t* cells, uint8_t* palettes, int32_t N, hipStream_t s);
int cc_gif_map(const uint8_t* frames, const uint8_t* cells, uint8_t* indices, int32_t N, int32_t H, int32_t W, hipStream_t s);
int cc_gif_lzw(const uint8_t* indices, uint8_t* slots, int32_t* chunk_bits, int32_t N, int32_t H, int32_t W, int32_t chunk, hipStream_t s);
int cc_gif_pack_scan(const int32_t* chunk_bits, int64_t* chunk_off, int32_t* frame_bytes, int32_t N, int32_t H, int32_t W, int32_t chunk, hipStream_t s);
int cc_gif_pack(const uint8_t* slots, const int32_t* chunk_bits, const int64_t* chunk_off, uint8_t* out, int32_t N, int32_t H, int32_t W, int32_t chunk,
                int64_t out_bytes, hipStream_t s);

// PNG launchers (png.hip); entry points and argument checks in core.cpp
int64_t cc_png_slot_bytes();
int64_t cc_png_chunk_bytes();
int cc_png_filter(const uint8_t* frames, uint8_t* filtered, int32_t N, int32_t H, int32_t W, hipStream_t s);
int cc_png_tokens(const uint8_t* filtered, uint32_t* tokens, int32_t* ntok, uint32_t* hist, int32_t N, int64_t L, hipStream_t s);
int cc_png_codes(const uint32_t* hist, uint32_t* codes, uint32_t* header, int32_t* header_bits, int32_t* chunk_bits, int32_t N, int32_t C, hipStream_t s);
int cc_png_emit(const uint32_t* tokens, const int32_t* ntok, const uint32_t* codes, const uint32_t* header, const int32_t* header_bits, uint8_t* slots,
                int64_t total, hipStream_t s);
int cc_png_pack_scan(const int32_t* chunk_bits, int64_t* chunk_off, int32_t* frame_bytes, int32_t N, int32_t C, hipStream_t s);
int cc_png_pack(const uint8_t* slots, const int32_t* chunk_bits, const int64_t* chunk_off, uint8_t* out, int32_t N, int32_t C, int64_t out_bytes,
                hipStream_t s);
int cc_png_adler(const uint8_t* filtered, uint32_t* partials, uint32_t* adler, int32_t N, int64_t L, hipStream_t s);

// PNG decoding launchers (pngdec.hip); entry points and argument checks in core.cpp
int cc_pngdec_inflate(const uint8_t* data, int64_t data_bytes, const int64_t* streams, uint8_t* filtered, int32_t* status, int32_t N, int32_t H,
                      int32_t W, hipStream_t s);
int cc_pngdec_unfilter(const uint8_t* filtered, uint8_t* rgb, int32_t* status, int32_t N, int32_t H, int32_t W, hipStream_t s);

// GIF decoding launchers (gifdec.hip); entry points and argument checks in core.cpp
int cc_gifdec_codes(const uint8_t* data, int64_t data_bytes, const int64_t* desc, int32_t* parent, int32_t* len, int32_t* off, uint8_t* first,
                    uint8_t* last, int64_t total_codes, int32_t* ncodes, int32_t* status, int32_t N, hipStream_t s);
int cc_gifdec_pixels(const int64_t* desc, const int32_t* parent, const int32_t* len, const int32_t* off, const uint8_t* last, int64_t total_codes,
                     const int32_t* ncodes, uint8_t* planes, int64_t plane_bytes, int32_t N, int64_t max_codes, hipStream_t s);
int cc_gifdec_compose(const uint8_t* data, int64_t data_bytes, const int64_t* desc, const uint8_t* planes, int64_t plane_bytes, uint8_t* canvas,
                      uint8_t* out, int32_t* status, int32_t N, int32_t n_out, int32_t H, int32_t W, hipStream_t s);
