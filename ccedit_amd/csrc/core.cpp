// Error reporting / device info for libccedit_hip.so.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "common.h"

static thread_local char g_err[512] = "";

void cc_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

static thread_local char g_kernel[96] = "";

// Name of the kernel template a GEMM / attention entry point dispatched to (for per-kernel roofline accounting in bench.py)
void cc_note_kernel(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_kernel, sizeof(g_kernel), fmt, ap);
    va_end(ap);
}

extern "C" const char* ccedit_last_kernel(void) { return g_kernel; }

extern "C" int ccedit_abi_version(void) { return CCEDIT_ABI_VERSION; }

extern "C" const char* ccedit_last_error(void) { return g_err; }

extern "C" int ccedit_device_info(char* name, int name_len) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) {
        cc_set_error("hipGetDevice: %s", hipGetErrorString(e));
        return -(int)e;
    }
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, dev);
    if (e != hipSuccess) {
        cc_set_error("hipGetDeviceProperties: %s", hipGetErrorString(e));
        return -(int)e;
    }
    if (name && name_len > 0) {
        strncpy(name, prop.gcnArchName, (size_t)name_len - 1);
        name[name_len - 1] = 0;
    }
    return prop.multiProcessorCount;
}

// ---- dispatch policy (common.h: CcPolicy) ----
static CcPolicy g_policy;
const CcPolicy& cc_policy() { return g_policy; }

namespace {
struct PolicyEntry {
    const char* name;
    int CcPolicy::*field;
};
const PolicyEntry kPolicy[] = {
    {"conv_halo", &CcPolicy::conv_halo},     {"conv_wide", &CcPolicy::conv_wide},     {"g8", &CcPolicy::g8},           {"g8_conv", &CcPolicy::g8_conv},
    {"g8_temporal", &CcPolicy::g8_temporal}, {"g8_split", &CcPolicy::g8_split}, {"g8_mfma16", &CcPolicy::g8_mfma16}, {"lin320", &CcPolicy::lin320},
    {"lin320s", &CcPolicy::lin320s},         {"lin640", &CcPolicy::lin640},   {"temp320", &CcPolicy::temp320},
    {"attn_short", &CcPolicy::attn_short},   {"attn_text", &CcPolicy::attn_text}, {"attn_spatial", &CcPolicy::attn_spatial},
    {"attn_pv16", &CcPolicy::attn_pv16},     {"attn_opt", &CcPolicy::attn_opt},       {"gn_flat", &CcPolicy::gn_flat}, {"gn_apply_flat", &CcPolicy::gn_apply_flat},
    {"f32_split", &CcPolicy::f32_split},
};
}  // namespace

extern "C" int ccedit_policy_set(const char* name, int32_t value) {
    CC_CHECK_ARG(name != nullptr, "ccedit_policy_set: null name");
    for (const PolicyEntry& e : kPolicy)
        if (!strcmp(e.name, name)) {
            g_policy.*(e.field) = value;
            return CCEDIT_OK;
        }
    cc_set_error("ccedit_policy_set: unknown switch '%s'", name);
    return CCEDIT_EINVAL;
}

extern "C" int ccedit_policy_get(const char* name, int32_t* value) {
    CC_CHECK_ARG(name != nullptr && value != nullptr, "ccedit_policy_get: null argument");
    for (const PolicyEntry& e : kPolicy)
        if (!strcmp(e.name, name)) {
            *value = g_policy.*(e.field);
            return CCEDIT_OK;
        }
    cc_set_error("ccedit_policy_get: unknown switch '%s'", name);
    return CCEDIT_EINVAL;
}

// Comma-separated names of the table, in declaration order
extern "C" const char* ccedit_policy_names(void) {
    static char buf[512] = "";
    if (!buf[0]) {
        size_t n = 0;
        for (const PolicyEntry& e : kPolicy) n += (size_t)snprintf(buf + n, sizeof(buf) - n, "%s%s", n ? "," : "", e.name);
    }
    return buf;
}

// ---- pixel I/O (kernels and launchers: pixel.hip).  Everything is checked here, before any HIP call.
static const int64_t kPixelMax = (int64_t)1 << 31;      // element counts the 32-bit tap arithmetic and the rank counters are sized for

extern "C" int ccedit_resize_u8_pil(const void* src, void* dst, void* tmp, const int32_t* ytab, int32_t yk, const int32_t* xtab, int32_t xk,
                                    int32_t N, int32_t Hs, int32_t Ws, int32_t H, int32_t W, int32_t out_f32, void* stream) {
    CC_CHECK_ARG(src && dst && ytab, "ccedit_resize_u8_pil: null pointer (src, dst and ytab are required)");
    CC_CHECK_ARG(N > 0 && Hs > 0 && Ws > 0 && H > 0 && W > 0, "ccedit_resize_u8_pil: sizes must be positive (N=%d, %dx%d -> %dx%d)", N, Hs, Ws, H, W);
    CC_CHECK_ARG(yk >= 1 && yk <= 4096 && (!xtab || (xk >= 1 && xk <= 4096)), "ccedit_resize_u8_pil: tap counts yk=%d xk=%d (1 ... 4096)", yk, xk);
    CC_CHECK_ARG(xtab || Ws == W, "ccedit_resize_u8_pil: xtab may only be null when the width does not change (%d -> %d)", Ws, W);
    CC_CHECK_ARG(!xtab || tmp, "ccedit_resize_u8_pil: the horizontal pass needs tmp (N x Hs x W x 3 bytes)");
    CC_CHECK_ARG((int64_t)N * Hs * (Ws > W ? Ws : W) * 3 < kPixelMax && (int64_t)N * H * W * 3 < kPixelMax,
                 "ccedit_resize_u8_pil: more than 2^31 bytes in one call (N=%d, %dx%d -> %dx%d)", N, Hs, Ws, H, W);
    return cc_pixel_resize_u8((const uint8_t*)src, dst, (uint8_t*)tmp, ytab, yk, xtab, xk, N, Hs, Ws, H, W, out_f32, (hipStream_t)stream);
}

extern "C" int ccedit_resize_f32_bicubic(const float* src, float* dst, const int32_t* ytab, const int32_t* xtab, int64_t planes, int32_t Hs,
                                         int32_t Ws, int32_t H, int32_t W, void* stream) {
    CC_CHECK_ARG(src && dst && ytab && xtab, "ccedit_resize_f32_bicubic: null pointer");
    CC_CHECK_ARG(planes > 0 && Hs > 0 && Ws > 0 && H > 0 && W > 0, "ccedit_resize_f32_bicubic: sizes must be positive (planes=%lld, %dx%d -> %dx%d)",
                 (long long)planes, Hs, Ws, H, W);
    CC_CHECK_ARG(planes < kPixelMax && planes * Hs * Ws < kPixelMax * 4 && planes * H * W < kPixelMax * 4,
                 "ccedit_resize_f32_bicubic: more than 2^33 elements in one call");
    return cc_pixel_resize_f32(src, dst, ytab, xtab, planes, Hs, Ws, H, W, (hipStream_t)stream);
}

extern "C" int ccedit_kth_values(const float* x, int32_t B, int64_t n, const int64_t* ranks, int32_t n_ranks, float* out, void* workspace,
                                 void* stream) {
    CC_CHECK_ARG(x && ranks && out && workspace, "ccedit_kth_values: null pointer");
    CC_CHECK_ARG(B > 0 && B <= 65535 && n > 0 && n < kPixelMax, "ccedit_kth_values: B=%d (1 ... 65535), n=%lld (1 ... 2^31 - 1)", B, (long long)n);
    CC_CHECK_ARG(n_ranks >= 1 && n_ranks <= 4, "ccedit_kth_values: n_ranks=%d (1 ... 4)", n_ranks);
    for (int r = 0; r < n_ranks; ++r)
        CC_CHECK_ARG(ranks[r] >= 1 && ranks[r] <= n, "ccedit_kth_values: rank %lld outside 1 ... n=%lld (1-based, as torch.kthvalue)",
                     (long long)ranks[r], (long long)n);
    return cc_pixel_kth_values(x, B, n, ranks, n_ranks, out, workspace, (hipStream_t)stream);
}

extern "C" int ccedit_minmax_f32(const float* x, int32_t B, int64_t n, float* out, void* stream) {
    CC_CHECK_ARG(x && out, "ccedit_minmax_f32: null pointer");
    CC_CHECK_ARG(B > 0 && B <= 65535 && n > 0, "ccedit_minmax_f32: B=%d (1 ... 65535), n=%lld (> 0)", B, (long long)n);
    return cc_pixel_minmax(x, B, n, out, (hipStream_t)stream);
}

extern "C" int ccedit_depth_hint(const float* depth, float* hint, const float* stats, int32_t stat_stride, int32_t B, int64_t n, int32_t flip,
                                 void* stream) {
    CC_CHECK_ARG(depth && hint && stats, "ccedit_depth_hint: null pointer");
    CC_CHECK_ARG(B > 0 && B <= 65535 && n > 0, "ccedit_depth_hint: B=%d (1 ... 65535), n=%lld (> 0)", B, (long long)n);
    CC_CHECK_ARG(stat_stride == 0 || stat_stride >= 2, "ccedit_depth_hint: stat_stride=%d (0: one (lo, hi) pair for all clips, else >= 2)", stat_stride);
    return cc_pixel_depth_hint(depth, hint, stats, stat_stride, B, n, flip, (hipStream_t)stream);
}

extern "C" int ccedit_frames_to_u8(const float* x, void* out, int32_t B, int64_t P, int32_t mode, int32_t unit_range, void* stream) {
    CC_CHECK_ARG(x && out, "ccedit_frames_to_u8: null pointer");
    CC_CHECK_ARG(B > 0 && B <= 65535 && P > 0, "ccedit_frames_to_u8: B=%d (1 ... 65535), P=%lld (> 0)", B, (long long)P);
    CC_CHECK_ARG(mode == 0 || mode == 1, "ccedit_frames_to_u8: mode=%d (0: truncate 255 v, 1: truncate 255 v + 0.5)", mode);
    return cc_pixel_frames_to_u8(x, (uint8_t*)out, B, P, mode, unit_range, (hipStream_t)stream);
}

// ---- edit masks (kernels and launchers: mask.hip).  Everything is checked here, before any HIP call.
extern "C" int ccedit_mask_resize_nearest(const void* src, void* dst, const int32_t* ytab, const int32_t* xtab, int32_t N, int32_t Hs, int32_t Ws,
                                          int32_t H, int32_t W, void* stream) {
    CC_CHECK_ARG(src && dst && ytab && xtab, "ccedit_mask_resize_nearest: null pointer");
    CC_CHECK_ARG(N > 0 && Hs > 0 && Ws > 0 && H > 0 && W > 0, "ccedit_mask_resize_nearest: sizes must be positive (N=%d, %dx%d -> %dx%d)", N, Hs, Ws,
                 H, W);
    CC_CHECK_ARG((int64_t)N * Hs * Ws < kPixelMax && (int64_t)N * H * W < kPixelMax,
                 "ccedit_mask_resize_nearest: more than 2^31 bytes in one call (N=%d, %dx%d -> %dx%d)", N, Hs, Ws, H, W);
    return cc_mask_resize_nearest((const uint8_t*)src, (uint8_t*)dst, ytab, xtab, N, Hs, Ws, H, W, (hipStream_t)stream);
}

extern "C" int ccedit_mask_latent(const void* mask_px, void* mask_lat, int64_t N, int32_t H, int32_t W, void* stream) {
    CC_CHECK_ARG(mask_px && mask_lat, "ccedit_mask_latent: null pointer");
    CC_CHECK_ARG(N > 0 && H > 0 && W > 0 && H % 8 == 0 && W % 8 == 0, "ccedit_mask_latent: N=%lld frames of %dx%d (positive, H and W multiples of 8)",
                 (long long)N, H, W);
    CC_CHECK_ARG(N < kPixelMax && N * H * W < kPixelMax * 4, "ccedit_mask_latent: more than 2^33 pixels in one call");
    CC_CHECK_ARG(((uintptr_t)mask_px & 7) == 0, "ccedit_mask_latent: the pixel mask must be 8-byte aligned (a row of a cell is one 8-byte load)");
    return cc_mask_latent((const uint8_t*)mask_px, (uint8_t*)mask_lat, N, H, W, (hipStream_t)stream);
}

extern "C" int ccedit_inpaint_blend(const float* x, const float* x0, const float* noise, const void* mask, float* y, int32_t B, int32_t C, int64_t P,
                                    float sigma, float s, void* stream) {
    CC_CHECK_ARG(x && x0 && noise && mask && y, "ccedit_inpaint_blend: null pointer");
    CC_CHECK_ARG(B > 0 && C > 0 && P > 0 && P < kPixelMax * 4 && (int64_t)B * C * P < kPixelMax * 4,
                 "ccedit_inpaint_blend: B=%d C=%d P=%lld (positive, at most 2^33 elements)", B, C, (long long)P);
    CC_CHECK_ARG(s > 0.0f, "ccedit_inpaint_blend: s=%g must be positive (s = sqrt(1 + sigma^2))", (double)s);
    return cc_mask_inpaint_blend(x, x0, noise, (const uint8_t*)mask, y, B, C, P, sigma, s, (hipStream_t)stream);
}

extern "C" int ccedit_mask_composite(const float* result, const float* original, const void* mask_px, float* out, int32_t B, int64_t P, void* stream) {
    CC_CHECK_ARG(result && original && mask_px && out, "ccedit_mask_composite: null pointer");
    CC_CHECK_ARG(B > 0 && P > 0 && P < kPixelMax * 4 && (int64_t)B * 3 * P < kPixelMax * 4,
                 "ccedit_mask_composite: B=%d P=%lld (positive, at most 2^33 elements)", B, (long long)P);
    return cc_mask_composite(result, original, (const uint8_t*)mask_px, out, B, P, (hipStream_t)stream);
}

extern "C" int ccedit_mask_dilate(const void* src, void* tmp, void* dst, int64_t N, int32_t H, int32_t W, int32_t radius, int32_t invert, void* stream) {
    CC_CHECK_ARG(src && dst && (tmp || radius == 0), "ccedit_mask_dilate: null pointer (tmp alone may be null, with radius 0)");
    CC_CHECK_ARG(N > 0 && H > 0 && W > 0 && W % 4 == 0, "ccedit_mask_dilate: N=%lld masks of %dx%d (positive, W a multiple of 4)", (long long)N, H, W);
    CC_CHECK_ARG(N < kPixelMax && N * H * W < kPixelMax * 4, "ccedit_mask_dilate: more than 2^33 pixels in one call");
    CC_CHECK_ARG(radius >= 0 && radius <= 32, "ccedit_mask_dilate: radius=%d (0 ... 32)", radius);
    CC_CHECK_ARG(invert == 0 || invert == 1, "ccedit_mask_dilate: invert=%d (0 or 1)", invert);
    CC_CHECK_ARG((((uintptr_t)src | (uintptr_t)tmp | (uintptr_t)dst) & 3) == 0, "ccedit_mask_dilate: src, tmp and dst must be 4-byte aligned");
    CC_CHECK_ARG(src != dst && tmp != dst && src != tmp, "ccedit_mask_dilate: src, tmp and dst must be different buffers");
    return cc_mask_dilate((const uint8_t*)src, (uint8_t*)tmp, (uint8_t*)dst, N, H, W, radius, invert, (hipStream_t)stream);
}

// ---- graded edit masks (kernels and launchers: softmask.hip; the level re-injection: mask.hip).  Everything is checked here, before any
// HIP call.
extern "C" int ccedit_mask_feather(const void* src, void* tmp16, void* dst, int64_t N, int32_t H, int32_t W, int32_t radius, void* stream) {
    CC_CHECK_ARG(src && tmp16 && dst, "ccedit_mask_feather: null pointer");
    CC_CHECK_ARG(N > 0 && H > 0 && W > 0 && W % 4 == 0, "ccedit_mask_feather: N=%lld maps of %dx%d (positive, W a multiple of 4)", (long long)N, H, W);
    CC_CHECK_ARG(N < kPixelMax && N * H * W < kPixelMax * 4, "ccedit_mask_feather: more than 2^33 pixels in one call");
    CC_CHECK_ARG(radius >= 0 && radius <= 64, "ccedit_mask_feather: radius=%d (0 ... 64)", radius);
    CC_CHECK_ARG((((uintptr_t)src | (uintptr_t)tmp16 | (uintptr_t)dst) & 3) == 0, "ccedit_mask_feather: src, tmp16 and dst must be 4-byte aligned");
    CC_CHECK_ARG(src != dst && tmp16 != dst && src != tmp16, "ccedit_mask_feather: src, tmp16 and dst must be different buffers");
    return cc_mask_feather((const uint8_t*)src, (uint16_t*)tmp16, (uint8_t*)dst, N, H, W, radius, (hipStream_t)stream);
}

extern "C" int ccedit_mask_latent_graded(const void* mask_px, void* strength_lat, int64_t N, int32_t H, int32_t W, void* stream) {
    CC_CHECK_ARG(mask_px && strength_lat, "ccedit_mask_latent_graded: null pointer");
    CC_CHECK_ARG(N > 0 && H > 0 && W > 0 && H % 8 == 0 && W % 8 == 0,
                 "ccedit_mask_latent_graded: N=%lld frames of %dx%d (positive, H and W multiples of 8)", (long long)N, H, W);
    CC_CHECK_ARG(N < kPixelMax && N * H * W < kPixelMax * 4, "ccedit_mask_latent_graded: more than 2^33 pixels in one call");
    CC_CHECK_ARG(((uintptr_t)mask_px & 7) == 0,
                 "ccedit_mask_latent_graded: the strength map must be 8-byte aligned (a row of a cell is one 8-byte load)");
    return cc_mask_latent_graded((const uint8_t*)mask_px, (uint8_t*)strength_lat, N, H, W, (hipStream_t)stream);
}

extern "C" int ccedit_mask_composite_graded(const float* result, const float* original, const void* strength_px, float* out, int32_t B, int64_t P,
                                            void* stream) {
    CC_CHECK_ARG(result && original && strength_px && out, "ccedit_mask_composite_graded: null pointer");
    CC_CHECK_ARG(B > 0 && P > 0 && P < kPixelMax * 4 && (int64_t)B * 3 * P < kPixelMax * 4,
                 "ccedit_mask_composite_graded: B=%d P=%lld (positive, at most 2^33 elements)", B, (long long)P);
    return cc_mask_composite_graded(result, original, (const uint8_t*)strength_px, out, B, P, (hipStream_t)stream);
}

extern "C" int ccedit_inpaint_blend_level(const float* x, const float* x0, const float* noise, const void* strength, float* y, int32_t B, int32_t C,
                                          int64_t P, int32_t thr, float sigma, float s, void* stream) {
    CC_CHECK_ARG(x && x0 && noise && strength && y, "ccedit_inpaint_blend_level: null pointer");
    CC_CHECK_ARG(B > 0 && C > 0 && P > 0 && P < kPixelMax * 4 && (int64_t)B * C * P < kPixelMax * 4,
                 "ccedit_inpaint_blend_level: B=%d C=%d P=%lld (positive, at most 2^33 elements)", B, C, (long long)P);
    CC_CHECK_ARG(thr >= 1 && thr <= 255, "ccedit_inpaint_blend_level: thr=%d (1 ... 255: strength 0 is never free, strength 255 always)", thr);
    CC_CHECK_ARG(s > 0.0f, "ccedit_inpaint_blend_level: s=%g must be positive (s = sqrt(1 + sigma^2))", (double)s);
    return cc_mask_inpaint_blend_level(x, x0, noise, (const uint8_t*)strength, y, B, C, P, thr, sigma, s, (hipStream_t)stream);
}

// ---- windows of a long clip (kernels and launchers: window.hip).  Everything the host can see is checked here, before any HIP call;
// the device tables (starts, coef, the pointer table) are held inside their tensors by the kernels themselves.
static int window_shape_ok(const char* fn, int32_t W, int32_t B, int32_t C, int32_t N, int32_t T, int64_t P) {
    CC_CHECK_ARG(W >= 1 && W <= 4096 && B > 0 && C > 0 && T >= 1 && N >= T && P > 0,
                 "%s: W=%d (1 ... 4096) windows of T=%d frames over N=%d (N >= T >= 1), B=%d C=%d P=%lld (positive)", fn, W, T, N, B, C, (long long)P);
    CC_CHECK_ARG((int64_t)B * C < kPixelMax && P < kPixelMax * 4 && (int64_t)B * C * N * P < kPixelMax * 4 && (int64_t)W * B * C * T * P < kPixelMax * 4,
                 "%s: more than 2^33 elements in one call (W=%d B=%d C=%d N=%d T=%d P=%lld)", fn, W, B, C, N, T, (long long)P);
    return CCEDIT_OK;
}

extern "C" int ccedit_window_gather(const float* x, float* xw, const int32_t* starts, int32_t W, int32_t B, int32_t C, int32_t N, int32_t T,
                                    int64_t P, void* stream) {
    CC_CHECK_ARG(x && xw && starts, "ccedit_window_gather: null pointer");
    if (int rc = window_shape_ok("ccedit_window_gather", W, B, C, N, T, P)) return rc;
    return cc_window_gather(x, xw, starts, W, B * C, N, T, P, (hipStream_t)stream);
}

extern "C" int ccedit_window_fuse(const void* yw, float* out, const int32_t* starts, const float* coef, int32_t W, int32_t B, int32_t C,
                                  int32_t N, int32_t T, int64_t P, void* stream) {
    CC_CHECK_ARG(yw && out && starts && coef, "ccedit_window_fuse: null pointer");
    CC_CHECK_ARG(((uintptr_t)yw & 7) == 0, "ccedit_window_fuse: the table of window pointers must be 8-byte aligned");
    if (int rc = window_shape_ok("ccedit_window_fuse", W, B, C, N, T, P)) return rc;
    return cc_window_fuse((const float* const*)yw, out, starts, coef, W, B * C, N, T, P, (hipStream_t)stream);
}

// ---- tiles of a large frame (kernels and launchers: tile.hip).  Everything the host can see is checked here, before any HIP call;
// the device tables (starts, coef, the pointer table) are held inside their tensors by the kernels themselves.
static int tile_shape_ok(const char* fn, int32_t T, int64_t planes, int32_t h, int32_t w, int32_t th, int32_t tw) {
    CC_CHECK_ARG(T >= 1 && T <= 64 && planes > 0 && th >= 1 && tw >= 1 && h >= th && w >= tw,
                 "%s: T=%d (1 ... 64) tiles of %dx%d over frames of %dx%d (h >= th >= 1, w >= tw >= 1), planes=%lld (positive)", fn, T, th, tw, h, w,
                 (long long)planes);
    CC_CHECK_ARG(planes < kPixelMax && planes * h * w < kPixelMax * 4 && (int64_t)T * planes * th * tw < kPixelMax * 4,
                 "%s: more than 2^33 elements in one call (T=%d planes=%lld %dx%d, tiles of %dx%d)", fn, T, (long long)planes, h, w, th, tw);
    return CCEDIT_OK;
}

extern "C" int ccedit_tile_gather(const float* x, float* xt, const int32_t* starts, int32_t T, int64_t planes, int32_t h, int32_t w, int32_t th,
                                  int32_t tw, void* stream) {
    CC_CHECK_ARG(x && xt && starts, "ccedit_tile_gather: null pointer");
    CC_CHECK_ARG(((uintptr_t)x & 3) == 0 && ((uintptr_t)xt & 3) == 0 && ((uintptr_t)starts & 3) == 0, "ccedit_tile_gather: pointers must be 4-byte aligned");
    if (int rc = tile_shape_ok("ccedit_tile_gather", T, planes, h, w, th, tw)) return rc;
    return cc_tile_gather(x, xt, starts, T, planes, h, w, th, tw, (hipStream_t)stream);
}

extern "C" int ccedit_tile_fuse(const void* yt, float* out, const int32_t* starts, const float* coef, int32_t T, int64_t planes, int32_t h, int32_t w,
                                int32_t th, int32_t tw, void* stream) {
    CC_CHECK_ARG(yt && out && starts && coef, "ccedit_tile_fuse: null pointer");
    CC_CHECK_ARG(((uintptr_t)yt & 7) == 0, "ccedit_tile_fuse: the table of tile pointers must be 8-byte aligned");
    CC_CHECK_ARG(((uintptr_t)out & 3) == 0 && ((uintptr_t)coef & 3) == 0 && ((uintptr_t)starts & 3) == 0, "ccedit_tile_fuse: pointers must be 4-byte aligned");
    if (int rc = tile_shape_ok("ccedit_tile_fuse", T, planes, h, w, th, tw)) return rc;
    return cc_tile_fuse((const float* const*)yt, out, starts, coef, T, planes, h, w, th, tw, (hipStream_t)stream);
}

// ---- region prompts (kernels and launchers: region.hip).  Everything the host can see is checked here, before any HIP call; the
// device tables (coef, the pointer table) cannot take an access outside a tensor: coef is only ever read at the output's own index.
extern "C" int ccedit_region_weights(const void* masks, float* coef, int32_t K, int32_t T, int32_t H, int32_t W, int32_t F, void* stream) {
    CC_CHECK_ARG(masks && coef, "ccedit_region_weights: null pointer");
    CC_CHECK_ARG(K >= 1 && K <= 7, "ccedit_region_weights: K=%d regions (1 ... 7)", K);
    CC_CHECK_ARG(F >= 0 && F <= 8, "ccedit_region_weights: F=%d latent cells of feather (0 ... 8)", F);
    CC_CHECK_ARG(T >= 1 && H >= 8 && W >= 8 && H % 8 == 0 && W % 8 == 0 && H <= 65536 && W <= 65536,
                 "ccedit_region_weights: T=%d frames of %dx%d (T >= 1, H and W multiples of 8, 8 ... 65536)", T, H, W);
    CC_CHECK_ARG((int64_t)K * T * H * W < kPixelMax * 4 && (int64_t)T * ((H + 127) / 128) * ((W + 127) / 128) < kPixelMax,
                 "ccedit_region_weights: more than 2^33 mask bytes or 2^31 tiles in one call (K=%d T=%d %dx%d)", K, T, H, W);
    CC_CHECK_ARG(((uintptr_t)masks & 7) == 0 && ((uintptr_t)coef & 3) == 0, "ccedit_region_weights: masks must be 8-byte and coef 4-byte aligned");
    return cc_region_weights((const uint8_t*)masks, coef, K, T, H, W, F, (hipStream_t)stream);
}

extern "C" int ccedit_region_fuse(const void* yr, float* out, const float* coef, int32_t K, int32_t B, int32_t C, int32_t T, int64_t P,
                                  void* stream) {
    CC_CHECK_ARG(yr && out && coef, "ccedit_region_fuse: null pointer");
    CC_CHECK_ARG(K >= 1 && K <= 7, "ccedit_region_fuse: K=%d regions (1 ... 7; the table holds K + 1 pointers)", K);
    CC_CHECK_ARG(B > 0 && C > 0 && T >= 1 && P > 0, "ccedit_region_fuse: B=%d C=%d T=%d P=%lld (positive)", B, C, T, (long long)P);
    CC_CHECK_ARG((int64_t)B * C < kPixelMax && P < kPixelMax * 4 && (int64_t)B * C * T * P < kPixelMax * 4,
                 "ccedit_region_fuse: more than 2^33 elements in one call (B=%d C=%d T=%d P=%lld)", B, C, T, (long long)P);
    CC_CHECK_ARG(((uintptr_t)yr & 7) == 0, "ccedit_region_fuse: the table of region pointers must be 8-byte aligned");
    CC_CHECK_ARG(((uintptr_t)out & 3) == 0 && ((uintptr_t)coef & 3) == 0, "ccedit_region_fuse: out and coef must be 4-byte aligned");
    return cc_region_fuse((const float* const*)yr, out, coef, K, (int64_t)B * C, T, P, (hipStream_t)stream);
}

// ---- automatic edit masks (kernels and launchers: automask.hip).  Everything the host can see is checked here, before any HIP call;
// no kernel has an index that depends on data: `scale` is read at [b] and only compared against.
extern "C" int ccedit_automask_accumulate(const float* y, float* acc, int32_t B, int32_t C, int64_t P, int32_t first, void* stream) {
    CC_CHECK_ARG(y && acc, "ccedit_automask_accumulate: null pointer");
    CC_CHECK_ARG(B > 0 && P > 0, "ccedit_automask_accumulate: B=%d P=%lld (positive)", B, (long long)P);
    CC_CHECK_ARG(C >= 1 && C <= 16, "ccedit_automask_accumulate: C=%d channels (1 ... 16)", C);
    CC_CHECK_ARG(P < kPixelMax * 4 && 2 * (int64_t)B * C * P < kPixelMax * 4,
                 "ccedit_automask_accumulate: more than 2^33 elements in one call (B=%d C=%d P=%lld)", B, C, (long long)P);
    CC_CHECK_ARG(first == 0 || first == 1, "ccedit_automask_accumulate: first=%d (1: store, 0: add)", first);
    CC_CHECK_ARG(((uintptr_t)y & 3) == 0 && ((uintptr_t)acc & 3) == 0, "ccedit_automask_accumulate: y and acc must be 4-byte aligned");
    return cc_automask_accumulate(y, acc, B, C, P, first, (hipStream_t)stream);
}

extern "C" int ccedit_automask_binarize(const float* acc, const float* scale, float theta, void* bin, int32_t B, int64_t P, void* stream) {
    CC_CHECK_ARG(acc && scale && bin, "ccedit_automask_binarize: null pointer");
    CC_CHECK_ARG(B > 0 && P > 0 && P < kPixelMax * 4 && (int64_t)B * P < kPixelMax * 4,
                 "ccedit_automask_binarize: B=%d P=%lld (positive, at most 2^33 elements)", B, (long long)P);
    CC_CHECK_ARG(theta >= 0.0f && theta <= 3.0e38f, "ccedit_automask_binarize: theta=%g (finite, not negative)", (double)theta);
    CC_CHECK_ARG(((uintptr_t)acc & 3) == 0 && ((uintptr_t)scale & 3) == 0, "ccedit_automask_binarize: acc and scale must be 4-byte aligned");
    return cc_automask_binarize(acc, scale, theta, (uint8_t*)bin, B, P, (hipStream_t)stream);
}

extern "C" int ccedit_automask_vote(const void* bin, void* out, int32_t B, int32_t T, int32_t h, int32_t w, int32_t votes, void* stream) {
    CC_CHECK_ARG(bin && out, "ccedit_automask_vote: null pointer");
    CC_CHECK_ARG(B > 0 && T >= 1 && h >= 1 && w >= 1, "ccedit_automask_vote: B=%d clips of T=%d frames of %dx%d cells (positive)", B, T, h, w);
    CC_CHECK_ARG((int64_t)B * T * h * w < kPixelMax, "ccedit_automask_vote: more than 2^31 cells in one call (B=%d T=%d %dx%d)", B, T, h, w);
    CC_CHECK_ARG(votes >= 1 && votes <= 27, "ccedit_automask_vote: votes=%d of the 27 neighbours (1 ... 27)", votes);
    {
        const int64_t n = (int64_t)B * T * h * w;
        const uintptr_t a = (uintptr_t)bin, b = (uintptr_t)out;
        CC_CHECK_ARG(a + (uintptr_t)n <= b || b + (uintptr_t)n <= a, "ccedit_automask_vote: out must not alias bin (a cell reads its 26 neighbours)");
    }
    return cc_automask_vote((const uint8_t*)bin, (uint8_t*)out, B, T, h, w, votes, (hipStream_t)stream);
}

extern "C" int ccedit_automask_expand(const void* lat, void* px, int64_t N, int32_t h, int32_t w, void* stream) {
    CC_CHECK_ARG(lat && px, "ccedit_automask_expand: null pointer");
    CC_CHECK_ARG(N > 0 && h >= 1 && w >= 1, "ccedit_automask_expand: N=%lld masks of %dx%d cells (positive)", (long long)N, h, w);
    CC_CHECK_ARG(N < kPixelMax && N * 64 * h * w < kPixelMax * 4, "ccedit_automask_expand: more than 2^33 pixels in one call");
    CC_CHECK_ARG(((uintptr_t)px & 7) == 0, "ccedit_automask_expand: the pixel mask must be 8-byte aligned (a row of a cell is one 8-byte store)");
    return cc_automask_expand((const uint8_t*)lat, (uint8_t*)px, N, h, w, (hipStream_t)stream);
}

// ---- weighted prompts (kernel and launcher: prompt.hip).  Everything the host can see is checked here, before any HIP call; the kernel
// reads e at (row mod 77) and everything else at the output's own index.
extern "C" int ccedit_prompt_weight(const float* z, const float* e, const float* w, float* out, int32_t B, int32_t L, int32_t C, void* stream) {
    CC_CHECK_ARG(z && e && w && out, "ccedit_prompt_weight: null pointer");
    CC_CHECK_ARG(B > 0 && C > 0 && L > 0 && L % 77 == 0, "ccedit_prompt_weight: B=%d L=%d C=%d (positive, L a multiple of 77: whole CLIP chunks)", B, L,
                 C);
    CC_CHECK_ARG((int64_t)B * L * C < kPixelMax * 4, "ccedit_prompt_weight: more than 2^33 elements in one call (B=%d L=%d C=%d)", B, L, C);
    CC_CHECK_ARG(((uintptr_t)z & 3) == 0 && ((uintptr_t)e & 3) == 0 && ((uintptr_t)w & 3) == 0 && ((uintptr_t)out & 3) == 0,
                 "ccedit_prompt_weight: z, e, w and out must be 4-byte aligned");
    return cc_prompt_weight(z, e, w, out, (int64_t)B * L, C, (hipStream_t)stream);
}

// ---- prompt schedules (kernel and launcher: prompt.hip).  k0, k1 and a are HOST tables: every index is checked here, and the launcher
// passes the checked values to the kernel by value, so a bad index is this status and never an address.
extern "C" int ccedit_prompt_schedule(const float* c, const int32_t* k0, const int32_t* k1, const float* a, float* out, int32_t P, int32_t N,
                                      int32_t L, int32_t C, void* stream) {
    CC_CHECK_ARG(c && k0 && k1 && a && out, "ccedit_prompt_schedule: null pointer");
    CC_CHECK_ARG(P > 0 && N > 0 && L > 0 && C > 0, "ccedit_prompt_schedule: P=%d N=%d L=%d C=%d (positive)", P, N, L, C);
    CC_CHECK_ARG((int64_t)P * L * C < kPixelMax * 4 && (int64_t)N * L * C < kPixelMax * 4,
                 "ccedit_prompt_schedule: more than 2^33 elements in one call (P=%d N=%d L=%d C=%d)", P, N, L, C);
    CC_CHECK_ARG(((uintptr_t)c & 3) == 0 && ((uintptr_t)out & 3) == 0, "ccedit_prompt_schedule: c and out must be 4-byte aligned");
    for (int32_t f = 0; f < N; ++f) {
        CC_CHECK_ARG(k0[f] >= 0 && k0[f] < P && k1[f] >= 0 && k1[f] < P, "ccedit_prompt_schedule: frame %d: k0=%d k1=%d outside the %d prompts", f,
                     k0[f], k1[f], P);
        CC_CHECK_ARG(a[f] >= 0.0f && a[f] <= 1.0f, "ccedit_prompt_schedule: frame %d: a=%g (0 ... 1)", f, (double)a[f]);
    }
    {
        const uintptr_t cb = (uintptr_t)c, ce = cb + (uintptr_t)((int64_t)P * L * C * 4), ob = (uintptr_t)out, oe = ob + (uintptr_t)((int64_t)N * L * C * 4);
        CC_CHECK_ARG(ce <= ob || oe <= cb, "ccedit_prompt_schedule: out must not alias c (a frame reads prompts other frames' rows overlap)");
    }
    return cc_prompt_schedule(c, k0, k1, a, out, N, L, C, (hipStream_t)stream);
}

// ---- propagation of edited keyframes to every source frame (kernels and launchers: propagate.hip).  Everything the host can see is
// checked here, before any HIP call; the device tables (pairs, rank, g, the block vectors) are held in range by the kernels themselves.
static int prop_shape_ok(const char* fn, int32_t P, int32_t F, int32_t H, int32_t W) {
    CC_CHECK_ARG(P >= 1 && P <= 65534 && F >= 1 && F <= 65535, "%s: P=%d pairs (1 ... 65534) over F=%d frames (1 ... 65535)", fn, P, F);
    CC_CHECK_ARG(H >= 64 && W >= 64 && H % 64 == 0 && W % 64 == 0 && H <= 8192 && W <= 8192,
                 "%s: frames of %dx%d (H and W multiples of 64, 64 ... 8192: four pyramid levels of 8 x 8 blocks)", fn, H, W);
    CC_CHECK_ARG((int64_t)F * H * W * 3 < kPixelMax * 4 && (int64_t)P * H * W * 3 < kPixelMax * 4, "%s: more than 2^33 bytes in one call (P=%d F=%d %dx%d)",
                 fn, P, F, H, W);
    return CCEDIT_OK;
}

extern "C" int ccedit_prop_pyramid(const void* rgb, void* pyr, int32_t F, int32_t H, int32_t W, void* stream) {
    CC_CHECK_ARG(rgb && pyr, "ccedit_prop_pyramid: null pointer");
    if (int rc = prop_shape_ok("ccedit_prop_pyramid", 1, F, H, W)) return rc;
    CC_CHECK_ARG(((uintptr_t)rgb & 3) == 0 && ((uintptr_t)pyr & 7) == 0, "ccedit_prop_pyramid: rgb must be 4-byte and pyr 8-byte aligned");
    return cc_prop_pyramid((const uint8_t*)rgb, (uint8_t*)pyr, F, H, W, (hipStream_t)stream);
}

extern "C" int ccedit_prop_match(const void* pyr, const int32_t* pairs, const int32_t* rank, const int32_t* vec_parent, int32_t* vec_out, int32_t P,
                                 int32_t F, int32_t H, int32_t W, int32_t level, int32_t radius, void* stream) {
    CC_CHECK_ARG(pyr && pairs && rank && vec_out, "ccedit_prop_match: null pointer (vec_parent alone may be null: prediction zero)");
    if (int rc = prop_shape_ok("ccedit_prop_match", P, F, H, W)) return rc;
    CC_CHECK_ARG(level >= 0 && level <= 3, "ccedit_prop_match: level=%d (0 ... 3)", level);
    CC_CHECK_ARG(radius >= 1 && radius <= 4, "ccedit_prop_match: radius=%d (1 ... 4)", radius);
    CC_CHECK_ARG(!vec_parent || level <= 2, "ccedit_prop_match: level 3 is the coarsest, it has no parent vectors");
    int64_t off = 0;
    for (int l = 0; l < level; ++l) off += (int64_t)F * (H >> l) * (W >> l);
    return cc_prop_match((const uint8_t*)pyr + off, pairs, rank, vec_parent, vec_out, P, F, H >> level, W >> level, radius, (hipStream_t)stream);
}

extern "C" int ccedit_prop_warp(const void* src, const int32_t* vec, const int32_t* pairs, int32_t col, void* out, int32_t P, int32_t Fsrc, int32_t H,
                                int32_t W, int32_t C, void* stream) {
    CC_CHECK_ARG(src && vec && pairs && out, "ccedit_prop_warp: null pointer");
    if (int rc = prop_shape_ok("ccedit_prop_warp", P, Fsrc, H, W)) return rc;
    CC_CHECK_ARG(C == 1 || C == 3, "ccedit_prop_warp: C=%d channels (1: luma, 3: RGB)", C);
    CC_CHECK_ARG(col == 1 || col == 2, "ccedit_prop_warp: col=%d (the column of a pair row that names the source frame: 1 or 2)", col);
    CC_CHECK_ARG(((uintptr_t)out & 3) == 0, "ccedit_prop_warp: out must be 4-byte aligned");
    return cc_prop_warp((const uint8_t*)src, vec, pairs, col, (uint8_t*)out, P, Fsrc, H, W, C, (hipStream_t)stream);
}

extern "C" int ccedit_prop_blend(const void* warped_rgb, const void* warped_luma, const void* pyr, const int32_t* pairs, const int32_t* gtab,
                                 const void* rgb, const void* mask, void* out, int32_t NF, int32_t F, int32_t H, int32_t W, void* stream) {
    CC_CHECK_ARG(warped_rgb && warped_luma && pyr && pairs && gtab && out, "ccedit_prop_blend: null pointer");
    CC_CHECK_ARG((rgb == nullptr) == (mask == nullptr), "ccedit_prop_blend: rgb and mask come together (the source is put back where the mask is clear)");
    CC_CHECK_ARG(NF >= 1 && NF <= 32767, "ccedit_prop_blend: NF=%d in-between frames (1 ... 32767)", NF);
    if (int rc = prop_shape_ok("ccedit_prop_blend", 2 * NF, F, H, W)) return rc;
    CC_CHECK_ARG((((uintptr_t)warped_rgb | (uintptr_t)out | (uintptr_t)rgb | (uintptr_t)mask) & 3) == 0,
                 "ccedit_prop_blend: warped_rgb, out, rgb and mask must be 4-byte aligned");
    return cc_prop_blend((const uint8_t*)warped_rgb, (const uint8_t*)warped_luma, (const uint8_t*)pyr, pairs, gtab, (const uint8_t*)rgb,
                         (const uint8_t*)mask, (uint8_t*)out, NF, F, H, W, (hipStream_t)stream);
}

// ---- mask tracking (kernels and launchers: masktrack.hip).  The pair list and the block vectors are device data, held in range by
// the kernel; the per-pixel vectors of a step are any int16 pairs (the looked-up position is clamped into the frame).
extern "C" int ccedit_masktrack_select(const void* pyr, const int32_t* pairs, const int32_t* vec, void* vsel, int32_t P, int32_t F, int32_t H,
                                       int32_t W, void* stream) {
    CC_CHECK_ARG(pyr && pairs && vec && vsel, "ccedit_masktrack_select: null pointer");
    if (int rc = prop_shape_ok("ccedit_masktrack_select", P, F, H, W)) return rc;
    CC_CHECK_ARG(((uintptr_t)vsel & 3) == 0, "ccedit_masktrack_select: vsel must be 4-byte aligned");
    return cc_masktrack_select((const uint8_t*)pyr, pairs, vec, (uint32_t*)vsel, P, F, H, W, (hipStream_t)stream);
}

extern "C" int ccedit_masktrack_step(const void* v, const void* r, const void* mask_g, void* mask_f, int32_t H, int32_t W, int32_t limit,
                                     void* stream) {
    CC_CHECK_ARG(v && r && mask_g && mask_f, "ccedit_masktrack_step: null pointer");
    if (int rc = prop_shape_ok("ccedit_masktrack_step", 1, 1, H, W)) return rc;
    CC_CHECK_ARG(limit >= 0, "ccedit_masktrack_step: limit=%d (not negative)", limit);
    CC_CHECK_ARG(((uintptr_t)v & 15) == 0 && (((uintptr_t)r | (uintptr_t)mask_f) & 3) == 0,
                 "ccedit_masktrack_step: v must be 16-byte, r and mask_f 4-byte aligned");
    CC_CHECK_ARG(mask_g != mask_f, "ccedit_masktrack_step: mask_f is gathered from mask_g: two buffers");
    return cc_masktrack_step((const uint32_t*)v, (const uint32_t*)r, (const uint8_t*)mask_g, (uint8_t*)mask_f, H, W, limit, (hipStream_t)stream);
}

// ---- motion-following noise (kernels and launchers: noisewarp.hip).  Everything the host can see is checked here, before any HIP call;
// the keyframe numbers, the block vectors, the tracked positions, the origins and the index maps are device data, held in range by
// the kernels.  A clip of K keyframes with h w cells each must keep K h w below 2^31: the index map is int32 (and the claims, which
// reach K h w, stay inside 32 bits).
static int noisewarp_shape_ok(const char* fn, int32_t K, int32_t H, int32_t W) {
    CC_CHECK_ARG(K >= 1 && K <= 65535, "%s: K=%d keyframes (1 ... 65535)", fn, K);
    CC_CHECK_ARG(H >= 64 && W >= 64 && H % 64 == 0 && W % 64 == 0 && H <= 8192 && W <= 8192,
                 "%s: frames of %dx%d (H and W multiples of 64, 64 ... 8192: the matcher's four pyramid levels of 8 x 8 blocks)", fn, H, W);
    CC_CHECK_ARG((int64_t)K * (H / 8) * (W / 8) < kPixelMax, "%s: K=%d keyframes of %dx%d cells are 2^31 samples or more: the index map is int32", fn, K,
                 H / 8, W / 8);
    return CCEDIT_OK;
}

extern "C" int ccedit_noisewarp_track(const int32_t* vec, const int32_t* key, int32_t* track, int32_t K, int32_t F, int32_t H, int32_t W,
                                      int32_t limit, void* stream) {
    CC_CHECK_ARG(vec && key && track, "ccedit_noisewarp_track: null pointer");
    if (int rc = noisewarp_shape_ok("ccedit_noisewarp_track", K, H, W)) return rc;
    CC_CHECK_ARG(K >= 2 && F >= 2 && F <= 32767 && K <= F, "ccedit_noisewarp_track: K=%d keyframes among F=%d frames (2 <= K <= F <= 32767)", K, F);
    CC_CHECK_ARG(limit >= 0, "ccedit_noisewarp_track: limit=%d (not negative)", limit);
    CC_CHECK_ARG((int64_t)2 * (F - 1) * (H / 8) * (W / 8) * 2 < kPixelMax, "ccedit_noisewarp_track: F=%d frames of %dx%d: 2^31 vector components or more", F, H, W);
    return cc_noisewarp_track(vec, key, track, K, F, H, W, limit, (hipStream_t)stream);
}

extern "C" int ccedit_noisewarp_claim(const int32_t* track, const int32_t* org, void* table, int32_t k, int32_t K, int32_t H, int32_t W,
                                      void* stream) {
    CC_CHECK_ARG(track && org && table, "ccedit_noisewarp_claim: null pointer");
    if (int rc = noisewarp_shape_ok("ccedit_noisewarp_claim", K, H, W)) return rc;
    CC_CHECK_ARG(k >= 1 && k < K, "ccedit_noisewarp_claim: k=%d (1 ... K - 1 = %d: keyframe 0 inherits nothing)", k, K - 1);
    CC_CHECK_ARG(((uintptr_t)table & 3) == 0, "ccedit_noisewarp_claim: table must be 4-byte aligned");
    return cc_noisewarp_claim(track, org, (uint32_t*)table, k, H, W, (hipStream_t)stream);
}

extern "C" int ccedit_noisewarp_resolve(const int32_t* track, int32_t* org, const void* table, int32_t* src, void* inherited, int32_t k,
                                        int32_t K, int32_t H, int32_t W, void* stream) {
    CC_CHECK_ARG(track && org && table && src && inherited, "ccedit_noisewarp_resolve: null pointer");
    if (int rc = noisewarp_shape_ok("ccedit_noisewarp_resolve", K, H, W)) return rc;
    CC_CHECK_ARG(k >= 0 && k < K, "ccedit_noisewarp_resolve: k=%d (0 ... K - 1 = %d)", k, K - 1);
    CC_CHECK_ARG((((uintptr_t)table | (uintptr_t)inherited) & 3) == 0, "ccedit_noisewarp_resolve: table and inherited must be 4-byte aligned");
    return cc_noisewarp_resolve(track, org, (const uint32_t*)table, src, (uint32_t*)inherited, k, H, W, (hipStream_t)stream);
}

extern "C" int ccedit_noisewarp_check(const int32_t* src, int64_t maps, int64_t N, void* flag, void* stream) {
    CC_CHECK_ARG(src && flag, "ccedit_noisewarp_check: null pointer");
    CC_CHECK_ARG(maps >= 1 && N >= 1 && N < kPixelMax && maps * N < kPixelMax * 4, "ccedit_noisewarp_check: %lld maps of N=%lld indices (N below 2^31)",
                 (long long)maps, (long long)N);
    CC_CHECK_ARG((((uintptr_t)src | (uintptr_t)flag) & 3) == 0, "ccedit_noisewarp_check: src and flag must be 4-byte aligned");
    return cc_noisewarp_check(src, maps * N, N, (uint32_t*)flag, (hipStream_t)stream);
}

extern "C" int ccedit_noise_warp(const float* raw, const int32_t* src, float* out, int32_t B, int32_t C, int64_t N, void* stream) {
    CC_CHECK_ARG(raw && src && out, "ccedit_noise_warp: null pointer");
    CC_CHECK_ARG(B >= 1 && C >= 1 && N >= 1 && N < kPixelMax, "ccedit_noise_warp: B=%d C=%d N=%lld (positive, N below 2^31: the map is int32)", B, C,
                 (long long)N);
    CC_CHECK_ARG((int64_t)B * C < kPixelMax && (int64_t)B * C * N < kPixelMax * 4, "ccedit_noise_warp: more than 2^33 samples in one call");
    CC_CHECK_ARG((((uintptr_t)raw | (uintptr_t)src | (uintptr_t)out) & 3) == 0, "ccedit_noise_warp: raw, src and out must be 4-byte aligned");
    CC_CHECK_ARG(raw != out, "ccedit_noise_warp: out is gathered from raw: two buffers");
    return cc_noise_warp(raw, src, out, B, C, N, (hipStream_t)stream);
}

// ---- quality report (kernels and launchers: quality.hip).  Everything the host can see is checked here, before any HIP call; the pair
// list and the per-pixel vectors are device data, held in range by the kernel (frame numbers clamped into the clip, positions into
// the frame).  Both functions zero their accumulators themselves, on the stream.
extern "C" int ccedit_quality_pair(const void* a, const void* b, const void* mask, void* acc, int64_t N, int32_t H, int32_t W, void* stream) {
    CC_CHECK_ARG(a && b && acc, "ccedit_quality_pair: null pointer (mask alone may be null: every pixel is kept)");
    CC_CHECK_ARG(N >= 1 && N <= 65535, "ccedit_quality_pair: N=%lld frames (1 ... 65535)", (long long)N);
    CC_CHECK_ARG(H >= 8 && W >= 8 && H % 4 == 0 && W % 4 == 0 && H <= 16384 && W <= 16384,
                 "ccedit_quality_pair: frames of %dx%d (H and W multiples of 4, 8 ... 16384: 8 x 8 windows at stride 4)", H, W);
    CC_CHECK_ARG(N * H * W * 3 < kPixelMax * 4, "ccedit_quality_pair: more than 2^33 bytes in one call (N=%lld %dx%d)", (long long)N, H, W);
    CC_CHECK_ARG((((uintptr_t)a | (uintptr_t)b | (uintptr_t)mask) & 3) == 0 && ((uintptr_t)acc & 7) == 0,
                 "ccedit_quality_pair: a, b and mask must be 4-byte, acc 8-byte aligned");
    return cc_quality_pair((const uint8_t*)a, (const uint8_t*)b, (const uint8_t*)mask, (uint64_t*)acc, N, H, W, (hipStream_t)stream);
}

extern "C" int ccedit_quality_warp(const void* x, const void* y, const void* vsel, const int32_t* pairs, const void* mask, void* acc, int32_t P,
                                   int32_t F, int32_t H, int32_t W, int32_t limit, int32_t sel, void* stream) {
    CC_CHECK_ARG(x && vsel && pairs && acc, "ccedit_quality_warp: null pointer (y and, with sel = 0, mask may be null)");
    CC_CHECK_ARG(P >= 1 && P <= 32767, "ccedit_quality_warp: P=%d measurements (1 ... 32767: two pair rows each)", P);
    if (int rc = prop_shape_ok("ccedit_quality_warp", 2 * P, F, H, W)) return rc;
    CC_CHECK_ARG(limit >= 0, "ccedit_quality_warp: limit=%d (not negative)", limit);
    CC_CHECK_ARG(sel >= 0 && sel <= 2, "ccedit_quality_warp: sel=%d (0: all pixels, 1: mask >= 128, 2: mask < 128)", sel);
    CC_CHECK_ARG(sel == 0 || mask, "ccedit_quality_warp: sel=%d chooses pixels by the mask: give one", sel);
    CC_CHECK_ARG(((uintptr_t)vsel & 15) == 0 && (((uintptr_t)x | (uintptr_t)y | (uintptr_t)mask) & 3) == 0 && ((uintptr_t)acc & 7) == 0,
                 "ccedit_quality_warp: vsel must be 16-byte, x, y and mask 4-byte, acc 8-byte aligned");
    return cc_quality_warp((const uint8_t*)x, (const uint8_t*)y, (const uint32_t*)vsel, pairs, (const uint8_t*)mask, (uint64_t*)acc, P, F, H, W,
                           limit, sel, (hipStream_t)stream);
}

// ---- Motion-JPEG (kernels and launchers: mjpeg.hip).  Everything the host can see is checked here, before any HIP call; the device
// tables (constants, segment lengths and offsets) are held in range by the kernels themselves.
static int mjpeg_shape_ok(const char* fn, int32_t N, int32_t H, int32_t W) {
    CC_CHECK_ARG(N >= 1, "%s: N=%d frames (N >= 1)", fn, N);
    CC_CHECK_ARG(H >= 16 && W >= 16 && H % 16 == 0 && W % 16 == 0 && H <= 65520 && W <= 65520,
                 "%s: frames of %dx%d (H and W multiples of 16, 16 ... 65520: 4:2:0 MCUs)", fn, H, W);
    CC_CHECK_ARG((int64_t)N * (H / 16) * ((W / 16 + 3) / 4) < kPixelMax && (int64_t)N * H * W * 3 < kPixelMax * 4,
                 "%s: N=%d frames of %dx%d are more than one call takes (2^33 bytes, 2^31 strips of four MCUs)", fn, N, H, W);
    return CCEDIT_OK;
}

extern "C" int64_t ccedit_mjpeg_segment_bytes(int32_t W) {
    if (W < 16 || W % 16 != 0 || W > 65520) {
        cc_set_error("ccedit_mjpeg_segment_bytes: W=%d (a multiple of 16, 16 ... 65520)", W);
        return CCEDIT_EINVAL;
    }
    return cc_mjpeg_segment_bytes(W);
}

extern "C" int ccedit_mjpeg_transform(const void* frames, const int32_t* tables, void* coef, int32_t N, int32_t H, int32_t W, int32_t quality,
                                      void* stream) {
    CC_CHECK_ARG(frames && tables && coef, "ccedit_mjpeg_transform: null pointer (frames, tables and coef are required)");
    if (int rc = mjpeg_shape_ok("ccedit_mjpeg_transform", N, H, W)) return rc;
    CC_CHECK_ARG(quality >= 1 && quality <= 100, "ccedit_mjpeg_transform: quality=%d (1 ... 100)", quality);
    CC_CHECK_ARG((((uintptr_t)frames | (uintptr_t)coef) & 15) == 0 && ((uintptr_t)tables & 3) == 0,
                 "ccedit_mjpeg_transform: frames and coef must be 16-byte aligned, tables 4-byte");
    return cc_mjpeg_transform((const uint8_t*)frames, tables, (int16_t*)coef, N, H, W, quality, (hipStream_t)stream);
}

extern "C" int ccedit_mjpeg_entropy(const void* coef, const int32_t* tables, void* segments, int32_t* seg_len, int32_t N, int32_t H, int32_t W,
                                    void* stream) {
    CC_CHECK_ARG(coef && tables && segments && seg_len, "ccedit_mjpeg_entropy: null pointer");
    if (int rc = mjpeg_shape_ok("ccedit_mjpeg_entropy", N, H, W)) return rc;
    CC_CHECK_ARG(((uintptr_t)coef & 15) == 0 && (((uintptr_t)tables | (uintptr_t)seg_len) & 3) == 0,
                 "ccedit_mjpeg_entropy: coef must be 16-byte aligned, tables and seg_len 4-byte");
    return cc_mjpeg_entropy((const int16_t*)coef, tables, (uint8_t*)segments, seg_len, N, H, W, (hipStream_t)stream);
}

extern "C" int ccedit_mjpeg_pack_scan(const int32_t* seg_len, int64_t* seg_off, int32_t* frame_bytes, int32_t N, int32_t H, int32_t W,
                                      int32_t hdr_len, void* stream) {
    CC_CHECK_ARG(seg_len && seg_off && frame_bytes, "ccedit_mjpeg_pack_scan: null pointer");
    if (int rc = mjpeg_shape_ok("ccedit_mjpeg_pack_scan", N, H, W)) return rc;
    CC_CHECK_ARG(hdr_len >= 2 && hdr_len <= 65536, "ccedit_mjpeg_pack_scan: hdr_len=%d bytes of frame header (2 ... 65536)", hdr_len);
    CC_CHECK_ARG((((uintptr_t)seg_len | (uintptr_t)frame_bytes) & 3) == 0 && ((uintptr_t)seg_off & 7) == 0,
                 "ccedit_mjpeg_pack_scan: seg_len and frame_bytes must be 4-byte aligned, seg_off 8-byte");
    return cc_mjpeg_pack_scan(seg_len, seg_off, frame_bytes, N, H, W, hdr_len, (hipStream_t)stream);
}

extern "C" int ccedit_mjpeg_pack(const void* segments, const int32_t* seg_len, const int64_t* seg_off, const void* header, void* out, int32_t N,
                                 int32_t H, int32_t W, int32_t hdr_len, int64_t out_bytes, void* stream) {
    CC_CHECK_ARG(segments && seg_len && seg_off && header && out, "ccedit_mjpeg_pack: null pointer");
    if (int rc = mjpeg_shape_ok("ccedit_mjpeg_pack", N, H, W)) return rc;
    CC_CHECK_ARG(hdr_len >= 2 && hdr_len <= 65536, "ccedit_mjpeg_pack: hdr_len=%d bytes of frame header (2 ... 65536)", hdr_len);
    CC_CHECK_ARG(out_bytes >= (int64_t)N * (hdr_len + 2 * (int64_t)(H / 16)), "ccedit_mjpeg_pack: out_bytes=%lld is less than the headers and markers "
                 "of N=%d frames take", (long long)out_bytes, N);
    CC_CHECK_ARG(((uintptr_t)seg_len & 3) == 0 && ((uintptr_t)seg_off & 7) == 0, "ccedit_mjpeg_pack: seg_len must be 4-byte aligned, seg_off 8-byte");
    return cc_mjpeg_pack((const uint8_t*)segments, seg_len, seg_off, (const uint8_t*)header, (uint8_t*)out, N, H, W, hdr_len, out_bytes,
                         (hipStream_t)stream);
}

// ---- JPEG decoding (kernels and launchers: jpegdec.hip).  Geometry and everything else the host can see is checked here, before any HIP
// call; interval offsets and tables are device data, held in range by the kernels themselves.
static int jpegdec_geom_ok(const char* fn, int32_t H, int32_t W, int32_t ncomp, int32_t hs, int32_t vs) {
    CC_CHECK_ARG(H >= 1 && W >= 1 && H <= 65520 && W <= 65520, "%s: frames of %dx%d (H and W 1 ... 65520)", fn, H, W);
    CC_CHECK_ARG(ncomp == 1 || ncomp == 3, "%s: ncomp=%d (1 greyscale, 3 YCbCr)", fn, ncomp);
    CC_CHECK_ARG(ncomp == 1 || (hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2),
                 "%s: luma sampling %dx%d (1x1, 2x1 or 2x2: 4:4:4, 4:2:2, 4:2:0)", fn, hs, vs);
    return CCEDIT_OK;
}

static int jpegdec_shape_ok(const char* fn, int32_t N, int32_t H, int32_t W, int32_t ncomp, int32_t hs, int32_t vs) {
    CC_CHECK_ARG(N >= 1, "%s: N=%d frames (N >= 1)", fn, N);
    if (int rc = jpegdec_geom_ok(fn, H, W, ncomp, hs, vs)) return rc;
    CC_CHECK_ARG((double)N * (double)cc_jpegdec_plane_bytes(H, W, ncomp, hs, vs) < (double)(kPixelMax * 4) &&
                     (double)N * (double)cc_jpegdec_blocks(H, W, ncomp, hs, vs) < (double)kPixelMax,
                 "%s: N=%d frames of %dx%d are more than one call takes (2^33 bytes of planes, 2^31 blocks)", fn, N, H, W);
    CC_CHECK_ARG((double)N * H * W < (double)kPixelMax,          // one thread per pixel: a launch holds fewer than 2^32 threads
                 "%s: N=%d frames of %dx%d are more than one call takes (2^31 pixels)", fn, N, H, W);
    return CCEDIT_OK;
}

extern "C" int64_t ccedit_jpegdec_plane_bytes(int32_t H, int32_t W, int32_t ncomp, int32_t hs, int32_t vs) {
    if (jpegdec_geom_ok("ccedit_jpegdec_plane_bytes", H, W, ncomp, hs, vs)) return CCEDIT_EINVAL;
    return cc_jpegdec_plane_bytes(H, W, ncomp, hs, vs);
}

extern "C" int ccedit_jpegdec_entropy(const void* data, int64_t data_bytes, const int64_t* intervals, const int32_t* tables, void* coef,
                                      int32_t* status, int32_t N, int32_t H, int32_t W, int32_t ncomp, int32_t hs, int32_t vs,
                                      int32_t restart_interval, void* stream) {
    CC_CHECK_ARG(data && intervals && tables && coef && status, "ccedit_jpegdec_entropy: null pointer");
    if (int rc = jpegdec_shape_ok("ccedit_jpegdec_entropy", N, H, W, ncomp, hs, vs)) return rc;
    CC_CHECK_ARG(data_bytes >= 1 && data_bytes < kPixelMax * 4, "ccedit_jpegdec_entropy: data_bytes=%lld (1 ... 2^33)", (long long)data_bytes);
    CC_CHECK_ARG(restart_interval >= 0 && restart_interval <= 65535, "ccedit_jpegdec_entropy: restart_interval=%d MCUs (0 ... 65535)",
                 restart_interval);
    CC_CHECK_ARG((double)N * (double)cc_jpegdec_intervals(H, W, ncomp, hs, vs, restart_interval) < (double)kPixelMax,
                 "ccedit_jpegdec_entropy: N=%d frames hold more than 2^31 restart intervals", N);
    CC_CHECK_ARG(((uintptr_t)coef & 15) == 0 && ((uintptr_t)intervals & 7) == 0 && (((uintptr_t)tables | (uintptr_t)status) & 3) == 0,
                 "ccedit_jpegdec_entropy: coef must be 16-byte aligned, intervals 8-byte, tables and status 4-byte");
    return cc_jpegdec_entropy((const uint8_t*)data, data_bytes, intervals, tables, (int16_t*)coef, status, N, H, W, ncomp, hs, vs,
                              restart_interval, (hipStream_t)stream);
}

extern "C" int ccedit_jpegdec_idct(const void* coef, const int32_t* tables, void* planes, int32_t N, int32_t H, int32_t W, int32_t ncomp,
                                   int32_t hs, int32_t vs, void* stream) {
    CC_CHECK_ARG(coef && tables && planes, "ccedit_jpegdec_idct: null pointer");
    if (int rc = jpegdec_shape_ok("ccedit_jpegdec_idct", N, H, W, ncomp, hs, vs)) return rc;
    CC_CHECK_ARG(((uintptr_t)coef & 15) == 0 && ((uintptr_t)planes & 7) == 0 && ((uintptr_t)tables & 3) == 0,
                 "ccedit_jpegdec_idct: coef must be 16-byte aligned, planes 8-byte, tables 4-byte");
    return cc_jpegdec_idct((const int16_t*)coef, tables, (uint8_t*)planes, N, H, W, ncomp, hs, vs, (hipStream_t)stream);
}

extern "C" int ccedit_jpegdec_rgb(const void* planes, void* out, int32_t N, int32_t H, int32_t W, int32_t ncomp, int32_t hs, int32_t vs,
                                  void* stream) {
    CC_CHECK_ARG(planes && out, "ccedit_jpegdec_rgb: null pointer");
    if (int rc = jpegdec_shape_ok("ccedit_jpegdec_rgb", N, H, W, ncomp, hs, vs)) return rc;
    return cc_jpegdec_rgb((const uint8_t*)planes, (uint8_t*)out, N, H, W, ncomp, hs, vs, (hipStream_t)stream);
}

// ---- GIF (kernels and launchers: gif.hip).  Everything the host can see is checked here, before any HIP call; the chunk bit lengths and
// offsets the pack functions read are device data and are held in range by the kernels themselves.
static const int64_t kGifMaxPixels = (int64_t)1 << 24, kGifMaxChunks = (int64_t)1 << 22;
static const int32_t kGifChunkMax = 3072, kGifMaxFrames = 65535;

static int gif_shape_ok(const char* fn, int32_t N, int32_t H, int32_t W) {
    CC_CHECK_ARG(N >= 1 && N <= kGifMaxFrames, "%s: N=%d frames (1 ... 65535)", fn, N);
    CC_CHECK_ARG(H >= 1 && W >= 1 && H <= 65535 && W <= 65535 && (int64_t)H * W <= kGifMaxPixels,
                 "%s: frames of %dx%d (H and W 1 ... 65535, H * W <= 2^24)", fn, H, W);
    CC_CHECK_ARG((int64_t)N * H * W * 3 < kPixelMax * 4, "%s: N=%d frames of %dx%d are more than one call takes (2^33 bytes)", fn, N, H, W);
    return CCEDIT_OK;
}

static int gif_chunk_ok(const char* fn, int32_t N, int32_t H, int32_t W, int32_t chunk) {
    if (int rc = gif_shape_ok(fn, N, H, W)) return rc;
    CC_CHECK_ARG(chunk >= 1 && chunk <= kGifChunkMax, "%s: chunk=%d pixels (1 ... 3072: a chunk's dictionary never reaches code 4095)", fn, chunk);
    CC_CHECK_ARG((int64_t)N * (((int64_t)H * W + chunk - 1) / chunk) <= kGifMaxChunks, "%s: N=%d frames of %dx%d in chunks of %d pixels are more "
                 "than 2^22 chunks", fn, N, H, W, chunk);
    return CCEDIT_OK;
}

extern "C" int64_t ccedit_gif_slot_bytes(void) { return cc_gif_slot_bytes(); }

extern "C" int ccedit_gif_histogram(const void* frames, int64_t* moments, int32_t N, int32_t H, int32_t W, void* stream) {
    CC_CHECK_ARG(frames && moments, "ccedit_gif_histogram: null pointer (frames and moments are required)");
    if (int rc = gif_shape_ok("ccedit_gif_histogram", N, H, W)) return rc;
    CC_CHECK_ARG(((uintptr_t)moments & 7) == 0, "ccedit_gif_histogram: moments must be 8-byte aligned");
    return cc_gif_histogram((const uint8_t*)frames, moments, N, H, W, (hipStream_t)stream);
}

extern "C" int ccedit_gif_palette(int64_t* moments, void* cells, void* palettes, int32_t N, void* stream) {
    CC_CHECK_ARG(moments && cells && palettes, "ccedit_gif_palette: null pointer (moments, cells and palettes are required)");
    CC_CHECK_ARG(N >= 1 && N <= kGifMaxFrames, "ccedit_gif_palette: N=%d frames (1 ... 65535)", N);
    CC_CHECK_ARG(((uintptr_t)moments & 7) == 0, "ccedit_gif_palette: moments must be 8-byte aligned");
    return cc_gif_palette(moments, (uint8_t*)cells, (uint8_t*)palettes, N, (hipStream_t)stream);
}

extern "C" int ccedit_gif_map(const void* frames, const void* cells, void* indices, int32_t N, int32_t H, int32_t W, void* stream) {
    CC_CHECK_ARG(frames && cells && indices, "ccedit_gif_map: null pointer (frames, cells and indices are required)");
    if (int rc = gif_shape_ok("ccedit_gif_map", N, H, W)) return rc;
    return cc_gif_map((const uint8_t*)frames, (const uint8_t*)cells, (uint8_t*)indices, N, H, W, (hipStream_t)stream);
}

extern "C" int ccedit_gif_lzw(const void* indices, void* slots, int32_t* chunk_bits, int32_t N, int32_t H, int32_t W, int32_t chunk, void* stream) {
    CC_CHECK_ARG(indices && slots && chunk_bits, "ccedit_gif_lzw: null pointer (indices, slots and chunk_bits are required)");
    if (int rc = gif_chunk_ok("ccedit_gif_lzw", N, H, W, chunk)) return rc;
    CC_CHECK_ARG((((uintptr_t)slots | (uintptr_t)chunk_bits) & 3) == 0, "ccedit_gif_lzw: slots and chunk_bits must be 4-byte aligned");
    return cc_gif_lzw((const uint8_t*)indices, (uint8_t*)slots, chunk_bits, N, H, W, chunk, (hipStream_t)stream);
}

extern "C" int ccedit_gif_pack_scan(const int32_t* chunk_bits, int64_t* chunk_off, int32_t* frame_bytes, int32_t N, int32_t H, int32_t W,
                                    int32_t chunk, void* stream) {
    CC_CHECK_ARG(chunk_bits && chunk_off && frame_bytes, "ccedit_gif_pack_scan: null pointer");
    if (int rc = gif_chunk_ok("ccedit_gif_pack_scan", N, H, W, chunk)) return rc;
    CC_CHECK_ARG((((uintptr_t)chunk_bits | (uintptr_t)frame_bytes) & 3) == 0 && ((uintptr_t)chunk_off & 7) == 0,
                 "ccedit_gif_pack_scan: chunk_bits and frame_bytes must be 4-byte aligned, chunk_off 8-byte");
    return cc_gif_pack_scan(chunk_bits, chunk_off, frame_bytes, N, H, W, chunk, (hipStream_t)stream);
}

extern "C" int ccedit_gif_pack(const void* slots, const int32_t* chunk_bits, const int64_t* chunk_off, void* out, int32_t N, int32_t H, int32_t W,
                               int32_t chunk, int64_t out_bytes, void* stream) {
    CC_CHECK_ARG(slots && chunk_bits && chunk_off && out, "ccedit_gif_pack: null pointer");
    if (int rc = gif_chunk_ok("ccedit_gif_pack", N, H, W, chunk)) return rc;
    CC_CHECK_ARG(out_bytes >= 1 && out_bytes < kPixelMax * 4, "ccedit_gif_pack: out_bytes=%lld (1 ... 2^33: the sum of frame_bytes)",
                 (long long)out_bytes);
    CC_CHECK_ARG((((uintptr_t)slots | (uintptr_t)chunk_bits | (uintptr_t)out) & 3) == 0 && ((uintptr_t)chunk_off & 7) == 0,
                 "ccedit_gif_pack: slots, chunk_bits and out must be 4-byte aligned, chunk_off 8-byte");
    return cc_gif_pack((const uint8_t*)slots, chunk_bits, chunk_off, (uint8_t*)out, N, H, W, chunk, out_bytes, (hipStream_t)stream);
}

// ---- PNG (kernels and launchers: png.hip).  Everything the host can see is checked here, before any HIP call; token words, histograms
// and bit lengths are device data, which the kernels mask and clamp themselves.
static const int64_t kPngMaxLength = 65535 + 3 * kGifMaxPixels;          // H * (1 + 3 W) with H <= 65535 and H * W <= 2^24

static int png_streams_ok(const char* fn, int32_t N, int64_t L) {
    CC_CHECK_ARG(N >= 1 && N <= kGifMaxFrames, "%s: N=%d streams (1 ... 65535)", fn, N);
    CC_CHECK_ARG(L >= 1 && L <= kPngMaxLength, "%s: L=%lld bytes per stream (1 ... 65535 + 3 * 2^24)", fn, (long long)L);
    CC_CHECK_ARG((int64_t)N * ((L + cc_png_chunk_bytes() - 1) / cc_png_chunk_bytes()) <= kGifMaxChunks,
                 "%s: N=%d streams of %lld bytes are more than 2^22 chunks: encode fewer at a time", fn, N, (long long)L);
    return 0;
}

static int png_chunks_ok(const char* fn, int32_t N, int32_t C) {
    CC_CHECK_ARG(N >= 1 && N <= kGifMaxFrames, "%s: N=%d streams (1 ... 65535)", fn, N);
    CC_CHECK_ARG(C >= 1 && (int64_t)N * C <= kGifMaxChunks, "%s: C=%d chunks per stream (>= 1, N * C <= 2^22)", fn, C);
    return 0;
}

extern "C" int64_t ccedit_png_chunk_bytes(void) { return cc_png_chunk_bytes(); }
extern "C" int64_t ccedit_png_slot_bytes(void) { return cc_png_slot_bytes(); }

extern "C" int ccedit_png_filter(const void* frames, void* filtered, int32_t N, int32_t H, int32_t W, void* stream) {
    CC_CHECK_ARG(frames && filtered, "ccedit_png_filter: null pointer (frames and filtered are required)");
    if (int rc = gif_shape_ok("ccedit_png_filter", N, H, W)) return rc;
    return cc_png_filter((const uint8_t*)frames, (uint8_t*)filtered, N, H, W, (hipStream_t)stream);
}

extern "C" int ccedit_png_tokens(const void* filtered, uint32_t* tokens, int32_t* ntok, uint32_t* hist, int32_t N, int64_t L, void* stream) {
    CC_CHECK_ARG(filtered && tokens && ntok && hist, "ccedit_png_tokens: null pointer (filtered, tokens, ntok and hist are required)");
    if (int rc = png_streams_ok("ccedit_png_tokens", N, L)) return rc;
    CC_CHECK_ARG((((uintptr_t)tokens | (uintptr_t)ntok | (uintptr_t)hist) & 3) == 0, "ccedit_png_tokens: tokens, ntok and hist must be 4-byte aligned");
    return cc_png_tokens((const uint8_t*)filtered, tokens, ntok, hist, N, L, (hipStream_t)stream);
}

extern "C" int ccedit_png_codes(const uint32_t* hist, uint32_t* codes, uint32_t* header, int32_t* header_bits, int32_t* chunk_bits, int32_t N, int32_t C,
                                void* stream) {
    CC_CHECK_ARG(hist && codes && header && header_bits && chunk_bits, "ccedit_png_codes: null pointer");
    if (int rc = png_chunks_ok("ccedit_png_codes", N, C)) return rc;
    CC_CHECK_ARG((((uintptr_t)hist | (uintptr_t)codes | (uintptr_t)header | (uintptr_t)header_bits | (uintptr_t)chunk_bits) & 3) == 0,
                 "ccedit_png_codes: every buffer must be 4-byte aligned");
    return cc_png_codes(hist, codes, header, header_bits, chunk_bits, N, C, (hipStream_t)stream);
}

extern "C" int ccedit_png_emit(const uint32_t* tokens, const int32_t* ntok, const uint32_t* codes, const uint32_t* header, const int32_t* header_bits,
                               void* slots, int64_t chunks, void* stream) {
    CC_CHECK_ARG(tokens && ntok && codes && header && header_bits && slots, "ccedit_png_emit: null pointer");
    CC_CHECK_ARG(chunks >= 1 && chunks <= kGifMaxChunks, "ccedit_png_emit: chunks=%lld (1 ... 2^22)", (long long)chunks);
    CC_CHECK_ARG((((uintptr_t)tokens | (uintptr_t)ntok | (uintptr_t)codes | (uintptr_t)header | (uintptr_t)header_bits | (uintptr_t)slots) & 3) == 0,
                 "ccedit_png_emit: every buffer must be 4-byte aligned");
    return cc_png_emit(tokens, ntok, codes, header, header_bits, (uint8_t*)slots, chunks, (hipStream_t)stream);
}

extern "C" int ccedit_png_pack_scan(const int32_t* chunk_bits, int64_t* chunk_off, int32_t* frame_bytes, int32_t N, int32_t C, void* stream) {
    CC_CHECK_ARG(chunk_bits && chunk_off && frame_bytes, "ccedit_png_pack_scan: null pointer");
    if (int rc = png_chunks_ok("ccedit_png_pack_scan", N, C)) return rc;
    CC_CHECK_ARG((((uintptr_t)chunk_bits | (uintptr_t)frame_bytes) & 3) == 0 && ((uintptr_t)chunk_off & 7) == 0,
                 "ccedit_png_pack_scan: chunk_bits and frame_bytes must be 4-byte aligned, chunk_off 8-byte");
    return cc_png_pack_scan(chunk_bits, chunk_off, frame_bytes, N, C, (hipStream_t)stream);
}

extern "C" int ccedit_png_pack(const void* slots, const int32_t* chunk_bits, const int64_t* chunk_off, void* out, int32_t N, int32_t C, int64_t out_bytes,
                               void* stream) {
    CC_CHECK_ARG(slots && chunk_bits && chunk_off && out, "ccedit_png_pack: null pointer");
    if (int rc = png_chunks_ok("ccedit_png_pack", N, C)) return rc;
    CC_CHECK_ARG(out_bytes >= 1 && out_bytes < kPixelMax * 4, "ccedit_png_pack: out_bytes=%lld (1 ... 2^33: the sum of frame_bytes)",
                 (long long)out_bytes);
    CC_CHECK_ARG((((uintptr_t)slots | (uintptr_t)chunk_bits | (uintptr_t)out) & 3) == 0 && ((uintptr_t)chunk_off & 7) == 0,
                 "ccedit_png_pack: slots, chunk_bits and out must be 4-byte aligned, chunk_off 8-byte");
    return cc_png_pack((const uint8_t*)slots, chunk_bits, chunk_off, (uint8_t*)out, N, C, out_bytes, (hipStream_t)stream);
}

extern "C" int ccedit_png_adler(const void* filtered, uint32_t* partials, uint32_t* adler, int32_t N, int64_t L, void* stream) {
    CC_CHECK_ARG(filtered && partials && adler, "ccedit_png_adler: null pointer (filtered, partials and adler are required)");
    if (int rc = png_streams_ok("ccedit_png_adler", N, L)) return rc;
    CC_CHECK_ARG((((uintptr_t)partials | (uintptr_t)adler) & 3) == 0, "ccedit_png_adler: partials and adler must be 4-byte aligned");
    return cc_png_adler((const uint8_t*)filtered, partials, adler, N, L, (hipStream_t)stream);
}

// ---- PNG decoding (kernels and launchers: pngdec.hip).  Geometry and buffers are checked here, before any HIP call; the stream table
// is device data and is clamped into [0, data_bytes] by the kernel, the streams' content is checked by the decoder itself.
extern "C" int ccedit_pngdec_inflate(const void* data, int64_t data_bytes, const int64_t* streams, void* filtered, int32_t* status, int32_t N,
                                     int32_t H, int32_t W, void* stream) {
    CC_CHECK_ARG(data && streams && filtered && status, "ccedit_pngdec_inflate: null pointer (data, streams, filtered and status are required)");
    if (int rc = gif_shape_ok("ccedit_pngdec_inflate", N, H, W)) return rc;
    CC_CHECK_ARG(data_bytes >= 1 && data_bytes < kPixelMax * 4, "ccedit_pngdec_inflate: data_bytes=%lld (1 ... 2^33)", (long long)data_bytes);
    CC_CHECK_ARG(((uintptr_t)streams & 7) == 0 && ((uintptr_t)status & 3) == 0,
                 "ccedit_pngdec_inflate: streams must be 8-byte aligned, status 4-byte");
    return cc_pngdec_inflate((const uint8_t*)data, data_bytes, streams, (uint8_t*)filtered, status, N, H, W, (hipStream_t)stream);
}

extern "C" int ccedit_pngdec_unfilter(const void* filtered, void* rgb, int32_t* status, int32_t N, int32_t H, int32_t W, void* stream) {
    CC_CHECK_ARG(filtered && rgb && status, "ccedit_pngdec_unfilter: null pointer (filtered, rgb and status are required)");
    if (int rc = gif_shape_ok("ccedit_pngdec_unfilter", N, H, W)) return rc;
    CC_CHECK_ARG(((uintptr_t)status & 3) == 0, "ccedit_pngdec_unfilter: status must be 4-byte aligned");
    return cc_pngdec_unfilter((const uint8_t*)filtered, (uint8_t*)rgb, status, N, H, W, (hipStream_t)stream);
}

// ---- GIF decoding (kernels and launchers: gifdec.hip).  Geometry and buffers are checked here, before any HIP call; the descriptors
// are device data and are checked against these sizes by the kernels.
static const int64_t kGifdecMaxCodes = (int64_t)1 << 31;

static int gifdec_common_ok(const char* fn, int32_t N, int64_t total_codes) {
    CC_CHECK_ARG(N >= 1 && N <= kGifMaxFrames, "%s: N=%d images (1 ... 65535)", fn, N);
    CC_CHECK_ARG(total_codes >= 1 && total_codes < kGifdecMaxCodes, "%s: total_codes=%lld (1 ... 2^31 - 1)", fn, (long long)total_codes);
    return 0;
}

extern "C" int ccedit_gifdec_codes(const void* data, int64_t data_bytes, const int64_t* desc, int32_t* parent, int32_t* len, int32_t* off,
                                   void* first, void* last, int64_t total_codes, int32_t* ncodes, int32_t* status, int32_t N, void* stream) {
    CC_CHECK_ARG(data && desc && parent && len && off && first && last && ncodes && status, "ccedit_gifdec_codes: null pointer");
    if (int rc = gifdec_common_ok("ccedit_gifdec_codes", N, total_codes)) return rc;
    CC_CHECK_ARG(data_bytes >= 1 && data_bytes < kPixelMax * 4, "ccedit_gifdec_codes: data_bytes=%lld (1 ... 2^33)", (long long)data_bytes);
    CC_CHECK_ARG(((uintptr_t)desc & 7) == 0 && (((uintptr_t)parent | (uintptr_t)len | (uintptr_t)off | (uintptr_t)ncodes | (uintptr_t)status) & 3) == 0,
                 "ccedit_gifdec_codes: desc must be 8-byte aligned, parent, len, off, ncodes and status 4-byte");
    return cc_gifdec_codes((const uint8_t*)data, data_bytes, desc, parent, len, off, (uint8_t*)first, (uint8_t*)last, total_codes, ncodes, status, N,
                           (hipStream_t)stream);
}

extern "C" int ccedit_gifdec_pixels(const int64_t* desc, const int32_t* parent, const int32_t* len, const int32_t* off, const void* last,
                                    int64_t total_codes, const int32_t* ncodes, void* planes, int64_t plane_bytes, int32_t N, int64_t max_codes,
                                    void* stream) {
    CC_CHECK_ARG(desc && parent && len && off && last && ncodes && planes, "ccedit_gifdec_pixels: null pointer");
    if (int rc = gifdec_common_ok("ccedit_gifdec_pixels", N, total_codes)) return rc;
    CC_CHECK_ARG(plane_bytes >= 1 && plane_bytes < kPixelMax * 4, "ccedit_gifdec_pixels: plane_bytes=%lld (1 ... 2^33)", (long long)plane_bytes);
    CC_CHECK_ARG(max_codes >= 1 && max_codes <= kGifMaxPixels + 1 && max_codes <= total_codes,
                 "ccedit_gifdec_pixels: max_codes=%lld (1 ... 2^24 + 1, at most total_codes: the largest dCodeCap)", (long long)max_codes);
    CC_CHECK_ARG(((uintptr_t)desc & 7) == 0 && (((uintptr_t)parent | (uintptr_t)len | (uintptr_t)off | (uintptr_t)ncodes) & 3) == 0,
                 "ccedit_gifdec_pixels: desc must be 8-byte aligned, parent, len, off and ncodes 4-byte");
    return cc_gifdec_pixels(desc, parent, len, off, (const uint8_t*)last, total_codes, ncodes, (uint8_t*)planes, plane_bytes, N, max_codes,
                            (hipStream_t)stream);
}

extern "C" int ccedit_gifdec_compose(const void* data, int64_t data_bytes, const int64_t* desc, const void* planes, int64_t plane_bytes, void* canvas,
                                     void* out, int32_t* status, int32_t N, int32_t n_out, int32_t H, int32_t W, void* stream) {
    CC_CHECK_ARG(data && desc && planes && canvas && status, "ccedit_gifdec_compose: null pointer (data, desc, planes, canvas and status are required)");
    CC_CHECK_ARG(n_out >= 0 && n_out <= N && (out || n_out == 0), "ccedit_gifdec_compose: n_out=%d outputs (0 ... N, with a buffer)", n_out);
    if (int rc = gif_shape_ok("ccedit_gifdec_compose", N, H, W)) return rc;
    CC_CHECK_ARG(data_bytes >= 1 && data_bytes < kPixelMax * 4, "ccedit_gifdec_compose: data_bytes=%lld (1 ... 2^33)", (long long)data_bytes);
    CC_CHECK_ARG(plane_bytes >= 1 && plane_bytes < kPixelMax * 4, "ccedit_gifdec_compose: plane_bytes=%lld (1 ... 2^33)", (long long)plane_bytes);
    CC_CHECK_ARG(((uintptr_t)desc & 7) == 0 && ((uintptr_t)status & 3) == 0, "ccedit_gifdec_compose: desc must be 8-byte aligned, status 4-byte");
    return cc_gifdec_compose((const uint8_t*)data, data_bytes, desc, (const uint8_t*)planes, plane_bytes, (uint8_t*)canvas, (uint8_t*)out, status, N,
                             n_out, H, W, (hipStream_t)stream);
}
