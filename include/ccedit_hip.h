/*
 * ccedit_hip.h — C ABI of libccedit_hip.so: the MI355X (gfx950) kernels behind CCEdit's denoising
 * hot path (sgm pseudo-3D UNet + ControlNet2D + DPMPP2SAncestral + AutoencoderKL decode).
 *
 * The reference (RuoyuFeng/CCEdit) is pure Python on ATen and has NO FFI of its own: its operator
 * API is `instantiate_from_config` (sgm/util.py:168-185).  This header is the boundary the build adds
 * underneath that API.  Each entry point names the reference call sites whose vendor kernels
 * (cuDNN / cuBLAS / SDPA / ATen elementwise) it replaces.  INTEGRATION.md shows the Python-side
 * binding (ctypes) a reference maintainer would add.
 *
 * Conventions
 *   - plain C: device pointers as void*, sizes as int32/int64, scalars by value, one POD descriptor
 *     struct per fused op; no torch types.
 *   - every function enqueues on `stream` (a hipStream_t passed as void*) and returns immediately;
 *     no host synchronisation, no allocation, no ownership transfer.  Workspaces are caller-owned.
 *   - return value: 0 = ok; <0 = CCEDIT_E* (invalid argument / unsupported shape); >0 = hipError_t.
 *     `ccedit_last_error()` returns a thread-local message for the last non-zero return.
 *   - activations: bf16, "frames-outermost channels-last": logical (B*T, C, H, W) stored with
 *     strides (H*W*C, 1, W*C, C), i.e. a row-major [B*T*H*W pixels][C] matrix.  Weights: bf16,
 *     packed [Cout_pad][taps][Cin_pad] (K contiguous) by ccedit_amd/packing.py from the reference's
 *     OIHW / (O,I,K) / (O,I) fp32 tensors.  Biases, norm affine parameters, statistics: fp32.
 */
#ifndef CCEDIT_HIP_H
#define CCEDIT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CCEDIT_ABI_VERSION 12

#define CCEDIT_OK 0
#define CCEDIT_EINVAL (-1)       /* null pointer / bad size */
#define CCEDIT_EUNSUPPORTED (-2) /* shape or option outside what the kernels implement */

int ccedit_abi_version(void);
const char* ccedit_last_error(void);
/* name of the kernel template the last ccedit_gemm / ccedit_ff320 / ccedit_attention call of this thread dispatched to
 * ("g8_kernel 256x256", "conv_halo_kernel, four-slot weight ring" / "conv_halo_kernel, two-slot weight ring" by policy conv_halo,
 * "conv_halo_kernel, four-slot weight ring, 256-pixel tile" by policy conv_wide, "tap_gemm_kernel 128x128 s2", ...): bench.py's per-kernel roofline table */
const char* ccedit_last_kernel(void);
/* fills name with hipDeviceProp_t.gcnArchName of the current device; returns CU count or <0 */
int ccedit_device_info(char* name, int name_len);

/* Dispatch policy: ONE table of named integer switches that choose between kernels computing the same fp32 sums in a different order
 * (A/B arms and the "specialised kernels reproduce the generic ones" tests).  All default to the fast path.  The library never reads
 * the environment; the host sets entries before launching (process-wide, not thread-safe against concurrent launches).  Names:
 *   conv_halo conv_wide g8 g8_conv g8_temporal g8_split g8_mfma16 lin320 lin320s lin640 temp320 attn_short attn_text attn_spatial attn_pv16 attn_opt gn_flat
 *   gn_apply_flat f32_split
 *   (ccedit_policy_names() returns them comma-separated; semantics in csrc/common.h: CcPolicy)
 * Unknown name: CCEDIT_EINVAL. */
int ccedit_policy_set(const char* name, int32_t value);
int ccedit_policy_get(const char* name, int32_t* value);
const char* ccedit_policy_names(void);

/* ------------------------------------------------------------------------------------------
 * Tap-gather GEMM on MFMA: out[m][n] = epilogue( sum_{tap,c} W[n][tap][c] * A[src(m,tap)][c] )
 *
 * One kernel family covers every contraction of the path (reference call sites):
 *   mode LINEAR   nn.Linear (attention.py:377-383 to_q/to_k/to_v/to_out, :118 GEGLU proj, :136 FF out;
 *                 openaimodel.py:1216-1223 time_embed, :470-476 emb_layers), Conv2d 1x1
 *                 (attention.py:818-820 proj_in/out, openaimodel.py:508 skip_connection,
 *                 controlmodel.py:249-250 zero convs, model.py:169-180 VAE q/k/v/proj), Conv1d k=1 over T
 *                 (attention.py:1088-1130 proj_in/out_temporal, openaimodel.py:712-715) — all the same
 *                 [pixels][C] x [Cout][C]^T product in the channels-last layout.
 *   mode CONV2D   Conv2d 3x3 stride 1/2 pad 1 (openaimodel.py:445-449, 483-492, 369-376 Downsample op,
 *                 controlmodel.py:215-231 hint stem, model.py:100-110 VAE), optional fused nearest-2x
 *                 upsample of the source (openaimodel.py:254-263 Upsample3D, model.py:65-71).
 *   mode TEMPORAL Conv1d k=3 pad 1 over the T keyframes of one clip (openaimodel.py:617-629, 674-687,
 *                 250-252, 377-386, 1611-1621, 1627-1632): rows of frame t gather frames t-1, t, t+1
 *                 at the same pixel (row distance H*W), zero outside [0, T).
 * A second source (A2) supplies channels [Cin1, Cin) — the torch.cat([h, hs.pop()+control.pop()])
 * of controlmodel.py:539-543 without materialising it.
 * ------------------------------------------------------------------------------------------ */
enum { CCEDIT_GEMM_LINEAR = 0, CCEDIT_GEMM_CONV2D = 1, CCEDIT_GEMM_TEMPORAL = 2 };
enum { CCEDIT_ACT_NONE = 0, CCEDIT_ACT_SILU = 1, CCEDIT_ACT_GEGLU = 2,
       CCEDIT_ACT_QUICK_GELU = 3 /* x * sigmoid(1.702 x): the CLIP text MLP (FrozenCLIPEmbedder, encoders/modules.py:358-420) */ };

typedef struct CcGemmDesc {
    int64_t M;            /* output rows: pixels (B*T*Hout*Wout) or tokens */
    int32_t N;            /* packed output rows of W actually used (Cout; 2*inner for GEGLU) */
    int32_t Cin;          /* channels per tap (multiple of 8) */
    int32_t Cin1;         /* channels taken from A (== Cin when A2 is null) */
    int32_t taps;         /* 1, 3 (temporal) or 9 (3x3) */
    int32_t mode;         /* CCEDIT_GEMM_* */
    int32_t Hin, Win;     /* CONV2D: stored source frame size */
    int32_t Hout, Wout;   /* CONV2D: output frame size */
    int32_t stride, pad, ksize;
    int32_t upsample;     /* CONV2D: 1 = source is nearest-2x upsampled on the fly */
    int32_t T, HW;        /* TEMPORAL: frames per clip, pixels per frame */
    int32_t lda, lda2;    /* source row strides (elements) */
    int32_t ldc;          /* output row stride (elements) */
    int32_t Kpad;         /* weight row stride (elements), multiple of 64, >= taps*Cin */
    int32_t act;          /* CCEDIT_ACT_* (applied to acc + bias + group_bias, before residuals) */
    int32_t out_f32;      /* 1: store fp32 instead of bf16 */
    int32_t group_rows;   /* rows per group_bias row (T*H*W for the timestep-embedding add); 0 = unused */
    int32_t ldr1, ldr2;   /* residual row strides */
    int32_t tile;         /* 0 = auto; forcing a block shape is for tests / tuning: 1 = 128ch x 128pix, 2 = 64ch x 256pix,
                           * 3-5 = wider 8-wave shapes, 6 = 320ch x 128pix (N % 320 == 0, no gn_stats), 8 = LDS-halo 3x3 conv,
                           * 9 = register-resident weights (Linear, K = 320, N % 320 == 0, bias + one residual or GEGLU epilogue),
                           * 10 = the same at K = 640 (Linear, N % 128 == 0, M % 16 == 0; bias, one residual, row_sums, ln_stats / ln_sums),
                           * 11-13 = persistent eight-phase GEMM (block shape by Cout / 256ch x 256pix / 128ch x 512pix),
                           * 14 = streaming Conv1d k3 over T with 320 input channels (TEMPORAL, N % 64 == 0, HW % 16 == 0, unsharded frames;
                           *      bias, per-clip row bias, up to two residuals, gn_stats),
                           * 15 = LDS-halo 3x3 conv on 256-pixel (16 x 16) tiles (as 8, and Hout % 16 == 0, a source frame below 2^31 elements;
                           *      gn_rows need not be a multiple of 256) */
    int32_t korder;       /* weight K order: 0 = [tap][Cin]; 1 = [Cin/64][tap][64] (needs Cin % 64 == 0) */
    int32_t gn_rows;      /* with gn_stats: output rows per frame (H*W), a multiple of 128 dividing M (not a
                           * multiple of 256: block shape 1 is used); else 0 */
    /* TEMPORAL with the T keyframes of a clip sharded over ranks (0 = unsharded): the source holds Tsrc frames
     * per clip — tsrc_off halo frames received from the previous rank, the T local frames, then the next rank's —
     * and local frame 0 is global keyframe t0 of Tglob; taps outside [0, Tglob) read zeros (Conv1d padding). */
    int32_t Tsrc, tsrc_off, t0, Tglob;
    int32_t cgroup;       /* internal (set by the library): block-order parameters; pass 0 */
    int32_t ldgb;         /* row stride of group_bias in elements; 0 = N (rows of a wider matrix: all ResBlocks' emb_layers
                           * projections of one network come out of ONE GEMM, each layer reads its column slice) */
    float ln_eps;         /* 0 = off.  > 0 (Linear, K = 320, N % 320 == 0, no activation / residual; tile 0 or 9 — the call always runs the
                           * register-resident-weights kernel and is REFUSED with CCEDIT_EUNSUPPORTED otherwise): every row of
                           * A is LayerNorm-normalised WITHOUT affine, (x - mean) * rsqrt(var + ln_eps) rounded to bf16, before the
                           * product — `to_q(norm(x))` of attention.py:695-716 with gamma / beta folded into W / bias by the caller
                           * (W diag(gamma), b + W beta: ccedit_amd/packing.py:fold_layernorm) */
    const void* A;        /* bf16 [rows][lda] */
    const void* A2;       /* optional second source */
    const void* W;        /* bf16 [ceil(N,256)][Kpad] (rows zero-padded to the widest block shape) */
    const float* bias;    /* [N] in packed row order, or null */
    const float* group_bias; /* [M/group_rows][N] fp32 or null  (ResBlock: h + emb_out, openaimodel.py:762) */
    const void* res1;     /* bf16 residuals added after the activation, or null */
    const void* res2;
    void* out;            /* bf16 (or fp32) [M][ldc]; GEGLU writes N/2 columns */
    /* optional: GroupNorm(32, N) statistics of the tensor being written, accumulated in the epilogue so that the
     * following normalisation (openaimodel.py:441-444, 479-482; attention.py:153-156) does not re-read it:
     * float[M/gn_rows][32][2] (sum, sum of squares of the bf16-rounded outputs), ZEROED BY THE CALLER, added to
     * atomically.  Needs N % 32 == 0, N >= 256, bf16 output, no GEGLU.  Consumed by ccedit_groupnorm_spatial_apply. */
    double* gn_stats;
    /* optional scratch for split-K (outputs with far fewer 256 x 256 tiles than the chip has CUs and a long K loop — the 8x12 level
     * of the networks): ccedit_gemm_workspace_bytes(desc) bytes, 16-byte aligned, whose FIRST 4096 BYTES ARE ZERO before the
     * first call that uses the buffer (the arrival counters; every call leaves them zero again).  One buffer may serve all calls
     * of one stream; calls on different streams need different buffers.  null / too small: no split (same results up to the
     * fp32 summation order of the K loop, which split-K fixes per split count). */
    void* workspace;
    int64_t workspace_bytes;
    int32_t split_k;      /* internal (set by the library); pass 0 */
    /* 0 = off.  p + 1 (p = 0..3; ABI 9, was reserved): one output PARITY of `conv3x3(nearest_upsample_2x(x))` (Upsample.forward,
     * openaimodel.py:204-217 / 254-263) evaluated on the LOW-resolution source.  An output pixel (2 oy + py, 2 ox + px), py = p >> 1,
     * px = p & 1, sees only a 2 x 2 neighbourhood of the source: its nine taps collapse onto four with summed weights
     * (ccedit_amd/packing.py:pack_upsample_parities), 4/9 of the multiply-adds.  CONV2D with ksize 2, stride 1, Hout x Wout = Hin x Win =
     * the source frame, M = source pixels; tap (dy, dx) reads source pixel (oy - 1 + py + dy, ox - 1 + px + dx), zeros outside the
     * frame; the result row of source pixel (n, oy, ox) is stored at row (n 2H + 2 oy + py) 2W + 2 ox + px of `out`, which holds
     * 4 M rows.  `pad` / `upsample` are ignored; no gn_stats. */
    int32_t subpix;
    /* optional: LayerNorm folded into a plain Linear / GEGLU projection whose K is not 320 (`to_q(norm(x))`, `ff.net[0].proj(norm(x))`
     * of attention.py:695-716 at 640 / 1280 channels).  A holds the UN-normalised rows, W / bias the gamma / beta-folded weights
     * (as for ln_eps), ln_colsum[N] the row sums of the bf16 weights as packed, ln_stats[M][2] = (mean, rstd) of every row of A
     * (ccedit_row_stats).  The call computes rstd (W' x - mean colsum) + b'.  Persistent eight-phase kernel only (tile 0 / 11-13,
     * Linear, no residual / row bias / gn_stats); refused with CCEDIT_EUNSUPPORTED elsewhere. */
    const float* ln_colsum;
    const float* ln_stats;
    /* ... or ln_sums[M][2] = (sum, sum of squares) of every row of A in double, as a producing call accumulated them through
     * row_sums; then mean = s / Cin, rstd = rsqrt(q / Cin - mean^2 + ln_sums_eps).  Exactly one of ln_stats / ln_sums. */
    const double* ln_sums;
    /* optional, producer side (Linear, no activation, persistent eight-phase kernel; refused elsewhere): the epilogue adds every
     * output row's (sum, sum of squares) of the bf16-rounded values it stores to row_sums[M][2] (double, ZEROED BY THE CALLER) —
     * the LayerNorm statistics of the tensor being written, for the call that consumes it through ln_sums. */
    double* row_sums;
    float ln_sums_eps;
    /* CONV2D, 0 = off (ABI 9, was reserved).  1: the source frames carry their own vertical halo — Hin = the rows the taps may touch
     * (one row above and, for stride 1, one below the rows that produce output; zeros where the frame ends), Hout = output rows — so
     * the vertical padding is one less than `pad` (resp. than the parity's, with subpix; then Hin == Hout + 2).  How a frame whose ROWS
     * are sharded over ranks is convolved after the neighbours' boundary rows were received (ccedit_amd/parallel.py: RowShard;
     * BASELINE.json config 4).  Generic tap-gather kernel only.
     * 2 (ABI 10): the same sharded frame WITHOUT an extended copy — A holds the local rows only (Hin = local rows, padding geometry of
     * the whole frame), and taps one row above / below them read halo_top / halo_bot, bf16 [frames][Win][lda-strided rows] as received
     * from the neighbour ranks; a null pointer means the frame ends there (zeros). */
    int32_t vpad;
    const void* halo_top;
    const void* halo_bot;
    /* optional (ABI 12): the same weights as W once more in MFMA A-FRAGMENT order, for the kernels that keep a weight slice in
     * registers for their whole life (tile 9 / 10 / 14: K = 320 / 640 Linears, 320-channel Conv1d k3).  Block (t, s) — output rows
     * 16 t .. 16 t + 15, k 32 s .. 32 s + 31 of the [rows][Kpad] matrix W — is 1 KB at element offset (t * (Kpad / 32) + s) * 512:
     * 64 lanes x 8 bf16, lane (g = lane >> 4, c = lane & 15) holding W[16 t + c][32 s + 8 g .. + 7]; rows padded to a multiple of 16.
     * A wave then loads a fragment as ONE contiguous kilobyte instead of sixteen 64-byte row pieces: the per-launch weight preload
     * (200-400 KB per workgroup through the CU's L1-miss path) is 12 -> 4 us at 400 KB (tools/exp/lin640w.hip, round 6).
     * null: the kernels read W (same values). */
    const void* Wfrag;
} CcGemmDesc;

int ccedit_gemm(const CcGemmDesc* desc, void* stream);
/* Bytes of CcGemmDesc.workspace this call could use on an MI355X (0: the shape is never split).  No GPU needed. */
int64_t ccedit_gemm_workspace_bytes(const CcGemmDesc* desc);

/* ------------------------------------------------------------------------------------------
 * Fused transformer feed-forward, dim 320 (the 64x96 level of the UNet / ControlNet):
 *     out = x + W2 . GEGLU(W1 . LayerNorm(x) + b1) + b2
 * = `x = self.ff(self.norm3(x)) + x` of BasicTransformerBlock._forward (attention.py:695-716) and
 * `x = self.ff(self.norm2(x)) + x` of BasicTransformerSingleLayerBlock._forward (:758-761), with FeedForward /
 * GEGLU as in attention.py:115-141.  One kernel: x is read once, out written once, the 1280-wide hidden activation
 * stays in registers (ff320.hip).  Replaces ccedit_layernorm + two ccedit_gemm calls.
 *   wstream: the weights as ccedit_amd/packing.py:pack_ff320 lays them out — 42 chunks of 64 KB, one per iteration of the
 *            kernel's three-stage software pipeline over the 40 groups of 32 hidden units: per k-step the two GEMM1
 *            A-fragments (value, gate rows of W1 diag(gamma), group c; bf16, v_mfma_f32_32x32x16 lane order) and one GEMM2
 *            A-fragment of W2 (group c - 2), then float b1' = b1 + W1 beta of group c in accumulator order.
 *   b2p:     b2 in accumulator order, float[10][2][16].
 *   ln = 0:  no normalisation (mean 0, rstd 1; the packer must then be given gamma = 1, beta = 0).
 * ------------------------------------------------------------------------------------------ */
typedef struct CcFf320Desc {
    int64_t M;            /* tokens (rows of x / out) */
    int32_t dim, inner;   /* 320, 1280 */
    int32_t ldx, ldo;     /* row strides in elements (multiples of 8) */
    float eps;            /* LayerNorm eps (1e-5) */
    int32_t ln;           /* 1: LayerNorm folded in (statistics computed in the kernel) */
    const void* x;        /* bf16 [M][ldx] */
    void* out;            /* bf16 [M][ldo]; may NOT alias x (other workgroups' reads are not ordered against the stores) */
    const void* wstream;  /* packed weights, 42 * 65536 bytes (block tail: 46 or 50 chunks, see below) */
    const float* b2p;     /* float[320] in accumulator order */
    void* dbg;            /* null (tuning builds only: per-wave phase cycle counters) */
    /* Block tail (ABI 10; all null / 0 = the plain feed-forward above).  With `a` the kernel computes the whole tail of a dim-320
     * transformer block on the row tile it holds (attention.py:695-716 / 758-761 and the proj_out of :865-889 / :1141-1208):
     *     tok = W_o a + b_o + res;   tok = tok + W2 GEGLU(W1 LayerNorm(tok) + b1) + b2;   out = W_p tok + b_p + res2   (with res2)
     * x is not read.  wstream then is [4 prologue chunks | the 42 feed-forward chunks | 4 epilogue chunks] of 65536 bytes
     * (packing.pack_ff320_tail: 50 A-fragments of W_o / W_p per chunk, rows permuted like W2's); bop / bpp: b_o / b_p in accumulator
     * order like b2p.  res2 requires a.  tok and the feed-forward output are rounded to bf16 where the separate launches store them. */
    const void* a;        /* bf16 [M][lda]: input of the prologue projection (the attention output) */
    const void* res;      /* bf16 [M][ldr]: residual added to the prologue projection */
    const void* res2;     /* bf16 [M][ldr2]: residual added to the epilogue projection (null: no epilogue GEMM, out = the feed-forward's) */
    const float* bop;     /* float[320] */
    const float* bpp;     /* float[320] */
    int32_t lda, ldr, ldr2, pad_;
} CcFf320Desc;

int ccedit_ff320(const CcFf320Desc* desc, void* stream);

/* ------------------------------------------------------------------------------------------
 * Normalisation (fp32 statistics, bf16 in/out)
 * ------------------------------------------------------------------------------------------ */
/* GroupNorm(32, C) over (C/32 x H x W) per frame, optional fused SiLU.
 * Replaces nn.GroupNorm + nn.SiLU of openaimodel.py:441-444, 479-482 (eps 1e-5), attention.py:153-156,
 * model.py:50-53 (eps 1e-6).  x: [frames][hw][C]; stats workspace: double[frames*32*2] (zeroed here). */
int ccedit_groupnorm_spatial(const void* x, void* y, const float* gamma, const float* beta,
                             double* stats_ws, int32_t frames, int32_t hw, int32_t C, float eps,
                             int32_t silu, void* stream);
/* The apply half alone, for statistics that a producer already accumulated (CcGemmDesc.gn_stats):
 * stats: double[frames][32][2] = (sum, sum of squares) over the C/32 x hw elements of each group (double: the
 * producers' workgroups meet in global atomics, and in double their arrival order cannot move the fp32 mean / rstd —
 * results are reproducible from run to run). */
int ccedit_groupnorm_spatial_apply(const void* x, void* y, const float* gamma, const float* beta,
                                   const double* stats, int32_t frames, int32_t hw, int32_t C, float eps,
                                   int32_t silu, void* stream);
/* The statistics half alone: adds (sum, sum of squares) of every (frame, group) to stats = double[frames][32][2], ZEROED BY THE CALLER —
 * for frames whose rows are sharded over ranks (RowShard): local sums, all-reduced by the caller, then ccedit_groupnorm_spatial_apply
 * with the sums divided by the number of ranks (its element count is the LOCAL hw). */
int ccedit_groupnorm_spatial_stats(const void* x, double* stats, int32_t frames, int32_t hw, int32_t C, void* stream);
/* GroupNorm(32, C) over (C/32 x T) per pixel — the normalization() / norm_temporal applied to the
 * '(b h w) c t' view (openaimodel.py:617-619, 674-676; attention.py:1085, 1176).
 * x: [B*T][hw][C]; one statistics group = T frames x C/32 channels at one pixel. */
int ccedit_groupnorm_temporal(const void* x, void* y, const float* gamma, const float* beta,
                              int32_t B, int32_t T, int32_t hw, int32_t C, float eps, int32_t silu,
                              void* stream);
/* The same normalisation in two phases for frame-sharded clips: per-(clip, pixel, group) partial sum / sum-of-
 * squares over the LOCAL frames (stats: float[B*hw*32*2], fully overwritten), all-reduced by the caller across the
 * ranks that hold the other frames, then applied with count = (C/32) * T_global.  The output may be written into
 * a halo-extended buffer: frame t of clip b goes to frame index b*dst_frames + t + dst_off. */
int ccedit_groupnorm_temporal_stats(const void* x, float* stats, int32_t B, int32_t T, int32_t hw, int32_t C,
                                    void* stream);
int ccedit_groupnorm_temporal_apply(const void* x, void* y, const float* gamma, const float* beta,
                                    const float* stats, int32_t B, int32_t T, int32_t hw, int32_t C,
                                    float count, float eps, int32_t silu, int32_t dst_frames, int32_t dst_off,
                                    void* stream);
/* LayerNorm over C (eps 1e-5) — attention.py:667-669, 755-756. x,y: [rows][C] */
/* (mean, rstd = rsqrt(var + eps)) of every row of x[rows][C] (bf16, contiguous), fp32 pairs: the statistics half of
 * nn.LayerNorm (attention.py:611-613), consumed by CcGemmDesc.ln_stats.  Same arithmetic as ccedit_layernorm. */
int ccedit_row_stats(const void* x, float* stats, int64_t rows, int32_t C, float eps, void* stream);
int ccedit_layernorm(const void* x, void* y, const float* gamma, const float* beta, int64_t rows,
                     int32_t C, float eps, void* stream);

/* ------------------------------------------------------------------------------------------
 * Attention: softmax(q k^T * scale) v, bf16 MFMA, online softmax, fp32 accumulate.
 * Replaces F.scaled_dot_product_attention in CrossAttention.forward (attention.py:392-467) for
 *   - spatial self-attention      (Lq = Lk = h*w, one batch per frame)
 *   - text cross-attention        (Lk = 77, K/V shared by the T frames of a clip: kv_batch = batch / kv_div)
 *   - temporal self-attention     (Lq = Lk = T per pixel: rows of one sequence are H*W apart)
 * q/k/v/o are [rows][ld] matrices with heads side by side: head h occupies columns [h*d, (h+1)*d).
 * Row of (batch, i) = (batch / inner) * outer_rows + (batch % inner) * inner_rows + i * seq_rows.
 * ------------------------------------------------------------------------------------------ */
typedef struct CcAttnDesc {
    const void* q; const void* k; const void* v; void* o;
    int32_t ldq, ldk, ldv, ldo;       /* row strides in elements */
    int32_t heads, d;                 /* d in {40, 80, 160} or any multiple of 8 up to 160 */
    int32_t batches;                  /* number of (sequence) batches */
    int32_t Lq, Lk;
    int32_t q_inner; int64_t q_outer_rows, q_inner_rows, q_seq_rows;
    int32_t kv_div;                   /* kv batch = batch / kv_div (text K/V shared across frames) */
    int32_t kv_inner; int64_t kv_outer_rows, kv_inner_rows, kv_seq_rows;
    float scale;                      /* d^-0.5 */
    /* optional leading KV segment (anchor-frame keys of SpatialTransformer3DCA, attention.py:1324-1336:
     * context = cat([anchor tokens, x tokens])): keys [0, seg1_len) come from the kv batch
     * (batch / seg1_div) * seg1_mul + seg1_add, keys [seg1_len, Lk) from the regular kv batch.  0 = unused. */
    int32_t seg1_len, seg1_div, seg1_mul, seg1_add;
    int32_t causal;       /* 1: key j is visible to query i only if j <= i (CLIP text encoder); Lq == Lk, no segment */
    int32_t flags;        /* CCEDIT_ATTN_*; 0 = none (ABI 9; was reserved) */
} CcAttnDesc;

/* q already carries scale * log2(e) (folded into the to_q weights by the packer, one rounding instead of two): kernels then take
 * p = 2^(q.k - reference) without multiplying, and `scale` is ignored */
#define CCEDIT_ATTN_Q_LOG2 1
/* kv_div == 1 on the text form: every batch (frame) has K/V of its own (a prompt schedule's per-frame context).  Keeps the descriptor
 * off the text arms that stage the K/V a whole clip shares.  At d = 80, 64 <= Lk <= 96 and Lq >= 1536 contiguous rows per frame it is
 * served by the per-frame arm of attn_text_kernel (work split by frame, 320-channel group and row split), otherwise by the general
 * kernels.  With the flag, kv_div != 1 is an argument error. */
#define CCEDIT_ATTN_KV_PER_FRAME 2

int ccedit_attention(const CcAttnDesc* desc, void* stream);

/* ------------------------------------------------------------------------------------------
 * Layout / elementwise helpers (all HBM-bound)
 * ------------------------------------------------------------------------------------------ */
/* fp32 (B, C, T, H, W) -> bf16 [B*T][H*W][Cpad] (zero-filled pad channels), y = x*scale + shift.
 * Used for the latent (`x * c_in`, denoiser.py:40) and for the hint remap 1-(h+1)/2 (wrappers.py:160-162). */
int ccedit_ncthw_to_nhwc(const float* x, void* y, int32_t B, int32_t C, int32_t T, int32_t H, int32_t W,
                         int32_t Cpad, const float* scale_per_b, float scale, float shift, void* stream);
/* bf16/fp32 [B*T][H*W][ld] (first C columns) -> fp32 (B, C, T, H, W) */
int ccedit_nhwc_to_ncthw(const void* x, int32_t x_is_f32, int32_t ld, float* y, int32_t B, int32_t C,
                         int32_t T, int32_t H, int32_t W, void* stream);
/* out[:, :C1] = a ; out[:, C1:C1+C2] = b + c   (cat([h, hs.pop() + control.pop()]), controlmodel.py:543) */
int ccedit_cat_add(const void* a, const void* b, const void* c, void* out, int64_t rows, int32_t C1,
                   int32_t C2, void* stream);
/* The same, additionally accumulating the GroupNorm(32, C1+C2) statistics of `out` ([frames][hw][C1+C2]) into
 * stats = double[frames][32][2] (sum, sum of squares; ZEROED BY THE CALLER) for ccedit_groupnorm_spatial_apply —
 * the decoder ResBlock's in_layers.0 (openaimodel.py:441-444) then does not re-read the concatenation. */
int ccedit_cat_add_gn(const void* a, const void* b, const void* c, void* out, double* stats, int32_t frames,
                      int32_t hw, int32_t C1, int32_t C2, void* stream);
/* Row-block copy for the layout transposition of a frame-sharded clip (ccedit_amd/parallel.py: FrameShard.to_pixels / to_frames;
 * BASELINE.json config 4 — the reference has no multi-GPU path, scripts/sampling/sampling_tv2v.py:106 is a single .to("cuda")):
 * for s < n_blocks, rows [blocks[3s], + blocks[3s+2]) of src go to rows [blocks[3s+1], ...) of dst; with `add` (bf16 rows laid out
 * like dst) dst = src + add in fp32 with one rounding — the unpack of an all-to-all with the ResBlock skip folded in.
 * blocks: int64 [n_blocks][3] in DEVICE memory; max_rows = the largest block (grid sizing); row_bytes % 16 == 0. */
int ccedit_copy_row_blocks(const void* src, void* dst, const void* add, const int64_t* blocks, int32_t n_blocks,
                           int64_t max_rows, int32_t row_bytes, void* stream);
/* n_blocks strided 2-D copies sharing one geometry (rows x row_bytes, byte pitches) and differing in their byte offsets:
 * blocks = int64 [n_blocks][2] (src offset, dst offset) in DEVICE memory.  The column-slice halves of the head-parallel attention
 * exchange of a row-sharded clip (ccedit_amd/parallel.py: RowShard.to_heads / from_heads; BASELINE.json config 4).
 * row_bytes, pitches and offsets are multiples of 16. */
int ccedit_copy_2d_blocks(const void* src, void* dst, const int64_t* blocks, int32_t n_blocks, int64_t rows, int32_t row_bytes,
                          int64_t src_pitch, int64_t dst_pitch, void* stream);
/* y = a + b (bf16), n elements — `h = h + control.pop()` (controlmodel.py:537), `h += guided_hint` (:300) */
int ccedit_add(const void* a, const void* b, void* y, int64_t n, void* stream);
/* y = silu(x), bf16 elementwise (out_temporal's leading nn.SiLU, openaimodel.py:1627-1632) */
int ccedit_silu(const void* x, void* y, int64_t n, void* stream);
/* timestep_embedding (diffusionmodules/util.py:244-268): out bf16 [n][ld], [cos | sin], dim even */
int ccedit_timestep_embedding(const int64_t* t, void* out, int32_t n, int32_t dim, int32_t ld, void* stream);

/* p = softmax(s * scale) row-wise, fp32 in -> bf16 out, columns [cols, cols_pad) zero-filled.
 * The single-head d=512 attention of the VAE mid block (model.py:180-195) is evaluated as
 * GEMM (q k^T) -> this -> GEMM (p v); cols_pad <= 8192. */
int ccedit_softmax_rows(const float* s, void* p, int64_t rows, int32_t cols, int32_t cols_pad, int64_t lds,
                        int64_t ldp, float scale, void* stream);

/* Token + position embedding lookup of the CLIP text encoder (transformers CLIPTextEmbeddings, called from
 * FrozenCLIPEmbedder.forward, encoders/modules.py:393-413): out[b*L + i] = tok[ids[b*L + i]] + pos[i]  (bf16 out).
 * ids: int64 [rows]; tok: fp32 [vocab][C]; pos: fp32 [L][C].  ids are clamped to [0, vocab): validate on the host. */
int ccedit_embedding_lookup(const int64_t* ids, const float* tok, const float* pos, void* out, int64_t rows, int32_t L,
                            int32_t C, int32_t vocab, void* stream);

/* Posterior sample of the KL-VAE encoder (DiagonalGaussianDistribution.sample, distributions.py:24-41, called from
 * AutoencoderKLInferenceWrapper.encode, autoencoder.py:323-332): moments = fp32 [frames*hw][ldm] channels-last rows
 * [mean(zc) | logvar(zc)] (quant_conv output); noise, out = fp32 (frames, zc, h, w);
 * out = scale * (mean + exp(0.5 * clamp(logvar, -30, 20)) * noise).  The caller supplies the noise (the reference
 * draws it with torch.randn on the CPU global generator). */
int ccedit_gaussian_sample(const float* moments, const float* noise, float* out, int64_t frames, int32_t zc,
                           int32_t hw, int32_t ldm, float scale, void* stream);

/* ------------------------------------------------------------------------------------------
 * fp32 first-stage model (ABI 11).  The reference decodes with autocast disabled (sgm/models/diffusion.py:151-156): fp32 operands,
 * products and tensors.  These three entry points evaluate the KL-VAE in that arithmetic class: fp32 tensors in and out, fp32 sums.
 * ccedit_gemm_f32 has two realisations of the same fp32 contraction (policy `f32_split`): 1 (default, round 6) — every fp32 operand is
 * split EXACTLY into three bf16 numbers and an fp32 product is formed as six exact bf16 x bf16 products on v_mfma_f32_32x32x16_bf16 (the
 * dropped terms are <= 2^-25 of the product, below the rounding of any fp32 accumulation step); 0 — v_mfma_f32_32x32x2_f32; 2 — as 1 but only
 * the eight-wave kernel.  Same descriptor, same results to fp32 rounding (tests/test_vae_f32_gpu.py holds both to the same tolerances).
 * The engine selects the fp32 first stage from the yaml (ccedit_amd/vae.py, policy `vae_fp32`).
 *
 * ccedit_gemm_f32: out[m][n] = bias[n] + sum_k W[n][k] * src(A)[m][k] (+ res[m][n]); everything fp32, channels-last rows.
 *   mode 0  Linear / Conv 1x1: A [M][lda], k = channel < Cin (Cin % 4 == 0); W [N][ldw] with Kpad = Cpad = Cin rounded up to 16,
 *           columns [Cin, Kpad) ZERO (model.py:161-201 q/k/v/proj_out, nin_shortcut, quant / post_quant convs; the attention's
 *           q k^T and p v products with the other tensor in the role of W)
 *   mode 1  Conv2d 3x3: A [frames][Hin][Win][lda]; W [N][9][Cpad] (tap-major, tap = 3 ky + kx, columns [Cin, Cpad) zero);
 *           output pixel (y, x) reads source (y stride - pad + ky, x stride - pad + kx), zeros outside; Hout / Wout are given (the
 *           encoder's Downsample pads right / bottom only, model.py:74-93); upsample = 1: the taps walk over the nearest-2x
 *           upsampled source (2 Hin x 2 Win) without materialising it (model.py:56-71).  M = frames * Hout * Wout.
 *           upsample = 2 + 2 py + px (round 6, policy f32_split != 0 only): ONE OUTPUT PARITY of the same `conv3x3(nearest_upsample_2x(x))`
 *           as a 2 x 2 convolution on x itself — W [N][4][Cpad] holds the merged taps (ccedit_amd/vae_f32.py: pack_f32_parities),
 *           Hout x Wout = Hin x Win, stride 1, pad 1, no residual, M = frames * Hin * Win; the row of source pixel (y, x) is written to
 *           pixel (2 y + py, 2 x + px) of `out` = the 2 Hin x 2 Win frames.  Four calls fill the tensor at 4/9 of the multiply-adds.
 * A and W 16-byte aligned, lda % 4 == 0, ldw % 4 == 0; out / res any row stride >= N (16-byte accesses when a multiple of 4).
 * Fixed summation order: repeated calls are bit-identical. */
typedef struct CcGemmF32Desc {
    const float* A;
    const float* W;
    const float* bias; /* [N] or NULL */
    const float* res;  /* [M][ldr] or NULL */
    float* out;        /* [M][ldc] */
    int64_t M;
    int32_t N, Cin, Cpad, Kpad;
    int32_t lda, ldw, ldc, ldr;
    int32_t mode;
    int32_t Hin, Win, Hout, Wout, stride, pad, upsample;
} CcGemmF32Desc;
int ccedit_gemm_f32(const CcGemmF32Desc* desc, void* stream);
/* y = GroupNorm(32, C, eps)(x) [then SiLU when silu != 0] per frame over (hw x C / 32); x, y fp32 [frames][hw][C] (y may alias x),
 * C in {32, 64, 128, 256, 512, 1024}; stats = fp64 scratch [frames][32][2] (sum, sum of squares; zeroed here).  model.py:45-53. */
int ccedit_groupnorm_f32(const float* x, float* y, const float* gamma, const float* beta, double* stats, int32_t frames, int32_t hw,
                         int32_t C, float eps, int32_t silu, void* stream);
/* s[r][0..cols) = softmax(scale * s[r][0..cols)) in place, fp32 rows of stride ld; columns beyond cols are left alone
 * (rows of up to 8192 columns are held in registers, longer ones are re-read: three passes) */
int ccedit_softmax_rows_f32(float* s, int64_t rows, int32_t cols, int64_t ld, float scale, void* stream);

/* Sampler / guider / denoiser elementwise math on the fp32 latent (417,792 elements at 17x64x96):
 *   ccedit_cfg_denoise : den = x + (-sigma) * (eps_u + scale*(eps_c - eps_u))        [denoiser.py:40 with
 *                        c_skip=1, c_out=-sigma; guiders.py:25-29]   eps = fp32 [2][n]
 *   ccedit_axpby       : y = a*x + b*z                                                [sampling.py:388, 398-402]
 *   ccedit_mask_blend  : y = x*m + z*(1-m), all fp32 [n]                              [sampling.py:150-153, 213-216]
 */
int ccedit_mask_blend(const float* x, const float* z, const float* mask, float* y, int64_t n, void* stream);
int ccedit_cfg_denoise(const float* x, const float* eps2, float* den, int64_t n, float sigma, float scale,
                       void* stream);
int ccedit_axpby(const float* x, const float* z, float* y, int64_t n, float a, float b, void* stream);

/* ------------------------------------------------------------------------------------------
 * Pixel I/O (added without an ABI bump: six new functions, no struct or signature changed, CCEDIT_ABI_VERSION stays 12).
 * The host-side arithmetic of the sampling entry points between decoded uint8 frames and the engine's tensors
 * (scripts/sampling/util.py: load_img, load_video_keyframes, perform_save_locally_video; sampling_tv2v.py: depth_frames;
 * encoders/modules.py: DepthMidasEncoder / DepthZoeEncoder normalisation).  Kernels: csrc/pixel.hip; tap tables:
 * ccedit_amd/packing.py (pil_bicubic_taps, aten_bicubic_taps).  All pointers are device pointers except `ranks`.
 *
 * Tap table of one axis: int32 [out][2 + k]: first source index, tap count (<= k), k weights (zero padded).
 *
 * ccedit_resize_u8_pil: Pillow's 8-bit Image.resize(BICUBIC), bit for bit.  src uint8 [N][Hs][Ws][3] -> horizontal pass with xtab into
 *   tmp uint8 [N][Hs][W][3] ((2^21 + sum w p) >> 22 clipped to 0 ... 255, weights 22-bit fixed point) -> vertical pass with ytab.
 *   out_f32 = 0: dst uint8 [N][H][W][3];  out_f32 = 1: dst fp32 [3][N][H][W] = x / 255 * 2 - 1 (true division), i.e. the
 *   (1, 3, T, H, W) `keyframes` / (N, 3, H, W) `cond_img` (N = 1) tensor of the engine.  xtab = NULL (then Ws == W; tmp unused)
 *   skips the horizontal pass, as Pillow does for an unchanged axis.  Windows are held inside the image by the kernel.
 * ccedit_resize_f32_bicubic: F.interpolate(mode="bicubic", align_corners=False) on fp32 [planes][Hs][Ws] -> [planes][H][W]: tables with
 *   k = 4 and fp32 bit patterns as weights (a = -0.75), first = floor(src position) - 1, taps clamped to the border;
 *   out = sum_j wy_j (sum_i wx_i src[y_j][x_i]).  Agrees with ATen to fp32 rounding (<= 1e-5 on inputs in [-1, 1]).
 * ccedit_kth_values: out[b][r] = the ranks[r]-th smallest (1-based, as torch.kthvalue) of the n values of row b of x fp32 [B][n], for
 *   up to 4 ranks at once (`ranks` is a HOST array).  Exact (radix select, four 8-bit digits of the order-preserving integer image of the
 *   float).  workspace: B * 4128 bytes of device scratch, 4-byte aligned, contents irrelevant.  Inputs must be FINITE (NaN has no
 *   place in the order; -0.0 sorts immediately below +0.0).
 * ccedit_minmax_f32: out[b] = (min, max) of row b, fp32 [B][2]; same input contract.  The MiDaS hint takes ONE min / max over the
 *   whole batch of frames (encoders/modules.py:1376-1386): call it with B = 1 over all of them.
 * ccedit_depth_hint: depth fp32 [B][n] (n = T H W) + (lo, hi) = stats[b * stat_stride + {0, 1}] read from device memory (stat_stride 0:
 *   one pair for all clips) -> hint fp32 [B][3][n]: v = (d - lo) / (hi - lo) (true division), clamped to [0, 1], v * 2 - 1, negated when
 *   flip != 0 (MiDaS: near = bright), written to the three channels.  hi == lo gives NaN like the reference (0 / 0); it is not trapped.
 * ccedit_frames_to_u8: x fp32 [B][3][P] (P = T H W; the decoder's output in [-1, 1], or already in [0, 1] with unit_range != 0) ->
 *   uint8 [B][P][3]: v = clamp((x + 1) / 2, 0, 1), then mode 0: uint8(255 v) (truncation: the frames of the gif / frame files),
 *   mode 1: uint8(min(255 v + 0.5, 255)) (the grid PNG).  One rounding per reference operation: bit-identical to the numpy expression.
 */
int ccedit_resize_u8_pil(const void* src, void* dst, void* tmp, const int32_t* ytab, int32_t yk, const int32_t* xtab, int32_t xk,
                         int32_t N, int32_t Hs, int32_t Ws, int32_t H, int32_t W, int32_t out_f32, void* stream);
int ccedit_resize_f32_bicubic(const float* src, float* dst, const int32_t* ytab, const int32_t* xtab, int64_t planes, int32_t Hs,
                              int32_t Ws, int32_t H, int32_t W, void* stream);
int ccedit_kth_values(const float* x, int32_t B, int64_t n, const int64_t* ranks, int32_t n_ranks, float* out, void* workspace,
                      void* stream);
int ccedit_minmax_f32(const float* x, int32_t B, int64_t n, float* out, void* stream);
int ccedit_depth_hint(const float* depth, float* hint, const float* stats, int32_t stat_stride, int32_t B, int64_t n, int32_t flip,
                      void* stream);
int ccedit_frames_to_u8(const float* x, void* out, int32_t B, int64_t P, int32_t mode, int32_t unit_range, void* stream);

/* ------------------------------------------------------------------------------------------
 * Edit masks (added without an ABI bump: four new functions, CCEDIT_ABI_VERSION stays 12).  What lies between a user's mask and the
 * samplers' inpainting loops (`--inpainting_mode`; the reference's sampling_tv2v.py:385-407 leaves the mask to the user).  Kernels:
 * csrc/mask.hip.  Convention: set = edit (generated), clear = keep the original — x = x * mask + img_orig * (1 - mask).  A byte of a
 * PIXEL mask is set when it is >= 128, a byte of a LATENT mask when it is not 0.  All pointers are device pointers.
 *
 * ccedit_mask_resize_nearest: dst[n][y][x] = src[n][ytab[y]][xtab[x]], uint8 [N][Hs][Ws] -> [N][H][W]; the int32 index tables
 *   (ccedit_amd/packing.py: pil_nearest_index, Pillow's NEAREST: floor((i + 0.5) * in / out)) are clamped into the source by the kernel.
 * ccedit_mask_latent: pixel mask uint8 [N][H][W] (N = B T frames, H % 8 == W % 8 == 0, 8-byte aligned) -> latent mask uint8
 *   [N][H/8][W/8]: 1 where MORE than 32 of the 64 pixels of the 8 x 8 cell are set, else 0 — round(area mean) with the tie 32/64
 *   rounded to even, i.e. clamp(round(F.interpolate(mask, (T, H/8, W/8), mode="area")), 0, 1) of a binary mask, in integers.
 * ccedit_inpaint_blend: y = m ? x : (x0 + noise * sigma) / s over fp32 [B][C][P] (P = T h w) with the latent mask uint8 [B][P] broadcast
 *   over C; sigma and s = sqrt(1 + sigma^2) are computed by the host as the reference does.  One fp32 multiply, one add, one correctly
 *   rounded divide, not contracted: for a binary mask bit-equal to x * m + ((x0 + noise * sigma) / s) * (1 - m) in fp32 (up to the sign
 *   of a zero).  y may alias x.
 * ccedit_mask_composite: out = m ? result : original over fp32 [B][3][P] (P = T H W) with the pixel mask uint8 [B][P] broadcast over the
 *   three channels.  out may alias result.
 */
int ccedit_mask_resize_nearest(const void* src, void* dst, const int32_t* ytab, const int32_t* xtab, int32_t N, int32_t Hs, int32_t Ws,
                               int32_t H, int32_t W, void* stream);
int ccedit_mask_latent(const void* mask_px, void* mask_lat, int64_t N, int32_t H, int32_t W, void* stream);
int ccedit_inpaint_blend(const float* x, const float* x0, const float* noise, const void* mask, float* y, int32_t B, int32_t C, int64_t P,
                         float sigma, float s, void* stream);
int ccedit_mask_composite(const float* result, const float* original, const void* mask_px, float* out, int32_t B, int64_t P, void* stream);

/* ------------------------------------------------------------------------------------------
 * Windows (added without an ABI bump: two new functions, CCEDIT_ABI_VERSION stays 12).  A clip of N > T keyframes is covered by W
 * overlapping windows of T frames; at every network evaluation each window goes through the network at its usual shape and the
 * windows' denoised latents are cross-faded into one latent of N frames (ccedit_amd/windows.py: plan, WindowedDenoiser;
 * `--window_frames`).  Kernels: csrc/window.hip.  Latents are fp32 [B][C][frames][P], P = h w.  `starts` (int32 [W], ascending, each
 * 0 ... N - T) and `coef` (fp32 [W][T], per frame summing to 1 over the windows that cover it) are device tables uploaded once per
 * clip; the kernels clamp a start into 0 ... N - T and write 0 for a frame no window covers, so no table can take an access outside
 * its tensor.  All pointers are device pointers.
 *
 * ccedit_window_gather: xw[w][b][c][j][p] = x[b][c][starts[w] + j][p]; x is [B][C][N][P], xw [W][B][C][T][P] (window w is the contiguous
 *   tensor xw + w B C T P); all W windows in one launch, a bit copy.
 * ccedit_window_fuse: out[b][c][f][p] = sum, over the windows covering f in ascending w, of coef[w][f - starts[w]] *
 *   y_w[b][c][f - starts[w]][p]; out is [B][C][N][P], y_w [B][C][T][P] at yw[w].  `yw` is a DEVICE table of W pointers (8-byte aligned):
 *   the windows' outputs are read where the network left them, nothing is staged into one buffer first.  The first term is the
 *   product alone, every further term one multiply then one add, never an fma: bit-equal to the same loop in numpy float32, and a
 *   frame covered by one window (coefficient 1.0f) is a bit copy.  One launch, every output element written once, no atomics.
 */
int ccedit_window_gather(const float* x, float* xw, const int32_t* starts, int32_t W, int32_t B, int32_t C, int32_t N, int32_t T, int64_t P,
                         void* stream);
int ccedit_window_fuse(const void* yw, float* out, const int32_t* starts, const float* coef, int32_t W, int32_t B, int32_t C, int32_t N,
                       int32_t T, int64_t P, void* stream);

/* ------------------------------------------------------------------------------------------
 * Tiles (added without an ABI bump: two new functions, CCEDIT_ABI_VERSION stays 12).  A frame larger than the size the network is
 * built for is covered by T overlapping tiles of th x tw latent pixels; at every network evaluation each tile goes through the
 * network at its usual shape and the tiles' denoised latents are cross-faded into one latent of h x w (ccedit_amd/tiles.py: plan2d,
 * TiledDenoiser; `--tile_h`, `--tile_w`, `--tile_overlap`).  Kernels: csrc/tile.hip.  Latents are fp32 [planes][rows][columns],
 * planes = B C N.  `starts` (int32 [T][2]: row, column of each tile's first element; y major, x minor, ascending) and `coef` (fp32
 * [T][th][tw], per latent pixel summing to 1 over the tiles that cover it) are device tables uploaded once per clip; the kernels
 * clamp a start into 0 ... h - th / 0 ... w - tw and write 0 for an element no tile covers, so no table can take an access outside
 * its tensor.  All pointers are device pointers, 4-byte aligned; T is 1 ... 64, h >= th >= 1, w >= tw >= 1.
 *
 * ccedit_tile_gather: xt[t][p][i][j] = x[p][sy_t + i][sx_t + j]; x is [planes][h][w], xt [T][planes][th][tw] (tile t is the contiguous
 *   tensor xt + t planes th tw); all T tiles in one launch, a bit copy.
 * ccedit_tile_fuse: out[p][y][x] = sum, over the tiles covering (y, x) in ascending t, of coef[t][y - sy_t][x - sx_t] *
 *   y_t[p][y - sy_t][x - sx_t]; out is [planes][h][w], y_t [planes][th][tw] at yt[t].  `yt` is a DEVICE table of T pointers (8-byte
 *   aligned): the tiles' outputs are read where the network left them.  The first term is the product alone, every further term one
 *   multiply then one add, never an fma: bit-equal to the same loop in numpy float32, and an element covered by one tile
 *   (coefficient 1.0f) is a bit copy.  One launch, every output element written once, no atomics.
 * Both use 16-byte accesses for 4 consecutive elements of a row wherever the row length is a multiple of 4 and the addresses are
 * 16-byte aligned, decided per row in the kernel; any size and alignment is correct.
 */
int ccedit_tile_gather(const float* x, float* xt, const int32_t* starts, int32_t T, int64_t planes, int32_t h, int32_t w, int32_t th,
                       int32_t tw, void* stream);
int ccedit_tile_fuse(const void* yt, float* out, const int32_t* starts, const float* coef, int32_t T, int64_t planes, int32_t h, int32_t w,
                     int32_t th, int32_t tw, void* stream);

/* ------------------------------------------------------------------------------------------
 * Regions (added without an ABI bump: two new functions, CCEDIT_ABI_VERSION stays 12).  A prompt per masked region of the frame: at
 * every network evaluation the network runs once per prompt at its usual shape and the K + 1 denoised latents (region 0 is the base
 * prompt, which covers what the K regions leave) are blended into one by fixed per-cell coefficients (ccedit_amd/regions.py:
 * RegionDenoiser; `--region_prompt`, `--region_mask`, `--region_feather`).  Kernels: csrc/region.hip.  1 <= K <= 7, 0 <= F <= 8.  All
 * pointers are device pointers.
 *
 * ccedit_region_weights: masks uint8 [K][T][H][W] (H, W multiples of 8; 8-byte aligned; a pixel is set when its byte is >= 128) ->
 *   coef fp32 [K + 1][T][h][w], h = H / 8, w = W / 8, one launch.  a_r = set pixels of a latent cell (0 ... 64); s_r = the sum of a_r
 *   over the (2F + 1) x (2F + 1) cells around it, coordinates clamped into the frame (the edge is replicated, F may exceed h or w);
 *   tot = sum_r s_r, S = 64 (2F + 1)^2, D = max(S, tot), s_0 = D - tot; coef[r] = (float)((double)s_r / (double)D): formed from integers
 *   and rounded once per conversion, bit-equal to tests/_regions_numpy.py.  Every cell has a non-zero coefficient; where s_r = D the
 *   coefficient of r is exactly 1.0f and every other exactly 0.0f.
 * ccedit_region_fuse: out[b][c][t][p] = sum over r = 0 ... K, ascending, of coef[r][t][p] * y_r[b][c][t][p]; out and y_r are fp32
 *   [B][C][T][P], P = h w, y_r at yr[r].  `yr` is a DEVICE table of K + 1 pointers (8-byte aligned): the evaluations are read where the
 *   network left them.  A term whose coefficient is exactly 0 is SKIPPED — its y is not looked at, so a non-finite value of a region
 *   cannot reach a cell the region does not own; an element whose coefficients are all 0 is written 0.  The first term is the product
 *   alone, every further term one multiply then one add, never an fma: bit-equal to the same loop in numpy float32, and a cell owned
 *   by one region (coefficient 1.0f) is a bit copy.  One launch, every output element written once, no atomics; 16-byte accesses
 *   where P % 4 == 0 and the pointers allow, one element per access otherwise.
 */
int ccedit_region_weights(const void* masks, float* coef, int32_t K, int32_t T, int32_t H, int32_t W, int32_t F, void* stream);
int ccedit_region_fuse(const void* yr, float* out, const float* coef, int32_t K, int32_t B, int32_t C, int32_t T, int64_t P, void* stream);

/* ------------------------------------------------------------------------------------------
 * Automatic masks (added without an ABI bump: four new functions, CCEDIT_ABI_VERSION stays 12).  The edit mask of `--inpainting_mode`
 * from a source and a target prompt: the noised source latent is evaluated with (source prompt, target prompt) in the two halves of one
 * CFG-doubled batch, and where the two predictions disagree is where the edit happens (DiffEdit's mask step; ccedit_amd/automask.py;
 * `--mask_auto`, `--source_prompt`).  Kernels: csrc/automask.hip; definition: tests/_automask_numpy.py, reproduced bit for bit.  All
 * pointers are device pointers.  An invalid argument returns CCEDIT_EINVAL and launches nothing.
 *
 * ccedit_automask_accumulate: y fp32 [2B][C][P] (the source-prompt half first), acc fp32 [B][P], P = T h w, 1 <= C <= 16.
 *   s = ((|y[B+b][0][p] - y[b][0][p]| + |...[1]...|) + |...[2]...|) + ..., channels ascending, every subtract and add rounded to fp32;
 *   acc[b][p] = s with first = 1, acc[b][p] + s with first = 0.  A NaN in either half gives NaN.  16-byte accesses where P % 4 == 0 and
 *   y and acc are 16-byte aligned, one element per access otherwise.
 * ccedit_automask_binarize: bin[b][p] = acc[b][p] > theta * scale[b] ? 1 : 0, uint8 [B][P]; one fp32 multiply, strictly greater (a
 *   cell equal to the threshold, and a NaN, stay clear).  scale fp32 [B] is read from DEVICE memory (the result of ccedit_kth_values
 *   stays where it is: no host sync); theta finite and not negative.
 * ccedit_automask_vote: out[b][t][y][x] = (sum of bin[b][t+dt][y+dy][x+dx] != 0 over dt, dy, dx in {-1, 0, 1}, every coordinate clamped
 *   into the volume) >= votes ? 1 : 0; bin and out uint8 [B][T][h][w]; 1 <= votes <= 27.  out must not overlap bin.
 * ccedit_automask_expand: lat uint8 [N][h][w] (!= 0 is set) -> px uint8 [N][8h][8w] in {0, 255}, px 8-byte aligned; each lane writes the
 *   8 bytes of a cell's pixel row as one store.  ccedit_mask_latent of the result is lat's set cells as 1, byte for byte.
 */
int ccedit_automask_accumulate(const float* y, float* acc, int32_t B, int32_t C, int64_t P, int32_t first, void* stream);
int ccedit_automask_binarize(const float* acc, const float* scale, float theta, void* bin, int32_t B, int64_t P, void* stream);
int ccedit_automask_vote(const void* bin, void* out, int32_t B, int32_t T, int32_t h, int32_t w, int32_t votes, void* stream);
int ccedit_automask_expand(const void* lat, void* px, int64_t N, int32_t h, int32_t w, void* stream);

/* ------------------------------------------------------------------------------------------
 * Prompts (added without an ABI bump: one new function, CCEDIT_ABI_VERSION stays 12).  Long and weighted prompts: a prompt is cut into
 * n <= 4 chunks of 77 CLIP tokens, every chunk goes through the text encoder on its own and the rows are laid side by side — a context
 * of L = 77 n rows (ccedit_amd/prompt.py; `--prompt_chunks`, `--prompt_syntax weighted`).  Kernel: csrc/prompt.hip.  All pointers are
 * device pointers.
 *
 * ccedit_prompt_weight: out[b][t][c] = e[t mod 77][c] + w[b][t] * (z[b][t][c] - e[t mod 77][c]); z and out fp32 [B][L][C], L a multiple
 *   of 77; e fp32 [77][C], the encoding of the empty chunk (BOS, EOS x 76); w fp32 [B][L], the weight of every token.  fp32 subtract,
 *   multiply, add in that order, each rounded, never an fma: bit-equal to tests/_prompt_numpy.py.  A row with w == 1.0f is a BIT COPY of
 *   z (e + (z - e) is not z in floating point).  No reduction: a row depends on nothing but itself.  out may be z.  w is data: it must
 *   be finite (the Python wrapper refuses NaN / inf; the kernel has no index that depends on it).  One launch; 16-byte accesses where
 *   C % 4 == 0 and the pointers allow, one element per access otherwise.
 */
int ccedit_prompt_weight(const float* z, const float* e, const float* w, float* out, int32_t B, int32_t L, int32_t C, void* stream);

/* ------------------------------------------------------------------------------------------
 * Prompt schedules (added without an ABI bump: one new function and one flag of CcAttnDesc.flags, CCEDIT_ABI_VERSION stays 12).  A
 * prompt per time span of a clip (`--prompt_at`, `--prompt_ease`; ccedit_amd/schedule.py): the P distinct encoded prompts and a table
 * per keyframe become one text context per frame, which the spatial transformers' text attention then reads with kv_div = 1 and
 * CCEDIT_ATTN_KV_PER_FRAME.  Kernel: csrc/prompt.hip.
 *
 * ccedit_prompt_schedule: c fp32 [P][L][C] and out fp32 [N][L][C] are device pointers; k0, k1 (int32 [N], indices into the P prompts)
 *   and a (fp32 [N], 0 ... 1) are HOST tables.  out[f] = c[k0[f]] where a[f] == 0, c[k1[f]] where a[f] == 1 (both BIT COPIES, signed
 *   zeros included), otherwise c[k0[f]] + a[f] * (c[k1[f]] - c[k0[f]]): fp32 subtract, multiply, add in that order, each rounded, never
 *   an fma: bit-equal to tests/_schedule_numpy.py.  No reduction.  An index outside [0, P), an a outside [0, 1] or NaN is status -1
 *   before any launch (out is left untouched); the kernel receives the checked table by value.  One launch per 256 frames; 16-byte
 *   accesses where C % 4 == 0 and the pointers allow, one element per access otherwise.  out must not overlap c.
 */
int ccedit_prompt_schedule(const float* c, const int32_t* k0, const int32_t* k1, const float* a, float* out, int32_t P, int32_t N, int32_t L,
                           int32_t C, void* stream);

/* ------------------------------------------------------------------------------------------
 * Propagation (added without an ABI bump: four new functions, CCEDIT_ABI_VERSION stays 12).  Full-frame-rate output: the edited
 * keyframes are carried to every source frame between them along motion estimated on the source frames (ccedit_amd/propagate.py:
 * plan, tables, propagate_clip; `--propagate`).  Kernels: csrc/propagate.hip.  Everything is integer arithmetic on bytes and equals
 * tests/_propagate_numpy.py bit for bit.  Frames are uint8 [frames][H][W][3] (RGB) or [frames][H][W] (luma, masks), H and W multiples of
 * 64.  A PAIR is a row of four int32 on the device: (f, k, e, dist) — the frame that is produced, the keyframe it is matched against
 * (both numbers of source frames), the ordinal of that keyframe among the edited keyframes, and the weight of this side in the blend
 * (the distance to the OTHER keyframe).  The pairs of in-between frame j are rows 2 j (towards the earlier keyframe) and 2 j + 1.
 * Indices read from a pair are clamped into their tensor, `dist` into 1 ... 255, table entries into their range, block vectors into
 * +-32 (as a parent) / +-4096 (in the warp): no device table can take an access outside a tensor.
 *
 * ccedit_prop_pyramid: rgb [F][H][W][3] -> pyr: luma (77 R + 150 G + 29 B + 128) >> 8 as level 0 [F][H][W], then levels 1 ... 3, each the
 *   rounded mean (p00 + p01 + p10 + p11 + 2) >> 2 of the level before, [F][H >> l][W >> l], one after the other: F H W 85 / 64 bytes.
 *   rgb 4-byte, pyr 8-byte aligned.
 * ccedit_prop_match: one level, all P pairs in one launch.  Blocks are 8 x 8, the compared patch 16 x 16 (a 4-pixel apron, coordinates
 *   clamped).  Candidates (dy, dx) in +-radius (1 ... 4) around twice the vector of the parent block (by >> 1, bx >> 1) of vec_parent
 *   (null: around zero); the minimum of SAD * 256 + rank[(dy + radius) (2 radius + 1) + dx + radius] wins.  vec_out / vec_parent: int32
 *   [P][(H >> level) / 8][(W >> level) / 8][2] = (dy, dx), prediction included.
 * ccedit_prop_warp: out[p] = src[pair p, column col] sampled at 16 (y, x) + flow, clamped, bilinear with 4-bit fractions,
 *   (sum w p + 128) >> 8; flow (1/16 pixel) = the fixed-point bilinear interpolation of the level-0 block vectors `vec` around the
 *   block centres (t = 2 x - 7, blocks t >> 4 and its successor clamped, weights 16 - (t & 15) and t & 15, (sum + 8) >> 4).
 *   src [Fsrc][H][W][C], out [P][H][W][C], C = 3 or 1; col = 1 (source frames) or 2 (edited keyframes).  out 4-byte aligned.
 * ccedit_prop_blend: for in-between frame j: e = min(255, (5 x 5 edge-replicated box sum of |warped_luma[2 j + s] - luma of frame f| +
 *   12) / 25) per side s, w_s = dist_s gtab[e_s] (gtab: int32 [256], entries 1 ... 4096), out[j] = (w_0 A + w_1 B + (w_0 + w_1) / 2) /
 *   (w_0 + w_1) per channel of warped_rgb[2 j], [2 j + 1].  With rgb [F][H][W][3] and mask [F][H][W] (both or neither): the source pixel
 *   where frame f's mask byte is < 128.  warped_rgb [2 NF][H][W][3], warped_luma [2 NF][H][W], pyr as written by ccedit_prop_pyramid.
 */
int ccedit_prop_pyramid(const void* rgb, void* pyr, int32_t F, int32_t H, int32_t W, void* stream);
int ccedit_prop_match(const void* pyr, const int32_t* pairs, const int32_t* rank, const int32_t* vec_parent, int32_t* vec_out, int32_t P, int32_t F,
                      int32_t H, int32_t W, int32_t level, int32_t radius, void* stream);
int ccedit_prop_warp(const void* src, const int32_t* vec, const int32_t* pairs, int32_t col, void* out, int32_t P, int32_t Fsrc, int32_t H, int32_t W,
                     int32_t C, void* stream);
int ccedit_prop_blend(const void* warped_rgb, const void* warped_luma, const void* pyr, const int32_t* pairs, const int32_t* gtab, const void* rgb,
                      const void* mask, void* out, int32_t NF, int32_t F, int32_t H, int32_t W, void* stream);

/* ------------------------------------------------------------------------------------------
 * Mask tracking (added without an ABI bump: three new functions, CCEDIT_ABI_VERSION stays 12).  `--mask_track`: an edit mask painted
 * on one source frame is carried to every frame of the clip along the source's motion (ccedit_amd/masktrack.py: constants, pair lists,
 * track_clip).  Kernels: csrc/masktrack.hip, and ccedit_mask_dilate in csrc/mask.hip.  Everything is integer arithmetic on bytes and
 * equals tests/_masktrack_numpy.py bit for bit.  Frames, pyramids and pairs are those of "Propagation" above (of a pair row only
 * (f, k) are read).  A PER-PIXEL VECTOR is two int16 (dy, dx), [H][W][2].
 *
 * ccedit_masktrack_select: all P pairs in one launch.  pyr as written by ccedit_prop_pyramid (level 0 is read), vec: the level-0 block
 *   vectors int32 [P][H / 8][W / 8][2] of ccedit_prop_match, each component clamped into +-64 before use.  Per pixel p of block
 *   (y >> 3, x >> 3): the candidates are the vectors of the 3 x 3 neighbouring blocks (indices clamped) in the order (dby, dbx) = (0,0)
 *   (-1,0) (0,-1) (0,1) (1,0) (-1,-1) (-1,1) (1,-1) (1,1); S_c(p) = the 5 x 5 edge-replicated box sum of d_c = |Y_f(p') - Y_k(clamp(p' + c))|;
 *   the candidate of minimum S_c * 16 + order is written to vsel [P][H][W][2] (int16, 4-byte aligned).
 * ccedit_masktrack_step: one frame of the chain.  v, r: per-pixel vectors [H][W][2] of the pairs (f, g) and (g, f); q = clamp(p + v(p));
 *   mask_f(p) = mask_g(q), or 0 where |v_y(p) + r_y(q)| + |v_x(p) + r_x(q)| > limit.  v 16-byte, r and mask_f 4-byte aligned.
 * ccedit_mask_dilate: uint8 masks [N][H][W] (W % 4 == 0, 4-byte aligned) -> dst: the (2 radius + 1)^2 square maximum, the window clipped
 *   at the border (radius 0 ... 32; two separable passes through tmp [N][H][W], which may be null with radius 0), then, with invert = 1,
 *   255 - m.  src, tmp and dst are three different buffers.
 */
int ccedit_masktrack_select(const void* pyr, const int32_t* pairs, const int32_t* vec, void* vsel, int32_t P, int32_t F, int32_t H, int32_t W,
                            void* stream);
int ccedit_masktrack_step(const void* v, const void* r, const void* mask_g, void* mask_f, int32_t H, int32_t W, int32_t limit, void* stream);
int ccedit_mask_dilate(const void* src, void* tmp, void* dst, int64_t N, int32_t H, int32_t W, int32_t radius, int32_t invert, void* stream);

/* ------------------------------------------------------------------------------------------
 * Graded edit masks (added without an ABI bump: four new functions, CCEDIT_ABI_VERSION stays 12).  `--mask_graded`, `--mask_feather`:
 * a STRENGTH MAP is a uint8 pixel map, byte g = edit strength g / 255 (255: what a white mask pixel is, 0: a black one).  Kernels:
 * csrc/softmask.hip; the level re-injection is csrc/mask.hip's select kernel with the caller's threshold.  Feather and latent
 * strengths are integer arithmetic, the composite is four fp32 roundings; all equal tests/_softmask_numpy.py bit for bit.
 * Thresholds per step: ccedit_amd/softmask.py.  All pointers are device pointers.
 *
 * ccedit_mask_feather: uint8 maps [N][H][W] (W % 4 == 0, 4-byte aligned) -> dst: the mean over the (2 radius + 1)^2 square, the window
 *   clipped at the frame border, rounded half up: with S the sum of the bytes of the clipped window and A its pixel count,
 *   (2 S + A) / (2 A) in integers (radius 0 ... 64; 0 copies).  Two separable passes: row sums into tmp16, uint16 [N][H][W] (at most
 *   129 * 255 = 32 895), column sums in uint32.  Per map: nothing crosses from one of the N maps to the next.  src, tmp16 and dst are
 *   three different buffers.
 * ccedit_mask_latent_graded: pixel strengths uint8 [N][H][W] (H % 8 == W % 8 == 0, 8-byte aligned) -> latent strengths uint8
 *   [N][H/8][W/8]: (sum of the 64 bytes of the 8 x 8 cell + 32) >> 6; a white cell gives 255, a black one 0.
 * ccedit_mask_composite_graded: out = g == 255 ? result : g == 0 ? original : original + (result - original) * (float(g) / 255.0f) over
 *   fp32 [B][3][P] (P = T H W) with the strengths uint8 [B][P] broadcast over the three channels: one IEEE divide, one subtract, one
 *   multiply, one add, not contracted.  For a 0 / 255 map bit-equal to ccedit_mask_composite.  out may alias result.
 * ccedit_inpaint_blend_level: ccedit_inpaint_blend with m = (strength byte >= thr), thr 1 ... 255: y = m ? x : (x0 + noise * sigma) / s.
 *   Before walked step j of n a graded run passes thr = (255 (n - j) + n - 1) / n: a cell of strength L is free iff L n >= 255 (n - j).
 */
int ccedit_mask_feather(const void* src, void* tmp16, void* dst, int64_t N, int32_t H, int32_t W, int32_t radius, void* stream);
int ccedit_mask_latent_graded(const void* mask_px, void* strength_lat, int64_t N, int32_t H, int32_t W, void* stream);
int ccedit_mask_composite_graded(const float* result, const float* original, const void* strength_px, float* out, int32_t B, int64_t P,
                                 void* stream);
int ccedit_inpaint_blend_level(const float* x, const float* x0, const float* noise, const void* strength, float* y, int32_t B, int32_t C,
                               int64_t P, int32_t thr, float sigma, float s, void* stream);

/* ------------------------------------------------------------------------------------------
 * Motion-following noise (added without an ABI bump: five new functions, CCEDIT_ABI_VERSION stays 12).  `--noise_warp`: once per clip
 * it is decided which noise sample every latent cell (8 x 8 pixels) of every keyframe inherits from an earlier keyframe along the
 * source's motion, and every noise draw of the run is gathered through that decision (ccedit_amd/noisewarp.py: constants, build, wrap).
 * Kernels: csrc/noisewarp.hip.  Integer arithmetic and bit copies; all equal tests/_noisewarp_numpy.py bit for bit.  A clip is F
 * source frames of H x W (multiples of 64) with K keyframes; h = H / 8, w = W / 8, cells = h w, K cells < 2^31; the centre of cell
 * (i, j) is the pixel (8 i + 4, 8 j + 4).  All pointers are device pointers; device data is held in range by the kernels.
 *
 * ccedit_noisewarp_track: vec: block vectors int32 [2 (F - 1)][h][w][2] of ccedit_prop_match, for frame f >= 1 row 2 (f - 1) is the pair
 *   (f, f - 1) and row 2 (f - 1) + 1 the pair (f - 1, f); every component is clamped into +-64 where it is read.  key: int32 [K], the
 *   keyframes' frame numbers, key[0] = 0, strictly increasing.  One thread per (k >= 1, cell): p = the cell's centre; for f = key[k]
 *   down to key[k - 1] + 1: v = vec(f -> f - 1) at cell p >> 3, q = p + v, inside = q lies in the frame, q is clamped into it,
 *   r = vec(f - 1 -> f) at cell q >> 3, valid &= inside & (|v_y + r_y| + |v_x + r_x| <= limit), p = q.  track [K][cells][3] =
 *   (valid, Q_y, Q_x); row 0 is not written.
 * ccedit_noisewarp_claim: keyframe k >= 1.  A cell with valid track: c' = Q >> 3, (R', P') = org[k - 1][c'], P = P' + Q - centre(c');
 *   where P lies in the frame it bids atomicMax(table[R' cells + (P_y >> 3) w + (P_x >> 3)], k cells + (cells - 1 - idx) + 1).
 *   table: uint32 [K cells], zeroed once per clip.
 * ccedit_noisewarp_resolve: keyframe k, after its claim (k = 0: no claim, nothing is read).  A cell whose own bid the table holds gets
 *   org[k][idx] = (R', P), every other cell (k, own centre); src[k][idx] = R cells + (P_y >> 3) w + (P_x >> 3); inherited[k] (uint32 [K],
 *   zeroed once per clip) += the number of cells with R != k.  org [K][cells][3], src [K][cells].  Claim and resolve of the keyframes
 *   run in order on one stream: the kernel boundary is the ordering.
 * ccedit_noisewarp_check: CCEDIT_EINVAL where any of the maps' indices src [maps][N] lies outside 0 ... N - 1.  flag: one uint32 of
 *   workspace.  Waits for the stream (one word comes back to the host): once per map, not per draw.
 * ccedit_noise_warp: out[b][c][n] = raw[b][c][src[b][n]] over fp32 [B][C][N] moved as 32-bit words (NaN payloads survive), src int32
 *   [B][N], one map per clip; an index is held inside 0 ... N - 1.  16-byte stores where N % 4 == 0 and src and out are 16-byte aligned,
 *   4-byte accesses otherwise.  raw and out are two buffers.
 */
int ccedit_noisewarp_track(const int32_t* vec, const int32_t* key, int32_t* track, int32_t K, int32_t F, int32_t H, int32_t W, int32_t limit,
                           void* stream);
int ccedit_noisewarp_claim(const int32_t* track, const int32_t* org, void* table, int32_t k, int32_t K, int32_t H, int32_t W, void* stream);
int ccedit_noisewarp_resolve(const int32_t* track, int32_t* org, const void* table, int32_t* src, void* inherited, int32_t k, int32_t K,
                             int32_t H, int32_t W, void* stream);
int ccedit_noisewarp_check(const int32_t* src, int64_t maps, int64_t N, void* flag, void* stream);
int ccedit_noise_warp(const float* raw, const int32_t* src, float* out, int32_t B, int32_t C, int64_t N, void* stream);

/* ------------------------------------------------------------------------------------------
 * Quality report (added without an ABI bump: two new functions, CCEDIT_ABI_VERSION stays 12).  `--report_quality`: how faithful a
 * result is to its source (squared error, SSIM) and how steady a clip is along the source's motion (warp error); ccedit_amd/quality.py:
 * constants, compare, temporal, report.  Kernels: csrc/quality.hip.  Everything is integer arithmetic with 64-bit accumulators and
 * equals tests/_quality_numpy.py bit for bit; PSNR, SSIM and the means are formed from the exact integers on the host.  Frames are
 * uint8 [frames][H][W][3], masks uint8 [frames][H][W] (>= 128 = edited).  All pointers are device pointers; both functions zero acc
 * themselves, ordered on the stream.
 *
 * ccedit_quality_pair: a, b [N][H][W][3], mask [N][H][W] or null; a pixel is KEPT where mask is null or its byte is < 128.  H and W
 *   multiples of 4, 8 ... 16384; a, b, mask 4-byte, acc 8-byte aligned.  acc uint64 [N][8], per frame: [0 .. 2] sum of (a - b)^2 over the
 *   kept pixels for R, G, B; [3] the kept pixels; [4] sum of q over the counted windows (int64, two's complement); [5] the counted
 *   windows; [6], [7] sum of the luma (77 R + 150 G + 29 B + 128) >> 8 of a and of b over the kept pixels.  Windows: 8 x 8 at stride 4,
 *   at (4 i, 4 j) with 4 i + 8 <= H and 4 j + 8 <= W; a window counts iff all its 64 pixels are kept.  Per window over the lumas:
 *   s1 = sum a, s2 = sum b, saa, sbb, sab; va = 64 saa - s1^2, vb = 64 sbb - s2^2, cov = 64 sab - s1 s2; c1 = 26634, c2 = 239708
 *   ((0.01 * 255)^2 and (0.03 * 255)^2 times 4096); Nw = (2 s1 s2 + c1)(2 cov + c2), Dw = (s1^2 + s2^2 + c1)(va + vb + c2), both below
 *   2^63, |Nw| <= Dw; q = sign(Nw) floor(|Nw| 2^32 / Dw) exactly (an integer part of 0 or 1 and 32 shift-subtract steps; no
 *   floating-point divide).  Identical frames give q = 2^32 in every window.
 * ccedit_quality_warp: x [F][H][W][3], the sequence measured; y: a second one of the same shape that shares the vectors, or null;
 *   pairs int32 [2 P][4]: row 2 j = (f, g, ., .), row 2 j + 1 = (g, f, ., .) (ccedit_amd/masktrack.py pair_rows; f and g of row 2 j are
 *   read and clamped into 0 ... F - 1); vsel int16 [2 P][H][W][2] as ccedit_masktrack_select writes it for those rows (16-byte aligned);
 *   mask [F][H][W] or null; sel: 0 all pixels, 1 mask_f(p) >= 128, 2 mask_f(p) < 128 (sel != 0 with a null mask: status -1).  H and W as
 *   in "Propagation".  Per selected pixel p of frame f: v = vsel[2 j](p), q0 = p + v, inside = q0 lies in the frame, q = clamp(q0),
 *   r = vsel[2 j + 1](q), valid = inside and |v_y + r_y| + |v_x + r_x| <= limit.  acc uint64 [P][4], per measurement: sum over the valid
 *   pixels and the channels of (x_f(p) - x_g(q))^2, the same of y (0 where y is null), the valid pixels, the selected pixels.  Every
 *   access stays in range for any int16 content of vsel and any int32 content of pairs.
 */
int ccedit_quality_pair(const void* a, const void* b, const void* mask, void* acc, int64_t N, int32_t H, int32_t W, void* stream);
int ccedit_quality_warp(const void* x, const void* y, const void* vsel, const int32_t* pairs, const void* mask, void* acc, int32_t P, int32_t F,
                        int32_t H, int32_t W, int32_t limit, int32_t sel, void* stream);

/* ------------------------------------------------------------------------------------------
 * Motion-JPEG (added without an ABI bump: five new functions, CCEDIT_ABI_VERSION stays 12).  `--save_type mjpeg`: uint8 frames
 * [N][H][W][3] on the device (what ccedit_frames_to_u8 writes) -> one baseline JPEG per frame (ITU-T T.81: sequential DCT, 8 bit,
 * YCbCr 4:2:0, MCU 16 x 16, restart interval = one MCU row = one SEGMENT), ccedit_amd/mjpeg.py: constants, header, container.
 * Kernels: csrc/mjpeg.hip.  Everything is integer arithmetic and equals tests/_mjpeg_numpy.py byte for byte.  H and W are multiples
 * of 16, 16 ... 65520.  `tables`: int32 [816] from ccedit_amd/mjpeg.py (table_array: [0] base quantisation tables 2 x 64 row-major,
 * [128] zigzag, [192] FDCT matrix 8 x 8 at 13 bits, [256] nine colour factors at 16 bits, [272] DC codes 2 x 16 by size, [304] AC codes
 * 2 x 256 by run << 4 | size; a code is code << 8 | length).  Values read from it are held in range by the kernels (indices masked,
 * quantisers 1 ... 255, lengths <= 16), as are the segment lengths and offsets the pack functions read: no device table can take an
 * access outside a buffer.  A block codes to at most 63 x 26 + 27 bits whatever the tables hold; nothing is ever truncated.
 *
 * ccedit_mjpeg_segment_bytes: bytes of one segment's slot in `segments` (all its blocks at that bound, every byte stuffed), a
 *   multiple of 16; -1 for a W that is no multiple of 16.
 * ccedit_mjpeg_transform: frames -> coef int16 [N][H / 16][W / 16][6][64]: per MCU the blocks Y00 Y01 Y10 Y11 Cb Cr, each in zigzag
 *   order, quantised by the base tables scaled to `quality` (1 ... 100): q = sign(F) ((|F| + (Q << 17)) >> 18) / Q, AC clamped to
 *   +-1023.  frames and coef 16-byte aligned.
 * ccedit_mjpeg_entropy: coef -> the stuffed, padded entropy-coded bytes of segment i at segments + i * segment_bytes, its length in
 *   seg_len[i] (int32 [N * H / 16]).  DC predictors start at 0 in every segment; DC differences are clamped to +-2047.
 * ccedit_mjpeg_pack_scan: seg_len -> seg_off (int64 [N * H / 16]: where each segment starts in the packed output, the frames back to
 *   back, each `hdr_len` header bytes, its segments separated by RSTn, EOI) and frame_bytes (int32 [N]).
 * ccedit_mjpeg_pack: copies header, segments and markers into out (out_bytes = the sum of frame_bytes).
 */
int64_t ccedit_mjpeg_segment_bytes(int32_t W);
int ccedit_mjpeg_transform(const void* frames, const int32_t* tables, void* coef, int32_t N, int32_t H, int32_t W, int32_t quality, void* stream);
int ccedit_mjpeg_entropy(const void* coef, const int32_t* tables, void* segments, int32_t* seg_len, int32_t N, int32_t H, int32_t W, void* stream);
int ccedit_mjpeg_pack_scan(const int32_t* seg_len, int64_t* seg_off, int32_t* frame_bytes, int32_t N, int32_t H, int32_t W, int32_t hdr_len,
                           void* stream);
int ccedit_mjpeg_pack(const void* segments, const int32_t* seg_len, const int64_t* seg_off, const void* header, void* out, int32_t N, int32_t H,
                      int32_t W, int32_t hdr_len, int64_t out_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * JPEG decoding (added without an ABI bump: four new functions, CCEDIT_ABI_VERSION stays 12).  The JPEG sources of the entry points
 * (a directory of .jpg frames, a Motion-JPEG .avi) decoded on the device: the entropy-coded bytes of N baseline JPEG frames of ONE
 * geometry and ONE set of tables -> uint8 frames [N][H][W][3].  ccedit_amd/jpegdec.py parses the streams on the host (markers, tables,
 * where each restart interval lies) and refuses what is outside the subset before any call.  Kernels: csrc/jpegdec.hip; the entropy
 * stage's decode core is csrc/jpegdec_core.h, plain C++ that a host program compiles too.  Everything is integer arithmetic and equals
 * tests/_jpegdec_numpy.py byte for byte, which equals libjpeg(-turbo)'s accurate integer IDCT, "fancy" up-sampling and YCbCr -> RGB.
 *
 * Geometry: H, W 1 ... 65520; ncomp 1 (greyscale; hs and vs are ignored, a one-component scan is not interleaved) or 3 (YCbCr, luma
 * sampling hs x vs = 1x1, 2x1 or 2x2, chroma 1x1).  An MCU is 8 hs x 8 vs pixels: hs * vs luma blocks (row by row), then Cb, then Cr.
 * restart_interval: MCUs per restart interval, 0 = the whole frame is one interval.  I = intervals per frame = ceil(MCUs / interval).
 * One call takes N frames of fewer than 2^31 pixels, 2^31 blocks and 2^33 bytes of planes in all (what one launch per stage can index);
 * ccedit_amd/jpegdec.py cuts a clip into calls far below that.
 * `tables`: int32 [3416] from ccedit_amd/jpegdec.py (table_array: [0] quantisation tables 3 x 64 per COMPONENT in natural order, 0 ... 255;
 * [192] six selectors, the DC table of component 0 1 2 and the AC table of component 0 1 2, each 0 or 1; [200] four Huffman tables DC 0,
 * DC 1, AC 0, AC 1 of 804 words: lut [512] by the next 9 bits, length << 8 | symbol; maxcode [18] by length, -1 = none; valoff [18];
 * values [256]).  It is device data: every value that becomes an index is masked to its table.
 *
 * ccedit_jpegdec_plane_bytes: bytes of one frame's component planes (padded to whole MCUs: luma, then Cb, Cr), a multiple of 64;
 *   -1 for a geometry outside the above.
 * ccedit_jpegdec_entropy: data (data_bytes bytes) holds the entropy-coded bytes; intervals int64 [N * I][2] are the [start, end) of each
 *   restart interval in it (clamped into the buffer by the kernel).  One thread per interval decodes its MCUs into coef, int16
 *   [N][blocks][64] in MCU order, natural (row-major) order inside a block, 16-byte aligned, zeroed by the call itself; the DC prediction
 *   starts at 0 in every interval.  status int32 [N * I]: 0, or why the interval stopped (1 invalid Huffman code, 2 the data ends before
 *   the interval's blocks do, 3 a coefficient index passes 63, 4 DC size category above 11).  No read leaves [start, end), no write
 *   leaves the interval's blocks, whatever the bytes are.
 * ccedit_jpegdec_idct: coef -> planes uint8 [N][plane_bytes], 8-byte aligned: dequantisation, inverse DCT, level shift, clamp.
 * ccedit_jpegdec_rgb: planes -> out uint8 [N][H][W][3]: chroma up-sampling over the component's real size (ceil(W / hs) x ceil(H / vs)),
 *   YCbCr -> RGB; greyscale is replicated to the three channels.
 */
int64_t ccedit_jpegdec_plane_bytes(int32_t H, int32_t W, int32_t ncomp, int32_t hs, int32_t vs);
int ccedit_jpegdec_entropy(const void* data, int64_t data_bytes, const int64_t* intervals, const int32_t* tables, void* coef, int32_t* status,
                           int32_t N, int32_t H, int32_t W, int32_t ncomp, int32_t hs, int32_t vs, int32_t restart_interval, void* stream);
int ccedit_jpegdec_idct(const void* coef, const int32_t* tables, void* planes, int32_t N, int32_t H, int32_t W, int32_t ncomp, int32_t hs,
                        int32_t vs, void* stream);
int ccedit_jpegdec_rgb(const void* planes, void* out, int32_t N, int32_t H, int32_t W, int32_t ncomp, int32_t hs, int32_t vs, void* stream);

/* ------------------------------------------------------------------------------------------
 * GIF (added without an ABI bump: seven new functions, CCEDIT_ABI_VERSION stays 12).  `--gif_encoder device`: uint8 frames [N][H][W][3]
 * on the device (what ccedit_frames_to_u8 writes) -> per frame a palette of 256 colours, the pixels' indices and their LZW byte stream;
 * ccedit_amd/gif.py: constants, the frame loop, the container.  Kernels: csrc/gif.hip.  Every byte equals tests/_gif_numpy.py.
 * H and W are 1 ... 65535 with H * W <= 2^24; N <= 65535.
 *
 * The palette is Wu's variance-minimising quantiser on a grid of 32^3 cells (cell = r >> 3, g >> 3, b >> 3).  `moments`: int64
 * [N][5][33][33][33], index [cell r + 1][cell g + 1][cell b + 1] with a zero border: count, sum r, sum g, sum b, sum r^2 + g^2 + b^2 of
 * the full 8-bit values.  A box is (r0, r1] x (g0, g1] x (b0, b1] on that grid; (0, 32]^3 is cut up to 255 times.  The next box to cut is
 * the lowest-indexed one of maximal score (the variance m2 - (dr^2 + dg^2 + db^2) / w in float64; 0 for a box of one cell), until that
 * maximum is <= 0.  A cut position's score is (hr hr + hg hg + hb hb) / hw + (or or + og og + ob ob) / ow over the two halves, float64
 * from int64 operands, products summed left to right, IEEE division, no multiply-add contraction; positions with an empty half are
 * skipped; per direction the strictly greater score wins (the lowest position on ties); direction r if its best >= both others, else
 * g if its best >= both others, else b.  A box that cannot be cut gets score 0 and consumes no palette entry.
 *
 * ccedit_gif_slot_bytes: bytes of one chunk's slot in `slots` (chunk + 2 codes of 12 bits, a multiple of 16).
 * ccedit_gif_histogram: frames -> moments (zeroed by the call itself), 8-byte aligned.  Integer atomics: no dependence on the order.
 * ccedit_gif_palette: moments -> their inclusive 3-D prefix sums IN PLACE, then the cuts -> cells uint8 [N][32][32][32] (cell -> box =
 *   palette index) and palettes uint8 [N][256][3]: the box means (sum + w / 2) / w, unused entries 0.
 * ccedit_gif_map: frames, cells -> indices uint8 [N][H][W]; there is no nearest-colour search.
 * ccedit_gif_lzw: indices -> LZW codes.  A frame's H * W indices in raster order are cut into chunks of `chunk` pixels (1 ... 3072; the
 *   encoder uses 3072), C = ceil(H W / chunk) per frame, each coded from an empty dictionary (9 bits, next code 258).  After every code
 *   (the chunk's last one included) an entry is counted, and the width grows when the next free code exceeds 1 << width.  A chunk ends
 *   with Clear (256) at that width, a frame's last chunk with EOI (257); a frame's first chunk starts with Clear at 9 bits.  Codes are
 *   packed LSB first into chunk i's slot at slots + i * slot_bytes (4-byte aligned), its bit length goes to chunk_bits[i] (int32 [N * C]).
 * ccedit_gif_pack_scan: chunk_bits (clamped into the slot) -> chunk_off (int64 [N * C]: the bit offset of every chunk in the packed
 *   output, the frames back to back, each zero-padded to a byte) and frame_bytes (int32 [N]).
 * ccedit_gif_pack: the chunks' bits shifted to their offsets in out (out_bytes = the sum of frame_bytes; the buffer holds out_bytes
 *   rounded up to a multiple of 4, 4-byte aligned, zeroed by the call itself).  A chunk whose bits would leave the output is skipped.
 */
int64_t ccedit_gif_slot_bytes(void);
int ccedit_gif_histogram(const void* frames, int64_t* moments, int32_t N, int32_t H, int32_t W, void* stream);
int ccedit_gif_palette(int64_t* moments, void* cells, void* palettes, int32_t N, void* stream);
int ccedit_gif_map(const void* frames, const void* cells, void* indices, int32_t N, int32_t H, int32_t W, void* stream);
int ccedit_gif_lzw(const void* indices, void* slots, int32_t* chunk_bits, int32_t N, int32_t H, int32_t W, int32_t chunk, void* stream);
int ccedit_gif_pack_scan(const int32_t* chunk_bits, int64_t* chunk_off, int32_t* frame_bytes, int32_t N, int32_t H, int32_t W, int32_t chunk,
                         void* stream);
int ccedit_gif_pack(const void* slots, const int32_t* chunk_bits, const int64_t* chunk_off, void* out, int32_t N, int32_t H, int32_t W,
                    int32_t chunk, int64_t out_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * PNG (added without an ABI bump: nine new functions, CCEDIT_ABI_VERSION stays 12).  `--save_type png`: uint8 frames [N][H][W][3] on the
 * device (what ccedit_frames_to_u8 writes) -> per frame the deflate bits and the Adler-32 of its filtered rows; ccedit_amd/png.py:
 * constants, the frame loop, the zlib wrapper (78 01 ... Adler) and the PNG / APNG container.  Kernels: csrc/png.hip, csrc/png_huff.h.
 * Every byte equals tests/_png_numpy.py, which states the rules in full.  H and W are 1 ... 65535 with H * W <= 2^24; N <= 65535.
 *
 * The stages after the filter take N byte streams of L bytes each (L = H * (1 + 3 W) for frames; 1 ... 65535 + 3 * 2^24), cut into
 * C = ceil(L / chunk) chunks of ccedit_png_chunk_bytes() bytes, N * C <= 2^22; chunk i = stream * C + chunk number.  Each chunk becomes
 * ONE dynamic-Huffman deflate block; BFINAL is set on a stream's last chunk.
 *
 * ccedit_png_chunk_bytes / ccedit_png_slot_bytes: bytes of a chunk (16384), and of one chunk's slot in `slots` (the worst-case header,
 *   16 bits per byte, end-of-block; a multiple of 16).
 * ccedit_png_filter: frames -> filtered uint8 [N][H][1 + 3 W]: per row the filter byte (0 None, 1 Sub, 2 Up, 3 Average, 4 Paeth: the
 *   smallest sum of min(v, 256 - v) over the row, the lowest number on a tie) and the filtered bytes; the row above row 0 is zeros.
 * ccedit_png_tokens: filtered [N][L] -> tokens uint32 [N * C][chunk] (a literal's byte, or 1 << 31 | (length - 3) << 16 | (distance - 1)),
 *   ntok int32 [N * C] and hist uint32 [N * C][320] (literal/length symbols at 0, end-of-block counted once; distance symbols at 288).
 *   Greedy LZ77 inside the chunk over a single-entry hash table of 4096 positions; matches of 3 ... 258 bytes.
 * ccedit_png_codes: hist -> codes uint32 [N * C][320] (length << 16 | the canonical code, bits reversed; lengths <= 15), header uint32
 *   [N * C][144] (the block header's bits, LSB first: BFINAL, BTYPE = 2, HLIT, HDIST, HCLEN, the code-length code (<= 7 bits), the
 *   run-coded lengths), header_bits and chunk_bits int32 [N * C] (header + tokens + end-of-block).
 * ccedit_png_emit: tokens, ntok, codes, header, header_bits -> chunk i's bits at slots + i * slot_bytes (4-byte aligned, zeroed by the
 *   call itself); `chunks` = N * C.
 * ccedit_png_pack_scan / ccedit_png_pack: as the GIF pair: chunk_bits (clamped into the slot) -> chunk_off int64 [N * C] and frame_bytes
 *   int32 [N] (a stream's bits zero-padded to a byte); the chunks' bits shifted to their offsets in out (out_bytes = the sum of
 *   frame_bytes; the buffer holds out_bytes rounded up to a multiple of 4, 4-byte aligned, zeroed by the call itself).
 * ccedit_png_adler: filtered [N][L] -> adler uint32 [N] (s2 << 16 | s1); partials: uint32 [N * C][2] of scratch (per chunk the sums
 *   of d[k] and of (n - k) d[k] mod 65521).
 */
int64_t ccedit_png_chunk_bytes(void);
int64_t ccedit_png_slot_bytes(void);
int ccedit_png_filter(const void* frames, void* filtered, int32_t N, int32_t H, int32_t W, void* stream);
int ccedit_png_tokens(const void* filtered, uint32_t* tokens, int32_t* ntok, uint32_t* hist, int32_t N, int64_t L, void* stream);
int ccedit_png_codes(const uint32_t* hist, uint32_t* codes, uint32_t* header, int32_t* header_bits, int32_t* chunk_bits, int32_t N, int32_t C,
                     void* stream);
int ccedit_png_emit(const uint32_t* tokens, const int32_t* ntok, const uint32_t* codes, const uint32_t* header, const int32_t* header_bits,
                    void* slots, int64_t chunks, void* stream);
int ccedit_png_pack_scan(const int32_t* chunk_bits, int64_t* chunk_off, int32_t* frame_bytes, int32_t N, int32_t C, void* stream);
int ccedit_png_pack(const void* slots, const int32_t* chunk_bits, const int64_t* chunk_off, void* out, int32_t N, int32_t C, int64_t out_bytes,
                    void* stream);
int ccedit_png_adler(const void* filtered, uint32_t* partials, uint32_t* adler, int32_t N, int64_t L, void* stream);

/* ------------------------------------------------------------------------------------------
 * PNG decoding (added without an ABI bump: two new functions, CCEDIT_ABI_VERSION stays 12).  PNG sources (frame files, the frames of an
 * animated .png) -> uint8 frames [N][H][W][3] on the device; only the compressed bytes go up.  ccedit_amd/pngdec.py: the chunk parser
 * (signature, CRCs, IHDR, IDAT / fdAT) and the frame loop.  Kernels: csrc/pngdec.hip, csrc/pngdec_core.h.  The subset: bit depth 8,
 * colour type 2, no interlace; H and W 1 ... 65535 with H * W <= 2^24; N <= 65535.  L = H * (1 + 3 W).
 *
 * Both calls write one int32 pair per image to `status`: a code (0: decoded; the codes are pngdec_core.h's Status) and the byte
 * position that goes with it.  An image with a non-zero code is not complete; nothing outside the buffers below is read or written.
 *
 * ccedit_pngdec_inflate: N zlib streams -> N filtered images of exactly L bytes each.  data: uint8 [data_bytes], every stream's bytes;
 *   streams: int64 [N][2] on the device, (offset, length) of each stream in data (clamped into it); filtered: uint8 [N][L].  The full
 *   format: zlib header (CM 8, window <= 32 KiB, no FDICT, FCHECK), stored, fixed and dynamic blocks in any sequence, distances up to
 *   32768, lengths up to 258, overlapping copies, the trailing Adler-32 (verified).  Codes: 1 bad zlib header, 2 the stream runs past
 *   its input, 3 block type 3, 4 a stored block's LEN / NLEN disagree, 5 an over-subscribed or incomplete code (or too many symbols, or
 *   no end-of-block code), 6 bad code-length runs, 7 bits that are no code / symbol 286, 287 / distance code 30, 31, 8 a distance that
 *   reaches before the start, 9 the output would pass L, 10 the output ends short of L, 11 Adler-32 mismatch.  Position: the stream's
 *   input bytes touched when it stopped (code 2: its length; code 11: where the trailer begins; code 1: 0).  One wave per stream.
 * ccedit_pngdec_unfilter: filtered [N][L] -> rgb uint8 [N][H][W][3]: per row the filter byte (0 None, 1 Sub, 2 Up, 3 Average with
 *   floor, 4 Paeth with the specification's tie order; bpp 3; the row above row 0 is zeros) undone.  Code 12: a filter byte above 4,
 *   position: that byte's offset in the image's L bytes; the image's rows from the 64-row band that holds it on are not written.
 */
int ccedit_pngdec_inflate(const void* data, int64_t data_bytes, const int64_t* streams, void* filtered, int32_t* status, int32_t N, int32_t H,
                          int32_t W, void* stream);
int ccedit_pngdec_unfilter(const void* filtered, void* rgb, int32_t* status, int32_t N, int32_t H, int32_t W, void* stream);

/* ------------------------------------------------------------------------------------------
 * GIF decoding (added without an ABI bump: three new functions, CCEDIT_ABI_VERSION stays 12).  The images of one .gif -> uint8 frames
 * [n_out][H][W][3] on the device, composited on a canvas [H][W][3] that the caller carries from call to call; only the compressed bytes,
 * the palettes and one descriptor per image go up.  ccedit_amd/gifdec.py: the container parser and the frame loop.  Kernels:
 * csrc/gifdec.hip, csrc/gifdec_core.h.  H and W 1 ... 65535 with H * W <= 2^24; N <= 65535.
 *
 * data: uint8 [data_bytes]: every image's LZW stream (its sub-blocks concatenated) and every palette (RGB triples).
 * desc: int64 [N][16] on the device, per image: 0 x, 1 y, 2 w, 3 h (its rectangle on the canvas), 4 interlace flag, 5 transparent
 *   index or -1, 6 byte offset of its palette in data, 7 palette entries (1 ... 256), 8 LZW minimum code size (2 ... 8), 9 and 10 byte
 *   offset and length of its stream in data, 11 and 12 offset and capacity of its part of the code table (capacity >= min(w * h,
 *   8 * length / (min code size + 1)) + 1), 13 byte offset of its w * h indices in planes, 14 the output it is written to or -1,
 *   15 zero.  A descriptor that points outside a buffer or the canvas gives code 6 and is not used.
 * status: int32 [N][2] per call: a code (0: fine; the codes are gifdec_core.h's Status) and a position.
 *
 * ccedit_gifdec_codes: the bit streams -> the code table, without touching a pixel.  For data code k of an image (Clear and EOI are not
 *   counted): parent[k] (a code of the same image, -1: a literal), len[k] (its string's length), first[k] / last[k] (its string's first
 *   and last byte), off[k] (its pixel offset in stream order); ncodes[n]: the codes of image n.  Decoding stops at EOI or once w * h
 *   pixels are reached (the code that crosses the end keeps its full length).  Codes: 1 a code above the next free entry, 2 a first code
 *   after Clear that is not a literal, 3 the stream ends before w * h pixels, 4 minimum code size outside 2 ... 8; position: the bit
 *   position of the code.  One wave per image.
 * ccedit_gifdec_pixels: the code table -> planes uint8 [plane_bytes]: every image's indices in stream order.  One lane per code, one hop
 *   up the chain of parents per pixel.  max_codes: the largest capacity among the descriptors.
 * ccedit_gifdec_compose: for every canvas pixel, the images in order: inside the rectangle the index (an interlaced image's rows in
 *   four-pass order) and, unless it is the transparent index, its palette entry; an image with output >= 0 is written to
 *   out[output]; the canvas is read at the start and written at the end.  Code 5: an index at or beyond the palette's entries (the
 *   pixel is left as it was), position: the lowest such offset in the image's plane; the caller sets status to (0, INT32_MAX) before.
 */
int ccedit_gifdec_codes(const void* data, int64_t data_bytes, const int64_t* desc, int32_t* parent, int32_t* len, int32_t* off, void* first,
                        void* last, int64_t total_codes, int32_t* ncodes, int32_t* status, int32_t N, void* stream);
int ccedit_gifdec_pixels(const int64_t* desc, const int32_t* parent, const int32_t* len, const int32_t* off, const void* last, int64_t total_codes,
                         const int32_t* ncodes, void* planes, int64_t plane_bytes, int32_t N, int64_t max_codes, void* stream);
int ccedit_gifdec_compose(const void* data, int64_t data_bytes, const int64_t* desc, const void* planes, int64_t plane_bytes, void* canvas, void* out,
                          int32_t* status, int32_t N, int32_t n_out, int32_t H, int32_t W, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CCEDIT_HIP_H */
