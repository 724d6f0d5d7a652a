"""Python-side operator wrappers over the C ABI (include/ccedit_hip.h).

PyTorch is used for device memory (torch.empty on the caching allocator) and the stream handle only;
every arithmetic result below is produced by a hand-written HIP kernel in libccedit_hip.so.  All
activations are bf16 tensors in the frames-outermost channels-last layout: (N, H, W, C) contiguous,
N = B*T frames, equivalently a row-major [N*H*W][C] matrix.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

from . import hip, policy
from .hip import (ACT_GEGLU, ACT_NONE, ACT_QUICK_GELU, ACT_SILU, CcAttnDesc, CcFf320Desc, CcGemmDesc, GEMM_CONV2D, GEMM_LINEAR,
                  GEMM_TEMPORAL)
from .packing import PackedFF320, PackedWeight

BF16 = torch.bfloat16


class LaunchProfile:
    """Optional per-launch HIP-event timing of the dominant kernel families (used by bench.py only).
    Events are recorded on the stream the kernels are launched on (torch's current stream)."""

    def __init__(self):
        self.records = {}          # family -> list of (start_event, end_event, algorithmic_flops, algorithmic_bytes)
        self.executed = 0.0        # sum of executed FLOPs over all recorded launches

    def add(self, family, e0, e1, flops, nbytes, shape=None, kernel=None, exec_flops=None):
        if kernel is None:
            k = hip.lib().ccedit_last_kernel()           # the kernel template the entry point just dispatched to
            kernel = k.decode() if k else "?"
        # FLOPs the matrix pipe really retires for this launch where that differs from the algorithmic count (the parity form of
        # upsample + conv executes 4/9 of the reference convolution's multiply-adds)
        ex = flops if exec_flops is None else exec_flops
        self.records.setdefault(family, []).append((e0, e1, flops, nbytes, shape, kernel, ex))
        self.executed += ex

    def by_kernel(self, families=("tap_gemm", "attention", "memory")):
        """[{kernel, launches, ms, tflops, gbytes_per_s}] over the given families, sorted by time (gbytes_per_s: algorithmic bytes
        over the launch time — the number to hold against HBM for the `memory` family: norms, concatenation, layout passes)."""
        torch.cuda.synchronize()
        acc = {}
        for fam in families:
            for a, b, fl, nb, _, k, ex in self.records.get(fam, []):
                n, ms, f, by, _, fe = acc.get(k, (0, 0.0, 0.0, 0.0, fam, 0.0))
                acc[k] = (n + 1, ms + a.elapsed_time(b), f + fl, by + nb, fam, fe + ex)
        return sorted(({"kernel": k, "family": fam, "launches": n, "ms": ms, "tflops": f / (ms * 1e-3) / 1e12,
                        "exec_tflops": fe / (ms * 1e-3) / 1e12, "gbytes_per_s": by / (ms * 1e-3) / 1e9, "bytes": by}
                       for k, (n, ms, f, by, fam, fe) in acc.items()), key=lambda r: -r["ms"])

    def by_shape(self, family, with_kernel=False):
        """{shape: (launches, total_ms, tflops)} sorted by time (with_kernel: keyed on (shape, kernel label))."""
        torch.cuda.synchronize()
        acc = {}
        for a, b, fl, _, shape, _k, _ex in self.records.get(family, []):
            if with_kernel:
                shape = (shape, _k)
            n, ms, f = acc.get(shape, (0, 0.0, 0.0))
            acc[shape] = (n + 1, ms + a.elapsed_time(b), f + fl)
        return sorted(((k, n, ms, f / (ms * 1e-3) / 1e12) for k, (n, ms, f) in acc.items()), key=lambda r: -r[2])

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for fam, recs in self.records.items():
            ms = [r[0].elapsed_time(r[1]) for r in recs]
            out[fam] = dict(launches=len(recs), total_ms=sum(ms), avg_us=1e3 * sum(ms) / max(len(ms), 1),
                            flops=sum(r[2] for r in recs), bytes=sum(r[3] for r in recs))
        return out


PROFILE: Optional[LaunchProfile] = None


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _launch_mem(kernel: str, nbytes: float, fn, shape=None):
    """Run one bandwidth-bound launch; under bench.py's profiled step also time it (HIP events on the launch stream) with its
    algorithmic bytes (every operand read once, the result written once)."""
    if PROFILE is None:
        return fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    PROFILE.add("memory", e0, e1, 0.0, float(nbytes), (kernel,) + tuple(shape or ()), kernel)


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _chk_act(t: torch.Tensor, name: str):
    if t.dtype != BF16 or not t.is_cuda or not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous cuda bf16 tensor, got {t.dtype} {t.device} contiguous={t.is_contiguous()}")


WFRAG = policy.on("wfrag")      # 0: CcGemmDesc.Wfrag stays null (A/B of the coalesced weight preload)


def gemm(a2d: torch.Tensor, pw: PackedWeight, *, mode: int = GEMM_LINEAR, m: Optional[int] = None,
         hin: int = 0, win: int = 0, hout: int = 0, wout: int = 0, stride: int = 1, pad: int = 0, upsample: bool = False,
         t: int = 0, hw: int = 0, tsrc: int = 0, tsrc_off: int = 0, t0: int = 0, tglob: int = 0,
         a2: Optional[torch.Tensor] = None, act: int = ACT_NONE,
         group_bias: Optional[torch.Tensor] = None, group_rows: int = 0,
         res1: Optional[torch.Tensor] = None, res2: Optional[torch.Tensor] = None,
         out: Optional[torch.Tensor] = None, out_f32: bool = False, use_bias: bool = True, tile: int = 0,
         gn_rows: int = 0, ln_eps: float = 0.0, ln_stats: Optional[torch.Tensor] = None, ln_sums=None,
         row_sums: bool = False, subpix: int = 0, vpad: bool = False, halo=None) -> torch.Tensor:
    """out[m, :] = epilogue(sum_taps W . A[src(m, tap)]).  a2d: [rows, lda] bf16 (last dim contiguous).

    gn_rows > 0 (= H*W of the output frames) asks the epilogue to also accumulate the GroupNorm(32) statistics of
    the output; they travel with the returned tensor (`gn_stats_of`) and `groupnorm_spatial` then skips its own
    statistics pass.  Silently not fused when the shape does not qualify (see include/ccedit_hip.h)."""
    assert a2d.dtype == BF16 and a2d.is_cuda and a2d.stride(-1) == 1
    lda = a2d.stride(0)
    cin1 = a2d.shape[1]
    cin = cin1 + (a2.shape[1] if a2 is not None else 0)
    if cin != pw.cin:
        raise ValueError(f"gemm: source has {cin} channels, packed weight expects {pw.cin}")
    if m is None:
        m = a2d.shape[0]
    n_store = pw.n_out if pw.geglu else pw.n
    if out is None:
        out = torch.empty((m, n_store), dtype=torch.float32 if out_f32 else BF16, device=a2d.device)
    assert out.stride(-1) == 1 and out.shape[0] == (4 * m if subpix else m)
    d = CcGemmDesc()
    d.subpix, d.vpad = subpix, int(vpad)
    if halo is not None:            # (top, bottom) boundary rows of the neighbour ranks, each (frames, Win, C) with A's row stride, or None
        assert not vpad and mode == GEMM_CONV2D
        d.vpad = 2
        for h_ in halo:
            if h_ is not None and not (h_.dtype == BF16 and h_.is_cuda and h_.is_contiguous() and h_.dim() == 3 and h_.shape[1] == win
                                       and h_.shape[2] == lda):
                raise ValueError("gemm: halo rows must be contiguous cuda bf16 (frames, Win, lda) tensors")
        d.halo_top, d.halo_bot = _ptr(halo[0]), _ptr(halo[1])
    d.M, d.N, d.Cin, d.Cin1, d.taps, d.mode = m, pw.n, pw.cin, cin1, pw.taps, mode
    d.Hin, d.Win, d.Hout, d.Wout = hin, win, hout, wout
    d.stride, d.pad, d.ksize, d.upsample = stride, pad, pw.ksize, int(upsample)
    d.T, d.HW = t, hw
    d.Tsrc, d.tsrc_off, d.t0, d.Tglob = tsrc, tsrc_off, t0, tglob
    d.lda, d.lda2, d.ldc, d.Kpad = lda, (a2.stride(0) if a2 is not None else 0), out.stride(0), pw.kpad
    d.act = ACT_GEGLU if pw.geglu else act
    d.out_f32 = int(out.dtype == torch.float32)
    d.group_rows = group_rows
    if group_bias is not None:
        assert group_bias.dtype == torch.float32 and group_bias.stride(-1) == 1 and group_bias.shape[-1] == pw.n
        d.ldgb = group_bias.stride(0) if group_bias.dim() == 2 else pw.n
    d.ldr1 = res1.stride(0) if res1 is not None else 0
    d.ldr2 = res2.stride(0) if res2 is not None else 0
    d.tile = tile
    if ln_eps:          # rows of A normalised on the way in (lin320 only): the weight must come from packing.fold_layernorm
        if not ln320_applicable(m, pw, act, res1, res2, group_bias, out_f32, gn_rows):
            raise ValueError("gemm: ln_eps needs the K = 320 register-resident-weight shape (>= 32768 rows, plain Linear)")
        d.ln_eps, d.tile = ln_eps, 9
    if ln_stats is not None:      # rows of A are un-normalised LayerNorm inputs: (mean, rstd) applied in the epilogue (g8_kernel only)
        if pw.colsum is None or ln_stats.dtype != torch.float32 or tuple(ln_stats.shape) != (m, 2) or not ln_stats.is_contiguous():
            raise ValueError("gemm: ln_stats needs a packing.fold_layernorm weight and a contiguous fp32 [M, 2] statistics tensor")
        d.ln_stats, d.ln_colsum = ln_stats.data_ptr(), pw.colsum.data_ptr()
    if ln_sums is not None:       # ... or their (sum, sum of squares) as the producing GEMM left them (`row_sums=True` there): (tensor, eps)
        sums, eps = ln_sums
        if pw.colsum is None or sums.dtype != torch.float64 or tuple(sums.shape) != (m, 2) or not sums.is_contiguous():
            raise ValueError("gemm: ln_sums needs a packing.fold_layernorm weight and the contiguous fp64 [M, 2] sums of the producer")
        d.ln_sums, d.ln_sums_eps, d.ln_colsum = sums.data_ptr(), eps, pw.colsum.data_ptr()
    if row_sums:                  # LayerNorm statistics of the output, accumulated by the epilogue; they travel with the tensor (ln_sums_of)
        sums = _ZEROS.take(2 * m, out.device).view(m, 2)
        d.row_sums = sums.data_ptr()
        out._ln_sums = sums
    elif hasattr(out, "_ln_sums"):
        del out._ln_sums
    d.korder = pw.korder
    d.A, d.A2, d.W = a2d.data_ptr(), _ptr(a2), pw.w.data_ptr()
    d.Wfrag = _ptr(pw.wfrag) if WFRAG else None
    d.bias = _ptr(pw.bias) if use_bias else None
    d.group_bias = _ptr(group_bias)
    d.res1, d.res2, d.out = _ptr(res1), _ptr(res2), out.data_ptr()
    stats = None
    if (gn_rows > 0 and FUSE_GN_STATS and gn_rows % 128 == 0 and m % gn_rows == 0 and pw.n % 32 == 0 and pw.n >= 256
            and not pw.geglu and out.dtype == BF16 and out.shape[1] == pw.n and out.is_contiguous()):
        stats = zero_stats(m // gn_rows, out.device)
        d.gn_rows, d.gn_stats = gn_rows, stats.data_ptr()
        out._gn_stats = (stats, gn_rows)
    elif hasattr(out, "_gn_stats"):
        del out._gn_stats              # a caller-supplied `out` is being overwritten: statistics left on it are stale
    if m <= 8192 and pw.n * pw.kpad >= 1 << 21 and SPLIT_K:      # few output tiles, long K: lend the split-K scratch (include/ccedit_hip.h)
        need = hip.lib().ccedit_gemm_workspace_bytes(C.byref(d))
        if need:
            ws = _splitk_ws(need, out.device)
            d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
    if PROFILE is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        hip.check(hip.lib().ccedit_gemm(C.byref(d), _stream()), "ccedit_gemm")
        e1.record()
        nres = int(res1 is not None) + int(res2 is not None)
        alg_bytes = (a2d.shape[0] * cin1 * 2 + (a2.shape[0] * a2.shape[1] * 2 if a2 is not None else 0)      # sources, once
                     + m * out.shape[1] * out.element_size() + nres * m * pw.n * 2 + pw.n * pw.kpad * 2)   # out, residuals, W
        PROFILE.add("tap_gemm", e0, e1, pw.flops_per_row * m, float(alg_bytes),
                    (("lin", "conv", "temp")[mode] + ("+up" if upsample else "") + ("+up(parity)" if subpix else ""), m, pw.n, pw.taps * pw.cin, stride,
                     int(res1 is not None) + int(res2 is not None), d.act),
                    exec_flops=pw.flops_per_row * m * (4.0 / 9.0) if subpix else None)
        return out
    hip.check(hip.lib().ccedit_gemm(C.byref(d), _stream()), "ccedit_gemm")
    return out


def linear(x2d, pw, **kw):
    return gemm(x2d, pw, mode=GEMM_LINEAR, **kw)


def set_mark(t: torch.Tensor, name: str, value) -> None:
    """A host-side fact about the VALUES of a tensor (e.g. "its two CFG halves are equal"), carried as a Python attribute together with
    the tensor's in-place version counter: get_mark returns it only while the tensor has not been written since (ADVICE r5 — an
    inpainting blend or per-half noise added in place after marking must not leave a stale mark behind)."""
    setattr(t, name, (value, t._version))


def get_mark(t, name: str):
    """The marked value, or None when the tensor carries no such mark or was modified in place after it was marked."""
    m = getattr(t, name, None) if torch.is_tensor(t) else None
    if not (isinstance(m, tuple) and len(m) == 2):
        return None
    return m[0] if m[1] == t._version else None


LN320 = policy.on("ln320")      # 0: separate LayerNorm pass in front of the K = 320 projections


def ln320_applicable(m, pw, act=ACT_NONE, res1=None, res2=None, group_bias=None, out_f32=False, gn_rows=0) -> bool:
    """Can `linear(layernorm(x), pw)` run as ONE lin320 launch that normalises the rows in LDS?  Only single-slice layers
    (N = 320: to_q): every 320-channel slice of a wider layer is its own workgroup and would normalise the tile again — measured
    114 us against 153 us for LayerNorm + lin320 at N = 320, but 301 against 292 at N = 960 (tools/exp/ln320_time.py)."""
    return (LN320 and m >= 32768 and pw.cin == 320 and pw.taps == 1 and pw.kpad == 320 and pw.n == 320
            and not pw.geglu and act == ACT_NONE and res1 is None and res2 is None and group_bias is None and not out_f32
            and gn_rows == 0)


ATTN_Q_LOG2 = policy.on("attn_q_log2")      # 0: softmax scale applied inside the attention kernels (A/B)
FF320 = policy.on("ff320")      # 0: LayerNorm + two GEMMs instead of the fused dim-320 feed-forward
BLOCK_TAIL = policy.on("block_tail") and FF320      # to_out / proj_out of the dim-320 transformer tails inside the ff320 launch


def ff320(x2d: Optional[torch.Tensor], pk: PackedFF320, eps: float = 1e-5, ln: bool = True, out: Optional[torch.Tensor] = None,
          dbg: Optional[torch.Tensor] = None, a: Optional[torch.Tensor] = None, res: Optional[torch.Tensor] = None,
          res2: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = x + W2 . GEGLU(W1 . LayerNorm(x) + b1) + b2 for dim 320 in one kernel (csrc/ff320.hip).  x2d: [tokens, 320].
    Block tail (pk from packing.pack_ff320_tail): x2d is None and x = W_o . a + b_o + res is computed by the kernel's prologue GEMM;
    with res2 (and an epilogue pack) the result is W_p . (x + FF(LN(x))) + b_p + res2."""
    tail = a is not None
    src = a if tail else x2d
    assert src.dtype == BF16 and src.is_cuda and src.stride(-1) == 1 and src.shape[1] == 320
    m = src.shape[0]
    if out is None:
        out = torch.empty((m, 320), dtype=BF16, device=src.device)
    assert out.dtype == BF16 and out.stride(-1) == 1 and out.shape == (m, 320) and out.data_ptr() != src.data_ptr()
    d = CcFf320Desc()
    d.M, d.dim, d.inner, d.ldo, d.eps, d.ln = m, 320, 1280, out.stride(0), eps, int(ln)
    d.out, d.wstream, d.b2p = out.data_ptr(), pk.stream.data_ptr(), pk.b2p.data_ptr()
    d.dbg = None if dbg is None else dbg.data_ptr()
    nbytes = 2.0 * m * 320 * 2 + pk.stream.numel()
    if tail:
        if pk.bop is None or res is None or x2d is not None:
            raise ValueError("ff320: the block-tail form needs a packing.pack_ff320_tail pack, `a` and `res`, and no x2d")
        if (res2 is not None) != (pk.bpp is not None):
            raise ValueError("ff320: res2 goes with an epilogue pack (pack_ff320_tail(..., wp=...)), and only with one")
        for t_ in (res, res2):
            if t_ is not None:
                assert t_.dtype == BF16 and t_.is_cuda and t_.stride(-1) == 1 and tuple(t_.shape) == (m, 320) and t_.data_ptr() != out.data_ptr()
        d.a, d.lda, d.res, d.ldr, d.bop = a.data_ptr(), a.stride(0), res.data_ptr(), res.stride(0), pk.bop.data_ptr()
        nbytes += 2.0 * m * 320
        if res2 is not None:
            d.res2, d.ldr2, d.bpp = res2.data_ptr(), res2.stride(0), pk.bpp.data_ptr()
            nbytes += 2.0 * m * 320
    else:
        if pk.bop is not None:
            raise ValueError("ff320: a block-tail pack needs `a` / `res` (use pk.tail_of for the plain feed-forward)")
        d.x, d.ldx = x2d.data_ptr(), x2d.stride(0)
    if PROFILE is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        hip.check(hip.lib().ccedit_ff320(C.byref(d), _stream()), "ccedit_ff320")
        e1.record()
        PROFILE.add("tap_gemm", e0, e1, pk.flops_per_row * m, float(nbytes),
                    ("ff320" + ("+to_out" if tail else "") + ("+proj_out" if res2 is not None else ""), m, 320, 1280, 1, 1, 2))
        return out
    hip.check(hip.lib().ccedit_ff320(C.byref(d), _stream()), "ccedit_ff320")
    return out


def conv2d(x: torch.Tensor, pw: PackedWeight, stride: int = 1, pad: int = 1, upsample: bool = False,
           x2: Optional[torch.Tensor] = None, gn: bool = False, out_hw: Optional[tuple] = None, vpad: bool = False, halo=None,
           **kw) -> torch.Tensor:
    """x: (N, H, W, C) -> (N, Hout, Wout, Cout); 3x3 (pad 1) or 1x1 (pad 0) by the packed kernel size.
    gn=True: the output feeds a spatial GroupNorm — accumulate its statistics in the epilogue."""
    n, h, w, c = x.shape
    if pw.ksize == 1:
        pad = 0
    hv, wv = (2 * h, 2 * w) if upsample else (h, w)
    hout = (hv + 2 * pad - pw.ksize) // stride + 1
    wout = (wv + 2 * pad - pw.ksize) // stride + 1
    if vpad:                        # the frames carry their own halo rows (RowShard): no vertical padding
        assert pw.ksize == 3 and pad == 1 and not upsample and x2 is None
        hout = (hv - pw.ksize) // stride + 1
        kw["vpad"] = True
    if halo is not None:            # rows sharded over ranks, the neighbours' boundary rows as separate tensors (CcGemmDesc.vpad = 2)
        assert pw.ksize == 3 and pad == 1 and not upsample and x2 is None and not vpad
        kw["halo"] = halo
    if out_hw is not None:          # asymmetric padding (VAE Downsample, model.py:74-93: pad right/bottom only, conv pad 0):
        hout, wout = out_hw         # taps that fall outside the source read zeros, so only the output size changes
    a2 = None if x2 is None else x2.reshape(-1, x2.shape[-1])
    if pw.ksize == 1 and pw.taps == 1 and stride == 1 and not upsample and out_hw is None and not vpad and halo is None and CONV1X1_LINEAR:
        # a 1 x 1 convolution is a Linear over the pixels (zero convs, skip connections): the Linear dispatch reaches the streaming
        # K = 320 / 640 kernels and the persistent GEMM, the convolution modes do not
        out = gemm(x.reshape(-1, c), pw, mode=GEMM_LINEAR, a2=a2, gn_rows=hout * wout if gn else 0, **kw)
        return carry_gn_stats(out, out.view(n, hout, wout, out.shape[-1]))
    out = gemm(x.reshape(-1, c), pw, mode=GEMM_CONV2D, m=n * hout * wout, hin=h, win=w, hout=hout, wout=wout,
               stride=stride, pad=pad, upsample=upsample, a2=a2, gn_rows=hout * wout if gn else 0, **kw)
    return carry_gn_stats(out, out.view(n, hout, wout, out.shape[-1]))


CONV1X1_LINEAR = policy.on("conv1x1_linear")      # 0: 1 x 1 convs through the convolution mode (A/B)
SUBPIX = policy.on("subpix")      # 0: upsample + 3x3 conv through the nine-tap gather (A/B)


def conv2d_upsampled(x: torch.Tensor, pws, vpad: bool = False, halo=None, tile: int = 0) -> torch.Tensor:
    """conv3x3(nearest_upsample_2x(x)) as four 2 x 2 convolutions on x, one per output parity (packing.pack_upsample_parities):
    x (N, H, W, C) -> (N, 2H, 2W, Cout); every launch writes its quarter of the output pixels in place.  vpad: x carries one halo
    row above and below its H rows (RowShard, extended copy); halo = (top, bottom): the same rows as separate tensors."""
    _chk_act(x, "conv2d_upsampled")
    n, hx, w, c = x.shape
    h = hx - 2 if vpad else hx
    out = torch.empty((n * 4 * h * w, pws[0].n), dtype=BF16, device=x.device)
    for p, pw in enumerate(pws):
        gemm(x.reshape(-1, c), pw, mode=GEMM_CONV2D, m=n * h * w, hin=hx, win=w, hout=h, wout=w, stride=1, pad=0, out=out, subpix=p + 1,
             vpad=vpad, halo=halo, tile=tile)
    return out.view(n, 2 * h, 2 * w, pws[0].n)


def conv_temporal(x: torch.Tensor, t: int, pw: PackedWeight, gn: bool = False, **kw) -> torch.Tensor:
    """Conv1d over the T frames of each clip; x: (B*T, H, W, C)."""
    n, h, w, c = x.shape
    if pw.taps == 1:
        out = gemm(x.reshape(-1, c), pw, mode=GEMM_LINEAR, gn_rows=h * w if gn else 0, **kw)
    else:
        out = gemm(x.reshape(-1, c), pw, mode=GEMM_TEMPORAL, t=t, hw=h * w, gn_rows=h * w if gn else 0, **kw)
    return carry_gn_stats(out, out.view(n, h, w, out.shape[-1]))


def conv_temporal_sharded(x_ext: torch.Tensor, b: int, t_local: int, t0: int, t_glob: int, pw: PackedWeight,
                          gn: bool = False, **kw) -> torch.Tensor:
    """Conv1d (k3) over T for a frame shard.  x_ext: (B*(t_local+2), H, W, C) = per clip [halo from the previous
    rank | t_local local frames | halo from the next rank] (halo contents are ignored where they fall outside the
    clip); local frame 0 is global keyframe t0 of t_glob.  Returns (B*t_local, H, W, Cout)."""
    n, h, w, c = x_ext.shape
    assert n == b * (t_local + 2) and pw.taps == 3
    out = gemm(x_ext.reshape(-1, c), pw, mode=GEMM_TEMPORAL, m=b * t_local * h * w, t=t_local, hw=h * w,
               tsrc=t_local + 2, tsrc_off=1, t0=t0, tglob=t_glob, gn_rows=h * w if gn else 0, **kw)
    return carry_gn_stats(out, out.view(b * t_local, h, w, out.shape[-1]))


# ------------------------------------------------------------------------------------------
_ws_cache = {}


SPLIT_K = policy.get("g8_split") != 0
_splitk_cache = {}


def _splitk_ws(nbytes: int, device) -> torch.Tensor:
    """Split-K scratch of the current stream (arrival counters in the first 4096 bytes: zero when handed out, left zero by every
    call; launches of one stream are ordered, other streams get their own buffer)."""
    key = (device, torch.cuda.current_stream().cuda_stream)
    ws = _splitk_cache.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.zeros(nbytes, dtype=torch.uint8, device=device)
        _splitk_cache[key] = ws
    return ws


def _stats_ws(frames: int, device) -> torch.Tensor:
    key = (device, torch.cuda.current_stream().cuda_stream)
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < frames * 64:
        ws = torch.empty(max(frames * 64, 4096), dtype=torch.float64, device=device)
        _ws_cache[key] = ws
    return ws


class _ZeroArena:
    """Zero-initialised fp64 scratch for the fused GroupNorm statistics (double: see include/ccedit_hip.h): one memset per ~256 requests instead of one
    per producer launch (150 per network evaluation).  A slice is handed out once and never recycled — the tensors
    that carry the statistics keep the slab alive — and arenas are per (device, stream)."""
    SLAB = 256 * 34 * 64

    def __init__(self):
        self.slabs = {}

    def take(self, numel: int, device) -> torch.Tensor:
        key = (device, torch.cuda.current_stream().cuda_stream)
        slab, used = self.slabs.get(key, (None, 0))
        if slab is None or used + numel > slab.numel():
            slab, used = torch.zeros(max(self.SLAB, numel), dtype=torch.float64, device=device), 0
        self.slabs[key] = (slab, used + numel)
        return slab[used:used + numel]


_ZEROS = _ZeroArena()


def reset_stream_scratch():
    """Forget every cached scratch buffer (statistics workspace, zeroed arenas, split-K workspace) of EVERY stream.  Called at both
    ends of a HIP-graph capture: what is allocated while capturing belongs to that graph's memory pool and is zeroed by a captured
    fill, so nothing captured later may continue in it — and a capture spans several streams (the ControlNet's side stream keeps
    its own arenas): resetting only the capture stream's left the side stream's arena of an earlier graph in use by the next one,
    whose replays then accumulated GroupNorm statistics onto the previous replay's (round 3: the sampler run after the step
    benchmark produced non-finite frames)."""
    _ws_cache.clear()
    _ZEROS.slabs.clear()
    _splitk_cache.clear()


def zero_stats(frames: int, device) -> torch.Tensor:
    return _ZEROS.take(frames * 64, device).view(frames, 32, 2)


FUSE_GN_STATS = policy.on("fuse_gn_stats")      # 0: always the two-pass GroupNorm


def gn_stats_of(x: torch.Tensor, hw: int):
    """Statistics a producing GEMM left on `x` (None if it did not)."""
    st = getattr(x, "_gn_stats", None)
    return st[0] if st is not None and st[1] == hw else None


def carry_gn_stats(src: torch.Tensor, view: torch.Tensor) -> torch.Tensor:
    """`view` is a reshape of `src` (same memory): keep the producer's statistics attached."""
    st = getattr(src, "_gn_stats", None)
    if st is not None:
        view._gn_stats = st
    return view


def groupnorm_spatial(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, silu: bool) -> torch.Tensor:
    _chk_act(x, "groupnorm_spatial")
    n, h, w, c = x.shape
    y = torch.empty_like(x)
    st = gn_stats_of(x, h * w)
    if st is not None:
        assert st.shape[0] == n
        _launch_mem("gn_spatial_apply (statistics from the producer)", 4.0 * x.numel(), lambda: hip.check(
            hip.lib().ccedit_groupnorm_spatial_apply(x.data_ptr(), y.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                                     st.data_ptr(), n, h * w, c, eps, int(silu), _stream()),
            "ccedit_groupnorm_spatial_apply"), (n, h, w, c))
        return y
    ws = _stats_ws(n, x.device)
    _launch_mem("gn_spatial stats + apply (two reads)", 6.0 * x.numel(), lambda: hip.check(
        hip.lib().ccedit_groupnorm_spatial(x.data_ptr(), y.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                           ws.data_ptr(), n, h * w, c, eps, int(silu), _stream()),
        "ccedit_groupnorm_spatial"), (n, h, w, c))
    return y


def groupnorm_spatial_stats(x: torch.Tensor) -> torch.Tensor:
    """(sum, sum of squares) per (frame, group) of x (N, H, W, C): double (N, 32, 2).  The statistics half of `groupnorm_spatial` for
    frames whose rows are sharded over ranks: all-reduce, divide by the number of ranks, attach with `set_gn_stats`."""
    _chk_act(x, "groupnorm_spatial_stats")
    n, h, w, c = x.shape
    st = zero_stats(n, x.device)
    hip.check(hip.lib().ccedit_groupnorm_spatial_stats(x.data_ptr(), st.data_ptr(), n, h * w, c, _stream()), "ccedit_groupnorm_spatial_stats")
    return st


def set_gn_stats(x: torch.Tensor, stats: torch.Tensor):
    x._gn_stats = (stats, x.shape[1] * x.shape[2])
    return x


def groupnorm_temporal(x: torch.Tensor, b: int, t: int, gamma, beta, eps: float, silu: bool) -> torch.Tensor:
    _chk_act(x, "groupnorm_temporal")
    n, h, w, c = x.shape
    assert n == b * t
    y = torch.empty_like(x)
    _launch_mem("gn_temporal", 4.0 * x.numel(), lambda: hip.check(
        hip.lib().ccedit_groupnorm_temporal(x.data_ptr(), y.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                            b, t, h * w, c, eps, int(silu), _stream()), "ccedit_groupnorm_temporal"), (n, h, w, c))
    return y


def groupnorm_temporal_stats(x: torch.Tensor, b: int, t: int) -> torch.Tensor:
    """Partial (sum, sumsq) per (clip, pixel, group) over the local frames: fp32 (b*hw, 32, 2)."""
    _chk_act(x, "groupnorm_temporal_stats")
    n, h, w, c = x.shape
    assert n == b * t
    st = torch.empty((b * h * w, 32, 2), dtype=torch.float32, device=x.device)
    hip.check(hip.lib().ccedit_groupnorm_temporal_stats(x.data_ptr(), st.data_ptr(), b, t, h * w, c, _stream()),
              "ccedit_groupnorm_temporal_stats")
    return st


def groupnorm_temporal_apply(x: torch.Tensor, stats: torch.Tensor, b: int, t: int, t_glob: int, gamma, beta, eps: float,
                             silu: bool, out: Optional[torch.Tensor] = None, dst_frames: int = 0, dst_off: int = 0):
    """Apply with (all-reduced) statistics over t_glob frames; optionally write into a halo-extended buffer."""
    _chk_act(x, "groupnorm_temporal_apply")
    n, h, w, c = x.shape
    y = torch.empty_like(x) if out is None else out
    if dst_frames == 0:
        dst_frames, dst_off = t, 0
    hip.check(hip.lib().ccedit_groupnorm_temporal_apply(x.data_ptr(), y.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                                        stats.data_ptr(), b, t, h * w, c, float((c // 32) * t_glob), eps,
                                                        int(silu), dst_frames, dst_off, _stream()),
              "ccedit_groupnorm_temporal_apply")
    return y


def row_stats(x2d: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    """(mean, rstd) of every row: the statistics half of LayerNorm, for a GEMM that folds the normalisation (gemm(ln_stats=...))."""
    _chk_act(x2d, "row_stats")
    assert x2d.is_contiguous()
    st = torch.empty((x2d.shape[0], 2), dtype=torch.float32, device=x2d.device)
    _launch_mem("row_stats", 2.0 * x2d.numel(), lambda: hip.check(
        hip.lib().ccedit_row_stats(x2d.data_ptr(), st.data_ptr(), x2d.shape[0], x2d.shape[1], eps, _stream()), "ccedit_row_stats"))
    return st


LNF = policy.on("lnf")       # 0: LayerNorm passes in front of the 640 / 1280-channel projections (A/B)


def ln_sums_of(x: torch.Tensor):
    """(sum, sum of squares) per row that the producing GEMM left on `x` (None if it did not)."""
    return getattr(x, "_ln_sums", None)


def row_sums_applicable(m: int, pw, act: int = ACT_NONE) -> bool:
    """A Linear whose epilogue can accumulate the row sums of its output (the persistent eight-phase kernel's shapes)."""
    return LNF and LN_SUMS and m >= 4096 and pw.kpad >= 640 and pw.n >= 640 and pw.taps == 1 and not pw.geglu and act == ACT_NONE


LN_SUMS = policy.on("ln_sums")   # 0: statistics by ccedit_row_stats instead of the producer's epilogue (A/B)


def lnf_applicable(m: int, pw) -> bool:
    """ccedit_gemm's conditions for ln_stats (the persistent eight-phase kernel, csrc/gemm.hip)."""
    return LNF and pw is not None and pw.colsum is not None and m >= 4096 and pw.kpad >= 640 and pw.n >= 640 and pw.taps == 1


def layernorm(x2d: torch.Tensor, gamma, beta, eps: float = 1e-5) -> torch.Tensor:
    _chk_act(x2d, "layernorm")
    y = torch.empty_like(x2d)
    _launch_mem("layernorm", 4.0 * x2d.numel(), lambda: hip.check(
        hip.lib().ccedit_layernorm(x2d.data_ptr(), y.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                   x2d.shape[0], x2d.shape[1], eps, _stream()), "ccedit_layernorm"), tuple(x2d.shape))
    return y


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, d: int, *, batches: int, lq: int, lk: int,
              q_inner: int = 1, q_outer_rows: Optional[int] = None, q_inner_rows: int = 0, q_seq_rows: int = 1,
              kv_div: int = 1, kv_inner: int = 1, kv_outer_rows: Optional[int] = None, kv_inner_rows: int = 0,
              kv_seq_rows: int = 1, out: Optional[torch.Tensor] = None,
              seg1_len: int = 0, seg1_div: int = 1, seg1_mul: int = 0, seg1_add: int = 0, causal: bool = False,
              q_log2: bool = False, scale: Optional[float] = None, kv_per_frame: bool = False) -> torch.Tensor:
    """q/k/v: 2-D row-major views [rows, >= heads*d] (may be column slices of a fused buffer).  q_log2: q already carries
    d^-0.5 * log2(e) (folded into the to_q weights by the packer).  scale: the softmax scale, None = d^-0.5 (ignored with q_log2).
    kv_per_frame: text K/V of its own for every batch (CCEDIT_ATTN_KV_PER_FRAME; kv_div must be 1)."""
    if kv_per_frame and kv_div != 1:
        raise ValueError(f"attention: kv_per_frame means one kv batch per batch, got kv_div={kv_div}")
    for tns in (q, k, v):
        assert tns.dtype == BF16 and tns.is_cuda and tns.stride(-1) == 1
    if out is None:
        out = torch.empty((q.shape[0], heads * d), dtype=BF16, device=q.device)
    a = CcAttnDesc()
    a.q, a.k, a.v, a.o = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr()
    a.ldq, a.ldk, a.ldv, a.ldo = q.stride(0), k.stride(0), v.stride(0), out.stride(0)
    a.heads, a.d, a.batches, a.Lq, a.Lk = heads, d, batches, lq, lk
    a.q_inner, a.q_outer_rows, a.q_inner_rows, a.q_seq_rows = q_inner, (lq if q_outer_rows is None else q_outer_rows), q_inner_rows, q_seq_rows
    a.kv_div, a.kv_inner = kv_div, kv_inner
    a.kv_outer_rows, a.kv_inner_rows, a.kv_seq_rows = (lk if kv_outer_rows is None else kv_outer_rows), kv_inner_rows, kv_seq_rows
    a.scale = float(d) ** -0.5 if scale is None else float(scale)
    a.seg1_len, a.seg1_div, a.seg1_mul, a.seg1_add = seg1_len, seg1_div, seg1_mul, seg1_add
    a.causal = int(causal)
    a.flags = (hip.ATTN_Q_LOG2 if q_log2 else 0) | (hip.ATTN_KV_PER_FRAME if kv_per_frame else 0)
    if PROFILE is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        hip.check(hip.lib().ccedit_attention(C.byref(a), _stream()), "ccedit_attention")
        e1.record()
        nb = 2.0 * heads * d * (2.0 * batches * lq + 2.0 * (batches // kv_div) * lk)          # q, o, k, v once
        PROFILE.add("attention", e0, e1, 4.0 * batches * heads * lq * lk * d, nb, (batches, heads, d, lq, lk))
        return out
    hip.check(hip.lib().ccedit_attention(C.byref(a), _stream()), "ccedit_attention")
    return out


# ------------------------------------------------------------------------------------------
def ncthw_to_nhwc(x: torch.Tensor, cpad: int, scale_per_b: Optional[torch.Tensor] = None, scale: float = 1.0,
                  shift: float = 0.0) -> torch.Tensor:
    """fp32 (B, C, T, H, W) -> bf16 (B*T, H, W, cpad); y = x*scale(*scale_per_b[b]) + shift."""
    assert x.dtype == torch.float32 and x.is_cuda and x.is_contiguous() and x.ndim == 5
    b, c, t, h, w = x.shape
    y = torch.empty((b * t, h, w, cpad), dtype=BF16, device=x.device)
    hip.check(hip.lib().ccedit_ncthw_to_nhwc(x.data_ptr(), y.data_ptr(), b, c, t, h, w, cpad, _ptr(scale_per_b),
                                             scale, shift, _stream()), "ccedit_ncthw_to_nhwc")
    return y


def nhwc_to_ncthw(x: torch.Tensor, b: int, t: int, c: int) -> torch.Tensor:
    """(B*T, H, W, ld) bf16|fp32 -> fp32 (B, c, T, H, W) taking the first c channels."""
    assert x.is_cuda and x.is_contiguous() and x.ndim == 4
    n, h, w, ld = x.shape
    if n != b * t or c > ld or c < 1:
        raise ValueError(f"nhwc_to_ncthw: x {tuple(x.shape)} is not (b * t = {b} * {t}, h, w, >= c = {c})")
    y = torch.empty((b, c, t, h, w), dtype=torch.float32, device=x.device)
    hip.check(hip.lib().ccedit_nhwc_to_ncthw(x.data_ptr(), int(x.dtype == torch.float32), ld, y.data_ptr(), b, c, t, h, w,
                                             _stream()), "ccedit_nhwc_to_ncthw")
    return y


def cat_add(a: torch.Tensor, b: torch.Tensor, c: Optional[torch.Tensor], gn: bool = False) -> torch.Tensor:
    """(..., C1) ++ ((..., C2) + (..., C2)) along channels.  gn=True (4-D NHWC input): also accumulate the
    GroupNorm(32) statistics of the result for the `groupnorm_spatial` that follows."""
    _chk_act(a, "cat_add.a"), _chk_act(b, "cat_add.b")
    if a.shape[:-1] != b.shape[:-1] or (c is not None and c.shape != b.shape):
        raise ValueError(f"cat_add: mismatched shapes {tuple(a.shape)}, {tuple(b.shape)}"
                         + (f", {tuple(c.shape)}" if c is not None else "")
                         + " (frame sizes must be multiples of 64 pixels so that the UNet's 3 down/up levels agree)")
    c1, c2 = a.shape[-1], b.shape[-1]
    out = torch.empty((*a.shape[:-1], c1 + c2), dtype=BF16, device=a.device)
    if gn and FUSE_GN_STATS and a.dim() == 4 and (c1 + c2) % 32 == 0 and c1 + c2 <= 2560:
        n, hw = a.shape[0], a.shape[1] * a.shape[2]
        stats = zero_stats(n, a.device)
        nb = 2.0 * (a.numel() + b.numel() * (2 if c is not None else 1) + out.numel())
        _launch_mem("cat_add_gn", nb, lambda: hip.check(
            hip.lib().ccedit_cat_add_gn(a.data_ptr(), b.data_ptr(), _ptr(c), out.data_ptr(), stats.data_ptr(), n, hw,
                                        c1, c2, _stream()), "ccedit_cat_add_gn"), (n, hw, c1, c2))
        out._gn_stats = (stats, hw)
        return out
    nb = 2.0 * (a.numel() + b.numel() * (2 if c is not None else 1) + out.numel())
    _launch_mem("cat_add", nb, lambda: hip.check(
        hip.lib().ccedit_cat_add(a.data_ptr(), b.data_ptr(), _ptr(c), out.data_ptr(), a.numel() // c1, c1, c2,
                                 _stream()), "ccedit_cat_add"))
    return out


def copy_row_blocks(src: torch.Tensor, dst: torch.Tensor, blocks: torch.Tensor, max_rows: int, add: Optional[torch.Tensor] = None):
    """dst[blocks[s,1] : +blocks[s,2]] = src[blocks[s,0] : +blocks[s,2]] (+ add at the destination rows) for every block s.
    src / dst / add: 2-D row-major with the same row width; blocks: int64 (n, 3) on the device."""
    assert src.is_cuda and dst.is_cuda and src.is_contiguous() and dst.is_contiguous() and src.shape[1] == dst.shape[1]
    assert blocks.dtype == torch.int64 and blocks.is_cuda and blocks.is_contiguous() and blocks.shape[1] == 3
    if add is not None:
        assert add.dtype == BF16 and dst.dtype == BF16 and add.is_contiguous() and add.shape == dst.shape
    hip.check(hip.lib().ccedit_copy_row_blocks(src.data_ptr(), dst.data_ptr(), _ptr(add), blocks.data_ptr(), blocks.shape[0], max_rows,
                                               src.shape[1] * src.element_size(), _stream()), "ccedit_copy_row_blocks")
    return dst


def copy_2d_blocks(src: torch.Tensor, dst: torch.Tensor, blocks: torch.Tensor, rows: int, row_bytes: int):
    """For every block s: dst_bytes[blocks[s,1] + r * dst_pitch : + row_bytes] = src_bytes[blocks[s,0] + r * src_pitch : + row_bytes],
    r < rows.  src / dst: 2-D tensors with contiguous rows (the pitches are their row strides in bytes); blocks: int64 (n, 2) on the
    device, byte offsets from the tensors' first element."""
    assert src.is_cuda and dst.is_cuda and src.dim() == 2 and dst.dim() == 2 and src.stride(1) == 1 and dst.stride(1) == 1
    assert blocks.dtype == torch.int64 and blocks.is_cuda and blocks.is_contiguous() and blocks.shape[1] == 2
    hip.check(hip.lib().ccedit_copy_2d_blocks(src.data_ptr(), dst.data_ptr(), blocks.data_ptr(), blocks.shape[0], rows, row_bytes,
                                              src.stride(0) * src.element_size(), dst.stride(0) * dst.element_size(), _stream()),
              "ccedit_copy_2d_blocks")
    return dst


def add(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _chk_act(a, "add.a"), _chk_act(b, "add.b")
    y = torch.empty_like(a) if out is None else out
    hip.check(hip.lib().ccedit_add(a.data_ptr(), b.data_ptr(), y.data_ptr(), a.numel(), _stream()), "ccedit_add")
    return y


def silu(x: torch.Tensor) -> torch.Tensor:
    _chk_act(x, "silu")
    y = torch.empty_like(x)
    hip.check(hip.lib().ccedit_silu(x.data_ptr(), y.data_ptr(), x.numel(), _stream()), "ccedit_silu")
    return y


def timestep_embedding(t: torch.Tensor, dim: int) -> torch.Tensor:
    assert t.dtype == torch.int64 and t.is_cuda
    out = torch.empty((t.shape[0], dim), dtype=BF16, device=t.device)
    hip.check(hip.lib().ccedit_timestep_embedding(t.data_ptr(), out.data_ptr(), t.shape[0], dim, dim, _stream()),
              "ccedit_timestep_embedding")
    return out


def embedding_lookup(ids: torch.Tensor, tok: torch.Tensor, pos: torch.Tensor) -> torch.Tensor:
    """ids int64 (B, L) -> bf16 [B*L, C] = tok[ids] + pos (CLIP text embeddings)."""
    assert ids.dtype == torch.int64 and ids.is_cuda and ids.is_contiguous() and tok.dtype == pos.dtype == torch.float32
    b, l = ids.shape
    assert pos.shape[0] == l and tok.shape[1] == pos.shape[1]
    if int(ids.min()) < 0 or int(ids.max()) >= tok.shape[0]:
        raise ValueError(f"token id outside [0, {tok.shape[0]})")
    out = torch.empty((b * l, tok.shape[1]), dtype=BF16, device=ids.device)
    hip.check(hip.lib().ccedit_embedding_lookup(ids.data_ptr(), tok.data_ptr(), pos.data_ptr(), out.data_ptr(), b * l, l,
                                                tok.shape[1], tok.shape[0], _stream()), "ccedit_embedding_lookup")
    return out


def gaussian_sample(moments: torch.Tensor, noise: torch.Tensor, zc: int, scale: float = 1.0) -> torch.Tensor:
    """moments: fp32 [frames*hw, >=2*zc] channels-last rows [mean | logvar]; noise: fp32 (frames, zc, h, w)."""
    if not (moments.is_cuda and noise.is_cuda):
        raise ValueError(f"gaussian_sample: moments on {moments.device}, noise on {noise.device}: both must be on the GPU")
    if moments.dim() != 2 or moments.shape[1] < 2 * zc:
        raise ValueError(f"gaussian_sample: moments {tuple(moments.shape)} has fewer than 2 * zc = {2 * zc} columns")
    assert moments.dtype == torch.float32 and noise.dtype == torch.float32 and noise.is_contiguous() and moments.stride(-1) == 1
    n, c, h, w = noise.shape
    assert c == zc and moments.shape[0] == n * h * w
    out = torch.empty_like(noise)
    hip.check(hip.lib().ccedit_gaussian_sample(moments.data_ptr(), noise.data_ptr(), out.data_ptr(), n, zc, h * w,
                                               moments.stride(0), scale, _stream()), "ccedit_gaussian_sample")
    return out


def mask_blend(x: torch.Tensor, z: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """x * mask + z * (1 - mask), fp32 tensors of one shape."""
    for tns in (x, z, mask):
        assert tns.dtype == torch.float32 and tns.is_cuda and tns.is_contiguous() and tns.shape == x.shape
    y = torch.empty_like(x)
    hip.check(hip.lib().ccedit_mask_blend(x.data_ptr(), z.data_ptr(), mask.data_ptr(), y.data_ptr(), x.numel(), _stream()),
              "ccedit_mask_blend")
    return y


def cfg_denoise(x: torch.Tensor, eps2: torch.Tensor, sigma: float, scale: float) -> torch.Tensor:
    """x: fp32 latent (n elems); eps2: fp32 [2, n] (uncond first). -> denoised (guided) fp32."""
    if not (x.is_cuda and eps2.is_cuda):
        raise ValueError(f"cfg_denoise: x on {x.device}, eps2 on {eps2.device}: both must be on the GPU")
    if eps2.numel() != 2 * x.numel():
        raise ValueError(f"cfg_denoise: eps2 {tuple(eps2.shape)} does not hold two halves of x {tuple(x.shape)}")
    assert x.dtype == torch.float32 and eps2.dtype == torch.float32 and x.is_contiguous() and eps2.is_contiguous()
    den = torch.empty_like(x)
    hip.check(hip.lib().ccedit_cfg_denoise(x.data_ptr(), eps2.data_ptr(), den.data_ptr(), x.numel(), sigma, scale, _stream()),
              "ccedit_cfg_denoise")
    return den


def axpby(x: torch.Tensor, z: torch.Tensor, a: float, b: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    for name, tns in (("x", x), ("z", z), ("out", out)):
        if tns is None:
            continue
        if not tns.is_cuda:
            raise ValueError(f"axpby: {name} is on {tns.device}, not on the GPU")
        if tns.numel() != x.numel() or tns.dtype != x.dtype:
            raise ValueError(f"axpby: {name} {tuple(tns.shape)} {tns.dtype} does not match x {tuple(x.shape)} {x.dtype}")
    assert x.dtype == torch.float32 and x.is_contiguous() and z.is_contiguous() and (out is None or out.is_contiguous())
    y = torch.empty_like(x) if out is None else out
    hip.check(hip.lib().ccedit_axpby(x.data_ptr(), z.data_ptr(), y.data_ptr(), x.numel(), a, b, _stream()), "ccedit_axpby")
    return y


def softmax_rows(s: torch.Tensor, cols: int, cols_pad: int, scale: float) -> torch.Tensor:
    """s: fp32 [rows, >= cols] -> bf16 [rows, cols_pad] = softmax(s[:, :cols] * scale), zero pad."""
    assert s.dtype == torch.float32 and s.is_cuda and s.dim() == 2 and s.stride(-1) == 1
    if s.shape[1] < cols:
        raise ValueError(f"softmax_rows: s {tuple(s.shape)} has fewer than cols = {cols} columns")
    p = torch.empty((s.shape[0], cols_pad), dtype=BF16, device=s.device)
    hip.check(hip.lib().ccedit_softmax_rows(s.data_ptr(), p.data_ptr(), s.shape[0], cols, cols_pad, s.stride(0), cols_pad,
                                            scale, _stream()), "ccedit_softmax_rows")
    return p


# ------------------------------------------------------------------------------------------
# Pixel I/O (csrc/pixel.hip): uint8 frames <-> the engine's fp32 tensors
# ------------------------------------------------------------------------------------------
_TAPS = {}


def _taps(kind: str, in_size: int, out_size: int, device) -> torch.Tensor:
    """Device copy of one axis' tap table (packing.pil_bicubic_taps / aten_bicubic_taps), built once per size and device."""
    from . import packing
    key = (kind, in_size, out_size, str(device))
    if key not in _TAPS:
        build = packing.pil_bicubic_taps if kind == "pil" else packing.aten_bicubic_taps
        _TAPS[key] = torch.from_numpy(build(in_size, out_size)).to(device)
    return _TAPS[key]


def resize_u8_pil(frames: torch.Tensor, size, to_float: bool = False) -> torch.Tensor:
    """Pillow's `Image.resize((W, H), BICUBIC)` of uint8 frames (N, Hs, Ws, 3) on the device, bit for bit.
    -> uint8 (N, H, W, 3), or with `to_float` fp32 (3, N, H, W) = x / 255 * 2 - 1 (a clip's (1, 3, T, H, W) after [None])."""
    assert frames.dtype == torch.uint8 and frames.is_cuda and frames.is_contiguous() and frames.dim() == 4 and frames.shape[3] == 3
    n, hs, ws, _ = frames.shape
    h, w = int(size[0]), int(size[1])
    ytab = _taps("pil", hs, h, frames.device)
    xtab = _taps("pil", ws, w, frames.device) if ws != w else None        # Pillow skips the pass of an unchanged axis
    tmp = torch.empty((n, hs, w, 3), dtype=torch.uint8, device=frames.device) if xtab is not None else None
    out = (torch.empty((3, n, h, w), dtype=torch.float32, device=frames.device) if to_float
           else torch.empty((n, h, w, 3), dtype=torch.uint8, device=frames.device))
    hip.check(hip.lib().ccedit_resize_u8_pil(
        frames.data_ptr(), out.data_ptr(), None if tmp is None else tmp.data_ptr(), ytab.data_ptr(), ytab.shape[1] - 2,
        None if xtab is None else xtab.data_ptr(), 0 if xtab is None else xtab.shape[1] - 2, n, hs, ws, h, w, int(to_float),
        _stream()), "ccedit_resize_u8_pil")
    return out


def resize_bicubic(x: torch.Tensor, size) -> torch.Tensor:
    """`F.interpolate(x, size, mode="bicubic", align_corners=False)` of fp32 (N, C, Hs, Ws) on the device."""
    assert x.dtype == torch.float32 and x.is_cuda and x.is_contiguous() and x.dim() == 4
    n, c, hs, ws = x.shape
    h, w = int(size[0]), int(size[1])
    ytab, xtab = _taps("aten", hs, h, x.device), _taps("aten", ws, w, x.device)
    out = torch.empty((n, c, h, w), dtype=torch.float32, device=x.device)
    hip.check(hip.lib().ccedit_resize_f32_bicubic(x.data_ptr(), out.data_ptr(), ytab.data_ptr(), xtab.data_ptr(), n * c, hs, ws, h, w,
                                                  _stream()), "ccedit_resize_f32_bicubic")
    return out


def kth_values(x: torch.Tensor, ranks) -> torch.Tensor:
    """x fp32 (B, n), finite; ranks: up to four 1-based ranks (as torch.kthvalue) -> fp32 (B, len(ranks)) on the device, exact."""
    assert x.dtype == torch.float32 and x.is_cuda and x.is_contiguous() and x.dim() == 2
    ranks = [int(k) for k in ranks]
    b, n = x.shape
    out = torch.empty((b, len(ranks)), dtype=torch.float32, device=x.device)
    ws = torch.empty(b * hip.KTH_WORKSPACE_BYTES_PER_ROW // 4, dtype=torch.int32, device=x.device)
    hip.check(hip.lib().ccedit_kth_values(x.data_ptr(), b, n, (C.c_int64 * len(ranks))(*ranks), len(ranks), out.data_ptr(), ws.data_ptr(),
                                          _stream()), "ccedit_kth_values")
    return out


def minmax(x: torch.Tensor) -> torch.Tensor:
    """x fp32 (B, n), finite -> fp32 (B, 2) = (min, max) per row, on the device."""
    assert x.dtype == torch.float32 and x.is_cuda and x.is_contiguous() and x.dim() == 2
    out = torch.empty((x.shape[0], 2), dtype=torch.float32, device=x.device)
    hip.check(hip.lib().ccedit_minmax_f32(x.data_ptr(), x.shape[0], x.shape[1], out.data_ptr(), _stream()), "ccedit_minmax_f32")
    return out


def depth_hint(depth: torch.Tensor, stats: torch.Tensor, flip: bool) -> torch.Tensor:
    """depth fp32 (B, 1, T, H, W); stats fp32 (B, 2) or (1, 2) = (lo, hi) on the device -> (B, 3, T, H, W):
    clamp((d - lo) / (hi - lo), 0, 1) * 2 - 1, negated with `flip`.  Nothing is read back to the host."""
    assert depth.dtype == torch.float32 and depth.is_cuda and depth.is_contiguous() and depth.dim() == 5 and depth.shape[1] == 1
    assert stats.dtype == torch.float32 and stats.is_cuda and stats.is_contiguous() and stats.dim() == 2 and stats.shape[1] == 2
    b = depth.shape[0]
    assert stats.shape[0] in (1, b)
    out = torch.empty((b, 3) + tuple(depth.shape[2:]), dtype=torch.float32, device=depth.device)
    hip.check(hip.lib().ccedit_depth_hint(depth.data_ptr(), out.data_ptr(), stats.data_ptr(), 2 if stats.shape[0] == b and b > 1 else 0, b,
                                          depth[0].numel(), int(flip), _stream()), "ccedit_depth_hint")
    return out


def frames_to_u8(x: torch.Tensor, rounding: bool = False, unit_range: bool = False) -> torch.Tensor:
    """x fp32 (B, 3, T, H, W) in [-1, 1] (`unit_range`: already in [0, 1]) -> uint8 (B, T, H, W, 3):
    uint8(255 v) of v = clamp((x + 1) / 2, 0, 1), or uint8(min(255 v + 0.5, 255)) with `rounding`."""
    assert x.dtype == torch.float32 and x.is_cuda and x.is_contiguous() and x.dim() == 5 and x.shape[1] == 3
    b, _, t, h, w = x.shape
    out = torch.empty((b, t, h, w, 3), dtype=torch.uint8, device=x.device)
    hip.check(hip.lib().ccedit_frames_to_u8(x.data_ptr(), out.data_ptr(), b, t * h * w, int(rounding), int(unit_range), _stream()),
              "ccedit_frames_to_u8")
    return out


# ------------------------------------------------------------------------------------------
# Edit masks (csrc/mask.hip): set = edit, clear = keep.  Pixel masks: byte >= 128 is set; latent masks: byte != 0
# ------------------------------------------------------------------------------------------
_NEAREST = {}


def mask_resize_nearest(mask: torch.Tensor, size) -> torch.Tensor:
    """Pillow's `Image.resize((W, H), NEAREST)` of uint8 masks (N, Hs, Ws) on the device, byte for byte -> uint8 (N, H, W)."""
    from . import packing
    assert mask.dtype == torch.uint8 and mask.is_cuda and mask.is_contiguous() and mask.dim() == 3
    n, hs, ws = mask.shape
    h, w = int(size[0]), int(size[1])
    tabs = []
    for a, b in ((hs, h), (ws, w)):
        key = (a, b, str(mask.device))
        if key not in _NEAREST:
            _NEAREST[key] = torch.from_numpy(packing.pil_nearest_index(a, b)).to(mask.device)
        tabs.append(_NEAREST[key])
    out = torch.empty((n, h, w), dtype=torch.uint8, device=mask.device)
    hip.check(hip.lib().ccedit_mask_resize_nearest(mask.data_ptr(), out.data_ptr(), tabs[0].data_ptr(), tabs[1].data_ptr(), n, hs, ws, h, w,
                                                   _stream()), "ccedit_mask_resize_nearest")
    return out


def mask_latent(mask_px: torch.Tensor) -> torch.Tensor:
    """Pixel mask uint8 (B, T, H, W) (>= 128 = edit) -> latent mask uint8 (B, T, H / 8, W / 8): 1 where more than 32 of the 64 pixels of
    the cell are set — clamp(round(F.interpolate(mask, (T, H // 8, W // 8), mode="area")), 0, 1) of the binary mask."""
    assert mask_px.dtype == torch.uint8 and mask_px.is_cuda and mask_px.is_contiguous() and mask_px.dim() == 4
    b, t, h, w = mask_px.shape
    assert h % 8 == 0 and w % 8 == 0, f"mask of {h}x{w}: H and W must be multiples of 8"
    out = torch.empty((b, t, h // 8, w // 8), dtype=torch.uint8, device=mask_px.device)
    hip.check(hip.lib().ccedit_mask_latent(mask_px.data_ptr(), out.data_ptr(), b * t, h, w, _stream()), "ccedit_mask_latent")
    return out


def inpaint_blend(x: torch.Tensor, x0: torch.Tensor, noise: torch.Tensor, mask: torch.Tensor, sigma: float, s: float,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The known-region re-injection of an inpainting step in one pass: y = mask ? x : (x0 + noise * sigma) / s over fp32 (B, C, T, h, w)
    with the uint8 latent mask (B, T, h, w) broadcast over C (sampling.py:150-153, 213-216; s = sqrt(1 + sigma^2) from the host).
    `out` may be `x`."""
    for tns in (x, x0, noise):
        assert tns.dtype == torch.float32 and tns.is_cuda and tns.is_contiguous() and tns.shape == x.shape and tns.dim() == 5
    b, c, t, h, w = x.shape
    assert mask.dtype == torch.uint8 and mask.is_cuda and mask.is_contiguous() and tuple(mask.shape) == (b, t, h, w), \
        f"latent mask {tuple(mask.shape)} {mask.dtype} for a latent {tuple(x.shape)}: expected uint8 {(b, t, h, w)}"
    y = torch.empty_like(x) if out is None else out
    assert y.dtype == torch.float32 and y.is_contiguous() and y.shape == x.shape
    n = x.numel()
    _launch_mem("inpaint_blend", 16.0 * n + mask.numel(), lambda: hip.check(hip.lib().ccedit_inpaint_blend(
        x.data_ptr(), x0.data_ptr(), noise.data_ptr(), mask.data_ptr(), y.data_ptr(), b, c, t * h * w, float(sigma), float(s), _stream()),
        "ccedit_inpaint_blend"), (b, c, t, h, w))
    return y


def mask_composite(result: torch.Tensor, original: torch.Tensor, mask_px: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = mask ? result : original over fp32 frames (B, 3, T, H, W) with the uint8 pixel mask (B, T, H, W) (>= 128 = edit) broadcast
    over the channels: the untouched pixels put back after the VAE round trip.  `out` may be `result`."""
    for tns in (result, original):
        assert tns.dtype == torch.float32 and tns.is_cuda and tns.is_contiguous() and tns.shape == result.shape and tns.dim() == 5
    b, c, t, h, w = result.shape
    assert c == 3 and mask_px.dtype == torch.uint8 and mask_px.is_cuda and mask_px.is_contiguous() and tuple(mask_px.shape) == (b, t, h, w), \
        f"pixel mask {tuple(mask_px.shape)} {mask_px.dtype} for frames {tuple(result.shape)}: expected uint8 {(b, t, h, w)}"
    y = torch.empty_like(result) if out is None else out
    assert y.dtype == torch.float32 and y.is_contiguous() and y.shape == result.shape
    hip.check(hip.lib().ccedit_mask_composite(result.data_ptr(), original.data_ptr(), mask_px.data_ptr(), y.data_ptr(), b, t * h * w, _stream()),
              "ccedit_mask_composite")
    return y


# ------------------------------------------------------------------------------------------
# Windows of a long clip (csrc/window.hip): gather W windows of T frames, cross-fade their outputs back (ccedit_amd/windows.py)
# ------------------------------------------------------------------------------------------
def _chk_latent(t: torch.Tensor, name: str):
    if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or t.dim() != 5:
        raise ValueError(f"{name}: expected a contiguous cuda fp32 (B, C, frames, h, w) tensor, got {t.dtype} {t.device} {tuple(t.shape)} "
                         f"contiguous={t.is_contiguous()}")


def window_gather(x: torch.Tensor, starts: torch.Tensor, frames: int) -> torch.Tensor:
    """(B, C, N, h, w) fp32 -> (W, B, C, T, h, w): window i is x[:, :, starts[i]:starts[i] + T], all windows in one launch, a bit copy.
    `starts`: int32 (W,) on the device (windows.plan); the result's [i] are contiguous (B, C, T, h, w) tensors."""
    _chk_latent(x, "window_gather")
    assert starts.dtype == torch.int32 and starts.is_cuda and starts.is_contiguous() and starts.dim() == 1
    b, c, n, h, w = x.shape
    nw, t = starts.shape[0], int(frames)
    xw = torch.empty((nw, b, c, t, h, w), dtype=torch.float32, device=x.device)
    _launch_mem("window_gather", 8.0 * xw.numel(), lambda: hip.check(hip.lib().ccedit_window_gather(
        x.data_ptr(), xw.data_ptr(), starts.data_ptr(), nw, b, c, n, t, h * w, _stream()), "ccedit_window_gather"), (nw, b, c, t, h, w))
    return xw


def window_fuse(ys, starts: torch.Tensor, coef: torch.Tensor, frames: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The W windows' outputs `ys` (each (B, C, T, h, w) fp32, read in place through a device table of their addresses) -> (B, C, N, h, w):
    out[:, :, f] = sum over the windows covering f, ascending, of coef[i, f - starts[i]] * ys[i][:, :, f - starts[i]] — product first,
    then multiply and add per further term, bit-equal to that loop in numpy float32.  `coef`: fp32 (W, T) on the device (windows.plan)."""
    nw, n = len(ys), int(frames)
    assert nw >= 1 and starts.dtype == torch.int32 and starts.is_cuda and starts.is_contiguous() and tuple(starts.shape) == (nw,)
    for y in ys:
        _chk_latent(y, "window_fuse")
        assert y.shape == ys[0].shape and y.device == ys[0].device
    b, c, t, h, w = ys[0].shape
    assert coef.dtype == torch.float32 and coef.is_cuda and coef.is_contiguous() and tuple(coef.shape) == (nw, t)
    y = torch.empty((b, c, n, h, w), dtype=torch.float32, device=ys[0].device) if out is None else out
    assert y.dtype == torch.float32 and y.is_contiguous() and tuple(y.shape) == (b, c, n, h, w)
    # the W addresses change with every evaluation: 8 W bytes through pinned memory, not blocking (see Denoiser.__call__)
    table = torch.tensor([v.data_ptr() for v in ys], dtype=torch.int64).pin_memory().to(y.device, non_blocking=True)
    _launch_mem("window_fuse", 4.0 * (nw * ys[0].numel() + y.numel()), lambda: hip.check(hip.lib().ccedit_window_fuse(
        table.data_ptr(), y.data_ptr(), starts.data_ptr(), coef.data_ptr(), nw, b, c, n, t, h * w, _stream()), "ccedit_window_fuse"),
        (nw, b, c, n, h, w))
    return y


# ------------------------------------------------------------------------------------------
# Tiles of a large frame (csrc/tile.hip): gather T tiles of th x tw, cross-fade their outputs back (ccedit_amd/tiles.py)
# ------------------------------------------------------------------------------------------
def _chk_tile_starts(starts: torch.Tensor, name: str):
    if starts.dtype != torch.int32 or not starts.is_cuda or not starts.is_contiguous() or starts.dim() != 2 or starts.shape[1] != 2:
        raise ValueError(f"{name}: `starts` must be a contiguous cuda int32 (tiles, 2) table of (row, column), got {starts.dtype} "
                         f"{starts.device} {tuple(starts.shape)}")


def tile_gather(x: torch.Tensor, starts: torch.Tensor, tile_h: int, tile_w: int) -> torch.Tensor:
    """(B, C, N, h, w) fp32 -> (T, B, C, N, th, tw): tile i is x[..., sy:sy + th, sx:sx + tw] with (sy, sx) = starts[i], all tiles in one
    launch, a bit copy.  `starts`: int32 (T, 2) on the device (tiles.plan2d); the result's [i] are contiguous (B, C, N, th, tw) tensors."""
    _chk_latent(x, "tile_gather")
    _chk_tile_starts(starts, "tile_gather")
    b, c, n, h, w = x.shape
    nt, th, tw = starts.shape[0], int(tile_h), int(tile_w)
    xt = torch.empty((nt, b, c, n, max(th, 0), max(tw, 0)), dtype=torch.float32, device=x.device)
    _launch_mem("tile_gather", 8.0 * xt.numel(), lambda: hip.check(hip.lib().ccedit_tile_gather(
        x.data_ptr(), xt.data_ptr(), starts.data_ptr(), nt, b * c * n, h, w, th, tw, _stream()), "ccedit_tile_gather"), (nt, b, c, n, th, tw))
    return xt


def tile_fuse(ys, starts: torch.Tensor, coef: torch.Tensor, height: int, width: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The T tiles' outputs `ys` (each (B, C, N, th, tw) fp32, read in place through a device table of their addresses) -> (B, C, N, h, w):
    out[..., y, x] = sum over the tiles covering (y, x), ascending, of coef[i, y - sy_i, x - sx_i] * ys[i][..., y - sy_i, x - sx_i] — product
    first, then multiply and add per further term, bit-equal to that loop in numpy float32.  `coef`: fp32 (T, th, tw) on the device."""
    nt, h, w = len(ys), int(height), int(width)
    if nt < 1:
        raise ValueError("tile_fuse: no tiles")
    _chk_tile_starts(starts, "tile_fuse")
    for y in ys:
        _chk_latent(y, "tile_fuse")
        if y.shape != ys[0].shape or y.device != ys[0].device:
            raise ValueError(f"tile_fuse: tiles of different shapes or devices: {tuple(y.shape)} and {tuple(ys[0].shape)}")
    b, c, n, th, tw = ys[0].shape
    if starts.shape[0] != nt or coef.dtype != torch.float32 or not coef.is_cuda or not coef.is_contiguous() or tuple(coef.shape) != (nt, th, tw):
        raise ValueError(f"tile_fuse: {nt} tiles of {th}x{tw} need starts ({nt}, 2) and a contiguous cuda fp32 coef ({nt}, {th}, {tw}); got "
                         f"{tuple(starts.shape)} and {coef.dtype} {tuple(coef.shape)}")
    y = torch.empty((b, c, n, max(h, 0), max(w, 0)), dtype=torch.float32, device=ys[0].device) if out is None else out
    assert y.dtype == torch.float32 and y.is_contiguous() and tuple(y.shape) == (b, c, n, h, w)
    # the T addresses change with every evaluation: 8 T bytes through pinned memory, not blocking (see window_fuse)
    table = torch.tensor([v.data_ptr() for v in ys], dtype=torch.int64).pin_memory().to(y.device, non_blocking=True)
    _launch_mem("tile_fuse", 4.0 * (nt * ys[0].numel() + coef.numel() + y.numel()), lambda: hip.check(hip.lib().ccedit_tile_fuse(
        table.data_ptr(), y.data_ptr(), starts.data_ptr(), coef.data_ptr(), nt, b * c * n, h, w, th, tw, _stream()), "ccedit_tile_fuse"),
        (nt, b, c, n, h, w))
    return y


# ------------------------------------------------------------------------------------------
# Region prompts (csrc/region.hip): blend coefficients from K pixel masks, blend of the K + 1 evaluations (ccedit_amd/regions.py)
# ------------------------------------------------------------------------------------------
def region_weights(masks: torch.Tensor, feather: int) -> torch.Tensor:
    """uint8 (K, T, H, W) pixel masks (>= 128 = this region's prompt; H, W multiples of 8) -> fp32 (K + 1, T, H / 8, W / 8): coef[0] the base
    prompt's share of every latent cell, coef[r] region r's, from the masks' coverage summed over (2F + 1)^2 cells (regions.py); one
    launch, bit-equal to tests/_regions_numpy.py.  K, F and the sizes are checked by the entry point."""
    if masks.dtype != torch.uint8 or not masks.is_cuda or not masks.is_contiguous() or masks.dim() != 4:
        raise ValueError(f"region_weights: expected a contiguous cuda uint8 (K, T, H, W) tensor, got {masks.dtype} {masks.device} "
                         f"{tuple(masks.shape)} contiguous={masks.is_contiguous()}")
    k, t, hh, ww = masks.shape
    coef = torch.empty((k + 1, t, hh // 8, ww // 8), dtype=torch.float32, device=masks.device)
    _launch_mem("region_weights", float(masks.numel()) + 4.0 * coef.numel(), lambda: hip.check(hip.lib().ccedit_region_weights(
        masks.data_ptr(), coef.data_ptr(), k, t, hh, ww, int(feather), _stream()), "ccedit_region_weights"), (k, t, hh, ww, int(feather)))
    return coef


def region_fuse(ys, coef: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The K + 1 evaluations `ys` (each (B, C, T, h, w) fp32, read in place through a device table of their addresses) -> (B, C, T, h, w):
    out[b, c] = sum over r, ascending, of coef[r] * ys[r][b, c], terms whose coefficient is exactly 0 skipped — product first, then
    multiply and add per further term, bit-equal to that loop in numpy float32.  `coef`: fp32 (K + 1, T, h, w) on the device."""
    nr = len(ys)
    if nr < 1:
        raise ValueError("region_fuse: no regions")
    for y in ys:
        _chk_latent(y, "region_fuse")
        if y.shape != ys[0].shape or y.device != ys[0].device:
            raise ValueError(f"region_fuse: regions of different shapes or devices: {tuple(y.shape)} and {tuple(ys[0].shape)}")
    b, c, t, h, w = ys[0].shape
    if coef.dtype != torch.float32 or not coef.is_cuda or not coef.is_contiguous() or tuple(coef.shape) != (nr, t, h, w):
        raise ValueError(f"region_fuse: {nr} regions of {t} frames of {h}x{w} need a contiguous cuda fp32 coef ({nr}, {t}, {h}, {w}); got "
                         f"{coef.dtype} {coef.device} {tuple(coef.shape)}")
    y = torch.empty((b, c, t, h, w), dtype=torch.float32, device=ys[0].device) if out is None else out
    assert y.dtype == torch.float32 and y.is_contiguous() and tuple(y.shape) == (b, c, t, h, w)
    # the K + 1 addresses change with every evaluation: 8 (K + 1) bytes through pinned memory, not blocking (see window_fuse)
    table = torch.tensor([v.data_ptr() for v in ys], dtype=torch.int64).pin_memory().to(y.device, non_blocking=True)
    _launch_mem("region_fuse", 4.0 * (nr * ys[0].numel() + coef.numel() + y.numel()), lambda: hip.check(hip.lib().ccedit_region_fuse(
        table.data_ptr(), y.data_ptr(), coef.data_ptr(), nr - 1, b, c, t, h * w, _stream()), "ccedit_region_fuse"), (nr, b, c, t, h, w))
    return y


# ------------------------------------------------------------------------------------------
# Automatic edit masks (csrc/automask.hip): from the two halves of a denoiser output to a pixel mask (ccedit_amd/automask.py)
# ------------------------------------------------------------------------------------------
def _chk_cuda(t: torch.Tensor, dtype, name: str, what: str):
    if t.dtype != dtype or not t.is_cuda or not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous cuda {dtype} {what}, got {t.dtype} {t.device} {tuple(t.shape)} "
                         f"contiguous={t.is_contiguous()}")


def automask_accumulate(y: torch.Tensor, acc: Optional[torch.Tensor] = None, first: Optional[bool] = None) -> torch.Tensor:
    """y fp32 (2B, C, T, h, w), the source-prompt half first -> acc fp32 (B, T, h, w): the sum over the channels, ascending, of
    |y[B + b, c] - y[b, c]|, every operation rounded to fp32 (tests/_automask_numpy.py: accumulate).  Without `acc` the sum is stored
    into a new tensor; with it, added to it in place (`first=True`: stored into it)."""
    _chk_latent(y, "automask_accumulate")
    b2, c, t, h, w = y.shape
    if b2 % 2 or b2 < 2:
        raise ValueError(f"automask_accumulate: y {tuple(y.shape)} is not a doubled batch (source-prompt half, target-prompt half)")
    b = b2 // 2
    first = (acc is None) if first is None else bool(first)
    if acc is None:
        if not first:
            raise ValueError("automask_accumulate: first=False adds to `acc`, which was not given")
        acc = torch.empty((b, t, h, w), dtype=torch.float32, device=y.device)
    _chk_cuda(acc, torch.float32, "automask_accumulate", "acc")
    if tuple(acc.shape) != (b, t, h, w) or acc.device != y.device:
        raise ValueError(f"automask_accumulate: acc {tuple(acc.shape)} on {acc.device} for y {tuple(y.shape)}: expected {(b, t, h, w)} on {y.device}")
    _launch_mem("automask_accumulate", 4.0 * (y.numel() + (1 if first else 2) * acc.numel()), lambda: hip.check(
        hip.lib().ccedit_automask_accumulate(y.data_ptr(), acc.data_ptr(), b, c, t * h * w, int(first), _stream()),
        "ccedit_automask_accumulate"), (b, c, t, h, w))
    return acc


def automask_binarize(acc: torch.Tensor, scale: torch.Tensor, theta: float) -> torch.Tensor:
    """acc fp32 (B, T, h, w), scale fp32 (B,) ON THE DEVICE -> uint8 (B, T, h, w): 1 where acc > float32(theta) * scale[b], strictly.
    Nothing is read back."""
    _chk_cuda(acc, torch.float32, "automask_binarize", "acc (B, T, h, w)")
    _chk_cuda(scale, torch.float32, "automask_binarize", "scale (B,)")
    if acc.dim() != 4 or tuple(scale.shape) != (acc.shape[0],) or scale.device != acc.device:
        raise ValueError(f"automask_binarize: acc {tuple(acc.shape)} with scale {tuple(scale.shape)}: expected (B, T, h, w) and (B,) on one device")
    b = acc.shape[0]
    out = torch.empty(acc.shape, dtype=torch.uint8, device=acc.device)
    _launch_mem("automask_binarize", 5.0 * acc.numel(), lambda: hip.check(hip.lib().ccedit_automask_binarize(
        acc.data_ptr(), scale.data_ptr(), float(theta), out.data_ptr(), b, acc[0].numel(), _stream()), "ccedit_automask_binarize"),
        tuple(acc.shape))
    return out


def automask_vote(mask: torch.Tensor, votes: int) -> torch.Tensor:
    """uint8 (B, T, h, w) -> uint8 (B, T, h, w): 1 where at least `votes` (1 ... 27) of the 27 cells around a cell — t, y, x each one step
    either way, clamped into the clip — are set."""
    _chk_cuda(mask, torch.uint8, "automask_vote", "mask (B, T, h, w)")
    if mask.dim() != 4:
        raise ValueError(f"automask_vote: mask {tuple(mask.shape)}: expected (B, T, h, w)")
    b, t, h, w = mask.shape
    out = torch.empty_like(mask)
    _launch_mem("automask_vote", 2.0 * mask.numel(), lambda: hip.check(hip.lib().ccedit_automask_vote(
        mask.data_ptr(), out.data_ptr(), b, t, h, w, int(votes), _stream()), "ccedit_automask_vote"), (b, t, h, w, int(votes)))
    return out


def automask_expand(mask_lat: torch.Tensor) -> torch.Tensor:
    """Latent mask uint8 (B, T, h, w) (!= 0 = edit) -> pixel mask uint8 (B, T, 8h, 8w) in {0, 255}; mask_latent of it is the input's set
    cells as 1."""
    _chk_cuda(mask_lat, torch.uint8, "automask_expand", "latent mask (B, T, h, w)")
    if mask_lat.dim() != 4:
        raise ValueError(f"automask_expand: latent mask {tuple(mask_lat.shape)}: expected (B, T, h, w)")
    b, t, h, w = mask_lat.shape
    out = torch.empty((b, t, 8 * h, 8 * w), dtype=torch.uint8, device=mask_lat.device)
    _launch_mem("automask_expand", 65.0 * mask_lat.numel(), lambda: hip.check(hip.lib().ccedit_automask_expand(
        mask_lat.data_ptr(), out.data_ptr(), b * t, h, w, _stream()), "ccedit_automask_expand"), (b, t, h, w))
    return out


# ------------------------------------------------------------------------------------------
# Weighted prompts (csrc/prompt.hip): the emphasis rule on the text encoder's output (ccedit_amd/prompt.py)
# ------------------------------------------------------------------------------------------
def prompt_weight(z: torch.Tensor, e: torch.Tensor, w: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """z fp32 (B, 77 n, C), e fp32 (77, C) the empty chunk's encoding, w fp32 (B, 77 n) -> e[t mod 77] + w * (z - e[t mod 77]) per row:
    fp32 subtract, multiply, add, bit-equal to tests/_prompt_numpy.py; a row with w == 1 is a bit copy of z.  `out` may be z itself.
    Weights that are not finite are refused here (one reduction of 77 n B floats and one read-back, once per prompt)."""
    for name, tns in (("z", z), ("e", e), ("w", w), ("out", out)):
        if tns is not None and (tns.dtype != torch.float32 or not tns.is_cuda or not tns.is_contiguous()):
            raise ValueError(f"prompt_weight: {name} must be a contiguous cuda fp32 tensor, got {tns.dtype} {tns.device} "
                             f"contiguous={tns.is_contiguous()}")
    if z.dim() != 3 or z.shape[1] % 77 or tuple(e.shape) != (77, z.shape[2]) or tuple(w.shape) != tuple(z.shape[:2]):
        raise ValueError(f"prompt_weight: z (B, 77 n, C), e (77, C) and w (B, 77 n) expected; got {tuple(z.shape)}, {tuple(e.shape)}, {tuple(w.shape)}")
    if out is not None and tuple(out.shape) != tuple(z.shape):
        raise ValueError(f"prompt_weight: out {tuple(out.shape)} is not z's shape {tuple(z.shape)}")
    if not bool(torch.isfinite(w).all()):
        raise ValueError("prompt_weight: a weight is NaN or infinite")
    b, l, c = z.shape
    y = torch.empty_like(z) if out is None else out
    _launch_mem("prompt_weight", 4.0 * (2 * z.numel() + e.numel() + w.numel()), lambda: hip.check(hip.lib().ccedit_prompt_weight(
        z.data_ptr(), e.data_ptr(), w.data_ptr(), y.data_ptr(), b, l, c, _stream()), "ccedit_prompt_weight"), (b, l, c))
    return y


def prompt_schedule(contexts: torch.Tensor, k0, k1, a, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """contexts fp32 (P, L, C) on the device; k0, k1 int32 [N] and a float32 [N]: the HOST table of ccedit_amd/schedule.py's plan ->
    fp32 (N, L, C): contexts[k0] where a == 0, contexts[k1] where a == 1 (bit copies), else c0 + a * (c1 - c0) in fp32 subtract,
    multiply, add: bit-equal to tests/_schedule_numpy.py.  The library checks every index before it launches."""
    import numpy as np
    if contexts.dtype != torch.float32 or not contexts.is_cuda or contexts.dim() != 3:
        raise ValueError(f"prompt_schedule: contexts must be a cuda fp32 tensor (P, L, C), got {contexts.dtype} {contexts.device} {tuple(contexts.shape)}")
    if not contexts.is_contiguous():
        raise ValueError("prompt_schedule: contexts must be contiguous")
    k0 = np.ascontiguousarray(k0, dtype=np.int32)
    k1 = np.ascontiguousarray(k1, dtype=np.int32)
    a = np.ascontiguousarray(a, dtype=np.float32)
    if k0.ndim != 1 or k0.shape != k1.shape or k0.shape != a.shape or k0.size == 0:
        raise ValueError(f"prompt_schedule: k0, k1 and a must be vectors of one length N >= 1, got {k0.shape}, {k1.shape}, {a.shape}")
    p, l, c = contexts.shape
    n = int(k0.size)
    if out is None:
        out = torch.empty((n, l, c), dtype=torch.float32, device=contexts.device)
    elif tuple(out.shape) != (n, l, c) or out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous():
        raise ValueError(f"prompt_schedule: out must be a contiguous cuda fp32 tensor {(n, l, c)}, got {out.dtype} {tuple(out.shape)}")
    i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    _launch_mem("prompt_schedule", 4.0 * 3 * out.numel(), lambda: hip.check(hip.lib().ccedit_prompt_schedule(
        contexts.data_ptr(), k0.ctypes.data_as(i32p), k1.ctypes.data_as(i32p), a.ctypes.data_as(f32p), out.data_ptr(), p, n, l, c, _stream()),
        "ccedit_prompt_schedule"), (p, n, l, c))
    return out


# ------------------------------------------------------------------------------------------
# Propagation of edited keyframes to every source frame (csrc/propagate.hip; plan, tables and the clip loop: ccedit_amd/propagate.py)
# ------------------------------------------------------------------------------------------
def _chk_u8(t: torch.Tensor, name: str, dims: int):
    if t.dtype != torch.uint8 or not t.is_cuda or not t.is_contiguous() or t.dim() != dims:
        raise ValueError(f"{name}: expected a contiguous cuda uint8 tensor of {dims} dimensions, got {t.dtype} {t.device} {tuple(t.shape)} "
                         f"contiguous={t.is_contiguous()}")


def _chk_i32(t: torch.Tensor, name: str, shape):
    if t.dtype != torch.int32 or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected a contiguous cuda int32 tensor {tuple(shape)}, got {t.dtype} {t.device} {tuple(t.shape)}")


def prop_pyramid_bytes(f: int, h: int, w: int) -> int:
    return f * h * w * 85 // 64


def prop_level(pyr: torch.Tensor, f: int, h: int, w: int, level: int) -> torch.Tensor:
    """Level `level` of a pyramid written by prop_pyramid, as a (F, H >> level, W >> level) view."""
    off = sum(f * (h >> l) * (w >> l) for l in range(level))
    return pyr[off:off + f * (h >> level) * (w >> level)].view(f, h >> level, w >> level)


def prop_pyramid(rgb: torch.Tensor) -> torch.Tensor:
    """uint8 frames (F, H, W, 3) -> the four luma levels of all frames in one uint8 buffer (prop_level gives the views)."""
    _chk_u8(rgb, "prop_pyramid", 4)
    f, h, w, c = rgb.shape
    assert c == 3, f"prop_pyramid: RGB frames (F, H, W, 3), got {tuple(rgb.shape)}"
    pyr = torch.empty(prop_pyramid_bytes(f, h, w), dtype=torch.uint8, device=rgb.device)
    hip.check(hip.lib().ccedit_prop_pyramid(rgb.data_ptr(), pyr.data_ptr(), f, h, w, _stream()), "ccedit_prop_pyramid")
    return pyr


def prop_match(pyr: torch.Tensor, pairs: torch.Tensor, rank: torch.Tensor, parent: Optional[torch.Tensor], frames: int, h: int, w: int,
               level: int, radius: int) -> torch.Tensor:
    """One level of the block matching for all pairs (P, 4) of the call -> int32 vectors (P, (h >> level) / 8, (w >> level) / 8, 2)."""
    _chk_u8(pyr, "prop_match", 1)
    assert pyr.numel() == prop_pyramid_bytes(frames, h, w), f"prop_match: a pyramid of {frames} frames {h}x{w} has {prop_pyramid_bytes(frames, h, w)} bytes"
    p = pairs.shape[0]
    _chk_i32(pairs, "prop_match: pairs", (p, 4))
    _chk_i32(rank, "prop_match: rank", ((2 * radius + 1) ** 2,))
    nby, nbx = (h >> level) // 8, (w >> level) // 8
    if parent is not None:
        _chk_i32(parent, "prop_match: parent", (p, nby // 2, nbx // 2, 2))
    out = torch.empty((p, nby, nbx, 2), dtype=torch.int32, device=pyr.device)
    hip.check(hip.lib().ccedit_prop_match(pyr.data_ptr(), pairs.data_ptr(), rank.data_ptr(), None if parent is None else parent.data_ptr(),
                                          out.data_ptr(), p, frames, h, w, level, radius, _stream()), "ccedit_prop_match")
    return out


def prop_warp(src: torch.Tensor, vec: torch.Tensor, pairs: torch.Tensor, col: int) -> torch.Tensor:
    """src uint8 (Fsrc, H, W, 3) or (Fsrc, H, W) warped along the level-0 block vectors `vec` (P, H / 8, W / 8, 2), the source frame of
    pair p taken from column `col` of its row -> uint8 (P, H, W[, 3])."""
    if src.dim() not in (3, 4) or (src.dim() == 4 and src.shape[3] != 3):
        raise ValueError(f"prop_warp: frames (F, H, W, 3) or (F, H, W), got {tuple(src.shape)}")
    _chk_u8(src, "prop_warp", src.dim())
    fs, h, w = src.shape[:3]
    p = pairs.shape[0]
    _chk_i32(pairs, "prop_warp: pairs", (p, 4))
    _chk_i32(vec, "prop_warp: vec", (p, h // 8, w // 8, 2))
    out = torch.empty((p,) + tuple(src.shape[1:]), dtype=torch.uint8, device=src.device)
    hip.check(hip.lib().ccedit_prop_warp(src.data_ptr(), vec.data_ptr(), pairs.data_ptr(), int(col), out.data_ptr(), p, fs, h, w,
                                         3 if src.dim() == 4 else 1, _stream()), "ccedit_prop_warp")
    return out


def prop_blend(warped_rgb: torch.Tensor, warped_luma: torch.Tensor, pyr: torch.Tensor, pairs: torch.Tensor, gtab: torch.Tensor, frames: int,
               rgb: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The two warped keyframes (2 NF, H, W, 3) of every in-between frame, weighted by distance and by the confidence of the warped source
    lumas (2 NF, H, W) against the frame's own luma (level 0 of `pyr`) -> uint8 (NF, H, W, 3).  With `rgb` (F, H, W, 3) and `mask`
    (F, H, W): the source pixel where the frame's own mask is clear (< 128)."""
    _chk_u8(warped_rgb, "prop_blend: warped_rgb", 4)
    p, h, w, _ = warped_rgb.shape
    assert p % 2 == 0 and warped_rgb.shape[3] == 3, f"prop_blend: two warped keyframes per frame, got {tuple(warped_rgb.shape)}"
    _chk_u8(warped_luma, "prop_blend: warped_luma", 3)
    assert tuple(warped_luma.shape) == (p, h, w), f"prop_blend: warped_luma {tuple(warped_luma.shape)} for warped_rgb {tuple(warped_rgb.shape)}"
    _chk_u8(pyr, "prop_blend: pyr", 1)
    assert pyr.numel() == prop_pyramid_bytes(frames, h, w)
    _chk_i32(pairs, "prop_blend: pairs", (p, 4))
    _chk_i32(gtab, "prop_blend: gtab", (256,))
    if (rgb is None) != (mask is None):
        raise ValueError("prop_blend: rgb and mask come together")
    if rgb is not None:
        _chk_u8(rgb, "prop_blend: rgb", 4)
        _chk_u8(mask, "prop_blend: mask", 3)
        assert tuple(rgb.shape) == (frames, h, w, 3) and tuple(mask.shape) == (frames, h, w), \
            f"prop_blend: rgb {tuple(rgb.shape)} / mask {tuple(mask.shape)} for {frames} frames {h}x{w}"
    out = torch.empty((p // 2, h, w, 3), dtype=torch.uint8, device=warped_rgb.device)
    hip.check(hip.lib().ccedit_prop_blend(warped_rgb.data_ptr(), warped_luma.data_ptr(), pyr.data_ptr(), pairs.data_ptr(), gtab.data_ptr(),
                                          None if rgb is None else rgb.data_ptr(), None if mask is None else mask.data_ptr(), out.data_ptr(),
                                          p // 2, frames, h, w, _stream()), "ccedit_prop_blend")
    return out


# ------------------------------------------------------------------------------------------
# Mask tracking (csrc/masktrack.hip, ccedit_mask_dilate in csrc/mask.hip; constants, pair lists and the clip loop: ccedit_amd/masktrack.py)
# ------------------------------------------------------------------------------------------
def _chk_i16(t: torch.Tensor, name: str, shape):
    if t.dtype != torch.int16 or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected a contiguous cuda int16 tensor {tuple(shape)}, got {t.dtype} {t.device} {tuple(t.shape)}")


def masktrack_select(pyr: torch.Tensor, pairs: torch.Tensor, vec: torch.Tensor, frames: int, h: int, w: int) -> torch.Tensor:
    """All pairs (P, 4) of the call: per pixel the best of the 3 x 3 neighbouring blocks' level-0 vectors `vec` (P, h / 8, w / 8, 2) by the
    5 x 5 box sum of absolute luma differences -> int16 (P, h, w, 2) = (dy, dx)."""
    _chk_u8(pyr, "masktrack_select", 1)
    assert pyr.numel() == prop_pyramid_bytes(frames, h, w), f"masktrack_select: a pyramid of {frames} frames {h}x{w} has {prop_pyramid_bytes(frames, h, w)} bytes"
    p = pairs.shape[0]
    _chk_i32(pairs, "masktrack_select: pairs", (p, 4))
    _chk_i32(vec, "masktrack_select: vec", (p, h // 8, w // 8, 2))
    out = torch.empty((p, h, w, 2), dtype=torch.int16, device=pyr.device)
    hip.check(hip.lib().ccedit_masktrack_select(pyr.data_ptr(), pairs.data_ptr(), vec.data_ptr(), out.data_ptr(), p, frames, h, w, _stream()),
              "ccedit_masktrack_select")
    return out


def masktrack_step(v: torch.Tensor, r: torch.Tensor, mask_g: torch.Tensor, limit: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One frame of the chain: per-pixel vectors v (f -> g) and r (g -> f), int16 (H, W, 2), and g's mask uint8 (H, W) -> f's mask:
    mask_g at q = clamp(p + v(p)), or 0 where |v(p) + r(q)|_1 > limit.  `out`: where to write it (a frame of the clip's masks)."""
    _chk_u8(mask_g, "masktrack_step: mask_g", 2)
    h, w = mask_g.shape
    _chk_i16(v, "masktrack_step: v", (h, w, 2))
    _chk_i16(r, "masktrack_step: r", (h, w, 2))
    y = torch.empty((h, w), dtype=torch.uint8, device=mask_g.device) if out is None else out
    _chk_u8(y, "masktrack_step: out", 2)
    assert tuple(y.shape) == (h, w), f"masktrack_step: out {tuple(y.shape)} for a mask of {h}x{w}"
    hip.check(hip.lib().ccedit_masktrack_step(v.data_ptr(), r.data_ptr(), mask_g.data_ptr(), y.data_ptr(), h, w, int(limit), _stream()),
              "ccedit_masktrack_step")
    return y


def mask_dilate(mask: torch.Tensor, radius: int, invert: bool = False) -> torch.Tensor:
    """uint8 masks (..., H, W) -> their (2 radius + 1)^2 square maximum (window clipped at the border), then 255 - m with `invert`.
    radius 0 without invert is the identity: the mask itself comes back and nothing is launched."""
    if not 0 <= int(radius) <= 32:
        raise ValueError(f"mask_dilate: radius={radius} must be in 0 ... 32")
    if int(radius) == 0 and not invert:
        return mask
    _chk_u8(mask, "mask_dilate", mask.dim())
    assert mask.dim() >= 2 and mask.shape[-1] % 4 == 0, f"mask_dilate: masks (..., H, W) with W a multiple of 4, got {tuple(mask.shape)}"
    h, w = mask.shape[-2:]
    out = torch.empty_like(mask)
    tmp = torch.empty_like(mask) if radius else None
    hip.check(hip.lib().ccedit_mask_dilate(mask.data_ptr(), None if tmp is None else tmp.data_ptr(), out.data_ptr(), mask.numel() // (h * w), h, w,
                                           int(radius), int(bool(invert)), _stream()), "ccedit_mask_dilate")
    return out


# ------------------------------------------------------------------------------------------
# Graded edit masks (csrc/softmask.hip; thresholds and the flag check: ccedit_amd/softmask.py).  A strength map: uint8, byte g = g / 255
# ------------------------------------------------------------------------------------------
def mask_feather(mask: torch.Tensor, radius: int) -> torch.Tensor:
    """uint8 maps (..., H, W) -> their mean over the (2 radius + 1)^2 square, the window clipped at the frame border, rounded half up
    ((2 S + A) // (2 A) of the window's sum S and pixel count A).  Per map: nothing crosses frames.  radius 0 is the identity: the map
    itself comes back and nothing is launched."""
    if not 0 <= int(radius) <= 64:
        raise ValueError(f"mask_feather: radius={radius} must be in 0 ... 64")
    if int(radius) == 0:
        return mask
    _chk_u8(mask, "mask_feather", mask.dim())
    assert mask.dim() >= 2 and mask.shape[-1] % 4 == 0, f"mask_feather: maps (..., H, W) with W a multiple of 4, got {tuple(mask.shape)}"
    h, w = mask.shape[-2:]
    out = torch.empty_like(mask)
    tmp = torch.empty(mask.shape, dtype=torch.int16, device=mask.device)          # (the row sums, read as uint16)
    hip.check(hip.lib().ccedit_mask_feather(mask.data_ptr(), tmp.data_ptr(), out.data_ptr(), mask.numel() // (h * w), h, w, int(radius), _stream()),
              "ccedit_mask_feather")
    return out


def mask_latent_graded(mask_px: torch.Tensor) -> torch.Tensor:
    """Pixel strengths uint8 (B, T, H, W) -> latent strengths uint8 (B, T, H / 8, W / 8): (sum of the cell's 64 bytes + 32) >> 6."""
    assert mask_px.dtype == torch.uint8 and mask_px.is_cuda and mask_px.is_contiguous() and mask_px.dim() == 4
    b, t, h, w = mask_px.shape
    assert h % 8 == 0 and w % 8 == 0, f"strength map of {h}x{w}: H and W must be multiples of 8"
    out = torch.empty((b, t, h // 8, w // 8), dtype=torch.uint8, device=mask_px.device)
    hip.check(hip.lib().ccedit_mask_latent_graded(mask_px.data_ptr(), out.data_ptr(), b * t, h, w, _stream()), "ccedit_mask_latent_graded")
    return out


def inpaint_blend_level(x: torch.Tensor, x0: torch.Tensor, noise: torch.Tensor, strength: torch.Tensor, thr: int, sigma: float, s: float,
                        out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """inpaint_blend of a graded run: y = (strength >= thr) ? x : (x0 + noise * sigma) / s over fp32 (B, C, T, h, w) with the uint8 latent
    strengths (B, T, h, w) broadcast over C; thr = softmask.threshold(j, n), 1 ... 255.  `out` may be `x`."""
    if not 1 <= int(thr) <= 255:
        raise ValueError(f"inpaint_blend_level: thr={thr} must be in 1 ... 255")
    for tns in (x, x0, noise):
        assert tns.dtype == torch.float32 and tns.is_cuda and tns.is_contiguous() and tns.shape == x.shape and tns.dim() == 5
    b, c, t, h, w = x.shape
    assert strength.dtype == torch.uint8 and strength.is_cuda and strength.is_contiguous() and tuple(strength.shape) == (b, t, h, w), \
        f"latent strengths {tuple(strength.shape)} {strength.dtype} for a latent {tuple(x.shape)}: expected uint8 {(b, t, h, w)}"
    y = torch.empty_like(x) if out is None else out
    assert y.dtype == torch.float32 and y.is_contiguous() and y.shape == x.shape
    n = x.numel()
    _launch_mem("inpaint_blend_level", 16.0 * n + strength.numel(), lambda: hip.check(hip.lib().ccedit_inpaint_blend_level(
        x.data_ptr(), x0.data_ptr(), noise.data_ptr(), strength.data_ptr(), y.data_ptr(), b, c, t * h * w, int(thr), float(sigma), float(s),
        _stream()), "ccedit_inpaint_blend_level"), (b, c, t, h, w))
    return y


def mask_composite_graded(result: torch.Tensor, original: torch.Tensor, strength_px: torch.Tensor,
                          out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = g == 255 ? result : g == 0 ? original : original + (result - original) * (float(g) / 255) over fp32 frames (B, 3, T, H, W)
    with the uint8 pixel strengths (B, T, H, W) broadcast over the channels, four fp32 roundings.  `out` may be `result`."""
    for tns in (result, original):
        assert tns.dtype == torch.float32 and tns.is_cuda and tns.is_contiguous() and tns.shape == result.shape and tns.dim() == 5
    b, c, t, h, w = result.shape
    assert c == 3 and strength_px.dtype == torch.uint8 and strength_px.is_cuda and strength_px.is_contiguous() \
        and tuple(strength_px.shape) == (b, t, h, w), \
        f"pixel strengths {tuple(strength_px.shape)} {strength_px.dtype} for frames {tuple(result.shape)}: expected uint8 {(b, t, h, w)}"
    y = torch.empty_like(result) if out is None else out
    assert y.dtype == torch.float32 and y.is_contiguous() and y.shape == result.shape
    hip.check(hip.lib().ccedit_mask_composite_graded(result.data_ptr(), original.data_ptr(), strength_px.data_ptr(), y.data_ptr(), b, t * h * w,
                                                     _stream()), "ccedit_mask_composite_graded")
    return y


# ------------------------------------------------------------------------------------------
# Motion-following noise (csrc/noisewarp.hip; constants, the clip's build and the sampler wrap: ccedit_amd/noisewarp.py)
# ------------------------------------------------------------------------------------------
def noisewarp_track(vec: torch.Tensor, key, h: int, w: int, limit: int) -> torch.Tensor:
    """vec: the block vectors int32 (2 (F - 1), h / 8, w / 8, 2) of the adjacent pairs of F frames, for frame f row 2 (f - 1) = (f, f - 1)
    and row 2 (f - 1) + 1 = (f - 1, f); key: the keyframes' frame numbers (host integers, key[0] = 0, strictly increasing, below F)
    -> int32 (K, cells, 3) = (valid, Q_y, Q_x): every cell's centre followed from keyframe k back to keyframe k - 1; row 0 is zero."""
    if vec.dim() != 4 or vec.shape[0] % 2 or vec.shape[0] < 2:
        raise ValueError(f"noisewarp_track: vec (2 (F - 1), h / 8, w / 8, 2) of at least two frames, got {tuple(vec.shape)}")
    frames = vec.shape[0] // 2 + 1
    _chk_i32(vec, "noisewarp_track: vec", (2 * (frames - 1), h // 8, w // 8, 2))
    key = [int(i) for i in key]
    if len(key) < 2 or key[0] != 0 or key[-1] >= frames or any(b <= a for a, b in zip(key, key[1:])):
        raise ValueError(f"noisewarp_track: keyframes {key} of {frames} frames: at least two, from 0, strictly increasing, below the frame count")
    out = torch.zeros((len(key), (h // 8) * (w // 8), 3), dtype=torch.int32, device=vec.device)
    kd = torch.tensor(key, dtype=torch.int32).to(vec.device)
    hip.check(hip.lib().ccedit_noisewarp_track(vec.data_ptr(), kd.data_ptr(), out.data_ptr(), len(key), frames, h, w, int(limit), _stream()),
              "ccedit_noisewarp_track")
    return out


def noisewarp_origins(track: torch.Tensor, h: int, w: int):
    """track: int32 (K, cells, 3) of noisewarp_track -> (org int32 (K, cells, 3) = (R, P_y, P_x), src int32 (K, cells), inherited int32
    (K,)): keyframe 0 is its own origin; then per keyframe a claim and a resolve launch — of the cells that arrive at one sample of an
    earlier keyframe the smallest index inherits it, every other cell is fresh.  The counts stay on the device."""
    cells = (h // 8) * (w // 8)
    k_all = track.shape[0]
    _chk_i32(track, "noisewarp_origins: track", (k_all, cells, 3))
    dev = track.device
    org = torch.empty((k_all, cells, 3), dtype=torch.int32, device=dev)
    src = torch.empty((k_all, cells), dtype=torch.int32, device=dev)
    table = torch.zeros(k_all * cells, dtype=torch.int32, device=dev)          # (read and written as uint32)
    inherited = torch.zeros(k_all, dtype=torch.int32, device=dev)
    lib, st = hip.lib(), _stream()
    for k in range(k_all):
        if k:
            hip.check(lib.ccedit_noisewarp_claim(track.data_ptr(), org.data_ptr(), table.data_ptr(), k, k_all, h, w, st), "ccedit_noisewarp_claim")
        hip.check(lib.ccedit_noisewarp_resolve(track.data_ptr(), org.data_ptr(), table.data_ptr(), src.data_ptr(), inherited.data_ptr(), k, k_all,
                                               h, w, st), "ccedit_noisewarp_resolve")
    return org, src, inherited


def noisewarp_check(src: torch.Tensor) -> None:
    """src: int32 (B, K, cells) index maps.  An index outside 0 ... K cells - 1 is an error status (hip.HipLibraryError).  Waits for the device:
    once per map (noisewarp.wrap), never per draw."""
    if src.dtype != torch.int32 or not src.is_cuda or not src.is_contiguous() or src.dim() != 3:
        raise ValueError(f"noisewarp_check: expected a contiguous cuda int32 map (B, K, cells), got {src.dtype} {src.device} {tuple(src.shape)}")
    flag = torch.empty(1, dtype=torch.int32, device=src.device)
    hip.check(hip.lib().ccedit_noisewarp_check(src.data_ptr(), src.shape[0], src.shape[1] * src.shape[2], flag.data_ptr(), _stream()),
              "ccedit_noisewarp_check")


def noise_warp(raw: torch.Tensor, src: torch.Tensor, out: Optional[torch.Tensor] = None, checked: bool = False) -> torch.Tensor:
    """out[b][c][k][cell] = raw[b][c].flat[src[b][k][cell]] over fp32 (B, C, K, h, w) with int32 maps (B, K, h w): a 4-byte bit copy.
    checked=False: the map's indices are verified first (noisewarp_check: a device round trip) — a caller that verified its map once
    passes checked=True.  `out`: where to write (fp32, the shape of raw, dense; another buffer than raw)."""
    if raw.dtype != torch.float32 or not raw.is_cuda or not raw.is_contiguous() or raw.dim() != 5:
        raise ValueError(f"noise_warp: raw must be a contiguous cuda fp32 tensor (B, C, K, h, w), got {raw.dtype} {raw.device} {tuple(raw.shape)}")
    b, c, k, h, w = raw.shape
    _chk_i32(src, "noise_warp: src", (b, k, h * w))
    y = torch.empty_like(raw) if out is None else out
    if y.dtype != torch.float32 or not y.is_cuda or not y.is_contiguous() or tuple(y.shape) != tuple(raw.shape):
        raise ValueError(f"noise_warp: out must be a contiguous cuda fp32 tensor {tuple(raw.shape)}, got {y.dtype} {y.device} {tuple(y.shape)}")
    if not checked:
        noisewarp_check(src)
    n = k * h * w
    _launch_mem("noise_warp", 12.0 * b * c * n, lambda: hip.check(hip.lib().ccedit_noise_warp(
        raw.data_ptr(), src.data_ptr(), y.data_ptr(), b, c, n, _stream()), "ccedit_noise_warp"), (b, c, k, h, w))
    return y


# ------------------------------------------------------------------------------------------
# Quality report (csrc/quality.hip; constants, what is derived from the integers and the clip's loop: ccedit_amd/quality.py)
# ------------------------------------------------------------------------------------------
def quality_pair(a: torch.Tensor, b: torch.Tensor, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """a, b: uint8 frames (N, H, W, 3); mask: uint8 (N, H, W) or None — a pixel is kept where there is no mask or its byte is < 128
    -> int64 (N, 8) on the device, the accumulators' 64 bits as they are: per frame the squared error of R, G, B over the kept pixels,
    their number, the sum of the SSIM quotient q (scaled by 2^32, signed) over the 8 x 8 windows at stride 4 that are kept whole, the
    number of those windows, and the luma sums of a and of b over the kept pixels."""
    _chk_u8(a, "quality_pair: a", 4)
    _chk_u8(b, "quality_pair: b", 4)
    n, h, w, c = a.shape
    if c != 3 or tuple(b.shape) != tuple(a.shape) or b.device != a.device:
        raise ValueError(f"quality_pair: two clips of RGB frames (N, H, W, 3) on one device, got {tuple(a.shape)} and {tuple(b.shape)}")
    if n < 1 or h < 8 or w < 8 or h % 4 or w % 4:
        raise ValueError(f"quality_pair: {n} frames of {h}x{w}: at least one frame, H and W multiples of 4 and at least 8 (8 x 8 windows at stride 4)")
    if mask is not None:
        _chk_u8(mask, "quality_pair: mask", 3)
        if tuple(mask.shape) != (n, h, w) or mask.device != a.device:
            raise ValueError(f"quality_pair: mask {tuple(mask.shape)} for {n} frames of {h}x{w}")
    acc = torch.empty((n, 8), dtype=torch.int64, device=a.device)
    _launch_mem("quality_pair", float(n * h * w * (6 + (mask is not None))), lambda: hip.check(hip.lib().ccedit_quality_pair(
        a.data_ptr(), b.data_ptr(), _ptr(mask), acc.data_ptr(), n, h, w, _stream()), "ccedit_quality_pair"), (n, h, w))
    return acc


def quality_warp(x: torch.Tensor, vsel: torch.Tensor, pairs: torch.Tensor, limit: int, y: Optional[torch.Tensor] = None,
                 mask: Optional[torch.Tensor] = None, sel: int = 0) -> torch.Tensor:
    """x: uint8 frames (F, H, W, 3), the sequence measured; y: a second one of that shape measured along the same vectors, or None;
    pairs: int32 (2 P, 4), rows 2 j = (f, g, ., .) and 2 j + 1 = (g, f, ., .); vsel: int16 (2 P, H, W, 2), masktrack_select's vectors of those
    rows; mask: uint8 (F, H, W) or None; sel: 0 all pixels, 1 those of frame f with mask >= 128, 2 those with mask < 128.
    -> int64 (P, 4) on the device: the squared error of x and of y (0 without y) over the valid pixels and the three channels, the valid
    pixels — q = p + v(p) lies in frame g and |v(p) + r(q)|_1 <= limit — and the selected pixels."""
    _chk_u8(x, "quality_warp: x", 4)
    f, h, w, c = x.shape
    if c != 3:
        raise ValueError(f"quality_warp: RGB frames (F, H, W, 3), got {tuple(x.shape)}")
    if y is not None:
        _chk_u8(y, "quality_warp: y", 4)
        if tuple(y.shape) != tuple(x.shape) or y.device != x.device:
            raise ValueError(f"quality_warp: y {tuple(y.shape)} shares x's vectors: the shape of x {tuple(x.shape)}, on its device")
    if pairs.dim() != 2 or pairs.shape[0] < 2 or pairs.shape[0] % 2:
        raise ValueError(f"quality_warp: pairs (2 P, 4), two rows per measurement, got {tuple(pairs.shape)}")
    p2 = pairs.shape[0]
    _chk_i32(pairs, "quality_warp: pairs", (p2, 4))
    _chk_i16(vsel, "quality_warp: vsel", (p2, h, w, 2))
    if int(sel) not in (0, 1, 2):
        raise ValueError(f"quality_warp: sel={sel} (0: all pixels, 1: mask >= 128, 2: mask < 128)")
    if int(limit) < 0:
        raise ValueError(f"quality_warp: limit={limit} (not negative)")
    if mask is not None:
        _chk_u8(mask, "quality_warp: mask", 3)
        if tuple(mask.shape) != (f, h, w) or mask.device != x.device:
            raise ValueError(f"quality_warp: mask {tuple(mask.shape)} for {f} frames of {h}x{w}")
    acc = torch.empty((p2 // 2, 4), dtype=torch.int64, device=x.device)
    nbytes = (p2 // 2) * h * w * (8 + 6 * (1 + (y is not None)) + (mask is not None))
    _launch_mem("quality_warp", float(nbytes), lambda: hip.check(hip.lib().ccedit_quality_warp(
        x.data_ptr(), _ptr(y), vsel.data_ptr(), pairs.data_ptr(), _ptr(mask), acc.data_ptr(), p2 // 2, f, h, w, int(limit), int(sel),
        _stream()), "ccedit_quality_warp"), (p2 // 2, h, w))
    return acc


# ------------------------------------------------------------------------------------------
# Motion-JPEG output (csrc/mjpeg.hip; constants, header, container and the frame loop: ccedit_amd/mjpeg.py)
# ------------------------------------------------------------------------------------------
def mjpeg_segment_bytes(w: int) -> int:
    n = int(hip.lib().ccedit_mjpeg_segment_bytes(int(w)))
    if n < 0:
        hip.check(n, "ccedit_mjpeg_segment_bytes")
    return n


def mjpeg_transform(frames: torch.Tensor, tables: torch.Tensor, quality: int) -> torch.Tensor:
    """uint8 frames (N, H, W, 3) -> quantised coefficients int16 (N, H / 16, W / 16, 6, 64): per MCU Y00 Y01 Y10 Y11 Cb Cr, zigzag order."""
    _chk_u8(frames, "mjpeg_transform", 4)
    n, h, w, c = frames.shape
    assert c == 3, f"mjpeg_transform: RGB frames (N, H, W, 3), got {tuple(frames.shape)}"
    _chk_i32(tables, "mjpeg_transform: tables", (816,))
    coef = torch.empty((n, h // 16, w // 16, 6, 64), dtype=torch.int16, device=frames.device)
    hip.check(hip.lib().ccedit_mjpeg_transform(frames.data_ptr(), tables.data_ptr(), coef.data_ptr(), n, h, w, int(quality), _stream()),
              "ccedit_mjpeg_transform")
    return coef


def mjpeg_entropy(coef: torch.Tensor, tables: torch.Tensor):
    """coefficients (N, MR, MC, 6, 64) -> (segments uint8 (N * MR, segment_bytes), seg_len int32 (N * MR,)): one restart interval per
    MCU row, stuffed and padded."""
    if coef.dtype != torch.int16 or not coef.is_cuda or not coef.is_contiguous() or coef.dim() != 5 or tuple(coef.shape[3:]) != (6, 64):
        raise ValueError(f"mjpeg_entropy: expected contiguous cuda int16 coefficients (N, H / 16, W / 16, 6, 64), got {coef.dtype} {tuple(coef.shape)}")
    _chk_i32(tables, "mjpeg_entropy: tables", (816,))
    n, mr, mc = coef.shape[:3]
    segments = torch.empty((n * mr, mjpeg_segment_bytes(mc * 16)), dtype=torch.uint8, device=coef.device)
    seg_len = torch.empty((n * mr,), dtype=torch.int32, device=coef.device)
    hip.check(hip.lib().ccedit_mjpeg_entropy(coef.data_ptr(), tables.data_ptr(), segments.data_ptr(), seg_len.data_ptr(), n, mr * 16, mc * 16,
                                             _stream()), "ccedit_mjpeg_entropy")
    return segments, seg_len


def mjpeg_pack_scan(seg_len: torch.Tensor, frames: int, h: int, w: int, hdr_len: int):
    """-> (seg_off int64 (N * MR,), frame_bytes int32 (N,)): where every segment starts in the packed output, and each frame's size."""
    _chk_i32(seg_len, "mjpeg_pack_scan: seg_len", (frames * (h // 16),))
    seg_off = torch.empty((frames * (h // 16),), dtype=torch.int64, device=seg_len.device)
    frame_bytes = torch.empty((frames,), dtype=torch.int32, device=seg_len.device)
    hip.check(hip.lib().ccedit_mjpeg_pack_scan(seg_len.data_ptr(), seg_off.data_ptr(), frame_bytes.data_ptr(), frames, h, w, int(hdr_len), _stream()),
              "ccedit_mjpeg_pack_scan")
    return seg_off, frame_bytes


def mjpeg_pack(segments: torch.Tensor, seg_len: torch.Tensor, seg_off: torch.Tensor, header: torch.Tensor, frames: int, h: int, w: int,
               out_bytes: int) -> torch.Tensor:
    """-> uint8 (out_bytes,): the frames back to back, each header + segments separated by RSTn + EOI."""
    _chk_u8(segments, "mjpeg_pack: segments", 2)
    _chk_u8(header, "mjpeg_pack: header", 1)
    assert tuple(segments.shape) == (frames * (h // 16), mjpeg_segment_bytes(w)), f"mjpeg_pack: segments {tuple(segments.shape)}"
    _chk_i32(seg_len, "mjpeg_pack: seg_len", (frames * (h // 16),))
    if seg_off.dtype != torch.int64 or not seg_off.is_cuda or not seg_off.is_contiguous() or tuple(seg_off.shape) != tuple(seg_len.shape):
        raise ValueError(f"mjpeg_pack: seg_off: expected a contiguous cuda int64 tensor {tuple(seg_len.shape)}, got {seg_off.dtype} {tuple(seg_off.shape)}")
    out = torch.empty((int(out_bytes),), dtype=torch.uint8, device=segments.device)
    hip.check(hip.lib().ccedit_mjpeg_pack(segments.data_ptr(), seg_len.data_ptr(), seg_off.data_ptr(), header.data_ptr(), out.data_ptr(), frames, h, w,
                                          header.numel(), int(out_bytes), _stream()), "ccedit_mjpeg_pack")
    return out


# ------------------------------------------------------------------------------------------
# JPEG decoding (csrc/jpegdec.hip; the parser, the tables and the frame loop: ccedit_amd/jpegdec.py)
# ------------------------------------------------------------------------------------------
JPEGDEC_TABLE_WORDS = 3416


def jpegdec_plane_bytes(h: int, w: int, ncomp: int, hs: int, vs: int) -> int:
    n = int(hip.lib().ccedit_jpegdec_plane_bytes(int(h), int(w), int(ncomp), int(hs), int(vs)))
    if n < 0:
        hip.check(n, "ccedit_jpegdec_plane_bytes")
    return n


def _jpegdec_counts(h: int, w: int, ncomp: int, hs: int, vs: int, restart_interval: int):
    """-> (blocks per frame, restart intervals per frame)"""
    if ncomp == 1:
        hs = vs = 1
    mcus = -(-w // (8 * hs)) * -(-h // (8 * vs))
    return mcus * (1 if ncomp == 1 else hs * vs + 2), (-(-mcus // restart_interval) if restart_interval else 1)


def jpegdec_entropy(data: torch.Tensor, intervals: torch.Tensor, tables: torch.Tensor, frames: int, h: int, w: int, ncomp: int, hs: int, vs: int,
                    restart_interval: int):
    """entropy-coded bytes (uint8 (B,)) and each restart interval's [start, end) in them (int64 (N * I, 2)) -> (coef int16 (N, blocks, 64):
    MCU order, natural order inside a block; status int32 (N, I): 0, or why the interval stopped)."""
    _chk_u8(data, "jpegdec_entropy: data", 1)
    _chk_i32(tables, "jpegdec_entropy: tables", (JPEGDEC_TABLE_WORDS,))
    if not (0 <= int(restart_interval) <= 65535) or int(frames) < 1:
        raise ValueError(f"jpegdec_entropy: frames={frames} (>= 1), restart_interval={restart_interval} (0 ... 65535)")
    jpegdec_plane_bytes(h, w, ncomp, hs, vs)                # (checks the geometry)
    blocks, per = _jpegdec_counts(h, w, ncomp, hs, vs, int(restart_interval))
    if (intervals.dtype != torch.int64 or not intervals.is_cuda or not intervals.is_contiguous() or tuple(intervals.shape) != (frames * per, 2)
            or data.numel() < 1):
        raise ValueError(f"jpegdec_entropy: intervals: expected a contiguous cuda int64 tensor {(frames * per, 2)} and at least one byte of data, "
                         f"got {intervals.dtype} {tuple(intervals.shape)}, {data.numel()} bytes")
    coef = torch.empty((frames, blocks, 64), dtype=torch.int16, device=data.device)
    status = torch.empty((frames, per), dtype=torch.int32, device=data.device)
    hip.check(hip.lib().ccedit_jpegdec_entropy(data.data_ptr(), data.numel(), intervals.data_ptr(), tables.data_ptr(), coef.data_ptr(),
                                               status.data_ptr(), int(frames), int(h), int(w), int(ncomp), int(hs), int(vs), int(restart_interval),
                                               _stream()), "ccedit_jpegdec_entropy")
    return coef, status


def jpegdec_idct(coef: torch.Tensor, tables: torch.Tensor, h: int, w: int, ncomp: int, hs: int, vs: int) -> torch.Tensor:
    """coef (N, blocks, 64) -> the component planes uint8 (N, plane_bytes): luma, Cb, Cr, each padded to whole MCUs."""
    _chk_i32(tables, "jpegdec_idct: tables", (JPEGDEC_TABLE_WORDS,))
    pb = jpegdec_plane_bytes(h, w, ncomp, hs, vs)
    blocks, _ = _jpegdec_counts(h, w, ncomp, hs, vs, 0)
    if coef.dtype != torch.int16 or not coef.is_cuda or not coef.is_contiguous() or coef.dim() != 3 or tuple(coef.shape[1:]) != (blocks, 64):
        raise ValueError(f"jpegdec_idct: expected contiguous cuda int16 coefficients (N, {blocks}, 64), got {coef.dtype} {tuple(coef.shape)}")
    planes = torch.empty((coef.shape[0], pb), dtype=torch.uint8, device=coef.device)
    hip.check(hip.lib().ccedit_jpegdec_idct(coef.data_ptr(), tables.data_ptr(), planes.data_ptr(), coef.shape[0], int(h), int(w), int(ncomp), int(hs),
                                            int(vs), _stream()), "ccedit_jpegdec_idct")
    return planes


def jpegdec_rgb(planes: torch.Tensor, h: int, w: int, ncomp: int, hs: int, vs: int) -> torch.Tensor:
    """planes (N, plane_bytes) -> uint8 frames (N, H, W, 3)."""
    _chk_u8(planes, "jpegdec_rgb: planes", 2)
    pb = jpegdec_plane_bytes(h, w, ncomp, hs, vs)
    if planes.shape[1] != pb or planes.shape[0] < 1:
        raise ValueError(f"jpegdec_rgb: planes {tuple(planes.shape)}, a frame of {h}x{w} has {pb} bytes of planes")
    out = torch.empty((planes.shape[0], int(h), int(w), 3), dtype=torch.uint8, device=planes.device)
    hip.check(hip.lib().ccedit_jpegdec_rgb(planes.data_ptr(), out.data_ptr(), planes.shape[0], int(h), int(w), int(ncomp), int(hs), int(vs), _stream()),
              "ccedit_jpegdec_rgb")
    return out


# ------------------------------------------------------------------------------------------
# GIF output (csrc/gif.hip; constants, the frame loop and the container: ccedit_amd/gif.py)
# ------------------------------------------------------------------------------------------
def gif_slot_bytes() -> int:
    from . import gif
    n = int(hip.lib().ccedit_gif_slot_bytes())
    if n != gif.SLOT_BYTES:
        raise hip.HipLibraryError(f"ccedit_gif_slot_bytes: the library reserves {n} bytes per chunk, ccedit_amd/gif.py says {gif.SLOT_BYTES}")
    return n


def _gif_frames(frames: torch.Tensor, name: str):
    from . import gif
    _chk_u8(frames, name, 4)
    n, h, w, c = frames.shape
    if c != 3 or n < 1:
        raise ValueError(f"{name}: RGB frames (N, H, W, 3), N >= 1, got {tuple(frames.shape)}")
    gif.check_size(h, w)
    return n, h, w


def _gif_chunks(name: str, n: int, h: int, w: int, chunk: int) -> int:
    from . import gif
    gif.check_size(h, w)
    if int(chunk) != chunk or not 1 <= int(chunk) <= gif.CHUNK or int(n) < 1:
        raise ValueError(f"{name}: frames={n} (>= 1), chunk={chunk!r} pixels (an integer 1 ... {gif.CHUNK})")
    return gif.chunks_of(h, w, chunk)


def gif_histogram(frames: torch.Tensor) -> torch.Tensor:
    """uint8 frames (N, H, W, 3) -> moments int64 (N, 5, 33, 33, 33): count, sum r, sum g, sum b, sum r^2 + g^2 + b^2 per cell
    (r >> 3, g >> 3, b >> 3) at index cell + 1: a zero border."""
    from . import gif
    n, h, w = _gif_frames(frames, "gif_histogram")
    moments = torch.empty((n, gif.MOMENTS, gif.SIDE, gif.SIDE, gif.SIDE), dtype=torch.int64, device=frames.device)
    hip.check(hip.lib().ccedit_gif_histogram(frames.data_ptr(), moments.data_ptr(), n, h, w, _stream()), "ccedit_gif_histogram")
    return moments


def gif_palette(moments: torch.Tensor):
    """moments (N, 5, 33, 33, 33), turned into their inclusive 3-D prefix sums IN PLACE -> (cells uint8 (N, 32, 32, 32): cell -> palette
    index, palettes uint8 (N, 256, 3)): Wu's cuts, the rounded box means."""
    from . import gif
    if (moments.dtype != torch.int64 or not moments.is_cuda or not moments.is_contiguous() or moments.dim() != 5 or moments.shape[0] < 1
            or tuple(moments.shape[1:]) != (gif.MOMENTS, gif.SIDE, gif.SIDE, gif.SIDE)):
        raise ValueError(f"gif_palette: expected contiguous cuda int64 moments (N, {gif.MOMENTS}, {gif.SIDE}, {gif.SIDE}, {gif.SIDE}), got "
                         f"{moments.dtype} {moments.device} {tuple(moments.shape)}")
    n = moments.shape[0]
    cells = torch.empty((n, gif.GRID, gif.GRID, gif.GRID), dtype=torch.uint8, device=moments.device)
    palettes = torch.empty((n, gif.COLORS, 3), dtype=torch.uint8, device=moments.device)
    hip.check(hip.lib().ccedit_gif_palette(moments.data_ptr(), cells.data_ptr(), palettes.data_ptr(), n, _stream()), "ccedit_gif_palette")
    return cells, palettes


def gif_map(frames: torch.Tensor, cells: torch.Tensor) -> torch.Tensor:
    """frames (N, H, W, 3), cells (N, 32, 32, 32) -> indices uint8 (N, H, W)."""
    from . import gif
    n, h, w = _gif_frames(frames, "gif_map")
    _chk_u8(cells, "gif_map: cells", 4)
    if tuple(cells.shape) != (n, gif.GRID, gif.GRID, gif.GRID):
        raise ValueError(f"gif_map: cells {tuple(cells.shape)} for {n} frames: expected {(n, gif.GRID, gif.GRID, gif.GRID)}")
    indices = torch.empty((n, h, w), dtype=torch.uint8, device=frames.device)
    hip.check(hip.lib().ccedit_gif_map(frames.data_ptr(), cells.data_ptr(), indices.data_ptr(), n, h, w, _stream()), "ccedit_gif_map")
    return indices


def gif_lzw(indices: torch.Tensor, chunk: Optional[int] = None):
    """indices (N, H, W) -> (slots uint8 (N * C, slot_bytes), chunk_bits int32 (N * C,)): every chunk of `chunk` pixels (default: gif.CHUNK)
    coded on its own."""
    from . import gif
    chunk = gif.CHUNK if chunk is None else chunk
    _chk_u8(indices, "gif_lzw: indices", 3)
    n, h, w = indices.shape
    c = _gif_chunks("gif_lzw", n, h, w, chunk)
    slots = torch.empty((n * c, gif_slot_bytes()), dtype=torch.uint8, device=indices.device)
    chunk_bits = torch.empty((n * c,), dtype=torch.int32, device=indices.device)
    hip.check(hip.lib().ccedit_gif_lzw(indices.data_ptr(), slots.data_ptr(), chunk_bits.data_ptr(), n, h, w, int(chunk), _stream()), "ccedit_gif_lzw")
    return slots, chunk_bits


def gif_pack_scan(chunk_bits: torch.Tensor, frames: int, h: int, w: int, chunk: Optional[int] = None):
    """-> (chunk_off int64 (N * C,): every chunk's bit offset in the packed output, frame_bytes int32 (N,))."""
    from . import gif
    chunk = gif.CHUNK if chunk is None else chunk
    c = _gif_chunks("gif_pack_scan", frames, h, w, chunk)
    _chk_i32(chunk_bits, "gif_pack_scan: chunk_bits", (frames * c,))
    chunk_off = torch.empty((frames * c,), dtype=torch.int64, device=chunk_bits.device)
    frame_bytes = torch.empty((frames,), dtype=torch.int32, device=chunk_bits.device)
    hip.check(hip.lib().ccedit_gif_pack_scan(chunk_bits.data_ptr(), chunk_off.data_ptr(), frame_bytes.data_ptr(), int(frames), int(h), int(w),
                                             int(chunk), _stream()), "ccedit_gif_pack_scan")
    return chunk_off, frame_bytes


def gif_pack(slots: torch.Tensor, chunk_bits: torch.Tensor, chunk_off: torch.Tensor, frames: int, h: int, w: int, chunk: int,
             out_bytes: int) -> torch.Tensor:
    """-> uint8 (out_bytes,): the frames' LZW byte streams back to back, each its chunks' bits back to back, zero-padded to a byte."""
    c = _gif_chunks("gif_pack", frames, h, w, chunk)
    _chk_u8(slots, "gif_pack: slots", 2)
    if tuple(slots.shape) != (frames * c, gif_slot_bytes()):
        raise ValueError(f"gif_pack: slots {tuple(slots.shape)}: expected {(frames * c, gif_slot_bytes())}")
    _chk_i32(chunk_bits, "gif_pack: chunk_bits", (frames * c,))
    if chunk_off.dtype != torch.int64 or not chunk_off.is_cuda or not chunk_off.is_contiguous() or tuple(chunk_off.shape) != (frames * c,):
        raise ValueError(f"gif_pack: chunk_off: expected a contiguous cuda int64 tensor {(frames * c,)}, got {chunk_off.dtype} {tuple(chunk_off.shape)}")
    if int(out_bytes) < 1:
        raise ValueError(f"gif_pack: out_bytes={out_bytes} (the sum of frame_bytes, >= 1)")
    out = torch.empty(((int(out_bytes) + 3) // 4 * 4,), dtype=torch.uint8, device=slots.device)
    hip.check(hip.lib().ccedit_gif_pack(slots.data_ptr(), chunk_bits.data_ptr(), chunk_off.data_ptr(), out.data_ptr(), int(frames), int(h), int(w),
                                        int(chunk), int(out_bytes), _stream()), "ccedit_gif_pack")
    return out[:int(out_bytes)]


# ------------------------------------------------------------------------------------------
# PNG output (csrc/png.hip; constants, the frame loop and the container: ccedit_amd/png.py).  32-bit words (tokens, histograms, code
# tables, header bits) travel as int32 tensors holding the uint32 bit patterns.
# ------------------------------------------------------------------------------------------
def png_slot_bytes() -> int:
    from . import png
    n, c = int(hip.lib().ccedit_png_slot_bytes()), int(hip.lib().ccedit_png_chunk_bytes())
    if n != png.SLOT_BYTES or c != png.CHUNK:
        raise hip.HipLibraryError(f"ccedit_png_slot_bytes / ccedit_png_chunk_bytes: the library codes chunks of {c} bytes into slots of {n}, "
                                  f"ccedit_amd/png.py says {png.CHUNK} and {png.SLOT_BYTES}")
    return n


def _png_chunks(name: str, t: torch.Tensor, streams: int, width: int) -> int:
    """A per-chunk int32 table (streams * C, width) -> C."""
    if (t.dtype != torch.int32 or not t.is_cuda or not t.is_contiguous() or t.dim() != 2 or t.shape[1] != width or int(streams) < 1
            or t.shape[0] < 1 or t.shape[0] % int(streams)):
        raise ValueError(f"{name}: expected a contiguous cuda int32 tensor (streams * C, {width}) for {streams} streams, got {t.dtype} {t.device} "
                         f"{tuple(t.shape)}")
    return t.shape[0] // int(streams)


def png_filter(frames: torch.Tensor) -> torch.Tensor:
    """uint8 frames (N, H, W, 3) -> filtered uint8 (N, H, 1 + 3 W): per row the filter byte and the filtered bytes."""
    from . import png
    _chk_u8(frames, "png_filter", 4)
    n, h, w, c = frames.shape
    if c != 3 or n < 1:
        raise ValueError(f"png_filter: RGB frames (N, H, W, 3), N >= 1, got {tuple(frames.shape)}")
    png.check_size(h, w)
    out = torch.empty((n, h, png.row_bytes(w)), dtype=torch.uint8, device=frames.device)
    hip.check(hip.lib().ccedit_png_filter(frames.data_ptr(), out.data_ptr(), n, h, w, _stream()), "ccedit_png_filter")
    return out


def _png_streams(filtered: torch.Tensor, name: str):
    from . import png
    _chk_u8(filtered, name, 2)
    n, length = filtered.shape
    if n < 1 or length < 1:
        raise ValueError(f"{name}: byte streams (N, L) with N >= 1 and L >= 1, got {tuple(filtered.shape)}")
    png_slot_bytes()
    return n, length, png.chunks_of(length)


def png_tokens(filtered: torch.Tensor):
    """Byte streams uint8 (N, L) -> (tokens int32 (N * C, CHUNK), ntok int32 (N * C,), hist int32 (N * C, HIST_WORDS)): every chunk of
    png.CHUNK bytes walked on its own."""
    from . import png
    n, length, c = _png_streams(filtered, "png_tokens")
    tokens = torch.empty((n * c, png.CHUNK), dtype=torch.int32, device=filtered.device)
    ntok = torch.empty((n * c,), dtype=torch.int32, device=filtered.device)
    hist = torch.empty((n * c, png.HIST_WORDS), dtype=torch.int32, device=filtered.device)
    hip.check(hip.lib().ccedit_png_tokens(filtered.data_ptr(), tokens.data_ptr(), ntok.data_ptr(), hist.data_ptr(), n, length, _stream()),
              "ccedit_png_tokens")
    return tokens, ntok, hist


def png_codes(hist: torch.Tensor, streams: int):
    """hist (streams * C, HIST_WORDS) -> (codes int32 (streams * C, HIST_WORDS), header int32 (streams * C, HEADER_WORDS), header_bits and
    chunk_bits int32 (streams * C,)); a stream's last chunk gets BFINAL."""
    from . import png
    c = _png_chunks("png_codes: hist", hist, streams, png.HIST_WORDS)
    png_slot_bytes()
    total = hist.shape[0]
    codes = torch.empty((total, png.HIST_WORDS), dtype=torch.int32, device=hist.device)
    header = torch.empty((total, png.HEADER_WORDS), dtype=torch.int32, device=hist.device)
    header_bits = torch.empty((total,), dtype=torch.int32, device=hist.device)
    chunk_bits = torch.empty((total,), dtype=torch.int32, device=hist.device)
    hip.check(hip.lib().ccedit_png_codes(hist.data_ptr(), codes.data_ptr(), header.data_ptr(), header_bits.data_ptr(), chunk_bits.data_ptr(),
                                         int(streams), c, _stream()), "ccedit_png_codes")
    return codes, header, header_bits, chunk_bits


def png_emit(tokens: torch.Tensor, ntok: torch.Tensor, codes: torch.Tensor, header: torch.Tensor, header_bits: torch.Tensor) -> torch.Tensor:
    """-> slots uint8 (chunks, slot_bytes): every chunk's header, tokens and end-of-block, LSB first."""
    from . import png
    total = _png_chunks("png_emit: tokens", tokens, 1, png.CHUNK)
    _png_chunks("png_emit: codes", codes, total, png.HIST_WORDS)
    _png_chunks("png_emit: header", header, total, png.HEADER_WORDS)
    _chk_i32(ntok, "png_emit: ntok", (total,))
    _chk_i32(header_bits, "png_emit: header_bits", (total,))
    slots = torch.empty((total, png_slot_bytes()), dtype=torch.uint8, device=tokens.device)
    hip.check(hip.lib().ccedit_png_emit(tokens.data_ptr(), ntok.data_ptr(), codes.data_ptr(), header.data_ptr(), header_bits.data_ptr(),
                                        slots.data_ptr(), total, _stream()), "ccedit_png_emit")
    return slots


def png_pack_scan(chunk_bits: torch.Tensor, streams: int):
    """-> (chunk_off int64 (streams * C,): every chunk's bit offset in the packed output, frame_bytes int32 (streams,))."""
    if chunk_bits.dim() != 1 or int(streams) < 1 or chunk_bits.shape[0] < 1 or chunk_bits.shape[0] % int(streams):
        raise ValueError(f"png_pack_scan: chunk_bits (streams * C,) for {streams} streams, got {tuple(chunk_bits.shape)}")
    _chk_i32(chunk_bits, "png_pack_scan: chunk_bits", chunk_bits.shape)
    total = chunk_bits.shape[0]
    chunk_off = torch.empty((total,), dtype=torch.int64, device=chunk_bits.device)
    frame_bytes = torch.empty((int(streams),), dtype=torch.int32, device=chunk_bits.device)
    hip.check(hip.lib().ccedit_png_pack_scan(chunk_bits.data_ptr(), chunk_off.data_ptr(), frame_bytes.data_ptr(), int(streams), total // int(streams),
                                             _stream()), "ccedit_png_pack_scan")
    return chunk_off, frame_bytes


def png_pack(slots: torch.Tensor, chunk_bits: torch.Tensor, chunk_off: torch.Tensor, streams: int, out_bytes: int) -> torch.Tensor:
    """-> uint8 (out_bytes,): the streams' deflate bytes back to back, each its chunks' bits back to back, zero-padded to a byte."""
    _chk_u8(slots, "png_pack: slots", 2)
    total = slots.shape[0]
    if int(streams) < 1 or total < 1 or total % int(streams) or slots.shape[1] != png_slot_bytes():
        raise ValueError(f"png_pack: slots {tuple(slots.shape)} for {streams} streams: expected (streams * C, {png_slot_bytes()})")
    _chk_i32(chunk_bits, "png_pack: chunk_bits", (total,))
    if chunk_off.dtype != torch.int64 or not chunk_off.is_cuda or not chunk_off.is_contiguous() or tuple(chunk_off.shape) != (total,):
        raise ValueError(f"png_pack: chunk_off: expected a contiguous cuda int64 tensor {(total,)}, got {chunk_off.dtype} {tuple(chunk_off.shape)}")
    if int(out_bytes) < 1:
        raise ValueError(f"png_pack: out_bytes={out_bytes} (the sum of frame_bytes, >= 1)")
    out = torch.empty(((int(out_bytes) + 3) // 4 * 4,), dtype=torch.uint8, device=slots.device)
    hip.check(hip.lib().ccedit_png_pack(slots.data_ptr(), chunk_bits.data_ptr(), chunk_off.data_ptr(), out.data_ptr(), int(streams),
                                        total // int(streams), int(out_bytes), _stream()), "ccedit_png_pack")
    return out[:int(out_bytes)]


def png_adler(filtered: torch.Tensor) -> torch.Tensor:
    """Byte streams uint8 (N, L) -> their Adler-32 words, int64 (N,) (0 ... 2^32 - 1)."""
    n, length, c = _png_streams(filtered, "png_adler")
    partials = torch.empty((n * c, 2), dtype=torch.int32, device=filtered.device)
    adler = torch.empty((n,), dtype=torch.int32, device=filtered.device)
    hip.check(hip.lib().ccedit_png_adler(filtered.data_ptr(), partials.data_ptr(), adler.data_ptr(), n, length, _stream()), "ccedit_png_adler")
    return adler.to(torch.int64) & 0xffffffff


# ------------------------------------------------------------------------------------------
# PNG decoding (csrc/pngdec.hip; the chunk parser and the frame loop: ccedit_amd/pngdec.py)
# ------------------------------------------------------------------------------------------
def pngdec_inflate(data: torch.Tensor, streams: torch.Tensor, h: int, w: int):
    """zlib streams (uint8 (B,): their bytes; int64 (N, 2): offset and length of each in them) of images of h x w -> (filtered uint8
    (N, h * (1 + 3 w)), status int32 (N, 2): code (0: decoded) and input byte position)."""
    from . import png
    _chk_u8(data, "pngdec_inflate: data", 1)
    png.check_size(h, w)
    if (streams.dtype != torch.int64 or not streams.is_cuda or not streams.is_contiguous() or streams.dim() != 2 or streams.shape[1] != 2
            or streams.shape[0] < 1 or data.numel() < 1):
        raise ValueError(f"pngdec_inflate: streams: expected a contiguous cuda int64 tensor (N, 2), N >= 1, and at least one byte of data, "
                         f"got {streams.dtype} {tuple(streams.shape)}, {data.numel()} bytes")
    n = streams.shape[0]
    filtered = torch.empty((n, png.filtered_bytes(h, w)), dtype=torch.uint8, device=data.device)
    status = torch.empty((n, 2), dtype=torch.int32, device=data.device)
    hip.check(hip.lib().ccedit_pngdec_inflate(data.data_ptr(), data.numel(), streams.data_ptr(), filtered.data_ptr(), status.data_ptr(), n, int(h),
                                              int(w), _stream()), "ccedit_pngdec_inflate")
    return filtered, status


def pngdec_unfilter(filtered: torch.Tensor, h: int, w: int):
    """filtered uint8 (N, h * (1 + 3 w)) -> (uint8 frames (N, h, w, 3), status int32 (N, 2): code (0, or 12: a filter byte above 4) and
    that byte's offset)."""
    from . import png
    _chk_u8(filtered, "pngdec_unfilter: filtered", 2)
    png.check_size(h, w)
    if filtered.shape[0] < 1 or filtered.shape[1] != png.filtered_bytes(h, w):
        raise ValueError(f"pngdec_unfilter: filtered {tuple(filtered.shape)}, an image of {h}x{w} has {png.filtered_bytes(h, w)} filtered bytes")
    n = filtered.shape[0]
    out = torch.empty((n, int(h), int(w), 3), dtype=torch.uint8, device=filtered.device)
    status = torch.empty((n, 2), dtype=torch.int32, device=filtered.device)
    hip.check(hip.lib().ccedit_pngdec_unfilter(filtered.data_ptr(), out.data_ptr(), status.data_ptr(), n, int(h), int(w), _stream()),
              "ccedit_pngdec_unfilter")
    return out, status


# ------------------------------------------------------------------------------------------
# GIF decoding (csrc/gifdec.hip; the container parser, the descriptors and the frame loop: ccedit_amd/gifdec.py)
# ------------------------------------------------------------------------------------------
def _gifdec_desc(desc: torch.Tensor, name: str) -> int:
    from . import gifdec
    if (desc.dtype != torch.int64 or not desc.is_cuda or not desc.is_contiguous() or desc.dim() != 2 or desc.shape[1] != gifdec.DESC_WORDS
            or desc.shape[0] < 1):
        raise ValueError(f"{name}: desc: expected a contiguous cuda int64 tensor (N, {gifdec.DESC_WORDS}), N >= 1, got {desc.dtype} {tuple(desc.shape)}")
    return desc.shape[0]


def gifdec_codes(data: torch.Tensor, desc: torch.Tensor, total_codes: int):
    """The LZW streams in `data` (uint8 (B,)) of the images described by `desc` (int64 (N, 16): gifdec.py describe) -> (table int32
    (3, total_codes): parent, len, off of every data code; ends uint8 (2, total_codes): first and last byte of its string; ncodes int32
    (N,); status int32 (N, 2): code (0: decoded) and bit position).  No pixel is touched."""
    _chk_u8(data, "gifdec_codes: data", 1)
    n = _gifdec_desc(desc, "gifdec_codes")
    if int(total_codes) < 1 or data.numel() < 1:
        raise ValueError(f"gifdec_codes: total_codes={total_codes} (>= 1: the sum of the descriptors' capacities), {data.numel()} bytes of data")
    table = torch.empty((3, int(total_codes)), dtype=torch.int32, device=data.device)
    ends = torch.empty((2, int(total_codes)), dtype=torch.uint8, device=data.device)
    ncodes = torch.empty((n,), dtype=torch.int32, device=data.device)
    status = torch.empty((n, 2), dtype=torch.int32, device=data.device)
    hip.check(hip.lib().ccedit_gifdec_codes(data.data_ptr(), data.numel(), desc.data_ptr(), table[0].data_ptr(), table[1].data_ptr(),
                                            table[2].data_ptr(), ends[0].data_ptr(), ends[1].data_ptr(), int(total_codes), ncodes.data_ptr(),
                                            status.data_ptr(), n, _stream()), "ccedit_gifdec_codes")
    return table, ends, ncodes, status


def gifdec_pixels(desc: torch.Tensor, table: torch.Tensor, ends: torch.Tensor, ncodes: torch.Tensor, plane_bytes: int, max_codes: int) -> torch.Tensor:
    """The code table of gifdec_codes -> planes uint8 (plane_bytes,): every image's indices in stream order at its descriptor's plane
    offset.  max_codes: the largest capacity among the descriptors."""
    n = _gifdec_desc(desc, "gifdec_pixels")
    _chk_u8(ends, "gifdec_pixels: ends", 2)
    if table.dtype != torch.int32 or not table.is_cuda or not table.is_contiguous() or table.dim() != 2 or table.shape[0] != 3 \
            or tuple(ends.shape) != (2, table.shape[1]) or table.shape[1] < 1:
        raise ValueError(f"gifdec_pixels: expected table int32 (3, C) and ends uint8 (2, C), got {table.dtype} {tuple(table.shape)}, {tuple(ends.shape)}")
    _chk_i32(ncodes, "gifdec_pixels: ncodes", (n,))
    total = table.shape[1]
    if int(plane_bytes) < 1 or not 1 <= int(max_codes) <= total:
        raise ValueError(f"gifdec_pixels: plane_bytes={plane_bytes} (>= 1), max_codes={max_codes} (1 ... {total})")
    planes = torch.empty((int(plane_bytes),), dtype=torch.uint8, device=desc.device)
    hip.check(hip.lib().ccedit_gifdec_pixels(desc.data_ptr(), table[0].data_ptr(), table[1].data_ptr(), table[2].data_ptr(), ends[1].data_ptr(),
                                             total, ncodes.data_ptr(), planes.data_ptr(), int(plane_bytes), n, int(max_codes), _stream()),
              "ccedit_gifdec_pixels")
    return planes


def gifdec_compose(data: torch.Tensor, desc: torch.Tensor, planes: torch.Tensor, canvas: torch.Tensor, n_out: int):
    """The images' index planes composited in order on `canvas` (uint8 (H, W, 3), updated in place) -> (uint8 (n_out, H, W, 3): the images
    whose descriptor names an output; status int32 (N, 2): code (0, or 5: an index beyond the palette) and the offset in the plane)."""
    from . import gif
    _chk_u8(data, "gifdec_compose: data", 1)
    _chk_u8(planes, "gifdec_compose: planes", 1)
    _chk_u8(canvas, "gifdec_compose: canvas", 3)
    n = _gifdec_desc(desc, "gifdec_compose")
    h, w = canvas.shape[0], canvas.shape[1]
    gif.check_size(h, w)
    if canvas.shape[2] != 3 or not 0 <= int(n_out) <= n or data.numel() < 1 or planes.numel() < 1:
        raise ValueError(f"gifdec_compose: canvas {tuple(canvas.shape)} (H, W, 3), n_out={n_out} (0 ... {n}), {data.numel()} bytes of data, "
                         f"{planes.numel()} of planes")
    out = torch.empty((int(n_out), h, w, 3), dtype=torch.uint8, device=canvas.device)
    status = torch.empty((n, 2), dtype=torch.int32, device=canvas.device)
    status[:, 0] = 0
    status[:, 1] = 0x7fffffff
    hip.check(hip.lib().ccedit_gifdec_compose(data.data_ptr(), data.numel(), desc.data_ptr(), planes.data_ptr(), planes.numel(), canvas.data_ptr(),
                                              out.data_ptr() if n_out else None, status.data_ptr(), n, int(n_out), h, w, _stream()),
              "ccedit_gifdec_compose")
    return out, status
