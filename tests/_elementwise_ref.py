"""float64 references, per-element bounds and fp32 emulations of the kernels of csrc/elementwise.hip.

Three things per operation, all on the CPU:

  ref_*    the operation in float64, written from its definition (the formula the comment above the kernel cites), by explicit
           index arithmetic.  tests/test_elementwise_ref.py holds each against the obvious torch expression.
  bound_*  the largest |got - ref| a CORRECT kernel may show, element by element.  Derived here from the number formats and the
           arithmetic the kernel does, never from what a kernel returned.
  emu_*    the kernel's own steps in float32 (output rounded to bf16 where the kernel rounds), with switches that each plant ONE
           defect.  The correct emulation has to pass the bound and each defect has to miss it: that is the evidence that
           tests/test_elementwise_gpu.py would notice a subtly wrong kernel.

Scalars that cross the C ABI as `float` (scale, sigma, a, b, shift) are rounded to fp32 before they are used, here as there: f32().

bf16 rounding.  bf16 keeps 8 significant bits (7 stored), so one ulp of r in [2^e, 2^(e+1)) is 2^(e-7) and round-to-nearest of an
exact r is within half of it, 2^(e-8) <= 2^-8 |r|; the bound is tight just above 2^e (at the first tie, r = 2^e (1 + 2^-8)).  The
kernels round an fp32 value v = r (1 + eps) and not r itself: |bf16(v) - r| <= 2^(e-8) + |eps| |r|.  So every bound below is
2^-8 |ref| plus a slack for eps, and the slack is derived per operation.
"""
import math

import numpy as np
import torch

BF = torch.bfloat16
F64 = torch.float64
F32 = torch.float32

GRID_ITEMS = 8192 * 256                    # grid_for(): at most 8192 workgroups of 256 threads -> one loop pass covers this many items
WRAP_ITEMS = GRID_ITEMS + 3 * 256 + 5      # every thread of the capped grid runs a second pass, the last workgroup is ragged
SENT_BF_BITS = 0x7FC0                      # bf16 quiet NaN: no kernel here produces it from finite inputs
SENT_F32_BITS = 0x7FC5A5A5                  # an fp32 quiet NaN with a payload: an ordinary value such as -7.0 can be a legitimate result
#                                            (among millions of fp32 results one is, now and then) and would read as never written

LN10000_F32 = float(np.float32(9.210340371976184))       # the literal of timestep_embedding_kernel, as fp32 holds it
LOG2E_F32 = float(np.float32(1.4426950408889634))


def f32(v: float) -> float:
    """A Python float as the C ABI's `float` parameter receives it."""
    return float(np.float32(v))


def rnd_bf(*shape, seed=0, scale=1.0):
    """bf16-representable fp32 normal values (what tests/test_ops_gpu.py: _rnd makes)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF).float()


def rnd_f32(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def all_bf16_in(lo: float, hi: float) -> torch.Tensor:
    """Every finite bf16 value in [lo, hi] (both signs of zero included), as fp32."""
    bits = torch.arange(0, 1 << 16, dtype=torch.int32).to(torch.int16)
    v = bits.view(BF).float()
    return v[torch.isfinite(v) & (v >= lo) & (v <= hi)].contiguous()


# ------------------------------------------------------------------------------------------
# comparison
# ------------------------------------------------------------------------------------------
def excess(got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor) -> float:
    """max over elements of |got - ref| / bound (0 / 0 counts as 0, anything over a zero bound or non-finite as inf)."""
    got, ref, bound = got.to(F64).reshape(-1), ref.to(F64).reshape(-1), bound.to(F64).reshape(-1)
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    if not bool(torch.isfinite(got).all()):
        return math.inf
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)      # err > 0 over bound == 0 gives inf
    return float(ratio.max()) if ratio.numel() else 0.0


def assert_within(got, ref, bound, what=""):
    e = excess(got, ref, bound)
    if e > 1.0:
        g, r, b = got.to(F64).reshape(-1), ref.to(F64).reshape(-1), bound.to(F64).reshape(-1)
        bad = (~torch.isfinite(g)) | ((g - r).abs() > b)
        i = int(torch.nonzero(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {g.numel()} elements outside their bound, worst {e:.3g} x; first at flat index {i}: "
                             f"got {float(g[i])!r}, reference {float(r[i])!r}, bound {float(b[i]):.3g}")
    return e


def assert_bits_equal(got: torch.Tensor, want: torch.Tensor, what=""):
    """Same dtype, same shape, same bit patterns (so -0 != +0 and a NaN equals itself)."""
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype} {tuple(got.shape)} vs {want.dtype} {tuple(want.shape)}"
    it = {2: torch.int16, 4: torch.int32}[got.element_size()]
    a, b = got.contiguous().view(it).reshape(-1), want.contiguous().view(it).reshape(-1)
    if not torch.equal(a, b):
        bad = torch.nonzero(a != b).reshape(-1)
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.numel()} of {a.numel()} elements differ in bits; first at flat index {i}: "
                             f"got {float(got.reshape(-1)[i])!r}, want {float(want.reshape(-1)[i])!r}")


def sentinel_fill(numel: int, dtype, device="cpu") -> torch.Tensor:
    if dtype == BF:
        return torch.full((numel,), SENT_BF_BITS, dtype=torch.int16, device=device).view(BF)
    assert dtype == F32
    return torch.full((numel,), SENT_F32_BITS, dtype=torch.int32, device=device).view(F32)


def is_sentinel(t: torch.Tensor) -> torch.Tensor:
    if t.dtype == BF:
        return t.contiguous().view(torch.int16) == SENT_BF_BITS
    assert t.dtype == F32
    return t.contiguous().view(torch.int32) == SENT_F32_BITS


def assert_sentinels(buf: torch.Tensor, written: torch.Tensor, what=""):
    """buf: the whole flat output buffer, guard region included; written: bool mask of the elements the call has to write.  Every
    written element has lost the sentinel and every other one still holds it."""
    s = is_sentinel(buf.reshape(-1).cpu())
    w = written.reshape(-1)
    assert s.shape == w.shape
    left = s & w
    assert not bool(left.any()), f"{what}: {int(left.sum())} elements never written, first at flat index {int(torch.nonzero(left)[0])}"
    hit = ~s & ~w
    assert not bool(hit.any()), f"{what}: {int(hit.sum())} elements written outside the output, first at flat index {int(torch.nonzero(hit)[0])}"


# ------------------------------------------------------------------------------------------
# layout changes
# ------------------------------------------------------------------------------------------
def ref_ncthw_to_nhwc(x, cpad, scale_per_b=None, scale=1.0, shift=0.0):
    """(B, C, T, H, W) -> float64 (B*T, H, W, cpad): y[b*T + t, h, w, c] = x[b, c, t, h, w] * scale * scale_per_b[b] + shift, 0 for c >= C."""
    b, c, t, h, w = x.shape
    y = torch.zeros((b * t, h, w, cpad), dtype=F64)
    for bi in range(b):
        sc = f32(scale) * (float(scale_per_b[bi]) if scale_per_b is not None else 1.0)
        for ci in range(c):
            for ti in range(t):
                y[bi * t + ti, :, :, ci] = x[bi, ci, ti].to(F64) * sc + f32(shift)
    return y


def bound_ncthw_to_nhwc(x, cpad, scale_per_b=None, scale=1.0, shift=0.0):
    """fp32: scale_per_b[b] * scale (1 rounding), x * sc (1), + shift (1; one fewer with an FMA) -> at most 3 * 2^-24 relative to
    M = |x sc| + |shift|; 2^-22 M leaves a third in hand.  Then the bf16 rounding.  With scale 1, no scale_per_b and shift 0 the fp32
    steps are exact and the result is bit-equal to bf16(x): the GPU test asks for that instead."""
    ref = ref_ncthw_to_nhwc(x, cpad, scale_per_b, scale, shift)
    m = ref_ncthw_to_nhwc(x.abs(), cpad, None if scale_per_b is None else scale_per_b.abs(), abs(scale), abs(shift))
    b, c = x.shape[:2]
    m[..., c:] = 0                        # pad channels: exactly zero
    return 2.0 ** -8 * ref.abs() + 2.0 ** -22 * m


def emu_ncthw_to_nhwc(x, cpad, scale_per_b=None, scale=1.0, shift=0.0, pad_garbage=False):
    b, c, t, h, w = x.shape
    sc = torch.full((b,), f32(scale), dtype=F32)
    if scale_per_b is not None:
        sc = scale_per_b.to(F32) * sc
    v = x.to(F32) * sc.view(b, 1, 1, 1, 1) + torch.tensor(f32(shift), dtype=F32)
    y = torch.zeros((b * t, h, w, cpad), dtype=F32)
    y[..., :c] = v.permute(0, 2, 3, 4, 1).reshape(b * t, h, w, c)
    if pad_garbage and cpad > c:
        y[..., c:] = f32(shift)            # defect: the pad channels get `0 * sc + shift` instead of 0
    return y.to(BF)


def ref_nhwc_to_ncthw(x, b, t, c):
    """(B*T, H, W, ld) -> (B, c, T, H, W) in the input's values widened to fp32: y[b, c, t, h, w] = x[b*T + t, h, w, c]."""
    n, h, w, ld = x.shape
    assert n == b * t and c <= ld
    y = torch.empty((b, c, t, h, w), dtype=F32)
    for bi in range(b):
        for ti in range(t):
            for ci in range(c):
                y[bi, ci, ti] = x[bi * t + ti, :, :, ci].to(F32)
    return y


# ------------------------------------------------------------------------------------------
# one-add kernels (exact: one fp32 add, one rounding)
# ------------------------------------------------------------------------------------------
def ref_cat_add(a, b, c=None):
    """(rows, C1) ++ ((rows, C2) + (rows, C2)) in float64."""
    rows, c1, c2 = a.shape[0], a.shape[1], b.shape[1]
    y = torch.empty((rows, c1 + c2), dtype=F64)
    y[:, :c1] = a.to(F64)
    y[:, c1:] = b.to(F64) + (c.to(F64) if c is not None else 0.0)
    return y


def exact_cat_add(a, b, c=None):
    """The bits a correct kernel writes: a copied, (b + c) added in fp32 and rounded once."""
    rows, c1, c2 = a.shape[0], a.shape[1], b.shape[1]
    y = torch.empty((rows, c1 + c2), dtype=BF)
    y[:, :c1] = a
    y[:, c1:] = b if c is None else (b.float() + c.float()).to(BF)
    return y


def exact_add(a, b):
    return (a.float() + b.float()).to(BF)


def bound_bf16_exact_arith(ref):
    """An fp32 add of two bf16 values whose exponents differ by less than 16 is exact, so the only error is the rounding."""
    return 2.0 ** -8 * ref.abs()


def exact_embedding_lookup(ids, tok, pos):
    """ids (B, L) int64, tok (vocab, C) fp32, pos (L, C) fp32 -> bf16 (B*L, C) = tok[ids] + pos, one fp32 add and one rounding."""
    b, l = ids.shape
    out = torch.empty((b * l, tok.shape[1]), dtype=BF)
    for li in range(l):                       # position by position: rows li, li + L, ...
        out[li::l] = (tok[ids[:, li]] + pos[li]).to(BF)
    return out


def ref_embedding_lookup(ids, tok, pos):
    b, l = ids.shape
    return (tok.to(F64)[ids.reshape(-1)] + pos.to(F64).repeat(b, 1))


def bound_embedding_lookup(ids, tok, pos):
    """One fp32 add (2^-24 of the result, bounded by the terms) and the bf16 rounding."""
    b, l = ids.shape
    m = tok.to(F64).abs()[ids.reshape(-1)] + pos.to(F64).abs().repeat(b, 1)
    return 2.0 ** -8 * ref_embedding_lookup(ids, tok, pos).abs() + 2.0 ** -23 * m


# ------------------------------------------------------------------------------------------
# silu
# ------------------------------------------------------------------------------------------
def ref_silu(x):
    """x / (1 + exp(-x)) in float64; exp(-x) = inf for x < -709 gives -0."""
    x = x.to(F64)
    return x / (1.0 + torch.exp(-x))


def bound_silu(x):
    """2^-8 |ref| (bf16) + 2^-22 |x| (fp32), u = 2^-24.  The kernel computes x * rcp(1 + exp2(-x log2e)).  -x log2e is rounded to
    fp32, |x| u relative in e = exp(-x); v_exp_f32 is 1 ulp (2u).  The sigmoid s = 1 / (1 + e) follows e with relative sensitivity
    1 - s; the sum and the product are one rounding each (u) and v_rcp_f32 1 ulp (2u).  So the result's absolute error is at most
    |x| s ((1 - s)(|x| + 2) + 4) u, and with |x| s (1 - s) <= 0.23 that is (4 s + 0.7) u |x|: 2^-22 |x| = 4u |x| up to the last
    fraction, which the first term supplies (it exceeds the actual rounding error by 2^-16 |ref| at least, see the module docstring).
    emu_silu checks the sum of it over every bf16 input."""
    x = x.to(F64)
    ref = ref_silu(x).abs()
    return 2.0 ** -8 * ref + silu_f32_term(x) + flush_term(ref)


def silu_f32_term(x):
    """The fp32 share of bound_silu (derivation there): what silu_f's own arithmetic may add to a result BEFORE it is rounded to
    the output format.  tests/_epilogue_ref.py uses it as the SiLU budget of the GEMM epilogues, which call the same silu_f."""
    return 2.0 ** -22 * x.to(F64).abs()


def flush_term(ref_abs):
    """A result below 2^-126 is subnormal in bf16 as in fp32: no 8-bit significand there, and the hardware may flush it (the fp32
    emulation on subnormal bf16 inputs misses the other terms by 256 x: the quantum of a bf16 subnormal is 2^-133)."""
    return torch.where(ref_abs < 2.0 ** -126, 2.0 ** -126, 0.0)


def emu_silu(x, ieee_div=False):
    x = x.to(F32)
    e = torch.exp2(-x * torch.tensor(LOG2E_F32, dtype=F32))
    if ieee_div:
        return (x / (1.0 + e)).to(BF)
    return (x * (1.0 / (1.0 + e))).to(BF)


def silu_exp_overflows(x):
    """Where exp(-x) is beyond fp32: the kernel's sigmoid is rcp(inf) = 0 there and the result a signed zero."""
    return torch.exp(-x.to(F64)) > float(np.finfo(np.float32).max)


# ------------------------------------------------------------------------------------------
# timestep embedding
# ------------------------------------------------------------------------------------------
def ref_timestep_embedding(t, dim):
    """[cos(t f_k) | sin(t f_k)], f_k = exp(-ln(10000) k / half), k < half = dim / 2: float64 (n, dim)."""
    half = dim // 2
    out = torch.empty((t.shape[0], dim), dtype=F64)
    for k in range(half):
        f = math.exp(-math.log(10000.0) * k / half)
        out[:, k] = torch.cos(t.to(F64) * f)
        out[:, half + k] = torch.sin(t.to(F64) * f)
    return out


def bound_timestep_embedding(ref):
    """The argument a = t f is computed in fp32, u = 2^-24.  The exponent x = ln(10000) k / half carries three roundings (the
    literal, the product, the quotient): 3u x absolute, which is 3u x relative in f = exp(-x); expf adds two ulps, 4u; t * f one
    rounding, u.  So |a - t f| <= t f (3u x + 5u), and since x exp(-x) <= 1 / e that is at most 999 * (3 / e + 5) * 2^-24 = 3.6e-4
    for t <= 999.  cos and sin have slope <= 1 and are themselves good to an ulp, so 2^-10 = 9.8e-4 is an absolute term with a factor
    of 2.7 in hand; then the bf16 rounding."""
    return 2.0 ** -8 * ref.abs() + 2.0 ** -10


def emu_timestep_embedding(t, dim, k_off=0, swap=False):
    half = dim // 2
    k = torch.arange(half, dtype=F32) + k_off
    f = torch.exp(torch.tensor(LN10000_F32, dtype=F32).neg() * k / torch.tensor(float(half), dtype=F32))
    a = t.to(F32)[:, None] * f[None, :]
    c, s = torch.cos(a), torch.sin(a)
    return (torch.cat([s, c], dim=1) if swap else torch.cat([c, s], dim=1)).to(BF)


# ------------------------------------------------------------------------------------------
# fp32 kernels: 2^-20 of the sum of the magnitudes of the expanded expression's terms
# ------------------------------------------------------------------------------------------
def bound_terms(m):
    """m: float64 sum of |term| over the expanded expression.  Each kernel's result carries at most five roundings of 2^-24, each
    relative to a partial result that the terms' magnitudes bound (derivations with the operations below), so a correct result is
    within 5 * 2^-24 < 2^-21 m whether or not the compiler contracts to FMA; 2^-20 leaves a factor of two."""
    return 2.0 ** -20 * m


def ref_gaussian_sample(moments, noise, zc, scale=1.0):
    """moments (frames*hw, ldm >= 2 zc) rows [mean(zc) | logvar(zc) | ...]; noise (frames, zc, h, w) ->
    scale * (mean + exp(0.5 clamp(logvar, -30, 20)) * noise), float64 NCHW.  Returns (ref, M)."""
    n, c, h, w = noise.shape
    assert c == zc and moments.shape[0] == n * h * w and moments.shape[1] >= 2 * zc
    ref = torch.empty(noise.shape, dtype=F64)
    mag = torch.empty(noise.shape, dtype=F64)
    s = f32(scale)
    for ci in range(zc):
        mean = moments[:, ci].to(F64).reshape(n, h, w)
        logvar = moments[:, zc + ci].to(F64).reshape(n, h, w)
        std = torch.exp(0.5 * torch.minimum(torch.maximum(logvar, torch.tensor(-30.0, dtype=F64)), torch.tensor(20.0, dtype=F64)))
        ref[:, ci] = s * (mean + std * noise[:, ci].to(F64))
        mag[:, ci] = abs(s) * (mean.abs() + (std * noise[:, ci].to(F64)).abs())
    return ref, mag        # roundings: expf (2 ulp), * noise, + mean, * scale; 0.5 * logvar and the clamp are exact


def emu_gaussian_sample(moments, noise, zc, scale=1.0, clamp=True, ld_tight=False, clamp_low=True, clamp_high=True):
    n, c, h, w = noise.shape
    mom = moments.to(F32)
    if ld_tight:                                # defect: rows read 2 * zc apart although the buffer's rows are wider
        flat = mom.contiguous().reshape(-1)
        mom = torch.as_strided(flat, (n * h * w, 2 * zc), (2 * zc, 1))
    mean = mom[:, :zc].reshape(n, h, w, zc).permute(0, 3, 1, 2)
    logvar = mom[:, zc:2 * zc].reshape(n, h, w, zc).permute(0, 3, 1, 2)
    if clamp and clamp_low:
        logvar = logvar.clamp(min=-30.0)
    if clamp and clamp_high:
        logvar = logvar.clamp(max=20.0)
    return torch.tensor(f32(scale), dtype=F32) * (mean + torch.exp(0.5 * logvar) * noise.to(F32))


def ref_mask_blend(x, z, m):
    """x m + z (1 - m).  Returns (ref, M)."""
    x, z, m = x.to(F64), z.to(F64), m.to(F64)
    return x * m + z * (1.0 - m), (x * m).abs() + (z * (1.0 - m)).abs()      # roundings: 1 - m, z *, x *, +


def emu_mask_blend(x, z, m, swap=False):
    x, z, m = x.to(F32), z.to(F32), m.to(F32)
    if swap:
        return x * (1.0 - m) + z * m
    return x * m + z * (1.0 - m)


def ref_cfg_denoise(x, eps2, sigma, scale):
    """DiscreteDenoiser (c_out = -sigma, c_skip = 1) on both halves of eps2 = [uncond | cond], then VanillaCFG:
    d_u + scale (d_c - d_u), d = x - sigma eps.  Returns (ref, M), M over the expansion
    (x - sigma e_u) + scale (x - sigma e_c) - scale (x - sigma e_u).

    Roundings, u = 2^-24, M_u = |x| + |sigma e_u|, M_c likewise: d_u and d_c two each (<= 2u M_u, 2u M_c); d_c - d_u one more
    (<= 3u (M_u + M_c) with the inherited ones); scale * that and + d_u one each: in all <= 3u M_u + 5u |scale| (M_u + M_c) <= 5u M."""
    n = x.numel()
    xf, e = x.to(F64).reshape(-1), eps2.to(F64).reshape(-1)
    assert e.numel() == 2 * n
    sg, sc = f32(sigma), f32(scale)
    du, dc = xf - sg * e[:n], xf - sg * e[n:]
    mu, mc = xf.abs() + (sg * e[:n]).abs(), xf.abs() + (sg * e[n:]).abs()
    return (du + sc * (dc - du)).reshape(x.shape), (mu + abs(sc) * (mu + mc)).reshape(x.shape)


def emu_cfg_denoise(x, eps2, sigma, scale, swap=False):
    n = x.numel()
    xf, e = x.to(F32).reshape(-1), eps2.to(F32).reshape(-1)
    eu, ec = (e[n:], e[:n]) if swap else (e[:n], e[n:])
    sg, sc = torch.tensor(f32(sigma), dtype=F32), torch.tensor(f32(scale), dtype=F32)
    du, dc = eu * -sg + xf, ec * -sg + xf
    return (du + sc * (dc - du)).reshape(x.shape)


def ref_axpby(x, z, a, b):
    """a x + b z.  Returns (ref, M = |a x| + |b z|): relative to the terms, so the cancellation of (1, -1) is covered."""
    x, z = x.to(F64), z.to(F64)
    return f32(a) * x + f32(b) * z, (f32(a) * x).abs() + (f32(b) * z).abs()


def emu_axpby(x, z, a, b, swap=False):
    if swap:
        a, b = b, a
    return torch.tensor(f32(a), dtype=F32) * x.to(F32) + torch.tensor(f32(b), dtype=F32) * z.to(F32)


# ------------------------------------------------------------------------------------------
# softmax over rows, bf16 out, zero pad
# ------------------------------------------------------------------------------------------
def ref_softmax_rows(s, cols, cols_pad, scale):
    """s (rows, >= cols) -> float64 (rows, cols_pad): exp(v - max v) / sum over the row, v = s[:, :cols] * scale; 0 in [cols, cols_pad)."""
    v = s[:, :cols].to(F64) * f32(scale)
    e = torch.exp(v - v.max(dim=1, keepdim=True).values)
    out = torch.zeros((s.shape[0], cols_pad), dtype=F64)
    out[:, :cols] = e / e.sum(dim=1, keepdim=True)
    return out


def bound_softmax_rows(ref):
    """2^-8 ref (bf16) + 2^-20 ref (fp32) + 2^-126 (subnormal results may be flushed).

    The fp32 error of one element, relative: s * scale rounded (|v| 2^-24 in the exponential), v - max rounded and its product with
    log2(e) rounded (|v - max| 2^-24 each), v_exp_f32, the sum of at most 8192 terms in four-way tree order, the reciprocal and the
    product (together below 2^-21); the rounding of max itself is common to the row and cancels.  Only elements above 2^-126 matter,
    there |v - max| < 88, and the GPU cases keep |v| <= 80 wherever the result is not flushed: at most (80 + 88 + 88) 2^-24 = 2^-16 in
    the extreme, about 2^-18 typically.  That is more than 2^-20, and still inside this bound: where the bf16 rounding error reaches
    2^-8 |2^e| (r at a tie, r >= 2^e (1 + 2^-8)) the term 2^-8 ref exceeds it by 2^-16 2^e, and below the first tie the value rounds
    to 2^e, with an error of r - 2^e itself.  emu_softmax_rows checks this with the kernel's steps."""
    return (2.0 ** -8 + 2.0 ** -20) * ref + 2.0 ** -126


def emu_softmax_rows(s, cols, cols_pad, scale, max_first64=False, pad_garbage=False, drop_wave=None):
    rows = s.shape[0]
    v = torch.full((rows, 8192), -math.inf, dtype=F32)
    v[:, :cols] = s[:, :cols].to(F32) * torch.tensor(f32(scale), dtype=F32)
    col = torch.arange(8192)
    src = v
    if max_first64:                 # defect: only wave 0 of the workgroup (threads 0..63: columns c with c % 256 < 64) feeds the maximum
        src = torch.where((col % 256 < 64)[None, :], v, torch.tensor(-math.inf))
    if drop_wave is not None:       # defect: the cross-wave maximum drops one of the four waves
        src = torch.where(((col % 256) // 64 != drop_wave)[None, :], v, torch.tensor(-math.inf))
    mx = src.max(dim=1, keepdim=True).values
    e = torch.exp2((v - mx) * torch.tensor(LOG2E_F32, dtype=F32))
    # the kernel's order of summation: thread tid adds its 32 register slots in order, the wave's 64 lanes in a butterfly, the four waves last
    part = e.reshape(rows, 32, 256)
    acc = torch.zeros((rows, 256), dtype=F32)
    for k in range(32):
        acc = acc + part[:, k, :]
    w = acc.reshape(rows, 4, 64)
    o = 32
    while o:
        w = w + w[:, :, torch.arange(64) ^ o]
        o >>= 1
    tot = ((w[:, 0, 0] + w[:, 1, 0]) + w[:, 2, 0]) + w[:, 3, 0]
    inv = (1.0 / tot)[:, None]
    out = (e[:, :cols_pad] * inv)
    out[:, cols:] = 0.0
    out = out.to(BF)
    if pad_garbage and cols_pad > cols:
        out[:, cols:] = sentinel_fill(1, BF)[0]          # defect: the pad columns are left as they were
    return out


# ------------------------------------------------------------------------------------------
# copy_2d_blocks, byte for byte
# ------------------------------------------------------------------------------------------
def emu_copy_2d_blocks(src_bytes: np.ndarray, dst_bytes: np.ndarray, blocks, rows, row_bytes, src_pitch, dst_pitch, dst_uses_src_pitch=False):
    """The kernel's definition on flat uint8 arrays: for every block (src offset, dst offset) and r < rows,
    dst[do + r dst_pitch : + row_bytes] = src[so + r src_pitch : + row_bytes]."""
    if dst_uses_src_pitch:
        dst_pitch = src_pitch
    for so, do in blocks:
        for r in range(rows):
            dst_bytes[do + r * dst_pitch: do + r * dst_pitch + row_bytes] = src_bytes[so + r * src_pitch: so + r * src_pitch + row_bytes]
    return dst_bytes


def to_heads_blocks(rows, c, world, parts=3):
    """The plans of RowShard.to_heads for q | k | v as column blocks of one (rows, parts * c) projection: per part j the blocks
    (source element offset, destination element offset) of the world column slices, cw = c / world wide."""
    cw = c // world
    return [[(j * c + r * cw, ((r * parts + j) * rows) * cw) for r in range(world)] for j in range(parts)]


def from_heads_blocks(rows, c, world):
    """The plan of RowShard.from_heads: (world * rows, cw) contiguous buffers into the columns of (rows, c)."""
    cw = c // world
    return [(r * rows * cw, r * cw) for r in range(world)]


# ------------------------------------------------------------------------------------------
# inputs shared by the CPU and the GPU tests
# ------------------------------------------------------------------------------------------
SOFTMAX_PEAK_COLS = (0, 64, 128, 192, 192 + 31 * 256)      # one column per wave of the workgroup, and a late register slot
SOFTMAX_KINDS = ("random", "constant", "peaks", "span80")


def softmax_input(kind, rows, cols, lds, scale, seed=0):
    """fp32 (rows, lds): columns [cols, lds) alternate +inf and NaN (they must not be read).
    random: N(0, 3^2); constant: one value per row (every output 1 / cols); peaks: N(0, 1) with one column per row lifted so that
    s * scale is 100 above the rest — a maximum that misses that column's wave overflows exp; span80: s * scale spread evenly over
    [-80, 80] in shuffled order."""
    g = torch.Generator().manual_seed(seed)
    sc = f32(scale)
    if kind == "random":
        s = torch.randn(rows, cols, generator=g) * 3.0
    elif kind == "constant":
        s = (torch.randn(rows, 1, generator=g) * 3.0).expand(rows, cols).clone()
    elif kind == "peaks":
        s = torch.randn(rows, cols, generator=g) / sc
        peaks = [c for c in SOFTMAX_PEAK_COLS if c < cols] or [cols - 1]
        for r in range(rows):
            s[r, peaks[r % len(peaks)]] = 100.0 / sc
    elif kind == "span80":
        base = torch.linspace(-80.0, 80.0, cols) if cols > 1 else torch.tensor([80.0])
        s = torch.stack([base[torch.randperm(cols, generator=g)] for _ in range(rows)]) / sc
    else:
        raise KeyError(kind)
    full = torch.empty((rows, lds), dtype=F32)
    full[:, :cols] = s
    full[:, cols::2] = math.inf
    full[:, cols + 1::2] = math.nan
    return full


def gaussian_inputs(frames, zc, h, w, ldm, seed=0):
    """(wide, moments, noise): `wide` fp32 (frames*h*w, ldm) with NaN beyond the 2 zc moment columns, `moments` its [:, :2 zc] view.
    logvar cycles through clamped-low (< -30), exactly -30, exactly 20, clamped-high (> 20) and ordinary values in [-6, 2]; the
    cycle runs over the channel too, so a call of 16 elements has every kind and every call has the first, -45.  Where logvar is far
    below -30 the mean is 0: std is at most e^-15 there, and next to a mean of ordinary size a missing lower clamp would vanish in
    the bound, which is relative to |mean| + |std noise|."""
    g = torch.Generator().manual_seed(seed)
    rows = frames * h * w
    wide = torch.full((rows, ldm), math.nan, dtype=F32)
    wide[:, :zc] = torch.randn(rows, zc, generator=g) * 2.0
    ordinary = torch.rand(rows, zc, generator=g) * 8.0 - 6.0
    special = torch.tensor([-45.0, -30.0, 20.0, 27.5, -30.000002, 20.000002, -1e4, 88.0])
    pick = (torch.arange(rows)[:, None] * zc + torch.arange(zc)[None, :]) % 16
    wide[:, zc:2 * zc] = torch.where(pick < 8, special[pick % 8], ordinary)
    wide[:, :zc] = torch.where(wide[:, zc:2 * zc] < -31.0, torch.zeros(()), wide[:, :zc])
    noise = torch.randn(frames, zc, h, w, generator=g)
    return wide, wide[:, :2 * zc], noise
