"""Dyadic operands, float64 references, per-element bounds and fp32 emulations of the GEMM epilogues: activations and the bf16 store.

tests/_exact_ints.py makes every number a matrix kernel can form an integer, so the kernels are held bit for bit — but only where
the epilogue is linear, and only on results that are bf16 numbers already (|r| <= 256), so the store never rounds.  Here the same
recipe runs on a DYADIC grid: activations are integers, weights are {-1, 0, 1} * 2^-s, biases, row biases and residuals multiples
of 2^-4.  Every product and every partial sum in any order is a multiple of 2^-G (G = max(s, 4)) below 2^24 grid units: exact in
fp32.  So whatever the tile shape, K order, split or lane map, the fp32 value p that reaches the activation is known exactly in
float64, and only the epilogue is left to be judged:

  * no activation, bf16 out: the output is bf16_rne(p + residuals), bit for bit.  Results carry up to 12 significant bits, so the
    store ROUNDS; `tie_census` counts the exact ties among them and the generator asserts a minimum, with both parities of the
    kept bit (a truncating store, or one that rounds ties away from zero, cannot pass);
  * with an activation: |got - ref64| <= A + 1/2 ulp_out(|ref| + A) for every element, A being the budget of the activation's
    own arithmetic (`budget_*` below, each with its derivation) and the second term the one rounding of the store: the kernel
    rounds v with |v - ref| <= A, and the rounding error of v is at most half an ulp of |v| <= |ref| + A.

Per operation: ref_* (float64, from the definition), budget_* / bound_* (never fitted to a kernel's output), emu_* (the kernel's
own steps in fp32, written from csrc/common.h, csrc/gemm_epilogue.h, csrc/gemm8p.hip and csrc/ff320.hip, with switches that each
plant ONE defect).  tests/test_epilogue_ref.py shows on the CPU that every correct emulation meets its bound on the operands the
GPU tests use and that every planted defect misses it.

The second half of the file carries the same for the LayerNorm computed inside a kernel (tests/test_fused_layernorm_gpu.py): rows on
which that LayerNorm is exact in fp32 (`ln_rows`), fp32 emulations of ff320.hip's and lin320.hip's statistics, the ff320 block tail with
its derived bound, and the bound of the ln_sums consumer.
"""
import functools
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _elementwise_ref as R  # noqa: E402
import _exact_ints as E  # noqa: E402

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U = 2.0 ** -24                      # unit roundoff of fp32
ACT_NONE, ACT_SILU, ACT_QUICK_GELU = 0, 1, 3      # include/ccedit_hip.h (2 is GEGLU: a property of the packed weight)
QG_F32 = float(np.float32(1.702))   # the literal of gemm_epilogue.h as fp32 holds it
GELU_FIT = tuple(float(np.float32(c)) for c in (0.00101426306, -0.106775724, -2.30112134))      # common.h: gelu_erf_f
GELU_FIT_ABS = 3e-5                 # common.h states 2.6e-5 absolute for the fitted form; 3e-5 with its fp32 evaluation
AS_7_1_28 = tuple(float(np.float32(c)) for c in (0.0000430638, 0.0002765672, 0.0001520143, 0.0092705272, 0.0422820123, 0.0705230784))
AS_ERF_ABS = 3e-7                   # ff320.hip / Abramowitz & Stegun 7.1.28: |erf error| <= 3e-7
SQRT_HALF_F32 = float(np.float32(0.70710678118654752440))
GATE_RANGES = ((-12.0, -9.0, "[)"), (-9.0, -4.0, "[)"), (-4.0, -1.0, "[)"), (-1.0, 1.0, "[]"), (1.0, 4.0, "(]"), (4.0, 9.0, "(]"),
               (9.0, 12.0, "(]"))
MIN_PER_GATE_RANGE = 64             # gates in every range of GATE_RANGES (beyond +-9: the clamp)
MIN_TIE_SHARE = 1.0 / 64            # of the outputs of a rounding case are exact ties ...
MIN_PARITY_SHARE = 0.25             # ... and each parity of the kept bit has this share of the ties
SAT = 96.0                          # SiLU / quick-GELU: one channel block biased to -SAT (exp overflows), one to +SAT (saturated)


# ------------------------------------------------------------------------------------------
# number formats
# ------------------------------------------------------------------------------------------
def _f32_bits(v64):
    """float64 values that fp32 holds exactly -> their int64 fp32 bit patterns."""
    f = v64.to(F32)
    assert bool((f.to(F64) == v64).all()), "the value is not an fp32 number: the grid premise is broken"
    return f.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF


def _from_bits(bits):
    hi = (bits >> 16).to(torch.int32)
    return torch.where(hi >= 0x8000, hi - 0x10000, hi).to(torch.int16).view(BF)


def bf16_rne(v64):
    """Round-to-nearest-even to bf16 by integer arithmetic on the fp32 bit pattern (no cast of the library's is trusted)."""
    b = _f32_bits(v64)
    return _from_bits(b + 0x7FFF + ((b >> 16) & 1))


def bf16_trunc(v64):
    return _from_bits(_f32_bits(v64))


def bf16_ties_away(v64):
    return _from_bits(_f32_bits(v64) + 0x8000)


def store(v32, how="rne"):
    """An fp32 tensor through the kernel's f2bf, or one of the two defective stores."""
    return {"rne": bf16_rne, "trunc": bf16_trunc, "away": bf16_ties_away}[how](v32.to(F64))


def tie_census(v64):
    """(ties, kept bit even, kept bit odd): elements exactly half-way between two bf16 numbers, by the parity of the bit that stays."""
    b = _f32_bits(v64)
    tie = (b & 0xFFFF) == 0x8000
    odd = tie & (((b >> 16) & 1) == 1)
    return int(tie.sum()), int((tie & ~odd).sum()), int(odd.sum())


def assert_ties(v64, what=""):
    """The condition on the INPUTS of a rounding case: enough exact ties, both parities."""
    t, even, odd = tie_census(v64)
    n = v64.numel()
    assert t >= MIN_TIE_SHARE * n, f"{what}: {t} exact ties among {n} outputs, fewer than 1/64"
    assert min(even, odd) >= MIN_PARITY_SHARE * t, f"{what}: ties with an even / odd kept bit {even} / {odd}: one parity is short"
    return t, even, odd


def ulp(y, out_f32=False):
    """One unit in the last place of the output format at magnitude y >= 0 (float64): 2^(floor(log2 y) - 7) for bf16, - 23 for fp32;
    below 2^-126 the spacing of 2^-126's binade (what happens there is flush_term's business)."""
    _, e = torch.frexp(y.to(F64).clamp_min(2.0 ** -126))          # y = m 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(y, dtype=F64), e - (24 if out_f32 else 8))


def bound(ref, a, out_f32=False):
    """A + 1/2 ulp(|ref| + A) (+ 2^-126 where the result is subnormal and may be flushed)."""
    ref = ref.to(F64).abs()
    return a + 0.5 * ulp(ref + a, out_f32) + R.flush_term(ref)


# ------------------------------------------------------------------------------------------
# references (float64) and budgets
# ------------------------------------------------------------------------------------------
def ref_silu(v):
    return R.ref_silu(v)


def ref_quick_gelu(v):
    """v * sigmoid(1.702 v) (the CLIP text encoder's activation)."""
    v = v.to(F64)
    return v / (1.0 + torch.exp(-1.702 * v))


def ref_gelu_erf(g):
    g = g.to(F64)
    return 0.5 * g * (1.0 + torch.special.erf(g * math.sqrt(0.5)))


def ref_act(p, act):
    return {ACT_NONE: lambda v: v.to(F64), ACT_SILU: ref_silu, ACT_QUICK_GELU: ref_quick_gelu}[act](p)


def ref_geglu(value, gate):
    return value.to(F64) * ref_gelu_erf(gate)


def ref_epilogue(p, act, res=()):
    """The order gemm_epilogue.h implements: act(acc + bias + row bias) + res1 + res2; p is the pre-activation."""
    y = ref_act(p, act)
    for r in res:
        y = y + r
    return y


def budget_silu(p):
    return R.silu_f32_term(p)


def budget_quick_gelu(p):
    """2^-22 |v| = 4u |v|, u = 2^-24, for `v / (1.0f + __expf(-1.702f * v))` with an IEEE division.

    The exponent t = -1.702 v is formed as fl(c v) with c = fp32(1.702), |c / 1.702 - 1| = 1.3e-8 < u/4, and one rounding of the
    product, u; __expf is v_exp_f32(t log2e): the literal log2e as fp32 (1.3e-8 < u/4) and that product's rounding, u.  So the
    exponent is off by at most 2.5u |t| absolutely, which is the relative error of e = exp(t); v_exp_f32 adds 1 ulp = 2u.  With
    s = 1 / (1 + e) the sensitivity of s to e is (1 - s); 1 + e is one rounding (u) and the IEEE quotient v / (1 + e) another (u).
    The result v s therefore carries at most |v| s ((1 - s)(2.5 * 1.702 |v| + 2) + 2) u.  z s(z)(1 - s(z)) <= 0.2239 for the
    logistic s over all z = 1.702 |v|, so (1 - s) s 2.5 z <= 0.56, and 2 s (1 - s) + 2 s = 2 s (2 - s) <= 2: at most 2.56u |v| in
    all.  4u |v| leaves a third in hand.  Where exp overflows (1.702 |v| > 88.7, v < 0) the quotient is -0 and the
    reference below 2^-126: bound() adds flush_term there, as bound_silu does."""
    return 2.0 ** -22 * p.to(F64).abs()


def budget_act(p, act):
    if act == ACT_NONE:
        return torch.zeros_like(p, dtype=F64)
    return budget_silu(p) if act == ACT_SILU else budget_quick_gelu(p)


def budget_residual_adds(parts):
    """act(p) + res1 + res2 are fp32 additions of an inexact number: each rounds once, by at most u times the magnitude of its
    result, which the sum of the terms' magnitudes bounds.  `parts`: |act(p)|, |res1|, ... (float64); zero without residuals."""
    if len(parts) <= 1:
        return torch.zeros_like(parts[0])
    return (len(parts) - 1) * U * sum(parts)


def bound_epilogue(p, act, res=(), out_f32=False):
    """(ref, bound) of one SiLU / quick-GELU epilogue element by element."""
    a = ref_act(p, act)
    ref = ref_epilogue(p, act, res)
    budget = budget_act(p, act) + budget_residual_adds([a.abs()] + [r.abs() for r in res])
    return ref, bound(ref, budget, out_f32)


def budget_geglu(value, gate=None):
    """|value| * 3e-5: gelu_erf_f of common.h is good to 2.6e-5 ABSOLUTE as the source states (fp32 evaluation against fp64 erf on
    the host); v_exp_f32 and v_rcp_f32 are 1 ulp each on the device and the product with the value one rounding — at most 4u of
    |value gelu| <= 12 |value|, 2.9e-6 |value|, at the largest gate of the grid.  Where the approximation error peaks (|gate| ~ 3)
    that is 7e-7 |value|: 2.6e-5 + 0.1e-5 < 3e-5."""
    return value.to(F64).abs() * GELU_FIT_ABS


def budget_gelu_pipe(gate):
    """The budget of ff320.hip's GeluPipe for gelu(u) ALONE (times |value| for the product), from the stated 3e-7 of A&S 7.1.28:

        x = |u| / sqrt 2;  p = 1 + a1 x + ... + a6 x^6 (six fmas);  p^16 by four squarings;  erf = 1 - rcp(p^16);
        2 gelu = fma(|u|, erf, u);  result = (0.5 v) * that.

    Approximation: 3e-7 on erf.  fp32, u = 2^-24: x carries the literal's and the product's rounding, 1.25u; p is a Horner chain
    of positive terms, so its own six roundings add at most 2u relatively, and x's error moves it by 1.25u x p'/p.  Sixteen-fold
    through the squarings, whose own roundings add 8 + 4 + 2 + 1 = 15u, and v_rcp_f32 2u: erfc = p^-16 is off relatively by
    20u x p'/p + 49u.  Since p^-16 = erfc, 16 x p'/p = 2 x exp(-x^2) / (sqrt(pi) erfc), so erfc * 20u x p'/p = 1.41u x exp(-x^2)
    <= 0.6u (x exp(-x^2) <= 0.43).  1 - erfc rounds once more (u).  So |erf error| <= 3e-7 + 49u erfc(x) + 1.6u; it enters gelu
    with 0.5 |u|, and the fma and the last product round once each, 2u |gelu|:
        0.5 |u| (3e-7 + 49u erfc(|u| / sqrt 2) + 1.6u) + 2u |gelu(u)|."""
    g = gate.to(F64)
    return 0.5 * g.abs() * (AS_ERF_ABS + U * (49.0 * torch.special.erfc(g.abs() * math.sqrt(0.5)) + 1.6)) + 2.0 * U * ref_gelu_erf(g).abs()


# ------------------------------------------------------------------------------------------
# fp32 emulations
# ------------------------------------------------------------------------------------------
def _t(c):
    return torch.tensor(c, dtype=F32)


def fma(a, b, c):
    """fmaf on fp32 tensors: the product is exact in float64 (48 bits) and the sum is rounded once more to fp32."""
    return (a.to(F64) * b.to(F64) + c.to(F64)).to(F32)


def _expf(t):
    """__expf: v_exp_f32(t * log2e)."""
    return torch.exp2(t * _t(R.LOG2E_F32))


def emu_silu(v):
    """common.h: silu_f = v * rcp(1 + __expf(-v))."""
    v = v.to(F32)
    return v * (1.0 / (1.0 + _expf(-v)))


def emu_quick_gelu(v):
    v = v.to(F32)
    return v / (1.0 + _expf(_t(-QG_F32) * v))


def emu_gelu_erf(v, clamp=True):
    """common.h: gelu_erf_f — fmed3 clamp at +-9, two fmas in t = vc^2, exp2(p * vc), v * rcp(1 + e)."""
    v = v.to(F32)
    vc = v.clamp(-9.0, 9.0) if clamp else v
    t = vc * vc
    p = fma(t, _t(GELU_FIT[0]), _t(GELU_FIT[1]))
    p = fma(t, p, _t(GELU_FIT[2]))
    e = torch.exp2(p * vc)
    return v * (1.0 / (1.0 + e))


def emu_gelu_tanh(v):
    v = v.to(F32)
    return 0.5 * v * (1.0 + torch.tanh(_t(0.7978845608028654) * (v + _t(0.044715) * v * v * v)))


def emu_gelu_pipe(u):
    """ff320.hip: GeluPipe stages 1-14 for one gate: returns gelu(u) = 0.5 * (u + |u| erf(|u| / sqrt 2))."""
    u = u.to(F32)
    ax = u.abs()
    x = ax * _t(SQRT_HALF_F32)
    p = fma(x, _t(AS_7_1_28[0]), _t(AS_7_1_28[1]))
    for c in AS_7_1_28[2:]:
        p = fma(x, p, _t(c))
    p = fma(x, p, _t(1.0))
    for _ in range(4):
        p = p * p
    p = 1.0 - 1.0 / p
    return 0.5 * fma(ax, p, u)


def emu_geglu_pipe(value, gate):
    """ff320.hip stages 0 and 15: (0.5 v) * (u + |u| erf), rounded to bf16 as the GEMM2 operand."""
    return store((0.5 * value.to(F32)) * (2.0 * emu_gelu_pipe(gate)))


def emu_geglu(acc_v, acc_g, b_v, b_g, gelu="fit", swap=False, gate_bias_from_value=False, how="rne"):
    """gemm_epilogue.h: f2bf((x + bx) * gelu_erf_f(g + bg)).  acc_*: the fp32 sums, b_*: the biases.  Defects: another GELU
    (`quick`, `tanh`, `noclamp`), value and gate exchanged, the gate's bias read from the value's slot, a defective store."""
    x = acc_v.to(F32) + b_v.to(F32)
    g = acc_g.to(F32) + (b_v if gate_bias_from_value else b_g).to(F32)
    if swap:
        x, g = g, x
    f = {"fit": emu_gelu_erf, "noclamp": lambda v: emu_gelu_erf(v, clamp=False), "quick": emu_quick_gelu, "tanh": emu_gelu_tanh}[gelu]
    return store(x * f(g), how)


def emu_epilogue(p, act, res=(), out_f32=False, how="rne", act_after_res=False, exchange=False, skip_hi4=False, skip_tail=False):
    """gemm_epilogue.h's plain arm on the exact pre-activation p (M, N): activation, residuals, store.  Defects: the activation
    after the residuals, SiLU and quick-GELU exchanged, no activation on channels 4-7 of every group of 8, none on the 4-channel
    tail arm (N % 8 == 4), a defective store."""
    v = p.to(F32)
    if exchange:
        act = {ACT_SILU: ACT_QUICK_GELU, ACT_QUICK_GELU: ACT_SILU}[act]
    f = {ACT_NONE: lambda t: t, ACT_SILU: emu_silu, ACT_QUICK_GELU: emu_quick_gelu}[act]
    rs = [r.to(F32) for r in res]
    if act_after_res:
        for r in rs:
            v = v + r
        v = f(v)
    else:
        a = f(v)
        ch = torch.arange(v.shape[-1])
        if skip_hi4:
            a = torch.where((ch % 8 >= 4), v, a)
        if skip_tail and v.shape[-1] % 8 == 4:
            a = torch.where(ch >= v.shape[-1] - 4, v, a)
        v = a
        for r in rs:
            v = v + r
    return v if out_f32 else store(v, how)


def emu_lnf(acc, b, colsum, mean, rstd, drop_colsum=False, rstd_on_bias=False):
    """gemm8p.hip's LayerNorm fold in fp32: the accumulators start at b / rstd - mean * colsum, the K loop adds W' x, the epilogue
    multiplies by rstd.  Returns the fp32 value that is stored (plain) or split into value | gate (GEGLU)."""
    acc, b, cs = acc.to(F32), b.to(F32), colsum.to(F32)
    mean, rstd = mean.to(F32)[:, None], rstd.to(F32)[:, None]
    start = (b[None, :] if rstd_on_bias else b[None, :] * (1.0 / rstd)) - (0.0 if drop_colsum else mean * cs[None, :])
    return (start + acc) * rstd


# ------------------------------------------------------------------------------------------
# operands on the dyadic grid
# ------------------------------------------------------------------------------------------
def _sixteenths(shape, lim, g):
    return E.ints(shape, -16 * lim, 16 * lim, g) / 16.0


def _bf16_exact(t, what):
    assert bool((t.to(BF).to(F64) == t).all()), f"{what} is not made of bf16 numbers"


def dyadic(xshape, wshape, fwd, seed=0, shift=6, xmax=8, rows_per_bias=0, frames_per_bias=0, nres=2, bmax=8, rmax=16, sat=False,
           bias=None):
    """E.operands on the grid: x integers in [-xmax, xmax], w = E.sparse_weight * 2^-shift, bias / row bias (|.| <= bmax) and
    residuals (|.| <= rmax) multiples of 2^-4.  Returns x, w, b, gb, res, acc = fwd(x, w) (what the K loop sums), p = the
    pre-activation acc + b + row bias, and asserts the grid premise through E.check_inputs on the problem scaled by 2^G.
    sat: channels [8, 16) are biased to -96 and [16, 24) to +96 (fewer than 24 channels: the last two blocks of 4)."""
    g = E.gen(seed)
    x = E.ints(xshape, -xmax, xmax, g)
    w = E.sparse_weight(wshape, g) * 2.0 ** -shift
    n = wshape[0]
    b = _sixteenths((n,), bmax, g) if bias is None else bias.clone()
    if sat:
        lo = (8, 16, 24) if n >= 24 else (n - 8, n - 4, n)
        b[lo[0]:lo[1]], b[lo[1]:lo[2]] = -SAT, SAT
    acc = fwd(x, w, None)
    p = fwd(x, w, b)
    gb = None
    if rows_per_bias:
        gb = _sixteenths(((p.shape[0] + rows_per_bias - 1) // rows_per_bias, n), bmax, g)
        p = p + gb.repeat_interleave(rows_per_bias, 0)[: p.shape[0]]
    if frames_per_bias:
        gb = _sixteenths((p.shape[0] // frames_per_bias, n), bmax, g)
        p = p + gb.repeat_interleave(frames_per_bias, 0)[:, :, None, None]
    res = [_sixteenths(p.shape, rmax, g) for _ in range(nres)]
    total = p
    for r in res:
        _bf16_exact(r, "a residual")
        total = total + r
    _bf16_exact(x, "x")
    _bf16_exact(w, "w")
    grid = 2.0 ** max(shift, 4)
    E.check_inputs(x, w * grid, total * grid, (2 * max(bmax, SAT if sat else 0) + nres * rmax) * grid, E.F32_EXACT)
    E.check_inputs(x, w * grid, p * grid, 0, E.F32_EXACT)
    return SimpleNamespace(x=x, w=w, b=b, gb=gb, res=res, r1=res[0] if nres > 0 else None, r2=res[1] if nres > 1 else None, acc=acc,
                           p=p, total=total)


def gate_census(gate):
    """Count of gates in each range of GATE_RANGES."""
    out = []
    for lo, hi, kind in GATE_RANGES:
        out.append(int(((gate >= lo if kind[0] == "[" else gate > lo) & (gate <= hi if kind[1] == "]" else gate < hi)).sum()))
    return out


def assert_gate_coverage(gate, what=""):
    counts = gate_census(gate)
    assert min(counts) >= MIN_PER_GATE_RANGE, f"{what}: gates per range {counts}, fewer than {MIN_PER_GATE_RANGE} in one"
    return counts


def assert_saturation(p, what=""):
    """SiLU / quick-GELU inputs: pre-activations below -88 (exp(-v) beyond fp32) and above +88 (sigmoid = 1) both occur."""
    lo, hi = int((p < -88.0).sum()), int((p > 88.0).sum())
    assert lo >= 64 and hi >= 64, f"{what}: {lo} pre-activations below -88, {hi} above +88"
    return lo, hi


def geglu_bias(inner, g):
    """[value | gate] biases, multiples of 2^-4: values in [-6, 6], gates spread evenly over [-11.5, 11.5] in shuffled order."""
    bv = _sixteenths((inner,), 6, g)
    steps = torch.round(torch.linspace(-11.5, 11.5, inner, dtype=F64) * 16.0) / 16.0
    return torch.cat([bv, steps[torch.randperm(inner, generator=g)]])


@functools.lru_cache(maxsize=None)
def geglu_case(m, inner, k, seed=0):
    """A GEGLU projection (m, 2 inner) <- k in the reference layout [value rows | gate rows]: gates on the grid k / 16."""
    g = E.gen(1000 + seed)
    o = dyadic((m, k), (2 * inner, k), F.linear, seed=seed, shift=4, xmax=4, nres=0, bias=geglu_bias(inner, g))
    o.value, o.gate = o.p[:, :inner], o.p[:, inner:]
    o.counts = assert_gate_coverage(o.gate, f"GEGLU {m}x{inner}<-{k}")
    o.ref = ref_geglu(o.value, o.gate)
    o.bound = bound(o.ref, budget_geglu(o.value))
    return o


@functools.lru_cache(maxsize=None)
def linear_case(m, n, k, rows, full, seed=0, sat=True):
    """A Linear (m, n) <- k: plain (bias only), or `full`: bias + row bias per `rows` rows + two residuals."""
    o = dyadic((m, k), (n, k), F.linear, seed=seed, rows_per_bias=rows if full else 0, nres=2 if full else 0, sat=sat)
    if sat:
        assert_saturation(o.p, f"Linear {m}x{n}<-{k}")
    return o


CONV_FWD = {"s1": lambda x, wt, b: F.conv2d(x, wt, b, padding=1),
            "up": lambda x, wt, b: F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), wt, b, padding=1)}


@functools.lru_cache(maxsize=None)
def conv_case(kind, n, cin, cout, h, w, nres=2, seed=0, sat=True):
    """Conv2d 3x3 on n frames of h x w (kind `s1`, or `up`: the fused nearest-2x source), per-frame row bias, residuals."""
    o = dyadic((n, cin, h, w), (cout, cin, 3, 3), CONV_FWD[kind], seed=seed, frames_per_bias=1, nres=nres, sat=sat)
    if sat:
        assert_saturation(o.p, f"conv {kind} {cin}->{cout}")
    return o


@functools.lru_cache(maxsize=None)
def lnf_case(m, n, k, geglu, seed=0):
    """Linear(LayerNorm(x)) with the statistics made by the caller: mean an integer in [-3, 3], rstd in {1/4, 1/2, 1, 2}, both
    varying per row; gamma = 1, beta = 0, so the folded weight is w itself.  The epilogue's rstd * (acc - mean * colsum) + b is
    exact: 1 / rstd is a power of two, b / rstd a multiple of 2^-6, mean * colsum a multiple of 2^-4."""
    g = E.gen(2000 + seed)
    inner = n // 2
    o = dyadic((m, k), (n, k), F.linear, seed=seed, shift=4, xmax=4, nres=0, bias=geglu_bias(inner, g) if geglu else None)
    o.mean = E.ints((m,), -3, 3, g)
    o.rstd = 2.0 ** E.ints((m,), -2, 1, g)
    o.colsum = o.w.sum(dim=1)
    o.p = o.rstd[:, None] * (o.acc - o.mean[:, None] * o.colsum[None, :]) + o.b[None, :]
    scale = 2.0 ** 6
    assert bool(((o.p * scale) == (o.p * scale).round()).all()) and (o.p.abs().max() * scale + 4 * 8 * scale) < E.F32_EXACT
    assert len(set(o.mean.tolist())) == 7 and len(set(o.rstd.tolist())) == 4
    if geglu:
        o.value, o.gate = o.p[:, :inner], o.p[:, inner:]
        o.counts = assert_gate_coverage(o.gate, "LayerNorm-folded GEGLU")
        o.ref = ref_geglu(o.value, o.gate)
        o.bound = bound(o.ref, budget_geglu(o.value))
    return o


# ------------------------------------------------------------------------------------------
# comparison
# ------------------------------------------------------------------------------------------
def worst(got, ref, bnd):
    """(largest |got - ref| / bound, its index) — what every GPU case prints."""
    g, r, b = got.to(F64).reshape(-1), ref.to(F64).reshape(-1), bnd.to(F64).reshape(-1)
    err = (g - r).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / b)
    ratio = torch.where(torch.isfinite(g), ratio, torch.full_like(ratio, math.inf))
    i = int(ratio.argmax())
    return float(ratio[i]), tuple(int(v) for v in np.unravel_index(i, tuple(ref.shape)))


def outside(got, ref, bnd):
    """Number of elements outside their bound."""
    g, r, b = got.to(F64).reshape(-1), ref.to(F64).reshape(-1), bnd.to(F64).reshape(-1)
    return int(((~torch.isfinite(g)) | ((g - r).abs() > b)).sum())


def assert_within(got, ref, bnd, what):
    ratio, at = worst(got, ref, bnd)
    print(f"{what}: max |err| / bound {ratio:.4f} at {at}")
    R.assert_within(got, ref, bnd, what)
    return ratio


def assert_rounded(got, total, what):
    """got (bf16) against bf16_rne of the exact float64 result, bit for bit; prints the tie census."""
    t, even, odd = tie_census(total)
    print(f"{what}: {t} exact ties ({even} kept bit even, {odd} odd) of {total.numel()}")
    R.assert_bits_equal(got.cpu().contiguous(), bf16_rne(total).reshape(got.shape), what)
    return t


# ------------------------------------------------------------------------------------------
# the cases shared by tests/test_epilogue_ref.py (CPU) and tests/test_epilogue_gpu.py
# ------------------------------------------------------------------------------------------
LIN_M, LIN_K, LIN_ROWS = 300, 40, 50              # ragged M against every block shape; K = 40 -> Kpad 64: a K tail
LIN_N = (320, 324)                                # 324: the 4-channel tail arm (N % 8 == 4)
ACTS = {"none": ACT_NONE, "silu": ACT_SILU, "quick_gelu": ACT_QUICK_GELU}
TAP_GEGLU = {656: (300, 328, 40), 640: (300, 320, 40)}          # packed N -> (m, inner, k): 328 is ragged against 64 / 128 / 256
G8_GEGLU = ((300, 256, 192), (300, 328, 192))
LIN320_GEGLU = tuple((m, inner, 320) for m in (32, 130) for inner in (160, 1280))
LNF_SHAPE = (300, 512, 256)


def all_geglu_cases():
    return tuple(TAP_GEGLU.values()) + G8_GEGLU + LIN320_GEGLU


# ------------------------------------------------------------------------------------------
# ff320 (ln = False): x + W2 . bf16(v * gelu(u)) + b2 with (v | u) = W1 . x + b1
# ------------------------------------------------------------------------------------------
FF_M = (48, 200)                    # ff320.hip: a round is 4 waves x 32 tokens = 128: one partly filled round; one whole + one ragged
FF_DIM, FF_INNER, FF_W2_NNZ = 320, 1280, 8


def bound_hidden(value, gate):
    """(h, bh): the hidden value v * gelu(u) in float64 and the bound on the bf16 number GEMM2 multiplies, |h_kernel - h| <= bh."""
    h = ref_geglu(value, gate)
    return h, bound(h, value.to(F64).abs() * budget_gelu_pipe(gate))


def budget_ff_sum(terms_abs, nterms):
    """fp32 accumulation of the second GEMM: out = b2 + x + sum_k w2_jk h_k, `nterms` non-zero terms per output (the zero products
    of the matrix pipe add nothing).  In any order, nterms - 1 additions round, each by at most one ulp = 2u of its result (the
    matrix pipe's internal additions are not documented to round to nearest; a VALU addition would be u), and every partial result
    is bounded by the sum of the terms' magnitudes: 2 (nterms - 1) u sum |t|.  The products themselves are exact (w2 = +-1)."""
    return 2.0 * (nterms - 1) * U * terms_abs


@functools.lru_cache(maxsize=None)
def ff320_case(m, seed=0):
    """x integers in [-2, 2]; W1 (2560, 320) dyadic-sparse with gates on the grid k / 16 over [-12, 12]; W2 (320, 1280) in {-1, 0, 1}
    with at most 8 non-zeros per row and one in every column (every hidden unit is observed); b2 multiples of 2^-4."""
    g = E.gen(3000 + seed + m)
    o = dyadic((m, FF_DIM), (2 * FF_INNER, FF_DIM), F.linear, seed=seed + m, shift=4, xmax=2, nres=0, bias=geglu_bias(FF_INNER, g))
    o.value, o.gate = o.p[:, :FF_INNER], o.p[:, FF_INNER:]
    o.counts = assert_gate_coverage(o.gate, f"ff320 M={m}")
    w2 = torch.zeros(FF_DIM, FF_INNER, dtype=F64)
    rows = torch.arange(FF_DIM)[:, None]
    for _ in range(FF_W2_NNZ // 4):
        cols = torch.randperm(FF_INNER, generator=g).reshape(FF_DIM, 4)
        w2[rows, cols] = (torch.randint(0, 2, (FF_DIM, 4), generator=g) * 2 - 1).double()
    assert bool((w2 != 0).any(dim=0).all()) and int((w2 != 0).sum(dim=1).max()) <= FF_W2_NNZ
    o.w2, o.b2 = w2, _sixteenths((FF_DIM,), 8, g)
    h, bh = bound_hidden(o.value, o.gate)
    o.h, o.bh = h, bh
    o.ref = o.x + o.b2[None, :] + h @ w2.t()
    mag = o.x.abs() + o.b2.abs()[None, :] + (h.abs() + bh) @ w2.abs().t()
    o.bound = bound(o.ref, bh @ w2.abs().t() + budget_ff_sum(mag, FF_W2_NNZ + 2))
    return o


def emu_ff320(o, gelu="pipe"):
    """The kernel's steps: the hidden value through GeluPipe (or a defective GELU) rounded to bf16, GEMM2 as an fp32 chain in k
    order that starts from b2 + x, the bf16 store."""
    f = {"pipe": emu_gelu_pipe, "fit": emu_gelu_erf, "tanh": emu_gelu_tanh, "quick": emu_quick_gelu}[gelu]
    h = store((0.5 * o.value.to(F32)) * (2.0 * f(o.gate))).to(F32)
    acc = o.b2.to(F32)[None, :] + o.x.to(F32)
    nz = (o.w2 != 0).nonzero()
    for j in range(FF_DIM):
        for k in nz[nz[:, 0] == j, 1].tolist():
            acc[:, j] = acc[:, j] + o.w2[j, k].to(F32) * h[:, k]
    return store(acc)


# ------------------------------------------------------------------------------------------
# LayerNorm computed INSIDE a kernel (ff320.hip `ln`, its block tail, lin320.hip `ln_eps`): rows on which it is exact
#
# z holds 80 / 80 entries +-1, 60 / 60 of +-2 and 20 / 20 of +-4: sum 0, sum of squares 1280.  A row x = s z + m over the 320 channels,
# s a power of two and m an integer, has mean m and variance 4 s^2; its normalised value is z / 2 in {+-1/2, +-1, +-2}.  Every fp32
# sum over such a row is exact in any order, the kernels' mean is m and their variance 4 s^2 bit for bit, and rsqrtf(4 s^2 + eps) is
# (1 - eps / (8 s^2)) / (2 s) give or take its last bits: the fp32 normalised value lies within 3e-5 (relative) of z / 2, a bf16
# number whose neighbours are 2e-3 away, so the bf16 operand of the MFMA is z / 2 EXACTLY whatever the hardware's rsqrtf returns in
# its last bits.  tests/test_epilogue_ref.py shows that with the emulations below for every row the GPU tests use, with rsqrtf moved
# by up to +-4 ulp.  `zeros` (lin320 only, which forms (x - mean) * rstd): 68 / 59 / 21 pairs and 24 zeros, same sum of squares.
# ------------------------------------------------------------------------------------------
LN_EPS = 1e-5                       # the product's epsilon
LN_SCALES = (0.25, 0.5, 1.0, 2.0, 4.0)
LN_BIG_MEAN = 96.0                  # a few rows have |mean| = 96 at s = 1/2: mean = 96 standard deviations, still 8 significant bits
LN_RSQRT_ULPS = 4                   # premise (nobody has measured this chip's rsqrtf): within 4 ulp of the correctly rounded value
INV320_F32 = float(np.float32(1.0) / np.float32(320.0))          # the kernels' literal 1.0f / 320
FF_CUS = 256                        # compute units of an MI355X; the GPU tests read the device's own count


def ff_rounds_m(cus=FF_CUS):
    """ff320's grid is min(rounds, CUs) workgroups of 128 tokens: the smallest M at which a workgroup runs a second round and the last
    round is ragged."""
    return 128 * cus + 200


def _ln_base(zeros):
    vals = []
    for v, c in (((1, 68), (2, 59), (4, 21)) if zeros else ((1, 80), (2, 60), (4, 20))):
        vals += [v] * c + [-v] * c
    z = torch.tensor(vals + [0] * (FF_DIM - len(vals)), dtype=F64)
    assert z.numel() == FF_DIM and z.sum().item() == 0 and (z * z).sum().item() == 4 * FF_DIM and int((z == 0).sum()) == (24 if zeros else 0)
    return z


@functools.lru_cache(maxsize=None)
def ln_rows(m, seed, zeros=False):
    """m rows x = s z + mean: z (its own permutation of the base vector per row), perm, s in {1/4 .. 4}, mean an integer in [-3, 3] —
    rows 5, m // 2 and m - 2 have mean +-96 at s = 1/2 — and the bf16-exact x.  s differs between adjacent rows, so their (s, mean)
    pairs do: statistics taken from a neighbouring token are seen."""
    g = E.gen(7000 + seed + (500 if zeros else 0))
    perm = torch.argsort(torch.rand(m, FF_DIM, generator=g), dim=1)
    z = _ln_base(zeros)[perm]
    si = torch.cumsum(torch.randint(1, len(LN_SCALES), (m,), generator=g), 0) % len(LN_SCALES)      # a step of 1 .. 4 (mod 5): never 0
    s = torch.tensor(LN_SCALES, dtype=F64)[si]
    mean = E.ints((m,), -3, 3, g)
    big = sorted({5, m // 2, m - 2}) if m >= 16 else []
    for i, r in enumerate(big):
        s[r], mean[r] = 0.5, LN_BIG_MEAN * (1 - 2 * (i & 1))
        for nb in (r - 1, r + 1):           # the neighbours keep another scale
            if 0 <= nb < m and nb not in big and s[nb] == 0.5:
                s[nb] = 2.0
    x = s[:, None] * z + mean[:, None]
    _bf16_exact(x, "a LayerNorm row")
    pair = torch.stack([s, mean], dim=1)
    assert m < 2 or bool((pair[1:] != pair[:-1]).any(dim=1).all()), "adjacent rows share (s, mean)"
    assert bool((x.sum(dim=1) == FF_DIM * mean).all()) and bool((((x - mean[:, None]) ** 2).sum(dim=1) == 4 * FF_DIM * s * s).all())
    return SimpleNamespace(z=z, perm=perm, s=s, mean=mean, x=x, big=big, zn=z / 2.0)


def _rsqrt_f32(v32, ulps=0):
    """rsqrtf: the correctly rounded value moved by `ulps` units in the last place."""
    r = (1.0 / torch.sqrt(v32.to(F64))).to(F32)
    return (r.view(torch.int32) + ulps).view(F32) if ulps else r


def _shift_rows(t, k):
    """Row r takes the value of row r + k (the ends repeat)."""
    return t[(torch.arange(t.shape[0]) + k).clamp(0, t.shape[0] - 1)]


def emu_ln_ff320(x, eps=LN_EPS, ulps=0, contract=False, stats_row=0, half_only=False, one_pass=False, no_mean=False):
    """ff320.hip, "LayerNorm statistics": lane half hi of a token holds channels 16 s + 8 hi .. + 7 of the 20 k-steps; it sums its 160
    values in that order, the halves meet through __shfl_xor(., 32), mu = sm * (1.0f / 320); the second pass sums fmaf(dv, dv, sq) the
    same way; rs = rsqrtf(sq * (1.0f / 320) + eps), rm = rs * mu, operand = f2bf(fmaf(rs, x, -rm)).  `contract`: the compiler fuses
    sq * (1/320) + eps into one fma.  Returns the bf16 operand in channel order.  Defects: statistics of row r + stats_row; the shuffle
    missing (each half normalises with its own 160 channels' sums); one-pass variance E[x^2] - mu^2; rs applied without the mean."""
    x32 = x.to(F32)
    m = x32.shape[0]
    xh = x32.view(m, 20, 2, 8).permute(0, 2, 1, 3).reshape(m, 2, 160)            # [token][hi][8 s + e]
    inv, e32 = _t(INV320_F32), _t(float(np.float32(eps)))

    def lane_sum(term):
        acc = torch.zeros(m, 2, dtype=F32)
        for i in range(160):
            acc = term(acc, i)
        return acc if half_only else acc + acc.flip(1)

    mu = lane_sum(lambda a, i: a + xh[:, :, i]) * inv
    if one_pass:
        sq = lane_sum(lambda a, i: fma(xh[:, :, i], xh[:, :, i], a))
        var = sq * inv - mu * mu
    else:
        sq = lane_sum(lambda a, i: fma(xh[:, :, i] - mu, xh[:, :, i] - mu, a))
        var = None
    v = (var + e32) if one_pass else (fma(sq, inv, e32) if contract else sq * inv + e32)
    rs = _rsqrt_f32(v, ulps)
    if stats_row:
        mu, rs = _shift_rows(mu, stats_row), _shift_rows(rs, stats_row)
    rm = torch.zeros_like(mu) if no_mean else rs * mu
    out = store(fma(rs[:, :, None], xh, -rm[:, :, None]))
    return out.view(m, 2, 20, 8).permute(0, 2, 1, 3).reshape(m, FF_DIM)


def emu_ln_lin320(x, eps=LN_EPS, ulps=0, contract=False, stats_row=0, one_pass=False, no_mean=False, skip_g32=False):
    """lin320.hip (both kernels), rows normalised in LDS: thread sub of the 16 of a row holds granules sub, sub + 16, sub + 32 (< 40) of
    8 channels; it sums them in that order, four __shfl_xor steps make the row's total, mean = sm * (1.0f / 320); q += dv * dv (or the
    fma the compiler contracts it to) the same way, rstd = rsqrtf(q * (1.0f / 320) + eps), operand = f2bf((x - mean) * rstd).
    Defects: statistics of row r + stats_row, one-pass variance, no mean, granules sub + 32 left out of the sums."""
    x32 = x.to(F32)
    m = x32.shape[0]
    xg = torch.zeros(m, 48, 8, dtype=F32)
    xg[:, :40] = x32.view(m, 40, 8)
    xt = xg.view(m, 3, 16, 8).permute(0, 2, 1, 3).reshape(m, 16, 24)            # [row][sub][8 k + e]
    valid = (torch.arange(3)[None, :, None] * 16 + torch.arange(16)[:, None, None] < (32 if skip_g32 else 40)).expand(16, 3, 8).reshape(16, 24)
    inv, e32 = _t(INV320_F32), _t(float(np.float32(eps)))
    lanes = torch.arange(16)

    def row_sum(term):
        acc = torch.zeros(m, 16, dtype=F32)
        for i in range(24):
            acc = torch.where(valid[None, :, i], term(acc, i), acc)
        for step in (1, 2, 4, 8):
            acc = acc + acc[:, lanes ^ step]
        return acc

    mean = row_sum(lambda a, i: a + xt[:, :, i]) * inv                            # (m, 16): the same value in all 16 threads
    sq = (lambda a, d: fma(d, d, a)) if contract else (lambda a, d: a + d * d)
    if one_pass:
        var = row_sum(lambda a, i: sq(a, xt[:, :, i])) * inv - mean * mean
        v = var + e32
    else:
        q = row_sum(lambda a, i: sq(a, xt[:, :, i] - mean))
        v = fma(q, inv, e32) if contract else q * inv + e32
    rstd = _rsqrt_f32(v, ulps)
    if stats_row:
        mean, rstd = _shift_rows(mean, stats_row), _shift_rows(rstd, stats_row)
    if no_mean:
        mean = torch.zeros_like(mean)
    out = store((xt - mean[:, :, None]) * rstd[:, :, None])                      # (m, 16, 24)
    return out.view(m, 16, 3, 8).permute(0, 2, 1, 3).reshape(m, 48, 8)[:, :40].reshape(m, FF_DIM)


LN_DEFECTS_FF = (("statistics of row r + 1", dict(stats_row=1)), ("statistics of row r - 1", dict(stats_row=-1)),
                 ("the lane's own 160 channels only", dict(half_only=True)), ("rs applied without the mean", dict(no_mean=True)),
                 ("eps taken as 1e-2", dict(eps=1e-2)))
LN_DEFECTS_LIN = (("statistics of row r + 1", dict(stats_row=1)), ("statistics of row r - 1", dict(stats_row=-1)),
                  ("rstd applied without the mean", dict(no_mean=True)), ("eps taken as 1e-2", dict(eps=1e-2)),
                  ("granules sub + 32 left out", dict(skip_g32=True)))


def ln_affine(g):
    """gamma per channel in {1/2, 1, 2}, beta multiples of 1/4 in [-1, 1]: both non-trivial."""
    gamma = 2.0 ** E.ints((FF_DIM,), -1, 1, g)
    beta = E.ints((FF_DIM,), -4, 4, g) / 4.0
    assert len(set(gamma.tolist())) == 3 and len(set(beta.tolist())) >= 5
    return gamma, beta


# ------------------------------------------------------------------------------------------
# ff320 with ln = True: out = x + b2 + W2 . bf16(v gelu(u)), (v | u) = W1 (gamma * LN(x) + beta) + b1 = (W1 diag(gamma)) (z / 2) + (b1 + W1 beta)
# ------------------------------------------------------------------------------------------
FF_KEEP = 256                       # cases of at most this many rows keep value / gate / h / bh for the CPU emulations


@functools.lru_cache(maxsize=None)
def ff320_ln_weights(seed=0):
    """W1 (2560, 320) = sparse +-1 * 2^-4, gamma, beta, b1 = geglu_bias, W2 / b2 as ff320_case.  g1 = W1 diag(gamma) and b1p = b1 + W1 beta
    are what pack_ff320 must form exactly; weff = g1 / 2 acts on the integers z (the grid is 2^-6: one bit finer than weights and biases
    alone need), so E.check_inputs holds on the problem scaled by 2^6."""
    g = E.gen(4000 + seed)
    w1 = E.sparse_weight((2 * FF_INNER, FF_DIM), g) * 2.0 ** -4
    gamma, beta = ln_affine(g)
    b1 = geglu_bias(FF_INNER, g)
    w2 = torch.zeros(FF_DIM, FF_INNER, dtype=F64)
    rows = torch.arange(FF_DIM)[:, None]
    for _ in range(FF_W2_NNZ // 4):
        cols = torch.randperm(FF_INNER, generator=g).reshape(FF_DIM, 4)
        w2[rows, cols] = (torch.randint(0, 2, (FF_DIM, 4), generator=g) * 2 - 1).double()
    assert bool((w2 != 0).any(dim=0).all()) and int((w2 != 0).sum(dim=1).max()) <= FF_W2_NNZ
    b2 = _sixteenths((FF_DIM,), 8, g)
    g1, b1p = w1 * gamma[None, :], b1 + w1 @ beta
    _bf16_exact(g1, "W1 diag(gamma)")
    assert bool((b1p.float().double() == b1p).all())
    o = SimpleNamespace(w1=w1, gamma=gamma, beta=beta, b1=b1, w2=w2, b2=b2, g1=g1, b1p=b1p, weff=g1 / 2.0)
    o.idx, o.val = sparse_rows(w2, FF_W2_NNZ)
    return o


def sparse_rows(w, nnz):
    """(idx, val), both (rows, nnz): the non-zero columns of every row in ascending order and their values, padded with (0, 0.0)."""
    assert int((w != 0).sum(dim=1).max()) <= nnz
    order = torch.argsort((w == 0).to(torch.int8), dim=1, stable=True)[:, :nnz]      # non-zeros first, each group in column order
    val = torch.gather(w, 1, order)
    return torch.where(val != 0, order, torch.zeros_like(order)), val


def sparse_apply(t, idx, val):
    """t (m, K) @ w.t() for w given by sparse_rows, in float64."""
    return (t[:, idx] * val[None]).sum(dim=-1)


@functools.lru_cache(maxsize=None)
def ff320_ln_case(m, seed=0):
    """The feed-forward on ln_rows(m): x the un-normalised rows (the residual), z / 2 the GEMM1 operand.  ref / bound as ff320_case —
    bound_hidden and budget_ff_sum unchanged, nothing added for the LayerNorm (its result is exact) — computed in row chunks.  hw, bhw,
    mhw: W2 h, |W2| bh and |W2| (|h| + bh), from which `with_residual` forms (ref, bound) for any exact residual rows."""
    wt, r = ff320_ln_weights(seed), ln_rows(m, seed)
    scale = 2.0 ** 6
    counts = [0] * len(GATE_RANGES)
    parts, keep = [], []
    for r0 in range(0, m, 2048):
        z = r.z[r0:r0 + 2048]
        p = (z.float() @ wt.weff.float().t()).double() + wt.b1p[None, :]         # exact in fp32: the grid premise, checked below
        if r0 == 0:
            E.check_inputs(z, wt.weff * scale, p * scale, wt.b1p.abs().max().item() * scale, E.F32_EXACT)
        value, gate = p[:, :FF_INNER], p[:, FF_INNER:]
        counts = [a + b for a, b in zip(counts, gate_census(gate))]
        h, bh = bound_hidden(value, gate)
        parts.append((sparse_apply(h, wt.idx, wt.val), sparse_apply(bh, wt.idx, wt.val.abs()), sparse_apply(h.abs() + bh, wt.idx, wt.val.abs())))
        if m <= FF_KEEP:
            keep.append((value, gate, h, bh))
    o = SimpleNamespace(x=r.x, z=r.z, rows=r, wt=wt, w2=wt.w2, b2=wt.b2, counts=counts, m=m)
    o.hw, o.bhw, o.mhw = (torch.cat([p[i] for p in parts]) for i in range(3))
    assert min(counts) >= MIN_PER_GATE_RANGE, f"ff320 ln M={m}: gates per range {counts}"
    if keep:
        o.value, o.gate, o.h, o.bh = (torch.cat([k[i] for k in keep]) for i in range(4))
    o.ref, o.bound = ff_with_residual(o, o.x)
    return o


def ff_with_residual(o, x):
    """(ref, bound) of x + b2 + W2 h for exact residual rows x: the hidden values' bounds through |W2|, the fp32 accumulation of the few
    non-zero terms, half an output ulp at the magnitude of the result."""
    ref = x + o.b2[None, :] + o.hw
    mag = x.abs() + o.b2.abs()[None, :] + o.mhw
    return ref, bound(ref, o.bhw + budget_ff_sum(mag, FF_W2_NNZ + 2))


def emu_ff_tokens(wt, tok, ln=None, operand=None, gelu="pipe", round_out=True):
    """The kernel's feed-forward on bf16 rows `tok` (fp32 / float64 tensor): LayerNorm (emu_ln_ff320 with the keywords `ln`; `operand`
    replaces its result), GEMM1 (exact on the grid; off it, the float64 sum rounded once), GeluPipe rounded to bf16, GEMM2 as an fp32
    chain over the non-zero terms in k order that starts from b2 + tok, the bf16 store (round_out = False: the fp32 accumulators)."""
    zn = (emu_ln_ff320(tok, **(ln or {})) if operand is None else operand).to(F64)
    p = (zn @ wt.g1.t() + wt.b1p[None, :]).to(F32)
    f = {"pipe": emu_gelu_pipe, "fit": emu_gelu_erf, "tanh": emu_gelu_tanh, "quick": emu_quick_gelu}[gelu]
    h = store((0.5 * p[:, :FF_INNER]) * (2.0 * f(p[:, FF_INNER:]))).to(F32)
    acc = wt.b2.to(F32)[None, :] + tok.to(F32)
    val = wt.val.to(F32)
    for k in range(wt.idx.shape[1]):
        acc = acc + val[None, :, k] * h[:, wt.idx[:, k]]
    return store(acc) if round_out else acc


# ------------------------------------------------------------------------------------------
# ff320 block tail: tok = W_o a + b_o + res;  t = tok + FF(LN(tok));  out = t  (to_out + FF)  or  W_p bf16(t) + b_p + x_in  (+ proj_out)
#
# Prologue: W_o = sparse +-{1, 1/2} with at most 8 non-zeros per row, a small integers, b_o multiples of 1/2 and the RESIDUAL chosen as
# the fix-up res = tok_target - b_o - W_o a, tok_target = ln_rows: every fp32 partial sum is a multiple of 1/4 below 2^9, the sum IS the
# target row, acc_to_frags rounds nothing, the LayerNorm gives z / 2 exactly and the plain case's (ref, bound) apply to t unchanged.
# Epilogue: the kernel rounds t to bf16 before it multiplies; with |t^ - t| <= delta (the plain bound, which already holds that half ulp)
#     |out - ref| <= |W_p| delta  +  budget_ff_sum(|b_p| + |x_in| + |W_p| (|t| + delta), nnz + 2)  +  1/2 ulp_out
# — the products W_p t^ are exact in fp32 (W_p = +-2^-s, t^ a bf16 number), the accumulation of the nnz + 2 terms rounds like GEMM2's.
# ------------------------------------------------------------------------------------------
TAIL_NNZ = 8


def tail_projection(g):
    """(320, 320) +-{1, 1/2}: eight times a random permutation matrix (<= 8 non-zeros per row, every column hit), and a non-zero in every
    (k-step of 16 input channels) x (tile of 32 output channels) block — all 4 chunks x 5 k-steps x 10 tiles of the prologue / epilogue."""
    w = torch.zeros(FF_DIM, FF_DIM, dtype=F64)
    rows = torch.arange(FF_DIM)
    for _ in range(TAIL_NNZ):
        w[rows, torch.randperm(FF_DIM, generator=g)] = (torch.randint(0, 2, (FF_DIM,), generator=g) * 2 - 1).double() * 2.0 ** -torch.randint(0, 2, (FF_DIM,), generator=g).double()
    nz = w != 0
    assert bool(nz.any(dim=0).all()) and int(nz.sum(dim=1).max()) <= TAIL_NNZ and int(nz.sum(dim=1).min()) >= 1
    assert bool(nz.view(10, 32, 20, 16).any(dim=3).any(dim=1).all()), "a (tile, k-step) block of the projection holds no weight"
    return w


@functools.lru_cache(maxsize=None)
def ff320_tail_weights(seed=0):
    g = E.gen(5000 + seed)
    o = SimpleNamespace(wo=tail_projection(g), wp=tail_projection(g), bo=E.ints((FF_DIM,), -16, 16, g) / 2.0, bp=_sixteenths((FF_DIM,), 8, g))
    o.oidx, o.oval = sparse_rows(o.wo, TAIL_NNZ)
    o.pidx, o.pval = sparse_rows(o.wp, TAIL_NNZ)
    return o


@functools.lru_cache(maxsize=None)
def ff320_tail_case(m, seed=0):
    """a, res, x_in for the tail around ff320_ln_case(m): .ref2 / .bound2 (to_out + FF) are the plain case's, .ref3 / .bound3 add proj_out."""
    ff, tw = ff320_ln_case(m, seed), ff320_tail_weights(seed)
    g = E.gen(5100 + seed + m)
    a = E.ints((m, FF_DIM), -2, 2, g)
    xin = _sixteenths((m, FF_DIM), 16, g)
    woa = sparse_apply(a, tw.oidx, tw.oval)
    res = ff.x - tw.bo[None, :] - woa
    _bf16_exact(res, "the fix-up residual")
    # below 128 at multiples of 1/2 (the rows with s = 1/4 carry quarters: those stay below 64)
    assert res.abs().max().item() < 128 and bool((res * 4 == (res * 4).round()).all()) and bool(((res * 2 == (res * 2).round()) | (res.abs() < 64)).all())
    assert torch.equal(woa + tw.bo[None, :] + res, ff.x)
    assert (a.abs() @ tw.wo.abs().t() + tw.bo.abs()[None, :] + res.abs()).max().item() * 4 < E.F32_EXACT      # partial sums: multiples of 1/4
    c = SimpleNamespace(ff=ff, tw=tw, a=a, res=res, xin=xin, m=m, ref2=ff.ref, bound2=ff.bound)
    t, dl = ff.ref, ff.bound
    c.ref3 = xin + tw.bp[None, :] + sparse_apply(t, tw.pidx, tw.pval)
    mag = xin.abs() + tw.bp.abs()[None, :] + sparse_apply(t.abs() + dl, tw.pidx, tw.pval.abs())
    c.bound3 = bound(c.ref3, sparse_apply(dl, tw.pidx, tw.pval.abs()) + budget_ff_sum(mag, TAIL_NNZ + 2))
    return c


def _chain(acc, src, idx, val):
    v = val.to(F32)
    for k in range(idx.shape[1]):
        acc = acc + v[None, :, k] * src[:, idx[:, k]]
    return acc


def emu_ff320_tail(c, epi, res_times=1, drop_bo=False, ln_before_res=False, chunk_shift=0, xin_row=0, round_t=True):
    """The block tail's steps in fp32: the prologue chain from b_o, the residual rows, acc_to_frags (bf16), emu_ff_tokens, and with `epi`
    the bf16 rounding of its result, the epilogue chain from b_p, the x_in rows, the store.  Defects: the residual added `res_times`
    times (0, 2), b_o dropped, the LayerNorm taken on the sum before the residual joined it, prologue chunk Q multiplied against the
    k-steps (80 channels of a) of chunk Q + chunk_shift, x_in of row r + xin_row, the feed-forward result not rounded before proj_out."""
    tw, m = c.tw, c.m
    a = c.a.to(F32)
    if chunk_shift:
        a = a.view(m, 4, 80)[:, (torch.arange(4) + chunk_shift) % 4].reshape(m, FF_DIM)
    acc = torch.zeros(m, FF_DIM, dtype=F32) if drop_bo else tw.bo.to(F32)[None, :].expand(m, FF_DIM)
    pre = _chain(acc, a, tw.oidx, tw.oval)
    acc = pre
    for _ in range(res_times):
        acc = acc + c.res.to(F32)
    tok = store(acc).to(F32)
    operand = emu_ln_ff320(store(pre).to(F32)) if ln_before_res else None
    t = emu_ff_tokens(c.ff.wt, tok, operand=operand, round_out=(not epi) or round_t)
    if not epi:
        return t
    acc = _chain(tw.bp.to(F32)[None, :].expand(m, FF_DIM), t.to(F32), tw.pidx, tw.pval)
    return store(acc + _shift_rows(c.xin, xin_row).to(F32))


TAIL_DEFECTS = (("res not added", dict(res_times=0)), ("res added twice", dict(res_times=2)), ("b_o dropped", dict(drop_bo=True)),
                ("LayerNorm before the residual", dict(ln_before_res=True)), ("prologue chunk Q on the k-steps of chunk Q + 1", dict(chunk_shift=1)),
                ("prologue chunk Q on the k-steps of chunk Q - 1", dict(chunk_shift=-1)))


# ------------------------------------------------------------------------------------------
# lin320 / lin320s with ln_eps: Linear(LayerNorm(x)) with the rows normalised in LDS
# ------------------------------------------------------------------------------------------
LIN320S_SLOTS = 7                   # lin320.hip: kBufsS
LIN_LN_SMALL = ((32, "lin320s_kernel"), (96, "lin320s_kernel"), (130, "lin320_kernel"))
LIN_LN_N = (320, 960)
LIN_LN_RAGGED_M = 32768 + 13
LIN_LN_WRAP_M = 32 * 256 * (LIN320S_SLOTS + 1)      # N = 320: 256 workgroups walk M / 32 tiles, M / 8192 each: one more than the ring has slots


@functools.lru_cache(maxsize=None)
def lin320_ln_weights(n, seed=0):
    """w (n, 320) = sparse +-1 * 2^-6, gamma / beta as ln_affine, b multiples of 2^-4; wf = w diag(gamma), bf = b + w beta: what
    fold_layernorm must form exactly."""
    g = E.gen(6000 + seed + n)
    w = E.sparse_weight((n, FF_DIM), g, rows_per_tile=16) * 2.0 ** -6
    gamma, beta = ln_affine(g)
    b = _sixteenths((n,), 8, g)
    wf, bf = w * gamma[None, :], b + w @ beta
    _bf16_exact(wf, "w diag(gamma)")
    assert bool((bf.float().double() == bf).all())
    return SimpleNamespace(w=w, b=b, gamma=gamma, beta=beta, wf=wf, bf=bf)


@functools.lru_cache(maxsize=None)
def lin320_ln_case(m, n, seed=0):
    """x = ln_rows(m, zeros allowed); total = wf (z / 2) + bf on the grid 2^-8: the kernel's fp32 sums are exact, the output is
    bf16_rne(total) bit for bit."""
    wt, r = lin320_ln_weights(n, seed), ln_rows(m, 100 + seed, zeros=True)
    total = (r.zn.float() @ wt.wf.float().t()).double() + wt.bf[None, :]
    scale = 2.0 ** 8
    E.check_inputs(r.z, wt.wf / 2.0 * scale, total[:4096] * scale, wt.bf.abs().max().item() * scale, E.F32_EXACT, rows_per_tile=16)
    return SimpleNamespace(x=r.x, rows=r, wt=wt, total=total, m=m, n=n)


# ------------------------------------------------------------------------------------------
# the ln_sums consumer (lin640s, g8): (mean, rstd) rebuilt in the kernel from the double sums s = K mean, q = K (var + mean^2)
#
# With var in {1/4, 1, 4, 16} the kernel's mean is exact and its (float)var too, but rstd = rsqrtf(var + eps) is not a power of two:
# rstd = r0 (1 + rho), r0 = var^-1/2, |rho| <= eps / (2 var) + 4 ulp (the premise on rsqrtf; an ulp taken as 2^-23 relative).  The
# kernels form  v = rstd * ((b * ir - mean * colsum) + sum_k w x),  ir = 1.0f / rstd.  Against ref = r0 (sum - mean colsum) + b:
#     rho r0 |sum - mean colsum|                                   rstd itself (b / rstd * rstd cancels)
#   + 3u |b|                                                       ir (2u: one ulp, whichever division the compiler emits) and b * ir (u)
#   + u (|b| + r0 |mean colsum|)                                   the subtraction (mean * colsum is exact: asserted)
#   + 2 (nnz + 1) u r0 (sum_k |w x| + |b| / r0 + |mean colsum|)    the matrix pipe adds exact products to an INEXACT start value: every
#                                                                  addition may round, by at most an ulp of a partial result (budget_ff_sum)
#   all times (1 + rho), + u |v| for the last product, + half an output ulp.
# ------------------------------------------------------------------------------------------
def ln_sums(o, k):
    """float64 [M, 2]: (K mean, K (var + mean^2)) with var = rstd^-2 — exact."""
    var = 1.0 / (o.rstd * o.rstd)
    return torch.stack([k * o.mean, k * (var + o.mean * o.mean)], dim=1).contiguous()


def ln_sums_rho(o, eps=LN_EPS):
    return eps * o.rstd * o.rstd / 2.0 + LN_RSQRT_ULPS * 2.0 ** -23


def bound_lnf_sums(o, eps=LN_EPS):
    """(ref, bound) of the plain LayerNorm-folded Linear of lnf_case when the statistics arrive as sums."""
    r0, rho = o.rstd[:, None], ln_sums_rho(o, eps)[:, None]
    mc = (o.mean[:, None] * o.colsum[None, :])
    assert bool((mc.float().double() == mc).all())
    b = o.b.abs()[None, :]
    nnz = ((o.w != 0).sum(dim=1) + 1).double()[None, :]
    sabs = o.x.abs() @ o.w.abs().t()
    a = rho * r0 * (o.acc - mc).abs() + (1.0 + rho) * (3.0 * U * b + U * (b + r0 * mc.abs()) + 2.0 * nnz * U * r0 * (sabs + b / r0 + mc.abs()))
    a = a + U * (o.p.abs() + a)
    return o.p, bound(o.p, a)


def emu_lnf_sums(o, k, side=0.0, eps=LN_EPS, mean_from_q=False, stats_row=0, **kw):
    """gemm8p.hip / lin640.hip with ln_sums: mean = (float)(s / K), rstd = rsqrtf((float)var + eps) taken at r0 (1 + side * rho): the
    exact value (side 0, the add of eps in fp32) or either end of the allowance; then emu_lnf and the store.  Defects: the mean read from
    q, the sums of row r + stats_row, and emu_lnf's."""
    sums = _shift_rows(ln_sums(o, k), stats_row)
    mean = (sums[:, 1] if mean_from_q else sums[:, 0]) / k
    var = (sums[:, 1] / k - (sums[:, 0] / k) ** 2).clamp_min(0.0).to(F32)
    rstd = _rsqrt_f32(var + _t(float(np.float32(eps)))).to(F64)
    if side:
        rstd = (var.to(F64) ** -0.5) * (1.0 + side * (eps / (2.0 * var.to(F64)) + LN_RSQRT_ULPS * 2.0 ** -23))
    return store(emu_lnf(o.acc, o.b, o.colsum, mean, rstd.to(F32), **kw))


LNF640 = {(16, 128): 1, (16, 640): 1, (304, 128): 0, (304, 640): 0}      # (M, N) -> seed at which lnf_case has all 7 means and 4 rstd values
