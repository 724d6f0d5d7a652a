"""The GEMM epilogues on a real MI355X against float64, element by element: activations and the direction of the bf16 store.

tests/test_exact_gpu.py holds every matrix kernel to an integer reference bit for bit, but only with act = 0 and on results that are
bf16 numbers already.  Here the operands sit on the dyadic grid of tests/_epilogue_ref.py (integer activations, weights
{-1, 0, 1} * 2^-s, biases and residuals multiples of 2^-4), so the fp32 value that reaches the epilogue is known exactly whatever
the tile shape, K order, split or lane map, and two kinds of assertion are left:

  * no activation: the output is bf16_rne(float64 result) bit for bit (fp32 out: the float64 result itself).  The results carry up
    to 12 significant bits; every case asserts a minimum of exact ties with both parities of the kept bit and prints the census;
  * SiLU, quick-GELU, GEGLU: |got - ref64| <= A + 1/2 ulp(|ref| + A) for EVERY element, A the activation's own budget
    (_epilogue_ref.budget_*).  Inputs cover gates in seven ranges over [-12, 12] (beyond +-9: the clamp of gelu_erf_f), and for
    SiLU / quick-GELU one channel block at -96 (exp overflows) and one at +96.

Every case asserts the kernel that ran, writes into a sentinel-filled wider buffer whose other columns must keep their sentinels,
and prints its largest |err| / bound and where it occurred.  tests/test_epilogue_ref.py shows on the CPU that the planted defects
(another GELU, a missing clamp, a truncating or ties-away store, the activation after the residual, ...) miss these bounds.

ff320 is held here with ln = False only.  Its `ln = True` path, both block-tail forms, lin320 / lin320s with ln_eps and the ln_stats /
ln_sums consumers normalise inside the kernel; on rows whose LayerNorm is exact in fp32 they are held per element as well, in
tests/test_fused_layernorm_gpu.py.
"""
import ctypes
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _elementwise_ref as R  # noqa: E402
import _exact_ints as E  # noqa: E402
import _epilogue_ref as P  # noqa: E402

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
TAP = {1: "tap_gemm_kernel 128ch x 128pix, 2 stages of K=64", 2: "tap_gemm_kernel 64ch x 256pix, 2 stages of K=64",
       3: "tap_gemm_kernel 128ch x 256pix, 3 stages of K=64", 4: "tap_gemm_kernel 256ch x 256pix, 4 stages of K=32",
       5: "tap_gemm_kernel 128ch x 512pix, 4 stages of K=32", 6: "tap_gemm_kernel 320ch x 128pix, 2 stages of K=32",
       7: "tap_gemm_kernel 256ch x 256pix, 4 stages of K=32"}
G8 = {12: "g8_kernel 256ch x 256pix", 13: "g8_kernel 128ch x 512pix"}
LEAD = 8                            # columns in front of an output slice: 16 bytes of bf16, the alignment of the kernels' stores


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _last():
    from ccedit_amd import hip
    return hip.lib().ccedit_last_kernel().decode()


@pytest.fixture
def mfma16():
    """set(v): the library's g8_mfma16 switch for the rest of the test; the value found is put back afterwards."""
    from ccedit_amd import hip
    lib = hip.lib()
    old = ctypes.c_int32(0)
    assert lib.ccedit_policy_get(b"g8_mfma16", ctypes.byref(old)) == 0

    def set_(v):
        assert lib.ccedit_policy_set(b"g8_mfma16", v) == 0
    try:
        yield set_
    finally:
        lib.ccedit_policy_set(b"g8_mfma16", old.value)


def _rows(t):
    return None if t is None else t.to(BF).cuda()


def _f32(t):
    return None if t is None else t.float().cuda()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().to(BF).cuda()


def _flat(t):
    return None if t is None else _nhwc(t).reshape(-1, t.shape[1])


def _rows64(t):      # float64 (N, C, H, W) -> float64 [N*H*W][C]
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _wide(rows, n, dtype=BF):
    """(whole buffer, its column slice [LEAD, LEAD + n)): sentinel-filled, a multiple of 8 wide, at least one guard column behind."""
    width = (n + LEAD + 1 + 7) // 8 * 8
    buf = R.sentinel_fill(rows * width, dtype, "cuda").view(rows, width)
    return buf, buf[:, LEAD:LEAD + n]


def _in_wide(t):
    """A bf16 operand as a column slice of a sentinel-filled wider buffer (row stride a multiple of 8)."""
    if t is None:
        return None
    buf, view = _wide(t.shape[0], t.shape[1])
    view.copy_(t.to(BF))
    return view


def _written(buf, n, what):
    """Exactly the slice was written: no sentinel left inside, every sentinel still there outside."""
    mask = torch.zeros(buf.shape, dtype=torch.bool)
    mask[:, LEAD:LEAD + n] = True
    R.assert_sentinels(buf, mask, what)


def _judge(got, o, act, out_f32, what):
    """got (M, N) on the device against case o: the rounding check (act 0) or the per-element bound."""
    got = got.cpu()
    if act == P.ACT_NONE:
        if out_f32:
            assert torch.equal(got.double(), o.total), f"{what}: fp32 output differs from the exact result"
            print(f"{what}: fp32 output exact")
        else:
            P.assert_ties(o.total, what)
            P.assert_rounded(got, o.total, what)
        return
    ref, bnd = P.bound_epilogue(o.p, act, o.res, out_f32)
    P.assert_within(got, ref, bnd, what)


# ------------------------------------------------------------------------------------------ tap_gemm, Linear
_TAP_LIN = [(t, n, a, full, f32) for n in P.LIN_N for t in range(1, 8) if t != 6 or n % 320 == 0 for a in P.ACTS for full in (False, True)
            for f32 in (False, True)]


@pytest.mark.parametrize("tile,n,act,full,out_f32", _TAP_LIN)
def test_tap_gemm_linear(tile, n, act, full, out_f32):
    """300 x N <- 40 (Kpad 64) in the seven block shapes: N = 320, and N = 324 whose last four channels take the `full == false`
    arm; none / SiLU / quick-GELU x {bias; bias + row bias per 50 rows + two residuals} x {bf16, fp32 out}; output and residuals are
    column slices of wider buffers."""
    _dev()
    from ccedit_amd import ops
    from ccedit_amd.packing import pack_weight
    o, a = P.linear_case(P.LIN_M, n, P.LIN_K, P.LIN_ROWS, full), P.ACTS[act]
    buf, out = _wide(P.LIN_M, n, F32 if out_f32 else BF)
    ops.linear(_rows(o.x), pack_weight(o.w, o.b).to("cuda"), act=a, group_bias=_f32(o.gb), group_rows=P.LIN_ROWS if full else 0,
               res1=_in_wide(o.r1), res2=_in_wide(o.r2), out=out, tile=tile)
    assert TAP[tile] in _last(), _last()
    what = f"tap_gemm tile {tile} N={n} {act} {'bias+rowbias+2res' if full else 'bias'} {'f32' if out_f32 else 'bf16'}"
    _written(buf, n, what)
    _judge(out, o, a, out_f32, what)


@pytest.mark.parametrize("tile,packed", [(t, 656) for t in (1, 2, 3, 4, 5, 7)] + [(6, 640)])
def test_tap_gemm_geglu(tile, packed):
    """GEGLU 300 x inner <- 40: packed N = 656 (inner 328: ragged against 64-, 128- and 256-channel tiles), 640 for the 320-channel shape."""
    _dev()
    from ccedit_amd import ops
    from ccedit_amd.packing import pack_weight
    m, inner, k = P.TAP_GEGLU[packed]
    o = P.geglu_case(m, inner, k)
    buf, out = _wide(m, inner)
    ops.linear(_rows(o.x), pack_weight(o.w, o.b, geglu=True).to("cuda"), out=out, tile=tile)
    assert TAP[tile] in _last(), _last()
    what = f"tap_gemm GEGLU tile {tile} packed N={packed}"
    _written(buf, inner, what)
    P.assert_within(out.cpu(), o.ref, o.bound, what)


# ------------------------------------------------------------------------------------------ tap_gemm, Conv2d
@pytest.mark.parametrize("tile", [1, 2, 3])
@pytest.mark.parametrize("kind", ["s1", "up"])
def test_tap_gemm_conv2d_silu(kind, tile):
    """The 3x3 gather's row map (two 9 x 7 frames; `up`: the fused nearest-2x source) under SiLU + per-frame row bias + two residuals."""
    _dev()
    from ccedit_amd import ops
    from ccedit_amd.packing import pack_weight
    o = P.conv_case(kind, 2, 64, 96, 9, 7)
    hw = o.p.shape[2] * o.p.shape[3]
    y = ops.conv2d(_nhwc(o.x), pack_weight(o.w, o.b).to("cuda"), act=P.ACT_SILU, group_bias=_f32(o.gb), group_rows=hw, res1=_flat(o.r1),
                   res2=_flat(o.r2), tile=tile, upsample=kind == "up")
    assert TAP[tile] in _last(), _last()
    ref, bnd = P.bound_epilogue(_rows64(o.p), P.ACT_SILU, [_rows64(r) for r in o.res])
    P.assert_within(y.reshape(-1, 96).cpu(), ref, bnd, f"tap_gemm conv {kind} SiLU tile {tile}")


# ------------------------------------------------------------------------------------------ conv_halo (tile 8)
@pytest.mark.parametrize("act", list(P.ACTS))
@pytest.mark.parametrize("cout,h,w", [(128, 16, 32), (320, 16, 20)])
def test_conv_halo(cout, h, w, act):
    """conv_halo_kernel 64 -> 128 at 16 x 32 and 64 -> 320 at 16 x 20 (the `narrow` last channel tile, a ragged last rectangle
    column), three frames, row bias + residual: the rounding case, SiLU and quick-GELU."""
    _dev()
    from ccedit_amd import ops
    from ccedit_amd.packing import pack_weight
    o, a = P.conv_case("s1", 3, 64, cout, h, w, nres=1), P.ACTS[act]
    y = ops.conv2d(_nhwc(o.x), pack_weight(o.w, o.b).to("cuda"), act=a, group_bias=_f32(o.gb), group_rows=h * w, res1=_flat(o.r1), tile=8)
    assert "conv_halo_kernel" in _last(), _last()
    _judge(y.reshape(-1, cout), SimpleFlat(o), a, False, f"conv_halo 64->{cout} {h}x{w} {act}")


class SimpleFlat:
    """A convolution case with its float64 tensors as [pixel][channel] rows."""

    def __init__(self, o):
        self.p, self.total, self.res = _rows64(o.p), _rows64(o.total), [_rows64(r) for r in o.res]


# ------------------------------------------------------------------------------------------ g8 (tiles 12, 13; both MFMA lane maps)
def _arms(mfma16, call, label, what):
    """call() under g8_mfma16 = 0 and = 2: the dispatched kernel is g8_kernel with `label` for both, and the two are bit-equal."""
    ys = []
    for arm in (0, 2):
        mfma16(arm)
        ys.append(call())
        assert "g8_kernel" in _last() and label in _last(), f"{what}: arm {arm} ran {_last()}"
    torch.cuda.synchronize()
    R.assert_bits_equal(ys[1].cpu().contiguous(), ys[0].cpu().contiguous(), f"{what}: 16x16x32 against 32x32x16")
    return ys


@pytest.mark.parametrize("tile", [12, 13])
@pytest.mark.parametrize("nres", [0, 1, 2])
def test_g8_rounding(mfma16, nres, tile):
    """513 x 656 <- 704 with 0 / 1 / 2 residuals (the plain and the residual epilogue): bf16_rne of the float64 result."""
    _dev()
    from ccedit_amd import ops
    from ccedit_amd.packing import pack_weight
    m, n, k = 513, 656, 704
    o = P.dyadic((m, k), (n, k), F.linear, seed=nres, nres=nres)
    pw, xd, r1, r2 = pack_weight(o.w, o.b).to("cuda"), _rows(o.x), _in_wide(o.r1), _in_wide(o.r2)
    what = f"g8 tile {tile}, {nres} residuals"

    def call():
        buf, out = _wide(m, n)
        ops.linear(xd, pw, res1=r1, res2=r2, out=out, tile=tile)
        _written(buf, n, what)
        return out
    for y in _arms(mfma16, call, G8[tile], what):
        _judge(y, o, P.ACT_NONE, False, what)


@pytest.mark.parametrize("tile", [12, 13])
@pytest.mark.parametrize("case", P.G8_GEGLU, ids=lambda c: "x".join(map(str, c)))
def test_g8_geglu(mfma16, case, tile):
    """GEGLU 300 x 512 <- 192 and packed N = 656 (inner 328, ragged)."""
    _dev()
    from ccedit_amd import ops
    from ccedit_amd.packing import pack_weight
    m, inner, k = case
    o = P.geglu_case(m, inner, k)
    pw, xd = pack_weight(o.w, o.b, geglu=True).to("cuda"), _rows(o.x)
    what = f"g8 GEGLU tile {tile} packed N={2 * inner}"

    def call():
        buf, out = _wide(m, inner)
        ops.linear(xd, pw, out=out, tile=tile)
        _written(buf, inner, what)
        return out
    for y in _arms(mfma16, call, G8[tile], what):
        P.assert_within(y.cpu(), o.ref, o.bound, what)


@pytest.mark.parametrize("tile", [12, 13])
@pytest.mark.parametrize("geglu", [False, True], ids=["plain", "geglu"])
def test_g8_layernorm_folded(mfma16, geglu, tile):
    """ops.linear(..., ln_stats=) with statistics made here: mean an integer in [-3, 3], rstd in {1/4, 1/2, 1, 2}, both per row, 300 x 512
    <- 256.  rstd * (acc - mean * colsum) + b is exact then: plain output = bf16_rne of it, GEGLU within the bound."""
    _dev()
    from ccedit_amd import ops
    from ccedit_amd.packing import _geglu_perm, fold_layernorm
    m, n, k = P.LNF_SHAPE
    o = P.lnf_case(m, n, k, geglu)
    pw = fold_layernorm([o.w.float()], [o.b.float()], torch.ones(k), torch.zeros(k), geglu=geglu).to("cuda")
    assert torch.equal(pw.colsum.double().cpu()[:n], (o.w[_geglu_perm(n)] if geglu else o.w).sum(dim=1))
    xd, st = _rows(o.x), torch.stack([o.mean, o.rstd], dim=1).float().contiguous().cuda()
    nout = n // 2 if geglu else n
    what = f"g8 LayerNorm folded {'GEGLU' if geglu else 'plain'} tile {tile}"

    def call():
        buf, out = _wide(m, nout)
        ops.linear(xd, pw, ln_stats=st, out=out, tile=tile)
        _written(buf, nout, what)
        return out
    for y in _arms(mfma16, call, "LayerNorm folded", what):
        assert G8[tile] in _last(), _last()
        if geglu:
            P.assert_within(y.cpu(), o.ref, o.bound, what)
        else:
            P.assert_ties(o.p, what)
            P.assert_rounded(y, o.p, what)


def test_g8_split_k_rounding(mfma16):
    """Split-K with the workspace lent (automatic dispatch), 300 x 1280 <- 5120 + residual: the reducer's store rounds to nearest even."""
    _dev()
    from ccedit_amd import ops
    from ccedit_amd.packing import pack_weight
    m, n, k = 300, 1280, 5120
    o = P.dyadic((m, k), (n, k), F.linear, seed=1, nres=1)
    pw, xd, rd = pack_weight(o.w, o.b).to("cuda"), _rows(o.x), _rows(o.r1)
    for y in _arms(mfma16, lambda: ops.linear(xd, pw, res1=rd), "split-K", "g8 split-K"):
        _judge(y, o, P.ACT_NONE, False, "g8 split-K")


# ------------------------------------------------------------------------------------------ register-resident weights
@pytest.mark.parametrize("case", P.LIN320_GEGLU, ids=lambda c: "x".join(map(str, c)))
def test_lin320_geglu(case):
    """tile 9, GEGLU at M = 32 / 130 and packed N = 320 / 2560: lin320_kernel."""
    _dev()
    from ccedit_amd import ops
    from ccedit_amd.packing import pack_weight
    m, inner, k = case
    o = P.geglu_case(m, inner, k)
    buf, out = _wide(m, inner)
    ops.linear(_rows(o.x), pack_weight(o.w, o.b, geglu=True).to("cuda"), out=out, tile=9)
    assert "lin320_kernel" in _last(), _last()
    what = f"lin320 GEGLU {m} x {2 * inner}"
    _written(buf, inner, what)
    P.assert_within(out.cpu(), o.ref, o.bound, what)


@pytest.mark.parametrize("m,n,k,tile,want", [(32, 320, 320, 9, "lin320s_kernel"), (130, 320, 320, 9, "lin320_kernel"),
                                             (16, 640, 640, 10, "lin640s_kernel")])
def test_streaming_linear_rounding(m, n, k, tile, want):
    """lin320s (whole 32-row tiles), lin320 (ragged M) and lin640s with a residual: the rounding case."""
    _dev()
    from ccedit_amd import ops
    from ccedit_amd.packing import pack_weight
    o = P.dyadic((m, k), (n, k), F.linear, seed=m, nres=1)
    buf, out = _wide(m, n)
    ops.linear(_rows(o.x), pack_weight(o.w, o.b).to("cuda"), res1=_in_wide(o.r1), out=out, tile=tile)
    assert want in _last(), _last()
    _written(buf, n, want)
    _judge(out, o, P.ACT_NONE, False, f"{want} {m} x {n}")


def test_temp320s_rounding():
    """tile 14: Conv1d k3 over T, three clips of three 4 x 4 frames, 320 -> 64, row bias + two residuals."""
    _dev()
    from ccedit_amd import ops
    from ccedit_amd.packing import pack_weight
    b_, t, c, cout, h, w = 3, 3, 320, 64, 4, 4
    o = P.dyadic((b_ * t, c, h, w), (cout, c, 3), E.temporal_ref(b_, t), seed=14, frames_per_bias=t)
    y = ops.conv_temporal(_nhwc(o.x), t, pack_weight(o.w, o.b).to("cuda"), group_bias=_f32(o.gb), group_rows=t * h * w, res1=_flat(o.r1),
                          res2=_flat(o.r2), tile=14)
    assert "temp320s_kernel" in _last(), _last()
    _judge(y.reshape(-1, cout), SimpleFlat(o), P.ACT_NONE, False, "temp320s")


@pytest.mark.parametrize("act", ["none", "silu"])
@pytest.mark.parametrize("cin,cout,stride", [(16, 16, 1), (16, 32, 2)])
def test_small_conv(cin, cout, stride, act):
    """small_conv3x3_kernel (automatic dispatch from 65 536 output pixels; two 200 x 328 output frames): the rounding case and SiLU."""
    _dev()
    from ccedit_amd import ops
    from ccedit_amd.packing import pack_weight
    n, h, w = 2, 200, 328
    if stride == 2:
        h, w = 2 * h, 2 * w - 2
    a = P.ACTS[act]
    o = P.dyadic((n, cin, h, w), (cout, cin, 3, 3), lambda x, wt, b: F.conv2d(x, wt, b, stride=stride, padding=1), seed=cin + stride, nres=0,
                 sat=a != P.ACT_NONE)
    if a != P.ACT_NONE:
        P.assert_saturation(o.p, "small conv")
    y = ops.conv2d(_nhwc(o.x), pack_weight(o.w, o.b).to("cuda"), stride=stride, act=a)
    assert "small_conv3x3_kernel" in _last(), _last()
    _judge(y.reshape(-1, y.shape[-1])[:, :cout], SimpleFlat(o), a, False, f"small conv {cin}->{cout} stride {stride} {act}")


# ------------------------------------------------------------------------------------------ ff320, ln = False
@pytest.mark.parametrize("m", P.FF_M)
def test_ff320(m):
    """x + W2 . bf16(v gelu(u)) + b2 without the LayerNorm, M = 48 (a partly filled round of 128 tokens) and 200 (one whole round, one
    ragged): the hidden value carries GeluPipe's budget and its bf16 rounding (bh), the output sum_k |w2_jk| bh_k, the fp32
    accumulation of the few non-zero terms and half an output ulp (_epilogue_ref.ff320_case)."""
    _dev()
    from ccedit_amd import ops
    from ccedit_amd.packing import pack_ff320
    o = P.ff320_case(m)
    pk = pack_ff320(o.w.float(), o.b.float(), o.w2.float(), o.b2.float(), None, None, device="cuda")
    out = R.sentinel_fill(m * P.FF_DIM, BF, "cuda").view(m, P.FF_DIM)
    ops.ff320(_rows(o.x), pk, ln=False, out=out)
    assert "ff320_kernel" in _last() and "to_out" not in _last(), _last()
    assert not bool(R.is_sentinel(out.cpu()).any()), "ff320: elements never written"
    P.assert_within(out.cpu(), o.ref, o.bound, f"ff320 M={m}")
