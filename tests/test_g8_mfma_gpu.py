"""The persistent eight-phase GEMM on 16x16x32 MFMAs (policy g8_mfma16, csrc/gemm8p.hip: MF16 = 1) against its 32x32x16 arm.

The two arms compute the same fp32 sums in a different order (k in groups of 32 instead of 16), and a lane owns other (channel,
pixel) pairs of the accumulator block.  On the integer-valued operands of tests/_exact_ints.py the order cannot matter, so arm 2
(16x16x32 on every arm of the kernel) must give the BITS of arm 0 and of the float64 reference: a channel or pixel misplaced by the new
accumulator map, a fragment read from the wrong row, a gate paired with the wrong value cannot hide behind a tolerance.  Every case
runs the arm-2 launch five times and compares the repeats bit for bit — a misplaced wait shows there first — and asserts the kernel
that ran, so a silent fall-back to another kernel cannot pass.  The host-only test at the end checks the policy table.
"""
import ctypes
import functools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _exact_ints as E  # noqa: E402

BF = torch.bfloat16
G8 = {12: "g8_kernel 256ch x 256pix", 13: "g8_kernel 128ch x 512pix"}
REPEATS = 5


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


def _nchw(y):
    return y.double().cpu().permute(0, 3, 1, 2).contiguous()


def _equal(got, ref, what):
    got = got.double().cpu()
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    if not torch.equal(got, ref):
        bad = (got != ref).nonzero()
        first = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {bad.shape[0]} of {ref.numel()} values differ from the reference; first at {first}: "
                             f"got {got[first].item()} want {ref[first].item()}; max |diff| {(got - ref).abs().max().item()}")


def _arms(mfma16, call, label, what, bit_equal=True):
    """call() -> tuple of tensors.  Arm 0 once, arm 2 REPEATS times: repeats bit-equal, arm 2 bit-equal to arm 0 (unless the case
    says why not), the dispatched kernel is g8_kernel with `label` in its name for both.  Returns (arm 0 results, arm 2 results)."""
    mfma16(0)
    y0 = call()
    assert "g8_kernel" in _last() and label in _last(), f"{what}: arm 0 ran {_last()}"
    mfma16(2)
    y2 = None
    for rep in range(REPEATS):
        y = call()
        assert "g8_kernel" in _last() and label in _last(), f"{what}: arm 2 ran {_last()}"
        if y2 is not None:
            for i, (a, b) in enumerate(zip(y, y2)):
                assert torch.equal(a, b), f"{what}: arm 2, result {i}: repeat {rep} differs from the first launch"
        y2 = y
    torch.cuda.synchronize()
    if bit_equal:
        for i, (a, b) in enumerate(zip(y2, y0)):
            _equal(a, b.double().cpu(), f"{what}: 16x16x32 against 32x32x16, result {i}")
    return y0, y2


# ------------------------------------------------------------------------------------------ Linear, 0 / 1 / 2 residuals
@functools.lru_cache(maxsize=None)
def _lin_operands(m, n, k, nres):
    return E.operands((m, k), (n, k), F.linear, seed=m + nres, nres=nres)


# two K tiles | eleven K tiles (odd), ragged M and N for both shapes | N whole 128-channel tiles, 2.5 256-channel tiles
_LIN = [(257, 384, 128), (513, 656, 704), (700, 640, 192)]


@pytest.mark.gpu
@pytest.mark.parametrize("tile", [12, 13])
@pytest.mark.parametrize("nres", [0, 1, 2])
@pytest.mark.parametrize("m,n,k", _LIN)
def test_linear_bit_equal(mfma16, m, n, k, nres, tile):
    _dev()
    from ccedit_amd import ops
    from ccedit_amd.packing import pack_weight
    o = _lin_operands(m, n, k, nres)
    pw, xd, kw = pack_weight(o.w, o.b).to("cuda"), _rows(o.x), dict(res1=_rows(o.r1), res2=_rows(o.r2), tile=tile)
    what = f"linear {m}x{n}<-{k}, {nres} residuals, tile {tile}"
    _, y2 = _arms(mfma16, lambda: (ops.linear(xd, pw, **kw),), G8[tile], what)
    _equal(y2[0], o.ref, what)


@pytest.mark.gpu
@pytest.mark.parametrize("tile", [12, 13])
@pytest.mark.parametrize("nres", [0, 1])
def test_linear_row_sums(mfma16, nres, tile):
    """row_sums (the LayerNorm sums left for the consumer) from the plain and from the residual epilogue: equal to the float64 row sums."""
    _dev()
    from ccedit_amd import ops
    from ccedit_amd.packing import pack_weight
    m, n, k = 513, 656, 704
    o = _lin_operands(m, n, k, nres)
    pw, xd, kw = pack_weight(o.w, o.b).to("cuda"), _rows(o.x), dict(res1=_rows(o.r1), tile=tile, row_sums=True)

    def call():
        y = ops.linear(xd, pw, **kw)
        return y, ops.ln_sums_of(y).clone()
    what = f"linear with row_sums, {nres} residuals, tile {tile}"
    _, y2 = _arms(mfma16, call, G8[tile], what)
    _equal(y2[0], o.ref, what)
    _equal(y2[1], torch.stack([o.ref.sum(dim=1), (o.ref * o.ref).sum(dim=1)], dim=1), what + ": sums")


@pytest.mark.gpu
@pytest.mark.parametrize("tile", [12, 13])
@pytest.mark.parametrize("nres", [0, 1])
def test_linear_row_bias_and_statistics(mfma16, nres, tile):
    """Per-frame row bias + fused GroupNorm statistics at the shape of test_exact_gpu.py::test_g8_linear_row_bias_and_statistics
    (3 frames of 512 rows onto 640 channels: gn_stats needs frames of whole 128-row blocks), plain and residual epilogue."""
    _dev()
    from ccedit_amd import ops
    from ccedit_amd.packing import pack_weight
    nfr, hw, k, cout = 3, 512, 256, 640
    o = E.operands((nfr * hw, k), (cout, k), F.linear, seed=tile + nres, rows_per_bias=hw, nres=nres)
    pw, xd = pack_weight(o.w, o.b).to("cuda"), _rows(o.x)
    kw = dict(group_bias=_f32(o.gb), group_rows=hw, res1=_rows(o.r1), gn_rows=hw, tile=tile)

    def call():
        y = ops.linear(xd, pw, **kw)
        st = ops.gn_stats_of(y, hw)
        assert st is not None, "the producer left no statistics"
        return y, st.clone()
    what = f"linear + row bias + statistics, {nres} residuals, tile {tile}"
    _, y2 = _arms(mfma16, call, G8[tile], what)
    _equal(y2[0], o.ref, what)
    _equal(y2[1], E.group_sums(o.ref.reshape(nfr, hw, 1, cout)), what + ": GroupNorm statistics")


@pytest.mark.gpu
@pytest.mark.parametrize("tile", [12, 13])
def test_linear_row_bias_ragged(mfma16, tile):
    """300 rows x 320 channels with a row bias per 160 rows: the last bias group and the last tiles of both dimensions are ragged."""
    _dev()
    from ccedit_amd import ops
    from ccedit_amd.packing import pack_weight
    m, n, k, rows = 300, 320, 192, 160
    o = E.operands((m, k), (n, k), F.linear, seed=tile, rows_per_bias=rows, nres=1)
    pw, xd = pack_weight(o.w, o.b).to("cuda"), _rows(o.x)
    kw = dict(group_bias=_f32(o.gb), group_rows=rows, res1=_rows(o.r1), tile=tile)
    _, y2 = _arms(mfma16, lambda: (ops.linear(xd, pw, **kw),), G8[tile], f"linear + row bias 300x320 tile {tile}")
    _equal(y2[0], o.ref, f"linear + row bias 300x320 tile {tile}")


# ------------------------------------------------------------------------------------------ GEGLU, LayerNorm folded
@pytest.mark.gpu
@pytest.mark.parametrize("tile", [12, 13])
def test_geglu_bit_equal(mfma16, tile):
    """GEGLU projection 300 x 512 <- 192: the fp32 pre-activations are exact integers in both arms, so the GELU sees identical
    inputs and the outputs are bit-equal; against float64 a * gelu(gate) within 2^-7 max|ref| (tests/test_ops_gpu.py: _close's
    relative term, without its absolute one)."""
    _dev()
    from ccedit_amd import ops
    from ccedit_amd.packing import pack_weight
    m, n, k = 300, 512, 192
    o = E.operands((m, k), (n, k), F.linear, seed=tile, nres=0)
    a, gate = o.ref.chunk(2, dim=-1)
    ref = a * F.gelu(gate)
    pw, xd = pack_weight(o.w, o.b, geglu=True).to("cuda"), _rows(o.x)
    _, y2 = _arms(mfma16, lambda: (ops.linear(xd, pw, tile=tile),), G8[tile], f"GEGLU tile {tile}")
    got = y2[0].double().cpu()
    assert got.shape == ref.shape
    err, lim = (got - ref).abs().max().item(), 2.0 ** -7 * ref.abs().max().item()
    print(f"GEGLU tile {tile}: max err {err:.4g}, limit {lim:.4g}")
    assert err <= lim, f"GEGLU tile {tile}: max err {err:.4g} > {lim:.4g}"


def _rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF).float()


@functools.lru_cache(maxsize=None)
def _lnf_case(geglu):
    m, c, n = 300, 256, 512
    x = _rnd(m, c, seed=1)
    x[: m // 4] += 3.0                                  # a quarter of the rows: mean 3, std 1
    x[m // 4: m // 2] *= 4.0
    w, b = _rnd(n, c, seed=2, scale=c ** -0.5), _rnd(n, seed=3)
    g, be = _rnd(c, seed=4) * 0.2 + 1.0, _rnd(c, seed=5) * 0.2
    ref = F.linear(F.layer_norm(x.double(), (c,), g.double(), be.double(), 1e-5), w.double(), b.double())
    if geglu:
        a, gate = ref.chunk(2, dim=-1)
        ref = a * F.gelu(gate)
    return x, w, b, g, be, ref


@pytest.mark.gpu
@pytest.mark.parametrize("tile", [12, 13])
@pytest.mark.parametrize("geglu", [False, True])
def test_layernorm_folded(mfma16, geglu, tile):
    """Linear(LayerNorm(x)) 300 x 512 <- 256 with the statistics applied in the epilogue, plain and GEGLU: rstd is no integer, so the
    arms may differ in the last bit — each is held to the float64 reference with the tolerance of
    test_ops_gpu.py::test_layernorm_folded_into_persistent_gemm (2^-7 max|ref| + 1e-3); the arm-2 repeats are still bit-equal."""
    _dev()
    from ccedit_amd import ops
    from ccedit_amd.packing import fold_layernorm
    x, w, b, g, be, ref = _lnf_case(geglu)
    xc = x.to(BF).cuda()
    st = ops.row_stats(xc, 1e-5)
    pw = fold_layernorm([w], [b], g, be, geglu=geglu).to("cuda")
    y0, y2 = _arms(mfma16, lambda: (ops.linear(xc, pw, ln_stats=st, tile=tile),), "LayerNorm folded", f"LayerNorm folded geglu={geglu} tile {tile}",
                   bit_equal=False)
    assert G8[tile] in _last(), _last()
    lim = 2.0 ** -7 * ref.abs().max().item() + 1e-3
    for arm, y in ((0, y0[0]), (2, y2[0])):
        got = y.double().cpu()
        assert got.shape == ref.shape and torch.isfinite(got).all()
        err = (got - ref).abs().max().item()
        print(f"LayerNorm folded geglu={geglu} tile {tile} arm {arm}: max err {err:.4g}, limit {lim:.4g}")
        assert err <= lim, f"arm {arm}: max err {err:.4g} > {lim:.4g}"


# ------------------------------------------------------------------------------------------ gathers
@pytest.mark.gpu
@pytest.mark.parametrize("tile", [12, 13])
def test_temporal_taps(mfma16, tile):
    """(1, 5, 64 -> 256, 16 x 32): row bias, two residuals and the fused statistics."""
    _dev()
    from ccedit_amd import ops
    from ccedit_amd.packing import pack_weight
    b_, t, c, cout, h, w = 1, 5, 64, 256, 16, 32
    o = E.operands((b_ * t, c, h, w), (cout, c, 3), E.temporal_ref(b_, t), seed=tile, frames_per_bias=t)
    pw, xd = pack_weight(o.w, o.b).to("cuda"), _nhwc(o.x)
    kw = dict(group_bias=_f32(o.gb), group_rows=t * h * w, res1=_flat(o.r1), res2=_flat(o.r2), gn=True, tile=tile)

    def call():
        y = ops.conv_temporal(xd, t, pw, **kw)
        return y, ops.gn_stats_of(y, h * w).clone()
    _, y2 = _arms(mfma16, call, G8[tile] + ", temporal taps", f"temporal taps tile {tile}")
    _equal(_nchw(y2[0]), o.ref, f"temporal taps tile {tile}")
    _equal(y2[1], E.group_sums(o.ref.permute(0, 2, 3, 1).reshape(b_ * t, h * w, 1, cout)), "temporal taps: GroupNorm statistics")


@pytest.mark.gpu
@pytest.mark.parametrize("tile", [12, 13])
@pytest.mark.parametrize("n,cin,cout,h,w", [(3, 64, 256, 8, 16), (5, 64, 384, 12, 16)])
def test_conv3x3_taps(mfma16, n, cin, cout, h, w, tile):
    """Nine-tap gather with row bias + residual; at 8 x 16 (whole 128-pixel blocks) the fused statistics too."""
    _dev()
    from ccedit_amd import ops
    from ccedit_amd.packing import pack_weight
    o = E.operands((n, cin, h, w), (cout, cin, 3, 3), lambda x, wt, b: F.conv2d(x, wt, b, padding=1), seed=n + tile, frames_per_bias=1, nres=1)
    pw, xd = pack_weight(o.w, o.b).to("cuda"), _nhwc(o.x)
    with_stats = (h * w) % 128 == 0 and cout >= 256
    kw = dict(group_bias=_f32(o.gb), group_rows=h * w, res1=_flat(o.r1), gn=with_stats, tile=tile)

    def call():
        y = ops.conv2d(xd, pw, **kw)
        return (y, ops.gn_stats_of(y, h * w).clone()) if with_stats else (y,)
    what = f"3x3 taps {n}x{h}x{w} -> {cout} tile {tile}"
    _, y2 = _arms(mfma16, call, G8[tile] + ", 3x3 taps", what)
    _equal(_nchw(y2[0]), o.ref, what)
    if with_stats:
        _equal(y2[1], E.group_sums(o.ref.permute(0, 2, 3, 1).reshape(n, h * w, 1, cout)), what + ": GroupNorm statistics")


@pytest.mark.gpu
@pytest.mark.parametrize("tile", [12, 13])
def test_upsample_parity_taps(mfma16, tile):
    """conv3x3(nearest 2x(x)) as four 2 x 2 parity convs on one odd 5 x 7 frame (the case of test_exact_gpu.py::test_upsample_parity_convs)."""
    _dev()
    from ccedit_amd import ops
    from ccedit_amd.packing import pack_upsample_parities
    n, h, w, cin, cout = 1, 5, 7, 64, 64
    o = E.operands((n, cin, h, w), (cout, cin, 3, 3),
                   lambda x, wt, b: F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), wt, b, padding=1), seed=tile, nres=0)
    pws, xd = pack_upsample_parities(o.w, o.b, device="cuda"), _nhwc(o.x)
    _, y2 = _arms(mfma16, lambda: (ops.conv2d_upsampled(xd, pws, tile=tile),), G8[tile] + ", upsample parity taps", f"parity convs tile {tile}")
    _equal(_nchw(y2[0]), o.ref, f"parity convs tile {tile}")


@pytest.mark.gpu
def test_split_k(mfma16):
    """Split-K, 300 x 1280 <- 5120 + residual (automatic dispatch with the workspace lent): the slots are in register order and writer
    and reducer are the same instantiation."""
    _dev()
    from ccedit_amd import ops
    from ccedit_amd.packing import pack_weight
    m, n, k = 300, 1280, 5120
    o = E.operands((m, k), (n, k), F.linear, seed=1, nres=1)
    pw, xd, rd = pack_weight(o.w, o.b).to("cuda"), _rows(o.x), _rows(o.r1)
    _, y2 = _arms(mfma16, lambda: (ops.linear(xd, pw, res1=rd),), "split-K", "split-K linear")
    _equal(y2[0], o.ref, "split-K linear")


# ------------------------------------------------------------------------------------------ host only
def test_policy_table_has_the_switch():
    """policy.TABLE carries g8_mfma16 on the library side, generic() turns it off, and the library takes 0 / 1 / 2 for it while every
    other name of the table is still accepted with its default."""
    from ccedit_amd import hip, policy
    assert "g8_mfma16" in policy.TABLE and policy.TABLE["g8_mfma16"][1] == "lib"
    assert "g8_mfma16=0" in policy.generic().split(",")
    lib = hip.lib()
    names = lib.ccedit_policy_names().decode().split(",")
    assert "g8_mfma16" in names
    assert sorted(names) == sorted(k for k, v in policy.TABLE.items() if v[1] == "lib")
    old = ctypes.c_int32(0)
    assert lib.ccedit_policy_get(b"g8_mfma16", ctypes.byref(old)) == 0
    try:
        for v in (0, 1, 2):
            got = ctypes.c_int32(-1)
            assert lib.ccedit_policy_set(b"g8_mfma16", v) == 0
            assert lib.ccedit_policy_get(b"g8_mfma16", ctypes.byref(got)) == 0 and got.value == v
    finally:
        lib.ccedit_policy_set(b"g8_mfma16", old.value)
    for name, (dflt, side, _) in policy.TABLE.items():
        if side == "lib":
            cur = ctypes.c_int32(0)
            assert lib.ccedit_policy_get(name.encode(), ctypes.byref(cur)) == 0, name
            assert lib.ccedit_policy_set(name.encode(), cur.value) == 0, name
    assert lib.ccedit_policy_set(b"g8_mfma17", 1) != 0
