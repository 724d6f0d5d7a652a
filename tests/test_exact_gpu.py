"""Exact-arithmetic parity on a real MI355X: every GEMM, convolution and statistics kernel against an integer reference, bit for bit.

tests/test_ops_gpu.py holds the matrix kernels to rounding-level tolerances on Gaussian operands; one dropped K element, one wrong
border tap or one pixel missing from a GroupNorm sum passes those (tests/test_exact_host.py shows it on the CPU).  Here the operands
are small integers (tests/_exact_ints.py), chosen so that every number a kernel can form is exactly representable:

  * products of two bf16 integers are exact in fp32, and every partial sum in any order stays below 2^24 — exact in the fp32
    accumulators, in the fp32 split-K workspace and in fp32 statistics partials;
  * the value after bias, row bias and residuals is an integer with |r| <= 256, and every such integer is a bf16 number (fp32 outputs
    of the VAE kernels: |r| <= 2^24);
  * sums and sums of squares of those outputs are far below 2^53: exact in the fp64 accumulators in any atomic order.

The generator asserts two conditions on its INPUTS before anything runs on the GPU: max|ref| <= 256 (2^24 for fp32 outputs), and
every K column of the weight — every (tap, cin) of a packed convolution — carries a non-zero, so every element of A is observed.
The convolution cases past one 64-channel input chunk ask for more (`rows_per_tile=16`): a non-zero in every K column inside EVERY
block of 16 output rows, the smallest MFMA row tile of the library — a kernel's defect lives in one channel tile, and at 320 -> 640
more than half of the (32-channel tile, K column) pairs of the plain recipe hold no weight (tests/test_exact_host.py).
The assertions on the kernels are torch.equal against float64 F.linear / F.conv2d / F.conv1d, and the label of the kernel that ran.

What this rests on: every kernel here accumulates bf16 x bf16 products in fp32 inside the matrix pipe (v_mfma_f32_32x32x16_bf16,
v_mfma_f32_16x16x32_bf16; the fp32 arm v_mfma_f32_32x32x2_f32).  tests/test_vae_f32_gpu.py already holds both fp32 arms to exact
integers (|x| <= 2000, |w| <= 3, K = 4608); this file extends that premise to every family.  Should a correct kernel differ by the
hardware's own arithmetic (a pattern tied to magnitude, not to tile edges, taps or tails), the remedy is a smaller operand range
asserted here and recorded in DESIGN.md section 5 — never a tolerance.
"""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _exact_ints as E  # noqa: E402

pytestmark = pytest.mark.gpu

BF = torch.bfloat16

# label of tap_gemm_kernel's block shapes by `tile` (csrc/gemm.hip: launch_tile)
TAP = {1: "tap_gemm_kernel 128ch x 128pix, 2 stages of K=64", 2: "tap_gemm_kernel 64ch x 256pix, 2 stages of K=64",
       3: "tap_gemm_kernel 128ch x 256pix, 3 stages of K=64", 4: "tap_gemm_kernel 256ch x 256pix, 4 stages of K=32",
       5: "tap_gemm_kernel 128ch x 512pix, 4 stages of K=32", 6: "tap_gemm_kernel 320ch x 128pix, 2 stages of K=32",
       7: "tap_gemm_kernel 256ch x 256pix, 4 stages of K=32"}
G8 = {12: "g8_kernel 256ch x 256pix", 13: "g8_kernel 128ch x 512pix"}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _last():
    from ccedit_amd import hip
    return hip.lib().ccedit_last_kernel().decode()


def _rows(t):      # float64 integers (M, C) -> bf16 cuda
    return None if t is None else t.to(BF).cuda()


def _f32(t):
    return None if t is None else t.float().cuda()


def _nhwc(t):      # float64 (N, C, H, W) -> bf16 cuda (N, H, W, C)
    return t.permute(0, 2, 3, 1).contiguous().to(BF).cuda()


def _flat(t):      # float64 (N, C, H, W) -> bf16 cuda [N*H*W][C]
    return None if t is None else _nhwc(t).reshape(-1, t.shape[1])


def _nchw(y):
    return y.double().cpu().permute(0, 3, 1, 2).contiguous()


def _equal(got, ref, what):
    got = got.double().cpu()
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    if not torch.equal(got, ref):
        bad = (got != ref).nonzero()
        first = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {bad.shape[0]} of {ref.numel()} values differ from the integer reference; first at {first}: "
                             f"got {got[first].item()} want {ref[first].item()}; max |diff| {(got - ref).abs().max().item()}")


def _strided(t, lead=64):
    """The same bf16 rows as columns [lead, lead + C) of a wider buffer whose other columns hold 7 (must not be read or written)."""
    wide = torch.full((t.shape[0], t.shape[1] + 2 * lead), 7.0, dtype=BF, device=t.device)
    wide[:, lead:lead + t.shape[1]] = t
    return wide[:, lead:lead + t.shape[1]]


def _stats_equal(y, hw, what):
    """The producer's fused GroupNorm statistics against the float64 sums of the values it wrote."""
    from ccedit_amd import ops
    st = ops.gn_stats_of(y, hw)
    assert st is not None, f"{what}: the producer left no statistics"
    n, c = y.numel() // (hw * y.shape[-1]), y.shape[-1]
    _equal(st, E.group_sums(y.cpu().reshape(n, hw, 1, c)), f"{what}: GroupNorm statistics")
    return st


# ------------------------------------------------------------------------------------------ tap_gemm, Linear
_LIN = [(300, 320, 320, 50), (77, 960, 768, 11), (64, 640, 40, 16), (1000, 4, 320, 125)]      # ragged M / N; K tail (Kpad 64); N = 4


@pytest.mark.parametrize("m,n,k,rows,tile", [s + (t,) for s in _LIN for t in range(1, 8) if t != 6 or s[1] % 320 == 0])
def test_tap_gemm_linear(m, n, k, rows, tile):
    """tap_gemm_kernel in its seven Linear block shapes: bias + row bias + two residuals, ragged M and N tiles, a K tail."""
    _dev()
    from ccedit_amd import ops
    from ccedit_amd.packing import pack_weight
    o = E.operands((m, k), (n, k), F.linear, seed=m + tile, rows_per_bias=rows)
    y = ops.linear(_rows(o.x), pack_weight(o.w, o.b).to("cuda"), group_bias=_f32(o.gb), group_rows=rows, res1=_rows(o.r1),
                   res2=_rows(o.r2), tile=tile)
    assert TAP[tile] in _last(), _last()
    _equal(y, o.ref, f"tap_gemm linear {m}x{n}x{k} tile {tile}")


@pytest.mark.parametrize("tile", [1, 2, 3, 4, 5, 6, 7])
def test_tap_gemm_linear_strided_and_second_source(tile):
    """Strided source, output and residuals (column slices of wider buffers that must stay untouched), and a second source whose
    concat split (40 of 64 channels) lands inside a K tile."""
    _dev()
    from ccedit_amd import ops
    from ccedit_amd.packing import pack_weight
    m, n, c1, c2 = 150, 320, 40, 24
    o = E.operands((m, c1 + c2), (n, c1 + c2), F.linear, seed=tile, rows_per_bias=50)
    pw = pack_weight(o.w, o.b).to("cuda")
    wide = torch.full((m, 2 * n), 7.0, dtype=BF, device="cuda")
    ops.linear(_strided(_rows(o.x[:, :c1])), pw, a2=_strided(_rows(o.x[:, c1:])), group_bias=_f32(o.gb), group_rows=50,
               res1=_strided(_rows(o.r1)), res2=_strided(_rows(o.r2), 32), out=wide[:, n:], tile=tile)
    assert TAP[tile] in _last(), _last()
    _equal(wide[:, n:], o.ref, f"strided operands + second source, tile {tile}")
    assert bool((wide[:, :n] == 7.0).all()), "columns outside the output slice were written"


# ------------------------------------------------------------------------------------------ tap_gemm, Conv2d
def _conv_case(kind, cin, cout, seed, rows_per_tile=0):
    """(operands, call) of one Conv2d geometry on two 9 x 7 frames (126 output pixels at stride 1: a tile straddles the frames)."""
    n, h, w = 2, 9, 7
    kw = {}
    halo = None
    if kind == "s1":
        fwd = lambda x, wt, b: F.conv2d(x, wt, b, padding=1)
    elif kind == "s2":
        fwd, kw = (lambda x, wt, b: F.conv2d(x, wt, b, stride=2, padding=1)), dict(stride=2)
    elif kind == "up":
        fwd, kw = (lambda x, wt, b: F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), wt, b, padding=1)), dict(upsample=True)
    elif kind == "asym":       # pad right / bottom only, stride 2, conv pad 0: taps outside the source read zeros
        fwd = lambda x, wt, b: F.conv2d(F.pad(x, (0, 1, 0, 1)), wt, b, stride=2)
        kw = dict(stride=2, pad=0, out_hw=((h + 1 - 3) // 2 + 1, (w + 1 - 3) // 2 + 1))
    elif kind == "vpad":       # the frames carry their own halo rows: no vertical padding
        fwd, kw = (lambda x, wt, b: F.conv2d(x, wt, b, padding=(0, 1))), dict(vpad=True)
    else:                      # "halo_top" / "halo_bot": one neighbour row as a separate tensor, the frame ends on the other side
        g = E.gen(seed + 99)
        halo = E.ints((n, cin, 1, w), -2, 2, g)
        zero = torch.zeros_like(halo)
        rows = (halo, zero) if kind == "halo_top" else (zero, halo)
        fwd = lambda x, wt, b: F.conv2d(torch.cat([rows[0], x, rows[1]], dim=2), wt, b, padding=(0, 1))
    o = E.operands((n, cin, h, w), (cout, cin, 3, 3), fwd, seed=seed, frames_per_bias=1, rows_per_tile=rows_per_tile)
    if halo is not None:
        hr = _nhwc(halo).reshape(n, w, cin).contiguous()
        kw = dict(halo=(hr, None) if kind == "halo_top" else (None, hr))
    return o, kw


@pytest.mark.parametrize("kind,cin,cout,tile", [(k, 64, 96, t) for k in ("s1", "s2", "up", "asym") for t in (1, 2, 3, 4, 5)]
                         + [(k, 64, 96, t) for k in ("vpad", "halo_top", "halo_bot") for t in (1, 2, 3)]
                         + [(k, 8, 320, t) for k in ("s1", "s2") for t in (1, 2, 3, 4, 5, 6)]
                         + [(k, 128, 96, t) for k in ("s1", "s2", "up", "asym") for t in (1, 2, 3, 4, 5)]
                         + [(k, 128, 96, t) for k in ("vpad", "halo_top", "halo_bot") for t in (1, 2, 3)]
                         + [("s1", 192, 320, t) for t in (1, 2, 3, 4, 5, 6)])
def test_tap_gemm_conv2d(kind, cin, cout, tile):
    """tap_gemm_kernel's 3x3 gather: stride 1 / 2, the fused nearest-2x source, asymmetric padding through out_hw, halo rows inside
    the frames (vpad) or as separate tensors with one side None, Cin = 8 (the padded latent; K = [tap][Cin] order) and Cin = 64
    (K = [Cin/64][tap][64] order) — image borders on all four sides of 9 x 7 frames, per-frame row bias and two residuals.
    Cin = 128 / 192: the K order read past chunk 0 (k-tile c * 9 + tap), every K column observed in every 16-channel block."""
    _dev()
    from ccedit_amd import ops
    from ccedit_amd.packing import pack_weight
    o, kw = _conv_case(kind, cin, cout, seed=tile + cin, rows_per_tile=16 if cin > 64 else 0)
    hw = o.ref.shape[2] * o.ref.shape[3]
    y = ops.conv2d(_nhwc(o.x), pack_weight(o.w, o.b).to("cuda"), group_bias=_f32(o.gb), group_rows=hw, res1=_flat(o.r1),
                   res2=_flat(o.r2), tile=tile, **kw)
    assert TAP[tile] in _last() and ("neighbour halo rows" in _last()) == kind.startswith("halo"), _last()
    _equal(_nchw(y), o.ref, f"tap_gemm conv {kind} {cin}->{cout} tile {tile}")


# ------------------------------------------------------------------------------------------ Conv1d over T: tap_gemm and g8
@pytest.mark.parametrize("t,tile,c", [pytest.param(t, tile, 64, id=f"{tile}-{t}") for t in (2, 3, 17) for tile in (1, 2, 3, 4, 5, 12, 13)]
                         + [pytest.param(3, tile, 128, id=f"{tile}-3-c128") for tile in (1, 2, 3, 4, 5, 12, 13)])
def test_temporal_conv(t, tile, c):
    """Conv1d k3 over T, two clips: the taps at the clip ends AND between the clips are zeros.  tap_gemm on ragged 3 x 5 frames, the
    persistent kernel's temporal gather on 4 x 8 frames (its row bias wants 32-row groups); per-clip row bias, two residuals.
    C = 128: two 64-channel chunks, every K column observed in every 16-channel block."""
    _dev()
    from ccedit_amd import ops
    from ccedit_amd.packing import pack_weight
    b_, cout = 2, 96
    h, w = (4, 8) if tile >= 12 else (3, 5)
    o = E.operands((b_ * t, c, h, w), (cout, c, 3), E.temporal_ref(b_, t), seed=10 * t + tile, frames_per_bias=t,
                   rows_per_tile=16 if c > 64 else 0)
    y = ops.conv_temporal(_nhwc(o.x), t, pack_weight(o.w, o.b).to("cuda"), group_bias=_f32(o.gb), group_rows=t * h * w,
                          res1=_flat(o.r1), res2=_flat(o.r2), tile=tile)
    want = G8[tile] + ", temporal taps" if tile >= 12 else TAP[tile]
    assert want in _last(), _last()
    _equal(_nchw(y), o.ref, f"temporal conv T={t} C={c} tile {tile}")


def test_temporal_conv_frame_sharded():
    """conv_temporal_sharded: every shard sees [halo | local frames | halo] per clip; halo frames outside the clip hold poison that must
    be ignored.  The shards stitched by hand equal the unsharded reference."""
    _dev()
    from ccedit_amd import ops
    from ccedit_amd.packing import pack_weight
    b_, t, c, h, w = 2, 5, 64, 4, 6
    o = E.operands((b_ * t, c, h, w), (c, c, 3), E.temporal_ref(b_, t), seed=5, nres=1)
    pw = pack_weight(o.w, o.b).to("cuda")
    x5, r5 = _nhwc(o.x).view(b_, t, h, w, c), _nhwc(o.r1).view(b_, t, h, w, c)
    outs = []
    for lo, hi in [(0, 2), (2, 3), (3, 5)]:
        tl = hi - lo
        ext = torch.full((b_, tl + 2, h, w, c), 7.0, dtype=BF, device="cuda")
        ext[:, 1:tl + 1] = x5[:, lo:hi]
        if lo > 0:
            ext[:, 0] = x5[:, lo - 1]
        if hi < t:
            ext[:, tl + 1] = x5[:, hi]
        y = ops.conv_temporal_sharded(ext.view(-1, h, w, c), b_, tl, lo, t, pw, res1=r5[:, lo:hi].contiguous().view(-1, c))
        assert "tap_gemm_kernel" in _last(), _last()
        outs.append(y.view(b_, tl, h, w, c))
    _equal(_nchw(torch.cat(outs, dim=1).reshape(b_ * t, h, w, c)), o.ref, "frame-sharded temporal conv")


# ------------------------------------------------------------------------------------------ convhalo (tile 8)
@pytest.mark.parametrize("cin,cout,h,w", [(64, 128, 16, 32), (64, 320, 16, 20), (64, 320, 16, 24)])      # 16 x 20: ragged last column
def test_conv_halo(cin, cout, h, w):
    """conv_halo_kernel: the input rectangle and its halo staged in LDS, nine taps read at shifted rows; image borders on all four
    sides, a ragged last rectangle column, row bias + residual, and (16 x 24 -> 320 channels: whole 128-pixel blocks) the statistics."""
    _dev()
    from ccedit_amd import ops
    from ccedit_amd.packing import pack_weight
    n = 3
    o = E.operands((n, cin, h, w), (cout, cin, 3, 3), lambda x, wt, b: F.conv2d(x, wt, b, padding=1), seed=w, frames_per_bias=1, nres=1)
    pw, xd = pack_weight(o.w, o.b).to("cuda"), _nhwc(o.x)
    kw = dict(group_bias=_f32(o.gb), group_rows=h * w, res1=_flat(o.r1), gn=True, tile=8)
    y = ops.conv2d(xd, pw, **kw)
    assert "conv_halo_kernel" in _last(), _last()
    _equal(_nchw(y), o.ref, f"halo conv {cin}->{cout} {h}x{w}")
    if cout >= 256 and (h * w) % 128 == 0:
        st = _stats_equal(y, h * w, "halo conv")
        for _ in range(2):
            y2 = ops.conv2d(xd, pw, **kw)
            assert torch.equal(y2, y) and torch.equal(ops.gn_stats_of(y2, h * w), st), "halo conv: run-to-run difference"
    else:
        assert ops.gn_stats_of(y, h * w) is None


# ---- convhalo past one 64-channel input chunk, both weight-ring arms (library policy `conv_halo`: 1 four-slot, 2 two-slot)
# (frames, Cin, Cout, H, W) and what the case reaches in csrc/convhalo.hip:
HALO_CASES = [
    (3, 128, 128, 8, 16),     # two chunks: both halo buffers, the waits with a halo rectangle in flight; one channel tile
    (3, 192, 320, 8, 12),     # three chunks (buffer 0 reused); 8 x 16 rectangles with 12 of 16 columns used; narrow last tile
    (2, 320, 640, 16, 24),    # five chunks; 16 x 8 rectangles; five channel tiles in groups 3 + 2 (cgroup); statistics, 384 rows
    (2, 128, 960, 16, 16),    # tiles_y = 2; eight channel tiles in groups 3 + 3 + 2, the last one narrow; statistics
    (2, 128, 1280, 16, 8),    # 16 x 8 with one rectangle column; ten channel tiles in groups 3 + 3 + 3 + 1; statistics, 128 rows
    (9, 128, 256, 8, 16),     # nine pixel tiles on eight XCDs: pt_per_xcd = 2, workgroups that return early
    (2, 128, 256, 24, 40),    # H a multiple of 8, not of 16: three rectangle rows, the third column ragged (8 of 16)
    (2, 128, 256, 32, 20),    # 16 x 8 rectangles, two rectangle rows, the third column ragged (4 of 8)
    (1, 64, 64, 8, 16),       # a narrow tile with no full tile beside it
]
HALO_LABEL = {1: "conv_halo_kernel, four-slot weight ring", 2: "conv_halo_kernel, two-slot weight ring"}
_halo_cache = {}


def _halo_operands(case):
    """Operands and float64 reference of one case: computed once, shared by the tests below, never modified."""
    if case not in _halo_cache:
        n, cin, cout, h, w = case
        _halo_cache[case] = E.operands((n, cin, h, w), (cout, cin, 3, 3), lambda x, wt, b: F.conv2d(x, wt, b, padding=1), seed=cout + w,
                                       frames_per_bias=1, nres=1, rows_per_tile=16)
    return _halo_cache[case]


def _set_halo_arm(value):
    from ccedit_amd import hip
    assert hip.lib().ccedit_policy_set(b"conv_halo", value) == 0


@pytest.fixture(params=[1, 2], ids=["four-slot", "two-slot"])
def halo_arm(request):
    """Both weight rings of the LDS-halo conv (library policy `conv_halo`)."""
    _dev()
    _set_halo_arm(request.param)
    yield request.param
    _set_halo_arm(1)


def _bits(t):
    return t.view(torch.int16)


class _HaloBuffers:
    """Device operands of one case in the forms the network never guarantees to be tight: the source is the column slice [64, 64 + Cin)
    of a buffer with row stride Cin + 128 and 2 W guard rows before the first and after the last frame, everything outside the
    frames' slice bf16 NaN (a kernel may load such memory, but none of it may reach a result, not even as 0 * NaN); the residual is
    a column slice of a wider buffer."""

    def __init__(self, case, o):
        from ccedit_amd.packing import pack_weight
        n, cin, cout, h, w = case
        self.case, self.o, self.rows, self.guard = case, o, n * h * w, 2 * w
        self.pw = pack_weight(o.w, o.b).to("cuda")
        self.src = torch.full((self.rows + 2 * self.guard, cin + 128), float("nan"), dtype=BF, device="cuda")
        self.src[self.guard:self.guard + self.rows, 64:64 + cin] = _flat(o.x)
        self.x = self.src[self.guard:self.guard + self.rows, 64:64 + cin].view(n, h, w, cin)
        flat = self.x.reshape(-1, cin)
        assert flat.data_ptr() == self.x.data_ptr() and flat.stride(0) == cin + 128       # the launch sees the slice, not a copy
        self.res_wide = torch.full((self.rows, cout + 128), 7.0, dtype=BF, device="cuda")
        self.res_wide[:, 64:64 + cout] = _flat(o.r1)
        self.res = self.res_wide[:, 64:64 + cout]
        self.src0, self.res0 = self.src.clone(), self.res_wide.clone()
        self.kw = dict(group_bias=_f32(o.gb), group_rows=h * w, res1=self.res, gn=True)

    def launch(self, tile=8, **kw):
        from ccedit_amd import ops
        return ops.conv2d(self.x, self.pw, tile=tile, **self.kw, **kw)

    def unchanged(self):
        assert torch.equal(_bits(self.src), _bits(self.src0)), "the source buffer was written"
        assert torch.equal(_bits(self.res_wide), _bits(self.res0)), "the residual buffer was written"


def _halo_first_launch(bufs, arm, tile=8):
    """Contiguous output, row bias + residual, gn=True: equal to the reference, the arm's label; statistics where the producer fuses
    them (Cout >= 256, frames of whole 128-pixel blocks): equal to the float64 group sums, three launches alike."""
    from ccedit_amd import ops
    n, cin, cout, h, w = bufs.case
    what = f"halo conv {n} x {cin}->{cout} {h}x{w}, {HALO_LABEL[arm]}"
    y = bufs.launch(tile)
    assert _last() == HALO_LABEL[arm], _last()
    _equal(_nchw(y), bufs.o.ref, what)
    st = None
    if cout >= 256 and (h * w) % 128 == 0:
        st = _stats_equal(y, h * w, what)
        for _ in range(2):
            y2 = bufs.launch(tile)
            assert torch.equal(y2, y) and torch.equal(ops.gn_stats_of(y2, h * w), st), f"{what}: run-to-run difference"
    else:
        assert ops.gn_stats_of(y, h * w) is None
    return y, st


@pytest.mark.parametrize("case", HALO_CASES, ids=lambda c: "{}x{}-{}-{}x{}".format(*c))
def test_conv_halo_chunks(halo_arm, case):
    """conv_halo4_kernel / conv_halo_kernel where their machinery is (HALO_CASES), on operands that observe every K column in every
    16-channel block: strided NaN-guarded source, strided residual; a contiguous launch with statistics, then a launch into a column
    slice of a wider, longer buffer holding the bit pattern 0x5A5A, which must survive everywhere outside the slice."""
    _dev()
    n, cin, cout, h, w = case
    bufs = _HaloBuffers(case, _halo_operands(case))
    _halo_first_launch(bufs, halo_arm)
    guard = 2 * w
    big = torch.full((bufs.rows + 2 * guard, cout + 128), 0x5A5A, dtype=torch.int16, device="cuda").view(BF)
    bufs.launch(out=big[guard:guard + bufs.rows, 64:64 + cout])
    assert _last() == HALO_LABEL[halo_arm], _last()
    _equal(_nchw(big[guard:guard + bufs.rows, 64:64 + cout].reshape(n, h, w, cout)), bufs.o.ref, "halo conv into a column slice")
    outside = _bits(big).clone()
    outside[guard:guard + bufs.rows, 64:64 + cout] = 0x5A5A
    assert bool((outside == 0x5A5A).all()), "elements outside the output slice were written"
    bufs.unchanged()


def test_conv_halo_automatic_dispatch(halo_arm):
    """320 -> 640 at 16 x 24 without a forced tile: the same kernel, the same bits."""
    _dev()
    case = HALO_CASES[2]
    bufs = _HaloBuffers(case, _halo_operands(case))
    _halo_first_launch(bufs, halo_arm, tile=0)
    bufs.unchanged()


@pytest.mark.parametrize("case", HALO_CASES, ids=lambda c: "{}x{}-{}-{}x{}".format(*c))
def test_conv_halo_arms_agree(case):
    """The documented claim of csrc/convhalo.hip: the two-slot kernel gives bit-identical results (same k-step order) — outputs and
    statistics of the two arms against each other."""
    _dev()
    bufs = _HaloBuffers(case, _halo_operands(case))
    try:
        got = {}
        for arm in (1, 2):
            _set_halo_arm(arm)
            got[arm] = _halo_first_launch(bufs, arm)
    finally:
        _set_halo_arm(1)
    assert torch.equal(got[1][0], got[2][0]), "the two weight rings wrote different outputs"
    assert (got[1][1] is None) == (got[2][1] is None)
    assert got[1][1] is None or torch.equal(got[1][1], got[2][1]), "the two weight rings left different statistics"


# ------------------------------------------------------------------------------------------ g8 (tiles 11-13)
@pytest.mark.parametrize("tile", [11, 12, 13])
@pytest.mark.parametrize("nres", [0, 1, 2])
def test_g8_linear(nres, tile):
    """The persistent eight-phase kernel on 513 x 656 <- 704: ragged M and N tiles, an odd number of K tiles, all residual epilogues;
    with row_sums the LayerNorm sums it leaves for the consumer equal the float64 row sums of what it wrote, three launches alike."""
    _dev()
    from ccedit_amd import ops
    from ccedit_amd.packing import pack_weight
    m, n, k = 513, 656, 704
    o = E.operands((m, k), (n, k), F.linear, seed=nres, nres=nres)
    pw, xd = pack_weight(o.w, o.b).to("cuda"), _rows(o.x)
    kw = dict(res1=_rows(o.r1), res2=_rows(o.r2), tile=tile)
    y = ops.linear(xd, pw, **kw)
    assert (G8[12] if tile == 11 else G8[tile]) in _last(), _last()
    _equal(y, o.ref, f"g8 linear, {nres} residuals, tile {tile}")
    sums = torch.stack([o.ref.sum(dim=1), (o.ref * o.ref).sum(dim=1)], dim=1)
    for _ in range(3):
        y2 = ops.linear(xd, pw, row_sums=True, **kw)
        assert "g8_kernel" in _last(), _last()
        _equal(y2, o.ref, "g8 linear with row_sums")
        _equal(ops.ln_sums_of(y2), sums, "g8 row_sums")


@pytest.mark.parametrize("tile", [12, 13])
def test_g8_linear_row_bias_and_statistics(tile):
    """Linear + per-frame row bias + residual + fused GroupNorm statistics (gn_rows): 3 frames of 512 rows onto 640 channels."""
    _dev()
    from ccedit_amd import ops
    from ccedit_amd.packing import pack_weight
    nfr, hw, k, cout = 3, 512, 256, 640
    o = E.operands((nfr * hw, k), (cout, k), F.linear, seed=tile, rows_per_bias=hw, nres=1)
    pw, xd = pack_weight(o.w, o.b).to("cuda"), _rows(o.x)
    kw = dict(group_bias=_f32(o.gb), group_rows=hw, res1=_rows(o.r1), gn_rows=hw, tile=tile)
    st = None
    for _ in range(3):
        y = ops.linear(xd, pw, **kw)
        assert G8[tile] in _last(), _last()
        _equal(y, o.ref, f"g8 linear + row bias tile {tile}")
        s = _stats_equal(y, hw, "g8 linear")
        assert st is None or torch.equal(s, st), "g8 linear statistics: run-to-run difference"
        st = s


@pytest.mark.parametrize("tile", [12, 13])
@pytest.mark.parametrize("n,cin,cout,h,w", [(5, 64, 384, 12, 16), (3, 64, 256, 8, 16), (3, 192, 384, 12, 16), (3, 128, 256, 8, 16)])
def test_g8_conv3x3(n, cin, cout, h, w, tile):
    """g8_kernel's nine-tap gather: zeros outside the frame, also between the frames of the batch; row bias + residual; at 8 x 16 (whole
    128-pixel blocks, a 256-pixel tile holds two frames) the fused statistics.  Cin = 192 (27 K tiles: an odd count) and 128: the K
    order past chunk 0 with every K column observed in every 16-channel block, and one launch on the plain epilogue."""
    _dev()
    from ccedit_amd import ops
    from ccedit_amd.packing import pack_weight
    o = E.operands((n, cin, h, w), (cout, cin, 3, 3), lambda x, wt, b: F.conv2d(x, wt, b, padding=1), seed=n + tile, frames_per_bias=1, nres=1,
                   rows_per_tile=16 if cin > 64 else 0)
    pw, xd = pack_weight(o.w, o.b).to("cuda"), _nhwc(o.x)
    with_stats = (h * w) % 128 == 0 and cout >= 256
    kw = dict(group_bias=_f32(o.gb), group_rows=h * w, res1=_flat(o.r1), gn=with_stats, tile=tile)
    st = None
    for _ in range(3):
        y = ops.conv2d(xd, pw, **kw)
        assert G8[tile] + ", 3x3 taps" in _last(), _last()
        _equal(_nchw(y), o.ref, f"g8 conv3x3 {n}x{h}x{w} tile {tile}")
        if with_stats:
            s = _stats_equal(y, h * w, "g8 conv3x3")
            assert st is None or torch.equal(s, st), "g8 conv statistics: run-to-run difference"
            st = s
    if cin > 64:
        y = ops.conv2d(xd, pw, tile=tile)
        assert G8[tile] + ", 3x3 taps" in _last(), _last()
        _equal(_nchw(y), o.ref - o.r1 - o.gb[:, :, None, None], f"g8 conv3x3 {n}x{h}x{w} tile {tile}, plain epilogue")


@pytest.mark.parametrize("tile", [12, 13])
def test_g8_temporal_with_statistics(tile):
    """g8_kernel's temporal gather on (1, 5, 64 -> 256, 16 x 32): row bias, two residuals and the fused statistics."""
    _dev()
    from ccedit_amd import ops
    from ccedit_amd.packing import pack_weight
    b_, t, c, cout, h, w = 1, 5, 64, 256, 16, 32
    o = E.operands((b_ * t, c, h, w), (cout, c, 3), E.temporal_ref(b_, t), seed=tile, frames_per_bias=t)
    pw, xd = pack_weight(o.w, o.b).to("cuda"), _nhwc(o.x)
    kw = dict(group_bias=_f32(o.gb), group_rows=t * h * w, res1=_flat(o.r1), res2=_flat(o.r2), gn=True, tile=tile)
    st = None
    for _ in range(3):
        y = ops.conv_temporal(xd, t, pw, **kw)
        assert G8[tile] + ", temporal taps" in _last(), _last()
        _equal(_nchw(y), o.ref, f"g8 temporal tile {tile}")
        s = _stats_equal(y, h * w, "g8 temporal")
        assert st is None or torch.equal(s, st), "g8 temporal statistics: run-to-run difference"
        st = s


@pytest.mark.parametrize("tile,cin", [pytest.param(t, 64, id=str(t)) for t in (1, 12, 13)]
                         + [pytest.param(t, 128, id=f"{t}-c128") for t in (1, 12, 13)])
def test_upsample_parity_convs(tile, cin):
    """conv3x3(nearest 2x(x)) as four 2 x 2 parity convs (conv2d_upsampled) on one odd 5 x 7 frame: the merged taps are sums of up to
    four weights in {-1, 0, 1} — integers, so the parity form equals the nine-tap float64 reference exactly.  Cin = 128: two chunks,
    every K column of the nine-tap weight observed in every 16-channel block."""
    _dev()
    from ccedit_amd import ops
    from ccedit_amd.packing import pack_upsample_parities
    n, h, w, cout = 1, 5, 7, 64
    o = E.operands((n, cin, h, w), (cout, cin, 3, 3),
                   lambda x, wt, b: F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), wt, b, padding=1), seed=tile, nres=0,
                   rows_per_tile=16 if cin > 64 else 0)
    y = ops.conv2d_upsampled(_nhwc(o.x), pack_upsample_parities(o.w, o.b, device="cuda"), tile=tile)
    assert (G8[tile] + ", upsample parity taps" if tile >= 12 else TAP[tile]) in _last(), _last()
    _equal(_nchw(y), o.ref, f"parity convs tile {tile}")


def test_g8_split_k():
    """Split-K with the workspace lent (automatic dispatch): partial accumulators through fp32 scratch, the last arriver reduces.
    Linear 3264 x 1280 <- 5120 + residual; Conv2d 3x3 1280 -> 1280 on 5 frames of 8 x 12 (odd tile count, ragged last tile) + row
    bias + residual; Conv1d k3 over T 1280 -> 1280, two clips of three 8 x 16 frames, two residuals and statistics."""
    _dev()
    from ccedit_amd import ops
    from ccedit_amd.packing import pack_weight
    m, n, k = 3264, 1280, 5120
    o = E.operands((m, k), (n, k), F.linear, seed=1, nres=1)
    pw, xd, rd = pack_weight(o.w, o.b).to("cuda"), _rows(o.x), _rows(o.r1)
    for _ in range(3):
        y = ops.linear(xd, pw, res1=rd)
        assert "split-K" in _last(), _last()
        _equal(y, o.ref, "split-K linear")
    nfr, c, h, w = 5, 1280, 8, 12
    o = E.operands((nfr, c, h, w), (c, c, 3, 3), lambda x, wt, b: F.conv2d(x, wt, b, padding=1), seed=2, frames_per_bias=1, nres=1)
    y = ops.conv2d(_nhwc(o.x), pack_weight(o.w, o.b).to("cuda"), group_bias=_f32(o.gb), group_rows=h * w, res1=_flat(o.r1))
    assert "split-K" in _last() and "3x3" in _last(), _last()
    _equal(_nchw(y), o.ref, "split-K conv3x3")
    b_, t, h, w = 2, 3, 8, 16
    o = E.operands((b_ * t, c, h, w), (c, c, 3), E.temporal_ref(b_, t), seed=3)
    pw, xd = pack_weight(o.w, o.b).to("cuda"), _nhwc(o.x)
    st = None
    for _ in range(3):
        y = ops.conv_temporal(xd, t, pw, res1=_flat(o.r1), res2=_flat(o.r2), gn=True)
        assert "split-K" in _last() and "temporal" in _last(), _last()
        _equal(_nchw(y), o.ref, "split-K temporal conv")
        s = _stats_equal(y, h * w, "split-K temporal")
        assert st is None or torch.equal(s, st), "split-K statistics: run-to-run difference"
        st = s


# ------------------------------------------------------------------------------------------ register-resident weights
@pytest.mark.parametrize("n,m", [(n, m) for n in (320, 960) for m in (32, 130, 1000)] + [(1280, 16384)])
def test_lin320(m, n):
    """tile 9: lin320_kernel (two K halves combined across wave sets; ragged M) and, for whole 32-pixel tiles, lin320s_kernel; plain,
    and with a residual on strided operands.  16384 x 1280: a workgroup walks 8 tiles, more than lin320s_kernel's seven ring slots."""
    _dev()
    from ccedit_amd import ops
    from ccedit_amd.packing import pack_weight
    k = 320
    o = E.operands((m, k), (n, k), F.linear, seed=m + n, nres=1)
    pw, xd = pack_weight(o.w, o.b).to("cuda"), _rows(o.x)
    want = "lin320s_kernel" if m % 32 == 0 else "lin320_kernel"
    y = ops.linear(xd, pw, tile=9)
    assert want in _last(), _last()
    _equal(y, o.ref - o.r1, f"lin320 {m}x{n}")
    wide = torch.full((m, 2 * n), 7.0, dtype=BF, device="cuda")
    ops.linear(_strided(xd), pw, res1=_strided(_rows(o.r1)), out=wide[:, n:], tile=9)
    assert want in _last(), _last()
    _equal(wide[:, n:], o.ref, f"lin320 {m}x{n} + residual, strided")
    assert bool((wide[:, :n] == 7.0).all()), "columns outside the output slice were written"


@pytest.mark.parametrize("m,n", [(16, 640), (2064, 1920), (4096, 1920)])
def test_lin640s(m, n):
    """tile 10: lin640s_kernel — one tile / ragged XCD ranges, the last 256-channel slice half empty / 8 tiles per workgroup (rings of
    five and six slots wrap); residual from a strided matrix, and the LayerNorm row sums of what it wrote (row_sums), three launches
    alike."""
    _dev()
    from ccedit_amd import ops
    from ccedit_amd.packing import pack_weight
    k = 640
    o = E.operands((m, k), (n, k), F.linear, seed=m, nres=1)
    pw, xd, rd = pack_weight(o.w, o.b).to("cuda"), _rows(o.x), _strided(_rows(o.r1))
    y = ops.linear(xd, pw, tile=10)
    assert "lin640s_kernel" in _last(), _last()
    _equal(y, o.ref - o.r1, f"lin640s {m}x{n}")
    sums = torch.stack([o.ref.sum(dim=1), (o.ref * o.ref).sum(dim=1)], dim=1)
    for _ in range(3):
        y = ops.linear(xd, pw, res1=rd, row_sums=True, tile=10)
        assert "lin640s_kernel" in _last(), _last()
        _equal(y, o.ref, f"lin640s {m}x{n} + residual")
        _equal(ops.ln_sums_of(y), sums, "lin640s row_sums")


@pytest.mark.parametrize("b_,t,cout,h,w", [(2, 5, 320, 8, 16), (3, 3, 64, 4, 4), (2, 4, 1280, 24, 24)])
def test_temp320s(b_, t, cout, h, w):
    """tile 14: temp320s_kernel — three rolling accumulators per pixel column, the missing MFMA at the clip ends and between clips,
    128-channel slices (320 = 128 + 128 + 64), row bias + two residuals, statistics with 10-channel groups across the lanes' quads.
    2 x 4 x 24 x 24 -> 1280: a workgroup walks 3 columns = 12 steps, more than the rings of six and nine slots hold."""
    _dev()
    from ccedit_amd import ops
    from ccedit_amd.packing import pack_weight
    c = 320
    o = E.operands((b_ * t, c, h, w), (cout, c, 3), E.temporal_ref(b_, t), seed=cout, frames_per_bias=t)
    pw, xd = pack_weight(o.w, o.b).to("cuda"), _nhwc(o.x)
    with_stats = cout >= 320 and (h * w) % 128 == 0
    kw = dict(group_bias=_f32(o.gb), group_rows=t * h * w, res1=_flat(o.r1), res2=_flat(o.r2), gn=with_stats, tile=14)
    st = None
    for _ in range(3):
        y = ops.conv_temporal(xd, t, pw, **kw)
        assert "temp320s_kernel" in _last(), _last()
        _equal(_nchw(y), o.ref, f"temp320s T={t} -> {cout}")
        if with_stats:
            s = _stats_equal(y, h * w, "temp320s")
            assert st is None or torch.equal(s, st), "temp320s statistics: run-to-run difference"
            st = s
    y = ops.conv_temporal(xd, t, pw, tile=14)
    assert "temp320s_kernel" in _last(), _last()
    _equal(_nchw(y), o.ref - o.r1 - o.r2 - o.gb.repeat_interleave(t, 0)[:, :, None, None], "temp320s plain")


@pytest.mark.parametrize("cin,cout,stride", [(32, 32, 1), (8, 4, 1), (16, 32, 2)])
def test_small_conv(cin, cout, stride):
    """small_conv3x3_kernel, reached by automatic dispatch from 65 536 output pixels (200 x 328 frames: a ragged last 32-pixel group);
    act = 0 only — the activations are not exact by nature."""
    _dev()
    from ccedit_amd import ops
    from ccedit_amd.packing import pack_weight
    n, h, w = 2, 200, 328
    if stride == 2:
        h, w = 2 * h, 2 * w - 2
    o = E.operands((n, cin, h, w), (cout, cin, 3, 3), lambda x, wt, b: F.conv2d(x, wt, b, stride=stride, padding=1), seed=cin, nres=0)
    y = ops.conv2d(_nhwc(o.x), pack_weight(o.w, o.b).to("cuda"), stride=stride)
    assert "small_conv3x3_kernel" in _last(), _last()
    _equal(_nchw(y)[:, :cout], o.ref, f"small conv {cin}->{cout} stride {stride}")


# ------------------------------------------------------------------------------------------ fp32 VAE kernels, both arms
@pytest.fixture(params=[1, 0], ids=["six-bf16-products", "mfma-f32"])
def arm(request):
    """Both realisations of ccedit_gemm_f32 (library policy `f32_split`)."""
    _dev()
    from ccedit_amd import hip
    assert hip.lib().ccedit_policy_set(b"f32_split", request.param) == 0
    yield request.param
    hip.lib().ccedit_policy_set(b"f32_split", 1)


def _f32_label(arm):
    return "six bf16 products" if arm else "f32_gemm_kernel"


# x up to 2^10 and weights up to 300 (more than 8 significant bits each: the hi / mid parts of both operands of the six-product arm
# carry value); ~48 products of <= 2^10 * 300 per output keep sum |x| |w| and the residual below 2^24
_F32 = dict(xmax=1024, wmax=300, bmax=1 << 16, rmax=1 << 16, out_max=E.F32_EXACT)


@pytest.mark.parametrize("m,cin,n,res", [(1000, 512, 512, True), (77, 20, 3, False), (130, 4, 4, True)])
def test_gemm_f32_linear(arm, m, cin, n, res):
    dev = _dev()
    from ccedit_amd import vae_f32 as V
    o = E.operands((m, cin), (n, cin), F.linear, seed=m, nres=int(res), **_F32)
    pw = V.pack_f32(o.w.float(), o.b.float(), dev)
    ldc = (n + 3) // 4 * 4
    out = torch.full((m, ldc), 7.0, device=dev)
    V.gemm_f32(o.x.float().to(dev), pw, res=_f32(o.r1), out=out)
    assert _f32_label(arm) in _last(), _last()
    _equal(out[:, :n], o.ref, f"gemm_f32 {m}x{n}<-{cin}")
    assert bool((out[:, n:] == 7.0).all()), "columns beyond N were written"


@pytest.mark.parametrize("cin,cout,h,w,kind", [(4, 128, 9, 13, "s1"), (64, 128, 7, 9, "up"), (128, 128, 13, 11, "down")])
def test_conv_f32(arm, cin, cout, h, w, kind):
    dev = _dev()
    from ccedit_amd import vae_f32 as V
    n = 3
    fwd = {"s1": lambda x, wt, b: F.conv2d(x, wt, b, padding=1),
           "up": lambda x, wt, b: F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), wt, b, padding=1),
           "down": lambda x, wt, b: F.conv2d(F.pad(x, (0, 1, 0, 1)), wt, b, stride=2)}[kind]
    o = E.operands((n, cin, h, w), (cout, cin, 3, 3), fwd, seed=h, nres=int(kind == "s1"), **_F32)
    xl = o.x.float().permute(0, 2, 3, 1).contiguous().to(dev)
    pw = V.pack_f32(o.w.float(), o.b.float(), dev)
    if kind == "s1":
        got = V.conv2d_f32(xl, pw, res=o.r1.float().permute(0, 2, 3, 1).contiguous().to(dev))
    elif kind == "up":
        got = V.conv2d_f32(xl, pw, upsample=True)
    else:
        got = V.conv2d_f32(xl, pw, stride=2, pad=0, out_hw=((h + 1 - 3) // 2 + 1, (w + 1 - 3) // 2 + 1))
    assert _f32_label(arm) in _last() and "3x3 taps" in _last(), _last()
    _equal(_nchw(got), o.ref, f"conv_f32 {kind} {cin}->{cout}")


def test_upsample_conv_f32_parity_form(arm):
    """The four parity convs with merged taps on the six-product kernels; on the fp32 matrix instruction the product runs the
    nine-tap gather instead.  Merged weights are sums of up to four integers: still exact."""
    dev = _dev()
    from ccedit_amd import vae_f32 as V
    cin, cout, n, h, w = 64, 128, 2, 7, 9
    o = E.operands((n, cin, h, w), (cout, cin, 3, 3),
                   lambda x, wt, b: F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), wt, b, padding=1), seed=7, nres=0,
                   **dict(_F32, wmax=75))                       # a merged tap sums four weights
    xl = o.x.float().permute(0, 2, 3, 1).contiguous().to(dev)
    if arm:
        got = torch.empty((n, 2 * h, 2 * w, cout), dtype=torch.float32, device=dev)
        for p, pw in enumerate(V.pack_f32_parities(o.w.float(), o.b.float(), dev)):
            V.gemm_f32(xl.reshape(-1, cin), pw, m=n * h * w, conv=(h, w, h, w, 1, 1, 2 + p), out=got.view(-1, cout))
            assert "upsample parity taps, six bf16 products" in _last(), _last()
    else:
        got = V.conv2d_f32(xl, V.pack_f32(o.w.float(), o.b.float(), dev), upsample=True)
        assert "f32_gemm_kernel" in _last(), _last()
    _equal(_nchw(got), o.ref, "upsample + conv f32")


# ------------------------------------------------------------------------------------------ statistics
@pytest.mark.parametrize("tile", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("cout", [320, 256])
def test_tap_gemm_fused_statistics(tile, cout):
    """CcGemmDesc.gn_stats from tap_gemm's conv, Linear and temporal producers (3 frames of 16 x 32; tile 1 also 16 x 24 = 384 pixels,
    the only block shape that may hold whole 128-pixel blocks): float64 sums of the values written, three launches alike."""
    _dev()
    from ccedit_amd import ops
    from ccedit_amd.packing import pack_weight
    n, cin, h, w = 3, 64, 16, 32
    conv = lambda x, wt, b: F.conv2d(x, wt, b, padding=1)
    o = E.operands((n, cin, h, w), (cout, cin, 3, 3), conv, seed=tile, frames_per_bias=1, nres=1)
    pw, xd = pack_weight(o.w, o.b).to("cuda"), _nhwc(o.x)
    ol = E.operands((n * h * w, 128), (cout, 128), F.linear, seed=tile + 10, nres=0)
    pwl, xl = pack_weight(ol.w, ol.b).to("cuda"), _rows(ol.x)
    ot = E.operands((n, 128, h, w), (cout, 128, 3), E.temporal_ref(1, n), seed=tile + 20, nres=0)
    pwt, xt = pack_weight(ot.w, ot.b).to("cuda"), _nhwc(ot.x)
    first = {}
    for _ in range(3):
        y = ops.conv2d(xd, pw, group_bias=_f32(o.gb), group_rows=h * w, res1=_flat(o.r1), gn=True, tile=tile)
        assert TAP[tile] in _last(), _last()
        _equal(_nchw(y), o.ref, "conv")
        z = ops.linear(xl, pwl, gn_rows=h * w, tile=tile)
        assert TAP[tile] in _last(), _last()
        _equal(z, ol.ref, "linear")
        zt = ops.conv_temporal(xt, n, pwt, gn=True, tile=tile)
        assert TAP[tile] in _last(), _last()
        _equal(_nchw(zt), ot.ref, "temporal")
        for name, t_ in (("conv", y), ("linear", z), ("temporal", zt)):
            s = _stats_equal(t_, h * w, f"tap_gemm {name} producer, tile {tile}")
            assert torch.equal(first.setdefault(name, s), s), f"{name} statistics: run-to-run difference"
    if tile == 1:
        o3 = E.operands((2, cin, 16, 24), (cout, cin, 3, 3), conv, seed=31, nres=0)
        y3 = ops.conv2d(_nhwc(o3.x), pack_weight(o3.w, o3.b).to("cuda"), gn=True, tile=1)
        assert TAP[1] in _last(), _last()
        _equal(_nchw(y3), o3.ref, "conv 16x24")
        _stats_equal(y3, 384, "tap_gemm conv producer, 384-pixel frames")


@pytest.mark.parametrize("c1,c2", [(32, 32), (64, 32), (640, 320)])
def test_cat_add_statistics(c1, c2):
    """cat_add(gn=True): a ++ (b + c) and the statistics of the result, on ragged 12 x 9 frames."""
    _dev()
    from ccedit_amd import ops
    n, h, w = 3, 12, 9
    g = E.gen(c1)
    a, b, c = E.ints((n, h, w, c1), -32, 32, g), E.ints((n, h, w, c2), -16, 16, g), E.ints((n, h, w, c2), -16, 16, g)
    ref = torch.cat([a, b + c], dim=-1)
    st = None
    for _ in range(3):
        y = ops.cat_add(_rows(a), _rows(b), _rows(c), gn=True)
        _equal(y, ref, f"cat_add {c1}+{c2}")
        s = _stats_equal(y, h * w, "cat_add")
        assert st is None or torch.equal(s, st), "cat_add statistics: run-to-run difference"
        st = s


@pytest.mark.parametrize("n,h,w,c", [(3, 5, 7, 64), (2, 4, 6, 2560), (2, 33, 17, 320)])
def test_groupnorm_spatial_stats(n, h, w, c):
    """groupnorm_spatial_stats: ragged pixel counts (35, 561: a partly filled last block), the widest tensor of the network."""
    _dev()
    from ccedit_amd import ops
    x = E.ints((n, h, w, c), -64, 64, E.gen(c))
    ref = E.group_sums(x)
    xd = _rows(x)
    for _ in range(3):
        _equal(ops.groupnorm_spatial_stats(xd), ref, f"groupnorm_spatial_stats {h}x{w}x{c}")


@pytest.mark.parametrize("b_,t,c", [(2, 17, 320), (2, 3, 1280), (3, 4, 160)])
def test_groupnorm_temporal_stats(b_, t, c):
    """groupnorm_temporal_stats accumulates in fp32: sums over T frames x C / 32 channels of |x| <= 64 stay below 17 * 40 * 64^2 =
    2.8 M < 2^24, so they are exact too."""
    _dev()
    from ccedit_amd import ops
    h, w = 3, 5
    x = E.ints((b_ * t, h, w, c), -64, 64, E.gen(t))
    xf = x.reshape(b_, t, h * w, 32, c // 32)
    ref = torch.stack([xf.sum(dim=(1, 4)), (xf * xf).sum(dim=(1, 4))], dim=-1).reshape(b_ * h * w, 32, 2)
    assert ref[..., 1].max().item() < E.F32_EXACT
    xd = _rows(x)
    for _ in range(3):
        _equal(ops.groupnorm_temporal_stats(xd, b_, t), ref, f"groupnorm_temporal_stats T={t} C={c}")


# ------------------------------------------------------------------------------------------ cancellation
def _cancel(m, n, k, call, want, what):
    o = E.cancellation(m, n, k, cols=(0, n // 2 + 1, n - 1), seed=k)
    from ccedit_amd.packing import pack_weight
    y = call(_rows(o.x), pack_weight(o.w).to("cuda"))
    assert want in _last(), _last()
    _equal(y, o.ref, f"{what}: +4096 + {o.ones} ones - 4096")


@pytest.mark.parametrize("family,m,n,k,tile,want", [
    ("tap_gemm K=64 tiles", 150, 320, 256, 1, TAP[1]), ("tap_gemm K=32 tiles", 150, 320, 256, 6, TAP[6]),
    ("g8 256x256", 300, 320, 256, 12, G8[12]), ("g8 128x512", 300, 320, 256, 13, G8[13]),
    ("lin320 (K halves combined)", 130, 320, 320, 9, "lin320_kernel"), ("lin320s", 128, 320, 320, 9, "lin320s_kernel"),
    ("lin640s", 48, 640, 640, 10, "lin640s_kernel"), ("g8 split-K", 300, 1280, 5120, 0, "split-K")])
def test_cancellation_needs_fp32_intermediates(family, m, n, k, tile, want):
    """One Linear per family with output columns whose first K element contributes +2^12, the last -2^12 and up to 256 in between +1
    each: exact only if every intermediate is fp32.  At the split-K shape the two large terms fall into different splits."""
    _dev()
    from ccedit_amd import ops
    _cancel(m, n, k, lambda x, pw: ops.linear(x, pw, tile=tile), want, family)
