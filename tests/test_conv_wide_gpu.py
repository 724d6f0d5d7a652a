"""The 256-pixel (16 x 16) tile of the LDS-halo 3x3 conv (csrc/convhalo.hip: conv_halo4_kernel<2, 2, 2, 4>, block shape 15, library policy
`conv_wide`) on exact integers: equal to the float64 reference and BIT-equal to the 128-pixel tile (block shape 8, `conv_halo` = 1).

Operands are those of tests/_exact_ints.py with a non-zero in every K column inside every block of 16 output rows; the buffers are the forms
of tests/test_exact_gpu.py's halo cases (helpers copied from there): a NaN-guarded strided source, a strided residual, and an output slice
inside a buffer filled with the bit pattern 0x5A5A.  What the wide tile changes against the 128-pixel one, and the case that reaches it:
one halo buffer restaged at every chunk boundary behind an extra barrier (Cin > 64), 11 halo issues recomputed per chunk with 32-bit
offsets from the frame's first element (frames > 1), a two-chunk epilogue with one wave column staged at a time, statistics that add up over
both chunks, the narrow last channel tile, the ragged last tile column."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _exact_ints as E  # noqa: E402

pytestmark = pytest.mark.gpu

BF = torch.bfloat16

# (frames, Cin, Cout, H, W)
WIDE_CASES = [
    (1, 64, 64, 16, 16),      # a narrow tile alone; one chunk; all four borders in one tile
    (2, 128, 128, 16, 32),    # the halo buffer restaged once; two tiles side by side
    (2, 192, 320, 32, 16),    # three chunks; two tile rows; channel tiles 128 + 128 + 64; statistics
    (9, 128, 256, 16, 16),    # nine pixel tiles on eight XCDs: pt_per_xcd = 2, workgroups that return early
    (2, 128, 960, 16, 16),    # eight channel tiles in groups 3 + 3 + 2, the last one narrow; statistics
    (2, 128, 256, 16, 24),    # the second tile column ragged (8 of 16)
]
WIDE_LABEL = "conv_halo_kernel, four-slot weight ring, 256-pixel tile"
NARROW_LABEL = "conv_halo_kernel, four-slot weight ring"
_cache = {}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _last():
    from ccedit_amd import hip
    return hip.lib().ccedit_last_kernel().decode()


def _set(name, value):
    from ccedit_amd import hip
    assert hip.lib().ccedit_policy_set(name, value) == 0


@pytest.fixture(autouse=True)
def _policy():
    """Every test starts from and leaves the library defaults of the two switches it touches."""
    _dev()
    _set(b"conv_halo", 1)
    _set(b"conv_wide", 1)
    yield
    _set(b"conv_halo", 1)
    _set(b"conv_wide", 1)


def _f32(t):
    return None if t is None else t.float().cuda()


def _flat(t):      # float64 (N, C, H, W) -> bf16 cuda [N*H*W][C]
    return t.permute(0, 2, 3, 1).contiguous().to(BF).cuda().reshape(-1, t.shape[1])


def _nchw(y):
    return y.double().cpu().permute(0, 3, 1, 2).contiguous()


def _bits(t):
    return t.view(torch.int16)


def _equal(got, ref, what):
    got = got.double().cpu()
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    if not torch.equal(got, ref):
        bad = (got != ref).nonzero()
        first = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {bad.shape[0]} of {ref.numel()} values differ from the integer reference; first at {first}: "
                             f"got {got[first].item()} want {ref[first].item()}; max |diff| {(got - ref).abs().max().item()}")


def _operands(case):
    """Operands and float64 reference of one case: computed once, shared by the tests below, never modified."""
    if case not in _cache:
        n, cin, cout, h, w = case
        _cache[case] = E.operands((n, cin, h, w), (cout, cin, 3, 3), lambda x, wt, b: F.conv2d(x, wt, b, padding=1), seed=cout + w,
                                  frames_per_bias=1, nres=1, rows_per_tile=16)
    return _cache[case]


class _Buffers:
    """Device operands of one case in the forms the network never guarantees to be tight: the source is the column slice [64, 64 + Cin)
    of a buffer with row stride Cin + 128 and 2 W guard rows before the first and after the last frame, everything outside the
    frames' slice bf16 NaN (a kernel may load such memory, but none of it may reach a result, not even as 0 * NaN); the residual is
    a column slice of a wider buffer."""

    def __init__(self, case):
        from ccedit_amd.packing import pack_weight
        o = _operands(case)
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

    def launch(self, tile, **kw):
        from ccedit_amd import ops
        return ops.conv2d(self.x, self.pw, tile=tile, **self.kw, **kw)

    def unchanged(self):
        assert torch.equal(_bits(self.src), _bits(self.src0)), "the source buffer was written"
        assert torch.equal(_bits(self.res_wide), _bits(self.res0)), "the residual buffer was written"


def _first_launch(bufs, tile, label):
    """Contiguous output, row bias + residual, gn=True: equal to the reference, the expected label; statistics where the producer fuses
    them (Cout >= 256, frames of whole 128-pixel blocks): equal to the float64 group sums, three launches alike."""
    from ccedit_amd import ops
    n, cin, cout, h, w = bufs.case
    what = f"halo conv {n} x {cin}->{cout} {h}x{w}, {label}"
    y = bufs.launch(tile)
    assert _last() == label, _last()
    _equal(_nchw(y), bufs.o.ref, what)
    st = None
    if cout >= 256 and (h * w) % 128 == 0:
        st = ops.gn_stats_of(y, h * w)
        assert st is not None, f"{what}: the producer left no statistics"
        _equal(st, E.group_sums(y.cpu().reshape(n, h * w, 1, cout)), f"{what}: GroupNorm statistics")
        for _ in range(2):
            y2 = bufs.launch(tile)
            assert torch.equal(y2, y) and torch.equal(ops.gn_stats_of(y2, h * w), st), f"{what}: run-to-run difference"
    else:
        assert ops.gn_stats_of(y, h * w) is None
    return y, st


@pytest.mark.parametrize("case", WIDE_CASES, ids=lambda c: "{}x{}-{}-{}x{}".format(*c))
def test_conv_wide(case):
    """Block shape 15 against the float64 reference and, bit for bit, against block shape 8 on the four-slot ring; then into a column slice
    of a wider, longer buffer holding 0x5A5A, which must survive everywhere outside the slice; the sources stay as they were."""
    n, cin, cout, h, w = case
    bufs = _Buffers(case)
    y, st = _first_launch(bufs, 15, WIDE_LABEL)
    y8, st8 = _first_launch(bufs, 8, NARROW_LABEL)
    assert torch.equal(_bits(y), _bits(y8)), "the 256-pixel tile and the 128-pixel tile wrote different bits"
    assert (st is None) == (st8 is None) and (st is None or torch.equal(st, st8)), "the two tiles left different statistics"
    if case in (WIDE_CASES[2], WIDE_CASES[4]):
        assert st is not None, "this case is here for its statistics"
    guard = 2 * w
    big = torch.full((bufs.rows + 2 * guard, cout + 128), 0x5A5A, dtype=torch.int16, device="cuda").view(BF)
    bufs.launch(15, out=big[guard:guard + bufs.rows, 64:64 + cout])
    assert _last() == WIDE_LABEL, _last()
    _equal(_nchw(big[guard:guard + bufs.rows, 64:64 + cout].reshape(n, h, w, cout)), bufs.o.ref, "256-pixel tile into a column slice")
    outside = _bits(big).clone()
    outside[guard:guard + bufs.rows, 64:64 + cout] = 0x5A5A
    assert bool((outside == 0x5A5A).all()), "elements outside the output slice were written"
    bufs.unchanged()


@pytest.mark.parametrize("case", WIDE_CASES, ids=lambda c: "{}x{}-{}-{}x{}".format(*c))
def test_conv_wide_automatic_dispatch(case):
    """Without a forced block shape: conv_wide = 1 (the default) keeps these small launches on the 128-pixel tile, conv_wide = 2 puts them
    on the 256-pixel one, conv_wide = 0 never; the same bits every time."""
    bufs = _Buffers(case)
    y1, _ = _first_launch(bufs, 0, NARROW_LABEL)
    _set(b"conv_wide", 2)
    y2, _ = _first_launch(bufs, 0, WIDE_LABEL)
    _set(b"conv_wide", 0)
    y0, _ = _first_launch(bufs, 0, NARROW_LABEL)
    assert torch.equal(_bits(y1), _bits(y2)) and torch.equal(_bits(y1), _bits(y0))
    bufs.unchanged()


def test_conv_wide_refuses_what_it_cannot_tile():
    """Block shape 15 on 8 x 16 frames (Hout % 16 != 0): refused with a message, nothing launched in its place."""
    from ccedit_amd import hip, ops
    from ccedit_amd.packing import pack_weight
    o = E.operands((1, 64, 8, 16), (64, 64, 3, 3), lambda x, wt, b: F.conv2d(x, wt, b, padding=1), seed=1, nres=0)
    x = o.x.permute(0, 2, 3, 1).contiguous().to(BF).cuda()
    with pytest.raises(Exception) as err:
        ops.conv2d(x, pack_weight(o.w, o.b).to("cuda"), tile=15)
    assert "tile 15" in str(err.value) or "tile 15" in hip.lib().ccedit_last_error().decode(), str(err.value)
