"""Why tests/test_exact_gpu.py exists, shown without a GPU: three single-element defects applied to the float64 reference.

Each mutation is one a mis-indexed kernel could make — one K element dropped from one dot product, one corner tap dropped at a
frame corner, one pixel left out of a GroupNorm group sum.  On the Gaussian operands of tests/test_ops_gpu.py every one of them
stays inside the limits that file asserts (`_close`: 2^-7 max|ref| + 1e-3; statistics: rtol 1e-4, atol 1e-2).  On the integer
operands of tests/_exact_ints.py every one of them changes the exact comparison, because every term there is a non-zero integer —
that every K column carries a weight is one of the two conditions the generator asserts.

Two more on the convolutions past one 64-channel input chunk: a K element that one channel TILE never observes (the condition
above holds over all of Cout only; `rows_per_tile` makes it hold in every block of 16 output rows), and a tap past the right edge
of a ragged rectangle column that reads the next image row instead of zero.
"""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _exact_ints as E  # noqa: E402
from test_ops_gpu import _close, _rnd  # noqa: E402      (the old limits, verbatim)


def _nonzero_term(x_col, w_col):
    """(row of x, row of w) whose product over this K element is non-zero — exists because the K column of w has a non-zero."""
    return int(x_col.ne(0).nonzero()[0]), int(w_col.ne(0).nonzero()[0])


def test_one_dropped_k_element():
    """test_linear's (257, 1280, 2560): the LAST K element of one dot product dropped (a ragged-tail mask one element short)."""
    m, n, k = 257, 1280, 2560
    x, w, b = _rnd(m, k, seed=1), _rnd(n, k, seed=2, scale=k ** -0.5), _rnd(n, seed=3)
    ref = F.linear(x, w, b)
    o = E.operands((m, k), (n, k), F.linear, seed=1, rows_per_bias=0, nres=2)
    i, j = _nonzero_term(o.x[:, k - 1], o.w[:, k - 1])
    bad = ref.clone()
    bad[i, j] -= x[i, k - 1] * w[j, k - 1]
    assert not torch.equal(bad, ref)
    _close(bad, ref, what="Gaussian operands: the dropped K element passes the tolerance")
    bad = o.ref.clone()
    bad[i, j] -= o.x[i, k - 1] * o.w[j, k - 1]
    assert not torch.equal(bad, o.ref), "integer operands: the dropped K element must change the result"


def test_one_dropped_corner_tap():
    """test_conv3x3's (320 -> 320, 16 x 24): at the top-left output pixel of a frame the tap (ky, kx) = (2, 2) — the only diagonal
    neighbour inside the frame — is dropped for one input channel (a border mask applied to the wrong corner)."""
    n, cin, cout, h, w = 3, 320, 320, 16, 24
    x = _rnd(n, cin, h, w, seed=1)
    wt, b = _rnd(cout, cin, 3, 3, seed=2, scale=(9 * cin) ** -0.5), _rnd(cout, seed=3)
    conv = lambda x_, w_, b_: F.conv2d(x_, w_, b_, padding=1)
    ref = conv(x, wt, b)
    o = E.operands((n, cin, h, w), (cout, cin, 3, 3), conv, seed=2, nres=0)
    c = 17
    f, co = _nonzero_term(o.x[:, c, 1, 1], o.w[:, c, 2, 2])
    bad = ref.clone()
    bad[f, co, 0, 0] -= x[f, c, 1, 1] * wt[co, c, 2, 2]
    assert not torch.equal(bad, ref)
    _close(bad, ref, what="Gaussian operands: the dropped corner tap passes the tolerance")
    bad = o.ref.clone()
    bad[f, co, 0, 0] -= o.x[f, c, 1, 1] * o.w[co, c, 2, 2]
    assert not torch.equal(bad, o.ref), "integer operands: the dropped corner tap must change the result"


def test_one_pixel_missing_from_a_group_sum():
    """test_gemm_fused_groupnorm_statistics' tensor (3 frames of 16 x 32, 320 channels): one value left out of one (frame, group) sum
    and sum of squares — on Gaussian data the largest one of the group with |v| <= 0.05 (one value in thirty is that small)."""
    n, cin, cout, h, w = 3, 64, 320, 16, 32
    x = _rnd(n, cin, h, w, seed=1)
    wt, b = _rnd(cout, cin, 3, 3, seed=2, scale=(9 * cin) ** -0.5), _rnd(cout, seed=3)
    res, gb = _rnd(n, cout, h, w, seed=4), _rnd(n, cout, seed=5)
    conv = lambda x_, w_, b_: F.conv2d(x_, w_, b_, padding=1)
    y = (conv(x, wt, b) + gb[:, :, None, None] + res).to(torch.bfloat16).double().permute(0, 2, 3, 1)
    yf = y.reshape(n, h * w, 32, cout // 32)
    s, q = yf.sum(dim=(1, 3)), (yf * yf).sum(dim=(1, 3))
    fr, grp = 1, 5
    cand = yf[fr, :, grp, :].abs()
    v = cand[cand <= 0.05].max()
    s_bad, q_bad = s.clone(), q.clone()
    s_bad[fr, grp] -= v
    q_bad[fr, grp] -= v * v
    assert v > 0 and not torch.equal(s_bad, s) and not torch.equal(q_bad, q)
    for atol in (1e-2, 2e-2):       # the limits of the fused-statistics tests
        assert torch.allclose(s_bad, s, rtol=1e-4, atol=atol) and torch.allclose(q_bad, q, rtol=1e-4, atol=atol)
    o = E.operands((n, cin, h, w), (cout, cin, 3, 3), conv, seed=3, frames_per_bias=1, nres=1)
    st = E.group_sums(o.ref.permute(0, 2, 3, 1))
    vals = o.ref.permute(0, 2, 3, 1).reshape(n, h * w, 32, cout // 32)[fr, :, grp, :].abs()
    vi = vals[vals > 0].min()                    # any non-zero value: an integer, at least 1
    bad = st.clone()
    bad[fr, grp, 0] -= vi
    bad[fr, grp, 1] -= vi * vi
    assert not torch.equal(bad[..., 0], st[..., 0]) and not torch.equal(bad[..., 1], st[..., 1])


def _drop_k(o, conv, rows, col):
    """The float64 reference with K element `col` (reference order: (cin, ky, kx) flattened) left out of every dot product of the
    output channels `rows`: exact, since every term is an integer."""
    only = torch.zeros_like(o.w).reshape(o.w.shape[0], -1)
    only[rows, col] = o.w.reshape(o.w.shape[0], -1)[rows, col]
    return o.ref - conv(o.x, only.reshape(o.w.shape), None)


def test_one_k_element_unobserved_in_a_channel_tile():
    """320 -> 640, 3x3: a kernel's defect lives in ONE channel tile.  On the recipe without rows_per_tile more than half of the
    (32-channel tile, K column) pairs hold no weight (one weight in every K column over ALL of Cout is all it guarantees), and a
    tile that drops such a K element from every one of its dot products still reproduces the reference bit for bit.  With
    rows_per_tile = 16 no (16-channel block, K column) pair is empty, and the same drop changes the reference at ANY column of
    ANY block: the block holds a weight there and the tap's source window holds a non-zero activation."""
    n, cin, cout, h, w = 1, 320, 640, 8, 8
    conv = lambda x_, w_, b_: F.conv2d(x_, w_, b_, padding=1)
    old = E.operands((n, cin, h, w), (cout, cin, 3, 3), conv, seed=1, frames_per_bias=1, nres=1)
    gaps = E.unobserved(old.w, 32)
    assert gaps.shape == (cout // 32, 9 * cin) and 0.5 < gaps.double().mean().item() < 0.65      # e^(-32 * 48 / 2880) = 0.587
    tile, col = gaps.nonzero()[0].tolist()
    rows = slice(32 * tile, 32 * tile + 32)
    assert torch.equal(_drop_k(old, conv, rows, col), old.ref), "old recipe: the dropped K element must go unnoticed"
    new = E.operands((n, cin, h, w), (cout, cin, 3, 3), conv, seed=1, frames_per_bias=1, nres=1, rows_per_tile=16)
    assert not bool(E.unobserved(new.w, 16).any()) and not bool(E.unobserved(new.w, 32).any())
    # a drop at (block, column) changes output (f, co, y, x) by w[co, column] * (the activation tap `column` reads there): non-zero
    # for some co of the block and some pixel — for every pair at once
    seen = (F.unfold(new.x, 3, padding=1) != 0).any(dim=2).any(dim=0)           # (Cin * 9,): same (cin, ky, kx) order as the weight
    assert seen.shape == (9 * cin,) and bool(seen.all())
    g = E.gen(7)
    pairs = [(2 * tile, col), (2 * tile + 1, col)] + [(int(torch.randint(0, cout // 16, (1,), generator=g)),
                                                      int(torch.randint(0, 9 * cin, (1,), generator=g))) for _ in range(6)]
    for blk, c in pairs:                                                        # ... and carried out: the old gap, six random pairs
        bad = _drop_k(new, conv, slice(16 * blk, 16 * blk + 16), c)
        assert not torch.equal(bad, new.ref), f"rows_per_tile = 16: dropping K column {c} from block {blk} must change the result"


def test_one_ragged_column_tap_reads_the_next_row():
    """test_conv3x3_lds_halo's (128 -> 256, 8 x 12: two 64-channel chunks, 12 of a rectangle's 16 columns used): at the last pixel
    of an image row the taps with kx = 2 lie one pixel past the right edge; a border test against the rectangle's width instead of
    the frame's reads the next address — the first pixel of the next row — instead of zero.  Applied to tap (1, 2) for one channel
    of chunk 1 at one output pixel."""
    n, cin, cout, h, w = 3, 128, 256, 8, 12
    x = _rnd(n, cin, h, w, seed=1)
    wt, b = _rnd(cout, cin, 3, 3, seed=2, scale=(9 * cin) ** -0.5), _rnd(cout, seed=3)
    conv = lambda x_, w_, b_: F.conv2d(x_, w_, b_, padding=1)
    ref = conv(x, wt, b)
    o = E.operands((n, cin, h, w), (cout, cin, 3, 3), conv, seed=2, frames_per_bias=1, nres=1, rows_per_tile=16)
    c, y = 64 + 17, 3                                   # chunk 1; output pixel (y, w - 1): the tap reads (y, w) -> (y + 1, 0)
    f, co = _nonzero_term(o.x[:, c, y + 1, 0], o.w[:, c, 1, 2])
    bad = ref.clone()
    bad[f, co, y, w - 1] += x[f, c, y + 1, 0] * wt[co, c, 1, 2]
    assert not torch.equal(bad, ref)
    _close(bad, ref, what="Gaussian operands: the tap that wraps into the next row passes the tolerance")
    bad = o.ref.clone()
    bad[f, co, y, w - 1] += o.x[f, c, y + 1, 0] * o.w[co, c, 1, 2]
    assert not torch.equal(bad, o.ref), "integer operands: the tap that wraps into the next row must change the result"


# (frames, Cin, Cout, H, W) of test_exact_gpu's conv_halo cases, and the other conv gathers' shapes past one 64-channel chunk
HALO_SHAPES = [(3, 128, 128, 8, 16), (3, 192, 320, 8, 12), (2, 320, 640, 16, 24), (2, 128, 960, 16, 16), (2, 128, 1280, 16, 8),
               (9, 128, 256, 8, 16), (2, 128, 256, 24, 40), (2, 128, 256, 32, 20), (1, 64, 64, 8, 16)]


def test_generator_conditions():
    """The operand recipe at the K and N of the network's layers: every K column observed, |ref| <= 256, integers throughout (the
    assertions live in _exact_ints.check_inputs); and a recipe that breaks a condition is refused.  With rows_per_tile = 16 at
    every conv_halo shape of test_exact_gpu (row bias and one residual, as there), 640 -> 320 at 8 x 12, and the multi-chunk shapes
    of the other conv gathers: the block condition, the same bounds, and group sums of squares below 2^24."""
    import pytest
    for k, n in [(2560, 1280), (320, 960), (640, 5120), (960, 320)]:
        o = E.operands((64, k), (n, k), F.linear, seed=k, rows_per_bias=16)
        assert o.ref.abs().max().item() <= E.BF16_EXACT
    conv = lambda x_, w_, b_: F.conv2d(x_, w_, b_, padding=1)
    for nf, cin, cout, h, w in HALO_SHAPES + [(1, 640, 320, 8, 12), (3, 192, 384, 12, 16), (2, 192, 320, 9, 7), (2, 128, 96, 9, 7)]:
        o = E.operands((nf, cin, h, w), (cout, cin, 3, 3), conv, seed=w, frames_per_bias=1, nres=1, rows_per_tile=16)
        assert not bool(E.unobserved(o.w, 16).any()) and o.ref.abs().max().item() <= E.BF16_EXACT
        if cout % 32 == 0:
            E.group_sums(o.ref.permute(0, 2, 3, 1))
    o = E.operands((6, 128, 3, 5), (96, 128, 3), E.temporal_ref(2, 3), seed=1, frames_per_bias=3, rows_per_tile=16)
    assert not bool(E.unobserved(o.w, 16).any())
    w0, w16 = E.sparse_weight((640, 320, 3, 3), E.gen(1)), E.sparse_weight((640, 320, 3, 3), E.gen(1), rows_per_tile=16)
    assert bool(((w0 == w16) | (w0 == 0)).all()), "rows_per_tile only adds weights: the draws before it are unchanged"
    with pytest.raises(AssertionError):
        E.check_inputs(o.x, E.sparse_weight((96, 128, 3), E.gen(1)), o.ref, 0, E.BF16_EXACT, rows_per_tile=16)
    with pytest.raises(AssertionError):
        E.operands((64, 640), (4, 640), F.linear, seed=1, xmax=64)        # 160 non-zeros per row times |x| <= 64: beyond 256
