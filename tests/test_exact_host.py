"""Why tests/test_exact_gpu.py exists, shown without a GPU: three single-element defects applied to the float64 reference.

Each mutation is one a mis-indexed kernel could make — one K element dropped from one dot product, one corner tap dropped at a
frame corner, one pixel left out of a GroupNorm group sum.  On the Gaussian operands of tests/test_ops_gpu.py every one of them
stays inside the limits that file asserts (`_close`: 2^-7 max|ref| + 1e-3; statistics: rtol 1e-4, atol 1e-2).  On the integer
operands of tests/_exact_ints.py every one of them changes the exact comparison, because every term there is a non-zero integer —
that every K column carries a weight is one of the two conditions the generator asserts.
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


def test_generator_conditions():
    """The operand recipe at the K and N of the network's layers: every K column observed, |ref| <= 256, integers throughout (the
    assertions live in _exact_ints.check_inputs); and a recipe that breaks a condition is refused."""
    import pytest
    for k, n in [(2560, 1280), (320, 960), (640, 5120), (960, 320)]:
        o = E.operands((64, k), (n, k), F.linear, seed=k, rows_per_bias=16)
        assert o.ref.abs().max().item() <= E.BF16_EXACT
    with pytest.raises(AssertionError):
        E.operands((64, 640), (4, 640), F.linear, seed=1, xmax=64)        # 160 non-zeros per row times |x| <= 64: beyond 256
