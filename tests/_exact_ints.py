"""Integer-valued operands for the exact-arithmetic kernel tests (tests/test_exact_gpu.py, tests/test_exact_host.py).

Every tensor here is float64 on the CPU and holds integers.  The recipe: activations dense in [-xmax, xmax] (2 for the bf16
kernels), weights in {-1, 0, +1} with about 48 non-zeros per output row and at least one in EVERY K column (`rows_per_tile=R`: in
every K column of every block of R consecutive output rows — a channel tile of a kernel), bias and row bias in [-8, 8], residuals
in [-16, 16].  Under the two conditions `check_inputs` asserts, a correct kernel reproduces the float64
reference bit for bit whatever its tile shape, K order, split or atomic order:

  * sum over K of |x| |w| plus the epilogue terms stays below 2^24, so every product and every partial sum in any order is an
    integer that fp32 holds exactly (accumulators, split-K workspace, fp32 statistics partials);
  * the final value is an integer with |r| <= 256, and every such integer is a bf16 number (8 significant bits).  The fp32 VAE
    kernels write fp32: their bound on |r| is 2^24.

Sums and sums of squares of such outputs are integers far below 2^53: exact in the fp64 statistics accumulators.
"""
from types import SimpleNamespace

import torch
import torch.nn.functional as F

BF16_EXACT = 256            # |integer| <= 2^8: representable in bf16
F32_EXACT = 1 << 24         # |integer| <= 2^24: representable in fp32 — and the bound on every partial sum
NNZ_PER_ROW = 48


def gen(seed):
    return torch.Generator().manual_seed(seed)


def ints(shape, lo, hi, g):
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).double()


def unobserved(w, rows_per_tile):
    """(tiles, K) mask of the (block of `rows_per_tile` consecutive output rows, K column) pairs in which the block holds no weight:
    a kernel whose defect lives in that channel tile may drop or misread that K element and the result does not change."""
    w2 = w.reshape(w.shape[0], -1)
    nt = (w2.shape[0] + rows_per_tile - 1) // rows_per_tile
    return torch.stack([(w2[t * rows_per_tile:(t + 1) * rows_per_tile] != 0).sum(dim=0) == 0 for t in range(nt)])


def sparse_weight(shape, g, wmax=1, rows_per_tile=0):
    """Reference-layout weight (O, I) / (O, I, K) / (O, I, KH, KW) with entries in {-wmax..-1, 0, 1..wmax}: density 48 / K (the
    density follows K, so the row sums stay near sqrt(48) whatever the layer), then one non-zero into every K column that got none —
    a K column without a weight would leave that element of A unobserved.
    rows_per_tile = R > 0: afterwards every block of R consecutive output rows (a kernel's channel tile, or a part of one) gets one
    +-1 at a random row of the block in every K column where the block holds no weight, so every K element is observed in EVERY
    tile.  These draws come after all the others: with the default 0 nothing extra is drawn and the weights are what they were."""
    n = shape[0]
    kk = 1
    for s in shape[1:]:
        kk *= s
    p = min(1.0, NNZ_PER_ROW / kk)
    mag = torch.randint(1, wmax + 1, (n, kk), generator=g).double()
    sign = (torch.randint(0, 2, (n, kk), generator=g) * 2 - 1).double()
    w = (torch.rand(n, kk, generator=g) < p).double() * sign * mag
    empty = ((w != 0).sum(dim=0) == 0).nonzero().flatten()
    if empty.numel():
        rows = torch.randint(0, n, (empty.numel(),), generator=g)
        w[rows, empty] = sign[rows, empty] * mag[rows, empty]
    if rows_per_tile:
        for r0 in range(0, n, rows_per_tile):
            blk = w[r0:r0 + rows_per_tile]                      # a view: the block is filled in place
            empty = ((blk != 0).sum(dim=0) == 0).nonzero().flatten()
            if empty.numel():
                rows = torch.randint(0, blk.shape[0], (empty.numel(),), generator=g)
                blk[rows, empty] = (torch.randint(0, 2, (empty.numel(),), generator=g) * 2 - 1).double()
    return w.reshape(shape)


def check_inputs(x, w, ref, extra, out_max, rows_per_tile=0):
    """The two conditions on the INPUTS (not tolerances): every K column of w carries a non-zero — with rows_per_tile = R inside
    every block of R consecutive output rows — and |ref| <= out_max.  Plus the premise of exactness itself: (largest row sum of
    |w|) * max|x| + the epilogue terms < 2^24 bounds every partial sum."""
    w2 = w.reshape(w.shape[0], -1)
    assert bool((w2 != 0).any(dim=0).all()), "a K column of the weight has no non-zero entry"
    if rows_per_tile:
        gaps = int(unobserved(w, rows_per_tile).sum())
        assert gaps == 0, f"{gaps} (block of {rows_per_tile} output rows, K column) pairs hold no weight"
    assert bool((ref == ref.round()).all()), "the reference is not integer-valued"
    assert ref.abs().max().item() <= out_max, f"max|ref| = {ref.abs().max().item()} > {out_max}"
    assert w2.abs().sum(dim=1).max().item() * x.abs().max().item() + extra < F32_EXACT, "partial sums may leave fp32's integers"


def operands(xshape, wshape, fwd, seed=0, xmax=2, wmax=1, bias=True, rows_per_bias=0, frames_per_bias=0, nres=2, out_max=BF16_EXACT,
             bmax=8, rmax=16, rows_per_tile=0):
    """x, w, bias, row bias, residuals and the float64 reference `fwd(x, w, bias) + row bias + residuals`.
    fwd: F.linear / F.conv2d / F.conv1d on float64; its result is (M, N) or (frames, C, H, W).
    rows_per_bias: one row-bias vector per that many GEMM rows (2-D results); frames_per_bias: per that many frames (4-D results).
    rows_per_tile: see sparse_weight (the bias, row bias and residual draws follow the weight's, so they differ from the default's)."""
    g = gen(seed)
    x = ints(xshape, -xmax, xmax, g)
    w = sparse_weight(wshape, g, wmax, rows_per_tile)
    b = ints((wshape[0],), -bmax, bmax, g) if bias else None
    ref = fwd(x, w, b)
    gb = None
    if rows_per_bias:
        gb = ints(((ref.shape[0] + rows_per_bias - 1) // rows_per_bias, ref.shape[1]), -bmax, bmax, g)
        ref = ref + gb.repeat_interleave(rows_per_bias, 0)[: ref.shape[0]]
    if frames_per_bias:
        gb = ints((ref.shape[0] // frames_per_bias, ref.shape[1]), -bmax, bmax, g)
        ref = ref + gb.repeat_interleave(frames_per_bias, 0)[:, :, None, None]
    res = [ints(ref.shape, -rmax, rmax, g) for _ in range(nres)]
    for r in res:
        ref = ref + r
    check_inputs(x, w, ref, 2 * bmax + nres * rmax, out_max, rows_per_tile)
    return SimpleNamespace(x=x, w=w, b=b, gb=gb, res=res, r1=res[0] if nres > 0 else None, r2=res[1] if nres > 1 else None, ref=ref)


def temporal_ref(b_, t):
    """Conv1d k3 over the T frames of each clip, x (b*t, C, H, W): F.conv1d on the '(b h w) c t' view (zeros at the clip ends)."""
    def fwd(x, w, bias):
        n, c, h, wd = x.shape
        xp = x.reshape(b_, t, c, h, wd).permute(0, 3, 4, 2, 1).reshape(b_ * h * wd, c, t)
        y = F.conv1d(xp, w, bias, padding=1)
        return y.reshape(b_, h, wd, w.shape[0], t).permute(0, 4, 3, 1, 2).reshape(n, w.shape[0], h, wd)
    return fwd


def group_sums(y_nhwc):
    """float64 (sum, sum of squares) per (frame, GroupNorm(32) group) of an integer-valued (N, H, W, C) tensor: (N, 32, 2).
    Also asserts the premise for fp32 partials inside the kernels: every group's sum of squares is below 2^24."""
    n, h, w, c = y_nhwc.shape
    yf = y_nhwc.double().reshape(n, h * w, 32, c // 32)
    st = torch.stack([yf.sum(dim=(1, 3)), (yf * yf).sum(dim=(1, 3))], dim=-1)
    assert st[..., 1].max().item() < F32_EXACT, "a group's sum of squares leaves fp32's integers"
    return st


def cancellation(m, n, k, cols, seed=0):
    """One Linear whose columns `cols` cancel: the first K element contributes +2^12 (64 * 64), the last -2^12, and min(K - 2, 256) of
    the elements in between +1 each (all of them when K <= 258, otherwise a random set per row), so the exact result is that count —
    an intermediate held in bf16 (a split-K partial, a staged accumulator, a combine across K halves) would lose the ones next to
    4096.  The other columns are the usual sparse {-1, 0, 1} rows (zero at both ends of K)."""
    g = gen(seed)
    ones = min(k - 2, 256)
    x = torch.zeros(m, k, dtype=torch.float64)
    order = torch.rand(m, k - 2, generator=g).argsort(dim=1)[:, :ones] + 1
    x.scatter_(1, order, 1.0)
    x[:, 0] = 64.0
    x[:, k - 1] = 64.0
    w = sparse_weight((n, k), g)
    w[:, 0] = 0.0
    w[:, k - 1] = 0.0
    for c in cols:
        w[c] = 1.0
        w[c, 0], w[c, k - 1] = 64.0, -64.0
    ref = F.linear(x, w)
    assert bool((ref[:, list(cols)] == ones).all())
    assert ref.abs().max().item() <= BF16_EXACT and bool((ref == ref.round()).all())
    return SimpleNamespace(x=x, w=w, ref=ref, ones=ones)
