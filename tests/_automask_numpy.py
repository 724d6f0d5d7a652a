"""The definition of the automatic edit mask (ccedit_amd/automask.py, csrc/automask.hip) in numpy: float32 with the operation order
written out, integers otherwise.  The kernels and the host code are tested against these functions bit for bit."""
import math

import numpy as np


def accumulate(y, acc=None):
    """y float32 (2B, C, T, h, w), the source-prompt half first -> float32 (B, T, h, w): ((|d_0| + |d_1|) + |d_2|) + ... with
    d_c = y[B + b, c] - y[b, c], channels ascending, one rounding per operation; stored (acc None) or added to `acc`."""
    y = np.asarray(y, dtype=np.float32)
    b = y.shape[0] // 2
    assert y.ndim == 5 and y.shape[0] == 2 * b and b >= 1
    s = None
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(y.shape[1]):
            d = np.abs((y[b:, c] - y[:b, c]).astype(np.float32)).astype(np.float32)
            s = d if s is None else (s + d).astype(np.float32)
        return s if acc is None else (np.asarray(acc, dtype=np.float32) + s).astype(np.float32)


def rank_of(q, n):
    """The 1-based rank of the q-quantile among n cells: min(n, max(1, ceil(q n))) in float64."""
    return min(int(n), max(1, int(math.ceil(float(q) * int(n)))))


def binarize(acc, quantile, theta):
    """acc float32 (B, T, h, w) -> uint8 (B, T, h, w): 1 where acc > float32(theta) * scale[b], strictly; scale[b] = the rank_of(quantile,
    T h w)-th smallest value of acc[b]."""
    acc = np.asarray(acc, dtype=np.float32)
    out = np.zeros(acc.shape, np.uint8)
    for b in range(acc.shape[0]):
        flat = np.sort(acc[b].reshape(-1))
        scale = flat[rank_of(quantile, flat.size) - 1]
        thr = np.float32(np.float32(theta) * np.float32(scale))
        out[b] = (acc[b] > thr).astype(np.uint8)
    return out


def vote(mask, votes):
    """uint8 (B, T, h, w) -> uint8: 1 where at least `votes` of the 27 cells (dt, dy, dx in {-1, 0, 1}, every coordinate clamped into the
    clip) are set.  votes = 0: the mask as it is."""
    mask = (np.asarray(mask) != 0).astype(np.int32)
    if int(votes) == 0:
        return mask.astype(np.uint8)
    _, t, h, w = mask.shape
    ti, yi, xi = np.arange(t), np.arange(h), np.arange(w)
    count = np.zeros(mask.shape, np.int32)
    for dt in (-1, 0, 1):
        tt = np.clip(ti + dt, 0, t - 1)
        for dy in (-1, 0, 1):
            yy = np.clip(yi + dy, 0, h - 1)
            for dx in (-1, 0, 1):
                xx = np.clip(xi + dx, 0, w - 1)
                count += mask[:, tt][:, :, yy][:, :, :, xx]
    return (count >= int(votes)).astype(np.uint8)


def expand(mask):
    """Latent mask (B, T, h, w), != 0 set -> pixel mask uint8 (B, T, 8h, 8w) in {0, 255}."""
    m = ((np.asarray(mask) != 0).astype(np.uint8) * np.uint8(255)).astype(np.uint8)
    return np.repeat(np.repeat(m, 8, axis=2), 8, axis=3)


def mask_latent(mask_px):
    """ops.mask_latent's rule: a cell is 1 where more than 32 of its 64 pixels are >= 128."""
    m = (np.asarray(mask_px) >= 128).astype(np.int32)
    b, t, hh, ww = m.shape
    return (m.reshape(b, t, hh // 8, 8, ww // 8, 8).sum(axis=(3, 5)) > 32).astype(np.uint8)


def mask_from(acc, quantile, theta, votes):
    """acc -> the pixel mask: binarize, vote, expand."""
    return expand(vote(binarize(acc, quantile, theta), votes))
