"""The arithmetic of region prompts, restated in numpy: what csrc/region.hip must reproduce bit for bit (ccedit_amd/regions.py keeps the
constants; nothing here imports the product)."""
import numpy as np


def cell_counts(masks: np.ndarray) -> np.ndarray:
    """uint8 (K, T, H, W), H and W multiples of 8 -> int64 (K, T, H/8, W/8): the pixels >= 128 of every 8 x 8 latent cell, 0 ... 64."""
    k, t, hh, ww = masks.shape
    assert hh % 8 == 0 and ww % 8 == 0
    return (masks >= 128).reshape(k, t, hh // 8, 8, ww // 8, 8).sum(axis=(3, 5)).astype(np.int64)


def box_sums(a: np.ndarray, feather: int) -> np.ndarray:
    """s[..., i, j] = sum of a over the (2F + 1) x (2F + 1) cells around (i, j), coordinates clamped into the frame (the edge replicated)."""
    f = int(feather)
    h, w = a.shape[-2:]
    s = np.zeros_like(a)
    for di in range(-f, f + 1):
        ii = np.clip(np.arange(h) + di, 0, h - 1)
        for dj in range(-f, f + 1):
            jj = np.clip(np.arange(w) + dj, 0, w - 1)
            s += a[..., ii[:, None], jj[None, :]]
    return s


def region_weights(masks: np.ndarray, feather: int) -> np.ndarray:
    """uint8 (K, T, H, W) -> float32 (K + 1, T, h, w): coef[0] the base prompt's share, coef[r] region r's.  Integers up to the one
    quotient, formed in float64 and converted to float32."""
    f = int(feather)
    s = box_sums(cell_counts(masks), f)                                # (K, T, h, w), 0 ... S
    big = 64 * (2 * f + 1) ** 2
    tot = s.sum(axis=0)
    d = np.maximum(big, tot)
    allr = np.concatenate([(d - tot)[None], s], axis=0)
    return (allr.astype(np.float64) / d[None].astype(np.float64)).astype(np.float32)


def region_fuse(ys, coef: np.ndarray) -> np.ndarray:
    """ys: K + 1 float32 arrays (B, C, T, h, w); coef float32 (K + 1, T, h, w) -> float32 (B, C, T, h, w).  Ascending r; a term whose
    coefficient is exactly 0 is skipped (its y is never looked at); the first term is the product alone, every further term one
    multiply (rounded) then one add (rounded).  An element with no term is 0."""
    out = np.zeros(ys[0].shape, np.float32)
    started = np.zeros(coef.shape[1:], bool)
    with np.errstate(all="ignore"):
        for r, y in enumerate(ys):
            use = coef[r] != 0
            term = (coef[r][None, None] * y).astype(np.float32)
            summed = (out + term).astype(np.float32)
            new = np.where(started[None, None], summed, term)
            out = np.where(use[None, None], new, out)
            started |= use
    return out
