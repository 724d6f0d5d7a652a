"""Graded edit masks restated in numpy: the definitions the kernels of csrc/softmask.hip, the level launcher of
csrc/mask.hip and ccedit_amd/softmask.py are tested against, bit for bit.  Nothing here imports the package."""
import numpy as np


def feather(m: np.ndarray, radius: int) -> np.ndarray:
    """uint8 maps (..., H, W) -> the mean over the (2 radius + 1)^2 square, the window clipped at the frame border:
    (2 S + A) // (2 A) with S the sum of the bytes in the clipped window and A its pixel count (round half up).  Per map."""
    assert m.dtype == np.uint8 and m.ndim >= 2 and radius >= 0
    h, w = m.shape[-2:]
    flat = m.reshape(-1, h, w).astype(np.int64)
    ii = np.zeros((flat.shape[0], h + 1, w + 1), np.int64)                 # summed-area table
    ii[:, 1:, 1:] = flat.cumsum(axis=1).cumsum(axis=2)
    y, x = np.arange(h), np.arange(w)
    y0, y1 = np.maximum(y - radius, 0), np.minimum(y + radius, h - 1) + 1
    x0, x1 = np.maximum(x - radius, 0), np.minimum(x + radius, w - 1) + 1
    s = (ii[:, y1][:, :, x1] - ii[:, y0][:, :, x1] - ii[:, y1][:, :, x0] + ii[:, y0][:, :, x0])
    a = ((y1 - y0)[:, None] * (x1 - x0)[None, :])[None]
    return ((2 * s + a) // (2 * a)).astype(np.uint8).reshape(m.shape)


def latent_strength(m: np.ndarray) -> np.ndarray:
    """Pixel strengths uint8 (..., H, W) -> latent strengths uint8 (..., H / 8, W / 8): (sum of the 64 bytes of the cell + 32) >> 6."""
    assert m.dtype == np.uint8 and m.shape[-2] % 8 == 0 and m.shape[-1] % 8 == 0
    h, w = m.shape[-2] // 8, m.shape[-1] // 8
    s = m.astype(np.int64).reshape(*m.shape[:-2], h, 8, w, 8).sum(axis=(-3, -1))
    return ((s + 32) >> 6).astype(np.uint8)


def threshold(j: int, n: int) -> int:
    """The smallest latent strength that is free before walked step j of n."""
    assert n >= 1 and 0 <= j < n
    return (255 * (n - j) + n - 1) // n


def blend_level(x, x0, noise, strength, thr, sigma, s):
    """float32 (B, C, T, h, w), strength uint8 (B, T, h, w): (strength >= thr) ? x : (x0 + noise * sigma) / s, three float32 roundings."""
    x, x0, noise = (np.asarray(a, np.float32) for a in (x, x0, noise))
    with np.errstate(over="ignore"):
        known = (x0 + noise * np.float32(sigma)) / np.float32(s)
    assert known.dtype == np.float32
    return np.where((strength >= thr)[:, None], x, known)


def composite_graded(result, original, g):
    """float32 (B, 3, T, H, W), g uint8 (B, T, H, W): g == 255 ? result : g == 0 ? original : original + (result - original) * (g / 255)
    with one float32 divide, subtract, multiply and add."""
    result, original = np.asarray(result, np.float32), np.asarray(original, np.float32)
    gg = g[:, None]
    a = gg.astype(np.float32) / np.float32(255.0)
    mix = original + (result - original) * a
    assert mix.dtype == np.float32
    return np.where(gg == 255, result, np.where(gg == 0, original, mix))
