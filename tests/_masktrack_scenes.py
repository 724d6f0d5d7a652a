"""Synthetic clips for the mask-tracking tests: the scene() generator of tests/test_propagate_gpu.py, extended to return the truth —
the object's rectangle on every frame as a 0 / 255 mask."""
import numpy as np


def textured(h, w, seed, smooth=5):
    rs = np.random.RandomState(seed)
    a = rs.randint(0, 256, (h, w, 3)).astype(np.float64)
    k = np.ones(smooth) / smooth
    for ax in (0, 1):
        a = np.apply_along_axis(lambda v: np.convolve(v, k, mode="same"), ax, a)
    return ((a - a.min()) / (a.max() - a.min()) * 255).astype(np.uint8)


def scene(h, w, frames, seed=0, bg=(1, -2), obj=(-2, 3), noise=0.0):
    """An object (its own texture, a third of the frame) moving by `obj` pixels per frame over a background moving by `bg`.
    noise: sigma of Gaussian noise in grey levels added to every frame.  -> (uint8 (frames, h, w, 3), truth masks uint8 (frames, h, w))."""
    big = textured(h + 2 * 8 * frames + 32, w + 2 * 8 * frames + 32, seed)
    oh, ow = h // 3, w // 3
    thing = textured(oh, ow, seed + 1, smooth=3)
    out, truth = [], []
    for t in range(frames):
        y0, x0 = 8 * frames + bg[0] * t, 8 * frames + bg[1] * t
        f = big[y0:y0 + h, x0:x0 + w].copy()
        oy = int(np.clip(h // 3 + obj[0] * t, 0, h - oh))
        ox = int(np.clip(w // 3 + obj[1] * t, 0, w - ow))
        f[oy:oy + oh, ox:ox + ow] = thing
        m = np.zeros((h, w), np.uint8)
        m[oy:oy + oh, ox:ox + ow] = 255
        out.append(f)
        truth.append(m)
    clip = np.stack(out)
    if noise:
        rs = np.random.RandomState(seed + 1000)
        clip = np.clip(np.rint(clip.astype(np.float64) + rs.normal(0.0, noise, clip.shape)), 0, 255).astype(np.uint8)
    return clip, np.stack(truth)


def random_frames(h, w, frames, seed):
    return np.random.RandomState(seed).randint(0, 256, (frames, h, w, 3)).astype(np.uint8)
