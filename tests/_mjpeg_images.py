"""The test images of the Motion-JPEG tests (tests/test_mjpeg.py, tests/test_mjpeg_gpu.py): a smooth gradient, smoothed noise, uniform
random bytes, all-0, all-255 and a frame whose left half is flat; the qualities; PSNR; Pillow as the independent decoder."""
import io

import numpy as np

QUALITIES = [1, 50, 90, 100]
IMAGES = ["gradient", "smooth", "random", "black", "white", "halfflat"]


def smoothed(h, w, seed, k=5):
    rs = np.random.RandomState(seed)
    a = rs.randint(0, 256, (h, w, 3)).astype(np.float64)
    ker = np.ones(k) / k
    for ax in (0, 1):
        a = np.apply_along_axis(lambda v: np.convolve(v, ker, mode="same"), ax, a)
    return ((a - a.min()) / (a.max() - a.min()) * 255).astype(np.uint8)


def image(name, h, w, seed=0):
    if name == "gradient":
        y, x = np.mgrid[0:h, 0:w]
        return np.stack([x * 255 // (w - 1), y * 255 // (h - 1), (x + y) * 255 // (h + w - 2)], -1).astype(np.uint8)
    if name == "smooth":
        return smoothed(h, w, seed)
    if name == "random":
        return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)
    if name == "black":
        return np.zeros((h, w, 3), np.uint8)
    if name == "white":
        return np.full((h, w, 3), 255, np.uint8)
    if name == "halfflat":
        a = np.random.RandomState(seed + 7).randint(0, 256, (h, w, 3)).astype(np.uint8)
        a[:, :w // 2] = (90, 160, 30)
        return a
    raise KeyError(name)


def psnr(a, b):
    return 10.0 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


def pil_decode(jpeg):
    from PIL import Image
    im = Image.open(io.BytesIO(jpeg))
    im.load()
    return im
