"""The inputs the JPEG decoder's tests share (tests/test_jpegdec.py on the CPU, tests/test_jpegdec_gpu.py on the device): the grid of
Pillow-written streams, the own encoder's streams, and the seeded corruptions of their entropy-coded data.  Everything is generated
here from seeds; the restatement's decode of the grid is computed once per process (reference())."""
import functools
import io
import itertools

import numpy as np
from PIL import Image

import _jpegdec_numpy as R
import _mjpeg_numpy as E
from ccedit_amd import jpegdec as J

SIZES = [(1, 1), (8, 8), (16, 16), (17, 19), (33, 50), (48, 32), (160, 16)]        # (H, W); 160 x 16: ten MCU rows, the restart marker number wraps past 7
SUBSAMPLING = ["4:4:4", "4:2:2", "4:2:0", "grey"]
QUALITY = [30, 75, 95, 100]
CONTENT = ["noise", "flat", "ramp", "primaries"]


def content(kind, h, w, seed):
    y, x = np.mgrid[0:h, 0:w]
    if kind == "noise":
        return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "flat":
        return np.full((h, w, 3), (200, 30, 90), np.uint8)
    if kind == "ramp":
        return np.stack([x * 255 // max(w - 1, 1), y * 255 // max(h - 1, 1), (x + y) * 255 // max(h + w - 2, 1)], axis=2).astype(np.uint8)
    prim = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0]], np.uint8)          # saturated, in a 2 x 2 checker
    return prim[((y // 2) % 2) * 2 + ((x // 2) % 2)]


def pillow_jpeg(img, subsampling, quality, optimize, restart, **kw):
    im = Image.fromarray(img)
    if subsampling == "grey":
        im = im.convert("L")
    else:
        kw["subsampling"] = subsampling
    if restart:
        kw["restart_marker_rows"] = 1
    b = io.BytesIO()
    im.save(b, format="JPEG", quality=quality, optimize=optimize, **kw)
    return b.getvalue()


def pillow_decode(jpeg):
    return np.array(Image.open(io.BytesIO(jpeg)).convert("RGB"))


@functools.lru_cache(maxsize=None)
def grid():
    """-> list of (name, jpeg bytes): sizes x subsampling x quality x Huffman tables x restart markers x content."""
    out = []
    for n, ((h, w), ss, q, opt, rst, kind) in enumerate(itertools.product(SIZES, SUBSAMPLING, QUALITY, (False, True), (False, True), CONTENT)):
        name = f"{h}x{w}-{ss}-q{q}-{'opt' if opt else 'std'}-{'rst' if rst else 'norst'}-{kind}"
        out.append((name, pillow_jpeg(content(kind, h, w, n), ss, q, opt, rst)))
    return out


@functools.lru_cache(maxsize=None)
def own_encoder():
    """-> list of (name, jpeg bytes) written by the project's encoder (its numpy restatement): noise and ramp at quality 40 and 90."""
    out = []
    for kind, q in itertools.product(("noise", "ramp"), (40, 90)):
        frames = np.stack([content(kind, 48, 32, 100 + q), content(kind, 48, 32, 200 + q)[::-1].copy()])
        out += [(f"own-{kind}-q{q}-{i}", j) for i, j in enumerate(E.encode_frames(frames, q))]
    return out


@functools.lru_cache(maxsize=None)
def reference():
    """-> {name: (info, coef, status, rgb)} of the restatement over grid() + own_encoder(): computed once, shared, never changed."""
    ref = {}
    for name, j in grid() + own_encoder():
        info = J.parse(j)
        coef, status = R.entropy(info, j)
        rgb = R.rgb(info, R.idct(info, coef))
        for a in (coef, status, rgb):
            a.setflags(write=False)
        ref[name] = (info, coef, status, rgb)
    return ref


CORRUPTIONS = 2000


def _corruption_stream():
    """The seeded corruptions, one after the other and without end: (name, info, data bytes, intervals int64 (I, 2), whole_file).  Byte
    flips, truncated intervals and markers inserted inside an interval of the entropy-coded data of small grid streams.  A byte flip
    keeps the file's layout: `whole_file` says that `data` is still a complete file (the parser may or may not accept it); the others
    are handed to the decode core as (data, intervals) only."""
    rng = np.random.default_rng(20250)
    base = [(n, j) for n, j in grid() if any(n.startswith(s) for s in ("16x16-", "17x19-", "8x8-")) and ("noise" in n or "ramp" in n)]
    count = 0
    while True:
        name, j = base[int(rng.integers(len(base)))]
        info = J.parse(j)
        iv = info.intervals.copy()
        k = int(rng.integers(len(iv)))
        lo, hi = int(iv[k, 0]), int(iv[k, 1])
        if hi - lo < 2:
            continue
        kind = ("flip", "cut", "marker")[int(rng.integers(3))]
        data = bytearray(j)
        if kind == "flip":
            for _ in range(int(rng.integers(1, 4))):
                data[int(rng.integers(lo, hi))] ^= 1 << int(rng.integers(8))
        elif kind == "cut":
            iv[k, 1] = int(rng.integers(lo, hi))
        else:
            at = int(rng.integers(lo, hi))
            m = (0xD0 + int(rng.integers(8)), 0xD9, 0xFF, 0xC4, 0x01)[int(rng.integers(5))]
            data[at:at] = bytes([0xFF, m])
            iv[k, 1] += 2
            iv[k + 1:] += 2
        yield f"{name}-{kind}{count}", info, bytes(data), iv, kind == "flip"
        count += 1


@functools.lru_cache(maxsize=None)
def corruptions():
    """-> the first CORRUPTIONS of _corruption_stream(), as a list."""
    return list(itertools.islice(_corruption_stream(), CORRUPTIONS))


@functools.lru_cache(maxsize=None)
def corruption_statuses():
    """The restatement's status words of corruptions(), in its order."""
    return [R.entropy(info, data, iv)[1] for _, info, data, iv, _ in corruptions()]


def gpu_corrupt_files(count=12):
    """-> list of (name, file bytes, status (I,)): the first `count` byte-flip corruptions that are still complete files the parser
    accepts with the layout unchanged, and that the decode core stops on.  FIXED: the rule and the seed decide them.  They are the
    first of corruptions(), which the hardening program runs; only as many are generated and decoded here as it takes to find them."""
    out = []
    for n, (name, info, data, iv, whole) in enumerate(_corruption_stream()):
        assert n < CORRUPTIONS, f"only {len(out)} of {count} such files among the {CORRUPTIONS} corruptions"
        if not whole:
            continue
        try:
            again = J.parse(data)
        except J.JpegUnsupported:
            continue
        if again.key() != info.key() or not np.array_equal(again.intervals, iv):
            continue
        status = R.entropy(info, data, iv)[1]
        if status.any():
            out.append((name, data, status))
            if len(out) == count:
                return out
