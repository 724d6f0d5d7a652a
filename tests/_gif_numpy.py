"""The device GIF encoder of ccedit_amd/csrc/gif.hip restated in plain numpy / Python: pixels in, palettes, indices and the exact bytes
of each frame's LZW stream and of the file out.  It is NORMATIVE: the GPU result is these bytes (tests/test_gif_gpu.py), and what these
bytes are worth is checked on the CPU (tests/test_gif.py: Pillow decodes them, quality against Pillow's own quantiser).  The constants
come from ccedit_amd/gif.py, their one place; none of the arithmetic and none of the container does.

  moments(frame)            uint8 (H, W, 3) -> int64 (5, 33, 33, 33): count, sum r, sum g, sum b, sum r^2 + g^2 + b^2 per cell, zero border
  prefix(m)                 -> their inclusive 3-D prefix sums
  cut_boxes(p)              -> the boxes (r0, r1, g0, g1, b0, b1), half open (lo, hi], after at most 255 cuts
  quantize_frame(frame)     -> (palette uint8 (256, 3), indices uint8 (H, W), cells uint8 (32, 32, 32), boxes)
  lzw_chunk / lzw_frame     indices -> (bits as an int, bit length) per chunk / the frame's byte stream
  encode_frames(frames)     -> per frame (palette bytes, LZW bytes): what ccedit_amd.gif.encode_frames returns
  file_bytes(encoded, ...)  -> the GIF file
"""
import struct

import numpy as np

from ccedit_amd import gif as G


# ---- the quantiser
def moments(frame):
    p = frame.reshape(-1, 3).astype(np.int64)
    r, g, b = p[:, 0], p[:, 1], p[:, 2]
    idx = (((r >> G.SHIFT) + 1) * G.SIDE + (g >> G.SHIFT) + 1) * G.SIDE + (b >> G.SHIFT) + 1
    m = np.zeros((G.MOMENTS, G.SIDE ** 3), np.int64)
    for k, v in enumerate((np.ones_like(r), r, g, b, r * r + g * g + b * b)):
        np.add.at(m[k], idx, v)
    return m.reshape(G.MOMENTS, G.SIDE, G.SIDE, G.SIDE)


def prefix(m):
    return m.cumsum(axis=1).cumsum(axis=2).cumsum(axis=3)


def vol(t, box):
    """The sum of the cells r0 < r <= r1, g0 < g <= g1, b0 < b <= b1 from the prefix table t (33, 33, 33) -> int."""
    r0, r1, g0, g1, b0, b1 = box
    return int(t[r1, g1, b1] - t[r1, g1, b0] - t[r1, g0, b1] + t[r1, g0, b0] - t[r0, g1, b1] + t[r0, g1, b0] + t[r0, g0, b1] - t[r0, g0, b0])


def box_score(p, box):
    r0, r1, g0, g1, b0, b1 = box
    if (r1 - r0) * (g1 - g0) * (b1 - b0) <= 1:
        return 0.0
    w, dr, dg, db, m2 = (float(vol(p[k], box)) for k in range(5))
    return m2 - (dr * dr + dg * dg + db * db) / w


def _lower_halves(t, box, d, pos):
    """Sums of the box cut in direction d at every position of `pos` (the half lo < x <= pos), int64 array."""
    q = np.moveaxis(t, d, 0)
    (a0, a1), (c0, c1) = [(box[2 * e], box[2 * e + 1]) for e in range(3) if e != d]
    face = lambda x: q[x, a1, c1] - q[x, a1, c0] - q[x, a0, c1] + q[x, a0, c0]
    return face(pos) - face(box[2 * d])


def best_cut(p, box):
    """-> (direction, position) or None.  Per direction the best interior position: strictly greater score, so the lowest wins ties;
    positions with an empty half are skipped.  Direction r if its best >= both others, else g if its best >= both others, else b."""
    whole = [vol(p[k], box) for k in range(4)]
    best = []
    for d in range(3):
        pos = np.arange(box[2 * d] + 1, box[2 * d + 1])
        if pos.size == 0:
            best.append((-1.0, -1))
            continue
        h = [_lower_halves(p[k], box, d, pos) for k in range(4)]
        o = [whole[k] - h[k] for k in range(4)]
        ok = (h[0] > 0) & (o[0] > 0)
        hf = [x.astype(np.float64) for x in h]
        of = [x.astype(np.float64) for x in o]
        with np.errstate(divide="ignore", invalid="ignore"):
            s = (hf[1] * hf[1] + hf[2] * hf[2] + hf[3] * hf[3]) / hf[0] + (of[1] * of[1] + of[2] * of[2] + of[3] * of[3]) / of[0]
        s = np.where(ok, s, -1.0)
        i = int(np.argmax(s))                   # the first of the maxima
        best.append((float(s[i]), int(pos[i])) if ok[i] else (-1.0, -1))
    (sr, _), (sg, _), (sb, _) = best
    d = 0 if (sr >= sg and sr >= sb) else (1 if (sg >= sr and sg >= sb) else 2)
    return None if best[d][1] < 0 else (d, best[d][1])


def cut_boxes(p):
    boxes = [(0, G.GRID, 0, G.GRID, 0, G.GRID)]
    score = [box_score(p, boxes[0])]
    while len(boxes) < G.COLORS:
        nxt = int(np.argmax(score))             # the lowest-indexed box of maximal score
        if not score[nxt] > 0.0:
            break
        cut = best_cut(p, boxes[nxt])
        if cut is None:                         # cannot be cut: score 0, no palette entry consumed
            score[nxt] = 0.0
            continue
        d, pos = cut
        lo, hi = list(boxes[nxt]), list(boxes[nxt])
        lo[2 * d + 1] = pos
        hi[2 * d] = pos
        boxes[nxt] = tuple(lo)
        boxes.append(tuple(hi))
        score[nxt] = box_score(p, boxes[nxt])
        score.append(box_score(p, boxes[-1]))
    return boxes


def quantize_frame(frame):
    p = prefix(moments(frame))
    boxes = cut_boxes(p)
    cells = np.zeros((G.GRID,) * 3, np.uint8)
    palette = np.zeros((G.COLORS, 3), np.uint8)
    for k, box in enumerate(boxes):
        r0, r1, g0, g1, b0, b1 = box
        cells[r0:r1, g0:g1, b0:b1] = k
        w = vol(p[0], box)
        palette[k] = [(vol(p[c], box) + w // 2) // w for c in (1, 2, 3)]
    f = frame.astype(np.int64) >> G.SHIFT
    return palette, cells[f[..., 0], f[..., 1], f[..., 2]], cells, boxes


def quantize(frames):
    """uint8 (N, H, W, 3) -> (palettes (N, 256, 3), indices (N, H, W))."""
    q = [quantize_frame(f) for f in frames]
    return np.stack([x[0] for x in q]), np.stack([x[1] for x in q])


# ---- LZW
def lzw_chunk(idx, first, last):
    """One chunk's indices -> (its bits as an int, LSB first; the number of bits; the number of codes without Clear / EOI)."""
    acc, nbits, width, nxt, codes = 0, 0, G.START_WIDTH, G.FIRST_CODE, 0
    table = {}

    def emit(code):
        nonlocal acc, nbits
        acc |= code << nbits
        nbits += width

    def count():
        nonlocal nxt, width
        nxt += 1
        if nxt > (1 << width):
            width += 1

    if first:
        emit(G.CLEAR)
    prev = int(idx[0])
    for c in idx[1:].tolist():
        key = (prev << 8) | c
        code = table.get(key)
        if code is not None:
            prev = code
            continue
        emit(prev)
        table[key] = nxt
        count()
        codes += 1
        prev = c
    emit(prev)
    count()
    codes += 1
    assert nxt < 4096 and width <= 12
    emit(G.EOI if last else G.CLEAR)
    return acc, nbits, codes


def lzw_chunks(indices, chunk=G.CHUNK):
    flat = np.asarray(indices, np.uint8).reshape(-1)
    n = -(-flat.size // chunk)
    return [lzw_chunk(flat[c * chunk:(c + 1) * chunk], c == 0, c == n - 1) for c in range(n)]


def lzw_frame(indices, chunk=G.CHUNK):
    """A frame's indices in raster order -> its LZW byte stream: the chunks' bits back to back, zero-padded to a byte."""
    acc, nbits = 0, 0
    for bits, n, _ in lzw_chunks(indices, chunk):
        acc |= bits << nbits
        nbits += n
    return acc.to_bytes((nbits + 7) // 8, "little")


def encode_frames(frames):
    pal, idx = quantize(frames)
    return [(pal[i].tobytes(), lzw_frame(idx[i])) for i in range(len(frames))]


# ---- the container
def file_bytes(encoded, duration_ms, w, h):
    out = b"GIF89a" + struct.pack("<HH", w, h) + bytes([0x70, 0, 0])                    # no global colour table
    out += bytes([0x21, 0xFF, 11]) + b"NETSCAPE2.0" + bytes([3, 1, 0, 0, 0])            # loop 0
    for palette, stream in encoded:
        out += bytes([0x21, 0xF9, 4, 0]) + struct.pack("<H", duration_ms // 10) + bytes([0, 0])
        out += bytes([0x2C]) + struct.pack("<HHHH", 0, 0, w, h) + bytes([0x80 | 7])       # local colour table, 2^(7 + 1) entries
        assert len(palette) == 768
        out += palette + bytes([G.MIN_CODE_SIZE])
        for at in range(0, len(stream), 255):
            out += bytes([len(stream[at:at + 255])]) + stream[at:at + 255]
        out += b"\x00"
    return out + b"\x3b"


def decode_file(path_or_file):
    """Every frame of a GIF as Pillow decodes it -> (uint8 (N, H, W, 3), the info dict of the first frame)."""
    from PIL import Image, ImageSequence
    im = Image.open(path_or_file)
    info = dict(im.info)
    info["n_frames"] = getattr(im, "n_frames", 1)
    return np.stack([np.array(f.convert("RGB")) for f in ImageSequence.Iterator(im)]), info
