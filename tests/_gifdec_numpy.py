"""The GIF decoder of ccedit_amd/gifdec.py restated in numpy / plain Python, in the SAME formulation as csrc/gifdec_core.h (stage A: the
code stream -> a table of codes without touching a pixel; stage B: every code's pixels by a walk up its parents; stage C: the frames
composited on a canvas), and a deliberately DIFFERENT classic decoder (a dictionary of byte strings, decoded in order) as the cross-check
of the formulation itself.  The container comes from ccedit_amd.gifdec.parse (no pixel arithmetic there)."""
import numpy as np

OK, CODE_ABOVE_NEXT, FIRST_NOT_LITERAL, STREAM_SHORT, BAD_MIN_CODE, BAD_INDEX = 0, 1, 2, 3, 4, 5


def width_at(m, j):
    """The width of the j-th data code after a Clear (j = 0: the first): the decoder's next free entry is clear + 1 + j when it reads it."""
    return min(12, ((1 << m) + 1 + j).bit_length())


def code_table(stream: bytes, m: int, npix: int):
    """Stage A -> (parent, length, first, last, off: int arrays over the data codes; status; bit position of the code that stopped it)."""
    if not 2 <= m <= 8:
        return (np.zeros(0, np.int64),) * 5 + (BAD_MIN_CODE, 0)
    bits = int.from_bytes(stream, "little")
    nbits = 8 * len(stream)
    clear, emax = 1 << m, 4096 - ((1 << m) + 2)
    parent, length, first, last, off = [], [], [], [], []
    bp, s, opos = 0, 0, 0

    def result(status, where):
        return tuple(np.asarray(a, np.int64) for a in (parent, length, first, last, off)) + (status, where)

    while True:
        k = len(parent)
        j = k - s
        w = width_at(m, j)
        if bp + w > nbits:
            return result(STREAM_SHORT, bp)
        c = (bits >> bp) & ((1 << w) - 1)
        if c == clear:
            bp += w
            s = k
            continue
        if c == clear + 1:
            return result(STREAM_SHORT, bp)
        if c < clear:
            parent.append(-1), length.append(1), first.append(c), last.append(c)
        else:
            e = c - (clear + 2)
            if j == 0:
                return result(FIRST_NOT_LITERAL, bp)
            if e > j - 1 or e >= emax:
                return result(CODE_ABOVE_NEXT, bp)
            p = s + e
            parent.append(p), length.append(length[p] + 1), first.append(first[p])
            last.append(first[p] if p + 1 == k else first[p + 1])
        off.append(opos)
        opos += length[-1]
        bp += w
        if opos >= npix:
            return result(OK, 0)


def code_pixels(parent, length, last, off, npix: int) -> np.ndarray:
    """Stage B: every code on its own, from its last byte up the chain of parents.  Pixels no code reaches stay 255."""
    out = np.full(npix, 255, np.uint8)
    for k in range(len(parent)):
        j = k
        for i in range(int(length[k]) - 1, -1, -1):
            if off[k] + i < npix:
                out[off[k] + i] = last[j]
            j = parent[j]
    return out


def interlaced_rows(h: int):
    """stream row -> rectangle row, in four-pass order"""
    return list(range(0, h, 8)) + list(range(4, h, 8)) + list(range(2, h, 4)) + list(range(1, h, 2))


def frame_indices(f):
    """One parsed frame -> (its indices (h, w) in display order, status, position): stages A and B."""
    parent, length, first, last, off, status, where = code_table(f.stream, f.min_code, f.w * f.h)
    if status:
        return None, status, where
    idx = code_pixels(parent, length, last, off, f.w * f.h).reshape(f.h, f.w)
    if f.interlace:
        shown = np.empty_like(idx)
        shown[interlaced_rows(f.h)] = idx
        idx = shown
    return idx, OK, 0


def compose(info, planes) -> np.ndarray:
    """Stage C: planes[i] the indices (h, w) of frame i in display order -> uint8 (N, H, W, 3).  Raises the decoder's ValueError on an
    index beyond a palette."""
    canvas = np.zeros((info.height, info.width, 3), np.uint8)
    out = []
    for i, (f, idx) in enumerate(zip(info.frames, planes)):
        pal = np.frombuffer(f.palette, np.uint8).reshape(-1, 3)
        if int(idx.max()) >= len(pal):
            raise ValueError(f"frame {i}: status {BAD_INDEX}")
        view = canvas[f.y:f.y + f.h, f.x:f.x + f.w]
        keep = idx == f.transparent
        view[~keep] = pal[idx[~keep]]
        out.append(canvas.copy())
    return np.stack(out)


def decode(info) -> np.ndarray:
    planes = []
    for i, f in enumerate(info.frames):
        idx, status, where = frame_indices(f)
        if status:
            raise ValueError(f"frame {i}: status {status} at bit {where}")
        planes.append(idx)
    return compose(info, planes)


# ---- the cross-check: the classic decoder, a dictionary of byte strings
def classic_indices(stream: bytes, m: int, npix: int):
    """-> the indices in stream order (bytes, cut at npix), or None where the stream is broken or short."""
    bits, nbits = int.from_bytes(stream, "little"), 8 * len(stream)
    clear, eoi = 1 << m, (1 << m) + 1
    table = {i: bytes([i]) for i in range(clear)}
    nxt, width, prev, bp = clear + 2, m + 1, None, 0
    out = bytearray()
    while len(out) < npix:
        if bp + width > nbits:
            return None
        c = (bits >> bp) & ((1 << width) - 1)
        bp += width
        if c == clear:
            table = {i: bytes([i]) for i in range(clear)}
            nxt, width, prev = clear + 2, m + 1, None
            continue
        if c == eoi:
            return None
        if prev is None:
            if c >= clear:
                return None
            entry = table[c]
        else:
            if c in table:
                entry = table[c]
            elif c == nxt and nxt < 4096:
                entry = prev + prev[:1]
            else:
                return None
            if nxt < 4096:
                table[nxt] = prev + entry[:1]
                nxt += 1
                if nxt == (1 << width) and width < 12:
                    width += 1
        out += entry
        prev = entry
    return bytes(out[:npix])
