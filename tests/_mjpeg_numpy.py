"""The Motion-JPEG encoder of ccedit_amd/csrc/mjpeg.hip restated in plain numpy / Python: pixels in, the exact bytes of each frame out.
It is NORMATIVE: the GPU result is these bytes (tests/test_mjpeg_gpu.py), and what these bytes are worth is checked on the CPU
(tests/test_mjpeg.py: Pillow decodes them, fidelity against Pillow's own encoder).  The tables and factors come from
ccedit_amd/mjpeg.py, their one place; none of the arithmetic does.

  transform(frames, q)      uint8 (N, H, W, 3) -> int16 (N, H / 16, W / 16, 6, 64): per MCU Y00 Y01 Y10 Y11 Cb Cr, each block in zigzag order
  code_interval(blocks)     one MCU row's blocks (nb, 64) -> the stuffed, padded entropy-coded bytes of its restart interval
  encode_frames(frames, q)  -> list of complete JPEG files
A `trace` dict, when given, counts what was coded: 'zrl' and 'eob' symbols, 'stuffed' bytes."""
import numpy as np

from ccedit_amd import mjpeg as M


def scaled_quant(quality):
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return [np.clip((base.astype(np.int64) * s + 50) // 100, 1, 255) for base in (M.QUANT_LUMA, M.QUANT_CHROMA)]


def planes(frames):
    """-> level-shifted Y (N, H, W), Cb and Cr (N, H / 2, W / 2), int64."""
    x = frames.astype(np.int64)
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    c = M.COLOR.astype(np.int64)
    y = (c[0] * r + c[1] * g + c[2] * b + (1 << 15)) >> 16
    s4 = lambda p: p[:, 0::2, 0::2] + p[:, 0::2, 1::2] + p[:, 1::2, 0::2] + p[:, 1::2, 1::2]
    rs, gs, bs = s4(r), s4(g), s4(b)
    cb = (c[3] * rs + c[4] * gs + c[5] * bs + (128 << 18) + (1 << 17) - 1) >> 18
    cr = (c[6] * rs + c[7] * gs + c[8] * bs + (128 << 18) + (1 << 17) - 1) >> 18
    return y - 128, cb - 128, cr - 128


def fdct_quant(blocks, quant):
    """(..., 8, 8) level-shifted samples [y][x], quant row-major (64,) -> (..., 64) quantised coefficients in zigzag order."""
    d = M.DCT.astype(np.int64)
    rows = (np.einsum("ux,...yx->...yu", d, blocks) + (1 << (M.DCT_ROW_SHIFT - 1))) >> M.DCT_ROW_SHIFT
    f = np.einsum("vy,...yu->...vu", d, rows).reshape(blocks.shape[:-2] + (64,))
    q = quant.astype(np.int64)
    mag = ((np.abs(f) + (q << (M.DCT_OUT_BITS - 1))) >> M.DCT_OUT_BITS) // q
    mag[..., 1:] = np.minimum(mag[..., 1:], M.AC_MAX)
    return (np.sign(f) * mag)[..., M.ZIGZAG]


def transform(frames, quality):
    n, h, w, _ = frames.shape
    assert h % 16 == 0 and w % 16 == 0
    ql, qc = scaled_quant(quality)
    y, cb, cr = planes(frames)
    mr, mc = h // 16, w // 16
    yb = y.reshape(n, mr, 2, 8, mc, 2, 8).transpose(0, 1, 4, 2, 5, 3, 6).reshape(n, mr, mc, 4, 8, 8)       # (by, bx) -> Y00 Y01 Y10 Y11
    cbb = cb.reshape(n, mr, 8, mc, 8).transpose(0, 1, 3, 2, 4)
    crb = cr.reshape(n, mr, 8, mc, 8).transpose(0, 1, 3, 2, 4)
    out = np.empty((n, mr, mc, 6, 64), np.int16)
    out[..., :4, :] = fdct_quant(yb, ql)
    out[..., 4, :] = fdct_quant(cbb, qc)
    out[..., 5, :] = fdct_quant(crb, qc)
    return out


def _value_bits(v, size):
    return (v if v > 0 else v + (1 << size) - 1) & ((1 << size) - 1)


def block_symbols(block, pred, comp, trace=None):
    """One block (64 coefficients in zigzag order) -> list of (bits, length)."""
    out = []
    d = int(np.clip(int(block[0]) - pred, -M.DC_DIFF_MAX, M.DC_DIFF_MAX))
    s = abs(d).bit_length()
    e = int(M.DC_CODES[comp][s])
    out.append((((e >> 8) << s) | _value_bits(d, s), (e & 255) + s))
    ac_codes = M.AC_CODES[comp]
    last = 0
    for k in np.flatnonzero(block[1:]) + 1:
        v = int(np.clip(int(block[k]), -M.AC_MAX, M.AC_MAX))
        run = int(k) - last - 1
        while run >= 16:
            e = int(ac_codes[0xF0])
            out.append((e >> 8, e & 255))
            run -= 16
            if trace is not None:
                trace["zrl"] = trace.get("zrl", 0) + 1
        s = abs(v).bit_length()
        e = int(ac_codes[(run << 4) | s])
        out.append((((e >> 8) << s) | _value_bits(v, s), (e & 255) + s))
        last = int(k)
    if last != 63:
        e = int(ac_codes[0])
        out.append((e >> 8, e & 255))
        if trace is not None:
            trace["eob"] = trace.get("eob", 0) + 1
    return out


def code_interval(blocks, trace=None):
    """blocks (nb, 64) of one MCU row in MCU order -> bytes: DC predictors start at 0, bits MSB first, padded with ones, FF -> FF 00."""
    pred = [0, 0, 0]
    syms = []
    for i, blk in enumerate(blocks):
        j = i % 6
        c = 0 if j < 4 else j - 3
        syms += block_symbols(blk, pred[c], int(c > 0), trace)
        pred[c] = int(blk[0])
    codes = np.array([s[0] for s in syms], np.int64)
    lens = np.array([s[1] for s in syms], np.int64)
    total = int(lens.sum())
    start = np.repeat(np.cumsum(lens) - lens, lens)
    j = np.arange(total) - start
    bits = ((np.repeat(codes, lens) >> (np.repeat(lens, lens) - 1 - j)) & 1).astype(np.uint8)
    bits = np.concatenate([bits, np.ones((-total) % 8, np.uint8)])
    raw = np.packbits(bits)
    ff = np.flatnonzero(raw == 0xFF)
    if trace is not None:
        trace["stuffed"] = trace.get("stuffed", 0) + len(ff)
    return np.insert(raw, ff + 1, 0).tobytes()


def interval_bytes(coef, trace=None):
    """coef (N, MR, MC, 6, 64) -> [frame][MCU row] bytes."""
    n, mr = coef.shape[:2]
    return [[code_interval(coef[f, r].reshape(-1, 64), trace) for r in range(mr)] for f in range(n)]


def assemble(header, segments):
    out = [header]
    for r, seg in enumerate(segments):
        out.append(seg)
        out.append(bytes([0xFF, 0xD0 + (r & 7)]) if r + 1 < len(segments) else b"\xff\xd9")
    return b"".join(out)


def encode_frames(frames, quality=M.DEFAULT_QUALITY, trace=None):
    frames = np.asarray(frames)
    assert frames.dtype == np.uint8 and frames.ndim == 4 and frames.shape[3] == 3
    header = M.frame_header(frames.shape[1], frames.shape[2], quality)
    return [assemble(header, segs) for segs in interval_bytes(transform(frames, quality), trace)]
