"""The JPEG decoder of ccedit_amd/csrc/jpegdec.hip restated in plain numpy / Python: a parsed stream in, the decoded frame out.
It is NORMATIVE for the GPU result (tests/test_jpegdec_gpu.py) and is itself held to Pillow byte for byte (tests/test_jpegdec.py).
The parser and the table layout come from ccedit_amd/jpegdec.py; none of the arithmetic does.

  entropy(info, data)       -> (coef int16 (blocks, 64): MCU order, natural order inside a block; status int32 (I,) per restart interval)
  idct(info, coef)          -> the component planes, uint8, padded to whole MCUs
  rgb(info, planes)         -> uint8 (H, W, 3): chroma up-sampling, YCbCr -> RGB
  decode(jpeg)              -> all three; a non-zero status is a ValueError
The statuses (and where an interval stops) are those of csrc/jpegdec_core.h: 1 invalid code, 2 data ends early, 3 coefficient index
passes 63, 4 DC size category above 11."""
import functools

import numpy as np

from ccedit_amd import jpegdec as J
from ccedit_amd.mjpeg import ZIGZAG

_ZZ = [int(z) for z in ZIGZAG]


@functools.lru_cache(maxsize=64)
def _lut16(bits, vals):
    """(BITS, HUFFVAL) -> list [65536]: length << 8 | symbol for the code the 16 bits start with, 0 if none does.  Read-only, and kept:
    most streams of a test share the standard tables."""
    lut = np.zeros(65536, np.int32)
    code, k = 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            lut[code << (16 - length):(code + 1) << (16 - length)] = (length << 8) | vals[k]
            code += 1
            k += 1
        code <<= 1
    return lut.tolist()


def _clean(seg):
    """The bytes the bit reader sees: FF 00 -> FF; an FF followed by anything else (or by nothing) ends the data."""
    a = np.frombuffer(seg, np.uint8)
    ff = np.flatnonzero(a == 0xFF)
    if len(ff):
        nxt = np.append(a, 1)[ff + 1]
        stop = ff[nxt != 0]
        if len(stop):
            a, ff = a[:stop[0]], ff[ff < stop[0]]
        a = np.delete(a, ff + 1)
    return a


def _decode_interval(seg, luts, info, n_mcus, out):
    """out: int16 (n_mcus * blocks_per_mcu, 64), zero on entry -> status."""
    a = _clean(seg)
    nbits = 8 * len(a)
    b = np.concatenate([a, np.zeros(8, np.uint8)]).astype(np.int64)
    win = ((b[:-3] << 24) | (b[1:-2] << 16) | (b[2:-1] << 8) | b[3:]).tolist()             # 32 bits from every byte
    p = 0
    bpm = info.blocks_per_mcu
    luma = bpm - 2
    pred = [0, 0, 0]
    for m in range(n_mcus):
        for j in range(bpm):
            c = 0 if info.ncomp == 1 or j < luma else j - luma + 1
            dc, ac = luts[info.dc_sel[c]], luts[2 + info.ac_sel[c]]
            blk = out[m * bpm + j]
            e = dc[(win[p >> 3] >> (16 - (p & 7))) & 0xFFFF]
            if e == 0:
                return 1
            p += e >> 8
            if p > nbits:
                return 2
            s = e & 255
            if s > 11:
                return 4
            d = 0
            if s:
                v = ((win[p >> 3] >> (16 - (p & 7))) & 0xFFFF) >> (16 - s)
                p += s
                if p > nbits:
                    return 2
                d = v if v >= (1 << (s - 1)) else v - (1 << s) + 1
            pred[c] = ((pred[c] + d + 32768) & 0xFFFF) - 32768
            blk[0] = pred[c]
            k = 1
            while k < 64:
                e = ac[(win[p >> 3] >> (16 - (p & 7))) & 0xFFFF]
                if e == 0:
                    return 1
                p += e >> 8
                if p > nbits:
                    return 2
                r, s = (e >> 4) & 15, e & 15
                if s == 0:
                    if r == 15:
                        k += 16
                        continue
                    break
                k += r
                if k > 63:
                    return 3
                v = ((win[p >> 3] >> (16 - (p & 7))) & 0xFFFF) >> (16 - s)
                p += s
                if p > nbits:
                    return 2
                blk[_ZZ[k]] = v if v >= (1 << (s - 1)) else v - (1 << s) + 1
                k += 1
    return 0


def entropy(info, data, intervals=None):
    """`intervals`: other [start, end) pairs than the parser found (the corruption tests cut and move them)."""
    luts = [_lut16(*h) if h is not None else None for h in info.huffman]
    iv = info.intervals if intervals is None else intervals
    coef = np.zeros((info.blocks, 64), np.int16)
    status = np.zeros(len(iv), np.int32)
    total, per, bpm = info.mcus_x * info.mcus_y, info.mcus_per_interval, info.blocks_per_mcu
    for i, (lo, hi) in enumerate(np.asarray(iv).tolist()):
        n = min(per, total - i * per)
        status[i] = _decode_interval(data[lo:hi], luts, info, n, coef[i * per * bpm:(i * per + n) * bpm])
    return coef, status


# ---- reconstruction: libjpeg's accurate integer inverse DCT ("islow"), 13-bit constants, 2 fraction bits after the first pass.
# All of it is int32 arithmetic modulo 2^32 (numpy wraps), as in the kernel; no stream an encoder writes comes near the wrap.
_F = dict(f0_298=2446, f0_390=3196, f0_541=4433, f0_765=6270, f0_899=7373, f1_175=9633, f1_501=12299, f1_847=15137, f1_961=16069,
          f2_053=16819, f2_562=20995, f3_072=25172)


def _pass(x, shift):
    """x: int32 (..., 8) along the last axis -> the 8 outputs, each rounded once: (v + 2^(shift - 1)) >> shift."""
    F = {k: np.int32(v) for k, v in _F.items()}
    i0, i1, i2, i3, i4, i5, i6, i7 = [x[..., i] for i in range(8)]
    z1 = (i2 + i6) * F["f0_541"]
    t2 = z1 - i6 * F["f1_847"]
    t3 = z1 + i2 * F["f0_765"]
    t0 = (i0 + i4) << 13
    t1 = (i0 - i4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = i7, i5, i3, i1
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * F["f1_175"]
    t0, t1, t2, t3 = t0 * F["f0_298"], t1 * F["f2_053"], t2 * F["f3_072"], t3 * F["f1_501"]
    z1, z2 = -z1 * F["f0_899"], -z2 * F["f2_562"]
    z3, z4 = z5 - z3 * F["f1_961"], z5 - z4 * F["f0_390"]
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    r = np.int32(1 << (shift - 1))
    outs = [t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3]
    return np.stack([(o + r) >> shift for o in outs], axis=-1)


def idct_blocks(coef, quant):
    """coef int16 (..., 64) natural order, quant (64,) -> uint8 (..., 8, 8)."""
    with np.errstate(over="ignore"):
        x = (coef.astype(np.int32) * quant.astype(np.int32)).reshape(coef.shape[:-1] + (8, 8))
        ws = _pass(np.swapaxes(x, -1, -2), 11)              # columns: ws[..., col, row]
        o = _pass(np.swapaxes(ws, -1, -2), 18)              # rows: o[..., row, col]
    v = ((o & 1023) ^ 512) - 512                            # the low 10 bits as a signed value: libjpeg's range-limit table, with
    return np.clip(v + 128, 0, 255).astype(np.uint8)        # the + 128 and the clamp


def idct(info, coef):
    mx, my, bpm = info.mcus_x, info.mcus_y, info.blocks_per_mcu
    c = coef.reshape(my, mx, bpm, 64)
    if info.ncomp == 1:
        return [idct_blocks(c[:, :, 0], info.quant[0]).transpose(0, 2, 1, 3).reshape(my * 8, mx * 8)]
    hs, vs = info.hs, info.vs
    y = idct_blocks(c[:, :, :hs * vs].reshape(my, mx, vs, hs, 64), info.quant[0])            # (my, mx, vs, hs, 8, 8)
    y = y.transpose(0, 2, 4, 1, 3, 5).reshape(my * vs * 8, mx * hs * 8)
    return [y] + [idct_blocks(c[:, :, hs * vs + i], info.quant[1 + i]).transpose(0, 2, 1, 3).reshape(my * 8, mx * 8) for i in range(2)]


def upsample(plane, hs, vs, h, w):
    """One chroma plane (padded) -> int64 (h, w) at the luma's size: libjpeg's "fancy" triangle filters; a plane of at most two real
    columns is replicated instead, as libjpeg does."""
    ch, cw = -(-h // vs), -(-w // hs)
    p = plane[:ch, :cw].astype(np.int64)
    if hs == 1:
        return p[:h, :w]
    if cw <= 2:
        return np.repeat(np.repeat(p, vs, axis=0), 2, axis=1)[:h, :w]
    if vs == 2:
        up, dn = np.concatenate([p[:1], p[:-1]]), np.concatenate([p[1:], p[-1:]])
        s = np.empty((2 * ch, cw), np.int64)
        s[0::2], s[1::2] = 3 * p + up, 3 * p + dn                                    # the vertical pass: 3 near + far
        a, r0, r1, edge, sh = 3, 8, 7, 4, 4
    else:
        s, a, r0, r1, edge, sh = p, 3, 1, 2, 4, 2
    left = np.concatenate([s[:, :1], s[:, :-1]], axis=1)
    right = np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
    out = np.empty((s.shape[0], 2 * cw), np.int64)
    out[:, 0::2] = (a * s + left + r0) >> sh
    out[:, 1::2] = (a * s + right + r1) >> sh
    if vs == 2:
        out[:, 0], out[:, -1] = (edge * s[:, 0] + r0) >> sh, (edge * s[:, -1] + r1) >> sh
    else:
        out[:, 0], out[:, -1] = s[:, 0], s[:, -1]
    return out[:h, :w]


def rgb(info, planes):
    h, w = info.height, info.width
    y = planes[0][:h, :w].astype(np.int64)
    if info.ncomp == 1:
        return np.repeat(y[..., None], 3, axis=2).astype(np.uint8)
    cb = upsample(planes[1], info.hs, info.vs, h, w) - 128
    cr = upsample(planes[2], info.hs, info.vs, h, w) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb + 32768 - 46802 * cr) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=2), 0, 255).astype(np.uint8)


def decode(jpeg):
    info = J.parse(jpeg)
    coef, status = entropy(info, jpeg)
    bad = np.flatnonzero(status)
    if len(bad):
        raise ValueError(f"restart interval {int(bad[0])}: {J.STATUS_TEXT[int(status[bad[0]])]}")
    return rgb(info, idct(info, coef))
