"""JPEG sources decoded on the GPU: a baseline JPEG decoder in three stages (ccedit_amd/csrc/jpegdec.hip),
the stages of the encoder of ccedit_amd/mjpeg.py in reverse.  The frames equal Pillow's (libjpeg-turbo: accurate integer IDCT, "fancy"
chroma up-sampling, 16-bit fixed-point YCbCr -> RGB) byte for byte, so this route and the host route are interchangeable.

  parse(data)            the stream, on the host: markers, tables and where every restart interval's entropy-coded bytes lie.  No pixel
                         arithmetic.  What is outside the subset below is a JpegUnsupported that names the reason, before any launch.
  decode(jpegs, device)  compressed bytes in, uint8 (N, H, W, 3) on the device out: entropy stage (bytes -> int16 coefficients, one thread
                         per restart interval), reconstruction (dequantisation + 8 x 8 inverse DCT -> component planes), colour (chroma
                         up-sampling + YCbCr -> RGB).  Frames of one call that share geometry and tables go through one launch per stage.

The subset: baseline sequential DCT (SOF0), 8 bit, Huffman, ONE scan with all components; greyscale, or YCbCr with luma sampling 1x1, 2x1
or 2x2 and chroma 1x1 (4:4:4, 4:2:2, 4:2:0); any 8-bit quantisation tables, any Huffman tables, any restart interval or none; H and W
1 ... 65520.  A file without restart markers is ONE interval per frame: it decodes correctly, with one thread per frame in the entropy
stage (the other two stages are as parallel as ever).  tests/_jpegdec_numpy.py restates the three stages in numpy.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .codec_common import launch_groups, parsed, per_launch
from .mjpeg import ZIGZAG

MAX_DIM = 65520
# ---- the int32 table the kernels read (include/ccedit_hip.h, "JPEG decoding"; csrc/jpegdec_core.h)
LUT_BITS = 9                                 # codes of up to 9 bits are one lookup: length << 8 | symbol (0: longer, or no code)
HUFF_LUT, HUFF_MAXCODE, HUFF_VALOFF, HUFF_VALS, HUFF_STRIDE = 0, 512, 530, 548, 804
#                                              per table: lut [512], maxcode [18] (by length, -1: no code of that length),
#                                              valoff [18] (index of the length's first value - its first code), vals [256]
TAB_QUANT, TAB_SEL, TAB_HUFF, TAB_SIZE = 0, 192, 200, 200 + 4 * HUFF_STRIDE
#                                              quant [3][64] per COMPONENT in natural order; sel [6]: DC table of component 0 1 2, AC table
#                                              of component 0 1 2 (0 or 1); the tables DC 0, DC 1, AC 0, AC 1

STATUS_TEXT = {1: "invalid Huffman code", 2: "the entropy-coded data ends before the interval's blocks do",
               3: "a coefficient index passes 63", 4: "invalid DC size category"}

MAX_FRAMES_PER_LAUNCH = 256
SCRATCH_BYTES = 256 << 20          # frames per launch are chosen so that coefficients + planes stay below this; results do not depend on it


class JpegUnsupported(ValueError):
    """The stream is outside the subset the device decodes (or is not a complete JPEG): the message names the reason."""


@dataclass
class JpegInfo:
    height: int
    width: int
    ncomp: int                     # 1 (greyscale) or 3 (YCbCr)
    hs: int                        # luma sampling factors (1, 1 for greyscale: a one-component scan is not interleaved)
    vs: int
    restart_interval: int          # MCUs per restart interval (DRI); 0: none
    quant: np.ndarray              # uint8 (ncomp, 64) per component, natural (row-major) order
    huffman: Tuple[Optional[Tuple[bytes, bytes]], ...]      # (BITS, HUFFVAL) of DC 0, DC 1, AC 0, AC 1; None: not defined
    dc_sel: Tuple[int, ...]        # per component: which DC / AC table
    ac_sel: Tuple[int, ...]
    intervals: np.ndarray          # int64 (I, 2): [start, end) of each restart interval's entropy-coded bytes in the file

    @property
    def mcus_x(self) -> int:
        return -(-self.width // (8 * self.hs))

    @property
    def mcus_y(self) -> int:
        return -(-self.height // (8 * self.vs))

    @property
    def blocks_per_mcu(self) -> int:
        return 1 if self.ncomp == 1 else self.hs * self.vs + 2

    @property
    def mcus_per_interval(self) -> int:
        return self.restart_interval or self.mcus_x * self.mcus_y

    @property
    def blocks(self) -> int:
        return self.mcus_x * self.mcus_y * self.blocks_per_mcu

    def key(self):
        """Frames with equal keys decode in one launch per stage: geometry, restart interval and every table."""
        return (self.height, self.width, self.ncomp, self.hs, self.vs, self.restart_interval, len(self.intervals), self.quant.tobytes(),
                self.huffman, self.dc_sel, self.ac_sel)


def huffman_table(bits: bytes, vals: bytes) -> np.ndarray:
    """(BITS, HUFFVAL) -> int32 [HUFF_STRIDE] as the kernel reads it (Annex C codes; layout at HUFF_*)."""
    t = np.zeros(HUFF_STRIDE, np.int32)
    t[HUFF_MAXCODE:HUFF_MAXCODE + 18] = -1
    t[HUFF_VALS:HUFF_VALS + len(vals)] = np.frombuffer(vals, np.uint8)
    code, k = 0, 0
    for length in range(1, 17):
        n = bits[length - 1]
        if n:
            if code + n > (1 << length):
                raise JpegUnsupported(f"bad Huffman table: more codes of {length} bits than the code space holds")
            t[HUFF_VALOFF + length] = k - code
            t[HUFF_MAXCODE + length] = code + n - 1
            if length <= LUT_BITS:
                for i in range(n):
                    lo = (code + i) << (LUT_BITS - length)
                    t[HUFF_LUT + lo:HUFF_LUT + lo + (1 << (LUT_BITS - length))] = (length << 8) | vals[k + i]
            code += n
            k += n
        code <<= 1
    return t


def table_array(info: JpegInfo) -> np.ndarray:
    """Everything the kernels need beside geometry: int32 [TAB_SIZE] (layout at TAB_*)."""
    t = np.zeros(TAB_SIZE, np.int32)
    t[TAB_QUANT:TAB_QUANT + 64 * info.ncomp] = info.quant.reshape(-1)
    t[TAB_SEL:TAB_SEL + info.ncomp] = info.dc_sel
    t[TAB_SEL + 3:TAB_SEL + 3 + info.ncomp] = info.ac_sel
    for i, h in enumerate(info.huffman):
        if h is not None:
            t[TAB_HUFF + i * HUFF_STRIDE:TAB_HUFF + (i + 1) * HUFF_STRIDE] = huffman_table(*h)
    return t


_SOF_REFUSED = {0xC1: "extended sequential DCT (SOF1)", 0xC2: "progressive JPEG (SOF2)", 0xC3: "lossless JPEG (SOF3)",
                0xC5: "differential sequential DCT (SOF5)", 0xC6: "differential progressive DCT (SOF6)", 0xC7: "differential lossless (SOF7)",
                0xC9: "arithmetic coding (SOF9)", 0xCA: "arithmetic coding (SOF10, progressive)", 0xCB: "arithmetic coding (SOF11, lossless)",
                0xCD: "arithmetic coding (SOF13)", 0xCE: "arithmetic coding (SOF14)", 0xCF: "arithmetic coding (SOF15)",
                0xCC: "arithmetic coding (DAC)"}


def parse(data: bytes) -> JpegInfo:
    """One JPEG file -> JpegInfo, or JpegUnsupported naming why the device does not decode it."""
    data = bytes(data)
    n = len(data)
    if n < 4 or data[:2] != b"\xff\xd8":
        raise JpegUnsupported("not a JPEG file (no SOI marker)")
    quant = {}
    huff: List[Optional[Tuple[bytes, bytes]]] = [None] * 4
    sof = sos = None
    restart = 0
    jfif, adobe = False, None
    pos = 2
    while sos is None:
        if pos + 2 > n:
            raise JpegUnsupported("truncated file (it ends before the scan)")
        if data[pos] != 0xFF:
            raise JpegUnsupported(f"bytes that are no marker segment at offset {pos}")
        m = data[pos + 1]
        if m == 0xFF:                            # fill byte
            pos += 1
            continue
        pos += 2
        if m == 0xD8 or m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if m == 0xD9:
            raise JpegUnsupported("no scan (EOI before SOS)")
        if pos + 2 > n:
            raise JpegUnsupported("truncated file (inside a marker segment)")
        length = struct.unpack_from(">H", data, pos)[0]
        if length < 2 or pos + length > n:
            raise JpegUnsupported("truncated file (a marker segment runs past its end)")
        seg = data[pos + 2:pos + length]
        pos += length
        if m in _SOF_REFUSED:
            raise JpegUnsupported(_SOF_REFUSED[m])
        if m == 0xC0:
            if sof is not None:
                raise JpegUnsupported("more than one frame header (SOF)")
            if len(seg) < 6 or len(seg) != 6 + 3 * seg[5]:
                raise JpegUnsupported("bad frame header (SOF0 length)")
            if seg[0] != 8:
                raise JpegUnsupported(f"{seg[0]} bit samples (only 8 bit)")
            h, w, nc = struct.unpack_from(">HHB", seg, 1)
            if nc == 4:
                raise JpegUnsupported("4 components (CMYK / YCCK)")
            if nc not in (1, 3):
                raise JpegUnsupported(f"{nc} components (only greyscale and YCbCr)")
            if not (1 <= h <= MAX_DIM and 1 <= w <= MAX_DIM):
                raise JpegUnsupported(f"size {h}x{w} (H and W 1 ... {MAX_DIM})")
            sof = (h, w, [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(nc)])
        elif m == 0xDB:
            at = 0
            while at < len(seg):
                pq, tq = seg[at] >> 4, seg[at] & 15
                if pq != 0:
                    raise JpegUnsupported("16-bit quantisation table entries")
                if tq > 3 or at + 65 > len(seg):
                    raise JpegUnsupported("bad quantisation table segment (DQT)")
                q = np.zeros(64, np.uint8)
                q[ZIGZAG] = np.frombuffer(seg[at + 1:at + 65], np.uint8)
                quant[tq] = q
                at += 65
        elif m == 0xC4:
            at = 0
            while at < len(seg):
                if at + 17 > len(seg):
                    raise JpegUnsupported("bad Huffman table segment (DHT)")
                tc, th = seg[at] >> 4, seg[at] & 15
                bits = seg[at + 1:at + 17]
                nv = sum(bits)
                if tc > 1 or th > 1:
                    raise JpegUnsupported(f"Huffman table class {tc} id {th} (baseline: class 0 / 1, id 0 / 1)")
                if nv > 256 or at + 17 + nv > len(seg):
                    raise JpegUnsupported("bad Huffman table segment (DHT)")
                vals = seg[at + 17:at + 17 + nv]
                huffman_table(bits, vals)                     # (refuses an over-full code)
                huff[2 * tc + th] = (bits, vals)
                at += 17 + nv
        elif m == 0xDD:
            if len(seg) != 2:
                raise JpegUnsupported("bad restart interval segment (DRI)")
            restart = struct.unpack(">H", seg)[0]
        elif m == 0xE0 and seg[:5] == b"JFIF\x00":
            jfif = True
        elif m == 0xEE and seg[:5] == b"Adobe" and len(seg) >= 12:
            adobe = seg[11]
        elif m == 0xDA:
            sos = seg
        elif m == 0xDC:
            raise JpegUnsupported("DNL marker (the number of lines defined after the scan)")
        # every other segment (APPn, COM, ...) is skipped
    if sof is None:
        raise JpegUnsupported("no frame header (SOF0) before the scan")
    h, w, comps = sof
    nc = len(comps)
    if len(sos) < 1 or len(sos) != 4 + 2 * sos[0]:
        raise JpegUnsupported("bad scan header (SOS length)")
    if sos[0] != nc:
        raise JpegUnsupported(f"multiple scans (the first holds {sos[0]} of {nc} components)")
    if [sos[1 + 2 * i] for i in range(nc)] != [c[0] for c in comps]:
        raise JpegUnsupported("scan components are not the frame's, in its order")
    if (sos[1 + 2 * nc], sos[2 + 2 * nc], sos[3 + 2 * nc]) != (0, 63, 0):
        raise JpegUnsupported("scan header with spectral selection / successive approximation (not baseline)")
    dc_sel = tuple(sos[2 + 2 * i] >> 4 for i in range(nc))
    ac_sel = tuple(sos[2 + 2 * i] & 15 for i in range(nc))
    if nc == 3:
        if not jfif:
            if adobe is not None and adobe != 1:
                raise JpegUnsupported(f"Adobe colour transform {adobe} (only YCbCr)")
            if adobe is None and [c[0] for c in comps] == [82, 71, 66]:
                raise JpegUnsupported("components R, G, B without a colour transform (only YCbCr)")
        samp = [(c[1], c[2]) for c in comps]
        if samp[0] not in ((1, 1), (2, 1), (2, 2)) or samp[1] != (1, 1) or samp[2] != (1, 1):
            raise JpegUnsupported("sampling " + " ".join(f"{a}x{b}" for a, b in samp) + " (only 4:4:4, 4:2:2 and 4:2:0)")
        hs, vs = samp[0]
    else:
        if not 1 <= comps[0][1] <= 4 or not 1 <= comps[0][2] <= 4:
            raise JpegUnsupported("bad sampling factors")
        hs = vs = 1
    for i, c in enumerate(comps):
        if c[3] not in quant:
            raise JpegUnsupported(f"missing quantisation table {c[3]}")
        if dc_sel[i] > 1 or ac_sel[i] > 1:
            raise JpegUnsupported("scan selects a Huffman table id above 1 (not baseline)")
        if huff[dc_sel[i]] is None:
            raise JpegUnsupported(f"missing Huffman table (DC {dc_sel[i]})")
        if huff[2 + ac_sel[i]] is None:
            raise JpegUnsupported(f"missing Huffman table (AC {ac_sel[i]})")
    info = JpegInfo(h, w, nc, hs, vs, restart, np.stack([quant[c[3]] for c in comps]), tuple(huff), dc_sel, ac_sel, np.zeros((0, 2), np.int64))

    # ---- the entropy-coded data: every FF that is not FF 00 is a restart marker, a fill byte or the end of the scan
    a = np.frombuffer(data, np.uint8)[pos:]
    nxt = np.full(len(a), -1, np.int64)                          # (-1: FF as the last byte of the file)
    nxt[:-1] = a[1:]
    marks = np.flatnonzero((a == 0xFF) & (nxt != 0))
    intervals, start, fill, prev, done = [], pos, None, None, False
    for i in marks.tolist():
        m = int(nxt[i])
        if fill is not None and i != prev + 1:
            raise JpegUnsupported("FF fill bytes inside the entropy-coded data")
        prev = i
        if m < 0:
            break
        if m == 0xFF:
            fill = i if fill is None else fill
            continue
        end = pos + (i if fill is None else fill)
        fill = None
        if 0xD0 <= m <= 0xD7:
            if m - 0xD0 != len(intervals) & 7:
                raise JpegUnsupported(f"restart marker {m - 0xD0} where {len(intervals) & 7} is due")
            intervals.append((start, end))
            start = pos + i + 2
            continue
        intervals.append((start, end))
        if m == 0xD9:
            done = True
        elif m == 0xDA:
            raise JpegUnsupported("multiple scans")
        else:
            raise JpegUnsupported(f"marker FF {m:02X} after the scan where EOI is due (multiple scans or tables between them)")
        break
    if not done:
        raise JpegUnsupported("truncated file (no EOI after the entropy-coded data)")
    total = info.mcus_x * info.mcus_y
    want = -(-total // info.mcus_per_interval)
    if len(intervals) != want:
        raise JpegUnsupported(f"{len(intervals)} restart intervals in the scan where {want} are due")
    info.intervals = np.asarray(intervals, np.int64).reshape(-1, 2)
    return info


# ------------------------------------------------------------------------------------------
# the decoder: three stages on the device (ops.jpegdec_*), only the compressed bytes go up
# ------------------------------------------------------------------------------------------
def pack_group(infos: Sequence[JpegInfo], jpegs: Sequence[bytes]):
    """Frames of one key -> (data uint8: their entropy-coded bytes back to back, intervals int64 (N * I, 2) into it, tables int32)."""
    parts, ivs, at = [], [], 0
    for info, j in zip(infos, jpegs):
        lo, hi = int(info.intervals[0, 0]), int(info.intervals[-1, 1])
        parts.append(np.frombuffer(j, np.uint8)[lo:hi])
        ivs.append(info.intervals - lo + at)
        at += hi - lo
    data = np.concatenate(parts) if at else np.zeros(0, np.uint8)
    return np.ascontiguousarray(data), np.ascontiguousarray(np.concatenate(ivs)), table_array(infos[0])


def frame_scratch_bytes(info: JpegInfo) -> int:
    from . import ops
    return info.blocks * 128 + ops.jpegdec_plane_bytes(info.height, info.width, info.ncomp, info.hs, info.vs)


def _groups(infos: Sequence[JpegInfo]):
    """Indices of the frames per key, in the order the keys first appear, cut into launches under the scratch bound."""
    by_key = {}
    for i, info in enumerate(infos):
        by_key.setdefault(info.key(), []).append(i)
    for idx in by_key.values():
        for g in launch_groups(len(idx), per_launch(MAX_FRAMES_PER_LAUNCH, SCRATCH_BYTES, frame_scratch_bytes(infos[idx[0]]))):
            yield idx[g]


def _entropy(infos, jpegs, idx, device):
    """-> (coef int16 (n, blocks, 64), status int32 (n, I), tables) on the device for the frames `idx` of one key."""
    import torch
    from . import ops
    info = infos[idx[0]]
    data, ivs, tab = pack_group([infos[i] for i in idx], [jpegs[i] for i in idx])
    if data.size == 0:
        data = np.zeros(1, np.uint8)
    data_d = torch.from_numpy(data).to(device)
    ivs_d = torch.from_numpy(ivs).to(device)
    tab_d = torch.from_numpy(tab).to(device)
    coef, status = ops.jpegdec_entropy(data_d, ivs_d, tab_d, len(idx), info.height, info.width, info.ncomp, info.hs, info.vs,
                                       info.restart_interval)
    return coef, status, tab_d


def _raise_status(status, idx) -> None:
    bad = np.argwhere(status != 0)
    if len(bad):
        f, j = int(bad[0, 0]), int(bad[0, 1])
        code = int(status[f, j])
        raise ValueError(f"frame {idx[f]}, restart interval {j}: {STATUS_TEXT.get(code, f'status {code}')}")


def decode_coefficients(jpegs: Sequence[bytes], device, check: bool = True, infos: Optional[Sequence[JpegInfo]] = None):
    """The entropy stage alone -> per frame (coef int16 (blocks, 64) in MCU order, natural order inside a block; status int32 (I,)),
    both on the host.  check=False hands the status words back instead of raising."""
    infos = parsed(jpegs, infos, parse)
    out = [None] * len(jpegs)
    for idx in _groups(infos):
        coef, status, _ = _entropy(infos, jpegs, idx, device)
        coef, status = coef.cpu().numpy(), status.cpu().numpy()
        if check:
            _raise_status(status, idx)
        for k, i in enumerate(idx):
            out[i] = (coef[k], status[k])
    return out


def decode(jpegs: Sequence[bytes], device, infos: Optional[Sequence[JpegInfo]] = None):
    """N JPEG files (bytes) of one size -> uint8 (N, H, W, 3) on `device`.  `infos`: their parse() results, when the caller has them
    already (each file is then parsed once).  JpegUnsupported: a file outside the subset (nothing was launched);
    ValueError("frame i, restart interval j: ..."): its entropy-coded data is corrupt.  Pillow decodes such a file with a warning (it
    feeds zeros after a premature end and resynchronises at the next restart marker); this decoder stops and says where."""
    import torch
    from . import ops
    if len(jpegs) < 1:
        raise ValueError("decode: no frames")
    infos = parsed(jpegs, infos, parse)
    sizes = {(i.height, i.width) for i in infos}
    if len(sizes) != 1:
        raise ValueError(f"decode: frames of different sizes {sorted(sizes)}")
    h, w = infos[0].height, infos[0].width
    out = None                                                 # allocated only when more than one launch is made
    for idx in _groups(infos):
        info = infos[idx[0]]
        coef, status, tab_d = _entropy(infos, jpegs, idx, device)
        planes = ops.jpegdec_idct(coef, tab_d, h, w, info.ncomp, info.hs, info.vs)
        rgb = ops.jpegdec_rgb(planes, h, w, info.ncomp, info.hs, info.vs)
        _raise_status(status.cpu().numpy(), idx)               # (the one synchronisation per launch)
        if len(idx) == len(jpegs):
            return rgb
        if out is None:
            out = torch.empty((len(jpegs), h, w, 3), dtype=torch.uint8, device=device)
        if idx == list(range(idx[0], idx[0] + len(idx))):
            out[idx[0]:idx[0] + len(idx)] = rgb
        else:
            out[torch.as_tensor(idx, device=device)] = rgb
    return out
