"""Motion-JPEG video output (`--save_type mjpeg`): a baseline JPEG encoder on the GPU
(ccedit_amd/csrc/mjpeg.hip) and the AVI container around it, written and read here.

One JPEG per frame: baseline sequential DCT (ITU-T T.81), 8 bit, YCbCr (JFIF full range) 4:2:0, MCU 16 x 16, the Annex K quantisation
tables scaled by the usual quality rule, the four "typical" Annex K Huffman tables, a restart interval of one MCU row.  All arithmetic
is integer; the frames the kernels produce equal the numpy restatement the tests carry (tests/_mjpeg_numpy.py) byte for byte, and
there is no host fallback.  This module is the ONE place of the constants: the fixed-point factors, the tables and the header bytes.
The kernels receive them as one int32 table (device_tables); the restatement imports them from here.

The container is RIFF `AVI ` with one `MJPG` video stream, one `00dc` chunk per frame and an `idx1` index; read_avi walks the same
structure, which is how an .avi becomes a video SOURCE of the entry points: decode_avi_u8 hands the chunks to Pillow on the host,
decode_avi_device to the decoder on the GPU (ccedit_amd/jpegdec.py) — the same frames, byte for byte.
"""
from __future__ import annotations

import os
import struct
from typing import List, Sequence, Tuple

import numpy as np

from .codec_common import launch_groups, per_launch, split_bytes

# ---- the constants of the format: this is their one place
MCU = 16                    # 4:2:0: four Y blocks, one Cb, one Cr per 16 x 16 pixels
BLOCKS_PER_MCU = 6
DEFAULT_QUALITY = 90
COLOR_BITS = 16             # colour conversion: 16-bit fixed point
#                             Y  = (19595 R + 38470 G +  7471 B + 2^15) >> 16                        (0.299, 0.587, 0.114)
#                             Cb = (-11059 Rs - 21709 Gs + 32768 Bs + (128 << 18) + 2^17 - 1) >> 18     Rs, Gs, Bs: sums over the 2 x 2 pixels,
#                             Cr = ( 32768 Rs - 27439 Gs -  5329 Bs + (128 << 18) + 2^17 - 1) >> 18     so the rounded mean is ONE rounding
COLOR = np.array([19595, 38470, 7471, -11059, -21709, 32768, 32768, -27439, -5329], np.int32)
DCT_BITS = 13               # FDCT matrix C[u][x] = round(2^13 c(u) / 2 cos((2 x + 1) u pi / 16)), c(0) = 1 / sqrt 2
DCT_ROW_SHIFT = 8           # the row pass keeps 13 - 8 = 5 fraction bits: t = (sum_x C[u][x] p[x] + 2^7) >> 8
DCT_OUT_BITS = 2 * DCT_BITS - DCT_ROW_SHIFT       # = 18 fraction bits of the column pass's sums; quantisation rounds once:
#                             q = sign(F) ((|F| + (Q << 17)) >> 18) / Q     (exact: floor(a / (Q 2^18)) = floor(floor(a / 2^18) / Q))
AC_MAX = 1023               # what baseline Huffman coding can carry (size <= 10)
DC_DIFF_MAX = 2047          # (size <= 11)
MAX_BLOCK_BITS = 63 * 26 + 27       # 63 AC coefficients of 16 + 10 bits, a DC difference of 16 + 11: whatever the code tables hold
MAX_RIFF_BYTES = 2 ** 31 - 1        # no OpenDML: one RIFF chunk

DCT = np.array([[int(np.floor((2 ** DCT_BITS) * (np.sqrt(0.5) if u == 0 else 1.0) / 2.0 * np.cos((2 * x + 1) * u * np.pi / 16.0) + 0.5))
                 for x in range(8)] for u in range(8)], np.int32)

QUANT_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                       14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                       49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], np.int32)            # Annex K.1, row-major
QUANT_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                         47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32, np.int32)                                      # Annex K.2
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62,
                   63], np.int32)           # position in the scan -> row-major index

# Annex K.3: BITS (codes per length 1 ... 16) and HUFFVAL of the four typical tables
DC_LUMA_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
DC_CHROMA_BITS = [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
DC_VALS = list(range(12))
AC_LUMA_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D]
AC_LUMA_VALS = [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1,
    0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26,
    0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56,
    0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85,
    0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA,
    0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6,
    0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9,
    0xFA]
AC_CHROMA_BITS = [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]
AC_CHROMA_VALS = [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
    0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19,
    0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55,
    0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8,
    0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4,
    0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9,
    0xFA]
HUFFMAN = (("dc", 0, DC_LUMA_BITS, DC_VALS), ("ac", 0, AC_LUMA_BITS, AC_LUMA_VALS),
           ("dc", 1, DC_CHROMA_BITS, DC_VALS), ("ac", 1, AC_CHROMA_BITS, AC_CHROMA_VALS))       # in the order DHT carries them


def huffman_codes(bits: Sequence[int], vals: Sequence[int]) -> np.ndarray:
    """Annex C: int32 [256] indexed by symbol, code << 8 | length (0: the symbol has no code)."""
    assert len(bits) == 16 and sum(bits) == len(vals)
    tab = np.zeros(256, np.int32)
    code, k = 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            tab[vals[k]] = (code << 8) | length
            code += 1
            k += 1
        code <<= 1
    return tab


DC_CODES = (huffman_codes(DC_LUMA_BITS, DC_VALS), huffman_codes(DC_CHROMA_BITS, DC_VALS))
AC_CODES = (huffman_codes(AC_LUMA_BITS, AC_LUMA_VALS), huffman_codes(AC_CHROMA_BITS, AC_CHROMA_VALS))

# layout of the int32 table the kernels read (include/ccedit_hip.h, "Motion-JPEG")
TAB_QUANT, TAB_ZIGZAG, TAB_DCT, TAB_COLOR, TAB_DC, TAB_AC, TAB_SIZE = 0, 128, 192, 256, 272, 304, 816


def check_quality(quality: int) -> int:
    if int(quality) != quality or not 1 <= int(quality) <= 100:
        raise ValueError(f"quality {quality!r}: an integer 1 ... 100")
    return int(quality)


def check_size(h: int, w: int) -> None:
    if h < MCU or w < MCU or h % MCU or w % MCU or h > 65520 or w > 65520:
        raise ValueError(f"frames of {h}x{w}: H and W must be multiples of {MCU} (4:2:0 MCUs, no edge padding), 16 ... 65520")


def quant_tables(quality: int = DEFAULT_QUALITY) -> Tuple[List[int], List[int]]:
    """The two Annex K tables at `quality`, row-major: s = 5000 / q below 50, 200 - 2 q from 50, clamp((base s + 50) / 100, 1, 255)."""
    q = check_quality(quality)
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple([int(min(max((int(b) * s + 50) // 100, 1), 255)) for b in base] for base in (QUANT_LUMA, QUANT_CHROMA))


def table_array() -> np.ndarray:
    """The constants as the kernels take them: int32 [TAB_SIZE] — base quantisation tables (row-major), zigzag, FDCT matrix, colour
    factors, DC codes (2 x 16 by size), AC codes (2 x 256 by run << 4 | size), each code << 8 | length."""
    t = np.zeros(TAB_SIZE, np.int32)
    t[TAB_QUANT:TAB_QUANT + 64], t[TAB_QUANT + 64:TAB_QUANT + 128] = QUANT_LUMA, QUANT_CHROMA
    t[TAB_ZIGZAG:TAB_ZIGZAG + 64] = ZIGZAG
    t[TAB_DCT:TAB_DCT + 64] = DCT.reshape(-1)
    t[TAB_COLOR:TAB_COLOR + 9] = COLOR
    for c in range(2):
        t[TAB_DC + 16 * c:TAB_DC + 16 * c + 16] = DC_CODES[c][:16]
        t[TAB_AC + 256 * c:TAB_AC + 256 * c + 256] = AC_CODES[c]
    return t


_DEVICE_TABLES = {}


def device_tables(device):
    import torch
    key = str(device)
    if key not in _DEVICE_TABLES:
        _DEVICE_TABLES[key] = torch.from_numpy(table_array()).to(device)
    return _DEVICE_TABLES[key]


def _segment(marker: int, payload: bytes) -> bytes:
    return struct.pack(">BBH", 0xFF, marker, len(payload) + 2) + payload


def frame_header(h: int, w: int, quality: int = DEFAULT_QUALITY) -> bytes:
    """SOI, APP0 (JFIF 1.01), DQT, SOF0, DHT, DRI, SOS: everything of a frame in front of its entropy-coded data."""
    check_size(h, w)
    ql, qc = quant_tables(quality)
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    out += _segment(0xDB, b"".join(bytes([i]) + bytes(int(t[z]) for z in ZIGZAG) for i, t in enumerate((ql, qc))))
    out += _segment(0xC0, struct.pack(">BHHB", 8, h, w, 3) + bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    out += _segment(0xC4, b"".join(bytes([(0x10 if kind == "ac" else 0) | c]) + bytes(bits) + bytes(vals) for kind, c, bits, vals in HUFFMAN))
    out += _segment(0xDD, struct.pack(">H", w // MCU))
    out += _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return out


# ------------------------------------------------------------------------------------------
# the encoder: three stages on the device (ops.mjpeg_*), only the compressed bytes come to the host
# ------------------------------------------------------------------------------------------
MAX_FRAMES_PER_LAUNCH = 256       # ... and the pack stage's scan over the frames of a launch stays short
SCRATCH_BYTES = 256 << 20       # frames per launch are chosen so that the worst-case segment buffer stays below this; results do not depend on it


def segment_capacity(w: int) -> int:
    """Bytes the library reserves per restart interval: every block at MAX_BLOCK_BITS, every byte stuffed, the padded last byte too."""
    from . import ops
    return ops.mjpeg_segment_bytes(w)


def encode_frames(frames, quality: int = DEFAULT_QUALITY) -> List[bytes]:
    """uint8 frames (N, H, W, 3) on the device -> N complete JPEG files (bytes)."""
    import torch
    from . import ops
    q = check_quality(quality)
    if frames.dim() != 4 or frames.shape[3] != 3 or frames.dtype != torch.uint8 or not frames.is_cuda:
        raise ValueError(f"encode_frames: uint8 frames (N, H, W, 3) on the device, got {frames.dtype} {tuple(frames.shape)} {frames.device}")
    n, h, w, _ = frames.shape
    check_size(h, w)
    frames = frames.contiguous()
    tables = device_tables(frames.device)
    header = torch.frombuffer(bytearray(frame_header(h, w, q)), dtype=torch.uint8).to(frames.device)
    out: List[bytes] = []
    for g in launch_groups(n, per_launch(MAX_FRAMES_PER_LAUNCH, SCRATCH_BYTES, (h // MCU) * segment_capacity(w))):
        chunk = frames[g]
        coef = ops.mjpeg_transform(chunk, tables, q)
        scratch, seg_len = ops.mjpeg_entropy(coef, tables)
        seg_off, frame_bytes = ops.mjpeg_pack_scan(seg_len, chunk.shape[0], h, w, header.numel())
        sizes = frame_bytes.cpu().tolist()                       # the byte counts: what lets the host take exactly the compressed bytes
        out.extend(split_bytes(ops.mjpeg_pack(scratch, seg_len, seg_off, header, chunk.shape[0], h, w, sum(sizes)).cpu().numpy().tobytes(), sizes))
    return out


# ------------------------------------------------------------------------------------------
# the container
# ------------------------------------------------------------------------------------------
def _chunk(fourcc: bytes, payload: bytes) -> bytes:
    return fourcc + struct.pack("<I", len(payload)) + payload + (b"\x00" if len(payload) & 1 else b"")


def _list(kind: bytes, payload: bytes) -> bytes:
    return b"LIST" + struct.pack("<I", len(payload) + 4) + kind + payload


def write_avi(path: str, jpegs: Sequence[bytes], fps: int, h: int, w: int) -> str:
    """RIFF `AVI `: hdrl (avih, one strl: strh vids / MJPG, strf BITMAPINFOHEADER), movi (one 00dc chunk per frame, padded to even
    length), idx1.  The frame rate is dwRate / dwScale = fps / 1.  A file that would pass 2 GiB is refused (no OpenDML)."""
    n = len(jpegs)
    if n < 1:
        raise ValueError("write_avi: no frames")
    if int(fps) != fps or int(fps) < 1:
        raise ValueError(f"write_avi: fps {fps!r} must be a positive integer (dwRate / dwScale = fps / 1)")
    fps = int(fps)
    check_size(h, w)
    movi_bytes = sum(8 + len(j) + (len(j) & 1) for j in jpegs)
    total = 12 + (8 + 4 + 8 + 56 + 8 + 4 + 8 + 56 + 8 + 40) + (8 + 4 + movi_bytes) + (8 + 16 * n)
    if total > MAX_RIFF_BYTES:
        raise ValueError(f"write_avi: {n} frames make {total} bytes, more than one RIFF chunk holds (2 GiB, no OpenDML): write fewer frames "
                         "or lower the quality")
    biggest = max(len(j) for j in jpegs)
    avih = struct.pack("<14I", 1000000 // fps, biggest * fps, 0, 0x10, n, 0, 1, biggest, w, h, 0, 0, 0, 0)            # AVIF_HASINDEX
    strh = b"vids" + b"MJPG" + struct.pack("<IHHIIIIIIIIhhhh", 0, 0, 0, 0, 1, fps, 0, n, biggest, 0xFFFFFFFF, 0, 0, 0, w, h)
    strf = struct.pack("<IiiHH4sIiiII", 40, w, h, 1, 24, b"MJPG", w * h * 3, 0, 0, 0, 0)
    hdrl = _list(b"hdrl", _chunk(b"avih", avih) + _list(b"strl", _chunk(b"strh", strh) + _chunk(b"strf", strf)))
    movi, idx, at = [], [], 4                                      # idx1 offsets count from the `movi` fourcc
    for j in jpegs:
        movi.append(_chunk(b"00dc", j))
        idx.append(b"00dc" + struct.pack("<III", 0x10, at, len(j)))                                                    # AVIIF_KEYFRAME
        at += len(movi[-1])
    body = b"AVI " + hdrl + _list(b"movi", b"".join(movi)) + _chunk(b"idx1", b"".join(idx))
    assert len(body) + 8 == total, (len(body) + 8, total)
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)
    return path


def read_avi(path: str) -> Tuple[List[bytes], int, int, int]:
    """-> (jpegs, fps, H, W) of an .avi with one MJPG video stream.  Everything else is a ValueError that says why."""
    if not os.path.isfile(path):
        raise ValueError(f"{path}: no such .avi file")
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < 12 or data[:4] != b"RIFF" or data[8:12] != b"AVI ":
        raise ValueError(f"{path}: not a RIFF AVI file")
    riff_end = 8 + struct.unpack_from("<I", data, 4)[0]
    if riff_end > len(data):
        raise ValueError(f"{path}: truncated (the RIFF chunk says {riff_end} bytes, the file has {len(data)})")

    def walk(at, end):
        while at + 8 <= end:
            fourcc, size = data[at:at + 4], struct.unpack_from("<I", data, at + 4)[0]
            if at + 8 + size > end:
                raise ValueError(f"{path}: truncated (chunk {fourcc!r} at {at} runs past its parent)")
            yield fourcc, at + 8, size
            at += 8 + size + (size & 1)

    jpegs, fps, h, w, handler = [], None, None, None, None
    for fourcc, at, size in walk(12, riff_end):
        if fourcc == b"LIST" and data[at:at + 4] == b"hdrl":
            for f2, a2, s2 in walk(at + 4, at + size):
                if f2 == b"LIST" and data[a2:a2 + 4] == b"strl" and handler is None:
                    for f3, a3, s3 in walk(a2 + 4, a2 + s2):
                        if f3 == b"strh" and s3 >= 56 and data[a3:a3 + 4] == b"vids":
                            handler = data[a3 + 4:a3 + 8]
                            scale, rate = struct.unpack_from("<II", data, a3 + 20)
                            if scale < 1 or rate % scale:
                                raise ValueError(f"{path}: frame rate {rate} / {scale} is not an integer")
                            fps = rate // scale
                        elif f3 == b"strf" and s3 >= 40 and handler is not None:
                            w, h = struct.unpack_from("<ii", data, a3 + 4)
                            handler = data[a3 + 16:a3 + 20]
        elif fourcc == b"LIST" and data[at:at + 4] == b"movi":
            jpegs = [data[a2:a2 + s2] for f2, a2, s2 in walk(at + 4, at + size) if f2 in (b"00dc", b"00db")]
    if handler is None or fps is None or h is None:
        raise ValueError(f"{path}: no video stream header (hdrl / strl / strh vids / strf)")
    if handler.upper() != b"MJPG":
        raise ValueError(f"{path}: the video stream is {handler!r}, only MJPG (Motion-JPEG) is read")
    if not jpegs:
        raise ValueError(f"{path}: no frames (no 00dc chunk in movi)")
    return jpegs, int(fps), abs(int(h)), int(w)


def decode_avi_u8(path: str) -> np.ndarray:
    """All frames of an MJPG .avi -> uint8 (N, H, W, 3) on the host (Pillow decodes each chunk)."""
    import io
    from PIL import Image
    jpegs, _, h, w = read_avi(path)
    frames = []
    for i, j in enumerate(jpegs):
        try:
            a = np.array(Image.open(io.BytesIO(j)).convert("RGB"))
        except Exception as e:
            raise ValueError(f"{path}: frame {i} does not decode as JPEG: {e}") from e
        if a.shape != (h, w, 3):
            raise ValueError(f"{path}: frame {i} is {a.shape[0]}x{a.shape[1]}, the stream header says {h}x{w}")
        frames.append(a)
    return np.stack(frames, axis=0)


def parse_avi(path: str):
    """An MJPG .avi -> (jpegs, their jpegdec.parse() results, H, W): every frame parsed ONCE and held to the stream header's size.
    jpegdec.JpegUnsupported (naming file and frame): a frame outside the subset the device decodes."""
    from . import jpegdec
    jpegs, _, h, w = read_avi(path)
    infos = []
    for i, j in enumerate(jpegs):
        try:
            info = jpegdec.parse(j)
        except jpegdec.JpegUnsupported as e:
            raise jpegdec.JpegUnsupported(f"{path}: frame {i}: {e}") from e
        if (info.height, info.width) != (h, w):
            raise ValueError(f"{path}: frame {i} is {info.height}x{info.width}, the stream header says {h}x{w}")
        infos.append(info)
    return jpegs, infos, h, w


def decode_avi_device(path: str, device, select=None, parsed=None):
    """All frames of an MJPG .avi -> uint8 (N, H, W, 3) on `device`, decoded there (ccedit_amd/jpegdec.py): only the compressed bytes go
    up.  The frames equal decode_avi_u8's byte for byte.  `select`: number of frames -> the indices to decode (every frame is still
    parsed, so that a file goes one way as a whole).  `parsed`: parse_avi(path), when the caller has it already.
    jpegdec.JpegUnsupported: a frame outside the subset the device decodes.
    Corrupt entropy-coded data, which Pillow decodes with a warning, is a ValueError naming file, frame and restart interval."""
    from . import jpegdec
    jpegs, infos, _, _ = parse_avi(path) if parsed is None else parsed
    pick = range(len(jpegs)) if select is None else [int(i) for i in select(len(jpegs))]
    try:
        return jpegdec.decode([jpegs[i] for i in pick], device, infos=[infos[i] for i in pick])
    except jpegdec.JpegUnsupported:
        raise
    except ValueError as e:
        raise ValueError(f"{path}: {'' if select is None else 'selected '}{e}") from e
