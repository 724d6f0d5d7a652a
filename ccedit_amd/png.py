"""Lossless video output (`--save_type png`): animated PNG whose deflate streams are coded on the device
(ccedit_amd/csrc/png.hip) and the PNG / APNG container around them, written here.

8-bit RGB (colour type 2, no interlace), one zlib stream per frame.  Every row is filtered by the PNG filter (None, Sub, Up, Average,
Paeth) whose bytes have the smallest sum of min(v, 256 - v), ties to the lowest number; the row above the first is zeros.  The frame's
H * (1 + 3 W) filtered bytes are cut into CHUNKs, each coded on its own as ONE dynamic-Huffman deflate block (BTYPE = 2): a greedy LZ77
over a single-entry hash table of HASH_SIZE positions (no chains, no lazy evaluation, no match reaches before the chunk), histograms
of the 286 literal/length and 30 distance symbols, plain Huffman code lengths repaired to 15 bits (7 for the code-length alphabet), the
header with the run codes 16 / 17 / 18, the tokens.  There are no stored blocks.  A frame's stream is 78 01, its chunks' bits back to
back (BFINAL only on the last), zero padding to a byte, Adler-32 of the filtered bytes.  The rules in full: tests/_png_numpy.py, whose
bytes the kernels equal; there is no host fallback.  This module is the ONE place of the constants.

CHUNK.  Measured with the numpy restatement (bytes of one frame's zlib stream; Pillow's default PNG file of the same pixels beside it;
tests/test_png.py asserts the ratios of the files):

    CHUNK      real crop 256x384 (tests/golden)   content("photo", 128, 192)   content("photo", 512, 768)
     8 KiB              96 325                            60 846                       953 435
    16 KiB              95 514                            60 644                       950 970
    32 KiB              95 048                            60 532                       949 806
    Pillow              81 614                            61 776                       969 233

16 KiB is taken.  Against 8 KiB the block header (about 100 bytes) and the cold start of the hash table are paid half as often, 0.3 to 0.8 %
of the file.  32 KiB gains 0.1 to 0.5 % more but doubles what the token stage waits for: a chunk is walked serially by one lane, so that
stage — nine tenths of the device time — takes as long as ONE chunk takes, and a 512 x 768 frame would have only 37 chunks to spread
over the chip.  With 16 KiB of bytes, the 8 KiB table and the histograms of a chunk in LDS two chunks share a workgroup below 64 KB.
"""
from __future__ import annotations

import struct
import zlib
from typing import List, Sequence

from .codec_common import check_frames, duration_ms, launch_groups, per_launch, split_bytes      # noqa: F401  (duration_ms: png.duration_ms, as the gif route hands it over)

# ---- the constants of the format: this is their one place
FILTERS = 5                     # None, Sub, Up, Average, Paeth
CHUNK = 16384                   # filtered bytes per independently coded chunk (= deflate block)
HASH_BITS = 12
HASH_SIZE = 1 << HASH_BITS      # single-entry table: uint16 positions, 0xffff = empty (csrc/png.hip kHashSize)
HASH_MUL = 2654435761           # hash = ((b0 | b1 << 8 | b2 << 16) * HASH_MUL mod 2^32) >> (32 - HASH_BITS)
MIN_MATCH, MAX_MATCH = 3, 258
LITLEN_SYMS, DIST_SYMS, CL_SYMS = 286, 30, 19
EOB = 256
MAX_BITS, CL_MAX_BITS = 15, 7
DIST_AT = 288                   # a chunk's histogram / code table: literal/length symbols at 0, distance symbols at DIST_AT
HIST_WORDS = 320
TOKEN_MATCH = 1 << 31           # a token word: a literal's byte, or TOKEN_MATCH | (length - 3) << 16 | (distance - 1)
TOKENS_CHUNKS_PER_WORKGROUP = 2     # one lane per chunk; bytes, hash table and histograms of a chunk in LDS (csrc/png.hip kTokChunks)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
# the worst case of a block header: BFINAL + BTYPE, HLIT, HDIST, HCLEN, 19 code-length lengths, and 316 code lengths that each cost a
# 7-bit code and (16 / 17 / 18) up to 7 extra bits
HEADER_MAX_BITS = 3 + 5 + 5 + 4 + 3 * CL_SYMS + (LITLEN_SYMS + DIST_SYMS) * (CL_MAX_BITS + 7)
HEADER_WORDS = (HEADER_MAX_BITS + 31) // 32 + 3 & ~3
# a token costs at most 16 bits per byte it covers (a match of 3 bytes: 15 + 5 + 15 + 13 = 48 bits; a literal: 15), end-of-block 15
SLOT_BYTES = ((HEADER_MAX_BITS + 16 * CHUNK + MAX_BITS + 31) // 32 + 3) // 4 * 16
# what a chunk of noise can cost beyond its own bytes (tests/_png_numpy.py derives it): the worst-case header, and the 257 symbols of a
# chunk without a match under the code "255 literals at 8 bits, the rarest literal and end-of-block at 9", which no Huffman code exceeds:
# at most CHUNK / 256 + 9 bits over 8 per byte
HEADER_MAX = (HEADER_MAX_BITS + CHUNK // 256 + 9 + 7) // 8
ADLER_MOD = 65521
MAX_PIXELS = 1 << 24            # H * W of a frame (gif.MAX_PIXELS)
MAX_SIDE = 65535
MAX_CHUNK_LENGTH = (1 << 31) - 1        # a PNG chunk's length field
SIGNATURE = b"\x89PNG\r\n\x1a\n"


def row_bytes(w: int) -> int:
    return 1 + 3 * int(w)


def filtered_bytes(h: int, w: int) -> int:
    return int(h) * row_bytes(w)


def chunks_of(length: int, chunk: int = CHUNK) -> int:
    """Chunks of a filtered stream of `length` bytes."""
    return -(-int(length) // int(chunk))


def check_size(h: int, w: int) -> None:
    if not (1 <= int(h) <= MAX_SIDE and 1 <= int(w) <= MAX_SIDE and int(h) * int(w) <= MAX_PIXELS):
        raise ValueError(f"frames of {h}x{w}: H and W must be 1 ... {MAX_SIDE} with H * W <= 2^24 (what the device PNG encoder takes)")
    length = filtered_bytes(h, w)
    if 2 + chunks_of(length) * SLOT_BYTES + 4 + 4 > MAX_CHUNK_LENGTH:          # (cannot happen below 2^24 pixels; kept as the format's own limit)
        raise ValueError(f"frames of {h}x{w}: a frame's stream could exceed the 2^31 - 1 bytes a PNG chunk holds")


# ------------------------------------------------------------------------------------------
# the encoder: the stages on the device (ops.png_*); packed streams, their byte counts and the Adler words come to the host
# ------------------------------------------------------------------------------------------
MAX_FRAMES_PER_LAUNCH = 64
SCRATCH_BYTES = 256 << 20         # frames per launch are chosen so that filtered bytes, tokens, tables and slots stay below this; results do not depend on it


def frames_per_launch(h: int, w: int) -> int:
    length = filtered_bytes(h, w)
    per_frame = length + chunks_of(length) * (4 * CHUNK + 2 * 4 * HIST_WORDS + 4 * HEADER_WORDS + SLOT_BYTES + 32) + (length + 1) // 2
    return per_launch(MAX_FRAMES_PER_LAUNCH, SCRATCH_BYTES, per_frame)


def encode_filtered(filtered) -> List[bytes]:
    """uint8 filtered bytes (N, L) on the device -> each row's zlib stream: the deflate stages of one launch group."""
    from . import ops
    n, length = filtered.shape
    tokens, ntok, hist = ops.png_tokens(filtered)
    codes, header, header_bits, chunk_bits = ops.png_codes(hist, n)
    slots = ops.png_emit(tokens, ntok, codes, header, header_bits)
    chunk_off, frame_bytes = ops.png_pack_scan(chunk_bits, n)
    adler = ops.png_adler(filtered).cpu().tolist()
    sizes = frame_bytes.cpu().tolist()                              # the byte counts: what lets the host take exactly the coded bytes
    packed = ops.png_pack(slots, chunk_bits, chunk_off, n, sum(sizes)).cpu().numpy().tobytes()
    return [b"\x78\x01" + body + struct.pack(">I", a & 0xffffffff) for body, a in zip(split_bytes(packed, sizes), adler)]


def encode_frames(frames) -> List[bytes]:
    """uint8 frames (N, H, W, 3) on the device -> per frame its zlib stream (what IDAT / fdAT carry)."""
    from . import ops
    frames = check_frames(frames, "encode_frames", check_size)
    n, h, w, _ = frames.shape
    out: List[bytes] = []
    for g in launch_groups(n, frames_per_launch(h, w)):
        out.extend(encode_filtered(ops.png_filter(frames[g]).reshape(-1, filtered_bytes(h, w))))
    return out


# ------------------------------------------------------------------------------------------
# the container
# ------------------------------------------------------------------------------------------
def _chunk(kind: bytes, data: bytes) -> bytes:
    if len(data) > MAX_CHUNK_LENGTH:
        raise ValueError(f"write_apng: a {kind.decode()} chunk of {len(data)} bytes exceeds 2^31 - 1")
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xffffffff)


def write_apng(path: str, streams: Sequence[bytes], duration_ms: int, W: int, H: int) -> str:
    """PNG signature, IHDR (8-bit RGB, no interlace); for more than one frame acTL (frame count, plays 0 = for ever) and per frame an fcTL
    (the full frame at offset 0, delay duration_ms / 1000 s, dispose 0, blend 0), IDAT for the first frame and fdAT for the others, fcTL
    and fdAT numbered in one sequence; IEND.  One frame: a plain PNG without acTL and fcTL."""
    if len(streams) < 1:
        raise ValueError("write_apng: no frames")
    check_size(H, W)
    if not 0 <= int(duration_ms) <= 65535:
        raise ValueError(f"write_apng: duration {duration_ms!r} ms is outside what the 16-bit delay numerator holds (0 ... 65535)")
    parts = [SIGNATURE, _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0))]
    animated = len(streams) > 1
    if animated:
        parts.append(_chunk(b"acTL", struct.pack(">II", len(streams), 0)))
    seq = 0
    for i, stream in enumerate(streams):
        if len(stream) < 8:
            raise ValueError(f"write_apng: frame {i}: a zlib stream, got {len(stream)} bytes")
        if animated:
            parts.append(_chunk(b"fcTL", struct.pack(">IIIIIHHBB", seq, W, H, 0, 0, int(duration_ms), 1000, 0, 0)))
            seq += 1
        if i == 0:
            parts.append(_chunk(b"IDAT", bytes(stream)))
        else:
            parts.append(_chunk(b"fdAT", struct.pack(">I", seq) + bytes(stream)))
            seq += 1
    parts.append(_chunk(b"IEND", b""))
    with open(path, "wb") as f:
        f.write(b"".join(parts))
    return path
