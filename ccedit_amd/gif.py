"""GIF output encoded on the device (`--gif_encoder device`): a colour quantiser and a chunked LZW coder on the
GPU (ccedit_amd/csrc/gif.hip) and the GIF89a container around them, written here.

Per frame a local palette of 256 colours from Wu's variance-minimising quantiser on a 32 x 32 x 32 grid of cells (cell = r >> 3, g >> 3,
b >> 3): five integer moment tables (count, sum r, sum g, sum b, sum r^2 + g^2 + b^2) on a 33^3 grid with a zero border, their inclusive
3-D prefix sums in int64, 255 cuts of the box (0, 32]^3 scored in float64, the box means with integer rounding as palette entries and a
32^3 byte table cell -> box that maps the pixels: no nearest-colour search, no dithering (Pillow's adaptive route does not dither either).

The frame's indices are LZW-coded in CHUNKs of 3072 pixels, each from an empty dictionary (9 bits, next code 258), so that the chunks
are independent — the trick of mjpeg.hip's restart intervals: GIF allows a Clear code anywhere.  A chunk adds at most 3071 entries, so
code 4095 is never reached and there is no dictionary-full case.  After every emitted code (the chunk's last one included) an entry is
counted and the width grows once the next free code exceeds 1 << width; the chunk ENDS with Clear (256) at that width — the decoder reads
it at the width the chunk finished with — and the frame's last chunk with EOI (257); only the first chunk starts with a Clear, at 9 bits.
Codes are packed LSB first, a frame's stream is its chunks' bits back to back, zero-padded to a byte.

The files the kernels produce equal the numpy restatement the tests carry (tests/_gif_numpy.py) byte for byte, and there is no host
fallback.  This module is the ONE place of the constants.  The container (header without a global colour table, NETSCAPE2.0 loop 0,
per frame a graphic control extension, an image descriptor with a local colour table, sub-blocks of 255 bytes) is framed on the host.
"""
from __future__ import annotations

import struct
from typing import List, Sequence, Tuple

from .codec_common import check_frames, duration_ms, launch_groups, per_launch, split_bytes      # noqa: F401  (duration_ms: gif.duration_ms, as the Pillow route hands it over)

# ---- the constants of the format: this is their one place
GRID = 32                   # cells per colour axis: cell = value >> SHIFT
SHIFT = 3
SIDE = GRID + 1             # the moment tables carry a zero border: index = cell + 1
MOMENTS = 5                 # count, sum r, sum g, sum b, sum (r^2 + g^2 + b^2)
MOMENT_WORDS = MOMENTS * SIDE ** 3          # int64 words of one frame's tables (1.4 MB)
COLORS = 256
MIN_CODE_SIZE = 8
CLEAR, EOI, FIRST_CODE = 256, 257, 258
START_WIDTH = 9
CHUNK = 3072                # pixels per independently coded chunk: 258 + 3072 < 4096
LZW_CHUNKS_PER_WORKGROUP = 4        # one lane per chunk, a 16 KB hash table in LDS each (csrc/gif.hip kLzwChunks; what tools/gif_time.py reports)
SLOT_BYTES = ((12 * (CHUNK + 2) + 31) // 32 + 3) // 4 * 16       # a chunk's slot: CHUNK codes, a leading and a trailing Clear / EOI at 12 bits
MAX_PIXELS = 1 << 24        # H * W of a frame
MAX_SIDE = 65535            # the screen descriptor's 16 bits
SUB_BLOCK = 255


def check_size(h: int, w: int) -> None:
    if not (1 <= int(h) <= MAX_SIDE and 1 <= int(w) <= MAX_SIDE and int(h) * int(w) <= MAX_PIXELS):
        raise ValueError(f"frames of {h}x{w}: H and W must be 1 ... {MAX_SIDE} with H * W <= 2^24 (what the device GIF encoder takes)")


def chunks_of(h: int, w: int, chunk: int = CHUNK) -> int:
    return -(-(int(h) * int(w)) // int(chunk))


# ------------------------------------------------------------------------------------------
# the encoder: the stages on the device (ops.gif_*), only palettes and LZW bytes come to the host
# ------------------------------------------------------------------------------------------
MAX_FRAMES_PER_LAUNCH = 64
SCRATCH_BYTES = 256 << 20         # frames per launch are chosen so that moment tables, indices and chunk slots stay below this; results do not depend on it


def frames_per_launch(h: int, w: int) -> int:
    per_frame = MOMENT_WORDS * 8 + GRID ** 3 + COLORS * 3 + h * w + chunks_of(h, w) * (SLOT_BYTES + 16) + (h * w * 3 + 1) // 2
    return per_launch(MAX_FRAMES_PER_LAUNCH, SCRATCH_BYTES, per_frame)


def _quantize_launch(frames):
    from . import ops
    cells, palettes = ops.gif_palette(ops.gif_histogram(frames))
    return palettes, ops.gif_map(frames, cells)


def quantize(frames):
    """uint8 frames (N, H, W, 3) on the device -> (palettes uint8 (N, 256, 3), indices uint8 (N, H, W)), both on the device."""
    import torch
    frames = check_frames(frames, "quantize", check_size)
    parts = [_quantize_launch(frames[g]) for g in launch_groups(frames.shape[0], frames_per_launch(frames.shape[1], frames.shape[2]))]
    return torch.cat([p for p, _ in parts], dim=0), torch.cat([i for _, i in parts], dim=0)


def encode_indices(indices, chunk: int = CHUNK) -> List[bytes]:
    """uint8 indices (N, H, W) on the device -> each frame's LZW byte stream (LZW and pack stages of one launch group)."""
    from . import ops
    n, h, w = indices.shape
    slots, chunk_bits = ops.gif_lzw(indices, chunk)
    chunk_off, frame_bytes = ops.gif_pack_scan(chunk_bits, n, h, w, chunk)
    sizes = frame_bytes.cpu().tolist()                              # the byte counts: what lets the host take exactly the coded bytes
    return split_bytes(ops.gif_pack(slots, chunk_bits, chunk_off, n, h, w, chunk, sum(sizes)).cpu().numpy().tobytes(), sizes)


def encode_frames(frames) -> List[Tuple[bytes, bytes]]:
    """uint8 frames (N, H, W, 3) on the device -> per frame (palette: 768 bytes, the frame's LZW byte stream)."""
    frames = check_frames(frames, "encode_frames", check_size)
    out: List[Tuple[bytes, bytes]] = []
    for g in launch_groups(frames.shape[0], frames_per_launch(frames.shape[1], frames.shape[2])):
        palettes, indices = _quantize_launch(frames[g])
        streams = encode_indices(indices)
        pal = palettes.cpu().numpy()
        out.extend((pal[i].tobytes(), streams[i]) for i in range(len(streams)))
    return out


# ------------------------------------------------------------------------------------------
# the container
# ------------------------------------------------------------------------------------------
def _sub_blocks(data: bytes) -> bytes:
    parts = []
    for at in range(0, len(data), SUB_BLOCK):
        piece = data[at:at + SUB_BLOCK]
        parts.append(bytes([len(piece)]) + piece)
    parts.append(b"\x00")
    return b"".join(parts)


def write_gif(path: str, encoded: Sequence[Tuple[bytes, bytes]], duration_ms: int, W: int, H: int) -> str:
    """GIF89a: logical screen descriptor without a global colour table, NETSCAPE2.0 with loop 0, per frame a graphic control extension
    (delay duration_ms // 10 centiseconds, no disposal, no transparency), an image descriptor of the full frame with a local colour table
    of 256 entries, LZW minimum code size 8, the stream in sub-blocks of 255 bytes; trailer."""
    if len(encoded) < 1:
        raise ValueError("write_gif: no frames")
    check_size(H, W)
    delay = int(duration_ms) // 10
    if not 0 <= delay <= 65535:
        raise ValueError(f"write_gif: duration {duration_ms!r} ms is outside what the 16-bit delay holds (0 ... 655359)")
    parts = [b"GIF89a", struct.pack("<HHBBB", W, H, 0x70, 0, 0), b"\x21\xff\x0bNETSCAPE2.0\x03\x01\x00\x00\x00"]
    for i, (palette, stream) in enumerate(encoded):
        if len(palette) != COLORS * 3 or len(stream) < 1:
            raise ValueError(f"write_gif: frame {i}: a palette of {COLORS * 3} bytes and a non-empty LZW stream, got {len(palette)} and {len(stream)}")
        parts.append(b"\x21\xf9\x04" + struct.pack("<BHB", 0, delay, 0) + b"\x00")
        parts.append(b"\x2c" + struct.pack("<HHHHB", 0, 0, W, H, 0x87))
        parts.append(bytes(palette))
        parts.append(bytes([MIN_CODE_SIZE]) + _sub_blocks(bytes(stream)))
    parts.append(b"\x3b")
    with open(path, "wb") as f:
        f.write(b"".join(parts))
    return path
