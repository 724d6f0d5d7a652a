"""GIF sources decoded on the GPU: the frames of a .gif in three stages (ccedit_amd/csrc/gifdec.hip), none of
which is a serial walk over pixels.  The frames equal Pillow's (scripts/sampling/util.py through video_io._sequence_u8) byte for byte, so
this route and the host route are interchangeable.  Opt-in: `--gif_decoder device` / gif_decoder="device" of the loaders.

  parse(data)            the container, on the host: signature, logical screen, global colour table, the graphic control extension
                         (disposal, transparent flag and index; every other extension is skipped by its sub-blocks), image descriptors,
                         local colour tables, the minimum code size, each image's data sub-blocks concatenated, the trailer.  No pixel
                         arithmetic.  What is outside the subset below is a GifUnsupported that names the reason, a structural defect a
                         ValueError that names it, both before any launch.
  decode_gif(data, ...)  compressed bytes in, uint8 (N, H, W, 3) on the device out.  Stage A (one wave per image): the code stream ->
                         a table of codes (parent, length, first / last byte, pixel offset), from the code stream alone: a code's width
                         follows from the count of codes since the last Clear, a dictionary entry is named by two earlier codes.
                         Stage B (one lane per code): the code's pixels, one hop up the chain of parents per pixel.  Stage C (one
                         thread per canvas pixel): the images of a launch composited in order; the canvas is carried between launches.

The subset: canvas within gif.check_size; minimum code size 2 ... 8; every frame has a palette (local or global) and a non-empty rectangle
inside the canvas; frame 0 covers the whole canvas at offset 0 and has no transparent flag; every frame but the last has disposal 0 or 1
(the last frame's disposal cannot change a pixel and is ignored).  Later frames may be any sub-rectangle, interlaced or not, with or
without a transparent index, with their own palette or the global one.  Outside it Pillow's results depend on its RGBA canvas rules
(a transparent or partial first frame, disposal 2 / 3 in mid-clip): those files stay Pillow's.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence

import numpy as np

from . import gif
from .codec_common import launch_groups, per_launch

# (csrc/gifdec_core.h Status)
STATUS_TEXT = {1: "a code above the next free entry", 2: "a first code after Clear that is not a literal",
               3: "the stream ends before the image's pixels", 4: "a minimum code size outside 2 ... 8",
               5: "an index at or beyond the palette's size", 6: "a descriptor outside its buffers"}

DESC_WORDS = 16
(D_X, D_Y, D_W, D_H, D_INTERLACE, D_TRANSPARENT, D_PAL_OFF, D_PAL_SIZE, D_MIN_CODE, D_STREAM_OFF, D_STREAM_LEN, D_CODE_OFF, D_CODE_CAP, D_PLANE_OFF,
 D_SLOT) = range(15)
MAX_FRAMES_PER_LAUNCH = 256
SCRATCH_BYTES = 256 << 20          # frames per launch are chosen so that code tables and index planes stay below this; results do not depend on it
CODE_BYTES = 14                    # of one code's table entry: parent, len, off (int32), first, last (uint8)


class GifUnsupported(ValueError):
    """The file is a GIF outside the subset the device decodes: the message names the reason."""


@dataclass
class GifFrame:
    x: int
    y: int
    w: int
    h: int
    interlace: bool
    transparent: int               # the transparent index, -1: none
    disposal: int
    palette: bytes                 # RGB triples, local or global
    min_code: int
    stream: bytes                  # the data sub-blocks, concatenated

    @property
    def max_codes(self) -> int:
        """The bound of the frame's data codes: each yields a pixel at least and takes min_code + 1 bits at least; one more."""
        return min(self.w * self.h, 8 * len(self.stream) // (self.min_code + 1)) + 1


@dataclass
class GifInfo:
    height: int
    width: int
    frames: List[GifFrame]

    @property
    def n_frames(self) -> int:
        return len(self.frames)


def _cut(what: str, pos: int) -> GifUnsupported:
    return GifUnsupported(f"truncated file ({what} is cut at offset {pos})")


def _sub_blocks(data: bytes, pos: int, what: str):
    """-> (the sub-blocks from pos on, concatenated; the offset behind their terminator)"""
    parts = []
    while True:
        if pos >= len(data):
            raise _cut(what, pos)
        size = data[pos]
        pos += 1
        if size == 0:
            return b"".join(parts), pos
        if pos + size > len(data):
            raise _cut(what, pos)
        parts.append(data[pos:pos + size])
        pos += size


def parse(data: bytes) -> GifInfo:
    """One GIF file -> GifInfo; GifUnsupported: outside the subset (a truncated file included: Pillow reads what is there);
    ValueError: not a well-formed GIF."""
    data = bytes(data)
    n = len(data)
    if data[:6] not in (b"GIF87a", b"GIF89a"):
        raise ValueError("not a GIF file (bad signature)")
    if n < 13:
        raise _cut("the logical screen descriptor", n)
    width, height, packed = struct.unpack_from("<HHB", data, 6)
    pos = 13
    global_palette = None
    if packed & 0x80:
        size = 3 << ((packed & 7) + 1)
        if pos + size > n:
            raise _cut("the global colour table", pos)
        global_palette = data[pos:pos + size]
        pos += size
    try:
        gif.check_size(height, width)
    except ValueError as e:
        raise GifUnsupported(f"canvas {height}x{width} (H and W 1 ... {gif.MAX_SIDE}, H * W <= 2^24)") from e
    frames: List[GifFrame] = []
    disposal, transparent = 0, -1
    while True:
        if pos >= n:
            raise _cut("the file (no trailer)", pos)
        kind = data[pos]
        pos += 1
        if kind == 0x3B:
            break
        if kind == 0x21:
            if pos >= n:
                raise _cut("an extension", pos)
            label = data[pos]
            pos += 1
            if label == 0xF9:
                if pos + 6 > n:
                    raise _cut("the graphic control extension", pos)
                if data[pos] != 4 or data[pos + 5] != 0:
                    raise ValueError(f"bad graphic control extension at offset {pos - 2}")
                flags, tindex = data[pos + 1], data[pos + 4]
                disposal, transparent = (flags >> 2) & 7, (tindex if flags & 1 else -1)
                pos += 6
            else:
                _, pos = _sub_blocks(data, pos, "an extension")
            continue
        if kind != 0x2C:
            raise ValueError(f"unknown block 0x{kind:02x} at offset {pos - 1}")
        if pos + 9 > n:
            raise _cut("an image descriptor", pos)
        x, y, w, h, flags = struct.unpack_from("<HHHHB", data, pos)
        pos += 9
        palette = global_palette
        if flags & 0x80:
            size = 3 << ((flags & 7) + 1)
            if pos + size > n:
                raise _cut("a local colour table", pos)
            palette = data[pos:pos + size]
            pos += size
        if pos >= n:
            raise _cut("an image", pos)
        min_code = data[pos]
        stream, pos = _sub_blocks(data, pos + 1, "an image's data")
        i = len(frames)
        if palette is None:
            raise GifUnsupported(f"frame {i} has no palette (neither a local nor a global colour table)")
        if not 2 <= min_code <= 8:
            raise GifUnsupported(f"frame {i}: minimum code size {min_code} (only 2 ... 8)")
        if w < 1 or h < 1 or x + w > width or y + h > height:
            raise GifUnsupported(f"frame {i}: rectangle {w}x{h} at {x},{y} is empty or outside the canvas of {width}x{height}")
        if i == 0 and (x, y, w, h) != (0, 0, width, height):
            raise GifUnsupported(f"a partial first frame ({w}x{h} at {x},{y} on a canvas of {width}x{height})")
        if i == 0 and transparent >= 0:
            raise GifUnsupported("a transparent first frame")
        frames.append(GifFrame(x, y, w, h, bool(flags & 0x40), transparent, disposal, palette, min_code, stream))
        disposal, transparent = 0, -1
    if not frames:
        raise ValueError("no image in the file")
    for i, f in enumerate(frames[:-1]):
        if f.disposal not in (0, 1):
            raise GifUnsupported(f"frame {i}: disposal {f.disposal} before the last frame (only 0 and 1)")
    return GifInfo(int(height), int(width), frames)


# ------------------------------------------------------------------------------------------
# the decoder: three stages on the device (ops.gifdec_*); the compressed bytes, the palettes and one descriptor per frame go up
# ------------------------------------------------------------------------------------------
def frame_scratch_bytes(f: GifFrame) -> int:
    return f.max_codes * CODE_BYTES + f.w * f.h


def frames_per_launch(info: GifInfo) -> int:
    return per_launch(MAX_FRAMES_PER_LAUNCH, SCRATCH_BYTES, max(frame_scratch_bytes(f) for f in info.frames))


def describe(frames: Sequence[GifFrame], slots: Sequence[int]):
    """The frames of one launch -> (data uint8: their streams and palettes back to back; desc int64 (N, 16); the code table's entries;
    the planes' bytes; the largest code capacity).  slots[i]: the output frame i is written to, -1: none."""
    desc = np.zeros((len(frames), DESC_WORDS), np.int64)
    parts, at, palettes = [], 0, {}
    codes = plane = 0
    for i, f in enumerate(frames):
        if f.palette not in palettes:
            palettes[f.palette] = at
            parts.append(f.palette)
            at += len(f.palette)
        desc[i, :D_SLOT + 1] = (f.x, f.y, f.w, f.h, int(f.interlace), f.transparent, palettes[f.palette], len(f.palette) // 3, f.min_code, at,
                                len(f.stream), codes, f.max_codes, plane, slots[i])
        parts.append(f.stream)
        at += len(f.stream)
        codes += f.max_codes
        plane += f.w * f.h
    data = np.frombuffer(b"".join(parts), np.uint8).copy()
    return data, desc, codes, plane, max(f.max_codes for f in frames)


def status_error(code: int, position: int, frame: int) -> ValueError:
    where = "bit" if code < 5 else "pixel"
    return ValueError(f"frame {frame}: {STATUS_TEXT.get(code, 'status')} (code {code} at {where} {position})")


def decode_group(frames: Sequence[GifFrame], slots: Sequence[int], canvas, check_from: int = 0):
    """One launch group: the frames composited in order on `canvas` (uint8 (H, W, 3) on the device, updated in place) -> the selected
    frames uint8 (number of slots >= 0, H, W, 3).  A stream the device stops in, or an index beyond a palette: the ValueError of
    status_error, with the frame counted from check_from."""
    import torch
    from . import ops
    data, desc, codes, plane, largest = describe(frames, slots)
    device = canvas.device
    data_d, desc_d = torch.from_numpy(data).to(device), torch.from_numpy(desc).to(device)
    table, ends, ncodes, st_codes = ops.gifdec_codes(data_d, desc_d, codes)
    planes = ops.gifdec_pixels(desc_d, table, ends, ncodes, plane, largest)
    out, st_compose = ops.gifdec_compose(data_d, desc_d, planes, canvas, sum(1 for s in slots if s >= 0))
    a, b = st_codes.cpu().numpy(), st_compose.cpu().numpy()                      # (the one synchronisation per launch)
    status = np.where(a[:, :1] != 0, a, b)
    bad = np.flatnonzero(status[:, 0])
    if len(bad):
        i = int(bad[0])
        raise status_error(int(status[i, 0]), int(status[i, 1]), check_from + i)
    return out


def decode_gif(data: bytes, device, select: Optional[Callable[[int], Sequence[int]]] = None, info: Optional[GifInfo] = None,
               frames_per_group: Optional[int] = None):
    """The frames of one .gif file -> uint8 (N, H, W, 3) on `device`: all, or those at the indices select(number of frames).  Every frame
    up to the last selected one is decoded (the canvas accumulates), only the selected ones are written.  frames_per_group: frames of
    one launch (default: what the scratch bound allows); the result does not depend on it.  GifUnsupported / ValueError from the parser:
    nothing was launched; ValueError("frame i: ... (code c at bit p)"): the device stopped in that frame's stream."""
    import torch
    info = parse(data) if info is None else info
    idx = list(range(info.n_frames)) if select is None else [int(i) for i in select(info.n_frames)]
    if not idx or any(not 0 <= i < info.n_frames for i in idx):
        raise ValueError(f"decode_gif: frame indices {idx} of a file with {info.n_frames} frames")
    wanted = sorted(set(idx))
    upto = wanted[-1] + 1
    per = frames_per_launch(info) if frames_per_group is None else int(frames_per_group)
    if per < 1:
        raise ValueError(f"decode_gif: frames_per_group={frames_per_group} (>= 1)")
    canvas = torch.zeros((info.height, info.width, 3), dtype=torch.uint8, device=device)      # (frame 0 covers it)
    outs = []
    for g in launch_groups(upto, per):
        slots, k = [], 0
        for i in range(g.start, g.stop):
            slots.append(k if i in wanted else -1)
            k += i in wanted
        out = decode_group(info.frames[g], slots, canvas, g.start)
        if k:
            outs.append(out)
    out = outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)
    if idx != wanted:
        out = out[torch.tensor([wanted.index(i) for i in idx], device=out.device)]
    return out
