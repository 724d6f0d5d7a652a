"""PNG sources decoded on the GPU: frame files and the frames of an animated .png, in two stages
(ccedit_amd/csrc/pngdec.hip), the stages of ccedit_amd/png.py in reverse.  The frames equal Pillow's byte for byte, so this route and
the host route are interchangeable.

  parse(data)             the container, on the host: signature, every chunk's CRC, IHDR, acTL / fcTL, and per frame the zlib payload
                          (all IDAT chunks, or the frame's fdAT chunks without their sequence numbers).  No pixel arithmetic.  What
                          is outside the subset below is a PngUnsupported that names the reason, a structural defect a ValueError
                          that names it, both before any launch.
  decode(datas, device)   compressed bytes in, uint8 (N, H, W, 3) on the device out: inflate (one wave per stream: the full deflate
                          format, Adler-32 verified) and unfilter (one wave per image, 64 rows as a skewed wavefront).
  decode_apng(data, ...)  the same for the frames of one animated file.

The subset: bit depth 8, colour type 2 (truecolour), no interlace, sides and pixel count within png.check_size.  Ancillary chunks are
ignored, as Pillow ignores them for the pixels of a mode-RGB image (a tRNS on colour type 2 included).  An animated file is served
when acTL is present, an fcTL precedes IDAT (the default image is the first frame) and every fcTL covers the full canvas at offset 0:
without alpha, dispose and blend operations then cannot change a pixel.
"""
from __future__ import annotations

import struct
import zlib
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence

import numpy as np

from . import png
from .codec_common import launch_groups, parsed, per_launch

STATUS_TEXT = {1: "bad zlib header", 2: "the stream runs past its input", 3: "block type 3", 4: "a stored block's LEN and NLEN disagree",
               5: "an over-subscribed or incomplete Huffman code", 6: "bad code-length runs", 7: "invalid code or symbol",
               8: "a distance that reaches before the stream's start", 9: "the output would pass the image's size",
               10: "the output ends short of the image's size", 11: "Adler-32 mismatch", 12: "a filter byte above 4"}

MAX_FRAMES_PER_LAUNCH = 256
SCRATCH_BYTES = 256 << 20          # frames per launch are chosen so that the filtered bytes stay below this; results do not depend on it


class PngUnsupported(ValueError):
    """The file is a PNG outside the subset the device decodes: the message names the reason."""


@dataclass
class PngInfo:
    height: int
    width: int
    frames: List[bytes]            # per frame its zlib stream
    animated: bool                 # acTL present

    @property
    def n_frames(self) -> int:
        return len(self.frames)


_COLOUR = {0: "greyscale", 3: "palette", 4: "greyscale with alpha", 6: "RGBA (alpha)"}


def parse(data: bytes) -> PngInfo:
    """One PNG / APNG file -> PngInfo; PngUnsupported: outside the subset; ValueError: not a well-formed PNG."""
    data = bytes(data)
    n = len(data)
    if data[:8] != png.SIGNATURE:
        raise ValueError("not a PNG file (bad signature)")
    pos = 8
    ihdr = None
    actl = None
    frames: List[List[bytes]] = []
    seq = 0
    idat_seen = idat_closed = iend = False
    pending_fctl = False
    while not iend:
        if pos == n:
            raise ValueError("truncated file (no IEND chunk)")
        if pos + 8 > n:
            raise ValueError(f"truncated file (a chunk header is cut at offset {pos})")
        length, kind = struct.unpack_from(">I4s", data, pos)
        if length > png.MAX_CHUNK_LENGTH:
            raise ValueError(f"bad chunk length {length} at offset {pos}")
        if pos + 12 + length > n:
            raise ValueError(f"truncated file (the {kind.decode('latin-1')} chunk at offset {pos} runs past the end)")
        body = data[pos + 8:pos + 8 + length]
        if zlib.crc32(data[pos + 4:pos + 8 + length]) & 0xffffffff != struct.unpack_from(">I", data, pos + 8 + length)[0]:
            raise ValueError(f"bad CRC of the {kind.decode('latin-1')} chunk at offset {pos}")
        pos += 12 + length
        if ihdr is None and kind != b"IHDR":
            raise ValueError(f"missing IHDR (the first chunk is {kind.decode('latin-1')})")
        if idat_seen and kind != b"IDAT":
            idat_closed = True
        if kind == b"IHDR":
            if ihdr is not None or length != 13:
                raise ValueError("bad IHDR chunk")
            ihdr = struct.unpack(">IIBBBBB", body)
            w, h, depth, colour, comp, filt, lace = ihdr
            if depth == 16:
                raise PngUnsupported("16 bit samples (only 8 bit)")
            if colour in _COLOUR:
                raise PngUnsupported(f"{_COLOUR[colour]} (only 8-bit RGB, colour type 2)")
            if colour != 2 or depth != 8 or comp != 0 or filt != 0 or lace > 1:
                raise ValueError(f"bad IHDR (bit depth {depth}, colour type {colour}, compression {comp}, filter {filt}, interlace {lace})")
            if lace:
                raise PngUnsupported("Adam7 interlace")
            try:
                png.check_size(h, w)
            except ValueError as e:
                raise PngUnsupported(f"size {h}x{w} (H and W 1 ... {png.MAX_SIDE}, H * W <= 2^24)") from e
        elif kind == b"acTL":
            if length != 8 or actl is not None or idat_seen:
                raise ValueError("bad acTL chunk")
            actl = struct.unpack(">II", body)[0]
            if actl < 1:
                raise ValueError("bad acTL chunk (no frames)")
        elif kind == b"fcTL":
            if idat_seen:
                idat_closed = True
            if actl is None:
                continue                                     # (without acTL the file is a still image: Pillow ignores the chunk)
            if length != 26 or pending_fctl:
                raise ValueError("bad fcTL chunk" if length != 26 else "two fcTL chunks without data between them")
            s, fw, fh, fx, fy = struct.unpack_from(">IIIII", body)
            if s != seq:
                raise ValueError(f"broken fcTL / fdAT sequence (number {s} where {seq} is due)")
            seq += 1
            if (fw, fh, fx, fy) != (ihdr[0], ihdr[1], 0, 0):
                raise PngUnsupported(f"partial-frame fcTL ({fw}x{fh} at {fx},{fy} on a canvas of {ihdr[0]}x{ihdr[1]})")
            pending_fctl = True
        elif kind == b"IDAT":
            if idat_closed:
                raise ValueError("IDAT chunks that are not consecutive")
            if not idat_seen:
                idat_seen = True
                if actl is not None and not pending_fctl:
                    raise PngUnsupported("a default image outside the animation (IDAT before the first fcTL)")
                frames.append([])
                pending_fctl = False
            frames[0].append(body)
        elif kind == b"fdAT":
            if actl is None:
                continue                                     # (without acTL the file is a still image: Pillow ignores the chunk)
            if length < 4 or not idat_seen:
                raise ValueError("bad fdAT chunk")
            s = struct.unpack_from(">I", body)[0]
            if s != seq:
                raise ValueError(f"broken fcTL / fdAT sequence (number {s} where {seq} is due)")
            seq += 1
            if pending_fctl:
                frames.append([])
                pending_fctl = False
            elif len(frames) < 2:
                raise ValueError("fdAT without an fcTL before it")
            idat_closed = True
            frames[-1].append(body[4:])
        elif kind == b"IEND":
            iend = True
        else:
            if idat_seen:
                idat_closed = True
            if not kind[0] & 0x20 and kind != b"PLTE":
                raise ValueError(f"unknown critical chunk {kind.decode('latin-1')}")
    if not idat_seen:
        raise ValueError("missing IDAT")
    streams = [b"".join(f) for f in frames]
    if actl is None:
        streams = streams[:1]
    elif actl != len(streams) or pending_fctl:
        raise ValueError(f"acTL announces {actl} frames, the file holds {len(streams)}{' and an fcTL without data' if pending_fctl else ''}")
    return PngInfo(int(ihdr[1]), int(ihdr[0]), streams, actl is not None)


# ------------------------------------------------------------------------------------------
# the decoder: two stages on the device (ops.pngdec_*), only the compressed bytes and the offset table go up
# ------------------------------------------------------------------------------------------
def frames_per_launch(h: int, w: int) -> int:
    return per_launch(MAX_FRAMES_PER_LAUNCH, SCRATCH_BYTES, png.filtered_bytes(h, w))


def pack_streams(streams: Sequence[bytes]):
    """-> (data uint8: the streams back to back, table int64 (N, 2): offset and length of each)"""
    table = np.zeros((len(streams), 2), np.int64)
    at = 0
    for i, s in enumerate(streams):
        table[i] = (at, len(s))
        at += len(s)
    data = np.frombuffer(b"".join(streams), np.uint8).copy() if at else np.zeros(1, np.uint8)
    return data, table


def status_error(code: int, where: int, frame: int) -> ValueError:
    return ValueError(f"frame {frame}: {STATUS_TEXT.get(code, 'status')} (code {code} at byte {where})")


def decode_streams(streams: Sequence[bytes], h: int, w: int, device, check: bool = True):
    """N zlib streams of images of h x w -> (uint8 (N, h, w, 3) on the device, status int32 (N, 2) on the host: a frame's first non-zero
    (code, byte position) of the two stages).  check: a non-zero code raises the ValueError that names frame, code and position."""
    import torch
    from . import ops
    if len(streams) < 1:
        raise ValueError("decode: no frames")
    png.check_size(h, w)
    out = None
    status = np.zeros((len(streams), 2), np.int32)
    for g in launch_groups(len(streams), frames_per_launch(h, w)):
        s, part = g.start, streams[g]
        data, table = pack_streams(part)
        filtered, st_inflate = ops.pngdec_inflate(torch.from_numpy(data).to(device), torch.from_numpy(table).to(device), h, w)
        rgb, st_unfilter = ops.pngdec_unfilter(filtered, h, w)
        a, b = st_inflate.cpu().numpy(), st_unfilter.cpu().numpy()              # (the one synchronisation per launch)
        status[s:s + len(part)] = np.where(a[:, :1] != 0, a, b)
        if check:
            bad = np.flatnonzero(status[s:s + len(part), 0])
            if len(bad):
                i = s + int(bad[0])
                raise status_error(int(status[i, 0]), int(status[i, 1]), i)
        if len(part) == len(streams):
            return rgb, status
        if out is None:
            out = torch.empty((len(streams), h, w, 3), dtype=torch.uint8, device=device)
        out[s:s + len(part)] = rgb
    return out, status


def decode(datas: Sequence[bytes], device, infos: Optional[Sequence[PngInfo]] = None):
    """N PNG files (bytes) of one size -> uint8 (N, H, W, 3) on `device`: each file's first frame, as Image.open gives it.  `infos`: their
    parse() results, when the caller has them.  PngUnsupported / ValueError from the parser: nothing was launched;
    ValueError("frame i: ... (code c at byte p)"): the device stopped in that file's stream.  Pillow raises OSError on such a file."""
    if len(datas) < 1:
        raise ValueError("decode: no frames")
    infos = parsed(datas, infos, parse)
    sizes = {(i.height, i.width) for i in infos}
    if len(sizes) != 1:
        raise ValueError(f"decode: frames of different sizes {sorted(sizes)}")
    return decode_streams([i.frames[0] for i in infos], infos[0].height, infos[0].width, device)[0]


def decode_apng(data: bytes, device, select: Optional[Callable[[int], Sequence[int]]] = None, info: Optional[PngInfo] = None):
    """The frames of one animated (or still) PNG file -> uint8 (N, H, W, 3) on `device`: all, or those at the indices select(number of
    frames).  Only they are decoded, but the whole file is parsed, so that a clip goes one way as a whole."""
    info = parse(data) if info is None else info
    idx = list(range(info.n_frames)) if select is None else [int(i) for i in select(info.n_frames)]
    if any(not 0 <= i < info.n_frames for i in idx):
        raise ValueError(f"decode_apng: frame indices {idx} of a file with {info.n_frames} frames")
    try:
        return decode_streams([info.frames[i] for i in idx], info.height, info.width, device, check=True)[0]
    except PngUnsupported:
        raise
    except ValueError as e:
        msg = str(e)
        if msg.startswith("frame "):
            k = int(msg[6:msg.index(":")])
            raise ValueError(f"frame {idx[k]}{msg[msg.index(':'):]}") from e
        raise
