"""The routing of frame / video I/O as data (DESIGN.md sections 3.14 to 3.18): ONE table of source kinds with their device decoders
and ONE table of file writers.  scripts/sampling/util.py keeps the public loaders and save functions of the reference's names and asks
here which way a path goes; a further format is one entry here, and its codec module.

Sources.  A clip goes ONE way as a whole: every file (every frame of an .avi, the whole animated PNG) is parsed before anything is
decoded, and what the parser declines sends the whole clip to Pillow on the host, with one line on stderr.  Image files, GIFs and the
frames of a Motion-JPEG .avi or an animated .png are Pillow's on the host route; with a device, JPEG and PNG are decoded THERE
(jpegdec.py, pngdec.py: the same bytes as Pillow's), and a .gif is when the caller opts in (gif_decoder="device": gifdec.py, a kind's
`opt_in` decoders).  mp4 needs a codec library (decord / cv2 / imageio-ffmpeg) that is not installed.

Sinks.  `--save_type gif` (Pillow's writer, or the device's with `--gif_encoder device`), `mjpeg` and `png`: a numbered file in a
folder of its own; the device writers take uint8 frames where they are, or upload a host array once."""
from __future__ import annotations

import os
import re
import sys
from typing import Any, Callable, NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import gif, gifdec, jpegdec, mjpeg, png, pngdec
from .codec_common import duration_ms


def HWC3(x: np.ndarray) -> np.ndarray:
    """util.py:559-576: uint8 image with 1 / 3 / 4 channels (or none) -> 3 channels (alpha blended on white)."""
    assert x.dtype == np.uint8
    if x.ndim == 2:
        x = x[:, :, None]
    assert x.ndim == 3
    c = x.shape[2]
    assert c in (1, 3, 4)
    if c == 3:
        return x
    if c == 1:
        return np.concatenate([x, x, x], axis=2)
    color = x[:, :, 0:3].astype(np.float32)
    alpha = x[:, :, 3:4].astype(np.float32) / 255.0
    return (color * alpha + 255.0 * (1.0 - alpha)).clip(0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------
# sources: the device decoders
# ------------------------------------------------------------------------------------------
class Decoder(NamedTuple):
    """A codec the device decodes.  `parse` and `decode` are looked up on `module` at call time."""
    module: Any                                   # jpegdec / pngdec; its name is the prefix of the stderr line
    ext: Tuple[str, ...]                          # of the image files it takes (compared in lower case)
    declines: type                                # what parse raises for a clip that goes to Pillow instead; anything else propagates
    accepts: Optional[Callable[[Any], bool]]      # parsed header -> False: declined without a word
    reword: Callable[..., str]                    # (what, e, paths, idx) -> the text of a device status; str(e): raised as it is
    parse_clip: Callable[[str], Any]              # a video in one file -> what decode_clip takes; every frame is parsed
    decode_clip: Callable[..., torch.Tensor]      # (path, parsed, device, select) -> uint8 (N, h, w, 3) on the device


def _jpeg_status(what, e, paths=None, idx=None) -> str:
    """Files: "{what}: ..."; the frames of an .avi are worded by mjpeg.decode_avi_device (path, "selected " with a selection)."""
    return str(e) if paths is None or isinstance(e, jpegdec.JpegUnsupported) else f"{what}: {e}"


def _png_status(what, e, paths=None, idx=None) -> str:
    """Files: the decoder's "frame i" counts inside its call, the text names the file and its index in the clip."""
    m = re.match(r"frame (\d+): (.*)", str(e)) if paths else None
    if m:
        k = idx[int(m.group(1))]
        return f"{what}: {os.path.basename(paths[k])}: frame {k}: {m.group(2)}"
    return f"{what}: {e}"


def _parse_apng(path: str):
    with open(path, "rb") as f:
        data = f.read()
    return data, pngdec.parse(data)


def _parse_gif(path: str):
    with open(path, "rb") as f:
        data = f.read()
    return data, gifdec.parse(data)


JPEG = Decoder(jpegdec, (".jpg", ".jpeg"), jpegdec.JpegUnsupported, lambda info: info.ncomp == 3, _jpeg_status, mjpeg.parse_avi,
               lambda path, parsed, device, select: mjpeg.decode_avi_device(path, device, select, parsed))
PNG = Decoder(pngdec, (".png",), ValueError, None, _png_status, _parse_apng,           # (PngUnsupported is a ValueError: any declines)
              lambda path, parsed, device, select: pngdec.decode_apng(parsed[0], device, select, info=parsed[1]))
# (no image files: a directory of .gif stills is not a video of GIF frames.  GifUnsupported is a ValueError: any declines)
GIFDEC = Decoder(gifdec, (), ValueError, None, _png_status, _parse_gif,
                 lambda path, parsed, device, select: gifdec.decode_gif(parsed[0], device, select, info=parsed[1]))


def _declined(dec: Decoder, text: str) -> None:
    sys.stderr.write(f"[{dec.module.__name__.rsplit('.', 1)[-1]}] {text}; this clip is decoded by Pillow on the host\n")


def _reworded(e: ValueError, text: str):
    if text == str(e):
        raise e
    raise ValueError(text) from e


def files_u8_device(decoders, paths, device, what: str):
    """The image files `paths` -> list of uint8 (n, h, w, 3) tensors on `device`, by the first of `decoders` that takes ALL of them: ONE
    tensor from one batched call when they share a size, else one call and one (1, h, w, 3) tensor per file.  None: they go through
    Pillow as before — not all of them carry the decoder's extension (asked before any file is read), or one is not what `accepts`
    wants, or the parser declines one (one line on stderr names it).  Each file is parsed once; only the compressed bytes go up.  A
    stream the device stops in is a ValueError in the decoder's wording (`reword`)."""
    for dec in decoders:
        if not paths or not all(p.lower().endswith(dec.ext) for p in paths):
            continue
        datas, infos = [], []
        for p in paths:
            with open(p, "rb") as f:
                datas.append(f.read())
            try:
                infos.append(dec.module.parse(datas[-1]))
            except dec.declines as e:
                return _declined(dec, f"{what}: {os.path.basename(p)}: {e}")
            if dec.accepts is not None and not dec.accepts(infos[-1]):
                return None
        same = len({(i.height, i.width) for i in infos}) == 1
        out = []
        for idx in ([list(range(len(datas)))] if same else [[k] for k in range(len(datas))]):
            try:
                out.append(dec.module.decode([datas[k] for k in idx], device, infos=[infos[k] for k in idx]))
            except ValueError as e:
                _reworded(e, dec.reword(what, e, paths, idx))
        return out
    return None


def clip_u8_device(decoders, path: str, device, select=None):
    """The frames of a video in one file (all, or those at the indices select(number of frames)) -> uint8 (N, h, w, 3) on `device`,
    decoded there; only they are decoded, but everything is parsed, so that a clip goes ONE way as a whole.  None: the kind has no
    device decoder, or the parser declines (one line on stderr says why), and the clip then goes through Pillow as before."""
    for dec in decoders:
        try:
            parsed = dec.parse_clip(path)
        except dec.declines as e:
            return _declined(dec, dec.reword(path, e))
        try:
            return dec.decode_clip(path, parsed, device, select)
        except ValueError as e:
            _reworded(e, dec.reword(path, e))
    return None


# ------------------------------------------------------------------------------------------
# sources: the kinds
# ------------------------------------------------------------------------------------------
class Kind(NamedTuple):
    name: str
    matches: Callable[[str], bool]                # how a path is recognised
    count: Callable[[str], int]                   # its number of frames
    pil: Callable[..., Tuple[int, Callable]]      # (path, each) -> (n, pick): pick(i) = each(frame i as Pillow decodes it); files are opened when picked
    u8: Optional[Callable[[str], np.ndarray]]     # a video in one file: all frames by Pillow -> uint8 (N, h, w, 3) on the host
    device: Tuple[Decoder, ...]                   # who decodes it on the device, asked in this order
    opt_in: Tuple[Decoder, ...] = ()              # who decodes it on the device when the caller asks for it (gif_decoder="device"), after `device`


def is_apng(path: str) -> bool:
    """An animated PNG: a .png file with more than one frame (what --save_type png writes for a clip).  A still .png is not a video:
    it stays what it was at every place that asks (an unsupported video format; ONE mask image)."""
    if not path.lower().endswith(".png") or not os.path.isfile(path):
        return False
    from PIL import Image
    try:
        with Image.open(path) as im:
            return int(getattr(im, "n_frames", 1)) > 1
    except Exception:
        return False


def _pil_count(path: str) -> int:
    from PIL import Image
    return int(getattr(Image.open(path), "n_frames", 1))


def _pil_files(path: str, each):
    from PIL import Image
    files = sorted(os.listdir(path))
    return len(files), lambda i: each(Image.open(os.path.join(path, files[i])))


def _pil_sequence(path: str, each):
    from PIL import Image, ImageSequence
    frames = [each(fr) for fr in ImageSequence.Iterator(Image.open(path))]
    return len(frames), frames.__getitem__


def _pil_avi(path: str, each):
    from PIL import Image
    frames = [each(Image.fromarray(fr)) for fr in mjpeg.decode_avi_u8(path)]
    return len(frames), frames.__getitem__


def _sequence_u8(path: str) -> np.ndarray:
    """All frames of a .gif or an animated .png (transparency blended on white, as HWC3)."""
    n, pick = _pil_sequence(path, lambda fr: HWC3(np.array(fr.convert("RGBA") if fr.mode == "P" and "transparency" in fr.info else fr.convert("RGB"))))
    return np.stack([pick(i) for i in range(n)], axis=0)


# (.gif and .avi match case-sensitively, .png and the image files of the decoders in lower case: as ever)
FILES = Kind("directory", os.path.isdir, lambda p: len(os.listdir(p)), _pil_files, None, (JPEG, PNG))      # JPEG is asked before PNG
GIF = Kind(".gif", lambda p: p.endswith(".gif"), _pil_count, _pil_sequence, _sequence_u8, (), (GIFDEC,))
AVI = Kind(".avi", lambda p: p.endswith(".avi"), lambda p: len(mjpeg.read_avi(p)[0]), _pil_avi, mjpeg.decode_avi_u8, (JPEG,))
APNG = Kind("animated .png", is_apng, _pil_count, _pil_sequence, _sequence_u8, (PNG,))
KINDS = (FILES, GIF, AVI, APNG)


def kind_of(path: str, mp4_hint: bool = True, missing_ok: bool = False) -> Optional[Kind]:
    """The kind of source `path` is.  None of them: None with missing_ok, else the ValueError every loader raises — for an .mp4, with
    mp4_hint, the NotImplementedError that says which libraries would read it."""
    for kind in KINDS:
        if kind.matches(path):
            return kind
    if missing_ok:
        return None
    if mp4_hint and path.endswith(".mp4"):
        raise NotImplementedError("mp4 decoding needs decord / cv2 / imageio-ffmpeg, none of which is installed; "
                                  "extract the frames to a directory of images (or a .gif) instead")
    raise ValueError("Unsupported video format. Only support dirctory, .mp4, .gif and .avi (Motion-JPEG).")


# ------------------------------------------------------------------------------------------
# sinks
# ------------------------------------------------------------------------------------------
GIF_ENCODERS = ("pillow", "device")


def decoders_of(kind: Kind, gif_decoder: str = "pillow") -> Tuple[Decoder, ...]:
    """Who decodes a source of `kind` on the device: its `device` decoders, and with gif_decoder="device" its opt-in ones behind them
    (anything else: the route as it always was)."""
    return kind.device + kind.opt_in if gif_decoder == "device" else kind.device


def to_device(frames) -> torch.Tensor:
    """uint8 frames, a tensor or an array -> a contiguous device tensor (a host one is uploaded once, to the current device)."""
    if not torch.is_tensor(frames):
        frames = torch.from_numpy(np.ascontiguousarray(frames))
    if not frames.is_cuda:
        frames = frames.to(torch.device("cuda", torch.cuda.current_device()))
    return frames.contiguous()


def next_path(folder: str, stem: str, ext: str) -> str:
    """<folder>/<stem>-XXXX<ext>, XXXX the number of files the folder (made if need be) holds now."""
    os.makedirs(folder, exist_ok=True)
    return os.path.join(folder, f"{stem}-{len(os.listdir(folder)):04}{ext}")


def _write_gif_pillow(savepath: str, frames, fps) -> str:
    from PIL import Image
    imgs = [Image.fromarray(f) for f in frames]
    imgs[0].save(savepath, save_all=True, append_images=imgs[1:], duration=duration_ms(fps), loop=0)
    return savepath


def _write_gif_device(savepath: str, frames, fps, gif_encoder: str = "device") -> str:
    """Palettes and LZW streams come from the device (gif.py, csrc/gif.hip), only they come back; the container is written on the host."""
    frames = to_device(frames)
    return gif.write_gif(savepath, gif.encode_frames(frames), gif.duration_ms(fps), frames.shape[2], frames.shape[1])


def _write_avi(savepath: str, frames, fps, video_quality: int = 90) -> str:
    """Motion-JPEG, every frame encoded on the device (mjpeg.py, csrc/mjpeg.hip), only the compressed bytes come back."""
    frames = to_device(frames)
    return mjpeg.write_avi(savepath, mjpeg.encode_frames(frames, video_quality), fps, frames.shape[1], frames.shape[2])


def _write_apng(savepath: str, frames, fps) -> str:
    """An animated PNG (one frame: a plain PNG) holding exactly these bytes, rows filtered and deflate-coded on the device (png.py,
    csrc/png.hip); only the compressed streams come back, the container is written on the host."""
    frames = to_device(frames)
    return png.write_apng(savepath, png.encode_frames(frames), png.duration_ms(fps), frames.shape[2], frames.shape[1])


class Writer(NamedTuple):
    folder: str                       # under the save path
    stem: str
    ext: str
    write: Callable[..., str]         # (savepath, uint8 frames (T, H, W, 3), fps, **options) -> savepath
    on_device: bool                   # takes the frames where they are (a host array is uploaded); False: host frames
    options: Tuple[str, ...]          # what of (video_quality, gif_encoder) it is given: by keyword to `write` and to
    #                                   perform_save_locally_video, by position after fps to `saver`
    saver: str                        # the function of scripts/sampling/util.py that writes one clip with it


# (savetype, gif_encoder) -> writer; gif_encoder is 'pillow' wherever it does not apply
WRITERS = {("gif", "pillow"): Writer("gif", "animation", ".gif", _write_gif_pillow, False, (), "save_gif_u8"),
           ("gif", "device"): Writer("gif", "animation", ".gif", _write_gif_device, True, ("gif_encoder",), "save_gif_u8"),
           ("mjpeg", "pillow"): Writer("mjpeg", "animation", ".avi", _write_avi, True, ("video_quality",), "save_avi_u8"),
           ("png", "pillow"): Writer("png", "animation", ".png", _write_apng, True, (), "save_png_u8")}


def writer_of(savetype: str, gif_encoder: str = "pillow") -> Optional[Writer]:
    """The writer of a save type, None where that is no movie of uint8 frames (npy, mp4); the gif_encoder checks of every entry."""
    if gif_encoder not in GIF_ENCODERS:
        raise ValueError(f"gif_encoder {gif_encoder!r}: one of {GIF_ENCODERS}")
    if gif_encoder == "device" and savetype != "gif":
        raise ValueError(f"gif_encoder='device' encodes gifs: savetype must be 'gif', got {savetype!r}")
    return WRITERS.get((savetype, gif_encoder))


def save_u8(save_path: str, writer: Writer, frames, fps, **options) -> str:
    """uint8 frames (T, H, W, 3) -> <save_path>/<folder>/<stem>-XXXX<ext>, numbered by what the folder holds -> the path."""
    return writer.write(next_path(os.path.join(save_path, writer.folder), writer.stem, writer.ext), frames, fps, **options)
