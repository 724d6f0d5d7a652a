"""What the codec modules (gif.py, png.py, mjpeg.py, jpegdec.py, pngdec.py) share: the check of device frames, the frame duration, the
walk over launch groups, the split of packed bytes and the "parsed headers given or parse now" step.  No constant of a format lives
here: each stays in its module, which hands its own bounds and its own check_size in."""
from __future__ import annotations

from typing import Callable, Iterator, List, Optional, Sequence


def check_frames(frames, what: str, check_size: Callable[[int, int], None]):
    """uint8 frames (N, H, W, 3) on the device, N >= 1, of a size the caller's check_size takes -> the frames, contiguous."""
    import torch
    if not torch.is_tensor(frames) or frames.dim() != 4 or frames.shape[3] != 3 or frames.dtype != torch.uint8 or not frames.is_cuda \
            or frames.shape[0] < 1:
        raise ValueError(f"{what}: uint8 frames (N, H, W, 3) on the device, N >= 1, got "
                         f"{getattr(frames, 'dtype', type(frames))} {tuple(getattr(frames, 'shape', ()))} {getattr(frames, 'device', '')}")
    check_size(frames.shape[1], frames.shape[2])
    return frames.contiguous()


def duration_ms(fps) -> int:
    """The frame duration as the Pillow gif route hands it over: int(round(1000 / fps)).  A gif holds duration // 10 centiseconds, an
    animated PNG the fraction duration / 1000 s."""
    return int(round(1000.0 / fps))


def per_launch(max_frames: int, scratch_bytes: int, frame_bytes: int) -> int:
    """Frames of one launch: at most max_frames, and as many as keep frame_bytes each below scratch_bytes; at least one."""
    return max(1, min(int(max_frames), int(scratch_bytes) // int(frame_bytes)))


def launch_groups(n: int, per: int) -> Iterator[slice]:
    """The slices of n frames, `per` to a launch."""
    for s in range(0, n, per):
        yield slice(s, min(s + per, n))


def split_bytes(packed: bytes, sizes: Sequence[int]) -> List[bytes]:
    """The packed bytes of a launch, cut by the byte counts of its frames."""
    out, at = [], 0
    for b in sizes:
        out.append(packed[at:at + b])
        at += b
    return out


def parsed(datas: Sequence[bytes], infos: Optional[Sequence], parse: Callable) -> Sequence:
    """The parsed header of every file: the caller's (a reader that had to parse anyway hands them on), or parsed here."""
    if infos is None:
        return [parse(d) for d in datas]
    if len(infos) != len(datas):
        raise ValueError(f"decode: {len(infos)} parsed headers for {len(datas)} files")
    return infos
