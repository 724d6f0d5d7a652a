"""Mask tracking: an edit mask painted on ONE source frame follows the source's motion to every frame of the clip (`--mask_track`,
DESIGN.md section 3.20).

For a frame f, taken moving away from the anchor K, with its neighbour g on K's side (g = f - 1 forwards, f + 1 backwards): block
vectors f -> g and g -> f from the propagation's matcher (propagate.match_pairs, unchanged) -> per pixel the best of the 3 x 3
neighbouring blocks' vectors by a 5 x 5 box sum of absolute luma differences (select) -> a nearest lookup of g's mask, cleared where
the two directions disagree by more than FB_LIMIT: such a pixel is not visible in g — newly revealed, and revealed content lies
behind the tracked subject.  All of it is integer arithmetic on bytes in ccedit_amd/csrc/masktrack.hip, equal bit for bit to the numpy
restatement the tests carry; there is no host fallback.  This module holds what the host decides: the constants, the pair lists and
the loop over a clip (track_clip), and what follows tracking (finish: dilate, then invert).
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from .propagate import BLOCK, LEVELS

# ---- the constants of the algorithm: this is their one place on the host (csrc/masktrack.hip restates the candidate order and VEC_MAX)
CANDIDATES = ((0, 0), (-1, 0), (0, -1), (0, 1), (1, 0), (-1, -1), (-1, 1), (1, -1), (1, 1))      # (dby, dbx); the key is S * 16 + order
BOX = 5                     # side of the box sum of the selection
FB_LIMIT = 1                # largest |v(p) + r(q)|_1 of a consistent correspondence
VEC_MAX = 64                # block vectors are clamped into +-VEC_MAX by the kernel (the matcher's own reach is 46)
DILATE_MAX = 32             # largest --mask_dilate
PAIR_CHUNK = 32             # pairs per select launch: bounds the workspace (4 H W bytes per pair); results do not depend on it


def chain(frames: int, anchor: int):
    """The frames in the order they are tracked, each with its neighbour on the anchor's side: [(f, g)], forwards first."""
    if frames < 1:
        raise ValueError(f"mask tracking needs at least one frame, got {frames}")
    if not 0 <= anchor < frames:
        raise ValueError(f"--mask_frame {anchor} is outside the video's {frames} frames (0 ... {frames - 1})")
    return [(f, f - 1) for f in range(anchor + 1, frames)] + [(f, f + 1) for f in range(anchor - 1, -1, -1)]


def pair_rows(frames: int, anchor: int) -> np.ndarray:
    """int32 (2 (F - 1), 4): for the i-th frame of chain() row 2 i is (f, g, 0, 0) — v, the vectors the mask is looked up along — and
    row 2 i + 1 is (g, f, 0, 0) — r, the way back.  (Columns 2 and 3 belong to the propagation's blend; nothing here reads them.)"""
    rows = []
    for f, g in chain(frames, anchor):
        rows += [(f, g, 0, 0), (g, f, 0, 0)]
    return np.asarray(rows, np.int32).reshape(-1, 4)


def check_size(h: int, w: int, who: str = "mask tracking") -> None:
    m = BLOCK << (LEVELS - 1)
    if h < m or w < m or h % m or w % m:
        raise ValueError(f"{who}: frames of {h}x{w}: H and W must be multiples of {m} (four pyramid levels of 8 x 8 blocks) — choose --H and --W so")


def check_dilate(radius: int) -> None:
    if not 0 <= int(radius) <= DILATE_MAX:
        raise ValueError(f"--mask_dilate {radius} is outside 0 ... {DILATE_MAX}")


def track_clip(source_u8, anchor_mask, anchor: int, pair_chunk: Optional[int] = None):
    """source_u8: uint8 (F, H, W, 3) on the device, all source frames at the output size; anchor_mask: uint8 (H, W), 0 / 255, painted on
    frame `anchor`.  -> uint8 (F, H, W): the mask of every frame ([anchor] is anchor_mask byte for byte).  Four stages: the pyramid once,
    matching for all 2 (F - 1) adjacent pairs, select in launches of at most `pair_chunk` pairs (PAIR_CHUNK; a multiple of 2), and the
    two chains of steps, each step as soon as its two vector fields exist."""
    import torch
    from . import ops
    from .propagate import match_pairs
    for t, name, dims in ((source_u8, "source_u8", 4), (anchor_mask, "anchor_mask", 2)):
        if t.dtype != torch.uint8 or not t.is_cuda or t.dim() != dims:
            raise ValueError(f"track_clip: {name} must be a cuda uint8 tensor of {dims} dimensions, got {t.dtype} {t.device} {tuple(t.shape)}")
    n, h, w, c = source_u8.shape
    if c != 3:
        raise ValueError(f"track_clip: source_u8 {tuple(source_u8.shape)}: RGB frames (F, H, W, 3)")
    check_size(h, w, "track_clip")
    if tuple(anchor_mask.shape) != (h, w):
        raise ValueError(f"track_clip: anchor_mask {tuple(anchor_mask.shape)} for frames of {h}x{w}")
    chunk = PAIR_CHUNK if pair_chunk is None else int(pair_chunk)
    if chunk < 2 or chunk % 2:
        raise ValueError(f"track_clip: pair_chunk={chunk} must be a positive multiple of 2 (a frame's two pairs stay together)")
    rows = pair_rows(n, int(anchor))
    dev = source_u8.device
    masks = torch.empty((n, h, w), dtype=torch.uint8, device=dev)
    masks[anchor] = anchor_mask
    if rows.shape[0] == 0:
        return masks
    pyr = ops.prop_pyramid(source_u8.contiguous())
    pairs = torch.from_numpy(rows).to(dev)
    vec = match_pairs(pyr, pairs, n, h, w)
    for s in range(0, rows.shape[0], chunk):
        sel = ops.masktrack_select(pyr, pairs[s:s + chunk], vec[s:s + chunk], n, h, w)
        for i in range(0, sel.shape[0], 2):
            f, g = int(rows[s + i, 0]), int(rows[s + i, 1])
            ops.masktrack_step(sel[i], sel[i + 1], masks[g], FB_LIMIT, out=masks[f])
    return masks


def finish(masks, dilate: int = 0, invert: bool = False):
    """What follows tracking — and applies to untracked masks too — in this order: the (2 dilate + 1)^2 square maximum, then 255 - m.
    At the defaults the masks come back as they are and nothing is launched."""
    from . import ops
    check_dilate(dilate)
    if not dilate and not invert:
        return masks
    return ops.mask_dilate(masks.contiguous(), int(dilate), bool(invert))
