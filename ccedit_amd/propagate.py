"""Full-frame-rate output: the edited keyframes carried to every source frame between them (`--propagate`).

For an in-between frame f with keyframes a < f < b the motion f -> a and f -> b is estimated on the SOURCE frames (hierarchical block
matching on luma), the two edited keyframes are warped along it and blended by distance and by how well the warped source matches
the source frame.  All of it is integer arithmetic on bytes in ccedit_amd/csrc/propagate.hip, equal bit for bit to the numpy
restatement the tests carry; there is no host fallback.  This module holds what the host decides: the constants, the two tables,
which frame is produced from which pair (plan), and the loop over a clip (propagate_clip).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

# ---- the constants of the algorithm: this is their one place; kernels receive them as arguments or tables
LEVELS = 4                  # pyramid levels (H and W must be multiples of 8 << (LEVELS - 1) = 64)
BLOCK = 8                   # blocks are 8 x 8 on every level
APRON = 4                   # the compared patch is the block plus this many pixels on every side (16 x 16)
RADIUS_COARSEST = 4         # search +-4 around zero on the coarsest level
RADIUS_FINER = 2            # ... +-2 around twice the parent's vector on every finer one
BOX = 5                     # side of the box mean of the matching error
G_SCALE = 4096              # g(0)
G_SIGMA = 6.0               # g(e) = G_SCALE / (1 + (e / G_SIGMA)^2)
MAX_DIST = 255              # largest distance between neighbouring keyframes (the blend's weights stay inside 32 bits)
PAIR_CHUNK = 64             # pairs per launch: bounds the workspace (two warped RGB + luma frames per pair); results do not depend on it


def radius_of(level: int) -> int:
    return RADIUS_COARSEST if level == LEVELS - 1 else RADIUS_FINER


def rank_table(radius: int) -> np.ndarray:
    """int32 [(2R + 1)^2] indexed by (dy + R) (2R + 1) + dx + R: the candidate's place in the order (|dy| + |dx|, dy, dx).  The matching
    key is SAD * 256 + rank: on flat content the prediction (rank 0) wins, and the minimum does not depend on evaluation order."""
    n = 2 * radius + 1
    order = sorted((abs(dy) + abs(dx), dy, dx) for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1))
    tab = np.empty(n * n, np.int32)
    for r, (_, dy, dx) in enumerate(order):
        tab[(dy + radius) * n + dx + radius] = r
    return tab


def g_table() -> np.ndarray:
    """int32 [256]: the weight of a side whose warped source differs from the source frame by a local mean of e grey levels."""
    e = np.arange(256, dtype=np.float64)
    return np.maximum(1, np.round(G_SCALE / (1.0 + (e / G_SIGMA) ** 2))).astype(np.int32)


@dataclass
class Plan:
    key_index: np.ndarray       # (N,) the keyframes' source frame numbers, strictly increasing
    frames: np.ndarray          # (NF,) the in-between frames, ascending
    pairs: np.ndarray           # (2 NF, 4) int32 rows (f, k, ordinal of k among the keyframes, weight = distance to the OTHER keyframe)

    @property
    def first(self) -> int:
        return int(self.key_index[0])

    @property
    def last(self) -> int:
        return int(self.key_index[-1])

    @property
    def num_out(self) -> int:
        return self.last - self.first + 1


def plan(indices: Sequence[int], num_frames: int) -> Plan:
    """Which frames are produced from which pair of keyframes.  Refused (ValueError, with what to do about it): fewer than two
    keyframes, indices outside the video, indices that are not strictly increasing (what keyframe_indices' linspace fallback gives on a
    video that is too short), neighbouring keyframes further apart than MAX_DIST."""
    idx = np.asarray([int(i) for i in indices], np.int64)
    if idx.size < 2:
        raise ValueError(f"propagation needs at least two keyframes, got {idx.size}: raise --num_keyframes")
    if idx.min() < 0 or idx.max() >= num_frames:
        raise ValueError(f"keyframe indices {idx.tolist()} outside the video's {num_frames} frames")
    if (np.diff(idx) <= 0).any():
        raise ValueError(f"keyframe indices {idx.tolist()} are not strictly increasing: the video ({num_frames} frames) is too short for this many "
                         "keyframes at this frame-rate ratio — lower --num_keyframes or raise --target_fps")
    if np.diff(idx).max() > MAX_DIST:
        raise ValueError(f"neighbouring keyframes {int(np.diff(idx).max())} frames apart: at most {MAX_DIST} (raise --target_fps)")
    frames, pairs = [], []
    for n in range(idx.size - 1):
        a, b = int(idx[n]), int(idx[n + 1])
        for f in range(a + 1, b):
            frames.append(f)
            pairs.append((f, a, n, b - f))
            pairs.append((f, b, n + 1, f - a))
    return Plan(idx, np.asarray(frames, np.int64), np.asarray(pairs, np.int32).reshape(-1, 4))


_TABLES = {}


def device_tables(device):
    """(rank tables per level, g) on `device`, uploaded once."""
    import torch
    key = str(device)
    if key not in _TABLES:
        _TABLES[key] = ([torch.from_numpy(rank_table(radius_of(lv))).to(device) for lv in range(LEVELS)], torch.from_numpy(g_table()).to(device))
    return _TABLES[key]


def match_pairs(pyr, pairs, frames: int, h: int, w: int, rank_tabs=None):
    """Coarse to fine over all pairs of the call -> level-0 block vectors int32 (P, h / 8, w / 8, 2)."""
    from . import ops
    ranks = device_tables(pyr.device)[0] if rank_tabs is None else rank_tabs
    vec = None
    for lv in range(LEVELS - 1, -1, -1):
        vec = ops.prop_match(pyr, pairs, ranks[lv], vec, frames, h, w, lv, radius_of(lv))
    return vec


def propagate_clip(source_u8, key_index, edited_u8, masks=None, pair_chunk: Optional[int] = None):
    """source_u8: uint8 (F, H, W, 3) on the device, all source frames at the output size; key_index: the keyframes' frame numbers (N,);
    edited_u8: uint8 (N, H, W, 3), the edited keyframes; masks: None, or uint8 (F, H, W) (>= 128 = edit) — an in-between frame keeps the
    source where ITS OWN mask is clear.  -> uint8 (key_index[-1] - key_index[0] + 1, H, W, 3): keyframe positions hold edited_u8 byte for
    byte.  All pairs of a clip go through every stage in launches of at most `pair_chunk` pairs (PAIR_CHUNK; a multiple of 2)."""
    import torch
    from . import ops
    for t, name, dims in ((source_u8, "source_u8", 4), (edited_u8, "edited_u8", 4)) + (((masks, "masks", 3),) if masks is not None else ()):
        if t.dtype != torch.uint8 or not t.is_cuda or t.dim() != dims:
            raise ValueError(f"propagate_clip: {name} must be a cuda uint8 tensor of {dims} dimensions, got {t.dtype} {t.device} {tuple(t.shape)}")
    nf_all, h, w, _ = source_u8.shape
    p = plan(key_index, nf_all)
    if tuple(edited_u8.shape) != (len(p.key_index), h, w, 3):
        raise ValueError(f"propagate_clip: edited_u8 {tuple(edited_u8.shape)} for {len(p.key_index)} keyframes of {h}x{w}")
    if h % (BLOCK << (LEVELS - 1)) or w % (BLOCK << (LEVELS - 1)):
        raise ValueError(f"propagate_clip: frames of {h}x{w}: H and W must be multiples of {BLOCK << (LEVELS - 1)}")
    if masks is not None and tuple(masks.shape) != (nf_all, h, w):
        raise ValueError(f"propagate_clip: masks {tuple(masks.shape)} for {nf_all} frames of {h}x{w}")
    chunk = PAIR_CHUNK if pair_chunk is None else int(pair_chunk)
    if chunk < 2 or chunk % 2:
        raise ValueError(f"propagate_clip: pair_chunk={chunk} must be a positive multiple of 2 (a frame's two pairs stay together)")
    dev = source_u8.device
    first, n_out = p.first, p.num_out
    src = source_u8[first:first + n_out].contiguous()              # only the frames between the first and the last keyframe take part
    msk = None if masks is None else masks[first:first + n_out].contiguous()
    edited = edited_u8.contiguous()
    out = torch.empty((n_out, h, w, 3), dtype=torch.uint8, device=dev)
    out[torch.from_numpy(p.key_index - first).to(dev)] = edited
    if len(p.frames) == 0:
        return out
    pairs_host = p.pairs.copy()
    pairs_host[:, :2] -= first
    _, g = device_tables(dev)
    pyr = ops.prop_pyramid(src)
    luma0 = ops.prop_level(pyr, n_out, h, w, 0)
    for s in range(0, pairs_host.shape[0], chunk):
        rows = pairs_host[s:s + chunk]
        pairs = torch.from_numpy(np.ascontiguousarray(rows)).to(dev)
        vec = match_pairs(pyr, pairs, n_out, h, w)
        w_rgb = ops.prop_warp(edited, vec, pairs, 2)
        w_luma = ops.prop_warp(luma0, vec, pairs, 1)
        frames = ops.prop_blend(w_rgb, w_luma, pyr, pairs, g, n_out, rgb=src if msk is not None else None, mask=msk)
        out[torch.from_numpy(rows[0::2, 0].astype(np.int64)).to(dev)] = frames
    return out
