"""Motion-following noise: the noise a run draws is carried along the source's motion from keyframe to keyframe (`--noise_warp`,
DESIGN.md section 3.27).

Every draw of a run — the start latent, the ancestral noise of every step, the re-injection noise of --inpainting_mode — is white and
independent per keyframe, so only the network's temporal attention holds fine texture still on a moving surface.  Here it is decided
once per clip which noise sample every latent cell (8 x 8 pixels, one block of the matcher) of every keyframe inherits from an earlier
keyframe: block vectors between adjacent source frames in both directions (propagate.match_pairs, unchanged) -> every cell's centre
followed back to the previous keyframe, dropped where it leaves the frame or the two directions disagree by more than FB_LIMIT ->
through the previous keyframe's origins the position the sample had when it was first drawn; of the cells of a keyframe that arrive at
one sample the smallest index keeps it and the others draw fresh -> an index map `src` (K, cells) into the flattened (K, cells) noise
of the clip.  Applying it is a gather: every frame reads distinct samples, so the noise of every single frame stays exactly white,
and every operation is a bit copy, equal bit for bit to the numpy restatement the tests carry; there is no host fallback.  This
module holds what the host decides: the constants, the refusals, the clip's build and the wrap around a sampler's noise source.
"""
from __future__ import annotations

import math
from typing import Sequence

import numpy as np

from .masktrack import check_size, pair_rows

# ---- the constants of the algorithm: this is their one place on the host (csrc/noisewarp.hip restates VEC_MAX)
CELL = 8                    # a latent cell is 8 x 8 pixels = one block of the matcher
FB_LIMIT = 4                # largest |v(p) + r(q)|_1 of a consistent correspondence
VEC_MAX = 64                # block vectors are clamped into +-VEC_MAX where the kernel reads them (the matcher's own reach is 46)
TABLE_MAX = 2 ** 32 - 1     # K * cells must stay below it: a claim is k * cells + (cells - 1 - idx) + 1 in 32 bits
INDEX_MAX = 2 ** 31         # ... and below this: the index map is int32


def check_rho(rho: float) -> None:
    if not (isinstance(rho, (int, float)) and 0.0 <= float(rho) <= 1.0):
        raise ValueError(f"--noise_warp_rho {rho} is outside 0 ... 1: it is the correlation of a keyframe's noise with the noise it inherits "
                         "(1 = carried exactly, 0 = independent) — give a value in that range")


def check_clip(keyframes: int, h: int, w: int) -> None:
    """Refused before any launch: sizes the matcher does not take and clips whose claims or indices leave 32 bits."""
    check_size(h, w, "--noise_warp")
    n = int(keyframes) * (h // CELL) * (w // CELL)
    if n >= TABLE_MAX or n >= INDEX_MAX:
        raise ValueError(f"--noise_warp: {keyframes} keyframes of {h // CELL}x{w // CELL} cells are {n} noise samples per channel, more than "
                         f"the 32-bit index map holds ({INDEX_MAX - 1}) — lower --num_keyframes or the frame size")


def keys_of(key_index: Sequence[int], frames: int) -> np.ndarray:
    idx = np.asarray([int(i) for i in key_index], np.int64)
    if idx.size < 1 or idx.min() < 0 or idx.max() >= frames:
        raise ValueError(f"--noise_warp: keyframe indices {idx.tolist()} outside the video's {frames} frames")
    if (np.diff(idx) <= 0).any():
        raise ValueError(f"--noise_warp: keyframe indices {idx.tolist()} are not strictly increasing: the video ({frames} frames) is too short "
                         "for this many keyframes at this frame-rate ratio — lower --num_keyframes or raise --target_fps")
    return idx


def build(source_u8, key_index):
    """source_u8: uint8 (F, H, W, 3) on the device, all source frames at the output size; key_index: the keyframes' frame numbers (K,),
    strictly increasing.  -> (src int32 (K, cells) on the device, shares: list of K floats, the share of cells of every keyframe that
    inherit — 0.0 for keyframe 0).  Only the frames key[0] ... key[K - 1] take part: the pyramid once, matching for every adjacent pair
    in both directions, one track launch, a claim and a resolve launch per keyframe; the counts come back to the host once."""
    import torch
    from . import ops
    from .propagate import match_pairs
    if source_u8.dtype != torch.uint8 or not source_u8.is_cuda or source_u8.dim() != 4 or source_u8.shape[3] != 3:
        raise ValueError(f"noisewarp.build: source_u8 must be a cuda uint8 tensor (F, H, W, 3), got {source_u8.dtype} {source_u8.device} "
                         f"{tuple(source_u8.shape)}")
    n_all, h, w, _ = source_u8.shape
    key = keys_of(key_index, n_all)
    check_clip(key.size, h, w)
    cells = (h // CELL) * (w // CELL)
    dev = source_u8.device
    if key.size == 1:
        return torch.arange(cells, dtype=torch.int32, device=dev)[None].contiguous(), [0.0]
    first, n = int(key[0]), int(key[-1] - key[0]) + 1
    part = source_u8[first:first + n].contiguous()
    pyr = ops.prop_pyramid(part)
    pairs = torch.from_numpy(pair_rows(n, 0)).to(dev)              # for frame f: (f, f - 1), then (f - 1, f)
    vec = match_pairs(pyr, pairs, n, h, w)
    track = ops.noisewarp_track(vec, (key - first).tolist(), h, w, FB_LIMIT)
    _, src, inherited = ops.noisewarp_origins(track, h, w)
    return src, [float(c) / cells for c in inherited.cpu().tolist()]


def wrap(raw_sampler, src, rho: float = 1.0):
    """raw_sampler: a noise source, x -> noise of x's shape (a sampler's noise_sampler, or torch.randn_like); src: int32 (B, K, cells) on
    the device, one map per clip of the chunk.  -> a callable of the same kind.  For a 5-D x of the maps' shape (B, C, K, h, w): at
    rho = 1 one raw draw, gathered; at 0 <= rho < 1 a second raw draw e and rho * warped + sqrt(1 - rho^2) * e (ops.axpby) — unit
    variance again, correlated by rho with what the cell inherits.  Whatever else is asked for is the raw source's, unchanged."""
    import torch
    from . import ops
    check_rho(rho)
    rho = float(rho)
    if src.dtype != torch.int32 or not src.is_cuda or src.dim() != 3:
        raise ValueError(f"noisewarp.wrap: src must be a cuda int32 map (B, K, cells), got {src.dtype} {src.device} {tuple(src.shape)}")
    src = src.contiguous()
    ops.noisewarp_check(src)                                       # once per map: the draws below skip it
    b, k, cells = src.shape

    def sampler(x):
        if not (torch.is_tensor(x) and x.dim() == 5 and x.shape[0] == b and x.shape[2] == k and x.shape[3] * x.shape[4] == cells):
            return raw_sampler(x)
        warped = ops.noise_warp(raw_sampler(x).float().contiguous(), src, checked=True)
        if rho == 1.0:
            return warped
        e = raw_sampler(x).float().contiguous()
        return ops.axpby(warped, e, rho, math.sqrt(1.0 - rho * rho))

    return sampler
