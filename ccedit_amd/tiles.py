"""Large frames: a frame above the one size the network is built for, the tiles fused at every sampler evaluation.

The network, its kernels' fast paths, the captured graphs and the checkpoints are built and measured for ONE frame size (512 x 768 at
the top, a latent of 64 x 96).  A larger frame — any size that is a multiple of 8 pixels — is covered by overlapping tiles of that
one size.  At EVERY network evaluation of the sampler each tile goes through the unchanged network at the unchanged shape, and the
tiles' denoised latents are fused into one denoised latent of the frame by a fixed, normalised cross-fade (MultiDiffusion along
height and width; ccedit_amd/windows.py does the same along time).  The sampler, the guider, the per-step noise, the inpainting
re-injection, SDEdit, the prior mix and `--window_frames` run on the large latent exactly as on a small one: all they ever see is the
closure `denoiser(input, sigma, cond)`, which TiledDenoiser wraps.  A latent element in an overlap is the same number in every tile
that holds it, at every step, so there is no seam to hide afterwards.

  plan2d(lh, lw, th, tw, oh, ow)   tile starts and cross-fade coefficients (host, integers -> one fp32 rounding per coefficient)
  TiledDenoiser                    gather (one launch) -> the wrapped closure once per tile -> fuse (one launch); csrc/tile.hip
  first_stage_group                frames per first-stage call so that no VAE tensor outgrows a plain clip's at tile size

What is claimed: exact arithmetic, known shapes, the new range of frame sizes.  Nothing is claimed about image quality against a
direct evaluation at the large size; nobody has measured that.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Tuple

import numpy as np
import torch

from . import windows

MAX_TILES = 64          # what one fuse launch walks per element, and what the entry points accept


def _raw(t: int) -> np.ndarray:
    return np.array([min(k + 1, t - k) for k in range(t)], dtype=np.int64)


def plan2d(lh: int, lw: int, th: int, tw: int, oh: int, ow: int) -> Tuple[List[Tuple[int, int]], np.ndarray]:
    """(starts, coef) of the tiles of th x tw that cover a latent of lh x lw, neighbours sharing oh rows / ow columns (the last tile of
    an axis is pulled back to end with the frame, so it may share more).  All in latent units (8 pixels).

    starts: per axis windows.plan's rule — k * (t - o) while that tile ends before the frame does, then n - t — and the Cartesian
            product of the two lists, y major, x minor, ascending: [(sy, sx), ...].
    coef:   float32 (tiles, th, tw).  The raw weight of position (i, j) of a tile is the integer r_h(i) * r_w(j), r(k) = min(k + 1, t - k);
            coef[t][i][j] = raw / D with D the integer sum of the raw weights, at that latent pixel, of all tiles covering it — the
            quotient formed in float64 from integers and rounded to fp32 once.  Where one tile covers a pixel the coefficient is 1.0."""
    lh, lw, th, tw, oh, ow = (int(v) for v in (lh, lw, th, tw, oh, ow))
    for name, t in (("height", th), ("width", tw)):
        if t < 8 or t % 8:
            raise ValueError(f"tile {name} of {t} latent pixels ({8 * t} px): a tile is evaluated by the network directly, which needs "
                             f"multiples of 8 latent pixels (64 px) — choose a tile size that is a multiple of 64 px")
    for name, t, o in (("height", th, oh), ("width", tw, ow)):
        if not 0 <= o < t:
            raise ValueError(f"tile overlap {o} along the {name} for a tile of {t} latent pixels: need 0 <= overlap < tile")
    for name, n, t in (("height", lh, th), ("width", lw, tw)):
        if n < t:
            raise ValueError(f"frame {name} of {n} latent pixels ({8 * n} px) does not fill one tile of {t} ({8 * t} px): choose a "
                             f"smaller tile, or run this size without tiles")
    ys, _ = windows.plan(lh, th, oh)
    xs, _ = windows.plan(lw, tw, ow)
    if len(ys) * len(xs) > MAX_TILES:
        raise ValueError(f"{len(ys)} x {len(xs)} = {len(ys) * len(xs)} tiles of {th}x{tw} over a latent of {lh}x{lw}: more than "
                         f"{MAX_TILES} — use a larger tile or a smaller overlap")
    starts = [(sy, sx) for sy in ys for sx in xs]
    raw = _raw(th)[:, None] * _raw(tw)[None, :]                      # int64 (th, tw)
    total = np.zeros((lh, lw), dtype=np.int64)
    for sy, sx in starts:
        total[sy:sy + th, sx:sx + tw] += raw
    coef = np.empty((len(starts), th, tw), dtype=np.float32)
    for t, (sy, sx) in enumerate(starts):
        coef[t] = (raw.astype(np.float64) / total[sy:sy + th, sx:sx + tw].astype(np.float64)).astype(np.float32)
    return starts, coef


def window_count(num_frames: int, window: int = 0, overlap: Optional[int] = None) -> int:
    """Windows per tile: windows.plan's count when `window` is set and the clip is longer than it, else 1."""
    n, t = int(num_frames), int(window or 0)
    if t <= 0 or n <= t:
        return 1
    return len(windows.plan(n, t, t // 2 if overlap is None else int(overlap))[0])


def first_stage_group(frames_plain: int, th: int, tw: int, lh: int, lw: int) -> int:
    """Frames per first-stage call (windows.GroupedFirstStage) for frames of lh x lw when a plain clip is `frames_plain` frames of
    th x tw: max(1, T_plain th tw // (lh lw)), so no first-stage tensor holds more elements than the plain clip's at tile size
    (a group of one frame is bounded by check_frame_cap instead)."""
    return max(1, int(frames_plain) * int(th) * int(tw) // (int(lh) * int(lw)))


MAX_FRAME_LATENT = 46339          # the largest L = lh lw with L (L + 3) < 2^31


def check_frame_cap(lh: int, lw: int) -> None:
    """The first stage is global (GroupNorm and the mid-block attention span the frame), so it runs on whole frames, in groups of
    first_stage_group frames: a group of more than one frame holds no more elements than a plain clip at tile size.  What grows with
    the frame and not with the group is refused here (ValueError) instead of being left to a kernel's index arithmetic: the mid-block
    attention's scores are materialised per frame as L x ceil4(L) fp32 with L = lh lw (vae.py / vae_f32.py: attn_block), and at most
    MAX_FRAME_LATENT latent pixels keep that matrix — the largest first-stage tensor of one frame, 256 channels at full resolution
    being 2^14 L elements — below 2^31 elements."""
    lh, lw = int(lh), int(lw)
    if lh * lw > MAX_FRAME_LATENT:
        raise ValueError(f"a frame of {8 * lh}x{8 * lw} px has {lh * lw} latent pixels, more than {MAX_FRAME_LATENT}: the first stage's "
                         f"mid-block attention holds a score matrix of that many rows and columns per frame (2^31 elements) — use a "
                         f"smaller frame")


def check_supported(wrapper=None, cond: Optional[Dict] = None, config=None) -> None:
    """Refuse, before any GPU work, what tiles do not cover (windows.check_supported's list, in tiles' words): conditioning on a
    reference image (`cond_feat` is one latent of the whole frame, TVI2V) and row- or frame-sharded evaluation of the network."""
    try:
        windows.check_supported(wrapper=wrapper, cond=cond, config=config)
    except NotImplementedError as e:
        raise NotImplementedError(str(e).replace("windowed sampling (--window_frames)", "tiled sampling (--tile_h / --tile_w)")
                                  .replace("one centre frame of one window", "the whole frame, not to a tile")
                                  .replace("the windows one at a time", "the tiles one at a time")) from None


class TiledDenoiser:
    """`denoiser(input, sigma, cond)` over frames of lh x lw from a closure that handles th x tw: input (B, 4, N, lh, lw), already
    CFG-doubled by the guider; cond['control_hint'] (B, 3, N, 8 lh, 8 lw).  A frame of exactly one tile is one tile with coefficients
    1.0 — the wrapped closure's own bits.

    Per clip, not per evaluation: the plan and its device tables (per frame size), and the tiles' conditioning — control_hint crops
    made contiguous once per source tensor (keyed by identity + in-place version; the entry pins the source) so that the network's
    hint-stem cache and captured graphs see stable tensors; every other entry of `cond` is handed on as the same object.  The CFG marks
    survive: a gather of twin halves is twin halves, a crop of equal halves has equal halves — no device compare, no host sync per
    evaluation.

    With `window` (`--window_frames`) the tiles are the outer loop: each tile has its own windows.WindowedDenoiser (built without the
    wrapper, so it reserves nothing itself) around the same closure, and `wrapper` is told ONCE how many conditioning keys are
    evaluated in turn: reserve_windows(tiles x windows)."""

    def __init__(self, denoiser: Callable, tile: Tuple[int, int], overlap: Optional[Tuple[int, int]] = None, wrapper=None,
                 window: int = 0, window_overlap: Optional[int] = None):
        self.denoiser = denoiser
        self.th, self.tw = int(tile[0]), int(tile[1])
        self.oh, self.ow = default_overlap(self.th, self.tw) if overlap is None else (int(overlap[0]), int(overlap[1]))
        plan2d(self.th, self.tw, self.th, self.tw, self.oh, self.ow)          # argument check, before any GPU work
        self.window, self.window_overlap = int(window or 0), window_overlap
        if self.window:
            windows.plan(self.window, self.window, self.window // 2 if window_overlap is None else int(window_overlap))
        self.wrapper = wrapper
        check_supported(wrapper=wrapper)
        self._tables = {}                                        # (lh, lw, N, device) -> (starts, starts_dev, coef_dev)
        self._hints = None                                       # (source, version, [crops])
        self._windowed = {}                                      # tile index -> its WindowedDenoiser

    def tables(self, lh: int, lw: int, num_frames: int, device, frame_contexts: bool = False):
        key = (int(lh), int(lw), int(num_frames), str(device)) + ((True,) if frame_contexts else ())
        if key not in self._tables:
            starts, coef = plan2d(lh, lw, self.th, self.tw, self.oh, self.ow)
            self._tables[key] = (starts, torch.tensor(starts, dtype=torch.int32, device=device).reshape(len(starts), 2),
                                 torch.from_numpy(coef).to(device))
            if self.wrapper is not None and hasattr(self.wrapper, "reserve_windows"):
                nw = window_count(num_frames, self.window, self.window_overlap)
                if frame_contexts and nw > 1:        # a per-frame text context is sliced per window inside every tile (windows.py)
                    self.wrapper.reserve_windows(len(starts) * nw, frame_contexts=True)
                else:
                    self.wrapper.reserve_windows(len(starts) * nw)
        return self._tables[key]

    def _tile_hints(self, hint: torch.Tensor, starts) -> List[torch.Tensor]:
        from . import ops
        ent = self._hints
        if ent is None or ent[0] is not hint or ent[1] != hint._version or len(ent[2]) != len(starts):
            if hint.dim() != 5:
                raise ValueError(f"control_hint {tuple(hint.shape)}: expected (B, 3, N, H, W)")
            same = ops.get_mark(hint, "_halves_equal")
            crops = []
            for sy, sx in starts:
                cr = hint[:, :, :, 8 * sy:8 * (sy + self.th), 8 * sx:8 * (sx + self.tw)].contiguous()
                if cr.shape == hint.shape:                       # one tile over the whole frame: the source itself, marks and all
                    cr = hint
                elif same is not None:
                    ops.set_mark(cr, "_halves_equal", same)
                crops.append(cr)
            ent = self._hints = (hint, hint._version, crops)
        return ent[2]

    def _closure(self, i: int, num_frames: int) -> Callable:
        if not self.window or num_frames <= self.window:
            return self.denoiser
        if i not in self._windowed:
            self._windowed[i] = windows.WindowedDenoiser(self.denoiser, self.window, self.window_overlap, wrapper=None)
        return self._windowed[i]

    def __call__(self, input: torch.Tensor, sigma: torch.Tensor, cond: Dict) -> torch.Tensor:
        from . import ops
        check_supported(cond=cond)
        x = input.float().contiguous()
        if x.dim() != 5:
            raise ValueError(f"latent {tuple(x.shape)}: expected (B, 4, N, h, w)")
        n, lh, lw = x.shape[2], x.shape[3], x.shape[4]
        hint = cond["control_hint"]
        if tuple(hint.shape[2:]) != (n, 8 * lh, 8 * lw):
            raise ValueError(f"control_hint {tuple(hint.shape)} does not match a latent of {n} frames of {lh}x{lw} (x8)")
        ctx = cond.get("crossattn")
        if torch.is_tensor(ctx) and ctx.dim() == 3 and n > 1 and ctx.shape[0] == x.shape[0] * n:      # (one text context per frame)
            starts, starts_dev, coef_dev = self.tables(lh, lw, n, x.device, True)
        else:
            starts, starts_dev, coef_dev = self.tables(lh, lw, n, x.device)
        hints = self._tile_hints(hint, starts)
        xt = ops.tile_gather(x, starts_dev, self.th, self.tw)
        twins = ops.get_mark(input, "_cfg_twin_halves") is True
        ys = []
        for i in range(len(starts)):
            xi = xt[i]
            if twins:
                ops.set_mark(xi, "_cfg_twin_halves", True)
            ci = dict(cond)
            ci["control_hint"] = hints[i]
            ys.append(self._closure(i, n)(xi, sigma, ci).float().contiguous())
        return ops.tile_fuse(ys, starts_dev, coef_dev, lh, lw)


def default_overlap(th: int, tw: int) -> Tuple[int, int]:
    """A quarter of the tile per axis.  In latent units: (th // 4, tw // 4); the flags' pixel default (a quarter of the tile in pixels
    rounded down to a multiple of 8) is the same number."""
    return int(th) // 4, int(tw) // 4
