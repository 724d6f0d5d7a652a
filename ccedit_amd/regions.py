"""Region prompts: a prompt per masked region of the frame, the regions' denoised latents fused at every sampler evaluation.

An edit run takes one prompt for the whole frame.  With K region masks and K region prompts ("the bear becomes a panda, the background
becomes a snow field") the network — unchanged, at its unchanged shape — is evaluated K + 1 times at EVERY network evaluation of the
sampler, once per text context (region 0 is the base prompt, which covers whatever the regions leave), and the K + 1 denoised latents
are fused into one by a fixed, normalised per-cell blend (MultiDiffusion along the conditioning axis; ccedit_amd/windows.py does the
same along time, ccedit_amd/tiles.py along space).  The sampler, the guider, the per-step noise, the inpainting re-injection, SDEdit,
the prior mix, `--window_frames` and `--tile_h / --tile_w` run exactly as before: all they ever see is the closure
`denoiser(input, sigma, cond)`, which RegionDenoiser wraps — OUTERMOST, around the plain, the windowed or the tiled closure.  Two
regions never disagree about their boundary, because there is one latent at every step.

  weights(masks, feather)   K pixel masks -> the (K + 1, T, h, w) coefficient table, one launch (csrc/region.hip)
  RegionDenoiser            the wrapped closure once per context -> fuse (one launch)

The arithmetic (normative restatement: tests/_regions_numpy.py).  Per latent cell, a_r = the region's pixels >= 128 (0 ... 64); s_r = a_r
summed over the (2F + 1) x (2F + 1) cells around it, coordinates clamped into the frame, so 0 <= s_r <= S = 64 (2F + 1)^2 and a mask that
fills the frame keeps full weight at the border; tot = sum_r s_r, D = max(S, tot), s_0 = D - tot; coef[r] = float32(float64(s_r) /
float64(D)) — formed from integers and rounded once, like windows.plan.  Every cell has a non-zero coefficient; where s_r = D the
region's coefficient is exactly 1.0 and the others exactly 0.0; overlapping regions share by their feathered coverage.  The fuse adds
coef[r] * y_r over ascending r, SKIPPING terms whose coefficient is exactly 0 (a non-finite value of a region that does not cover a
cell cannot reach it), the first term the product alone and every further one a multiply and then an add: a cell owned by one region
is a bit copy of that region's evaluation.

The cost, plainly: K + 1 network evaluations per sampler evaluation.  What is claimed: exact arithmetic and known shapes.  Nothing is
claimed about image quality; nobody has measured that.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Sequence

import torch

MAX_REGIONS = 7         # K: what one fuse launch walks per element is K + 1 tensors, and what the entry points accept
MAX_FEATHER = 8         # F, latent cells
DEFAULT_FEATHER = 1
CELL = 8                # pixels per latent cell side
THRESHOLD = 128         # a mask pixel is set when its byte is >= this (the edit masks' convention)


def check_counts(num_prompts: int, num_masks: int) -> int:
    """K of `--region_prompt` / `--region_mask` (ValueError with what to do)."""
    if num_prompts != num_masks:
        raise ValueError(f"{num_prompts} --region_prompt and {num_masks} --region_mask: region r is the r-th pair — give one mask per prompt")
    if num_prompts > MAX_REGIONS:
        raise ValueError(f"{num_prompts} regions: at most {MAX_REGIONS} (with the base prompt, {MAX_REGIONS + 1} evaluations per step) — merge "
                         f"regions that share a prompt into one mask")
    return num_prompts


def check_feather(feather: int) -> int:
    f = int(feather)
    if not 0 <= f <= MAX_FEATHER:
        raise ValueError(f"--region_feather {feather}: the blend is feathered over 0 ... {MAX_FEATHER} latent cells (8 pixels each) — "
                         f"give a value in that range")
    return f


def weights(masks: torch.Tensor, feather: int = DEFAULT_FEATHER) -> torch.Tensor:
    """uint8 (K, T, H, W) on the device -> the coefficient table fp32 (K + 1, T, H / 8, W / 8), one launch."""
    from . import ops
    if masks.dim() != 4 or not 1 <= masks.shape[0] <= MAX_REGIONS:
        raise ValueError(f"region masks {tuple(masks.shape)}: expected (K, T, H, W) with 1 <= K <= {MAX_REGIONS}")
    if masks.shape[2] % CELL or masks.shape[3] % CELL:
        raise ValueError(f"region masks of {masks.shape[2]}x{masks.shape[3]} px: a latent cell is {CELL} x {CELL} pixels — sides must be multiples of {CELL}")
    return ops.region_weights(masks.contiguous(), check_feather(feather))


class RegionDenoiser:
    """`denoiser(input, sigma, cond)` with a text context per region: input (2, 4, T, h, w), CFG-doubled by the guider; `contexts` the
    K + 1 conditional `crossattn` tensors (1, L, C) of ONE length L (77, or 77 n with long prompts), region 0 (the base prompt) first; `coef` the device table of weights().

    Per clip, not per evaluation: K + 1 stable doubled `crossattn` tensors — the unconditional half of cond['crossattn'] followed by
    region r's context — made once per source tensor (keyed by identity + in-place version, the entry pins the source: the discipline
    of ccedit_amd/caches.py) so that the network's text K / V cache and captured graphs see K + 1 stable tensors.  Every other entry of
    `cond` is handed on as the same object (the hint-stem cache holds ONE entry for all regions).  The CFG mark of `input` is forwarded
    to every call — no device compare, no host sync per evaluation.  `wrapper` (the network wrapper) is told how many contexts its
    per-clip caches must hold (reserve_contexts); the closure inside — plain, windowed, tiled — reserves its windows itself."""

    def __init__(self, denoiser: Callable, contexts: Sequence[torch.Tensor], coef: torch.Tensor, wrapper=None):
        self.denoiser = denoiser
        self.contexts = list(contexts)
        if not 2 <= len(self.contexts) <= MAX_REGIONS + 1:
            raise ValueError(f"{len(self.contexts)} contexts: the base prompt's and 1 ... {MAX_REGIONS} regions'")
        for ctx in self.contexts:
            if ctx.dim() != 3 or ctx.shape[0] != 1 or ctx.shape != self.contexts[0].shape:
                raise ValueError(f"region context {tuple(ctx.shape)}: expected (1, tokens, C), the same for every region — region masks belong to "
                                 f"one clip")
        if coef.dim() != 4 or coef.shape[0] != len(self.contexts):
            raise ValueError(f"coefficient table {tuple(coef.shape)} for {len(self.contexts)} contexts: expected (K + 1, T, h, w)")
        self.coef = coef
        self.wrapper = wrapper
        self._doubled = None                                     # (source, version, [doubled crossattn per region])

    def _region_contexts(self, crossattn: torch.Tensor) -> List[torch.Tensor]:
        ent = self._doubled
        if ent is None or ent[0] is not crossattn or ent[1] != crossattn._version:
            if crossattn.dim() != 3 or crossattn.shape[0] != 2 or crossattn.shape[1:] != self.contexts[0].shape[1:]:
                raise ValueError(f"crossattn {tuple(crossattn.shape)}: expected the CFG-doubled (2, {self.contexts[0].shape[1]}, "
                                 f"{self.contexts[0].shape[2]}) of ONE clip — region masks belong to one clip")
            uncond = crossattn[:1]
            doubled = [torch.cat((uncond, ctx.to(device=crossattn.device, dtype=crossattn.dtype)), 0) for ctx in self.contexts]
            ent = self._doubled = (crossattn, crossattn._version, doubled)
            if self.wrapper is not None and hasattr(self.wrapper, "reserve_contexts"):
                self.wrapper.reserve_contexts(len(doubled))
        return ent[2]

    def __call__(self, input: torch.Tensor, sigma: torch.Tensor, cond: Dict) -> torch.Tensor:
        from . import ops
        if input.dim() != 5 or tuple(input.shape[2:]) != tuple(self.coef.shape[1:]):
            raise ValueError(f"latent {tuple(input.shape)} against a coefficient table {tuple(self.coef.shape)}: expected (B, 4, T, h, w) with the "
                             f"table's T, h, w")
        ys = []
        for ctx in self._region_contexts(cond["crossattn"]):
            ci = dict(cond)
            ci["crossattn"] = ctx
            # `input` itself goes to every call: the `_cfg_twin_halves` mark the guider put on it travels with the object
            ys.append(self.denoiser(input, sigma, ci).float().contiguous())
        return ops.region_fuse(ys, self.coef)
