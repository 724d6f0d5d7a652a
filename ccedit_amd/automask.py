"""Automatic edit masks: the mask of `--inpainting_mode` from a source prompt and a target prompt, no painted mask needed.

DiffEdit's mask step (Couairon et al., 2022) on this project's sampler evaluation.  The encoded clip z is noised part of the way,
x_k = z + sigma e_k, and the network is asked for its prediction under the source prompt and under the target prompt; where the two
disagree is where the edit has to happen.  A sampler evaluation here is a CFG-doubled batch of two text contexts over one latent, so ONE
evaluation with (source prompt, target prompt) in the two halves gives one sample of that difference at the cost of an ordinary step.
The samples' differences are summed, scaled by a high quantile, thresholded, cleaned by a 3 x 3 x 3 majority vote over space AND time
(specks and one-frame flicker go — the video-specific part) and expanded to the pixel mask every other mask of the project is.

  AutoMask(closure, wrapper)(z, sigma, c_src, c_tgt, samples, seed) -> acc     `samples` network evaluations, one accumulate launch each
  mask_from(acc, quantile, threshold, votes) -> uint8 (B, T, 8h, 8w)           kth value, binarize, vote, expand: four launches

The arithmetic (normative restatement: tests/_automask_numpy.py; kernels: csrc/automask.hip).
  acc[b, t, p] (+)= ((|y[B+b, 0] - y[b, 0]| + |... 1 ...|) + |... 2 ...|) + ...      fp32, channels ascending; sample 0 stores, later add
  rank = min(n, max(1, ceil(q n))), n = T h w; scale[b] = the rank-th smallest of acc[b] (exact, stays on the device)
  bin = acc > float32(theta) * scale[b]                                          one fp32 multiply, strictly greater
  vote = (sum of bin over dt, dy, dx in {-1, 0, 1}, coordinates clamped) >= V      V = 0: no launch
  pixel mask = 255 where vote, over the 8 x 8 pixels of the cell                   ops.mask_latent of it is `vote` again, byte for byte

The `closure` is the one the sampler gets — plain, windowed (`--window_frames`: the mask of a long clip through the windows) or tiled
(`--tile_h / --tile_w`) — so the mask costs `samples` sampler evaluations and nothing else of size.  The guest leaves no trace: its
noise comes from a CPU generator of its own (no draw from the global CPU or device generators, which the edit uses), and the network
wrapper's per-clip caches, reservations and captured graphs are put back as they were found.

What is claimed: exact arithmetic and a measured cost.  Nothing is claimed about the quality of the masks on real footage; nobody has
measured that.
"""
from __future__ import annotations

import math
from typing import Callable, Dict, List, Optional, Sequence, Union

import torch

MAX_SAMPLES = 16
DEFAULT_SAMPLES = 4
DEFAULT_STRENGTH = 0.5
DEFAULT_QUANTILE = 0.99
DEFAULT_THRESHOLD = 0.5
DEFAULT_VOTE = 14           # a majority of the 27 cells
MAX_VOTE = 27
GUIDER = "sgm.modules.diffusionmodules.guiders.VanillaCFGTV2V"


def rank_of(q: float, n: int) -> int:
    """The 1-based rank (as torch.kthvalue) of the q-quantile among n cells: min(n, max(1, ceil(q n))), in float64 on the host."""
    return min(int(n), max(1, int(math.ceil(float(q) * int(n)))))


def check_options(samples: int, strength: float, quantile: float, threshold: float, votes: int) -> None:
    """`--mask_auto_samples / _strength / _quantile / _threshold / _vote` (ValueError with what to do), before any video is opened."""
    if not 1 <= int(samples) <= MAX_SAMPLES:
        raise ValueError(f"--mask_auto_samples {samples}: every sample is one network evaluation, 1 ... {MAX_SAMPLES} of them — give a value "
                         f"in that range (default {DEFAULT_SAMPLES})")
    if not (0.0 < float(strength) <= 1.0):
        raise ValueError(f"--mask_auto_strength {strength}: the noise level is the first sigma of --sdedit_denoise_strength's schedule — give "
                         f"a value in (0, 1] (default {DEFAULT_STRENGTH})")
    if not (0.0 <= float(quantile) <= 1.0):
        raise ValueError(f"--mask_auto_quantile {quantile}: the scale of a clip is a quantile of its difference map — give a value in "
                         f"[0, 1] (default {DEFAULT_QUANTILE})")
    if not (0.0 <= float(threshold) < float("inf")):
        raise ValueError(f"--mask_auto_threshold {threshold}: a cell is set where its difference exceeds this fraction of the scale — give "
                         f"a finite value that is not negative (default {DEFAULT_THRESHOLD})")
    if not 0 <= int(votes) <= MAX_VOTE:
        raise ValueError(f"--mask_auto_vote {votes}: a cell stays where at least this many of the 27 cells around it (3 x 3 in space, 3 in "
                         f"time) are set — give 0 (no vote) ... {MAX_VOTE} (default {DEFAULT_VOTE})")


def nearest_keyframe(indices: Sequence[int], num_frames: int) -> List[int]:
    """For every source frame 0 ... num_frames - 1 the position (in `indices`) of its nearest keyframe; a tie goes to the earlier one."""
    idx = [int(i) for i in indices]
    if not idx:
        raise ValueError("no keyframes")
    out = []
    for f in range(int(num_frames)):
        best = 0
        for k in range(1, len(idx)):
            if abs(f - idx[k]) < abs(f - idx[best]):          # strictly: the earlier keyframe keeps a tie
                best = k
        out.append(best)
    return out


def generator(seed: int) -> torch.Generator:
    """The CPU generator of the automatic mask: the posterior draw of the encode and the samples' noise come from it, in that order."""
    return torch.Generator().manual_seed(int(seed))


class AutoMask:
    """`closure(input, sigma, cond)` is what the sampler gets.  __call__ evaluates it `samples` times on z + sigma e_k with the source
    prompt's conditioning in the first half of the doubled batch and the target prompt's in the second, and sums the absolute
    differences of the halves over the channels -> acc fp32 (B, T, h, w) on the device.

    Per clip, not per evaluation: ONE doubled `crossattn` (source rows, target rows) and ONE doubled `control_hint`, made by a guider
    of this object's own (VanillaCFGTV2V.prepare_inputs: the uc argument comes first, concatenations are kept per source pair), so the
    network's text K / V cache, hint-stem cache and captured graphs see stable tensors.  `wrapper` (the network wrapper) is told that
    ONE text context is evaluated per window (reserve_contexts(1)); its caches, reservations and graphs are snapshotted before and put
    back after the call.  The noise is drawn from `seed` — an int, or the torch.Generator of `generator()` when the caller has already
    drawn the encode's posterior noise from it — never from a global generator."""

    def __init__(self, closure: Callable, wrapper=None):
        from .config import instantiate_from_config
        self.closure = closure
        self.wrapper = wrapper
        self.guider = instantiate_from_config(dict(target=GUIDER, params=dict(scale=1.0)))

    def evaluate(self, x: torch.Tensor, sigma: float, c_src: Dict, c_tgt: Dict) -> torch.Tensor:
        """One doubled evaluation -> fp32 (2B, C, T, h, w), the source-prompt half first."""
        s = torch.full((x.shape[0],), float(sigma), dtype=torch.float32)
        return self.closure(*self.guider.prepare_inputs(x, s, c_tgt, c_src)).float().contiguous()

    def __call__(self, z: torch.Tensor, sigma: float, c_src: Dict, c_tgt: Dict, samples: int,
                 seed: Union[int, torch.Generator]) -> torch.Tensor:
        from . import ops
        if z.dim() != 5 or not z.is_cuda:
            raise ValueError(f"latent {tuple(z.shape)} on {z.device}: expected (B, 4, T, h, w) on the GPU")
        if not 1 <= int(samples) <= MAX_SAMPLES:
            raise ValueError(f"{samples} samples: 1 ... {MAX_SAMPLES}")
        if set(c_src) != set(c_tgt):
            raise ValueError(f"the source conditioning has {sorted(c_src)}, the target's {sorted(c_tgt)}: the two differ in the text alone")
        gen = seed if isinstance(seed, torch.Generator) else generator(seed)
        z = z.float().contiguous()
        w = self.wrapper
        state = w.cache_state() if w is not None and hasattr(w, "cache_state") else None
        if w is not None and hasattr(w, "reserve_contexts"):
            w.reserve_contexts(1)
        acc = None
        try:
            for _ in range(int(samples)):
                e = torch.randn(z.shape, generator=gen).to(z.device)
                x = ops.axpby(z, e, 1.0, float(sigma))
                acc = ops.automask_accumulate(self.evaluate(x, sigma, c_src, c_tgt), acc)
        finally:
            if state is not None:
                torch.cuda.current_stream().synchronize()        # (graphs of this call are dropped with the state: let them finish)
                w.restore_cache_state(state)
        return acc


def check_finite(acc: torch.Tensor, names: Optional[Sequence[str]] = None) -> None:
    """A difference map that is not finite is a ValueError naming the clip (one reduction and one read-back per chunk)."""
    ok = torch.isfinite(acc).flatten(1).all(dim=1).cpu().tolist()
    for b, good in enumerate(ok):
        if not good:
            name = names[b] if names else f"clip {b}"
            raise ValueError(f"--mask_auto: the difference map of {name} is not finite (a NaN or an infinity in the network's output under the "
                             f"source or the target prompt): no mask can be made from it")


def mask_from(acc: torch.Tensor, quantile: float = DEFAULT_QUANTILE, threshold: float = DEFAULT_THRESHOLD, votes: int = DEFAULT_VOTE,
              names: Optional[Sequence[str]] = None, latent: bool = False) -> torch.Tensor:
    """acc fp32 (B, T, h, w) on the device -> the pixel mask uint8 (B, T, 8h, 8w) in {0, 255} (`latent`: the voted latent mask (B, T, h,
    w) in {0, 1} instead).  The scale never leaves the device."""
    from . import ops
    if acc.dim() != 4 or acc.dtype != torch.float32 or not acc.is_cuda:
        raise ValueError(f"difference map {acc.dtype} {tuple(acc.shape)} on {acc.device}: expected fp32 (B, T, h, w) on the GPU")
    check_options(1, 1.0, quantile, threshold, votes)
    acc = acc.contiguous()
    check_finite(acc, names)
    b = acc.shape[0]
    n = acc[0].numel()
    scale = ops.kth_values(acc.view(b, n), [rank_of(quantile, n)]).view(b)
    m = ops.automask_binarize(acc, scale, float(threshold))
    if int(votes) > 0:
        m = ops.automask_vote(m, int(votes))
    return m if latent else ops.automask_expand(m)
