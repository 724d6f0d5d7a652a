"""Long clips: more keyframes than one window of the network, the windows fused at every sampler evaluation.

The network, its kernels' fast paths and the checkpoints are built for ONE window of T keyframes (17 for the shipped models).  A clip
of N > T keyframes is covered by W overlapping windows of T frames.  At EVERY network evaluation of the sampler each window goes
through the unchanged network at the unchanged shape, and the windows' denoised latents are fused into one denoised latent of N frames
by a fixed, normalised cross-fade (MultiDiffusion along time).  The sampler, the guider, the per-step noise, the inpainting
re-injection, SDEdit and the prior mix run on the long latent exactly as on a short one: all they ever see is the closure
`denoiser(input, sigma, cond)`, which WindowedDenoiser wraps.  A frame in an overlap is the same latent in both windows at every step,
so there is no seam to hide afterwards — this fuses predictions, it does not edit chunks and glue videos.

  plan(N, T, overlap)      window starts and cross-fade coefficients (host, integers -> one fp32 rounding per coefficient)
  WindowedDenoiser         gather (one launch) -> the wrapped closure once per window -> fuse (one launch); csrc/window.hip
  GroupedFirstStage        first-stage encode / decode of N frames in groups of at most T (per-frame work: the same bits, known shapes)
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Tuple

import numpy as np
import torch

# conditioning with a time axis other than control_hint, or tied to ONE centre frame: not windowed (sampling_tv2v_ref.py, TVI2V)
# what a config that produces `cond_feat` contains: the VAEEmbedder on `cond_img`, the network's controlnet_img
_REF_CONFIG_WORDS = ("cond_feat", "cond_img", "VAEEmbedder", "controlnet_img_config")
_UNSUPPORTED_KEYS = ("cond_feat", "interpolate_first", "interpolate_last", "interpolate_first_last")


def plan(num_frames: int, window: int, overlap: int) -> Tuple[List[int], np.ndarray]:
    """(starts, coef) of the windows that cover `num_frames` frames with windows of `window` frames, consecutive windows sharing
    `overlap` frames (the last window is pulled back to end with the clip, so it may share more).

    starts: k * (T - overlap) while that window ends before the clip does, then N - T.  Strictly increasing, every frame covered.
    coef:   float32 (W, T).  The raw weight of position j of a window is the integer r(j) = min(j + 1, T - j) (a triangle: 1 at both
            ends); coef[w][j] = r(j) / D with D the sum of the raw weights, at that frame, of all windows covering it — formed from
            integers in float64 and rounded to fp32 once.  Where one window covers a frame the coefficient is exactly 1.0."""
    n, t, o = int(num_frames), int(window), int(overlap)
    if t < 1 or not 0 <= o < t:
        raise ValueError(f"window of {t} frames with overlap {o}: need window >= 1 and 0 <= overlap < window")
    if n < t:
        raise ValueError(f"{n} frames do not fill one window of {t}")
    step = t - o
    starts = []
    k = 0
    while k * step + t < n:
        starts.append(k * step)
        k += 1
    starts.append(n - t)
    raw = [min(j + 1, t - j) for j in range(t)]
    total = [0] * n
    for s in starts:
        for j in range(t):
            total[s + j] += raw[j]
    coef = np.empty((len(starts), t), dtype=np.float32)
    for w, s in enumerate(starts):
        for j in range(t):
            coef[w, j] = np.float32(np.float64(raw[j]) / np.float64(total[s + j]))
    return starts, coef


def check_supported(wrapper=None, cond: Optional[Dict] = None, config=None) -> None:
    """Refuse, before any GPU work, what windows do not cover: conditioning on one reference image (`cond_feat` belongs to one centre
    frame of one window) and row- or frame-sharded evaluation of the network."""
    if cond is not None:
        bad = [k for k in _UNSUPPORTED_KEYS if cond.get(k) is not None]
        if bad:
            raise NotImplementedError(f"windowed sampling (--window_frames) does not support the conditioning {bad}: a reference image "
                                      f"belongs to one centre frame of one window")
    if config is not None and any(k in str(config) for k in _REF_CONFIG_WORDS):
        raise NotImplementedError("windowed sampling (--window_frames) does not support configs with `cond_feat` (TVI2V): a reference "
                                  "image belongs to one centre frame of one window")
    if wrapper is not None and (getattr(wrapper, "frame_shard", None) is not None or getattr(wrapper, "row_shard", None) is not None):
        raise NotImplementedError("windowed sampling (--window_frames) evaluates the windows one at a time on one GPU: not with a "
                                  "row- or frame-sharded network wrapper")


class WindowedDenoiser:
    """`denoiser(input, sigma, cond)` over N frames from a closure that handles T: input (B, 4, N, h, w), already CFG-doubled by the
    guider; cond['control_hint'] (B, 3, N, H, W).  N == T is one window with coefficients 1.0 — the wrapped closure's own bits.

    Per clip, not per evaluation: the plan and its device tables (per N), and the windows' conditioning — control_hint slices made
    contiguous once per source tensor (keyed by identity + in-place version, the entry pins the source: the discipline of
    ccedit_amd/caches.py) so that the network's hint-stem cache and captured graphs see W stable tensors; every other entry of `cond` is
    handed on as the same object (the text K / V cache hits for all windows).  The CFG marks survive: a gather of twin halves is
    twin halves, a slice of equal halves has equal halves — no device compare, no host sync per evaluation.
    `wrapper` (the network wrapper) is told how many windows its per-clip caches must hold (reserve_windows)."""

    def __init__(self, denoiser: Callable, window: int, overlap: Optional[int] = None, wrapper=None):
        self.denoiser = denoiser
        self.window = int(window)
        self.overlap = self.window // 2 if overlap is None else int(overlap)
        plan(self.window, self.window, self.overlap)             # argument check, before any GPU work
        self.wrapper = wrapper
        check_supported(wrapper=wrapper)
        self._tables = {}                                        # (N, device) -> (starts, starts_dev, coef_dev)
        self._hints = None                                       # (source, version, [slices])
        self._ctxs = None                                        # (source, version, [slices]) of a per-frame text context

    def tables(self, num_frames: int, device, frame_contexts: bool = False):
        key = (int(num_frames), str(device)) + ((True,) if frame_contexts else ())
        if key not in self._tables:
            starts, coef = plan(num_frames, self.window, self.overlap)
            self._tables[key] = (starts, torch.tensor(starts, dtype=torch.int32, device=device), torch.from_numpy(coef).to(device))
            if self.wrapper is not None and hasattr(self.wrapper, "reserve_windows"):
                if frame_contexts:                               # (a slice of the text context per window: the text K / V cache grows)
                    self.wrapper.reserve_windows(len(starts), frame_contexts=True)
                else:
                    self.wrapper.reserve_windows(len(starts))
        return self._tables[key]

    def _window_contexts(self, ctx: torch.Tensor, b: int, n: int, starts: List[int]) -> List[torch.Tensor]:
        """A per-frame text context (B * N, L, C) in (b t) order (a prompt schedule) is sliced along the frame axis exactly as
        control_hint is: W stable tensors (B * T, L, C) per source tensor."""
        ent = self._ctxs
        if ent is None or ent[0] is not ctx or ent[1] != ctx._version or len(ent[2]) != len(starts):
            c5 = ctx.view(b, n, *ctx.shape[1:])
            slices = []
            for s in starts:
                sl = c5[:, s:s + self.window]
                slices.append(ctx if sl.shape[1] == n else sl.reshape(b * sl.shape[1], *ctx.shape[1:]).contiguous())
            ent = self._ctxs = (ctx, ctx._version, slices)
        return ent[2]

    def _window_hints(self, hint: torch.Tensor, starts: List[int]) -> List[torch.Tensor]:
        from . import ops
        ent = self._hints
        if ent is None or ent[0] is not hint or ent[1] != hint._version or len(ent[2]) != len(starts):
            if hint.dim() != 5:
                raise ValueError(f"control_hint {tuple(hint.shape)}: expected (B, 3, N, H, W)")
            same = ops.get_mark(hint, "_halves_equal")
            slices = []
            for s in starts:
                sl = hint[:, :, s:s + self.window].contiguous()
                if sl.shape == hint.shape:                       # one window over the whole clip: the source itself, marks and all
                    sl = hint
                elif same is not None:
                    ops.set_mark(sl, "_halves_equal", same)
                slices.append(sl)
            ent = self._hints = (hint, hint._version, slices)
        return ent[2]

    def __call__(self, input: torch.Tensor, sigma: torch.Tensor, cond: Dict) -> torch.Tensor:
        from . import ops
        check_supported(cond=cond)
        x = input.float().contiguous()
        n = x.shape[2]
        if cond["control_hint"].shape[2] != n:
            raise ValueError(f"control_hint of {cond['control_hint'].shape[2]} frames for a latent of {n}")
        ctx = cond.get("crossattn")
        per_frame = torch.is_tensor(ctx) and ctx.dim() == 3 and n > 1 and ctx.shape[0] == x.shape[0] * n
        starts, starts_dev, coef_dev = self.tables(n, x.device, per_frame) if per_frame else self.tables(n, x.device)
        hints = self._window_hints(cond["control_hint"], starts)
        ctxs = self._window_contexts(ctx, x.shape[0], n, starts) if per_frame else None
        xw = ops.window_gather(x, starts_dev, self.window)
        twins = ops.get_mark(input, "_cfg_twin_halves") is True
        ys = []
        for i in range(len(starts)):
            xi = xw[i]
            if twins:
                ops.set_mark(xi, "_cfg_twin_halves", True)
            ci = dict(cond)
            ci["control_hint"] = hints[i]
            if ctxs is not None:
                ci["crossattn"] = ctxs[i]
            ys.append(self.denoiser(xi, sigma, ci).float().contiguous())
        return ops.window_fuse(ys, starts_dev, coef_dev, n)


class GroupedFirstStage:
    """The engine with encode_first_stage / decode_first_stage over at most `group` frames per call: first-stage work is per frame, so
    the result has the same bits as one call over all N frames while the kernels run at the shapes of a plain clip.  The posterior noise
    of an encode is drawn once for the whole clip, as the single call draws it, and handed on in slices.  Everything else is the engine's."""

    def __init__(self, model, group: int):
        self._model = model
        self._group = max(int(group), 1)

    def __getattr__(self, name):
        return getattr(self._model, name)

    def encode_first_stage(self, x: torch.Tensor, noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        if x.dim() != 5 or x.shape[2] <= self._group:
            return self._model.encode_first_stage(x, noise=noise)
        b, _, n, h, w = x.shape
        if noise is None:
            zc = self._model.first_stage_model.embed_dim
            noise = torch.randn(b * n, zc, h // 8, w // 8)           # CPU global generator: the single call's draw
        noise = noise.reshape(b, n, *noise.shape[1:])
        out = []
        for f0 in range(0, n, self._group):
            f1 = min(f0 + self._group, n)
            ng = noise[:, f0:f1].reshape(b * (f1 - f0), *noise.shape[2:])
            out.append(self._model.encode_first_stage(x[:, :, f0:f1].contiguous(), noise=ng))
        return torch.cat(out, dim=2)

    def decode_first_stage(self, z: torch.Tensor) -> torch.Tensor:
        if z.dim() != 5 or z.shape[2] <= self._group:
            return self._model.decode_first_stage(z)
        n = z.shape[2]
        return torch.cat([self._model.decode_first_stage(z[:, :, f0:min(f0 + self._group, n)].contiguous())
                          for f0 in range(0, n, self._group)], dim=2)

