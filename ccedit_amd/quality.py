"""Quality report: how faithful a result is to its source, and how steady it is along the source's motion (`--report_quality`,
tools/quality.py).

Two measurements that need no trained scorer.  FIDELITY: squared error per channel (-> PSNR) and SSIM on luma over 8 x 8 windows at
stride 4 between two clips, restricted to the pixels a mask keeps.  TEMPORAL CONSISTENCY (warp error): the SOURCE's motion from frame i
to frame i - 1 — the matcher of --propagate, the per-pixel selection and the forward-backward test of --mask_track, all unchanged — is
followed, and the squared change of the measured clip along it is averaged over the pixels frame i - 1 shows; the source's own value
stands beside it as the floor the motion estimate allows.  These are measures of fidelity and steadiness; they say nothing about how
well a prompt was followed.

The sums are integer arithmetic with 64-bit accumulators in ccedit_amd/csrc/quality.hip, equal bit for bit to the numpy restatement
the tests carry; there is no host fallback.  This module holds what the host decides: the constants, the pair list, the loop over a
clip, and the floating point — PSNR, SSIM, means and ratios are formed here, in Python, from the exact integers.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

from .masktrack import FB_LIMIT, check_size, pair_rows  # noqa: F401  (FB_LIMIT is this module's default limit: one place, masktrack's)

# ---- the constants of the measurement: this is their one place on the host (csrc/quality.hip restates the window and C1, C2)
WINDOW = 8                  # SSIM windows are WINDOW x WINDOW luma pixels ...
STRIDE = 4                  # ... at this stride; a window counts iff all of its pixels are kept
C1 = 26634                  # (0.01 * 255)^2 * WINDOW^4, rounded
C2 = 239708                 # (0.03 * 255)^2 * WINDOW^4, rounded
Q_ONE = 1 << 32             # the quotient q of a window is floor(|Nw| * Q_ONE / Dw) with Nw's sign: identical windows give Q_ONE
KEEP_BELOW = 128            # a pixel is kept where its mask byte is below this (the edit masks' threshold)
PAIR_CHUNK = 32             # pair rows per select launch: bounds the workspace (4 H W bytes per row); results do not depend on it
SEL_ALL, SEL_EDITED, SEL_KEPT = 0, 1, 2


def _ratio(a: int, b: int) -> Optional[float]:
    return None if b == 0 else a / b


def _psnr(sse: int, samples: int) -> Optional[float]:
    """10 log10(255^2 samples / SSE); None where nothing differs (or nothing was counted)."""
    return None if sse == 0 or samples == 0 else 10.0 * math.log10(65025 * samples / sse)


def _flicker(means: Sequence[Optional[float]]) -> Optional[float]:
    if len(means) < 2 or any(m is None for m in means):
        return None
    return sum(abs(b - a) for a, b in zip(means, means[1:])) / (len(means) - 1)


def derive_compare(rows: Sequence[Sequence[int]]) -> dict:
    """rows: per frame the eight integers of ops.quality_pair (slot 4 signed) -> the integers and what follows from them."""
    rows = [[int(v) for v in r] for r in rows]
    sse = [sum(r[c] for r in rows) for c in range(3)]
    count, qsum, windows = (sum(r[i] for r in rows) for i in (3, 4, 5))
    mean_a = [_ratio(r[6], r[3]) for r in rows]
    mean_b = [_ratio(r[7], r[3]) for r in rows]
    total = sum(sse)
    return {
        "frames": [dict(sse=r[:3], count=r[3], q_sum=r[4], windows=r[5], luma_a=r[6], luma_b=r[7]) for r in rows],
        "sse": sse, "count": count, "q_sum": qsum, "windows": windows,
        "identical": count > 0 and total == 0,
        "psnr": _psnr(total, 3 * count),
        "psnr_rgb": [_psnr(s, count) for s in sse],
        "ssim": None if windows == 0 else qsum / (windows * Q_ONE),
        "mean_luma_a": mean_a, "mean_luma_b": mean_b,
        "flicker": {"a": _flicker(mean_a), "b": _flicker(mean_b)},
    }


def derive_temporal(pairs: Sequence[Sequence[int]], rows: Sequence[Sequence[int]], with_y: bool) -> dict:
    """pairs: (f, g) per measurement; rows: the four integers of ops.quality_warp per measurement."""
    rows = [[int(v) for v in r] for r in rows]
    sx, sy, valid, selected = (sum(r[i] for r in rows) for i in range(4))
    return {
        "pairs": [[int(f), int(g)] for f, g in pairs],
        "sse_x": [r[0] for r in rows], "sse_y": [r[1] for r in rows] if with_y else None,
        "valid": [r[2] for r in rows], "selected": [r[3] for r in rows],
        "warp_mse": _ratio(sx, 3 * valid),
        "warp_mse_y": _ratio(sy, 3 * valid) if with_y else None,
        "valid_share": _ratio(valid, selected),
    }


def _side(t: dict) -> dict:
    """One selection of report(): the result's warp error beside the source's own."""
    r, s = t["warp_mse"], t["warp_mse_y"]
    return {"result": r, "source": s, "ratio": None if r is None or not s else r / s, "valid_share": t["valid_share"],
            "pairs": t["pairs"], "sse_result": t["sse_x"], "sse_source": t["sse_y"], "valid": t["valid"], "selected": t["selected"]}


def assemble(size, frames: int, fidelity: dict, temporal: Optional[dict], reason: Optional[str], masked: bool) -> dict:
    """The report's layout: report() fills it from the kernels' integers (and the tests from the restatement's)."""
    out = {"size": [int(size[0]), int(size[1])], "frames": int(frames), "masked": bool(masked),
           "fidelity": {k: v for k, v in fidelity.items() if k != "flicker"},
           "flicker": {"source": fidelity["flicker"]["a"], "result": fidelity["flicker"]["b"]},
           "temporal": None if temporal is None else {k: _side(t) for k, t in temporal.items()}}
    if temporal is None:
        out["reason"] = reason
    return out


def summary(rep: dict) -> dict:
    """What log_info.json keeps of a report: PSNR, SSIM, the warp error of result and source, the valid share."""
    t = (rep["temporal"] or {}).get("all") or {}
    return {"psnr": rep["fidelity"]["psnr"], "identical": rep["fidelity"]["identical"], "ssim": rep["fidelity"]["ssim"],
            "warp_mse_result": t.get("result"), "warp_mse_source": t.get("source"), "valid_share": t.get("valid_share")}


# ---- the device side
def _frames(t, name: str):
    import torch
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or not t.is_cuda or t.dim() != 4 or t.shape[3] != 3:
        raise ValueError(f"{name} must be a cuda uint8 tensor of RGB frames (F, H, W, 3), got "
                         f"{getattr(t, 'dtype', type(t))} {getattr(t, 'device', '')} {tuple(getattr(t, 'shape', ()))}")
    return t.contiguous()


def _mask(mask, like, name: str):
    """None, or a cuda mask (F, H, W) for the frames `like`: uint8 (>= 128 = edited) as it is, bool as 0 / 255."""
    import torch
    if mask is None:
        return None
    if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.uint8, torch.bool) or not mask.is_cuda:
        raise ValueError(f"{name}: the mask must be a cuda uint8 or bool tensor, got {getattr(mask, 'dtype', type(mask))} {getattr(mask, 'device', '')}")
    if tuple(mask.shape) != tuple(like.shape[:3]):
        raise ValueError(f"{name}: mask {tuple(mask.shape)} for frames {tuple(like.shape)}: one byte per pixel, (F, H, W)")
    if mask.dtype == torch.bool:
        mask = mask.to(torch.uint8) * 255
    return mask.contiguous()


def compare(a_u8, b_u8, mask=None) -> dict:
    """Fidelity of b to a: uint8 clips (F, H, W, 3) on the device, H and W multiples of 4 and at least 8; mask: None, or (F, H, W)
    (uint8 >= 128 or True = edited: left out) -> derive_compare of the kernel's integers."""
    from . import ops
    a, b = _frames(a_u8, "compare: a_u8"), _frames(b_u8, "compare: b_u8")
    acc = ops.quality_pair(a, b, _mask(mask, a, "compare"))
    return derive_compare(acc.cpu().tolist())            # (int64: slot 4 is the signed sum as it is, the others stay below 2^63)


def check_temporal(frames: int, h: int, w: int, who: str = "quality.temporal") -> None:
    """What the warp error needs (ValueError): two frames, and the matcher's size."""
    if frames < 2:
        raise ValueError(f"{who}: {frames} frame(s): the warp error compares neighbouring frames, it needs at least 2")
    check_size(h, w, who)


def _warp_sums(guide, x, y, mask, sels, limit: int, pair_chunk: Optional[int] = None):
    """The vectors of `guide` once, every selection of `sels` measured along them -> ((f, g) per measurement, {sel: rows of four
    integers})."""
    import torch
    from . import ops
    from .propagate import match_pairs
    n, h, w, _ = guide.shape
    chunk = PAIR_CHUNK if pair_chunk is None else int(pair_chunk)
    if chunk < 2 or chunk % 2:
        raise ValueError(f"quality.temporal: pair_chunk={chunk} must be a positive multiple of 2 (a measurement's two rows stay together)")
    rows = pair_rows(n, 0)                                           # (i, i - 1) and (i - 1, i) for i = 1 ... F - 1
    pairs = torch.from_numpy(rows).to(guide.device)
    pyr = ops.prop_pyramid(guide)
    vec = match_pairs(pyr, pairs, n, h, w)
    acc = {s: [] for s in sels}
    for s0 in range(0, rows.shape[0], chunk):
        vsel = ops.masktrack_select(pyr, pairs[s0:s0 + chunk], vec[s0:s0 + chunk], n, h, w)
        for s in sels:
            acc[s].append(ops.quality_warp(x, vsel, pairs[s0:s0 + chunk], limit, y=y, mask=mask if s else None, sel=s))
    return [(int(r[0]), int(r[1])) for r in rows[0::2]], {s: torch.cat(v).cpu().tolist() for s, v in acc.items()}


def temporal(guide_u8, x_u8, y_u8=None, mask=None, sel: int = SEL_ALL, limit: int = FB_LIMIT, pair_chunk: Optional[int] = None) -> dict:
    """Warp error of x (and of y, which shares the vectors) along the motion of `guide`: uint8 clips (F, H, W, 3) on the device, F >= 2,
    H and W multiples of 64; mask (F, H, W) with sel = SEL_EDITED / SEL_KEPT chooses the pixels of each frame i -> derive_temporal."""
    g, x = _frames(guide_u8, "temporal: guide_u8"), _frames(x_u8, "temporal: x_u8")
    y = None if y_u8 is None else _frames(y_u8, "temporal: y_u8")
    for t, name in ((x, "x_u8"), (y, "y_u8")):
        if t is not None and tuple(t.shape) != tuple(g.shape):
            raise ValueError(f"temporal: {name} {tuple(t.shape)} is measured along the guide's vectors: the guide's shape {tuple(g.shape)}")
    check_temporal(g.shape[0], g.shape[1], g.shape[2])
    if int(sel) not in (SEL_ALL, SEL_EDITED, SEL_KEPT):
        raise ValueError(f"temporal: sel={sel} (0: all pixels, 1: edited, 2: kept)")
    if int(sel) != SEL_ALL and mask is None:
        raise ValueError(f"temporal: sel={sel} chooses pixels by the mask: give one")
    fg, sums = _warp_sums(g, x, y, _mask(mask, g, "temporal"), (int(sel),), int(limit), pair_chunk)
    return derive_temporal(fg, sums[int(sel)], y is not None)


def report(source_u8, result_u8, mask=None) -> dict:
    """One dict for a source clip and its result, uint8 (F, H, W, 3) on the device; mask: None or (F, H, W), uint8 >= 128 / True =
    edited.  fidelity: result against source over the kept pixels (all of them without a mask); flicker: of the mean lumas over those
    pixels; temporal.all and, with a mask, temporal.edited: the warp error of the result beside the source's own along the source's
    motion, their ratio and the valid share — or "temporal": None with a `reason` where the clip has one frame or the size is off the
    matcher's grid."""
    src, res = _frames(source_u8, "report: source_u8"), _frames(result_u8, "report: result_u8")
    if tuple(src.shape) != tuple(res.shape):
        raise ValueError(f"report: source {tuple(src.shape)} and result {tuple(res.shape)}: the same frames, the same size")
    m = _mask(mask, src, "report")
    n, h, w, _ = src.shape
    fidelity = compare(src, res, m)
    temp = reason = None
    try:
        check_temporal(n, h, w, "quality report")
    except ValueError as e:
        reason = str(e)
    else:
        sels = (SEL_ALL,) if m is None else (SEL_ALL, SEL_EDITED)
        fg, sums = _warp_sums(src, res, src, m, sels, FB_LIMIT)
        temp = {("all", "edited")[s]: derive_temporal(fg, sums[s], True) for s in sels}
    return assemble((h, w), n, fidelity, temp, reason, m is not None)
