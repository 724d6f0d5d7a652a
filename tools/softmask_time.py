#!/usr/bin/env python3
"""The graded-mask kernels (csrc/softmask.hip, the level launcher of csrc/mask.hip) of ONE production clip, 17 x 512 x 768, same
process for both arms of each comparison:
  feather       ccedit_mask_feather of the clip's pixel masks at R = 8 and R = 64 (both passes, the uint16 workspace allocated outside)
  latent        ccedit_mask_latent_graded against ccedit_mask_latent
  re-injection  one ccedit_inpaint_blend_level on the latent (1, 4, 17, 64, 96) against one ccedit_inpaint_blend: the same kernel, the
                strengths of a feathered mask against its binary latent mask
  composite     ccedit_mask_composite_graded with the feathered strengths against ccedit_mask_composite with the binary mask
HIP-event time around the launches, median of 20 after three warm-up calls; the noise tensor is given, not drawn.  The feathered map is
compared with a float64 box mean on the CPU (torch, summed-area table) as a check, not as a timing arm.  Prints one JSON line.
   python tools/softmask_time.py [--frames 17]"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def event_us(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(ts)


def cpu_feather(m: torch.Tensor, r: int) -> torch.Tensor:
    """(2 S + A) // (2 A) over the clipped (2r + 1)^2 window of uint8 maps (N, H, W), by a summed-area table in int64."""
    n, h, w = m.shape
    ii = torch.zeros(n, h + 1, w + 1, dtype=torch.int64)
    ii[:, 1:, 1:] = m.long().cumsum(1).cumsum(2)
    y, x = torch.arange(h), torch.arange(w)
    y0, y1 = (y - r).clamp(min=0), (y + r).clamp(max=h - 1) + 1
    x0, x1 = (x - r).clamp(min=0), (x + r).clamp(max=w - 1) + 1
    s = ii[:, y1][:, :, x1] - ii[:, y0][:, :, x1] - ii[:, y1][:, :, x0] + ii[:, y0][:, :, x0]
    a = ((y1 - y0)[:, None] * (x1 - x0)[None, :])[None]
    return ((2 * s + a) // (2 * a)).to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=17)
    args = ap.parse_args()
    from ccedit_amd import hip, ops, softmask
    torch.set_num_threads(min(16, torch.get_num_threads()))
    torch.set_grad_enabled(False)
    hip.lib()
    if not torch.cuda.is_available():
        raise SystemExit("tools/softmask_time.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    T, H, W = args.frames, 512, 768
    h, w = H // 8, W // 8
    g = torch.Generator().manual_seed(0)
    x, x0, noise = (torch.randn(1, 4, T, h, w, generator=g).to(dev) for _ in range(3))
    mpx_cpu = ((torch.rand(1, T, H // 32, W // 32, generator=g) > 0.5).to(torch.uint8) * 255).repeat_interleave(32, 2).repeat_interleave(32, 3)
    mpx = mpx_cpu.to(dev).contiguous()
    res = {"latent": list(x.shape), "pixels": [T, H, W]}
    tmp = torch.empty(mpx.shape, dtype=torch.int16, device=dev)
    out = torch.empty_like(mpx)
    lib = hip.lib()
    for r in (8, 64):
        def feather():
            hip.check(lib.ccedit_mask_feather(mpx.data_ptr(), tmp.data_ptr(), out.data_ptr(), T, H, W, r, ops._stream()),
                      "ccedit_mask_feather")
        res[f"feather_r{r}_us"] = round(event_us(feather), 2)
        res[f"feather_r{r}_equal"] = bool(torch.equal(ops.mask_feather(mpx, r).cpu()[0], cpu_feather(mpx_cpu[0], r)))
    res["feather_mbytes"] = round(mpx.numel() * 6 / 1e6, 1)          # read 1, write 2, read 2, write 1 bytes per pixel (the windows hit the caches)
    soft = ops.mask_feather(mpx, 8)
    res["latent_graded_us"] = round(event_us(lambda: ops.mask_latent_graded(soft)), 2)
    res["latent_binary_us"] = round(event_us(lambda: ops.mask_latent(mpx)), 2)
    L, mlat = ops.mask_latent_graded(soft), ops.mask_latent(mpx)
    sigma = torch.tensor(3.0)
    s = torch.sqrt(1.0 + sigma ** 2)
    thr = softmask.threshold(15, 30)                                    # the middle of a 30-step walk: 128
    res["reinject_thr"] = thr
    res["reinject_level_us"] = round(event_us(lambda: ops.inpaint_blend_level(x, x0, noise, L, thr, float(sigma), float(s))), 2)
    res["reinject_binary_us"] = round(event_us(lambda: ops.inpaint_blend(x, x0, noise, mlat, float(sigma), float(s))), 2)
    res["reinject_equal_on_binary"] = bool(torch.equal(ops.inpaint_blend_level(x, x0, noise, mlat * 255, thr, float(sigma), float(s)),
                                                       ops.inpaint_blend(x, x0, noise, mlat, float(sigma), float(s))))
    frames_d, orig_d = ((torch.rand(1, 3, T, H, W, generator=g) * 2 - 1).to(dev) for _ in range(2))
    res["composite_graded_us"] = round(event_us(lambda: ops.mask_composite_graded(frames_d, orig_d, soft)), 2)
    res["composite_binary_us"] = round(event_us(lambda: ops.mask_composite(frames_d, orig_d, mpx)), 2)
    res["composite_equal_on_binary"] = bool(torch.equal(ops.mask_composite_graded(frames_d, orig_d, mpx), ops.mask_composite(frames_d, orig_d, mpx)))
    res["composite_mbytes"] = round((frames_d.numel() * 4 * 2 + mpx.numel()) / 1e6, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
