#!/usr/bin/env python3
"""The mask kernels (csrc/mask.hip) of ONE production clip, same process for both arms of each comparison:
  re-injection  one known-region re-injection of a sampler step on the latent (1, 4, 17, 64, 96): the three-launch path
                (ccedit_axpby, expand_as(...).contiguous() of the fp32 mask, ccedit_mask_blend) against ccedit_inpaint_blend
  mask side     ccedit_mask_latent and ccedit_mask_composite at 17 x 512 x 768 against the torch expressions on the CPU
                (F.interpolate(mode="area") + round + clamp; torch.where), at most 16 CPU threads
HIP-event time around the launches (the CPU arms: wall clock), median of 20 after three warm-up calls; the noise tensor is given, not
drawn, on both arms.  Prints one JSON line.   python tools/mask_time.py [--frames 17]"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

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


def wall_us(fn, reps=5):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=17)
    args = ap.parse_args()
    from ccedit_amd import hip, ops
    torch.set_num_threads(min(16, torch.get_num_threads()))
    torch.set_grad_enabled(False)
    hip.lib()
    if not torch.cuda.is_available():
        raise SystemExit("tools/mask_time.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    T, H, W = args.frames, 512, 768
    h, w = H // 8, W // 8
    g = torch.Generator().manual_seed(0)
    x, x0, noise = (torch.randn(1, 4, T, h, w, generator=g).to(dev) for _ in range(3))
    mpx_cpu = ((torch.rand(1, T, H // 32, W // 32, generator=g) > 0.5).to(torch.uint8) * 255).repeat_interleave(32, 2).repeat_interleave(32, 3)
    mpx = mpx_cpu.to(dev)
    mlat = ops.mask_latent(mpx)
    mf = mlat[:, None].float()                                   # (1, 1, T, h, w): what the three-launch path is handed
    sigma = torch.tensor(3.0)
    s = torch.sqrt(1.0 + sigma ** 2)
    inv = 1.0 / float(s)

    def unfused():
        return ops.mask_blend(x, ops.axpby(x0, noise, inv, float(sigma) * inv), mf.expand_as(x).contiguous())

    def fused():
        return ops.inpaint_blend(x, x0, noise, mlat, float(sigma), float(s))

    n = x.numel()
    res = {"latent": list(x.shape), "pixels": [T, H, W], "cpu_threads": torch.get_num_threads(),
           "reinject_three_launch_us": round(event_us(unfused), 2), "reinject_fused_us": round(event_us(fused), 2),
           "reinject_three_launch_mbytes": round(9 * n * 4 / 1e6, 2), "reinject_fused_mbytes": round((4 * n * 4 + mlat.numel()) / 1e6, 2),
           "reinject_max_abs_diff": float((unfused() - fused()).abs().max())}

    frames, orig = (torch.rand(1, 3, T, H, W, generator=g) * 2 - 1 for _ in range(2))
    frames_d, orig_d = frames.to(dev), orig.to(dev)

    def cpu_latent():
        m = (mpx_cpu >= 128).float()[:, None]
        return torch.clamp(torch.round(torch.nn.functional.interpolate(m, size=(T, h, w), mode="area")), 0, 1)

    def cpu_composite():
        return torch.where((mpx_cpu >= 128)[:, None], frames, orig)

    res["mask_latent_us"] = round(event_us(lambda: ops.mask_latent(mpx)), 2)
    res["mask_latent_cpu_us"] = round(wall_us(cpu_latent), 1)
    res["mask_latent_equal"] = bool(torch.equal(mlat.cpu(), cpu_latent()[:, 0].to(torch.uint8)))
    res["mask_composite_us"] = round(event_us(lambda: ops.mask_composite(frames_d, orig_d, mpx)), 2)
    res["mask_composite_cpu_us"] = round(wall_us(cpu_composite), 1)
    res["mask_composite_equal"] = bool(torch.equal(ops.mask_composite(frames_d, orig_d, mpx).cpu(), cpu_composite()))
    res["mask_composite_mbytes"] = round((frames.numel() * 4 * 2 + mpx.numel()) / 1e6, 1)      # half the mask set: result or original read, out written
    print(json.dumps(res))


if __name__ == "__main__":
    main()
