#!/usr/bin/env python3
"""Host route against the --gpu_io route for the pixel side of ONE production clip, same machine, same run:
  in   decoded uint8 frames (17 keyframes 1080 x 1920) + raw depth over 120 frames (384 x 512) -> `keyframes` (1, 3, 17, 512, 768) on the
       device + the ZoeDepth / MiDaS control hint (1, 3, 17, 512, 768) on the device
  out  decoder output (1, 3, 17, 512, 768) fp32 on the device -> uint8 frames (17, 512, 768, 3) on the host
Wall clock around a device synchronise, median of 5 after one warm-up; the host route runs on at most 16 CPU threads (what a job has).
Per kernel: algorithmic bytes over HIP-event time.  Prints one JSON line.   python tools/pixel_io_time.py [--frames 17]"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def wall(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def kernel_ms(fn, reps=5):
    fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=17)
    ap.add_argument("--depth_frames", type=int, default=120)
    args = ap.parse_args()
    from PIL import Image
    from ccedit_amd import hip, ops
    from scripts.sampling.util import keyframe_indices
    from sgm.modules.encoders.modules import DepthMidasEncoder, DepthZoeEncoder
    torch.set_num_threads(min(16, torch.get_num_threads()))
    torch.set_grad_enabled(False)
    hip.lib()
    dev = torch.device("cuda:0")
    T, Hs, Ws, H, W, hd, wd = args.frames, 1080, 1920, 512, 768, 384, 512
    rs = np.random.RandomState(0)
    small = rs.randint(0, 256, (T, Hs // 8, Ws // 8, 3)).astype(np.uint8)
    frames = np.ascontiguousarray(np.repeat(np.repeat(small, 8, axis=1), 8, axis=2))                       # decoded frames, uint8
    depth_all = torch.rand(args.depth_frames, hd, wd, generator=torch.Generator().manual_seed(0)) * 9 + 1
    idx = keyframe_indices(args.depth_frames, 20, 3, T)
    decoded = (torch.rand(1, 3, T, H, W, generator=torch.Generator().manual_seed(1)) * 2.2 - 1.1).to(dev)

    def host_in(enc):
        kf = torch.cat([(torch.from_numpy(np.array(Image.fromarray(f).resize((W, H), Image.BICUBIC))).permute(2, 0, 1).unsqueeze(0).float()
                         / 255.0 * 2.0 - 1.0).clamp(-1.0, 1.0) for f in frames], dim=0)
        kf = kf.permute(1, 0, 2, 3)[None].to(dev)
        d = torch.nn.functional.interpolate(depth_all[idx][:, None], size=(H, W), mode="bicubic", align_corners=False)[:, 0][None, None]
        return kf, enc.normalize(d.to(dev))                     # (the conditioner normalises on the tensor's device: torch kernels)

    def gpu_in(enc):
        kf = ops.resize_u8_pil(torch.from_numpy(frames).to(dev), (H, W), to_float=True)[None]
        d = ops.resize_bicubic(depth_all[idx][:, None].contiguous().to(dev), (H, W))[:, 0][None, None]
        return kf, enc.normalize_gpu(d)

    def host_out():
        x = torch.clamp((decoded + 1.0) / 2.0, 0.0, 1.0)
        return (255.0 * x[0].float().cpu().permute(1, 2, 3, 0).numpy()).astype(np.uint8)

    def gpu_out():
        return ops.frames_to_u8(decoded)[0].cpu().numpy()

    res = {"frames": T, "source": [Hs, Ws], "size": [H, W], "depth": [args.depth_frames, hd, wd], "cpu_threads": torch.get_num_threads()}
    for name, enc in (("zoe", DepthZoeEncoder), ("midas", DepthMidasEncoder)):
        res[f"in_{name}_host_ms"] = round(wall(lambda: host_in(enc)), 2)
        res[f"in_{name}_gpu_io_ms"] = round(wall(lambda: gpu_in(enc)), 2)
    res["out_host_ms"] = round(wall(host_out), 2)
    res["out_gpu_io_ms"] = round(wall(gpu_out), 2)
    assert np.array_equal(host_out(), gpu_out())
    a, b = host_in(DepthZoeEncoder), gpu_in(DepthZoeEncoder)
    res["keyframes_equal"] = bool(torch.equal(a[0], b[0]))
    res["hint_max_abs_diff"] = float((a[1] - b[1]).abs().max())

    # per kernel: device-resident operands, bytes that have to move / HIP-event time
    fd = torch.from_numpy(frames).to(dev)
    dd = depth_all[idx][:, None].contiguous().to(dev)
    dr = ops.resize_bicubic(dd, (H, W))[:, 0][None, None].contiguous()
    n = T * H * W
    stats = ops.kth_values(dr.view(1, -1), [int(0.02 * n), int(0.85 * n)])
    kern = {
        "resize_u8_pil->f32": (lambda: ops.resize_u8_pil(fd, (H, W), to_float=True), T * (Hs * Ws * 3 + 2 * Hs * W * 3 + H * W * 12)),
        "resize_u8_pil->u8": (lambda: ops.resize_u8_pil(fd, (H, W)), T * (Hs * Ws * 3 + 2 * Hs * W * 3 + H * W * 3)),
        "resize_f32_bicubic": (lambda: ops.resize_bicubic(dd, (H, W)), T * (hd * wd + H * W) * 4),
        "kth_values(2 ranks)": (lambda: ops.kth_values(dr.view(1, -1), [int(0.02 * n), int(0.85 * n)]), 4 * n * 4),
        "minmax": (lambda: ops.minmax(dr.view(1, -1)), n * 4),
        "depth_hint": (lambda: ops.depth_hint(dr, stats, False), n * 16),
        "frames_to_u8": (lambda: ops.frames_to_u8(decoded), n * 15),
    }
    res["kernels"] = {}
    for k, (fn, nbytes) in kern.items():
        ms = kernel_ms(fn)
        res["kernels"][k] = {"ms": round(ms, 4), "mbytes": round(nbytes / 1e6, 1), "gbytes_per_s": round(nbytes / ms / 1e6, 1)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
