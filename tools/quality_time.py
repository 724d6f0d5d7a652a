#!/usr/bin/env python3
"""The quality-report kernels (csrc/quality.hip) on ONE clip of 512 x 768, a moving synthetic scene and a result that differs from it:
  pair          ccedit_quality_pair over all frames, without and with a mask
  warp          ccedit_quality_warp over all F - 1 neighbouring pairs (x and y along one set of vectors), the per-pixel vectors made
                beforehand; without a mask and with sel = 1
  matcher       what the report runs before the warp kernel, unchanged: ccedit_prop_pyramid, the four levels of ccedit_prop_match and
                ccedit_masktrack_select for the same pairs
  report        ccedit_amd.quality.report as a whole (fidelity, matcher, warp, the integers brought to the host), without and with a mask
HIP-event time around the launches, median of 20 after three warm-up calls (the report: wall time with a device synchronisation, median
of 5).  Bytes are algorithmic: every operand read once.  Prints one JSON line.
   python tools/quality_time.py [--frames 17]"""
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


def wall_us(fn, reps=5, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(ts)


def moving_clip(frames: int, h: int, w: int, dev) -> torch.Tensor:
    """A smooth texture that moves by (1, -2) pixels per frame: uint8 (frames, h, w, 3)."""
    rs = np.random.RandomState(0)
    big = rs.randint(0, 256, (h // 8 + frames + 4, w // 8 + 2 * frames + 4, 3)).astype(np.uint8).repeat(8, 0).repeat(8, 1)
    big = (big.astype(np.int32) + rs.randint(-8, 9, big.shape)).clip(0, 255).astype(np.uint8)
    return torch.from_numpy(np.stack([big[t:t + h, 2 * (frames - t):2 * (frames - t) + w] for t in range(frames)])).to(dev).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=17)
    args = ap.parse_args()
    from ccedit_amd import hip, masktrack, ops, quality
    from ccedit_amd.propagate import match_pairs
    torch.set_num_threads(min(16, torch.get_num_threads()))
    torch.set_grad_enabled(False)
    hip.lib()
    if not torch.cuda.is_available():
        raise SystemExit("tools/quality_time.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    F, H, W = args.frames, 512, 768
    src = moving_clip(F, H, W, dev)
    res_clip = (255 - src).contiguous()
    mask = torch.zeros((F, H, W), dtype=torch.uint8, device=dev)
    mask[:, H // 4:3 * H // 4, W // 4:3 * W // 4] = 255
    out = {"frames": F, "size": [H, W]}

    def put(name, us, nbytes):
        out[name] = dict(us=round(us, 2), mbytes=round(nbytes / 1e6, 1), tb_per_s=round(nbytes / us / 1e6, 3))

    px = F * H * W
    put("pair", event_us(lambda: ops.quality_pair(src, res_clip)), 6 * px)
    put("pair_masked", event_us(lambda: ops.quality_pair(src, res_clip, mask)), 7 * px)

    rows = masktrack.pair_rows(F, 0)
    pairs = torch.from_numpy(rows).to(dev)
    chunk = quality.PAIR_CHUNK
    state = {}

    def matcher():
        pyr = ops.prop_pyramid(src)
        vec = match_pairs(pyr, pairs, F, H, W)
        state["vsel"] = [ops.masktrack_select(pyr, pairs[s:s + chunk], vec[s:s + chunk], F, H, W) for s in range(0, rows.shape[0], chunk)]

    out["matcher_us"] = round(event_us(matcher, reps=5, warm=2), 2)

    def warp(m, sel):
        for i, v in enumerate(state["vsel"]):
            ops.quality_warp(res_clip, v, pairs[i * chunk:(i + 1) * chunk], quality.FB_LIMIT, y=src, mask=m, sel=sel)

    ppx = (F - 1) * H * W                                                       # per measured pixel: v and r (8 bytes), x and y at p and at q (12)
    put("warp", event_us(lambda: warp(None, 0)), 20 * ppx)
    share = float((mask >= 128).float().mean())                                 # every pixel: v, mask, x and y at p (11); a selected one: r, x and y at q (10)
    put("warp_edited", event_us(lambda: warp(mask, 1)), (11 + 10 * share) * ppx)
    out["report_us"] = round(wall_us(lambda: quality.report(src, res_clip)), 1)
    out["report_masked_us"] = round(wall_us(lambda: quality.report(src, res_clip, mask)), 1)
    rep = quality.report(src, res_clip, mask)
    out["check"] = dict(valid_share=rep["temporal"]["all"]["valid_share"], ratio=rep["temporal"]["all"]["ratio"], ssim=rep["fidelity"]["ssim"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
