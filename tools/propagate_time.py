#!/usr/bin/env python3
"""What full-frame-rate output costs (ccedit_amd/propagate.py, csrc/propagate.hip): one production clip — 17 keyframes at gap 7 =
113 source frames of 512 x 768, 96 in-between frames, 192 pairs — stage by stage under HIP events (median of `--reps` after warm-up),
each stage over ALL pairs of the clip in launches of PAIR_CHUNK pairs as propagate_clip issues them, and propagate_clip as a whole.
Per stage: time, bytes moved (compulsory: every input read and every output written once) and the achieved GB/s; for the matching
also the SAD operations (one = |a - b| of one pixel pair, summed) per second.  Prints one JSON line.
  python tools/propagate_time.py [--keyframes 17] [--gap 7] [--H 512] [--W 768] [--reps 5]
A kernel trace of the same run:  rocprofv3 --kernel-trace --stats -- python tools/propagate_time.py --reps 2"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def event_ms(fn, reps, warm=2):
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
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def moving_clip(frames, h, w, seed=0):
    """A low-resolution random texture, up-sampled, panning by (1, 2) pixels per frame: something the matching can follow."""
    g = torch.Generator().manual_seed(seed)
    low = torch.rand(1, 3, (h + 2 * frames) // 8 + 2, (w + 4 * frames) // 8 + 2, generator=g)
    big = torch.nn.functional.interpolate(low, scale_factor=8, mode="bicubic", align_corners=False)[0].clamp(0, 1)
    big = (big * 255).to(torch.uint8).permute(1, 2, 0)
    return torch.stack([big[t:t + h, 2 * t:2 * t + w] for t in range(frames)]).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=17)
    ap.add_argument("--gap", type=int, default=7)
    ap.add_argument("--H", type=int, default=512)
    ap.add_argument("--W", type=int, default=768)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from ccedit_amd import hip, ops
    from ccedit_amd import propagate as P
    hip.lib()
    if not torch.cuda.is_available():
        raise SystemExit("tools/propagate_time.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    h, w = args.H, args.W
    keys = list(range(0, args.keyframes * args.gap, args.gap))
    nfr = keys[-1] + 1
    src = moving_clip(nfr, h, w).to(dev)
    edited = (255 - src[keys]).contiguous()
    pl = P.plan(keys, nfr)
    npairs = pl.pairs.shape[0]
    chunks = [torch.from_numpy(np.ascontiguousarray(pl.pairs[s:s + P.PAIR_CHUNK])).to(dev) for s in range(0, npairs, P.PAIR_CHUNK)]
    ranks, g = P.device_tables(dev)
    px = h * w
    res = dict(frames=nfr, keyframes=len(keys), gap=args.gap, size=[h, w], pairs=npairs, pair_chunk=P.PAIR_CHUNK, reps=args.reps)

    def stage(name, fn, nbytes, extra=None):
        ms = event_ms(fn, args.reps)
        res[name] = dict(ms=round(ms, 3), mbytes=round(nbytes / 1e6, 1), gb_per_s=round(nbytes / ms / 1e6, 1), **(extra(ms) if extra else {}))

    stage("pyramid", lambda: ops.prop_pyramid(src), nfr * px * (3 + 85 / 64))
    pyr = ops.prop_pyramid(src)
    luma0 = ops.prop_level(pyr, nfr, h, w, 0)
    # matching, level by level: both patches of every block read once (256 + (16 + 2R)^2 bytes), one vector pair written
    sad_ops, match_bytes = 0, 0
    for lv in range(P.LEVELS):
        r = P.radius_of(lv)
        blocks = npairs * ((h >> lv) // 8) * ((w >> lv) // 8)
        sad_ops += blocks * (2 * r + 1) ** 2 * 256
        match_bytes += blocks * (256 + (16 + 2 * r) ** 2 + 8 + (8 if lv < P.LEVELS - 1 else 0))
    stage("match", lambda: [P.match_pairs(pyr, c, nfr, h, w) for c in chunks], match_bytes,
          lambda ms: dict(sad_ops=sad_ops, gsad_per_s=round(sad_ops / ms / 1e6, 1), launches=P.LEVELS * len(chunks)))
    vecs = [P.match_pairs(pyr, c, nfr, h, w) for c in chunks]
    stage("warp_rgb", lambda: [ops.prop_warp(edited, v, c, 2) for v, c in zip(vecs, chunks)], npairs * px * 6)
    stage("warp_luma", lambda: [ops.prop_warp(luma0, v, c, 1) for v, c in zip(vecs, chunks)], npairs * px * 2)
    w_rgb = [ops.prop_warp(edited, v, c, 2) for v, c in zip(vecs, chunks)]
    w_luma = [ops.prop_warp(luma0, v, c, 1) for v, c in zip(vecs, chunks)]
    stage("blend", lambda: [ops.prop_blend(a, b, pyr, c, g, nfr) for a, b, c in zip(w_rgb, w_luma, chunks)], npairs * px * 4 + (npairs // 2) * px * 4)
    del w_rgb, w_luma, vecs
    total = event_ms(lambda: P.propagate_clip(src, keys, edited), args.reps)
    res["propagate_clip_ms"] = round(total, 3)
    res["stages_sum_ms"] = round(sum(res[k]["ms"] for k in ("pyramid", "match", "warp_rgb", "warp_luma", "blend")), 3)
    res["ms_per_output_frame"] = round(total / pl.num_out, 4)
    out = P.propagate_clip(src, keys, edited)
    res["keyframes_kept"] = bool(torch.equal(out[keys], edited))
    res["peak_memory_mb"] = round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
