#!/usr/bin/env python3
"""What motion-following noise costs (ccedit_amd/noisewarp.py, csrc/noisewarp.hip): one production clip — 113 source frames of
512 x 768, 17 keyframes at gap 7, 224 pairs — stage by stage under HIP events (median of `--reps` after warm-up): the pyramid, the
matching of all pairs, the track launch, the claim and resolve launches of all keyframes, and noisewarp.build as a whole (which also
brings the inherited counts back to the host); then what a run pays on EVERY draw: one gather of the clip's latent noise
(1, 4, 17, 64, 96) through the map, beside torch.randn_like of the same shape, and the wrap at rho = 1 and rho = 0.5.
Per stage: time, bytes moved (compulsory: every input read and every output written once) and the achieved GB/s.  Prints one JSON line.
  python tools/noisewarp_time.py [--keyframes 17] [--gap 7] [--H 512] [--W 768] [--reps 5]
A kernel trace of the same run:  rocprofv3 --kernel-trace --stats -- python tools/noisewarp_time.py --reps 2"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.propagate_time import event_ms, moving_clip  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=17)
    ap.add_argument("--gap", type=int, default=7)
    ap.add_argument("--H", type=int, default=512)
    ap.add_argument("--W", type=int, default=768)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from ccedit_amd import hip, ops
    from ccedit_amd import masktrack as M
    from ccedit_amd import noisewarp as N
    from ccedit_amd import propagate as P
    hip.lib()
    if not torch.cuda.is_available():
        raise SystemExit("tools/noisewarp_time.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    h, w, k = args.H, args.W, args.keyframes
    keys = [i * args.gap for i in range(k)]
    nfr = keys[-1] + 1
    cells = (h // 8) * (w // 8)
    src = moving_clip(nfr, h, w).to(dev)
    rows = M.pair_rows(nfr, 0)
    npairs, px = rows.shape[0], h * w
    pairs = torch.from_numpy(rows).to(dev)
    res = dict(frames=nfr, keyframes=k, gap=args.gap, size=[h, w], pairs=npairs, cells=cells, reps=args.reps)

    def stage(name, fn, nbytes, extra=None):
        ms = event_ms(fn, args.reps)
        res[name] = dict(ms=round(ms, 4), mbytes=round(nbytes / 1e6, 2), gb_per_s=round(nbytes / ms / 1e6, 1), **(extra(ms) if extra else {}))

    stage("pyramid", lambda: ops.prop_pyramid(src), nfr * px * (3 + 85 / 64))
    pyr = ops.prop_pyramid(src)
    match_bytes = sum(npairs * ((h >> lv) // 8) * ((w >> lv) // 8) * (256 + (16 + 2 * P.radius_of(lv)) ** 2 + 8 + (8 if lv < P.LEVELS - 1 else 0))
                      for lv in range(P.LEVELS))       # (as tools/propagate_time.py counts them)
    stage("match", lambda: P.match_pairs(pyr, pairs, nfr, h, w), match_bytes, lambda ms: dict(launches=P.LEVELS))
    vec = P.match_pairs(pyr, pairs, nfr, h, w)
    # track: per (k >= 1, cell) two vectors of 8 bytes per frame of the gap, 12 bytes written
    stage("track", lambda: ops.noisewarp_track(vec, keys, h, w, N.FB_LIMIT), (k - 1) * cells * (args.gap * 16 + 12), lambda ms: dict(launches=1))
    track = ops.noisewarp_track(vec, keys, h, w, N.FB_LIMIT)
    # origins: per keyframe the track and the previous origins read by claim and by resolve, one table word each way, origins and map written
    stage("origins", lambda: ops.noisewarp_origins(track, h, w), k * cells * (2 * 24 + 8 + 16),
          lambda ms: dict(launches=2 * k - 1, us_per_keyframe=round(ms * 1e3 / k, 2)))
    res["build_ms"] = round(event_ms(lambda: N.build(src, keys), args.reps), 3)
    res["stages_sum_ms"] = round(sum(res[s]["ms"] for s in ("pyramid", "match", "track", "origins")), 3)
    smap, shares = N.build(src, keys)
    res["inherited"] = [round(s, 4) for s in shares]
    res["unique_per_keyframe"] = bool(all(int(torch.unique(row).numel()) == cells for row in smap))

    x = torch.empty(1, 4, k, h // 8, w // 8, device=dev)
    maps = smap[None].contiguous()
    raw = torch.randn_like(x)
    out = torch.empty_like(x)
    stage("gather", lambda: ops.noise_warp(raw, maps, out=out, checked=True), x.numel() * 8 + maps.numel() * 4,
          lambda ms: dict(us=round(ms * 1e3, 2), shape=list(x.shape)))
    res["randn_like_us"] = round(event_ms(lambda: torch.randn_like(x), args.reps) * 1e3, 2)
    for rho in (1.0, 0.5):
        draw = N.wrap(torch.randn_like, maps, rho)
        res[f"draw_rho_{rho}_us"] = round(event_ms(lambda: draw(x), args.reps) * 1e3, 2)
    res["peak_memory_mb"] = round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
