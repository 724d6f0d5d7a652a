#!/usr/bin/env python3
"""What mask tracking costs (ccedit_amd/masktrack.py, csrc/masktrack.hip): one production clip — 113 source frames of 512 x 768, the
mask painted on the middle frame, 224 pairs — stage by stage under HIP events (median of `--reps` after warm-up), each stage over ALL
pairs of the clip as track_clip issues them (select in launches of PAIR_CHUNK pairs), and track_clip as a whole; beside it
propagate_clip on the same frames (17 keyframes at gap 7) as a yardstick, and dilate + invert of the clip's masks.
Per stage: time, bytes moved (compulsory: every input read and every output written once) and the achieved GB/s; for select also the
absolute differences (one = |a - b| of one pixel pair) per second.  Prints one JSON line.
  python tools/masktrack_time.py [--frames 113] [--anchor 56] [--H 512] [--W 768] [--reps 5]
A kernel trace of the same run:  rocprofv3 --kernel-trace --stats -- python tools/masktrack_time.py --reps 2"""
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
    ap.add_argument("--frames", type=int, default=113)
    ap.add_argument("--anchor", type=int, default=56)
    ap.add_argument("--H", type=int, default=512)
    ap.add_argument("--W", type=int, default=768)
    ap.add_argument("--dilate", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from ccedit_amd import hip, ops
    from ccedit_amd import masktrack as M
    from ccedit_amd import propagate as P
    hip.lib()
    if not torch.cuda.is_available():
        raise SystemExit("tools/masktrack_time.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    h, w, nfr = args.H, args.W, args.frames
    src = moving_clip(nfr, h, w).to(dev)
    anchor = torch.zeros((h, w), dtype=torch.uint8, device=dev)
    anchor[h // 3:2 * h // 3, w // 3:2 * w // 3] = 255
    rows = M.pair_rows(nfr, args.anchor)
    npairs, px = rows.shape[0], h * w
    pairs = torch.from_numpy(rows).to(dev)
    res = dict(frames=nfr, anchor=args.anchor, size=[h, w], pairs=npairs, pair_chunk=M.PAIR_CHUNK, reps=args.reps)

    def stage(name, fn, nbytes, extra=None):
        ms = event_ms(fn, args.reps)
        res[name] = dict(ms=round(ms, 3), mbytes=round(nbytes / 1e6, 1), gb_per_s=round(nbytes / ms / 1e6, 1), **(extra(ms) if extra else {}))

    stage("pyramid", lambda: ops.prop_pyramid(src), nfr * px * (3 + 85 / 64))
    pyr = ops.prop_pyramid(src)
    match_bytes = sum(npairs * ((h >> lv) // 8) * ((w >> lv) // 8) * (256 + (16 + 2 * P.radius_of(lv)) ** 2 + 8 + (8 if lv < P.LEVELS - 1 else 0))
                      for lv in range(P.LEVELS))       # (as tools/propagate_time.py counts them)
    stage("match", lambda: P.match_pairs(pyr, pairs, nfr, h, w), match_bytes, lambda ms: dict(launches=P.LEVELS))
    vec = P.match_pairs(pyr, pairs, nfr, h, w)
    starts = range(0, npairs, M.PAIR_CHUNK)
    # select: both frames of a pair read once, a block's nine vectors, four bytes per pixel written; 9 candidates x 25 differences per pixel
    diffs = npairs * px * len(M.CANDIDATES) * M.BOX * M.BOX
    stage("select", lambda: [ops.masktrack_select(pyr, pairs[s:s + M.PAIR_CHUNK], vec[s:s + M.PAIR_CHUNK], nfr, h, w) for s in starts],
          npairs * (px * 6 + (px // 64) * 8),
          lambda ms: dict(abs_diffs=diffs, gdiff_per_s=round(diffs / ms / 1e6, 1), launches=len(starts)))
    sel = ops.masktrack_select(pyr, pairs[:2], vec[:2], nfr, h, w)
    masks = torch.empty((nfr, h, w), dtype=torch.uint8, device=dev)
    masks[args.anchor] = anchor

    def steps():
        for i in range(0, npairs, 2):                      # the chain's launches and dependencies, every step on the same two fields
            ops.masktrack_step(sel[0], sel[1], masks[int(rows[i, 1])], M.FB_LIMIT, out=masks[int(rows[i, 0])])
    stage("steps", steps, (npairs // 2) * px * 10, lambda ms: dict(launches=npairs // 2, us_per_step=round(ms * 1e3 / (npairs // 2), 2)))
    del sel
    total = event_ms(lambda: M.track_clip(src, anchor, args.anchor), args.reps)
    res["track_clip_ms"] = round(total, 3)
    res["stages_sum_ms"] = round(sum(res[k]["ms"] for k in ("pyramid", "match", "select", "steps")), 3)
    res["ms_per_frame"] = round(total / nfr, 4)
    tracked = M.track_clip(src, anchor, args.anchor)
    res["anchor_kept"] = bool(torch.equal(tracked[args.anchor], anchor))
    res["set_fraction_first_last"] = [round(float((tracked[f] >= 128).float().mean()), 4) for f in (0, nfr - 1)]
    stage("dilate_invert", lambda: M.finish(tracked, args.dilate, True), nfr * px * 4, lambda ms: dict(radius=args.dilate))
    keys = list(range(0, nfr, 7))
    if len(keys) >= 2:
        edited = (255 - src[keys]).contiguous()
        res["propagate_clip_ms"] = round(event_ms(lambda: P.propagate_clip(src, keys, edited), args.reps), 3)
    res["peak_memory_mb"] = round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
