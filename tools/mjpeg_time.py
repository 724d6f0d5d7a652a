#!/usr/bin/env python3
"""What Motion-JPEG output costs (ccedit_amd/mjpeg.py, csrc/mjpeg.hip): a clip of 17 frames (the keyframes) and one of 113 frames (the
full-rate output of --propagate) of 512 x 768, stage by stage under HIP events (median of `--reps` after warm-up) — transform, entropy,
pack (scan + copy) — and encode_frames as a whole (device-to-host copies and the host's slicing included, wall clock).  Per stage:
time, bytes moved (compulsory: every input read and every output written once; for the entropy and pack stages the bytes actually
produced, not the slots reserved) and the achieved GB/s; the compressed size and the device-to-host bytes.  Beside it the wall time of
the gif route for the same frames (Pillow's per-frame adaptive palette on the host), the thing a user would otherwise wait for, with
its device-to-host bytes.  Prints one JSON line.
  python tools/mjpeg_time.py [--frames 17 113] [--H 512] [--W 768] [--quality 90] [--reps 5]
A kernel trace of the same run:  rocprofv3 --kernel-trace --stats -- python tools/mjpeg_time.py --reps 2"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.propagate_time import event_ms, moving_clip  # noqa: E402


def wall_ms(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[17, 113])
    ap.add_argument("--H", type=int, default=512)
    ap.add_argument("--W", type=int, default=768)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from ccedit_amd import hip, mjpeg, ops
    from scripts.sampling.util import save_gif_u8
    hip.lib()
    if not torch.cuda.is_available():
        raise SystemExit("tools/mjpeg_time.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    h, w, q = args.H, args.W, args.quality
    tab = mjpeg.device_tables(dev)
    header = torch.frombuffer(bytearray(mjpeg.frame_header(h, w, q)), dtype=torch.uint8).to(dev)
    res = dict(size=[h, w], quality=q, reps=args.reps, segment_bytes=ops.mjpeg_segment_bytes(w), clips={})
    for n in args.frames:
        frames = moving_clip(n, h, w).to(dev)
        px = n * h * w
        out = {}

        def stage(name, fn, nbytes):
            ms = event_ms(fn, args.reps)
            out[name] = dict(ms=round(ms, 3), mbytes=round(nbytes / 1e6, 2), gb_per_s=round(nbytes / ms / 1e6, 1))

        stage("transform", lambda: ops.mjpeg_transform(frames, tab, q), px * 3 + px * 3)
        coef = ops.mjpeg_transform(frames, tab, q)
        segments, seg_len = ops.mjpeg_entropy(coef, tab)
        coded = int(seg_len.sum())
        stage("entropy", lambda: ops.mjpeg_entropy(coef, tab), px * 3 + coded)
        _, frame_bytes = ops.mjpeg_pack_scan(seg_len, n, h, w, header.numel())
        total = int(frame_bytes.sum())

        def pack():
            off, _ = ops.mjpeg_pack_scan(seg_len, n, h, w, header.numel())
            return ops.mjpeg_pack(segments, seg_len, off, header, n, h, w, total)

        stage("pack", pack, coded + total)
        out["encode_frames_wall_ms"] = round(wall_ms(lambda: mjpeg.encode_frames(frames, q), args.reps), 3)
        out["stages_sum_ms"] = round(sum(out[k]["ms"] for k in ("transform", "entropy", "pack")), 3)
        out["compressed_bytes"] = total
        out["bytes_per_pixel"] = round(total / px, 4)
        out["device_to_host_bytes"] = total + 4 * n
        out["raw_rgb_bytes"] = px * 3
        with tempfile.TemporaryDirectory() as tmp:
            jpegs = mjpeg.encode_frames(frames, q)
            t0 = time.perf_counter()
            mjpeg.write_avi(os.path.join(tmp, "clip.avi"), jpegs, 20, h, w)
            out["write_avi_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            save_gif_u8(tmp, frames.cpu().numpy(), 20)                      # the gif route: 3 bytes per pixel to the host, Pillow's palettes
            out["gif_route_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
            out["gif_route_device_to_host_bytes"] = px * 3
            out["gif_bytes"] = os.path.getsize(os.path.join(tmp, "gif", "animation-0000.gif"))
        res["clips"][str(n)] = out
    res["peak_memory_mb"] = round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
