#!/usr/bin/env python3
"""What GIF output costs on the two routes (--gif_encoder pillow | device): a clip of 17 frames (the keyframes) and one of 113 frames (the
full-rate output of --propagate) of 512 x 768, photo-like (a panning texture), and one flat clip of 17 frames, the histogram's worst
case (every pixel of a wave in one cell).
The device route (ccedit_amd/gif.py, csrc/gif.hip) stage by stage under HIP events (median of `--reps` after warm-up, summed over the
launch groups of a clip) — histogram, palette (prefix sums + cuts), map, lzw, pack (scan + copy) — and end to end on the wall clock:
save_gif_u8(gif_encoder="device") from frames on the device, the download of palettes and LZW bytes and the file writing included.
The Pillow route end to end on the same frames: the download of 3 bytes per pixel and save_gif_u8 as the parent writes it (once per
clip: it takes seconds).  Prints one JSON line.
  python tools/gif_time.py [--frames 17 113] [--H 512] [--W 768] [--reps 5] [--no-pillow]
A kernel trace of the same run:  rocprofv3 --kernel-trace --stats -- python tools/gif_time.py --reps 2 --no-pillow"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.mjpeg_time import wall_ms  # noqa: E402
from tools.propagate_time import event_ms, moving_clip  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[17, 113])
    ap.add_argument("--H", type=int, default=512)
    ap.add_argument("--W", type=int, default=768)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-pillow", action="store_true", help="skip the Pillow route (seconds per clip)")
    args = ap.parse_args()
    from ccedit_amd import gif, hip, ops
    from scripts.sampling.util import save_gif_u8
    hip.lib()
    if not torch.cuda.is_available():
        raise SystemExit("tools/gif_time.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    h, w = args.H, args.W
    per = gif.frames_per_launch(h, w)
    res = dict(size=[h, w], reps=args.reps, chunk=gif.CHUNK, chunks_per_frame=gif.chunks_of(h, w), lzw_chunks_per_workgroup=gif.LZW_CHUNKS_PER_WORKGROUP,
               lzw_lanes_per_chunk=1, frames_per_launch=per, slot_bytes=gif.SLOT_BYTES, clips={})
    clips = [(str(n), moving_clip(n, h, w)) for n in args.frames]
    clips.append(("flat17", torch.full((17, h, w, 3), 200, dtype=torch.uint8)))
    for name, host_frames in clips:
        frames = host_frames.to(dev)
        n = frames.shape[0]
        px = n * h * w
        groups = [frames[s:s + per] for s in range(0, n, per)]
        out = {}

        def stage(key, fn):
            out[key] = round(event_ms(fn, args.reps), 3)

        stage("histogram_ms", lambda: [ops.gif_histogram(g) for g in groups])
        moments = [ops.gif_histogram(g) for g in groups]
        stage("palette_ms", lambda: [ops.gif_palette(m.clone()) for m in moments])          # (in place: on a copy; the copy is timed too)
        stage("moments_copy_ms", lambda: [m.clone() for m in moments])
        tables = [ops.gif_palette(m) for m in moments]
        stage("map_ms", lambda: [ops.gif_map(g, t[0]) for g, t in zip(groups, tables)])
        indices = [ops.gif_map(g, t[0]) for g, t in zip(groups, tables)]
        stage("lzw_ms", lambda: [ops.gif_lzw(i) for i in indices])
        coded = [ops.gif_lzw(i) for i in indices]
        totals = [int(ops.gif_pack_scan(c[1], i.shape[0], h, w)[1].sum()) for c, i in zip(coded, indices)]

        def pack():
            for (slots, bits), i, total in zip(coded, indices, totals):
                off, _ = ops.gif_pack_scan(bits, i.shape[0], h, w)
                ops.gif_pack(slots, bits, off, i.shape[0], h, w, gif.CHUNK, total)

        stage("pack_ms", pack)
        out["palette_ms"] = round(out["palette_ms"] - out.pop("moments_copy_ms"), 3)
        out["stages_sum_ms"] = round(sum(out[k] for k in ("histogram_ms", "palette_ms", "map_ms", "lzw_ms", "pack_ms")), 3)
        out["encode_frames_wall_ms"] = round(wall_ms(lambda: gif.encode_frames(frames), args.reps), 3)
        out["lzw_bytes"] = sum(totals)
        out["device_to_host_bytes"] = sum(totals) + n * (768 + 4)
        out["raw_rgb_bytes"] = px * 3
        with tempfile.TemporaryDirectory() as tmp:
            out["device_route_wall_ms"] = round(wall_ms(lambda: save_gif_u8(os.path.join(tmp, "device"), frames, 20, gif_encoder="device"),
                                                        args.reps), 3)
            out["device_gif_bytes"] = os.path.getsize(os.path.join(tmp, "device", "gif", "animation-0000.gif"))
            if not args.no_pillow:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                save_gif_u8(os.path.join(tmp, "pillow"), frames.cpu().numpy(), 20)           # the parent's route: 3 bytes per pixel to the host
                out["pillow_route_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
                out["pillow_gif_bytes"] = os.path.getsize(os.path.join(tmp, "pillow", "gif", "animation-0000.gif"))
                out["speedup"] = round(out["pillow_route_wall_ms"] / out["device_route_wall_ms"], 1)
        res["clips"][name] = out
        print(f"[gif_time] {name}: {json.dumps(out)}", file=sys.stderr, flush=True)
    res["peak_memory_mb"] = round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
