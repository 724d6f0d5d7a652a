#!/usr/bin/env python3
"""What lossless PNG output costs on the two routes, frames on the device to the written file: a clip of 17 frames (the keyframes) and one
of 113 frames (the full-rate output of --propagate) of 512 x 768, photo-like (a panning texture).
The device route (ccedit_amd/png.py, csrc/png.hip) stage by stage under HIP events — filter, tokens, codes, emit, pack (scan + copy),
adler; median [min, max] of `--reps` after warm-up, summed over the launch groups of a clip — and end to end on the wall clock:
save_png_u8 from frames on the device, the download of the packed streams and the file writing included, with the bytes that crossed to
the host.  The other route end to end on the same frames: the download of 3 bytes per pixel and Pillow's save_all APNG (once per clip:
it takes seconds).  Also what Pillow takes for ONE grid PNG of 17 frames side by side (the grid stays on Pillow).  Prints one JSON line.
  python tools/png_time.py [--frames 17 113] [--H 512] [--W 768] [--reps 5] [--no-pillow]
A kernel trace of the same run:  rocprofv3 --kernel-trace --stats -- python tools/png_time.py --reps 2 --no-pillow"""
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

from tools.propagate_time import moving_clip  # noqa: E402


def spread(ts):
    return [round(statistics.median(ts), 3), round(min(ts), 3), round(max(ts), 3)]


def event_ms(fn, reps, warm=2):
    """-> [median, min, max] ms under HIP events."""
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
    return spread(ts)


def wall_ms(fn, reps, warm=1):
    """-> [median, min, max] ms on the wall clock, the device idle before and after."""
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return spread(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[17, 113])
    ap.add_argument("--H", type=int, default=512)
    ap.add_argument("--W", type=int, default=768)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-pillow", action="store_true", help="skip the Pillow route (seconds per clip)")
    args = ap.parse_args()
    from PIL import Image
    from ccedit_amd import hip, ops, png
    from scripts.sampling.util import save_png_u8
    hip.lib()
    if not torch.cuda.is_available():
        raise SystemExit("tools/png_time.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    h, w = args.H, args.W
    length = png.filtered_bytes(h, w)
    per = png.frames_per_launch(h, w)
    res = dict(size=[h, w], reps=args.reps, timing="[median, min, max] ms", device=torch.cuda.get_device_name(0), chunk=png.CHUNK,
               chunks_per_frame=png.chunks_of(length), tokens_chunks_per_workgroup=png.TOKENS_CHUNKS_PER_WORKGROUP, tokens_lanes_per_chunk=1,
               hash_entries=png.HASH_SIZE, frames_per_launch=per, slot_bytes=png.SLOT_BYTES, clips={})
    for n in args.frames:
        frames = moving_clip(n, h, w).to(dev)
        groups = [frames[s:s + per] for s in range(0, n, per)]
        out = {}
        out["filter_ms"] = event_ms(lambda: [ops.png_filter(g) for g in groups], args.reps)
        filtered = [ops.png_filter(g).reshape(-1, length) for g in groups]
        out["tokens_ms"] = event_ms(lambda: [ops.png_tokens(f) for f in filtered], args.reps)
        toks = [ops.png_tokens(f) for f in filtered]
        out["codes_ms"] = event_ms(lambda: [ops.png_codes(t[2], f.shape[0]) for t, f in zip(toks, filtered)], args.reps)
        codes = [ops.png_codes(t[2], f.shape[0]) for t, f in zip(toks, filtered)]
        out["emit_ms"] = event_ms(lambda: [ops.png_emit(t[0], t[1], c[0], c[1], c[2]) for t, c in zip(toks, codes)], args.reps)
        slots = [ops.png_emit(t[0], t[1], c[0], c[1], c[2]) for t, c in zip(toks, codes)]
        totals = [int(ops.png_pack_scan(c[3], f.shape[0])[1].sum()) for c, f in zip(codes, filtered)]

        def pack():
            for s, c, f, total in zip(slots, codes, filtered, totals):
                off, _ = ops.png_pack_scan(c[3], f.shape[0])
                ops.png_pack(s, c[3], off, f.shape[0], total)

        out["pack_ms"] = event_ms(pack, args.reps)
        out["adler_ms"] = event_ms(lambda: [ops.png_adler(f) for f in filtered], args.reps)
        out["stages_sum_ms"] = round(sum(out[k][0] for k in ("filter_ms", "tokens_ms", "codes_ms", "emit_ms", "pack_ms", "adler_ms")), 3)
        out["encode_frames_wall_ms"] = wall_ms(lambda: png.encode_frames(frames), args.reps)
        out["deflate_bytes"] = sum(totals)
        out["device_to_host_bytes"] = sum(totals) + n * (4 + 8)                  # the streams, per frame a byte count and an Adler word
        out["raw_rgb_bytes"] = n * h * w * 3
        with tempfile.TemporaryDirectory() as tmp:
            out["device_route_wall_ms"] = wall_ms(lambda: save_png_u8(os.path.join(tmp, "device"), frames, 20), args.reps)
            out["device_png_bytes"] = os.path.getsize(os.path.join(tmp, "device", "png", "animation-0000.png"))
            if not args.no_pillow:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                imgs = [Image.fromarray(f) for f in frames.cpu().numpy()]           # 3 bytes per pixel to the host
                imgs[0].save(os.path.join(tmp, "pillow.png"), save_all=True, append_images=imgs[1:], duration=50, loop=0)
                out["pillow_route_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
                out["pillow_png_bytes"] = os.path.getsize(os.path.join(tmp, "pillow.png"))
                out["speedup"] = round(out["pillow_route_wall_ms"] / out["device_route_wall_ms"][0], 1)
                if n == 17:                                                        # the grid PNG of perform_save_locally_video: stays on Pillow
                    import numpy as np
                    grid = np.concatenate(list(frames.cpu().numpy()), axis=1)
                    t0 = time.perf_counter()
                    Image.fromarray(grid).save(os.path.join(tmp, "grid.png"))
                    res["pillow_grid_png_17_frames_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        res["clips"][str(n)] = out
        print(f"[png_time] {n}: {json.dumps(out)}", file=sys.stderr, flush=True)
    res["peak_memory_mb"] = round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
