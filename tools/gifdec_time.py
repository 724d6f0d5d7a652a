#!/usr/bin/env python3
"""What decoding GIF sources costs (ccedit_amd/gifdec.py, csrc/gifdec.hip): clips of 17 frames (the keyframes) and 113 frames (the source
side of --propagate) of 512 x 768, as files of the project's two writers —
  pillow     video_io._write_gif_pillow (Pillow's writer: a global palette, later frames cropped to what changed, a transparent index);
  device     the device writer's format (ccedit_amd/gif.py: local palettes, a Clear every 3072 pixels);
each decoded two ways, wall clock from the file's bytes on the host to uint8 frames on the device (median of `--reps` after warm-up):
  host       Pillow decodes frame by frame on one host thread (video_io._sequence_u8), the raw frames are uploaded;
  device     gifdec.decode_gif: parse on the host, upload of the compressed bytes, three stages on the device.
For the device route also the host's parse time alone, the stages under HIP events, and per frame the code count and the longest string
(one lane of stage B walks a whole string: a long one is a long lane).  The two routes' frames are compared byte for byte on the way.
Prints one JSON line.
  python tools/gifdec_time.py [--frames 17 113] [--H 512] [--W 768] [--reps 3]"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
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
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    from ccedit_amd import gif, gifdec, hip, ops, video_io
    hip.lib()
    if not torch.cuda.is_available():
        raise SystemExit("tools/gifdec_time.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    h, w = args.H, args.W
    res = dict(size=[h, w], reps=args.reps, clips={})
    for n in args.frames:
        frames = moving_clip(n, h, w)
        clip = {}
        with tempfile.TemporaryDirectory() as tmp:
            paths = dict(pillow=video_io._write_gif_pillow(os.path.join(tmp, "pillow.gif"), list(frames.numpy()), 10),
                         device=gif.write_gif(os.path.join(tmp, "device.gif"), gif.encode_frames(frames.to(dev)), 100, w, h))
            for kind, path in paths.items():
                with open(path, "rb") as f:
                    data = f.read()

                def host():
                    return torch.from_numpy(video_io._sequence_u8(path)).to(dev)

                def device():
                    return gifdec.decode_gif(data, dev)

                out = dict(compressed_bytes=len(data), raw_rgb_bytes=n * h * w * 3)
                assert torch.equal(host(), device()), f"{kind}: the two routes' frames differ"
                out["host_wall_ms"] = round(wall_ms(host, args.reps), 2)
                out["device_wall_ms"] = round(wall_ms(device, args.reps), 2)
                t0 = time.perf_counter()
                info = gifdec.parse(data)
                out["parse_host_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
                stages = dict(codes=[], pixels=[], compose=[])
                counts, longest = [], []
                per = gifdec.frames_per_launch(info)
                canvas = torch.zeros((h, w, 3), dtype=torch.uint8, device=dev)
                for s in range(0, n, per):                                       # the launches decode_gif makes, stage by stage
                    part = info.frames[s:s + per]
                    packed, desc, codes, plane, largest = gifdec.describe(part, list(range(len(part))))
                    packed, desc_d = torch.from_numpy(packed).to(dev), torch.from_numpy(desc).to(dev)
                    stages["codes"].append(event_ms(lambda: ops.gifdec_codes(packed, desc_d, codes), args.reps))
                    table, ends, ncodes, _ = ops.gifdec_codes(packed, desc_d, codes)
                    stages["pixels"].append(event_ms(lambda: ops.gifdec_pixels(desc_d, table, ends, ncodes, plane, largest), args.reps))
                    planes = ops.gifdec_pixels(desc_d, table, ends, ncodes, plane, largest)
                    stages["compose"].append(event_ms(lambda: ops.gifdec_compose(packed, desc_d, planes, canvas, len(part)), args.reps))
                    lengths, nc = table[1].cpu().numpy(), ncodes.cpu().numpy()
                    for i in range(len(part)):
                        lo = int(desc[i, gifdec.D_CODE_OFF])
                        counts.append(int(nc[i]))
                        longest.append(int(lengths[lo:lo + nc[i]].max()))
                out["launches"] = len(stages["codes"])
                out["stage_ms"] = {k: round(sum(v), 3) for k, v in stages.items()}
                out["codes_per_frame"] = dict(min=min(counts), median=int(np.median(counts)), max=max(counts))
                out["longest_string_per_frame"] = dict(min=min(longest), median=int(np.median(longest)), max=max(longest))
                out["device_over_host"] = round(out["device_wall_ms"] / out["host_wall_ms"], 3)
                clip[kind] = out
        res["clips"][str(n)] = clip
    res["peak_memory_mb"] = round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
