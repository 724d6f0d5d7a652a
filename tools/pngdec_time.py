#!/usr/bin/env python3
"""What decoding PNG sources costs (ccedit_amd/pngdec.py, csrc/pngdec.hip): clips of 17 frames (the keyframes) and 113 frames (the source
side of --propagate) of 512 x 768, as two kinds of source —
  files      Pillow-written .png frame files (zlib level 6, adaptive filters);
  apng       the own encoder's animated .png (ccedit_amd/png.py: one dynamic block per 16 KiB);
each decoded two ways, wall clock from compressed bytes on the host to uint8 frames on the device (median of `--reps` after warm-up):
  host       Pillow decodes frame by frame on one host thread, the raw frames are uploaded (the route without this decoder);
  device     pngdec.decode / decode_apng: parse on the host, upload of the compressed bytes, two stages on the device.
For the device route also the host's parse time alone and the stages under HIP events.  The two routes' frames are compared byte for
byte on the way.  Prints one JSON line.
  python tools/pngdec_time.py [--frames 17 113] [--H 512] [--W 768] [--reps 3]"""
from __future__ import annotations

import argparse
import io
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
    from PIL import Image, ImageSequence
    from ccedit_amd import hip, ops, png, pngdec
    hip.lib()
    if not torch.cuda.is_available():
        raise SystemExit("tools/pngdec_time.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    h, w = args.H, args.W
    res = dict(size=[h, w], reps=args.reps, clips={})
    for n in args.frames:
        frames = moving_clip(n, h, w)
        files = []
        for f in frames.numpy():
            b = io.BytesIO()
            Image.fromarray(f).save(b, format="PNG")
            files.append(b.getvalue())
        with tempfile.TemporaryDirectory() as tmp:
            path = png.write_apng(os.path.join(tmp, "clip.png"), png.encode_frames(frames.to(dev)), 100, w, h)
            with open(path, "rb") as f:
                apng = f.read()
        clip = {}
        for kind in ("files", "apng"):
            if kind == "files":
                def host():
                    return torch.from_numpy(np.stack([np.array(Image.open(io.BytesIO(d))) for d in files])).to(dev)

                def device():
                    return pngdec.decode(files, dev)

                def parse():
                    return [s for d in files for s in pngdec.parse(d).frames]
                compressed = sum(len(d) for d in files)
            else:
                def host():
                    return torch.from_numpy(np.stack([np.array(fr.convert("RGB")) for fr in ImageSequence.Iterator(Image.open(io.BytesIO(apng)))])).to(dev)

                def device():
                    return pngdec.decode_apng(apng, dev)

                def parse():
                    return pngdec.parse(apng).frames
                compressed = len(apng)
            out = dict(compressed_bytes=compressed, raw_rgb_bytes=n * h * w * 3)
            assert torch.equal(host(), device()), f"{kind}: the two routes' frames differ"
            out["host_wall_ms"] = round(wall_ms(host, args.reps), 2)
            out["device_wall_ms"] = round(wall_ms(device, args.reps), 2)
            t0 = time.perf_counter()
            streams = parse()
            out["parse_host_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
            stages = dict(inflate=[], unfilter=[])
            per = pngdec.frames_per_launch(h, w)
            for s in range(0, n, per):                                           # the launches decode() makes, stage by stage
                data, table = (torch.from_numpy(a).to(dev) for a in pngdec.pack_streams(streams[s:s + per]))
                stages["inflate"].append(event_ms(lambda: ops.pngdec_inflate(data, table, h, w), args.reps))
                filtered, _ = ops.pngdec_inflate(data, table, h, w)
                stages["unfilter"].append(event_ms(lambda: ops.pngdec_unfilter(filtered, h, w), args.reps))
            out["launches"] = len(stages["inflate"])
            out["stage_ms"] = {k: round(sum(v), 3) for k, v in stages.items()}
            out["device_over_host"] = round(out["device_wall_ms"] / out["host_wall_ms"], 3)
            clip[kind] = out
        res["clips"][str(n)] = clip
    res["peak_memory_mb"] = round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
