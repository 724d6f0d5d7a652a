#!/usr/bin/env python3
"""What decoding JPEG sources costs (ccedit_amd/jpegdec.py, csrc/jpegdec.hip): a clip of 113 frames (the source side of --propagate) of
512 x 768, as two kinds of source —
  restart    the frames of the own encoder's .avi: one restart interval per MCU row, 32 entropy threads per frame;
  norestart  Pillow-written JPEGs without restart markers: one interval, so ONE entropy thread per frame;
each decoded two ways, wall clock from compressed bytes on the host to uint8 frames on the device (median of `--reps` after warm-up):
  pillow     Pillow decodes frame by frame on one host thread, the raw frames are uploaded (today's route);
  device     jpegdec.decode: parse on the host, upload of the compressed bytes, three stages on the device.
For the device route also the host's parse time alone and the stages under HIP events.  The two routes' frames are compared byte for
byte on the way.  Prints one JSON line.
  python tools/jpegdec_time.py [--frames 113] [--H 512] [--W 768] [--quality 90] [--reps 3]"""
from __future__ import annotations

import argparse
import io
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

from tools.mjpeg_time import wall_ms  # noqa: E402
from tools.propagate_time import event_ms, moving_clip  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=113)
    ap.add_argument("--H", type=int, default=512)
    ap.add_argument("--W", type=int, default=768)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    from PIL import Image
    from ccedit_amd import hip, jpegdec, mjpeg, ops
    hip.lib()
    if not torch.cuda.is_available():
        raise SystemExit("tools/jpegdec_time.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    n, h, w, q = args.frames, args.H, args.W, args.quality
    frames = moving_clip(n, h, w)
    sources = {"restart": mjpeg.encode_frames(frames.to(dev), q), "norestart": []}
    for f in frames.numpy():
        b = io.BytesIO()
        Image.fromarray(f).save(b, format="JPEG", quality=q, subsampling="4:2:0")
        sources["norestart"].append(b.getvalue())
    res = dict(frames=n, size=[h, w], quality=q, reps=args.reps, sources={})
    for kind, jpegs in sources.items():
        def pillow():
            host = np.stack([np.array(Image.open(io.BytesIO(j)).convert("RGB")) for j in jpegs])
            return torch.from_numpy(host).to(dev)

        out = dict(compressed_bytes=sum(len(j) for j in jpegs), raw_rgb_bytes=n * h * w * 3)
        info = jpegdec.parse(jpegs[0])
        out["intervals_per_frame"] = len(info.intervals)
        assert torch.equal(pillow(), jpegdec.decode(jpegs, dev)), f"{kind}: the two routes' frames differ"
        out["pillow_wall_ms"] = round(wall_ms(pillow, args.reps), 2)
        out["device_wall_ms"] = round(wall_ms(lambda: jpegdec.decode(jpegs, dev), args.reps), 2)
        t0 = time.perf_counter()
        infos = [jpegdec.parse(j) for j in jpegs]
        out["parse_host_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        stages = dict(entropy=[], idct=[], rgb=[])
        for idx in jpegdec._groups(infos):                                      # the launches decode() makes, stage by stage
            g = infos[idx[0]]
            data, ivs, tab = (torch.from_numpy(a).to(dev) for a in jpegdec.pack_group([infos[i] for i in idx], [jpegs[i] for i in idx]))
            geo = (g.height, g.width, g.ncomp, g.hs, g.vs)
            stages["entropy"].append(event_ms(lambda: ops.jpegdec_entropy(data, ivs, tab, len(idx), *geo, g.restart_interval), args.reps))
            coef, _ = ops.jpegdec_entropy(data, ivs, tab, len(idx), *geo, g.restart_interval)
            stages["idct"].append(event_ms(lambda: ops.jpegdec_idct(coef, tab, *geo), args.reps))
            planes = ops.jpegdec_idct(coef, tab, *geo)
            stages["rgb"].append(event_ms(lambda: ops.jpegdec_rgb(planes, *geo), args.reps))
        out["launches"] = len(stages["entropy"])
        out["stage_ms"] = {k: round(sum(v), 3) for k, v in stages.items()}
        out["device_over_pillow"] = round(out["device_wall_ms"] / out["pillow_wall_ms"], 3)
        res["sources"][kind] = out
    res["peak_memory_mb"] = round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
