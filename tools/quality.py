#!/usr/bin/env python3
"""The quality report (ccedit_amd/quality.py, csrc/quality.hip) of any two clips the project reads — a directory of frames, a .gif, a
Motion-JPEG .avi, an animated .png: fidelity of --b to --a (PSNR, SSIM) and the warp error of --b beside --a's own along the motion of
--guide (default: --a).  This is how two runs are compared — for instance result/ of a run with and of one without --noise_warp, each
against the same original/ — and how a result_full/ file is measured against its source.
  --mask PATH   a clip of masks (one frame: used for every frame): luma >= 128 = edited; fidelity is measured over the other pixels and
                temporal.edited is added
  --size H W    bring every clip to this size the way the entry point's sources come (default: the clips' own size, which they must share)
The warp error needs H and W multiples of 64 and two frames; otherwise "temporal" is null and says why.  Measures of fidelity and
steadiness, not of how well a prompt was followed.  Prints one JSON document.
   python tools/quality.py --a outputs/x/default/original/png/animation-0000.png --b outputs/x/default/result/png/animation-0000.png"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def read_clip(path: str, size, dev) -> torch.Tensor:
    """-> uint8 (F, H, W, 3) on `dev`: at `size` through load_video_frames_u8, or the frames as they are."""
    from ccedit_amd import video_io
    from scripts.sampling import util
    if size:
        return util.load_video_frames_u8(path, tuple(size), dev)
    kind = video_io.kind_of(path)
    if kind is video_io.FILES:
        groups = util._files_u8([os.path.join(path, f) for f in sorted(os.listdir(path))], dev, path)
    else:
        groups = util._clip_u8(kind, path, dev)
    if len(groups) != 1:
        raise SystemExit(f"{path}: frames of different sizes — give --size H W")
    return groups[0].contiguous()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--a", required=True, help="the source clip")
    ap.add_argument("--b", required=True, help="the result clip")
    ap.add_argument("--guide", default=None, help="the clip whose motion is followed (default: --a)")
    ap.add_argument("--mask", default=None, help="a clip of masks, luma >= 128 = edited")
    ap.add_argument("--size", type=int, nargs=2, default=None, metavar=("H", "W"))
    args = ap.parse_args(argv)
    from ccedit_amd import hip, quality
    torch.set_grad_enabled(False)
    hip.lib()
    if not torch.cuda.is_available():
        raise SystemExit("tools/quality.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    a, b = read_clip(args.a, args.size, dev), read_clip(args.b, args.size, dev)
    if tuple(a.shape) != tuple(b.shape):
        raise SystemExit(f"--a holds {tuple(a.shape)} and --b {tuple(b.shape)}: the same number of frames at one size (see --size)")
    mask = None
    if args.mask:
        m = read_clip(args.mask, args.size, dev).to(torch.int32)
        m = ((77 * m[..., 0] + 150 * m[..., 1] + 29 * m[..., 2] + 128) >> 8).to(torch.uint8)
        if m.shape[0] == 1:
            m = m.expand(a.shape[0], -1, -1)
        if tuple(m.shape) != tuple(a.shape[:3]):
            raise SystemExit(f"--mask holds {tuple(m.shape)} for frames {tuple(a.shape)}: one frame, or one per frame, at their size")
        mask = m.contiguous()
    if args.guide is None:
        rep = quality.report(a, b, mask)
    else:                       # another clip's motion: the same layout, the vectors from --guide
        g = read_clip(args.guide, args.size, dev)
        if tuple(g.shape) != tuple(a.shape):
            raise SystemExit(f"--guide holds {tuple(g.shape)} for frames {tuple(a.shape)}")
        temp = reason = None
        try:
            sels = ("all",) if mask is None else ("all", "edited")
            temp = {k: quality.temporal(g, b, a, mask, sel=i) for i, k in enumerate(sels)}
        except ValueError as e:
            reason = str(e)
        rep = quality.assemble(a.shape[1:3], a.shape[0], quality.compare(a, b, mask), temp, reason, mask is not None)
    rep["a"], rep["b"], rep["guide"], rep["mask"] = args.a, args.b, args.guide or args.a, args.mask
    print(json.dumps(rep, indent=2))


if __name__ == "__main__":
    main()
