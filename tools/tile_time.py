#!/usr/bin/env python3
"""What a large frame costs (ccedit_amd/tiles.py, csrc/tile.hip), both arms in ONE process on one box:
  plain   a clip of 17 keyframes at 512 x 768 through DPMPP2SAncestral + VanillaCFGTV2V (the full-width network, synthetic weights)
  tiled   a clip of 17 keyframes at 1024 x 1536 through the same sampler and the tiled closure: tiles of 512 x 768 at the default
          overlap (a quarter of the tile) -> 9 tiles
Reported: (1) the HIP-event time of one tiled sampler evaluation (gather, 9 network evaluations, fuse), median over the evaluations
in which every tile replayed its graph; (2) the yardstick for the gather and fuse overhead: the count of tile evaluations times the
median replayed plain evaluation measured in the same process; their ratio; the two kernels alone (median of 20 after three warm-up
calls); the wrapper's evaluation counts; peak device memory.  Prints one JSON line (and writes it to --out).
(3) --direct: ONE direct evaluation of the network at 1024 x 1536, the only place the network ever runs at a size it has not run at
before.  It runs as a separate child process under its own `timeout`, started only after the tiled numbers are written; if it is
refused, fails or runs out of time that is written down and nothing is tried again.
  python tools/tile_time.py [--steps 4] [--out FILE] [--direct] [--direct_timeout 240]"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N, TH, TW, L, CTX = 17, 64, 96, 77, 768          # frames, the tile in latent pixels, text tokens, text width
LH, LW = 2 * TH, 2 * TW                          # the large frame: 1024 x 1536 px


def event_us(fn, reps=20, warm=3):
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
        ts.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(ts)


def clip_inputs(dev, lh, lw, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(1, 4, N, lh, lw, generator=g)
    cc, cuc = torch.randn(1, L, CTX, generator=g), torch.randn(1, L, CTX, generator=g)
    low = torch.rand(1, 1, N, lh // 4, lw // 4, generator=g)
    hint = torch.nn.functional.interpolate(low, size=(N, 8 * lh, 8 * lw), mode="trilinear", align_corners=False)
    hint = (hint * 2 - 1).repeat(1, 3, 1, 1, 1).contiguous()
    return x.to(dev), cc.to(dev), cuc.to(dev), hint.to(dev)


def make_sampler(dev, steps):
    from ccedit_amd.config import instantiate_from_config
    dd = "sgm.modules.diffusionmodules."
    denoiser = instantiate_from_config(dict(target=dd + "denoiser.DiscreteDenoiser", params=dict(
        num_idx=1000, weighting_config=dict(target=dd + "denoiser_weighting.EpsWeighting"),
        scaling_config=dict(target=dd + "denoiser_scaling.EpsScaling"),
        discretization_config=dict(target=dd + "discretizer.LegacyDDPMDiscretization")))).to(dev)
    sampler = instantiate_from_config(dict(target=dd + "sampling.DPMPP2SAncestralSampler", params=dict(
        num_steps=steps, eta=1.0, s_noise=1.0, verbose=False, discretization_config=dict(target=dd + "discretizer.LegacyDDPMDiscretization"),
        guider_config=dict(target=dd + "guiders.VanillaCFGTV2V", params=dict(scale=7.5)))))
    return sampler, denoiser


def run_clip(wrapper, dev, lh, lw, steps, tiled: bool):
    """One clip; every sampler evaluation timed with HIP events and labelled by what the wrapper did in it."""
    from ccedit_amd.tiles import TiledDenoiser
    sampler, denoiser = make_sampler(dev, steps)
    x, cc, cuc, hint = clip_inputs(dev, lh, lw, 43)
    c, uc = dict(crossattn=cc, control_hint=hint), dict(crossattn=cuc, control_hint=hint.clone())
    wrapper.reserve_windows(0)
    wrapper.reset_caches()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()

    def denoise(inp, sigma, cond):
        return denoiser(wrapper, inp, sigma, cond)

    inner = TiledDenoiser(denoise, (TH, TW), wrapper=wrapper) if tiled else denoise
    recs = []

    def closure(inp, sigma, cond):
        before = dict(wrapper.graph_counts or {})
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = inner(inp, sigma, cond)
        e1.record()
        after = dict(wrapper.graph_counts or {})
        delta = {k: after.get(k, 0) - before.get(k, 0) for k in after} if after.keys() == before.keys() else after
        kinds = [k for k, v in delta.items() if v]
        recs.append(("replay" if kinds == ["replay"] else "other", e0, e1, sum(delta.values())))
        return out

    out = sampler(closure, x, c, uc=uc)
    torch.cuda.synchronize()
    replay = [e0.elapsed_time(e1) for kind, e0, e1, _ in recs if kind == "replay"]
    other = [round(e0.elapsed_time(e1), 2) for kind, e0, e1, _ in recs if kind != "replay"]
    return dict(latent=[lh, lw], sampler_evaluations=len(recs), network_evaluations_per_sampler_evaluation=recs[-1][3],
                counts=dict(wrapper.graph_counts), first_evaluations_ms=other,
                replay_median_ms=round(statistics.median(replay), 3) if replay else None,
                replay_min_ms=round(min(replay), 3) if replay else None, replay_max_ms=round(max(replay), 3) if replay else None,
                peak_memory_mb=round(torch.cuda.max_memory_allocated() / 2 ** 20, 1), finite=bool(torch.isfinite(out).all()),
                host_compares=len(wrapper._twin_val))


def build(dev):
    from ccedit_amd import hip
    from ccedit_amd.sgm_compat import build_network
    from ccedit_amd.utils.synth import fill_module_
    torch.set_grad_enabled(False)
    hip.lib()
    w = build_network(dev)
    fill_module_(w, prefix="model.")
    w.diffusion_model.pack(dev)
    return w


def direct_child():
    """One eager evaluation of the network at the large size, then one more, timed.  Its own process: whatever happens here ends here."""
    dev = torch.device("cuda:0")
    w = build(dev)
    w.use_graph = False
    x, cc, cuc, hint = clip_inputs(dev, LH, LW, 43)
    x2 = torch.cat([x, x])
    t = torch.full((2,), 500, dtype=torch.int64, device=dev)
    cond = dict(crossattn=torch.cat([cuc, cc]), control_hint=torch.cat([hint, hint]))
    ms = []
    for _ in range(2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = w(x2, t, cond)
        e1.record()
        torch.cuda.synchronize()
        ms.append(round(e0.elapsed_time(e1), 2))
    print(json.dumps(dict(direct_evaluations_ms=ms, finite=bool(torch.isfinite(out).all()),
                          peak_memory_mb=round(torch.cuda.max_memory_allocated() / 2 ** 20, 1))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--out", type=str, default="")
    ap.add_argument("--direct", action="store_true")
    ap.add_argument("--direct_timeout", type=int, default=240)
    ap.add_argument("--direct_child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/tile_time.py measures on the GPU; none is visible")
    if args.direct_child:
        return direct_child()
    from ccedit_amd import ops
    from ccedit_amd.tiles import default_overlap, plan2d
    dev = torch.device("cuda:0")
    oh, ow = default_overlap(TH, TW)
    starts, coef = plan2d(LH, LW, TH, TW, oh, ow)
    res = dict(frames=N, frame_px=[8 * LH, 8 * LW], tile_px=[8 * TH, 8 * TW], overlap_px=[8 * oh, 8 * ow], tiles=len(starts), steps=args.steps)

    w = build(dev)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 4, N, LH, LW, generator=g).to(dev)
    ys = [torch.randn(2, 4, N, TH, TW, generator=g).to(dev) for _ in starts]
    sd, cd = torch.tensor(starts, dtype=torch.int32, device=dev).reshape(-1, 2), torch.from_numpy(coef).to(dev)
    res["gather_us"] = round(event_us(lambda: ops.tile_gather(x, sd, TH, TW)), 2)
    res["fuse_us"] = round(event_us(lambda: ops.tile_fuse(ys, sd, cd, LH, LW)), 2)
    res["gather_mbytes"] = round(8 * len(starts) * ys[0].numel() / 1e6, 2)
    res["fuse_mbytes"] = round(4 * (len(starts) * ys[0].numel() + coef.size + x.numel()) / 1e6, 2)
    del x, ys

    res["plain"] = run_clip(w, dev, TH, TW, args.steps, tiled=False)
    res["tiled"] = run_clip(w, dev, LH, LW, args.steps, tiled=True)
    res["plain_again"] = run_clip(w, dev, TH, TW, args.steps, tiled=False)       # the same arm after the other: the box's own drift
    w.reserve_windows(0)
    p, q = res["plain"]["replay_median_ms"], res["tiled"]["replay_median_ms"]
    res["tiled_evaluation_ms"] = q
    res["yardstick_ms"] = round(len(starts) * p, 3) if p else None
    res["ratio"] = round(q / (len(starts) * p), 4) if p and q else None
    res["direct"] = "not run"
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if args.direct:
        # a fresh child process (this one keeps its GPU state), under its own time limit; one attempt
        cmd = ["timeout", "-k", "10", str(args.direct_timeout), sys.executable, os.path.abspath(__file__), "--direct_child"]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
            last = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ""
            direct = json.loads(last) if r.returncode == 0 and last.startswith("{") else dict(
                failed=True, exit_status=r.returncode, stderr_tail=r.stderr[-600:])
        except Exception as e:          # (could not even be started: written down like any other failure)
            direct = dict(failed=True, error=f"{type(e).__name__}: {e}")
        res["direct"] = direct
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
