#!/usr/bin/env python3
"""What a long clip costs (ccedit_amd/windows.py, csrc/window.hip), both arms in ONE process on one box:
  plain     a clip of 17 keyframes at 512 x 768 through DPMPP2SAncestral + VanillaCFGTV2V (the full-width network, synthetic weights)
  windowed  a clip of 41 keyframes through the same sampler and the windowed closure: windows of 17, overlap 8 -> W = 4
Reported per arm: the HIP-event time of every network evaluation, the eager and the capturing ones listed apart from the median of
the replayed ones; the wrapper's evaluation counts; peak device memory.  And the two kernels alone at the production size (median of
20 after three warm-up calls).  The claim to check: a windowed clip costs W plain network evaluations per sampler evaluation and no
more — `replay_ratio` is the windowed median per replayed evaluation over the plain one.  Prints one JSON line.
  python tools/window_time.py [--steps 8] [--frames 41] [--window 17] [--overlap 8]"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

H, W, L, CTX = 64, 96, 77, 768


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


def clip_inputs(dev, n, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(1, 4, n, H, W, generator=g)
    cc, cuc = torch.randn(1, L, CTX, generator=g), torch.randn(1, L, CTX, generator=g)
    low = torch.rand(1, 1, n, H // 4, W // 4, generator=g)
    hint = torch.nn.functional.interpolate(low, size=(n, 8 * H, 8 * W), mode="trilinear", align_corners=False)
    hint = (hint * 2 - 1).repeat(1, 3, 1, 1, 1).contiguous()
    return x.to(dev), cc.to(dev), cuc.to(dev), hint.to(dev)


def run_clip(wrapper, dev, n, steps, window=None, overlap=None):
    from ccedit_amd.config import instantiate_from_config
    from ccedit_amd.windows import WindowedDenoiser
    dd = "sgm.modules.diffusionmodules."
    denoiser = instantiate_from_config(dict(target=dd + "denoiser.DiscreteDenoiser", params=dict(
        num_idx=1000, weighting_config=dict(target=dd + "denoiser_weighting.EpsWeighting"),
        scaling_config=dict(target=dd + "denoiser_scaling.EpsScaling"),
        discretization_config=dict(target=dd + "discretizer.LegacyDDPMDiscretization")))).to(dev)
    sampler = instantiate_from_config(dict(target=dd + "sampling.DPMPP2SAncestralSampler", params=dict(
        num_steps=steps, eta=1.0, s_noise=1.0, verbose=False, discretization_config=dict(target=dd + "discretizer.LegacyDDPMDiscretization"),
        guider_config=dict(target=dd + "guiders.VanillaCFGTV2V", params=dict(scale=7.5)))))
    x, cc, cuc, hint = clip_inputs(dev, n, 43)
    c, uc = dict(crossattn=cc, control_hint=hint), dict(crossattn=cuc, control_hint=hint.clone())
    wrapper.reserve_windows(0)
    wrapper.reset_caches()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    recs = []

    def network(xx, tt, cond):
        before = dict(wrapper.graph_counts)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = wrapper(xx, tt, cond)
        e1.record()
        kind = next((k for k, v in wrapper.graph_counts.items() if v != before.get(k, 0)), "eager")
        recs.append((kind, e0, e1))
        return out

    def denoise(inp, sigma, cond):
        return denoiser(network, inp, sigma, cond)

    closure = denoise if window is None else WindowedDenoiser(denoise, window, overlap, wrapper=wrapper)
    out = sampler(closure, x, c, uc=uc)
    torch.cuda.synchronize()
    ms = {}
    for kind, e0, e1 in recs:
        ms.setdefault(kind, []).append(e0.elapsed_time(e1))
    res = dict(frames=n, sampler_evaluations=2 * steps - 1, network_evaluations=len(recs), counts=dict(wrapper.graph_counts),
               eager_ms=[round(v, 2) for v in ms.get("eager", [])], capture_ms=[round(v, 2) for v in ms.get("capture", [])],
               replay_median_ms=round(statistics.median(ms["replay"]), 3) if ms.get("replay") else None,
               replay_min_ms=round(min(ms["replay"]), 3) if ms.get("replay") else None,
               replay_max_ms=round(max(ms["replay"]), 3) if ms.get("replay") else None,
               peak_memory_mb=round(torch.cuda.max_memory_allocated() / 2 ** 20, 1), finite=bool(torch.isfinite(out).all()),
               host_compares=len(wrapper._twin_val))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--frames", type=int, default=41)
    ap.add_argument("--window", type=int, default=17)
    ap.add_argument("--overlap", type=int, default=8)
    args = ap.parse_args()
    from ccedit_amd import hip, ops
    from ccedit_amd.sgm_compat import build_network
    from ccedit_amd.utils.synth import fill_module_
    from ccedit_amd.windows import plan
    torch.set_grad_enabled(False)
    hip.lib()
    if not torch.cuda.is_available():
        raise SystemExit("tools/window_time.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    n, t = args.frames, args.window
    starts, coef = plan(n, t, args.overlap)
    res = dict(window=t, overlap=args.overlap, starts=starts, steps=args.steps)

    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 4, n, H, W, generator=g).to(dev)
    ys = [torch.randn(2, 4, t, H, W, generator=g).to(dev) for _ in starts]
    sd, cd = torch.tensor(starts, dtype=torch.int32, device=dev), torch.from_numpy(coef).to(dev)
    res["gather_us"] = round(event_us(lambda: ops.window_gather(x, sd, t)), 2)
    res["fuse_us"] = round(event_us(lambda: ops.window_fuse(ys, sd, cd, n)), 2)
    res["gather_mbytes"] = round(8 * len(starts) * ys[0].numel() / 1e6, 2)
    res["fuse_mbytes"] = round(4 * (len(starts) * ys[0].numel() + x.numel()) / 1e6, 2)
    del x, ys

    w = build_network(dev)
    fill_module_(w, prefix="model.")
    w.diffusion_model.pack(dev)
    res["plain"] = run_clip(w, dev, t, args.steps)
    res["windowed"] = run_clip(w, dev, n, args.steps, window=t, overlap=args.overlap)
    res["plain_again"] = run_clip(w, dev, t, args.steps)           # the same arm after the other: the box's own drift
    p, q = res["plain"]["replay_median_ms"], res["windowed"]["replay_median_ms"]
    res["replay_ratio"] = round(q / p, 4) if p and q else None
    print(json.dumps(res))


if __name__ == "__main__":
    main()
