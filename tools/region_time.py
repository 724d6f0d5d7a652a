#!/usr/bin/env python3
"""What region prompts cost (ccedit_amd/regions.py, csrc/region.hip), both arms in ONE process on one box, at 17 x 512 x 768 with K = 2:
  plain    a clip of 17 keyframes at 512 x 768 through DPMPP2SAncestral + VanillaCFGTV2V (the full-width network, synthetic weights)
  regions  the same clip through the region closure: 3 text contexts (the base prompt and two regions: the right half of the frame
           and a band across it, feathered over one latent cell), so 3 network evaluations per sampler evaluation and one fuse
Reported: (1) the HIP-event time of one region sampler evaluation (3 network evaluations, fuse), median over the evaluations in which
every context replayed its graph; (2) the yardstick: (K + 1) times the median replayed plain evaluation measured in the same process
— never the new code; their ratio; (3) the two kernels alone under HIP events (median of 20 after three warm-up calls) with their
algorithmic bytes and GB/s; the wrapper's evaluation counts and cache sizes; peak device memory.  Prints one JSON line (and writes it
to --out).
  python tools/region_time.py [--steps 4] [--out FILE]"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N, LH, LW, L, CTX, K, FEATHER = 17, 64, 96, 77, 768, 2, 1          # frames, the latent, text tokens, text width, regions, feather


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


def region_masks() -> np.ndarray:
    """uint8 (K, N, 512, 768): region 1 the right half of the frame, region 2 a band across it (they overlap)."""
    m = np.zeros((K, N, 8 * LH, 8 * LW), np.uint8)
    m[0, :, :, 4 * LW:] = 255
    m[1, :, 3 * LH:5 * LH, :] = 255
    return m


def clip_inputs(dev, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(1, 4, N, LH, LW, generator=g)
    ctx = [torch.randn(1, L, CTX, generator=g) for _ in range(K + 2)]          # the base prompt, the negative prompt, K regions
    low = torch.rand(1, 1, N, LH // 4, LW // 4, generator=g)
    hint = torch.nn.functional.interpolate(low, size=(N, 8 * LH, 8 * LW), mode="trilinear", align_corners=False)
    hint = (hint * 2 - 1).repeat(1, 3, 1, 1, 1).contiguous()
    return x.to(dev), [v.to(dev) for v in ctx], hint.to(dev)


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


def run_clip(wrapper, dev, steps, coef=None):
    """One clip; every sampler evaluation timed with HIP events and labelled by what the wrapper did in it."""
    from ccedit_amd.regions import RegionDenoiser
    sampler, denoiser = make_sampler(dev, steps)
    x, ctx, hint = clip_inputs(dev, 43)
    c, uc = dict(crossattn=ctx[0], control_hint=hint), dict(crossattn=ctx[1], control_hint=hint.clone())
    wrapper.reserve_windows(0)
    wrapper.reset_caches()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()

    def denoise(inp, sigma, cond):
        return denoiser(wrapper, inp, sigma, cond)

    inner = denoise if coef is None else RegionDenoiser(denoise, [ctx[0]] + ctx[2:], coef, wrapper=wrapper)
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
    return dict(sampler_evaluations=len(recs), network_evaluations_per_sampler_evaluation=recs[-1][3], counts=dict(wrapper.graph_counts),
                first_evaluations_ms=other, replay_median_ms=round(statistics.median(replay), 3) if replay else None,
                replay_min_ms=round(min(replay), 3) if replay else None, replay_max_ms=round(max(replay), 3) if replay else None,
                peak_memory_mb=round(torch.cuda.max_memory_allocated() / 2 ** 20, 1), finite=bool(torch.isfinite(out).all()),
                host_compares=len(wrapper._twin_val), graphs=len(wrapper._graphs), hint_stem_entries=len(wrapper._hint_val),
                text_kv_entries=len(wrapper._tkv_val))


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/region_time.py measures on the GPU; none is visible")
    from ccedit_amd import ops, regions
    dev = torch.device("cuda:0")
    res = dict(frames=N, frame_px=[8 * LH, 8 * LW], regions=K, contexts=K + 1, feather=FEATHER, steps=args.steps)

    masks = torch.from_numpy(region_masks()).to(dev)
    coef = regions.weights(masks, FEATHER)
    g = torch.Generator().manual_seed(0)
    ys = [torch.randn(2, 4, N, LH, LW, generator=g).to(dev) for _ in range(K + 1)]
    res["weights_us"] = round(event_us(lambda: ops.region_weights(masks, FEATHER)), 2)
    res["fuse_us"] = round(event_us(lambda: ops.region_fuse(ys, coef)), 2)
    # algorithmic bytes: every operand read once, the result written once (the fuse skips evaluations whose coefficients are 0 —
    # `fuse_read_mbytes` counts what it does read at these masks)
    res["weights_mbytes"] = round((masks.numel() + 4 * coef.numel()) / 1e6, 2)
    res["fuse_mbytes"] = round(4 * ((K + 1) * ys[0].numel() + coef.numel() + ys[0].numel()) / 1e6, 2)
    c4 = (coef.reshape(K + 1, -1, 4) != 0).any(dim=2).float().mean().item()          # share of the 16-byte groups that are read
    res["fuse_read_mbytes"] = round(4 * (c4 * (K + 1) * ys[0].numel() + coef.numel() + ys[0].numel()) / 1e6, 2)
    for k in ("weights", "fuse"):
        res[k + "_gbytes_per_s"] = round(res[k + "_mbytes"] * 1e6 / (res[k + "_us"] * 1e-6) / 1e9, 1)
    res["fuse_read_gbytes_per_s"] = round(res["fuse_read_mbytes"] * 1e6 / (res["fuse_us"] * 1e-6) / 1e9, 1)
    del ys

    w = build(dev)
    res["plain"] = run_clip(w, dev, args.steps)
    res["regions_clip"] = run_clip(w, dev, args.steps, coef=coef)
    res["plain_again"] = run_clip(w, dev, args.steps)                 # the same arm after the other: the box's own drift
    w.reserve_windows(0)
    p, q = res["plain"]["replay_median_ms"], res["regions_clip"]["replay_median_ms"]
    res["region_evaluation_ms"] = q
    res["yardstick_ms"] = round((K + 1) * p, 3) if p else None
    res["ratio"] = round(q / ((K + 1) * p), 4) if p and q else None
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
