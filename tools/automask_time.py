#!/usr/bin/env python3
"""What an automatic mask costs (ccedit_amd/automask.py, csrc/automask.hip), both arms in ONE process on one box, at 17 x 512 x 768:
  plain     `samples` ordinary sampler evaluations of a noised latent (guider, closure, CFG combine), from empty per-clip caches — the
            first evaluation eager, the second captured, the rest replayed: the life of a clip's first evaluations
  automask  AutoMask.__call__ with the same number of samples, from empty caches too: per sample a CPU noise draw, the axpby, ONE
            doubled network evaluation with (source prompt, target prompt) in the halves, the accumulate launch; then mask_from
The plain arm runs once more BEFORE both (`warmup`: the process's first evaluations pay for loading every kernel) and once more after
(`plain_again`: the box's own drift).  Reported: per arm the wall time of the whole call (synchronised) and the HIP-event time of
every closure evaluation in order; the ratio of the automask's evaluations to the plain arm's before it and after it, evaluation by
evaluation and in total; mask_from alone; each of the four kernels (and the order statistic they sit beside) under HIP events
(median of 20 after three warm-up calls) with its algorithmic bytes and TB/s; peak memory.  The full-width network with synthetic
weights.  Prints one JSON line (and writes it to --out).
  python tools/automask_time.py [--samples 4] [--out FILE]"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.region_time import LH, LW, N, build, clip_inputs, event_us, make_sampler  # noqa: E402


def timed(inner, recs):
    def closure(inp, sigma, cond):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = inner(inp, sigma, cond)
        e1.record()
        recs.append((e0, e1))
        return out
    return closure


def arm(wrapper, dev, samples, auto: bool):
    from ccedit_amd import automask, ops
    sampler, denoiser = make_sampler(dev, 4)
    z, ctx, hint = clip_inputs(dev, 43)
    c, uc = dict(crossattn=ctx[0], control_hint=hint), dict(crossattn=ctx[1], control_hint=hint.clone())
    c_src = dict(c, crossattn=ctx[2])
    sigma = float(sampler.discretization(sampler.num_steps)[2])
    wrapper.reserve_windows(0)
    wrapper.reset_caches()
    recs = []
    closure = timed(lambda inp, s, cond: denoiser(wrapper, inp, s, cond), recs)
    gen = torch.Generator().manual_seed(5)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    if auto:
        acc = automask.AutoMask(closure, wrapper=wrapper)(z, sigma, c_src, c, samples, gen)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        mask = automask.mask_from(acc)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        extra = dict(mask_from_ms=round((t2 - t1) * 1e3, 3), cells_set=round(float((mask != 0).float().mean()), 4),
                     caches_after=[len(wrapper._graphs), len(wrapper._hint_val), len(wrapper._tkv_val)])
    else:
        s_in = torch.full((1,), sigma)
        for _ in range(samples):
            x = ops.axpby(z, torch.randn(z.shape, generator=gen).to(dev), 1.0, sigma)
            out = sampler.denoise(x, closure, s_in, c, uc)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        extra = dict(finite=bool(torch.isfinite(out).all()))
    evals = [round(e0.elapsed_time(e1), 3) for e0, e1 in recs]
    return dict(wall_ms=round((t1 - t0) * 1e3, 3), evaluations_ms=evals, evaluations_total_ms=round(sum(evals), 3), sigma=round(sigma, 4),
                peak_memory_mb=round(torch.cuda.max_memory_allocated() / 2 ** 20, 1), **extra)


def kernels(dev, res):
    from ccedit_amd import automask, ops
    g = torch.Generator().manual_seed(0)
    y = torch.randn(2, 4, N, LH, LW, generator=g).to(dev)
    acc = ops.automask_accumulate(y)
    n = acc[0].numel()
    scale = ops.kth_values(acc.view(1, n), [automask.rank_of(0.99, n)]).view(1)
    bits = ops.automask_binarize(acc, scale, 0.5)
    voted = ops.automask_vote(bits, 14)
    cells = acc.numel()
    table = dict(accumulate_first=(lambda: ops.automask_accumulate(y), 4 * (y.numel() + cells)),
                 accumulate_add=(lambda: ops.automask_accumulate(y, acc), 4 * (y.numel() + 2 * cells)),
                 kth_values=(lambda: ops.kth_values(acc.view(1, n), [automask.rank_of(0.99, n)]), 4 * cells),
                 binarize=(lambda: ops.automask_binarize(acc, scale, 0.5), 5 * cells),
                 vote=(lambda: ops.automask_vote(bits, 14), 2 * cells),
                 expand=(lambda: ops.automask_expand(voted), 65 * cells))
    for name, (fn, nbytes) in table.items():
        us = event_us(fn)
        res[name] = dict(us=round(us, 2), mbytes=round(nbytes / 1e6, 3), tbytes_per_s=round(nbytes / (us * 1e-6) / 1e12, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/automask_time.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    res = dict(frames=N, frame_px=[8 * LH, 8 * LW], samples=args.samples)
    w = build(dev)
    kernels(dev, res)
    res["warmup"] = arm(w, dev, args.samples, auto=False)           # the process's first evaluations: kernels are loaded here
    res["plain"] = arm(w, dev, args.samples, auto=False)
    res["automask"] = arm(w, dev, args.samples, auto=True)
    res["plain_again"] = arm(w, dev, args.samples, auto=False)      # the same arm after the other: the box's own drift
    w.reserve_windows(0)
    a = res["automask"]
    for name in ("plain", "plain_again"):
        p = res[name]
        res["ratio_vs_" + name] = dict(per_evaluation=[round(x / y, 4) for x, y in zip(a["evaluations_ms"], p["evaluations_ms"])],
                                       evaluations_total=round(a["evaluations_total_ms"] / p["evaluations_total_ms"], 4),
                                       wall=round(a["wall_ms"] / p["wall_ms"], 4))
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
