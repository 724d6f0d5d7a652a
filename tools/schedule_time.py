#!/usr/bin/env python3
"""What a prompt schedule costs (ccedit_amd/schedule.py, csrc/prompt.hip, the per-frame arm of csrc/attntext.hip), everything in ONE
process on one box, at 17 x 512 x 768:
  plain      a clip of 17 keyframes at 512 x 768 through DPMPP2SAncestral + VanillaCFGTV2V (the full-width network, synthetic weights)
  schedule   the same clip with a text context per frame: three prompts keyed at frames 0, 8 and 16, linear ease
Reported: (1) the HIP-event time of one sampler evaluation with per-frame contexts, median over the evaluations that replayed their
graph, against the same figure of plain clips run BEFORE and AFTER it (the yardstick and the box's own drift); (2) the once-per-clip
text K / V GEMM of both networks for 2 x 17 x 77 context rows against 2 x 77; (3) ccedit_prompt_schedule alone; (4) the per-launch table:
the text attention of the four levels (34 frames; 6144 / 1536 / 384 / 96 query rows; 77 keys; 8 heads of 40 / 80 / 160 / 160) with
K / V per frame under policy attn_text 1 / 0 — where the per-frame arm applies (d = 80 from 1536 rows per frame) that is the arm
against the general kernel, elsewhere the general kernel twice (the kernel labels are reported; the flag keeps the shared arm off
either way) — and further row counts around the arm's lower limit.  Operands are cold: four rotating buffer sets, each query buffer rewritten
by a producer pass right before its launch (as the to_q GEMM leaves it in the network), the two arms alternating launch by launch;
median, min and max per arm, and the medians of the first and the second half of the repetitions as the run-to-run spread.
Prints one JSON line (and writes it to --out).
  python tools/schedule_time.py [--steps 4] [--reps 10] [--out FILE]"""
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

N, LH, LW, L, CTX = 17, 64, 96, 77, 768          # frames, the latent, text tokens, text width
KEYS = [(0, 0), (8, 1), (16, 2)]                 # (keyframe, prompt): three prompts over the clip
NB = 4                                           # rotating buffer sets of the per-launch table
KV_LD = 24960                                    # row stride of the UNet's batched text K / V projection (16 blocks)


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


def clip_inputs(dev, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(1, 4, N, LH, LW, generator=g)
    ctx = torch.randn(4, L, CTX, generator=g)                                  # three prompts and the negative prompt
    low = torch.rand(1, 1, N, LH // 4, LW // 4, generator=g)
    hint = torch.nn.functional.interpolate(low, size=(N, 8 * LH, 8 * LW), mode="trilinear", align_corners=False)
    hint = (hint * 2 - 1).repeat(1, 3, 1, 1, 1).contiguous()
    return x.to(dev), ctx.to(dev), hint.to(dev)


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


def run_clip(wrapper, dev, steps, scheduled: bool):
    """One clip; every sampler evaluation timed with HIP events and labelled by what the wrapper did in it."""
    from ccedit_amd import schedule
    sampler, denoiser = make_sampler(dev, steps)
    x, ctx, hint = clip_inputs(dev, 43)
    c, uc = dict(crossattn=ctx[:1].contiguous(), control_hint=hint), dict(crossattn=ctx[3:].contiguous(), control_hint=hint.clone())
    if scheduled:
        c["crossattn"], uc["crossattn"] = schedule.conditioning(ctx[:3].contiguous(), ctx[3:], schedule.plan(KEYS, N, "linear"))
    wrapper.reserve_windows(0)
    wrapper.reset_caches()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    recs = []

    def closure(inp, sigma, cond):
        before = dict(wrapper.graph_counts or {})
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = denoiser(wrapper, inp, sigma, cond)
        e1.record()
        after = dict(wrapper.graph_counts or {})
        delta = {k: after.get(k, 0) - before.get(k, 0) for k in after} if after.keys() == before.keys() else after
        kinds = [k for k, v in delta.items() if v]
        recs.append(("replay" if kinds == ["replay"] else "other", e0, e1))
        return out

    out = sampler(closure, x, c, uc=uc)
    torch.cuda.synchronize()
    replay = [e0.elapsed_time(e1) for kind, e0, e1 in recs if kind == "replay"]
    other = [round(e0.elapsed_time(e1), 2) for kind, e0, e1 in recs if kind != "replay"]
    return dict(sampler_evaluations=len(recs), counts=dict(wrapper.graph_counts), first_evaluations_ms=other,
                replay_median_ms=round(statistics.median(replay), 3) if replay else None,
                replay_min_ms=round(min(replay), 3) if replay else None, replay_max_ms=round(max(replay), 3) if replay else None,
                peak_memory_mb=round(torch.cuda.max_memory_allocated() / 2 ** 20, 1), finite=bool(torch.isfinite(out).all()),
                context_rows=int(c["crossattn"].shape[0] + uc["crossattn"].shape[0]) * L, text_kv_entries=len(wrapper._tkv_val),
                text_kv_mbytes=round(sum(t.kv_all.numel() * 2 for t in wrapper._tkv_val.values() if t.kv_all is not None) / 2 ** 20, 1))


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


def attention_row(dev, d, lq, reps, frames=34, heads=8):
    """One row of the per-launch table: text attention with K / V per frame on the arm (policy attn_text = 1) and on the general
    kernel (0), cold operands, alternating."""
    from ccedit_amd import hip, ops
    lib = hip.lib()
    c = heads * d
    g = torch.Generator().manual_seed(d + lq)
    src = torch.randn(frames * lq, c, generator=g).to(torch.bfloat16).to(dev)
    sets = []
    for i in range(NB):
        kv = torch.randn(frames * L, 2 * c + 64, generator=g).to(torch.bfloat16)
        wide = torch.empty(frames * L, KV_LD, dtype=torch.bfloat16, device=dev)             # this block's [K | V] inside the batched projection
        wide[:, 640:640 + 2 * c].copy_(kv[:, :2 * c])
        sets.append((torch.empty_like(src), wide[:, 640:640 + c], wide[:, 640 + c:640 + 2 * c], torch.empty_like(src)))
    times, labels = {1: [], 0: []}, {}

    def launch(i, arm):
        q, k, v, o = sets[i]
        lib.ccedit_policy_set(b"attn_text", arm)
        q.copy_(src)                                                                        # the producer: q is freshly written, nothing else is cached
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.attention(q, k, v, heads, d, batches=frames, lq=lq, lk=L, kv_div=1, kv_per_frame=True, out=o)
        e1.record()
        labels[arm] = lib.ccedit_last_kernel().decode()
        return e0, e1
    try:
        for i in range(NB):                                                                 # warm-up: both arms on every set
            launch(i, 1), launch(i, 0)
        torch.cuda.synchronize()
        same = bool(torch.isfinite(sets[0][3].float()).all())
        evs = []
        for rep in range(reps):
            for i in range(NB):
                for arm in ((1, 0) if (rep + i) % 2 == 0 else (0, 1)):
                    evs.append((arm, launch(i, arm)))
        torch.cuda.synchronize()
        for arm, (e0, e1) in evs:
            times[arm].append(e0.elapsed_time(e1) * 1e3)
    finally:
        lib.ccedit_policy_set(b"attn_text", 1)

    def stats(ts):
        h = len(ts) // 2
        return dict(median_us=round(statistics.median(ts), 1), min_us=round(min(ts), 1), max_us=round(max(ts), 1),
                    first_half_median_us=round(statistics.median(ts[:h]), 1), second_half_median_us=round(statistics.median(ts[h:]), 1))
    return dict(d=d, rows=lq, frames=frames, keys=L, finite=same, arm=dict(kernel=labels[1], **stats(times[1])),
                general=dict(kernel=labels[0], **stats(times[0])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", type=str, default="")
    ap.add_argument("--skip_clips", action="store_true", help="only the kernels and the per-launch table")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/schedule_time.py measures on the GPU; none is visible")
    from ccedit_amd import ops, schedule
    dev = torch.device("cuda:0")
    res = dict(frames=N, frame_px=[8 * LH, 8 * LW], keyed=[f for f, _ in KEYS], ease="linear", steps=args.steps)

    g = torch.Generator().manual_seed(0)
    ctx = torch.randn(3, L, CTX, generator=g).to(dev)
    table = schedule.plan(KEYS, N, "linear")
    out = torch.empty(N, L, CTX, device=dev)
    res["prompt_schedule_us"] = round(event_us(lambda: ops.prompt_schedule(ctx, *table, out=out)), 2)
    res["prompt_schedule_mbytes"] = round(4 * (ctx.numel() + out.numel()) / 1e6, 2)

    # the four levels of the network, then further row counts for the arm's lower limit
    res["attention_levels"] = [attention_row(dev, d, lq, args.reps) for d, lq in ((40, 6144), (80, 1536), (160, 384), (160, 96))]
    res["attention_limit"] = [attention_row(dev, d, lq, args.reps) for d, lq in ((40, 1536), (40, 384), (40, 96), (80, 384), (80, 96))]
    torch.cuda.empty_cache()

    if not args.skip_clips:
        w = build(dev)
        net = w.diffusion_model
        for name, rows in (("text_kv_per_frame_us", 2 * N * L), ("text_kv_per_clip_us", 2 * L)):
            c2 = torch.randn(rows, CTX, generator=g).to(torch.bfloat16).to(dev)
            res[name] = dict(unet=round(event_us(lambda: net.text_kv(c2)), 1), controlnet=round(event_us(lambda: net.controlnet.text_kv(c2)), 1))
        res["plain"] = run_clip(w, dev, args.steps, False)
        res["schedule_clip"] = run_clip(w, dev, args.steps, True)
        res["plain_again"] = run_clip(w, dev, args.steps, False)         # the same arm after the other: the box's own drift
        w.reserve_windows(0)
        p, q, p2 = (res[k]["replay_median_ms"] for k in ("plain", "schedule_clip", "plain_again"))
        res["extra_ms_per_evaluation"] = round(q - (p + p2) / 2, 3) if p and q and p2 else None
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
