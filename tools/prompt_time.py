#!/usr/bin/env python3
"""What long prompts cost (ccedit_amd/prompt.py, csrc/prompt.hip, csrc/attntextlong.hip), everything in ONE process on one box, HIP events,
median of 20 after three warm-up calls, three alternating rounds per comparison:
  attention  the text cross-attention launches of production (34 frames = 17 keyframes x 2 CFG halves, two clips' K / V; 6144 query rows
             per frame at d = 40 x 8 heads, 1536 at d = 80 x 8 heads) for Lk = 154 / 231 / 308: the long text arm against the same
             launch with policy attn_text = 0 (the kernel that served it before the arm: its label is reported).  Per (d, Lk): the
             three medians of each arm, the medians of those, the spread between the rounds (max - min of an arm's rounds, the larger of
             the two arms) and `wins` = the arm's median is below the other's by more than that spread
  network    one evaluation of the full-width network at 17 x 512 x 768 (CFG-doubled, replayed graph) with a context of n x 77 rows,
             n = 1, 2, 3, 4
  weight     ccedit_prompt_weight on (2, 77 n, 768), n = 1 and 4, half of the weights 1
Prints one JSON line (and writes it to --out).
  python tools/prompt_time.py [--skip-network] [--out FILE]"""
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

N, LH, LW, CTX = 17, 64, 96, 768          # frames, the latent, text width
LAUNCHES = ((40, 8, 6144), (80, 8, 1536))            # (d, heads, query rows per frame) of the 64 x 96 and the 32 x 48 level
KEYS = (154, 231, 308)
BF = torch.bfloat16


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


def attention_rows(dev):
    from ccedit_amd import hip, ops
    lib = hip.lib()
    out = []
    for d, heads, lq in LAUNCHES:
        c, frames, clips = heads * d, 2 * N, 2
        g = torch.Generator().manual_seed(d)
        q = torch.randn(frames * lq, c, generator=g).to(BF).to(dev)
        o = torch.empty_like(q)
        for lk in KEYS:
            kv = torch.randn(clips * lk, 2 * c, generator=g).to(BF).to(dev)

            def launch():
                ops.attention(q, kv[:, :c], kv[:, c:], heads, d, batches=frames, lq=lq, lk=lk, kv_div=N, out=o)
            arm, other, names = [], [], {}
            for _ in range(3):                                     # alternating rounds: the box's drift lands on both arms
                for value, ts, key in ((1, arm, "arm"), (0, other, "other")):
                    assert lib.ccedit_policy_set(b"attn_text", value) == 0
                    try:
                        ts.append(round(event_us(launch), 2))
                        names[key] = lib.ccedit_last_kernel().decode()
                    finally:
                        lib.ccedit_policy_set(b"attn_text", 1)
            ma, mo = statistics.median(arm), statistics.median(other)
            spread = max(max(arm) - min(arm), max(other) - min(other))
            out.append(dict(d=d, heads=heads, rows_per_frame=lq, frames=frames, keys=lk, arm=names["arm"], other=names["other"], arm_us=arm,
                            other_us=other, arm_median_us=ma, other_median_us=mo, spread_us=round(spread, 2), wins=bool(mo - ma > spread)))
    return out


def weight_rows(dev):
    from ccedit_amd import ops
    out = []
    for n in (1, 4):
        g = torch.Generator().manual_seed(n)
        z, e = torch.randn(2, 77 * n, CTX, generator=g).to(dev), torch.randn(77, CTX, generator=g).to(dev)
        w = torch.where(torch.rand(2, 77 * n, generator=g) < 0.5, torch.tensor(1.0), torch.tensor(1.3)).to(dev)
        us = event_us(lambda: ops.prompt_weight(z, e, w))          # (the wrapper's finiteness check and its read-back included)
        out.append(dict(chunks=n, us=round(us, 2), mbytes=round(4 * (2 * z.numel() + e.numel() + w.numel()) / 1e6, 3)))
    return out


def network_rows(dev):
    from ccedit_amd import hip
    from ccedit_amd.sgm_compat import build_network
    from ccedit_amd.utils.synth import fill_module_
    hip.lib()
    w = build_network(dev)
    fill_module_(w, prefix="model.")
    w.diffusion_model.pack(dev)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(1, 4, N, LH, LW, generator=g).repeat(2, 1, 1, 1, 1).to(dev)
    t = torch.tensor([500, 500], dtype=torch.int64, device=dev)
    low = torch.rand(1, 1, N, LH // 4, LW // 4, generator=g)
    hint = torch.nn.functional.interpolate(low, size=(N, 8 * LH, 8 * LW), mode="trilinear", align_corners=False)
    hint = (hint * 2 - 1).repeat(2, 3, 1, 1, 1).contiguous().to(dev)
    ctxs = {n: torch.randn(2, 77 * n, CTX, generator=g).to(dev) for n in (1, 2, 3, 4)}
    rounds = {n: [] for n in ctxs}
    for _ in range(3):
        for n, ctx in ctxs.items():
            c = dict(crossattn=ctx, control_hint=hint)
            w.reset_caches()
            rounds[n].append(round(event_us(lambda: w(x, t, c), reps=20, warm=3) / 1e3, 3))          # eager, capture, replay, then replays
    return [dict(chunks=n, context_rows=77 * n, ms=v, median_ms=statistics.median(v), counts=dict(w.graph_counts or {})) for n, v in rounds.items()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-network", action="store_true")
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/prompt_time.py measures on the GPU; none is visible")
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    res = dict(frames=N, frame_px=[8 * LH, 8 * LW])
    res["attention"] = attention_rows(dev)
    res["weight"] = weight_rows(dev)
    if not args.skip_network:
        res["network"] = network_rows(dev)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
