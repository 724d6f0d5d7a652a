"""g8_kernel's K loop on 32x32x16 MFMAs (policy g8_mfma16 = 0) against 16x16x32 (= 2: every arm), on every distinct g8 launch shape of
one network evaluation: same process, alternating arms, three rounds, rotating cold operands (each timed launch reads an activation
another launch's worth of traffic ago), full-range random data.  The shape list is read from the per-shape rows `bench.py --full --breakdown` prints (default:
profiles/g8_mfma16_shapes.txt, the g8 rows of one such run):

    CCEDIT_BREAKDOWN_ROWS=400 python bench.py --gpus 1 --steps 3 --warmup 2 --full --breakdown --no-cpu-baseline --no-clip --no-tvi2v --no-c4 2> breakdown.txt
    python tools/exp/g8_mfma_ab.py breakdown.txt

A row is "tap_gemm (kind, M, N, K, stride, residuals, act) x launches  ms  TF/s  kernel".  What it does not carry is rebuilt from the bench geometry: 34 frames
(CFG-doubled 17), frames of 2:3 aspect, clips of T = 17; row bias and fused statistics are left out (epilogue extras of a few percent
of a launch, the same for both arms).  Prints median and min per arm and shape, the class sums weighted by launches per step, and
the total."""
import ast, ctypes, os, re, socket, statistics, sys
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..")))
import torch
from ccedit_amd import hip, ops
from ccedit_amd.packing import fold_layernorm, pack_upsample_parities, pack_weight

BF = torch.bfloat16
FRAMES, T = 34, 17
ROUNDS, NBUF, REPS = 3, 3, 4
lib = hip.lib()


def geometry(m):
    for nf in (FRAMES, T):          # the CFG-doubled batch, or one half of it
        hw = m // nf
        h = int(round((hw * 2 / 3) ** 0.5))
        if nf * hw == m and 2 * hw == 3 * h * h:
            return nf, h, 3 * h // 2
    raise ValueError(f"M = {m}: not 34 or 17 frames of 2:3 aspect")


def build(kind, m, n, k, nres, act, kernel):
    """-> (label class, launch(i) on buffer set i)."""
    tile = 13 if "128ch x 512pix" in kernel else 12
    split = "split-K" in kernel
    if split:
        tile = 0          # split-K is chosen by the automatic dispatch when the workspace is lent
    res = [[torch.randn(m, n, device="cuda").to(BF) for _ in range(NBUF)] for _ in range(nres)]
    kw = lambda i: dict(res1=res[0][i] if nres > 0 else None, res2=res[1][i] if nres > 1 else None, tile=tile)
    if kind == "lin":
        a = [torch.randn(m, k, device="cuda").to(BF) for _ in range(NBUF)]
        geglu = act == hip.ACT_GEGLU
        w, b = torch.randn(n, k) * k ** -0.5, torch.randn(n)
        if "LayerNorm folded" in kernel:
            pw = fold_layernorm([w], [b], torch.rand(k) + 0.5, torch.randn(k) * 0.1, geglu=geglu).to("cuda")
            st = [ops.row_stats(x, 1e-5) for x in a]
            return "LayerNorm folded", lambda i: ops.linear(a[i], pw, ln_stats=st[i], tile=tile)
        pw = pack_weight(w, b, geglu=geglu).to("cuda")
        return ("split-K" if split else ("GEGLU" if geglu else "linear")), lambda i: ops.linear(a[i], pw, **kw(i))
    nf, h, wd = geometry(m)
    if kind == "temp":
        cin = k // 3
        a = [torch.randn(nf, h, wd, cin, device="cuda").to(BF) for _ in range(NBUF)]
        pw = pack_weight(torch.randn(n, cin, 3) * k ** -0.5, torch.randn(n)).to("cuda")
        return ("split-K" if split else "temporal taps"), lambda i: ops.conv_temporal(a[i], T, pw, **kw(i))
    if kind == "conv+up(parity)":
        cin = k // 4          # (the dump's K is that of the packed 2 x 2 window)
        a = [torch.randn(nf, h, wd, cin, device="cuda").to(BF) for _ in range(NBUF)]
        pws = pack_upsample_parities(torch.randn(n, cin, 3, 3) * (9 * cin) ** -0.5, torch.randn(n), device="cuda")
        return ("split-K" if split else "parity taps (4 launches)"), lambda i: ops.conv2d_upsampled(a[i], pws, tile=tile)
    assert kind == "conv", kind
    cin = k // 9
    a = [torch.randn(nf, h, wd, cin, device="cuda").to(BF) for _ in range(NBUF)]
    pw = pack_weight(torch.randn(n, cin, 3, 3) * k ** -0.5, torch.randn(n)).to("cuda")
    return ("split-K" if split else "3x3 taps"), lambda i: ops.conv2d(a[i], pw, **kw(i))


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(__file__), "..", "..", "profiles", "g8_mfma16_shapes.txt")
    shapes = {}
    for line in open(path):
        mt = re.match(r"tap_gemm\s+(\(.*?\))\s+x\s*(\d+)\s+[\d.]+ ms\s+[\d.]+ TF/s\s+(g8_kernel.*?)\s*$", line)
        if mt:
            key = tuple(ast.literal_eval(mt.group(1))) + (mt.group(3),)
            shapes[key] = shapes.get(key, 0) + int(mt.group(2))
    assert shapes, f"{path}: no g8_kernel rows"
    print(f"box {socket.gethostname()}: {torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs", flush=True)
    found = ctypes.c_int32(0)
    assert lib.ccedit_policy_get(b"g8_mfma16", ctypes.byref(found)) == 0
    parity_seen = set()
    tot, cls_tot = {0: 0.0, 2: 0.0}, {}
    for key, cnt in sorted(shapes.items(), key=lambda kv: kv[0]):
        kind, m, n, k, _stride, nres, act, kernel = key[0], int(key[1]), int(key[2]), int(key[3]), key[4], int(key[5]), int(key[6]), key[7]
        per_call = 1
        if kind == "conv+up(parity)":          # the dump has one row per parity launch; the tool launches the four together
            if (m, n, k) in parity_seen:
                continue
            parity_seen.add((m, n, k))
            cnt = sum(c for kk, c in shapes.items() if kk[0] == kind and (int(kk[1]), int(kk[2]), int(kk[3])) == (m, n, k))
            per_call = 4
        cls, launch = build(kind, m, n, k, nres, act, kernel)
        t = {0: [], 2: []}
        names = {}
        for rnd in range(ROUNDS):
            for arm in (0, 2):
                assert lib.ccedit_policy_set(b"g8_mfma16", arm) == 0
                for i in range(NBUF):
                    launch(i)
                names[arm] = lib.ccedit_last_kernel().decode()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for rep in range(REPS):
                    for i in range(NBUF):
                        launch(i)
                e1.record()
                torch.cuda.synchronize()
                t[arm].append(e0.elapsed_time(e1) * 1e3 / (REPS * NBUF * per_call))
        lib.ccedit_policy_set(b"g8_mfma16", found.value)
        assert "g8_kernel" in names[0] and names[0] == names[2], names
        med = {a: statistics.median(v) for a, v in t.items()}
        c = cls_tot.setdefault((cls, "128x512" if "128ch" in kernel else "256x256"), {0: 0.0, 2: 0.0, "n": 0})
        c["n"] += cnt
        for a in (0, 2):
            tot[a] += cnt * med[a]
            c[a] += cnt * med[a]
        print(f"{kind:16s} M={m:6d} N={n:5d} K={k:6d} res={nres} x{cnt:3d} | 32x32x16 med {med[0]:8.1f} min {min(t[0]):8.1f} us | 16x16x32 med {med[2]:8.1f} "
              f"min {min(t[2]):8.1f} us | ratio {med[2] / med[0]:.4f} | {names[2]}", flush=True)
    print("per class, weighted by launches per step (median):")
    for (cls, shape), c in sorted(cls_tot.items()):
        print(f"  {cls:26s} {shape}  x{c['n']:3d}: 32x32x16 {c[0] / 1e3:7.3f} ms, 16x16x32 {c[2] / 1e3:7.3f} ms, ratio {c[2] / c[0]:.4f}")
    print(f"all g8 launches of a step: 32x32x16 {tot[0] / 1e3:.3f} ms, 16x16x32 {tot[2] / 1e3:.3f} ms, difference {(tot[2] - tot[0]) / 1e3:+.3f} ms")


if __name__ == "__main__":
    main()
