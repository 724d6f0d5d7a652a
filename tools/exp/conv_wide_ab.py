"""3x3 stride-1 convs of the 64x96 / 32x48 levels on the LDS-halo kernel: 128-pixel tiles (policy conv_wide = 0) against 256-pixel tiles
(conv_wide = 2), same process, alternating rounds, rotating (cold) inputs; the two must give the same bits (same k-step order per
accumulator).  Every distinct conv_halo shape of the step, the 17-frame launches of the shared CFG prefix included; `cnt` = launches per
step (0: listed for the dispatch rule only).  Output: profiles/conv_wide_ab.txt."""
import sys, os
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..")))
import torch
from ccedit_amd import hip, ops
from ccedit_amd.packing import pack_weight
lib = hip.lib()
tot = {0: 0.0, 2: 0.0}
for n, h, w, cin, cout, cnt in ((34, 64, 96, 320, 320, 14), (34, 64, 96, 640, 320, 2), (34, 64, 96, 960, 320, 1), (34, 32, 48, 320, 640, 2),
                                (34, 32, 48, 640, 640, 9), (34, 32, 48, 960, 640, 1), (34, 32, 48, 1280, 640, 1), (34, 32, 48, 1920, 640, 1),
                                (17, 64, 96, 320, 320, 0), (17, 32, 48, 320, 640, 0), (17, 32, 48, 640, 640, 0)):
    pw = pack_weight(torch.randn(cout, cin, 3, 3) * (9 * cin) ** -0.5, torch.randn(cout)).to("cuda")
    a = [torch.randn(n, h, w, cin, device="cuda").to(torch.bfloat16) for _ in range(3)]
    res, outs, label = {}, {}, {}
    for rnd in range(3):
        for pol in (0, 2):
            lib.ccedit_policy_set(b"conv_wide", pol)
            for x in a:
                y = ops.conv2d(x, pw)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for rep in range(4):
                for x in a:
                    y = ops.conv2d(x, pw)
            e1.record()
            torch.cuda.synchronize()
            res.setdefault(pol, []).append(e0.elapsed_time(e1) * 1e3 / 12)
            outs[pol], label[pol] = y, lib.ccedit_last_kernel().decode()
    lib.ccedit_policy_set(b"conv_wide", 1)
    same = torch.equal(outs[0], outs[2])
    fl = 2.0 * n * h * w * cin * 9 * cout
    b0, b2 = min(res[0]), min(res[2])
    tot[0] += cnt * b0; tot[2] += cnt * b2
    wgs = n * (h // 16) * ((w + 15) // 16) * ((cout + 127) // 128)
    print(f"{n}x{h}x{w} {cin}->{cout} x{cnt}: 128-pixel {b0:8.1f} us (spread {max(res[0]) - b0:5.1f}) {fl / b0 / 1e6:7.1f} TF/s | 256-pixel {b2:8.1f} us "
          f"(spread {max(res[2]) - b2:5.1f}) {fl / b2 / 1e6:7.1f} TF/s | ratio {b2 / b0:.4f} | {wgs} wide workgroups | same bits {same} | {label[0]} / {label[2]}",
          flush=True)
print(f"weighted by launches per step: 128-pixel {tot[0] / 1e3:.2f} ms, 256-pixel {tot[2] / 1e3:.2f} ms")
