"""Every dispatch arm of ccedit_amd/csrc/norm.hip against ONE float64 reference (tests/_norm_ref.py; pinned on the CPU by
tests/test_norm_ref.py, which also shows that every case notices the mistakes its form can make).

Arms (tests/_norm_ref.py: CASES): temporal GroupNorm on the flat kernel <17> / <20> at the smallest grids that reach it (ragged last
workgroup, clip boundaries inside a workgroup, a one-pixel last workgroup), the same inputs on the cached kernel (gn_flat = 0), the
cached kernel on small grids (nsl 1 / 2 / 4, 48 lanes per slice, cpg < 8, C = 960 at the flat arm's size), the general two-sweep
kernel (T = 21, 32), sharded statistics + apply into halo-extended buffers; spatial GroupNorm on all five template arms of the
wave-per-row apply, the flat apply at RS = 1 and 8 around its 4096-row threshold, both entry points, the one-pass kernel at the last
sizes inside its bound and the first outside; LayerNorm and row_stats at 2 / 4 / 8 rows per wave with odd tails, and at three rows;
|mean| = 192 std on every arm that forms E[x^2] - mean^2 in fp32.

Every case asserts the kernel label, finite output, the error against the reference (2^-6 max|ref| + 1e-3; row_stats 1e-5 relative),
untouched guards around the outputs (0x5A5A) and untouched inputs (NaN around them), and identical bits on a second launch where the
arm has a fixed summation order.  The launches go to the C entry points directly: the wrappers of ccedit_amd/ops.py allocate their
own outputs, and the outputs here are views into guarded buffers.
"""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _norm_ref import BF, CASES, EPS, Case, check_case, dst_frames, inner  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _launcher(case: Case, variant: int, dev):
    from ccedit_amd import hip, ops
    lib = hip.lib()
    last = lambda: lib.ccedit_last_kernel().decode()          # noqa: E731
    stream = torch.cuda.current_stream().cuda_stream
    c, d, silu = case.c, case.dims, int(case.silu)

    def launch(p):
        xs = [b.to(dev) for b in p.xbufs]
        gbuf, bbuf = p.gbuf.to(dev), p.bbuf.to(dev)
        outs = [o.buf.to(dev) for o in p.outs]
        xv = [inner(x, shape) for x, shape in zip(xs, p.xshapes)]
        yv = [inner(o, out.shape) for o, out in zip(outs, p.outs)]
        g, b = inner(gbuf, (c,)), inner(bbuf, (c,))
        labels = []
        if case.op == "gt":
            hip.check(lib.ccedit_groupnorm_temporal(xv[0].data_ptr(), yv[0].data_ptr(), g.data_ptr(), b.data_ptr(), d["b"], d["t"], d["hw"], c,
                                                    EPS, silu, stream), "ccedit_groupnorm_temporal")
            labels.append(last())
        elif case.op == "gt2":
            # every shard: partial statistics; summed (the all-reduce); applied into a buffer with dst_off halo frames in front
            parts, stat_labels = [], set()
            for x, ts in zip(xv, d["shards"]):
                parts.append(ops.groupnorm_temporal_stats(x.view(d["b"] * ts, d["hw"], 1, c), d["b"], ts))
                stat_labels.add(last())
            stats = parts[0] + parts[1] + parts[2]
            apply_labels = set()
            for x, y, ts in zip(xv, yv, d["shards"]):
                ops.groupnorm_temporal_apply(x.view(d["b"] * ts, d["hw"], 1, c), stats, d["b"], ts, sum(d["shards"]), g, b, EPS, bool(silu),
                                             out=y.view(BF), dst_frames=dst_frames(case, ts), dst_off=d["dst_off"])
                apply_labels.add(last())
            labels = sorted(stat_labels, reverse=True) + sorted(apply_labels)
        elif case.op == "gs":
            x4 = xv[0].view(d["frames"], d["hw"], 1, c)
            if d["entry"] == "internal":
                ws = torch.empty(max(64 * d["frames"], 4096), dtype=torch.float64, device=dev)
                hip.check(lib.ccedit_groupnorm_spatial(x4.data_ptr(), yv[0].data_ptr(), g.data_ptr(), b.data_ptr(), ws.data_ptr(), d["frames"],
                                                       d["hw"], c, EPS, silu, stream), "ccedit_groupnorm_spatial")
                labels.append(last())
            else:
                st = ops.groupnorm_spatial_stats(x4)
                hip.check(lib.ccedit_groupnorm_spatial_apply(x4.data_ptr(), yv[0].data_ptr(), g.data_ptr(), b.data_ptr(), st.data_ptr(),
                                                             d["frames"], d["hw"], c, EPS, silu, stream), "ccedit_groupnorm_spatial_apply")
                labels.append(last())
                # the same through the wrapper: statistics attached by set_gn_stats
                y2 = ops.groupnorm_spatial(ops.set_gn_stats(x4, st), g, b, EPS, bool(silu))
                assert last() == labels[0] and torch.equal(y2.view(torch.int16).reshape(-1), yv[0].reshape(-1)), "set_gn_stats path differs"
        else:
            hip.check(lib.ccedit_layernorm(xv[0].data_ptr(), yv[0].data_ptr(), g.data_ptr(), b.data_ptr(), d["rows"], c, EPS, stream), "ccedit_layernorm")
            labels.append(last())
            hip.check(lib.ccedit_row_stats(xv[0].data_ptr(), yv[1].data_ptr(), d["rows"], c, EPS, stream), "ccedit_row_stats")
            labels.append(last())
        torch.cuda.synchronize()
        return [o.cpu() for o in outs], [t.cpu() for t in xs + [gbuf, bbuf]], labels

    def with_policy(p):
        saved = []
        try:
            for name, value in case.policies[variant]:
                old = ctypes.c_int32()
                assert lib.ccedit_policy_get(name.encode(), ctypes.byref(old)) == 0
                saved.append((name, old.value))
                assert lib.ccedit_policy_set(name.encode(), value) == 0
            return launch(p)
        finally:
            for name, value in saved:
                lib.ccedit_policy_set(name.encode(), value)

    return with_policy


@pytest.mark.parametrize("case", CASES, ids=lambda cs: cs.name)
def test_norm_arm(case: Case):
    dev = _dev()
    for variant in range(len(case.policies)):
        check_case(case, variant, _launcher(case, variant, dev))
