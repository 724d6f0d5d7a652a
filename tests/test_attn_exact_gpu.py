"""The five attention kernels against an exact reference, element by element.

tests/_attn_exact.py puts q, k, v on an integer grid with a softmax scale of exactly one log2 unit (CCEDIT_ATTN_Q_LOG2, or
scale = float32(ln 2) through the `scale` keyword of ops.attention): every score is an integer, every probability and every rescale
factor a power of two, every partial sum exact in fp32 in any order.  What a kernel still rounds is 1.0f / l, o * inv and the bf16
store, so for EVERY addressed element

    |got - ref| <= 2^-17 |ref| + 1/2 ulp_bf16(|ref| (1 + 2^-17)),        +-0 where ref == 0,

with ref one float64 division of two exactly known integers; in rows whose denominator is a power of two the output equals
bf16_rne(ref) bit for bit.  Against `2^-6 max|ref| + 4e-3` over the whole tensor (tests/test_ops_gpu.py, tests/test_attn_desc_gpu.py)
this notices one dropped, doubled or padded key, a missed rescale of one accumulator tile, a wrong denominator, a flush of small
probabilities and a store that does not round to nearest even — tests/test_attn_exact_ref.py plants each of them.

Cases: the smallest shape that reaches each arm of attn_kernel (every head dim, 1 / 4 / 8 waves, single buffer and ring, masked
tail, both block orders, causal, two segments, the short and text layouts under policy 0), attn_spatial_kernel (d 40 / 80, the
optimistic and the tracked reference, both PV products, masked tail, leading segment, ragged Lq), attn_short_kernel and
attn_text_kernel; each plain, shifted by -24 (a key of the zero page, score 0, would take the row over), with spiked rows (one
group of keys 2^190 above the rest: everything else underflows; on the spatial kernel the optimistic pass overflows and the
workgroup runs again) and, where Lk > 128, as a staircase that raises every row's maximum in every key tile.  The harness rules of
tests/_attn_cases.py hold: slices of wider buffers, NaN off the read masks, 0x5A5A off the written mask, inputs unchanged, the
kernel label, a second launch bit-identical.
"""
import os
import sys
import time

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _attn_exact import CASES, check_exact  # noqa: E402

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
STATS = {}
T0 = time.time()


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.mark.parametrize("case", CASES, ids=lambda cs: cs.name)
def test_exact(case):
    dev = _dev()
    from ccedit_amd import hip, ops
    lib = hip.lib()

    def launch(b, desc, policy):
        dq, dk, do = b.qbuf.to(dev), b.kbuf.to(dev), b.obuf.to(dev)
        dv = dk if b.vbuf is b.kbuf else b.vbuf.to(dev)
        try:
            for name, value in policy.items():
                assert lib.ccedit_policy_set(name.encode(), value) == 0
            ops.attention(dq[:, b.qcols], dk[:, b.kcols], dv[:, b.vcols], case.heads, case.d, out=do.view(BF)[:, b.ocols], **desc)
            label = lib.ccedit_last_kernel().decode()
        finally:
            for name in policy:
                lib.ccedit_policy_set(name.encode(), 1)          # every attention switch defaults to 1 (CcPolicy, common.h)
        torch.cuda.synchronize()
        return do.cpu(), dq.cpu(), dk.cpu(), dv.cpu(), label

    check_exact(case, launch, STATS)


def test_summary():
    """Per kernel, over the cases that ran in this process: the figures DESIGN.md 5.3 records."""
    _dev()
    for kernel, st in sorted(STATS.items()):
        print(f"[attn-exact-summary] {kernel}: {st['launches']} launches, {st['elements']} elements; worst |err| / bound {st['worst']:.4f}; "
              f"largest (|err| - ulp/2) / |ref| {st['excess']:.3e} ({'<=' if st['excess'] <= 2.0 ** -23 else '>'} 2^-23); "
              f"elements differing from bf16_rne(ref) {st['differ']}")
    print(f"[attn-exact-summary] {sum(st['launches'] for st in STATS.values())} launches in {time.time() - T0:.1f} s")
