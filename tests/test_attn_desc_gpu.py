"""ccedit_attention's descriptor forms that network.py launches and no single-GPU test reached, each against ONE float64
reference that interprets the descriptor (tests/_attn_ref.py; pinned on the CPU by tests/test_attn_ref.py, which also shows that
every case notices the address mistake it is there for).

Forms (tests/_attn_cases.py): the anchor frame appended after the frames (seg1_mul = 1, seg1_add = frames: run_frames, keyframes
sharded) on the general and the spatial kernel; temporal attention with Lq != Lk (run_temporal, frames sharded) on the short kernel
and, past its prefetch bound, on the general one; row-sharded spatial attention with q in log2 units (Lk = world * Lq); the
head-sharded call (1 or 2 heads, 1 or 3 batches: the grid rounded up to 8 with early-returning workgroups, both block orders); the
text kernel and the other three writing into a column slice (ldo != heads * d) with ragged Lq and guard rows; d = 16.

Every case runs through one harness.  q, k, v and out are column slices of wider, longer buffers; what the descriptor does not
address is bf16 NaN on the input side (production buffers are torch.empty: a kernel may load such memory — pad granules, whole
320-channel rows, rows of a neighbouring clip — but may not let it reach the result, not even as 0 * NaN) and a fixed bit pattern
on the output side, which must survive the launch bit for bit.  Tolerance: that of the attention tests of tests/test_ops_gpu.py,
2^-6 max|ref| + 4e-3, whose sensitivity to a dropped, duplicated or mis-paired key those tests' docstrings and the defect table show.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _attn_cases import CASES, Case, check_case  # noqa: E402

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.mark.parametrize("case", CASES, ids=lambda cs: cs.name)
def test_descriptor_form(case: Case):
    dev = _dev()
    from ccedit_amd import hip, ops

    def launch(b):
        dq, dk, do = b.qbuf.to(dev), b.kbuf.to(dev), b.obuf.to(dev)
        dv = dk if b.vbuf is b.kbuf else b.vbuf.to(dev)
        ops.attention(dq[:, b.qcols], dk[:, b.kcols], dv[:, b.vcols], case.heads, case.d, out=do.view(BF)[:, b.ocols], **case.desc)
        label = hip.lib().ccedit_last_kernel().decode()
        torch.cuda.synchronize()
        return do.cpu(), dq.cpu(), dk.cpu(), dv.cpu(), label

    check_case(case, launch)
