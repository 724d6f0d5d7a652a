"""Text cross-attention with K / V of its own for every frame (CCEDIT_ATTN_KV_PER_FRAME, kv_div = 1: a prompt schedule's per-frame
context) on a real MI355X, through the harness and the float64 reference of tests/test_attn_desc_gpu.py (tests/_attn_cases.py,
tests/_attn_ref.py) and with its tolerance, 2^-6 max|ref| + 4e-3.

The buffers are Gaussians seeded per element, so every batch's K / V differ: a kernel that reads frame 0's (or the clip's first) keys
for a later frame is off by the size of the result.  6 batches (2 clips x 3 frames).  The flag keeps the descriptor off the text arms
that stage K / V shared by a clip (attntext.hip, attntextlong.hip) — Lq = 2080 is where the shared arm would have claimed it
(kv_div * Lq >= 2048).  Where it was measured to win (d = 80, at least 1536 rows per frame) the descriptor takes attntext.hip's
per-frame arm, work split by frame, 320-channel group and row split; everything else — d = 40, d = 160, short frames, 154 keys — the
general kernel, which has always handled kv_div = 1; `ccedit_last_kernel` says which kernel ran.  The reference does not know the flag: it only selects a kernel.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _attn_cases import Case, build, check_case, tolerance  # noqa: E402
from _attn_ref import attn_ref  # noqa: E402

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
GENERAL = "attn_kernel"
FRAME = "attn_text_frame_kernel"          # attntext.hip's per-frame arm: d = 80, 64 <= Lk <= 96, at least 1536 rows per frame


def _cases():
    out = []
    for lq in (40, 2080):                                   # one partial 32-row tile; 65 tiles, the last one partial
        for lk in (64, 77, 96):
            out.append(Case(f"perframe-d40-{lq}x{lk}", GENERAL, 8, 40, dict(batches=6, lq=lq, lk=lk, kv_outer_rows=lk + 5)))
    out.append(Case("perframe-d80-72x77", GENERAL, 8, 80, dict(batches=6, lq=72, lk=77, kv_outer_rows=82)))     # two 320-channel groups
    out.append(Case("perframe-d160-72x77", GENERAL, 2, 160, dict(batches=6, lq=72, lk=77)))
    out.append(Case("perframe-d80-2080x154", GENERAL, 4, 80, dict(batches=6, lq=2080, lk=154)))                   # a two-chunk prompt
    # the arm: two groups, 6 frames -> 6 row splits of a frame; 1544 rows are 49 tiles (splits of 8 and 9, the last tile partial),
    # 1536 rows 48 tiles (8 each) and the smallest size the arm takes; one row fewer, or rows of a frame that are not contiguous, and
    # the general kernel runs
    for lk in (64, 77, 96):
        out.append(Case(f"perframe-d80-1544x{lk}", FRAME, 8, 80, dict(batches=6, lq=1544, lk=lk, kv_outer_rows=lk + 5)))
    out.append(Case("perframe-d80-1536x77", FRAME, 8, 80, dict(batches=6, lq=1536, lk=77)))
    out.append(Case("perframe-d80-1535x77", GENERAL, 8, 80, dict(batches=6, lq=1535, lk=77)))
    out.append(Case("perframe-d80-1544x77-one-group", FRAME, 4, 80, dict(batches=6, lq=1544, lk=77)))             # 6 workgroups' worth of frames: S = 6
    out.append(Case("perframe-d80-1540x77-gaps", GENERAL, 4, 80, dict(batches=6, lq=1540, lk=77, q_outer_rows=1543)))
    for i, cs in enumerate(out):
        cs.seed = 1000 + 10 * i
    return out


CASES = _cases()


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _launcher(case, dev, **flag):
    from ccedit_amd import hip, ops

    def launch(b):
        dq, dk, do = b.qbuf.to(dev), b.kbuf.to(dev), b.obuf.to(dev)
        dv = dk if b.vbuf is b.kbuf else b.vbuf.to(dev)
        ops.attention(dq[:, b.qcols], dk[:, b.kcols], dv[:, b.vcols], case.heads, case.d, out=do.view(BF)[:, b.ocols], **case.desc, **flag)
        label = hip.lib().ccedit_last_kernel().decode()
        torch.cuda.synchronize()
        return do.cpu(), dq.cpu(), dk.cpu(), dv.cpu(), label
    return launch


@pytest.mark.parametrize("case", CASES, ids=lambda cs: cs.name)
def test_per_frame_keys(case: Case):
    dev = _dev()
    check_case(case, _launcher(case, dev, kv_per_frame=True))


def test_the_flag_is_what_keeps_the_shared_arm_off():
    """Without the flag the same descriptor (kv_div = 1, 2080 rows) is the shared text arm's; the results agree within the bound."""
    dev = _dev()
    case = next(cs for cs in CASES if cs.name == "perframe-d40-2080x77")
    b = build(case)
    with_flag = _launcher(case, dev, kv_per_frame=True)(b)
    without = _launcher(case, dev)(b)
    assert with_flag[4] == "attn_kernel d=40" and without[4] == "attn_text_kernel d=40"
    ref, written = attn_ref(b.qbuf[:, b.qcols], b.kbuf[:, b.kcols], b.vbuf[:, b.vcols], case.heads, case.d, out=b.obuf.view(BF)[:, b.ocols],
                            **case.desc)
    for got in (with_flag[0], without[0]):
        assert ((got.view(BF)[:, b.ocols].double() - ref)[written].abs().max().item()) <= tolerance(ref[written])


@pytest.mark.parametrize("d, heads, lq, kernel", [(40, 8, 2080, GENERAL), (80, 8, 72, GENERAL), (80, 8, 1544, FRAME)])
def test_keys_repeated_per_frame_give_what_shared_keys_give(d, heads, lq, kernel):
    """The same K / V for the 3 frames of each of 2 clips, once shared (kv_div = 3) and once laid out per frame (kv_div = 1 and the
    flag): both within the bound of ONE float64 reference."""
    dev = _dev()
    from ccedit_amd import hip, ops
    lk, c = 77, heads * d
    g = torch.Generator().manual_seed(40 + d)
    q = torch.randn(6 * lq, c, generator=g).to(BF)
    kv = torch.randn(2 * lk, 2 * c, generator=g).to(BF)
    kv_rep = kv.view(2, 1, lk, 2 * c).expand(2, 3, lk, 2 * c).reshape(6 * lk, 2 * c).contiguous()
    ref, written = attn_ref(q, kv[:, :c], kv[:, c:], heads, d, batches=6, lq=lq, lk=lk, kv_div=3)
    assert bool(written.all())
    dq, dkv, dkr = q.to(dev), kv.to(dev), kv_rep.to(dev)
    shared = ops.attention(dq, dkv[:, :c], dkv[:, c:], heads, d, batches=6, lq=lq, lk=lk, kv_div=3)
    label_shared = hip.lib().ccedit_last_kernel().decode()
    per_frame = ops.attention(dq, dkr[:, :c], dkr[:, c:], heads, d, batches=6, lq=lq, lk=lk, kv_div=1, kv_per_frame=True)
    label_pf = hip.lib().ccedit_last_kernel().decode()
    lim = tolerance(ref)
    e_s = (shared.cpu().double() - ref).abs().max().item()
    e_p = (per_frame.cpu().double() - ref).abs().max().item()
    print(f"[attn-perframe] d={d} lq={lq}: shared ({label_shared}) max err {e_s:.4g}, per frame ({label_pf}) {e_p:.4g}, limit {lim:.4g}")
    assert label_pf == f"{kernel} d={d}"
    assert e_s <= lim and e_p <= lim


def test_the_flag_needs_kv_div_1():
    dev = _dev()
    from ccedit_amd import hip
    from ccedit_amd.hip import CcAttnDesc
    import ctypes as C
    q = torch.zeros(6 * 40, 320, dtype=BF, device=dev)
    kv = torch.zeros(6 * 77, 640, dtype=BF, device=dev)
    a = CcAttnDesc()
    a.q, a.k, a.v, a.o = q.data_ptr(), kv.data_ptr(), kv[:, 320:].data_ptr(), q.data_ptr()
    a.ldq, a.ldk, a.ldv, a.ldo = 320, 640, 640, 320
    a.heads, a.d, a.batches, a.Lq, a.Lk = 8, 40, 6, 40, 77
    a.q_inner, a.q_outer_rows, a.q_seq_rows, a.kv_div, a.kv_inner, a.kv_outer_rows, a.kv_seq_rows = 1, 40, 1, 3, 1, 77, 1
    a.scale, a.flags = 40 ** -0.5, hip.ATTN_KV_PER_FRAME
    assert hip.lib().ccedit_attention(C.byref(a), None) == -1
    assert b"CCEDIT_ATTN_KV_PER_FRAME needs kv_div == 1, got 3" in hip.lib().ccedit_last_error()
