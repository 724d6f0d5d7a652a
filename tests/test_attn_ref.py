"""tests/_attn_ref.py pinned without a GPU, so that a wrong reference cannot hide a wrong kernel.

1. On the five layouts that tests/test_ops_gpu.py builds by hand (plain, fused qkv slices, kv_div, temporal, anchor + self; the
   constructions are copied at reduced sizes) the descriptor-interpreting reference equals float64 F.scaled_dot_product_attention
   to 1e-12, and its written / read masks have exactly the expected population.
2. Every case of tests/test_attn_desc_gpu.py builds, addresses only memory inside its buffers, and names the kernel that the
   applicability rules select.
3. A defect table in the manner of tests/test_exact_host.py: the natural mistake for each new descriptor form, made in a copy of
   the address rule, moves the result of every case of that form by at least 4x the tolerance the GPU test asserts — on that case's
   own inputs.  (The unaddressed memory holds Gaussians instead of NaN here, so that a read that goes astray gives a number.)
"""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _attn_cases import BF, CASES, EXTRA_ROWS, LOG2E, Case, build, check_case, expected_kernel, tolerance  # noqa: E402
from _attn_ref import Rules, attn_read_masks, attn_ref  # noqa: E402
from test_ops_gpu import _rnd, _sdpa_ref  # noqa: E402      (the hand-built references, verbatim)

HEADS, D = 2, 40
C = HEADS * D


def _same(got, ref):
    assert got.dtype == torch.float64 and got.shape == ref.shape
    assert (got - ref).abs().max().item() <= 1e-12, (got - ref).abs().max().item()


def test_plain_layout_with_spare_rows():
    b, lq, lk = 3, 50, 33
    q, k, v = _rnd(b, lq, C, seed=1).double(), _rnd(b, lk, C, seed=2).double(), _rnd(b, lk, C, seed=3).double()
    spare = torch.full((4, C), float("nan"), dtype=torch.float64)
    q2, k2, v2 = torch.cat([q.reshape(-1, C), spare]), torch.cat([k.reshape(-1, C), spare]), torch.cat([v.reshape(-1, C), spare])
    o, written = attn_ref(q2, k2, v2, HEADS, D, batches=b, lq=lq, lk=lk)
    _same(o[:b * lq].reshape(b, lq, C), _sdpa_ref(q, k, v, HEADS))
    assert o.shape == (b * lq + 4, C) and written[:b * lq].all() and not written[b * lq:].any() and (o[b * lq:] == 0).all()
    mq, mk, mv = attn_read_masks(q2.shape, k2.shape, v2.shape, HEADS, D, batches=b, lq=lq, lk=lk)
    assert (int(mq.sum()), int(mk.sum()), int(mv.sum()), int(written.sum())) == (b * lq * C, b * lk * C, b * lk * C, b * lq * C)
    assert not mq[b * lq:].any() and not mk[b * lk:].any() and not mv[b * lk:].any()


def test_fused_qkv_slices():
    n, lq = 4, 24
    qkv = _rnd(n * lq, 3 * C, seed=1).double()
    kw = dict(batches=n, lq=lq, lk=lq)
    o, written = attn_ref(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], HEADS, D, **kw)
    _same(o.reshape(n, lq, C), _sdpa_ref(qkv[:, :C].reshape(n, lq, C), qkv[:, C:2 * C].reshape(n, lq, C), qkv[:, 2 * C:].reshape(n, lq, C), HEADS))
    masks = attn_read_masks((n * lq, C), (n * lq, C), (n * lq, C), HEADS, D, **kw)
    assert written.all() and all(m.all() for m in masks)
    # one head of two: half the columns of every view, none of the other head's
    o1, w1 = attn_ref(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], 1, D, **kw)
    assert int(w1.sum()) == n * lq * D and w1[:, :D].all() and torch.equal(o1[:, :D], o[:, :D])


def test_text_kv_shared_by_the_frames_of_a_clip():
    fpc, clips, lq, lk = 3, 2, 24, 11
    n = clips * fpc
    q = _rnd(n, lq, C, seed=2).double()
    kv = torch.cat([_rnd(clips * lk, 2 * C, seed=3).double(), torch.full((2, 2 * C), float("nan"), dtype=torch.float64)])
    kw = dict(batches=n, lq=lq, lk=lk, kv_div=fpc)
    o, written = attn_ref(q.reshape(-1, C), kv[:, :C], kv[:, C:], HEADS, D, **kw)
    kk = kv[:clips * lk, :C].reshape(clips, lk, C).repeat_interleave(fpc, 0)
    vv = kv[:clips * lk, C:].reshape(clips, lk, C).repeat_interleave(fpc, 0)
    _same(o.reshape(n, lq, C), _sdpa_ref(q, kk, vv, HEADS))
    mq, mk, mv = attn_read_masks((n * lq, C), kv[:, :C].shape, kv[:, C:].shape, HEADS, D, **kw)
    assert written.all() and mq.all() and int(mk.sum()) == int(mv.sum()) == clips * lk * C and not mk[clips * lk:].any()


def test_temporal_rows_a_frame_apart():
    clips, hw, t = 2, 5, 4
    x = _rnd(clips * t * hw, 3 * C, seed=1).double()        # rows ordered (clip, frame, pixel)
    kw = dict(batches=clips * hw, lq=t, lk=t, q_inner=hw, q_outer_rows=t * hw, q_inner_rows=1, q_seq_rows=hw,
              kv_inner=hw, kv_outer_rows=t * hw, kv_inner_rows=1, kv_seq_rows=hw)
    o, written = attn_ref(x[:, :C], x[:, C:2 * C], x[:, 2 * C:], HEADS, D, **kw)
    xs = x.reshape(clips, t, hw, 3 * C).permute(0, 2, 1, 3).reshape(clips * hw, t, 3 * C)
    ref = _sdpa_ref(xs[..., :C], xs[..., C:2 * C], xs[..., 2 * C:], HEADS)
    _same(o, ref.reshape(clips, hw, t, C).permute(0, 2, 1, 3).reshape(clips * t * hw, C))
    assert written.all() and all(m.all() for m in attn_read_masks(*[(clips * t * hw, C)] * 3, HEADS, D, **kw))


def test_anchor_and_self_keys():
    t, clips, hw = 3, 2, 20
    n = clips * t
    q = _rnd(n, hw, C, seed=1).double()
    kv = _rnd(n, hw, 2 * C, seed=2).double()
    kv2 = kv.reshape(-1, 2 * C)
    kw = dict(batches=n, lq=hw, lk=2 * hw, kv_outer_rows=hw, seg1_len=hw, seg1_div=t, seg1_mul=t, seg1_add=t // 2)
    o, written = attn_ref(q.reshape(-1, C), kv2[:, :C], kv2[:, C:], HEADS, D, **kw)
    anchor = kv.reshape(clips, t, hw, 2 * C)[:, t // 2].repeat_interleave(t, 0)
    ctx = torch.cat([anchor, kv], dim=1)
    _same(o.reshape(n, hw, C), _sdpa_ref(q, ctx[..., :C], ctx[..., C:], HEADS))
    mq, mk, mv = attn_read_masks((n * hw, C), (n * hw, C), (n * hw, C), HEADS, D, **kw)
    assert written.all() and mq.all() and mk.all() and mv.all()
    # the anchor frames alone (no own keys: Lk = seg1_len) read one frame per clip
    kw.update(lk=hw)
    _, mk, _ = attn_read_masks((n * hw, C), (n * hw, C), (n * hw, C), HEADS, D, **kw)
    assert int(mk.sum()) == clips * hw * C and mk[hw:2 * hw].all() and not mk[:hw].any()


def test_causal_and_log2_scores():
    b, l = 2, 37
    q, k, v = _rnd(b * l, C, seed=1).double(), _rnd(b * l, C, seed=2).double(), _rnd(b * l, C, seed=3).double()
    qq, kk, vv = (t.view(b, l, HEADS, D).transpose(1, 2) for t in (q, k, v))
    ref = F.scaled_dot_product_attention(qq, kk, vv, is_causal=True).transpose(1, 2).reshape(b * l, C)
    _same(attn_ref(q, k, v, HEADS, D, batches=b, lq=l, lk=l, causal=True)[0], ref)
    plain = attn_ref(q, k, v, HEADS, D, batches=b, lq=l, lk=l)[0]
    _same(attn_ref(q * (D ** -0.5 * LOG2E), k, v, HEADS, D, batches=b, lq=l, lk=l, q_log2=True)[0], plain)
    with pytest.raises(AssertionError):
        attn_ref(q, k, v, HEADS, D, batches=b + 1, lq=l, lk=l)          # a descriptor that leaves the view is refused, not wrapped


# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda cs: cs.name)
def test_gpu_case_is_well_formed(case: Case):
    """The buffers of a GPU case: every addressed element inside them (attn_read_masks asserts it), exactly the unaddressed input
    elements NaN, slices and strides on the 16-byte grid, and the intended kernel the one the applicability rules select."""
    assert expected_kernel(case) == case.kernel
    b = build(case)
    r = Rules(case.heads, case.d, **case.desc)
    c = case.heads * case.d
    q, k, v = b.qbuf[:, b.qcols], b.kbuf[:, b.kcols], b.vbuf[:, b.vcols]
    mq, mk, mv = attn_read_masks(q.shape, k.shape, v.shape, case.heads, case.d, **case.desc)
    assert int(mq.sum()) == r.batches * r.lq * c
    assert not mq[-EXTRA_ROWS:].any() and not mk[-EXTRA_ROWS:].any() and not mv[-EXTRA_ROWS:].any()
    for view, m in ((q, mq), (k, mk), (v, mv)):
        assert torch.isfinite(view[m]).all() and torch.isnan(view[~m]).all()
    nan_in = int(torch.isnan(b.qbuf).sum())
    assert nan_in == b.qbuf.numel() - int(mq.sum()) and nan_in > 0
    if case.kv_fused:
        assert b.vbuf is b.kbuf and int(torch.isnan(b.kbuf).sum()) == b.kbuf.numel() - int(mk.sum()) - int(mv.sum())
    for t, cols in ((b.qbuf, b.qcols), (b.kbuf, b.kcols), (b.vbuf, b.vcols), (b.obuf, b.ocols)):
        assert t.stride(0) % 8 == 0 and cols.start % 8 == 0 and cols.start > 0 and cols.stop < t.shape[1]
    assert b.obuf.shape[0] == b.qbuf.shape[0] and (b.obuf == 0x5A5A).all() and torch.isfinite(b.obuf.view(torch.bfloat16)).all()


def _hand_built(case: Case, q, k, v):
    """[q rows, heads * d] float64: the case's result by reshape / permute and SDPA, written for the case's layout (rows the
    descriptor does not address are left 0).  q, k, v: the float64 views without the spare rows at the end."""
    r = Rules(case.heads, case.d, **case.desc)
    c = case.heads * case.d
    if r.q_log2:
        q = q * (math.log(2.0) * case.d ** 0.5)               # SDPA multiplies by d^-0.5: scores q.k ln 2
    out = torch.zeros(q.shape, dtype=torch.float64)
    if case.name.startswith("anchor_appended"):
        fpc, hw, frames = case.meta["frames_per_clip"], r.lq, r.batches
        own = k.reshape(-1, hw, c), v.reshape(-1, hw, c)          # frames own frames, then one appended anchor frame per clip
        kk, vv = (torch.cat([t[frames:].repeat_interleave(fpc, 0), t[:frames]], dim=1) for t in own)
        return _sdpa_ref(q.reshape(frames, hw, c), kk, vv, case.heads).reshape(-1, c)
    if r.q_inner > 1:                                             # temporal: rows ordered (clip, frame, pixel)
        hw, clips = r.q_inner, r.batches // r.q_inner
        qf = r.q_outer_rows // hw                                 # frames per clip in the q buffer (one may be a guard frame)
        pad = clips * qf * hw - q.shape[0]
        qs = torch.cat([q, torch.zeros(pad, c, dtype=torch.float64)]).reshape(clips, qf, hw, c)[:, :r.lq].permute(0, 2, 1, 3).reshape(clips * hw, r.lq, c)
        ks, vs = (t.reshape(clips, r.lk, hw, c).permute(0, 2, 1, 3).reshape(clips * hw, r.lk, c) for t in (k, v))
        o = _sdpa_ref(qs, ks, vs, case.heads).reshape(clips, hw, r.lq, c).permute(0, 2, 1, 3)
        full = torch.zeros(clips, qf, hw, c, dtype=torch.float64)
        full[:, :r.lq] = o
        return full.reshape(-1, c)[:q.shape[0]]
    pad = r.batches * r.q_outer_rows - q.shape[0]                 # (the last batch has no guard rows of its own)
    qs = torch.cat([q, torch.zeros(pad, c, dtype=torch.float64)]).reshape(r.batches, r.q_outer_rows, c)[:, :r.lq]
    kvb = r.batches // r.kv_div
    padk = kvb * r.kv_outer_rows - k.shape[0]
    ks, vs = (torch.cat([t, torch.zeros(padk, c, dtype=torch.float64)]).reshape(kvb, r.kv_outer_rows, c)[:, :r.lk].repeat_interleave(r.kv_div, 0)
              for t in (k, v))
    qh, kh, vh = (t.reshape(r.batches, -1, case.heads, case.d).transpose(1, 2) for t in (qs, ks, vs))
    o = F.scaled_dot_product_attention(qh, kh, vh, is_causal=bool(r.causal)).transpose(1, 2).reshape(r.batches, r.lq, c)
    full = torch.zeros(r.batches, r.q_outer_rows, c, dtype=torch.float64)
    full[:, :r.lq] = o
    return full.reshape(-1, c)[:q.shape[0]]


@pytest.mark.parametrize("case", CASES, ids=lambda cs: cs.name)
def test_gpu_case_reference_equals_hand_built_sdpa(case: Case):
    """What the GPU test compares against, on the very buffers it uses (NaN fill included), equals a reshape / permute + SDPA
    reference written by hand for the case's layout — the old way of building a reference, once more, as a check of the new one."""
    b = build(case)
    q, k, v = b.qbuf[:, b.qcols], b.kbuf[:, b.kcols], b.vbuf[:, b.vcols]
    ref, written = attn_ref(q, k, v, case.heads, case.d, out=b.obuf.view(torch.bfloat16)[:, b.ocols], **case.desc)
    assert torch.isfinite(ref).all() and (ref[~written] == 0).all()
    hand = _hand_built(case, q[:-EXTRA_ROWS].double(), k[:-EXTRA_ROWS].double(), v[:-EXTRA_ROWS].double())
    assert not written[-EXTRA_ROWS:].any() and torch.isfinite(hand[written[:-EXTRA_ROWS]]).all()
    assert (hand - ref[:-EXTRA_ROWS])[written[:-EXTRA_ROWS]].abs().max().item() <= 1e-12


def _emulated_launch(case, spoil=None):
    """A stand-in for the GPU in the harness: the hand-built result rounded to bf16 and stored where the descriptor says."""
    def launch(b):
        q, k, v = b.qbuf[:, b.qcols], b.kbuf[:, b.kcols], b.vbuf[:, b.vcols]
        hand = _hand_built(case, q[:-EXTRA_ROWS].double(), k[:-EXTRA_ROWS].double(), v[:-EXTRA_ROWS].double())
        written = attn_read_masks(q.shape, k.shape, v.shape, case.heads, case.d, **case.desc)[0]        # q and out share rows and columns
        obuf = b.obuf.clone()
        out = obuf.view(BF)[:, b.ocols]
        out[:-EXTRA_ROWS][written[:-EXTRA_ROWS]] = hand[written[:-EXTRA_ROWS]].to(BF)
        label = case.label
        if spoil == "guard":
            obuf[-1, b.ocols.start] = 0            # one element of a row the descriptor does not address
        elif spoil == "nan":
            out[0, 0] = float("nan")               # what 0 * NaN would leave
        elif spoil == "label":
            label = "attn_kernel d=8"
        return obuf, b.qbuf.clone(), b.kbuf.clone(), b.vbuf.clone(), label
    return launch


@pytest.mark.parametrize("case", CASES, ids=lambda cs: cs.name)
def test_harness_on_an_emulated_launch(case: Case):
    """The harness of the GPU test, run on every case with the hand-built float64 result (rounded to bf16) in the GPU's place: it
    passes — buffers, masks, reference and checks are consistent with each other (this says nothing about the kernels)."""
    check_case(case, _emulated_launch(case))


@pytest.mark.parametrize("spoil", ["guard", "nan", "label"])
def test_harness_refuses_a_spoiled_launch(spoil):
    case = next(cs for cs in CASES if cs.name == "strided_out-general")
    with pytest.raises(AssertionError):
        check_case(case, _emulated_launch(case, spoil))


# ------------------------------------------------------------------------------------------
# The defect table.  A mutant makes ONE mistake in the rule it overrides; a read that leaves the view is taken from the flat
# buffer behind it, wrapped at the buffer's end (a kernel would read whatever memory follows).
class _Flat(Rules):
    def gather(self, t, rows, h):
        flat = t.as_strided((t.untyped_storage().nbytes() // t.element_size() - t.storage_offset(),), (1,))
        idx = torch.tensor(rows)[:, None] * t.stride(0) + self.head_col(h) + torch.arange(self.d)[None]
        return flat[idx % flat.numel()]


def _seg1_mul_is_frames_per_clip(case):
    class Mutant(_Flat):          # network.py's unsharded call passes seg1_mul = frames_per_clip; the appended-anchor form needs 1
        def seg1_batch(self, batch):
            return (batch // self.seg1_div) * case.meta["frames_per_clip"] + self.seg1_add
    return Mutant


def _kv_outer_is_q_outer(case):
    class Mutant(_Flat):          # one `outer_rows` for both sides: right whenever Lq == Lk
        def kv_base(self, kvb):
            return (kvb // self.kv_inner) * self.q_outer_rows + (kvb % self.kv_inner) * self.kv_inner_rows
    return Mutant


def _ln2_is_rsqrt_d(case):
    class Mutant(_Flat):          # `scale` applied to a q that already carries it
        def score_scale(self):
            return float(self.d) ** -0.5
    return Mutant


def _head_offset_from_full_head_count(case):
    class Mutant(_Flat):          # rank 1 of a head-sharded launch offsetting by its GLOBAL head index, as in the unsharded tensor
        def head_col(self, h):
            return (self.heads + h) * self.d
    return Mutant


def _form(prefixes):
    return [cs for cs in CASES if cs.name.startswith(prefixes)]


DEFECTS = ([(cs, _seg1_mul_is_frames_per_clip) for cs in _form("anchor_appended")]
           + [(cs, _kv_outer_is_q_outer) for cs in _form(("temporal", "strided_out-short"))]
           + [(cs, _ln2_is_rsqrt_d) for cs in _form("rowshard_qlog2")]
           + [(cs, _head_offset_from_full_head_count) for cs in _form("headshard")])


def test_defect_table_covers_every_new_form():
    assert len(_form("anchor_appended")) == 4 and len(_form("temporal")) == 9 and len(_form("rowshard_qlog2")) == 3 and len(_form("headshard")) == 12


@pytest.mark.parametrize("case,mutant", DEFECTS, ids=lambda x: x.name if isinstance(x, Case) else x.__name__.strip("_"))
def test_address_mistake_moves_the_result(case: Case, mutant):
    b = build(case, nan_fill=False)
    q, k, v = b.qbuf[:, b.qcols], b.kbuf[:, b.kcols], b.vbuf[:, b.vcols]
    out = b.obuf.view(torch.bfloat16)[:, b.ocols]
    ref, written = attn_ref(q, k, v, case.heads, case.d, out=out, **case.desc)
    bad, written_bad = attn_ref(q, k, v, case.heads, case.d, rules=mutant(case), out=out, **case.desc)
    assert torch.equal(written, written_bad)
    move = (bad - ref)[written].abs().max().item()
    lim = tolerance(ref[written])
    print(f"[attn-defect] {case.name}: {mutant.__name__.strip('_')} moves the result by {move:.4g} = {move / lim:.1f} x the limit {lim:.4g}")
    assert move >= 4 * lim, f"{case.name}: the mistake moves the result by {move:.4g}, limit {lim:.4g}: the case would not notice it"
