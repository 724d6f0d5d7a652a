"""The descriptor forms of tests/test_attn_desc_gpu.py and the buffers they run on (helper; no tests in here).

Every case mirrors a call that ccedit_amd/network.py makes and that no single-GPU test reached: the keywords are the ones
`ops.attention` takes.  `build` lays the operands out the way production memory looks: q, k, v and out are column slices (offsets
that are multiples of 8 elements, the alignment the kernels ask for) of buffers that are wider and longer than the descriptor needs;
every input element the descriptor does not address is bf16 NaN (such memory comes from torch.empty: a kernel may load it, it may not
let it reach the result), the whole output buffer holds a fixed finite bit pattern.  tests/test_attn_ref.py builds the same cases
without a GPU to show that each is sensitive to the address mistake it is there for.
"""
import math
from dataclasses import dataclass, field

import torch

from _attn_ref import Rules, attn_read_masks

BF = torch.bfloat16
LOG2E = 1.4426950408889634
OUT_FILL = 0x5A5A                     # bf16 1.7e16: finite, and no kernel result looks like it
EXTRA_ROWS = 3                        # rows past the last addressed one, in every buffer


@dataclass
class Case:
    name: str
    kernel: str                       # the kernel this case is meant to reach (label of ccedit_last_kernel without " d=...")
    heads: int
    d: int
    desc: dict                        # keywords of ops.attention
    kv_fused: bool = True             # k and v are slices of ONE [rows, 2c] projection (8 unaddressed columns between them)
    lead: int = 8                     # unaddressed columns before / after the slices of q, k, v
    trail: int = 8
    out_lead: int = 8
    out_trail: int = 8
    meta: dict = field(default_factory=dict)      # what the defect table needs: frames_per_clip, full_heads
    seed: int = 0

    @property
    def label(self):
        return f"{self.kernel} d={self.d}"


POLICY_DEFAULTS = dict(attn_short=1, attn_text=1, attn_spatial=1, attn_pv16=1, attn_opt=1)       # CcPolicy, common.h


def expected_arm(case: Case, policy: dict = None) -> dict:
    """ccedit_attention's selection (attention.hip) with the applicability rules of attnshort.hip / attntext.hip / attnspatial.hip
    restated from their literals, under `policy` (switches of ccedit_policy_set that differ from the defaults); the alignment
    conditions hold for every buffer `build` makes (asserted there).  Besides the kernel: what decides the code path inside it.

        kernel        label of ccedit_last_kernel without " d=..."
        nw            waves per workgroup (32 query rows each)
        buffers       K / V tiles in LDS: 1 (attn_kernel, Lk <= 64), 2 (its ring), 3 (the spatial ring), 0 = all keys staged at once
        masked_tail   the last 64-key tile reaches past Lk (general / spatial); keys past Lk are masked (short: Lk < 32, text: Lk < 96)
        block_order   "qtile": heads of a (batch, query tile) back to back (attn_kernel at Lk <= 128 without a leading segment, and
                      the text kernel); "head": query tiles of a (batch, head) back to back; "pixel": the short kernel's persistent loop
        opt, pv16     spatial kernel only: the optimistic first pass, the 16x16x32 PV product (d = 40)
    """
    pol = dict(POLICY_DEFAULTS, **(policy or {}))
    assert set(pol) == set(POLICY_DEFAULTS)
    r = Rules(case.heads, case.d, **case.desc)
    c = case.heads * case.d
    plain_q = not r.q_log2
    short = (case.d in (40, 80, 160) and c % 320 == 0 and r.lq <= 32 and r.lk <= 32 and (r.lq + 2 * r.lk) * (320 // 8) <= 8 * 256
             and r.seg1_len == 0 and not r.causal)
    text = (case.d in (40, 80) and 64 <= r.lk <= 96 and r.seg1_len == 0 and not r.causal and c % 320 == 0 and 32 % max(c // 320, 1) == 0
            and r.q_inner == 1 and r.q_seq_rows == 1 and r.q_outer_rows == r.lq and r.kv_inner == 1 and r.kv_seq_rows == 1
            and r.kv_outer_rows >= r.lk and r.batches % r.kv_div == 0 and r.kv_div * r.lq >= 2048)
    spatial = ((case.d == 40 or (case.d == 80 and pol["attn_spatial"] == 1)) and r.lq >= 1024 and r.lk >= 192 and not r.causal
               and r.seg1_len % 64 == 0)
    if pol["attn_short"] and plain_q and short:
        return dict(kernel="attn_short_kernel", nw=4, buffers=0, masked_tail=r.lk < 32, block_order="pixel")
    if pol["attn_text"] and plain_q and text:
        return dict(kernel="attn_text_kernel", nw=8, buffers=0, masked_tail=r.lk < 96, block_order="qtile")
    if pol["attn_spatial"] and spatial:
        return dict(kernel="attn_spatial_kernel", nw=8, buffers=3, masked_tail=r.lk % 64 != 0, block_order="head",
                    opt=bool(pol["attn_opt"]), pv16=bool(pol["attn_pv16"]) and case.d == 40)
    assert case.d in (8, 16, 32, 40, 64, 80, 128, 160), "head dim not instantiated"
    nw = 1 if r.lq <= 32 else (8 if case.d <= 80 and r.lq >= 1024 else 4)
    return dict(kernel="attn_kernel", nw=nw, buffers=1 if r.lk <= 64 else 2, masked_tail=r.lk % 64 != 0,
                block_order="qtile" if r.lk <= 128 and r.seg1_len == 0 else "head")


def expected_kernel(case: Case, policy: dict = None) -> str:
    return expected_arm(case, policy)["kernel"]


def _temporal(tl, tg, hw=12, clips=2, q_frames=None):
    """network.py run_temporal, frame-sharded: tl local query frames against the tg gathered key frames of every pixel."""
    return dict(batches=clips * hw, lq=tl, lk=tg, q_inner=hw, q_outer_rows=(q_frames or tl) * hw, q_inner_rows=1, q_seq_rows=hw,
                kv_inner=hw, kv_outer_rows=tg * hw, kv_inner_rows=1, kv_seq_rows=hw)


def _appended_anchor(clips, fpc, hw):
    """network.py run_frames, keyframes sharded: the anchor frame's K/V of clip b appended as kv frame frames + b."""
    frames = clips * fpc
    return dict(batches=frames, lq=hw, lk=2 * hw, kv_outer_rows=hw, seg1_len=hw, seg1_div=fpc, seg1_mul=1, seg1_add=frames)


def _cases():
    out = []
    for d in (40, 80):
        out.append(Case(f"anchor_appended-general-d{d}", "attn_kernel", 4, d, _appended_anchor(2, 3, 96), meta=dict(frames_per_clip=3)))
    for d in (40, 80):
        out.append(Case(f"anchor_appended-spatial-d{d}", "attn_spatial_kernel", 2, d, _appended_anchor(2, 2, 1088), meta=dict(frames_per_clip=2)))
    for d, heads in ((40, 8), (80, 4), (160, 2)):
        for tl, tg in ((2, 5), (3, 17), (9, 32)):
            # cc_attn_short_applicable: (Lq + 2 Lk) * 40 granules <= 8 * 256, i.e. Lq + 2 Lk <= 51: 12 and 37 pass, 73 does not
            kernel = "attn_short_kernel" if tl + 2 * tg <= 51 else "attn_kernel"
            out.append(Case(f"temporal-{tl}x{tg}-d{d}", kernel, heads, d, _temporal(tl, tg)))
    out.append(Case("rowshard_qlog2-96x2-d40", "attn_kernel", 4, 40, dict(batches=2, lq=96, lk=192, q_log2=True)))
    for d in (40, 80):
        out.append(Case(f"rowshard_qlog2-1024x2-d{d}", "attn_spatial_kernel", 2, d, dict(batches=1, lq=1024, lk=2048, q_log2=True)))
    for heads in (1, 2):
        for batches in (1, 3):
            for lq, lk, kernel in ((200, 200, "attn_kernel"), (200, 77, "attn_kernel"), (1024, 1024, "attn_spatial_kernel")):
                out.append(Case(f"headshard-h{heads}-b{batches}-{lq}x{lk}", kernel, heads, 40, dict(batches=batches, lq=lq, lk=lk),
                                kv_fused=False, lead=8, trail=16, meta=dict(full_heads=8)))
    for lk in (77, 64, 96):
        out.append(Case(f"text_strided_out-lk{lk}", "attn_text_kernel", 8, 40,
                        dict(batches=4, lq=1100, lk=lk, kv_div=2, kv_outer_rows=lk + 5), out_lead=8, out_trail=56))
    # strided output on the other kernels, ragged Lq, three guard rows (one guard frame) after each batch's last query row
    out.append(Case("strided_out-general", "attn_kernel", 2, 40, dict(batches=3, lq=70, lk=77, q_outer_rows=73), out_lead=8, out_trail=56))
    out.append(Case("strided_out-spatial", "attn_spatial_kernel", 1, 40, dict(batches=2, lq=1030, lk=200, q_outer_rows=1033),
                    out_lead=8, out_trail=56))
    out.append(Case("strided_out-short", "attn_short_kernel", 8, 40, _temporal(2, 5, q_frames=3), out_lead=8, out_trail=56))
    out.append(Case("d16-70x130", "attn_kernel", 4, 16, dict(batches=3, lq=70, lk=130)))
    out.append(Case("d16-causal-130", "attn_kernel", 4, 16, dict(batches=3, lq=130, lk=130, causal=True)))
    for i, cs in enumerate(out):
        cs.seed = 10 * i
    return out


CASES = _cases()


def _gauss(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF)      # as test_ops_gpu._rnd: bf16-rounded Gaussians


@dataclass
class Built:
    qbuf: torch.Tensor                # the whole buffers (CPU, bf16); out: int16
    kbuf: torch.Tensor
    vbuf: torch.Tensor                # the same object as kbuf when k and v are slices of one projection
    obuf: torch.Tensor
    qcols: slice                      # the column slices that are handed to ops.attention
    kcols: slice
    vcols: slice
    ocols: slice
    written: torch.Tensor = None      # mask of the out VIEW


def build(case: Case, nan_fill: bool = True) -> Built:
    """The CPU buffers of one case.  nan_fill=False puts Gaussians where the NaNs would be (the addressed elements are the same
    numbers either way): the defect table of tests/test_attn_ref.py measures how far a mis-addressed read moves the result."""
    r = Rules(case.heads, case.d, **case.desc)
    c = case.heads * case.d
    q_rows = max(r.q_row(b, r.lq - 1) for b in range(r.batches)) + 1 + EXTRA_ROWS
    kv_rows = max(r.kv_row(b, j) for b in range(r.batches) for j in {0, max(r.seg1_len - 1, 0), r.lk - 1}) + 1 + EXTRA_ROWS
    qw = case.lead + c + case.trail
    kw = case.lead + c + 8 + c + case.trail if case.kv_fused else qw
    ow = case.out_lead + c + case.out_trail
    # what the kernels ask of a view: 16-byte aligned rows and slices (attention.hip: ld % 8; the short and text kernels: ldo % 8)
    assert all(x % 8 == 0 for x in (qw, kw, ow, case.lead, case.out_lead, c))

    def fill(rows, width, seed, scale=1.0):
        return torch.full((rows, width), math.nan, dtype=BF) if nan_fill else _gauss((rows, width), seed, scale)

    qscale = case.d ** -0.5 * LOG2E if r.q_log2 else 1.0          # q_log2: what the packer folds into to_q, rounded to bf16 once
    qbuf = fill(q_rows, qw, case.seed + 5, qscale)
    kbuf = fill(kv_rows, kw, case.seed + 6)
    vbuf = kbuf if case.kv_fused else fill(kv_rows, kw, case.seed + 7)
    qcols = slice(case.lead, case.lead + c)
    kcols = qcols
    vcols = slice(case.lead + c + 8, case.lead + 2 * c + 8) if case.kv_fused else qcols
    ocols = slice(case.out_lead, case.out_lead + c)
    q, k, v = qbuf[:, qcols], kbuf[:, kcols], vbuf[:, vcols]
    mq, mk, mv = attn_read_masks(q.shape, k.shape, v.shape, case.heads, case.d, **case.desc)
    q[mq] = _gauss(q.shape, case.seed + 1, qscale)[mq]
    k[mk] = _gauss(k.shape, case.seed + 2)[mk]
    v[mv] = _gauss(v.shape, case.seed + 3)[mv]
    obuf = torch.full((q_rows, ow), OUT_FILL, dtype=torch.int16)
    return Built(qbuf, kbuf, vbuf, obuf, qcols, kcols, vcols, ocols)


def tolerance(ref_on_mask: torch.Tensor) -> float:
    """The limit of the attention tests of tests/test_ops_gpu.py: 2^-6 of max |ref| plus 4e-3."""
    return 2.0 ** -6 * ref_on_mask.abs().max().item() + 4e-3


def check_case(case: Case, launch) -> None:
    """The one harness of tests/test_attn_desc_gpu.py.  launch(built) runs the case once on copies of the buffers and returns
    (out buffer int16, q buffer, k buffer, v buffer, kernel label), all on the CPU, as they are after the launch."""
    from _attn_ref import attn_ref
    b = build(case)
    ref, written = attn_ref(b.qbuf[:, b.qcols], b.kbuf[:, b.kcols], b.vbuf[:, b.vcols], case.heads, case.d,
                            out=b.obuf.view(BF)[:, b.ocols], **case.desc)
    full_mask = torch.zeros(b.obuf.shape, dtype=torch.bool)
    full_mask[:, b.ocols] = written
    got_bits, q_after, k_after, v_after, label = launch(b)
    got = got_bits.view(BF)[:, b.ocols].double()
    finite = bool(torch.isfinite(got[written]).all())
    err = (got - ref)[written].abs().max().item()
    lim = tolerance(ref[written])
    touched = int((got_bits != b.obuf)[~full_mask].sum())
    print(f"[attn-desc] {case.name}: {label}; max err {err:.4g}, limit {lim:.4g} (max|ref| {ref[written].abs().max().item():.4g}); "
          f"non-finite {not finite}; unaddressed output elements changed {touched}")
    assert label == case.label, f"{case.name}: ran {label!r}, meant for {case.label!r}"
    assert finite, f"{case.name}: non-finite output: unaddressed (NaN) memory reached the result"
    assert err <= lim, f"{case.name}: max err {err:.4g} > {lim:.4g}"
    assert touched == 0, f"{case.name}: {touched} output elements outside the addressed set were written"
    for name, after, before in (("q", q_after, b.qbuf), ("k", k_after, b.kbuf), ("v", v_after, b.vbuf)):
        assert torch.equal(after.view(torch.int16), before.view(torch.int16)), f"{case.name}: the launch changed {name}"
    again = launch(b)[0]
    assert torch.equal(again, got_bits), f"{case.name}: a second launch gave other bits"
