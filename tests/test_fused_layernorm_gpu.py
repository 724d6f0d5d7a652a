"""LayerNorm computed INSIDE a kernel, on a real MI355X, per element: ff320 with ln = True, both block-tail forms of ff320, lin320 /
lin320s with ln_eps, lin640s with ln_stats, and the ln_sums consumer of lin640s and g8.

tests/test_epilogue_gpu.py leaves these forms out because a LayerNorm in the kernel rounds.  It does not on the rows of
tests/_epilogue_ref.ln_rows: x = s z + m, z a permutation of 80 / 80 entries +-1, 60 / 60 of +-2 and 20 / 20 of +-4, s a power of two, m an
integer.  Mean m and variance 4 s^2 come out of the kernels' fp32 sums exactly, and the normalised value lies within 3e-5 of z / 2, a bf16
number: the MFMA operand is z / 2 bit for bit whatever rsqrtf returns in its last bits (tests/test_epilogue_ref.py shows it for every row
used here, rsqrtf moved by +-4 ulp, and that the planted defects — a neighbour's statistics, a missing shuffle, no mean, another eps, a
forgotten granule — change it; a ONE-PASS variance does not: on bf16-exact rows its fp32 sums are exact too, see that test).  Adjacent
rows differ in (s, m), a few rows have |m| = 96 at s = 1/2.  Downstream of the LayerNorm everything is the dyadic machinery of
tests/_epilogue_ref.py:

  * ff320, ln = True: |got - ref64| <= the bound of the ln = False case, nothing added for the LayerNorm; M = 48, 200 and 128 CUs + 200,
    the smallest M at which a workgroup walks a second round (pipeline_reset, the ring across rounds, the ragged last round) — that M
    once with ln = False as well.  gamma in {1/2, 1, 2}, beta multiples of 1/4, folded by pack_ff320 exactly (asserted);
  * block tail: the residual is the fix-up that makes W_o a + b_o + res land on an ln_rows row, so the prologue rounds nothing; the
    `to_out + FF` form has the plain bound, `+ proj_out` the bound derived next to _epilogue_ref.ff320_tail_case.  (PREFETCH_A of
    ff320.hip is compiled out — TAIL_PREFETCH_A = 0 — so the rows of a round are read at its top in every form.)
  * lin320 / lin320s with ln_eps: bf16_rne(float64 result) bit for bit, exact ties of both parities required; small shapes and N = 960
    (three slices) through ccedit_gemm, since ops.linear sends ln_eps from 32 768 rows and N = 320 only; M = 32 768 + 13 and M = 65 536
    (8 tiles per workgroup against lin320s_kernel's 7 ring slots) through ops.linear;
  * lin640s with ln_stats (tile 10): M = 16 / 304, N = 128 / 640, bit for bit; with ln_sums (lin640s and g8 tiles 12 / 13): rstd =
    rsqrtf(var + eps) is no power of two, so that case is bounded (_epilogue_ref.bound_lnf_sums), rsqrtf taken within 4 ulp: a premise.

Every case asserts the kernel that ran, reads a strided source, writes into a sentinel-filled wider buffer whose other columns must keep
their sentinels, prints its largest |err| / bound and where, and repeats the launch once for equal bits.

measured (MI355X, 256 CUs, first run; max |err| / bound): ff320 ln M = 48 / 200 / 32 968: 0.9785 / 0.9743 / 0.9996, ln = False at 32 968:
0.9996, `to_out + FF` the same three figures, `+ proj_out` 0.5474 / 0.5879 / 0.6937 — each equal to the fp32 emulation's figure on the
CPU where that runs (M = 48, 200); the largest ones are bf16 ties of the output, where half an ulp IS the bound.  lin320 / lin320s
with ln_eps and lin640s with ln_stats: every case bit for bit (1 765 to 3 649 648 exact ties per case with ln_eps, 73 to 11 925 with
ln_stats, both parities of the kept bit in each).  ln_sums: lin640s 0.9985 - 0.9988, g8 tiles 12 / 13 0.9989 in both lane maps (ties again).  Every
second launch bit-equal, every sentinel outside the slices intact.
"""
import ctypes
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _elementwise_ref as R  # noqa: E402
import _epilogue_ref as P  # noqa: E402

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
LEAD = 8                            # columns in front of a slice: 16 bytes of bf16, the alignment of the kernels' loads and stores
G8 = {12: "g8_kernel 256ch x 256pix", 13: "g8_kernel 128ch x 512pix"}
FF_LABEL = {None: "ff320_kernel", False: "ff320_kernel (to_out + FF)", True: "ff320_kernel (block tail: to_out + FF + proj_out)"}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _last():
    from ccedit_amd import hip
    return hip.lib().ccedit_last_kernel().decode()


def _wide(rows, n, lead=LEAD, width=None):
    """(whole buffer, its column slice [lead, lead + n)): sentinel-filled, a multiple of 8 wide, at least one guard column behind."""
    width = width or (n + lead + 1 + 7) // 8 * 8
    buf = R.sentinel_fill(rows * width, BF, "cuda").view(rows, width)
    return buf, buf[:, lead:lead + n]


def _in_wide(t, lead=LEAD, width=None):
    """A bf16 operand as a column slice of a sentinel-filled wider buffer."""
    buf, view = _wide(t.shape[0], t.shape[1], lead, width)
    view.copy_(t.to(BF))
    return view


def _written(buf, n, what):
    mask = torch.zeros(buf.shape, dtype=torch.bool)
    mask[:, LEAD:LEAD + n] = True
    R.assert_sentinels(buf, mask, what)


def _ran(label):
    """The label of the last launch is `label` (and not a longer form that contains it)."""
    last = _last()
    return label in last and (label != FF_LABEL[None] or "to_out" not in last) and (label != FF_LABEL[False] or "proj_out" not in last)


def _twice(launch, m, n, label, what):
    """launch(out) into two sentinel-filled wider buffers: the kernel label, exactly the slice written, equal bits; returns the output."""
    outs = []
    for _ in range(2):
        buf, out = _wide(m, n)
        launch(out)
        assert _ran(label), f"{what}: ran {_last()}"
        torch.cuda.synchronize()
        _written(buf, n, what)
        outs.append(out.cpu().contiguous())
    R.assert_bits_equal(outs[1], outs[0], f"{what}: second launch")
    return outs[0]


def _ff_m(m):
    return P.ff_rounds_m(torch.cuda.get_device_properties(0).multi_processor_count) if m == "rounds" else m


FF_SHAPES = list(P.FF_M) + ["rounds"]


# ------------------------------------------------------------------------------------------ ff320
@functools.lru_cache(maxsize=None)
def _ff_packs():
    """(ln pack, pre-folded pack for ln = False) of the one weight set; pack_ff320's fold is exact: both streams are equal."""
    from ccedit_amd.packing import pack_ff320
    wt = P.ff320_ln_weights()
    ln = pack_ff320(wt.w1.float(), wt.b1.float(), wt.w2.float(), wt.b2.float(), wt.gamma.float(), wt.beta.float())
    pre = pack_ff320(wt.g1.float(), wt.b1p.float(), wt.w2.float(), wt.b2.float(), None, None)
    assert torch.equal(ln.stream, pre.stream) and torch.equal(ln.b2p, pre.b2p), "pack_ff320: W1 diag(gamma) / b1 + W1 beta are not exact"
    half = pack_ff320(wt.weff.float(), wt.b1p.float(), wt.w2.float(), wt.b2.float(), None, None, device="cuda")
    ln.stream, ln.b2p = ln.stream.cuda(), ln.b2p.cuda()
    return ln, half


@pytest.mark.parametrize("m", FF_SHAPES)
def test_ff320_ln(m):
    """x + W2 . bf16(v gelu(u)) + b2 with the LayerNorm in the kernel, on ln_rows: the ln = False bound, unchanged."""
    _dev()
    from ccedit_amd import ops
    m = _ff_m(m)
    o = P.ff320_ln_case(m)
    pk, _ = _ff_packs()
    xd = _in_wide(o.x)
    got = _twice(lambda out: ops.ff320(xd, pk, eps=P.LN_EPS, ln=True, out=out), m, P.FF_DIM, FF_LABEL[None], f"ff320 ln M={m}")
    P.assert_within(got, o.ref, o.bound, f"ff320 ln M={m} (max |ref| {o.ref.abs().max().item():.1f})")


def test_ff320_no_ln_past_one_round():
    """ln = False on the integers z with the pre-folded weights at M = 128 CUs + 200: the first per-element check of any arm past a round."""
    _dev()
    from ccedit_amd import ops
    m = _ff_m("rounds")
    o = P.ff320_ln_case(m)
    _, half = _ff_packs()
    ref, bnd = P.ff_with_residual(o, o.z)
    xd = _in_wide(o.z)
    got = _twice(lambda out: ops.ff320(xd, half, ln=False, out=out), m, P.FF_DIM, FF_LABEL[None], f"ff320 ln=False M={m}")
    P.assert_within(got, ref, bnd, f"ff320 ln=False M={m}")


@functools.lru_cache(maxsize=None)
def _tail_pack(epi):
    from ccedit_amd.packing import pack_ff320_tail
    tw = P.ff320_tail_weights()
    return pack_ff320_tail(_ff_packs()[0], tw.wo.float(), tw.bo.float(), tw.wp.float() if epi else None, tw.bp.float() if epi else None, device="cuda")


@pytest.mark.parametrize("m", FF_SHAPES)
@pytest.mark.parametrize("epi", [False, True], ids=["to_out+FF", "to_out+FF+proj_out"])
def test_ff320_block_tail(epi, m):
    """tok = W_o a + b_o + res lands exactly on an ln_rows row; t = tok + FF(LN(tok)) within the plain bound; with proj_out
    W_p bf16(t) + b_p + x_in within |W_p| delta + the accumulation term + half an ulp.  a is a column slice of a 960-wide buffer."""
    _dev()
    from ccedit_amd import ops
    m = _ff_m(m)
    c = P.ff320_tail_case(m)
    pk = _tail_pack(epi)
    ad, rd, xd = _in_wide(c.a, 320, 960), _in_wide(c.res), _in_wide(c.xin) if epi else None
    what = f"block tail {'to_out + FF + proj_out' if epi else 'to_out + FF'} M={m}"
    got = _twice(lambda out: ops.ff320(None, pk, eps=P.LN_EPS, a=ad, res=rd, res2=xd, out=out), m, P.FF_DIM, FF_LABEL[epi], what)
    ref, bnd = (c.ref3, c.bound3) if epi else (c.ref2, c.bound2)
    P.assert_within(got, ref, bnd, what)


# ------------------------------------------------------------------------------------------ lin320 / lin320s with ln_eps
@functools.lru_cache(maxsize=None)
def _lin_pack(n):
    from ccedit_amd.packing import fold_layernorm
    wt = P.lin320_ln_weights(n)
    pw = fold_layernorm([wt.w.float()], [wt.b.float()], wt.gamma.float(), wt.beta.float())
    assert torch.equal(pw.w[:n, :P.FF_DIM].double(), wt.wf) and torch.equal(pw.bias[:n].double(), wt.bf), "fold_layernorm is not exact"
    return pw.to("cuda")


def _gemm_ln(xd, pw, out, eps):
    """ccedit_gemm with CcGemmDesc.ln_eps on tile 9, the descriptor built as ops.gemm builds it (ops.linear refuses ln_eps below 32 768 rows)."""
    from ccedit_amd import hip
    d = hip.CcGemmDesc()
    d.M, d.N, d.Cin, d.Cin1, d.taps, d.mode = xd.shape[0], pw.n, pw.cin, xd.shape[1], pw.taps, hip.GEMM_LINEAR
    d.stride, d.ksize, d.lda, d.ldc, d.Kpad, d.korder = 1, pw.ksize, xd.stride(0), out.stride(0), pw.kpad, pw.korder
    d.act, d.tile, d.ln_eps = hip.ACT_NONE, 9, eps
    d.A, d.W, d.Wfrag, d.bias, d.out = xd.data_ptr(), pw.w.data_ptr(), pw.wfrag.data_ptr(), pw.bias.data_ptr(), out.data_ptr()
    hip.check(hip.lib().ccedit_gemm(ctypes.byref(d), torch.cuda.current_stream().cuda_stream), "ccedit_gemm")


def _judge_lin(got, o, what):
    P.assert_ties(o.total, what)
    P.assert_rounded(got, o.total, what)


@pytest.mark.parametrize("n", P.LIN_LN_N)
@pytest.mark.parametrize("m,want", P.LIN_LN_SMALL)
def test_lin320_ln_small(m, want, n):
    """M = 32 / 96 (lin320s_kernel) and 130 (lin320_kernel, ragged last tile); N = 320 and 960: three slices, each normalising the tile again."""
    _dev()
    o = P.lin320_ln_case(m, n)
    pw, xd = _lin_pack(n), _in_wide(o.x)
    got = _twice(lambda out: _gemm_ln(xd, pw, out, P.LN_EPS), m, n, want, f"{want} ln {m} x {n}")
    _judge_lin(got, o, f"{want} ln {m} x {n}")


@pytest.mark.parametrize("m,want", [(P.LIN_LN_RAGGED_M, "lin320_kernel"), (P.LIN_LN_WRAP_M, "lin320s_kernel")])
def test_lin320_ln_through_ops_linear(m, want):
    """ops.linear(..., ln_eps=1e-5): ragged M past 32 768, and 65 536 rows — every workgroup walks 8 tiles through lin320s_kernel's ring, so
    a slot is normalised in place, consumed and refilled: a stale or twice-normalised row would appear in the wrapped slot."""
    _dev()
    from ccedit_amd import ops
    o = P.lin320_ln_case(m, 320)
    pw, xd = _lin_pack(320), _in_wide(o.x)
    assert ops.ln320_applicable(m, pw)
    got = _twice(lambda out: ops.linear(xd, pw, ln_eps=P.LN_EPS, out=out), m, 320, want, f"{want} ln {m} x 320")
    _judge_lin(got, o, f"{want} ln {m} x 320")


# ------------------------------------------------------------------------------------------ lin640s / g8: ln_stats and ln_sums
@functools.lru_cache(maxsize=None)
def _lnf_pack(m, n, k):
    from ccedit_amd.packing import fold_layernorm
    o = P.lnf_case(m, n, k, False, P.LNF640.get((m, n), 0))
    pw = fold_layernorm([o.w.float()], [o.b.float()], torch.ones(k), torch.zeros(k)).to("cuda")
    assert torch.equal(pw.colsum.double().cpu()[:n], o.colsum)
    return o, pw


@pytest.mark.parametrize("n", [128, 640])
@pytest.mark.parametrize("m", [16, 304])
def test_lin640s_ln_stats(m, n):
    """tile 10 with (mean, rstd) per row riding in the tile's last DMA: one tile and 19 (ragged against the workgroup ranges), N = 128 (half a
    slice) and 640 (third slice half empty): bf16_rne(rstd (acc - mean colsum) + b) bit for bit."""
    _dev()
    from ccedit_amd import ops
    o, pw = _lnf_pack(m, n, 640)
    xd, st = _in_wide(o.x), torch.stack([o.mean, o.rstd], dim=1).float().contiguous().cuda()
    what = f"lin640s ln_stats {m} x {n}"
    got = _twice(lambda out: ops.linear(xd, pw, ln_stats=st, out=out, tile=10), m, n, "lin640s_kernel", what)
    P.assert_ties(o.p, what)
    P.assert_rounded(got, o.p, what)


@pytest.mark.parametrize("n", [128, 640])
@pytest.mark.parametrize("m", [16, 304])
def test_lin640s_ln_sums(m, n):
    """The same cases with the statistics as double sums (K mean, K (var + mean^2)), var in {1/4, 1, 4, 16}: bounded by bound_lnf_sums."""
    _dev()
    from ccedit_amd import ops
    o, pw = _lnf_pack(m, n, 640)
    xd, sums = _in_wide(o.x), P.ln_sums(o, 640).cuda()
    what = f"lin640s ln_sums {m} x {n}"
    got = _twice(lambda out: ops.linear(xd, pw, ln_sums=(sums, P.LN_EPS), out=out, tile=10), m, n, "lin640s_kernel", what)
    ref, bnd = P.bound_lnf_sums(o)
    P.assert_within(got, ref, bnd, what)


@pytest.mark.parametrize("tile", [12, 13])
def test_g8_ln_sums(tile):
    """g8 tiles 12 / 13 (300 x 512 <- 256) with ln_sums, both MFMA lane maps, each bounded.  The two maps are NOT bit-equal here, unlike
    everywhere else: the accumulators start from the inexact b / rstd - mean colsum, so the order in which a map adds the (exact) products
    decides the roundings — measured 3 of 153 600 elements apart, all cancellations near zero (-1.8e-7 against -2.1e-7)."""
    _dev()
    from ccedit_amd import hip, ops
    m, n, k = P.LNF_SHAPE
    o, pw = _lnf_pack(m, n, k)
    xd, sums = _in_wide(o.x), P.ln_sums(o, k).cuda()
    ref, bnd = P.bound_lnf_sums(o)
    lib, old = hip.lib(), ctypes.c_int32(0)
    assert lib.ccedit_policy_get(b"g8_mfma16", ctypes.byref(old)) == 0
    try:
        for arm in (0, 2):
            assert lib.ccedit_policy_set(b"g8_mfma16", arm) == 0
            what = f"g8 ln_sums tile {tile} mfma16={arm}"
            got = _twice(lambda out: ops.linear(xd, pw, ln_sums=(sums, P.LN_EPS), out=out, tile=tile), m, n, G8[tile], what)
            assert "LayerNorm folded" in _last(), _last()
            P.assert_within(got, ref, bnd, what)
    finally:
        lib.ccedit_policy_set(b"g8_mfma16", old.value)
