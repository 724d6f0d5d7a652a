"""tests/_attn_exact.py pinned without a GPU: the premise, the reference, the case table and what the bound notices.

1. The premise: fp32(float32(ln 2) * fp32(log2 e)) is exactly 1.0f and neither neighbouring float does that; `bf16_rne` equals the
   hardware's conversion.
2. Every case builds, meets the exactness condition (live terms within 24 of the row maximum, every other one >= 150 below, sums
   below 2^24 quanta) and the coverage conditions (asserted in `analyse`), and its exact reference equals the exp-based float64
   reference of tests/_attn_ref.py to 1e-12 with the same written mask.
3. The arm of every case is predicted from the literals of the four kernel files (`_attn_cases.expected_arm`) and equals the arm the
   case is listed for; the list reaches every arm the kernels have.  A retune that moves a case fails here first.
4. The harness of the GPU test passes with `bf16_rne(ref)` in the GPU's place and with an fp32 emulation of attn_kernel's online
   loop (64-key tiles, running maximum, rescale, both denominator forms), on every case.
5. The defect table: each mistake, planted in that emulation, misses the bound by >= 4 x on every case of its form (the forms are
   stated in DEFECTS).  Two defects cannot miss it by 4 x and are held to what they can do: a truncating store errs by < 1 ulp, 2 x
   the bound's rounding term (asserted: outside the bound on every case that rounds); a store that rounds ties away differs from
   round-to-nearest-even only AT a tie, where both neighbours are exactly 1/2 ulp away — inside any bound of this form.  It is
   caught by the harness's second assertion, bit equality in rows whose denominator is a power of two (the spiked rows of every
   spike case hold d exact ties per head, both parities).

One limit of the method.  On this grid P is exact in bf16, so the rounding of P, and a denominator that is inconsistent with the
rounded P, are not exercised; only the Gaussian tests (tests/test_ops_gpu.py, tests/test_attn_desc_gpu.py) see them, loosely.  Spikes
of 2^17 ... 2^40 (non-zero rescale factors on the spiked row itself in the tracked spatial arm) cannot be made exact — the sums span
more than 24 bits — and stay with those tests too.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _attn_exact as X  # noqa: E402
from _attn_cases import BF, Case, expected_arm  # noqa: E402
from _attn_ref import attn_ref  # noqa: E402

IDS = [cs.name for cs in X.CASES]


def test_unit_scale_in_fp32():
    f = np.float32
    l2e = f(1.4426950408889634)
    assert X.LN2F == float(f(math.log(2.0)))
    assert f(f(X.LN2F) * l2e) == f(1.0)
    for other in (np.nextafter(f(X.LN2F), f(0.0)), np.nextafter(f(X.LN2F), f(1.0))):
        assert f(other * l2e) != f(1.0)


def test_bf16_rne_is_the_hardware_conversion():
    g = torch.Generator().manual_seed(5)
    x = torch.cat([torch.randn(20000, generator=g) * 3.0, torch.tensor([128.5, 129.5, -128.5, -129.5, 0.0, 255.5, 256.0, 1.0])]).float()
    assert torch.equal(X.bf16_rne(x.double()), x.to(BF).double())
    ties = torch.tensor([128.5, 129.5, -130.5])
    assert X._round_bf16(ties.double(), "away").tolist() == [129.0, 130.0, -131.0]
    assert X._round_bf16(torch.tensor([128.9, -128.9]).double(), "trunc").tolist() == [128.0, -128.0]


@pytest.mark.parametrize("name", IDS)
def test_reference_equals_the_exp_based_float64_one(name):
    case = X.BY_NAME[name]
    a, b = X.analyse(case), X.grid_build(case)
    ref, written = attn_ref(b.qbuf[:, b.qcols], b.kbuf[:, b.kcols], b.vbuf[:, b.vcols], case.heads, case.d, **X.mode_desc(case, "q_log2"))
    assert torch.equal(written, a.written)
    assert (a.ref - ref)[written].abs().max().item() <= 1e-12


# what the issue's case list asks of the arms: (kernel, nw, buffers, masked_tail, block_order) and, per kernel, the head dims
ARMS_WANTED = {
    ("attn_kernel", 1, 1, False, "qtile"), ("attn_kernel", 1, 1, True, "qtile"), ("attn_kernel", 4, 2, False, "qtile"),
    ("attn_kernel", 4, 2, True, "head"), ("attn_kernel", 8, 2, True, "head"), ("attn_kernel", 8, 2, False, "head"),
    ("attn_kernel", 8, 2, True, "qtile"),
    ("attn_spatial_kernel", 8, 3, False, "head"), ("attn_spatial_kernel", 8, 3, True, "head"),
    ("attn_short_kernel", 4, 0, True, "pixel"), ("attn_text_kernel", 8, 0, True, "qtile"), ("attn_text_kernel", 8, 0, False, "qtile"),
}
DIMS_WANTED = {"attn_kernel": {8, 16, 32, 40, 64, 80, 128, 160}, "attn_spatial_kernel": {40, 80}, "attn_short_kernel": {40, 80, 160},
               "attn_text_kernel": {40, 80}}


def test_every_case_reaches_the_arm_it_is_listed_for():
    arms, dims, spatial = set(), {}, set()
    for case in X.CASES:
        for mode in case.meta["modes"]:
            for policy in case.meta["policies"]:
                arm = expected_arm(Case(case.name, case.kernel, case.heads, case.d, X.mode_desc(case, mode)), policy)
                assert arm["kernel"] == case.kernel, (case.name, mode, policy, arm)
                assert {k: arm[k] for k in ("nw", "buffers", "masked_tail", "block_order")} == \
                    {k: case.meta["arm"][k] for k in ("nw", "buffers", "masked_tail", "block_order")}, (case.name, mode, policy)
                arms.add((arm["kernel"], arm["nw"], arm["buffers"], arm["masked_tail"], arm["block_order"]))
                dims.setdefault(arm["kernel"], set()).add(case.d)
                if arm["kernel"] == "attn_spatial_kernel":
                    spatial.add((case.d, mode, arm["opt"], arm["pv16"]))
    assert ARMS_WANTED <= arms, ARMS_WANTED - arms
    assert dims == DIMS_WANTED
    assert spatial == ({(40, m, o, p) for m in ("q_log2", "scale") for o in (True, False) for p in (True, False)} |
                       {(80, m, o, False) for m in ("q_log2", "scale") for o in (True, False)})
    # q_log2 is not for the short and the text kernel (they apply `scale` themselves): those cases run with the keyword only
    assert all(cs.meta["modes"] == ("scale",) for cs in X.CASES if cs.kernel in ("attn_short_kernel", "attn_text_kernel"))


# ---- defect -> (the cases of its form, how it is held)
def _all(cs, a):
    return True


DEFECTS = {
    "drop_last_key": (_all, "key Lk - 1 dropped: every case"),
    "admit_key_lk": (lambda cs, a: cs.meta["variant"] == "shift", "key Lk admitted with score 0 and v = 0: the shift -24 cases"),
    "no_rescale_by_one": (lambda cs, a: cs.meta["variant"] == "stair", "no rescale when the maximum moves by exactly 1: the staircases"),
    "no_rescale_last_tile": (lambda cs, a: cs.desc["lk"] > 64, "no rescale of the last O^T row tile: every case with more than one key tile"),
    "neighbour_denominator": (lambda cs, a: cs.desc["lq"] > 1 and cs.desc["lk"] > 1, "the denominator of the row before: Lq, Lk > 1"),
    "flush_p": (lambda cs, a: X.uses_bump(cs), "p below 2^-8 of the running maximum flushed: every case with bump rows (Lk >= 16, Lq >= 3, no staircase)"),
    "scale_d": (lambda cs, a: cs.desc["lk"] > 1, "scale read as d^-0.5: every case with more than one key, in the mode that passes `scale`"),
    "causal_lt": (lambda cs, a: cs.desc.get("causal", False), "the causal bound j < i: the causal cases"),
    "channels_32_40": (lambda cs, a: cs.d == 40 and cs.desc["lk"] > 1, "channels [32, 40) left out of QK^T: d = 40 with more than one key"),
    "skip_spike_tile": (lambda cs, a: cs.meta["variant"] == "spike", "the tile of a spike key skipped: the spike cases"),
}


def _miss(case, values):
    """(largest |err| / bound over the addressed elements, inf where not finite; elements of power-of-two rows that differ from
    bf16_rne(ref)) of float64 values stored as bf16."""
    a = X.analyse(case)
    got = values.to(BF).double()
    err = (got - a.ref).abs()[a.written]
    ratio = X.miss(err, X.bound(a.ref)[a.written]).max().item() if bool(torch.isfinite(err).all()) else math.inf
    return ratio, int((got != X.bf16_rne(a.ref))[a.written & a.pow2].sum())


@pytest.mark.parametrize("name", IDS)
def test_harness_and_defect_table(name):
    case = X.BY_NAME[name]
    a = X.analyse(case)
    X.check_exact(case, X.fake_launch(case, lambda mode: X.bf16_rne(a.ref)))
    emu = {mode: X.emulate(case, mode) for mode in case.meta["modes"]}
    X.check_exact(case, X.fake_launch(case, lambda mode: emu[mode]))
    for defect, (form, what) in DEFECTS.items():
        if not form(case, a):
            continue
        mode = "scale" if defect == "scale_d" else case.meta["modes"][0]
        values = X.emulate(case, mode, defect)
        ratio, _ = _miss(case, values)
        print(f"[attn-exact-defect] {name}: {defect}: {ratio:.3g} x the bound")
        assert ratio >= 4.0, f"{name}: {defect} ({what}) misses the bound by {ratio:.3g} x only"
        with pytest.raises(AssertionError):
            X.check_exact(case, X.fake_launch(case, lambda m_: values))
    # the two store defects (module docstring): truncation is outside the bound wherever something is rounded; ties-away is caught
    # by bit equality in the power-of-two rows
    if case.desc["lk"] > 1:
        ratio, _ = _miss(case, X._round_bf16(a.ref, "trunc"))
        assert 1.0 < ratio < 2.0, f"{name}: a truncating store misses the bound by {ratio:.3g} x"
    if case.meta["variant"] == "spike" and len(case.meta["spike_keys"]) == 4:
        ratio, differ = _miss(case, X._round_bf16(a.ref, "away"))
        assert ratio <= 1.0 and differ > 0, (ratio, differ, a.pow2_ties)
        with pytest.raises(AssertionError, match="power-of-two denominator"):
            X.check_exact(case, X.fake_launch(case, lambda mode: X._round_bf16(a.ref, "away")))
        assert a.pow2_ties >= case.heads * case.d
