"""tests/_elementwise_ref.py pinned without a GPU, so that a wrong reference, a slack bound or a blind input cannot hide a wrong kernel.

1. Every float64 reference equals an independent formulation (the obvious torch expression; oracle/ccedit_oracle.py for the Gaussian
   sample).
2. For every operation an fp32 emulation of the kernel's own steps, rounded to bf16 where the kernel rounds, passes the bound the
   GPU test applies (tests/test_elementwise_gpu.py), on inputs drawn as that test draws them.
3. The same emulation with ONE planted defect misses it: the defect table below.
4. The host-side refusals of the ops wrappers that need no device to be shown.
"""
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _elementwise_ref as R  # noqa: E402
from _elementwise_ref import BF, F32, F64  # noqa: E402

TIMESTEP_DIMS = (2, 6, 250, 258, 320, 1280)
T_ALL = torch.arange(1000, dtype=torch.int64)


# ------------------------------------------------------------------------------------------
# 1. references against independent formulations
# ------------------------------------------------------------------------------------------
def test_ref_layout_changes_equal_permute():
    x = R.rnd_f32(2, 3, 3, 5, 7, seed=1)
    spb = torch.tensor([0.7, -1.3])
    got = R.ref_ncthw_to_nhwc(x, 8, spb, -0.5, 0.5)
    want = torch.zeros(6, 5, 7, 8, dtype=F64)
    want[..., :3] = (x.to(F64) * (spb.to(F64) * -0.5).view(2, 1, 1, 1, 1) + 0.5).permute(0, 2, 3, 4, 1).reshape(6, 5, 7, 3)
    assert torch.equal(got, want)
    y = R.rnd_f32(6, 5, 7, 16, seed=2)
    assert torch.equal(R.ref_nhwc_to_ncthw(y, 2, 3, 3), y[..., :3].reshape(2, 3, 5, 7, 3).permute(0, 4, 1, 2, 3).contiguous())
    yb = y.to(BF)
    assert torch.equal(R.ref_nhwc_to_ncthw(yb, 2, 3, 16), yb.float().reshape(2, 3, 5, 7, 16).permute(0, 4, 1, 2, 3).contiguous())


def test_ref_cat_add_add_and_embedding_equal_torch():
    a, b, c = (R.rnd_bf(121, n, seed=s).to(BF) for n, s in ((24, 1), (40, 2), (40, 3)))
    assert torch.equal(R.ref_cat_add(a, b, c), torch.cat([a.to(F64), b.to(F64) + c.to(F64)], dim=1))
    assert torch.equal(R.ref_cat_add(a, b, None), torch.cat([a, b], dim=1).to(F64))
    assert torch.equal(R.exact_cat_add(a, b, c), torch.cat([a, (b.float() + c.float()).to(BF)], dim=1))
    # the one-rounding result is within the bf16 bound of the float64 sum: the fp32 add in front of it is exact for these magnitudes
    R.assert_within(R.exact_cat_add(a, b, c), R.ref_cat_add(a, b, c), R.bound_bf16_exact_arith(R.ref_cat_add(a, b, c)), "cat_add")
    R.assert_within(R.exact_add(b, c), b.to(F64) + c.to(F64), R.bound_bf16_exact_arith(b.to(F64) + c.to(F64)), "add")
    g = torch.Generator().manual_seed(4)
    tok, pos = R.rnd_f32(100, 64, seed=5), R.rnd_f32(7, 64, seed=6)
    ids = torch.randint(0, 100, (3, 7), generator=g)
    ids[0, 0], ids[2, 6] = 0, 99
    want = torch.nn.functional.embedding(ids, tok) + pos[None]
    assert torch.equal(R.exact_embedding_lookup(ids, tok, pos), want.reshape(21, 64).to(BF))
    assert torch.equal(R.ref_embedding_lookup(ids, tok, pos), (torch.index_select(tok.to(F64), 0, ids.reshape(-1)).reshape(3, 7, 64)
                                                               + pos.to(F64)).reshape(21, 64))
    R.assert_within(R.exact_embedding_lookup(ids, tok, pos), R.ref_embedding_lookup(ids, tok, pos), R.bound_embedding_lookup(ids, tok, pos),
                    "embedding_lookup")


def test_ref_silu_timestep_softmax_equal_torch():
    x = R.all_bf16_in(-20.0, 20.0)
    assert x.numel() == 33602                     # 2 * (128 * 131 + 33) values, subnormals and both zeros included
    assert torch.allclose(R.ref_silu(x), torch.nn.functional.silu(x.to(F64)), rtol=1e-14, atol=0)
    for dim in TIMESTEP_DIMS:
        half = dim // 2
        freqs = torch.pow(torch.tensor(10000.0, dtype=F64), -torch.arange(half, dtype=F64) / half)
        args = T_ALL.to(F64)[:, None] * freqs[None]
        want = torch.cat([torch.cos(args), torch.sin(args)], dim=-1)
        assert (R.ref_timestep_embedding(T_ALL, dim) - want).abs().max() < 1e-12      # t f <= 999: 1e-13 in the argument
    for kind in R.SOFTMAX_KINDS:
        s = R.softmax_input(kind, 3, 300, 320, 0.37, seed=7)
        got = R.ref_softmax_rows(s, 300, 1024, 0.37)
        want = torch.softmax(s[:, :300].to(F64) * R.f32(0.37), dim=1)
        assert torch.allclose(got[:, :300], want, rtol=1e-13, atol=0) and not bool(got[:, 300:].any())


def test_ref_fp32_kernels_equal_torch_and_oracle():
    from oracle import ccedit_oracle as O
    wide, mom, noise = R.gaussian_inputs(3, 4, 5, 7, 16, seed=8)
    ref, mag = R.ref_gaussian_sample(mom, noise, 4, 0.18215)
    nchw = mom.to(F64).reshape(3, 5, 7, 8).permute(0, 3, 1, 2)
    want = O.gaussian_sample(nchw, noise.to(F64)) * R.f32(0.18215)
    assert torch.allclose(ref, want, rtol=1e-14, atol=0)
    assert bool((mag >= ref.abs() * (1 - 1e-12)).all())
    lv = mom[:, 4:]
    assert bool((lv < -30).any() and (lv == -30).any() and (lv == 20).any() and (lv > 20).any() and ((lv >= -6) & (lv <= 2)).any())
    x, z, m = R.rnd_f32(1000, seed=9), R.rnd_f32(1000, seed=10), torch.rand(1000, generator=torch.Generator().manual_seed(11))
    assert torch.allclose(R.ref_mask_blend(x, z, m)[0], torch.lerp(z.to(F64), x.to(F64), m.to(F64)), rtol=1e-13, atol=1e-15)
    e2 = torch.stack([R.rnd_f32(1000, seed=12), R.rnd_f32(1000, seed=13)])
    sg, sc = R.f32(14.6146), R.f32(7.5)
    du, dc = x.to(F64) - sg * e2[0].to(F64), x.to(F64) - sg * e2[1].to(F64)
    assert torch.allclose(R.ref_cfg_denoise(x, e2, 14.6146, 7.5)[0], torch.lerp(du, dc, torch.tensor(sc, dtype=F64)), rtol=1e-12, atol=1e-13)
    assert torch.equal(R.ref_axpby(x, z, 0.3, -1.7)[0], torch.add(R.f32(0.3) * x.to(F64), z.to(F64), alpha=R.f32(-1.7)))


def _as_strided_copy(src, dst, blocks, rows, row_elems):
    """RowShard._col_blocks on CPU tensors: its as_strided arm."""
    from ccedit_amd.parallel import RowShard
    return RowShard._col_blocks(types.SimpleNamespace(_plans={}), src, dst, blocks, None, rows, row_elems)


def test_copy_2d_blocks_emulation_equals_the_as_strided_arm():
    rows, c, world = 5, 64, 4
    cw = c // world
    qkv = R.rnd_bf(rows, 3 * c, seed=14).to(BF)
    want = R.sentinel_fill(world * 3 * rows * cw, BF).view(world * 3 * rows, cw)
    got = np.frombuffer(R.sentinel_fill(world * 3 * rows * cw, BF).view(torch.int16).numpy().tobytes(), dtype=np.uint8).copy()
    src = qkv.view(torch.int16).numpy().view(np.uint8).reshape(-1)
    for blocks in R.to_heads_blocks(rows, c, world):
        _as_strided_copy(qkv, want, blocks, rows, cw)
        R.emu_copy_2d_blocks(src, got, [(2 * a, 2 * b) for a, b in blocks], rows, 2 * cw, 2 * 3 * c, 2 * cw)
    assert not bool(R.is_sentinel(want).any())
    assert got.tobytes() == want.view(torch.int16).numpy().tobytes()


# ------------------------------------------------------------------------------------------
# 2. + 3. the correct fp32 emulation passes, one planted defect misses
# ------------------------------------------------------------------------------------------
def _passes(got, ref, bound):
    return R.excess(got, ref, bound) <= 1.0


def test_ncthw_to_nhwc_emulation_passes_and_nonzero_pad_fails():
    x, spb = R.rnd_f32(2, 3, 3, 5, 7, seed=20), torch.tensor([0.7, -1.3])
    for args in ((8, None, 1.0, 0.0), (8, spb, -0.5, 0.5), (16, spb, 1.0, 0.0)):
        ref, bound = R.ref_ncthw_to_nhwc(x, *args), R.bound_ncthw_to_nhwc(x, *args)
        assert _passes(R.emu_ncthw_to_nhwc(x, *args), ref, bound)
    args = (8, spb, -0.5, 0.5)
    assert not _passes(R.emu_ncthw_to_nhwc(x, *args, pad_garbage=True), R.ref_ncthw_to_nhwc(x, *args), R.bound_ncthw_to_nhwc(x, *args))
    assert torch.equal(R.emu_ncthw_to_nhwc(x, 3)[..., :3], x.permute(0, 2, 3, 4, 1).reshape(6, 5, 7, 3).to(BF))


def test_silu_emulation_passes_over_every_bf16_value():
    x = torch.cat([R.all_bf16_in(-3.0e38, 3.0e38)])
    ref, bound = R.ref_silu(x), R.bound_silu(x)
    for ieee in (False, True):
        got = R.emu_silu(x, ieee_div=ieee)
        assert bool(torch.isfinite(got.float()).all())
        assert _passes(got, ref, bound), R.excess(got, ref, bound)
        assert not bool(got.float()[R.silu_exp_overflows(x)].any())              # exactly +-0 where exp(-x) overflows fp32
    # results below 2^-126 are bf16 subnormals (quantum 2^-133): on them the two terms 2^-8 |ref| + 2^-22 |x| alone are missed by
    # the correct emulation, which is why bound_silu carries the flush term there — and only there
    sub = x[(x.abs() < 2.0 ** -125) & (x != 0)]                      # silu(x) = x / 2 there
    assert sub.numel() > 100 and bool((R.ref_silu(sub).abs() < 2.0 ** -126).all())
    two_terms = 2.0 ** -8 * R.ref_silu(sub).abs() + 2.0 ** -22 * sub.to(F64).abs()
    assert R.excess(R.emu_silu(sub), R.ref_silu(sub), two_terms) > 1.0
    normal = x[ref.abs() >= 2.0 ** -126]
    assert torch.equal(R.bound_silu(normal), 2.0 ** -8 * R.ref_silu(normal).abs() + 2.0 ** -22 * normal.to(F64).abs())
    # a SiLU that is subtly something else: the input off by one ulp of bf16 is far outside
    assert not _passes(R.emu_silu(x * (1 + 2.0 ** -7)), ref, bound)


def test_timestep_embedding_emulation_margin_and_defects():
    worst = 0.0
    for dim in TIMESTEP_DIMS:
        ref = R.ref_timestep_embedding(T_ALL, dim)
        bound = R.bound_timestep_embedding(ref)
        worst = max(worst, R.excess(R.emu_timestep_embedding(T_ALL, dim), ref, bound))
        if dim > 2:                       # half = 1 has only k = 0
            off = R.excess(R.emu_timestep_embedding(T_ALL, dim, k_off=1), ref, bound)
            assert off > 50.0, (dim, off)                                                      # frequency index off by one
        assert R.excess(R.emu_timestep_embedding(T_ALL, dim, swap=True), ref, bound) > 50.0    # cos and sin halves swapped
    print(f"timestep_embedding fp32 emulation: worst {worst:.3f} of the bound")
    assert worst <= 0.68, worst           # half a bf16 ulp just above |ref| = 1/2 is 2^-9 of 2^-9 + 2^-10 = 0.667; the fp32 argument adds the rest
    # the defect is loudest where the GPU test looks: t = 999
    ref = R.ref_timestep_embedding(T_ALL[-1:], 320)
    assert R.excess(R.emu_timestep_embedding(T_ALL[-1:], 320, k_off=1), ref, R.bound_timestep_embedding(ref)) > 50.0


SOFTMAX_CPU_CASES = [(3, 1, 64), (3, 63, 64), (3, 65, 128), (5, 257, 320), (5, 300, 1024), (3, 1000, 1024), (5, 8191, 8192), (5, 8192, 8192)]


@pytest.mark.parametrize("kind", R.SOFTMAX_KINDS)
def test_softmax_emulation_passes(kind):
    for rows, cols, cols_pad in SOFTMAX_CPU_CASES:
        for scale in (512 ** -0.5, 0.37):
            s = R.softmax_input(kind, rows, cols, cols + 3, scale, seed=cols)
            ref = R.ref_softmax_rows(s, cols, cols_pad, scale)
            got = R.emu_softmax_rows(s, cols, cols_pad, scale)
            e = R.excess(got, ref, R.bound_softmax_rows(ref))
            assert e <= 1.0, (kind, rows, cols, scale, e)
            assert not bool(got[:, cols:].float().any())
            assert bool(((got.to(F64).sum(dim=1) - 1.0).abs() <= 2.0 ** -8).all())
            if kind == "constant":
                assert torch.equal(got[:, :cols], torch.full((rows, cols), 1.0 / cols, dtype=F32).to(BF))


def test_softmax_defects_fail():
    scale = 512 ** -0.5
    # row max over the first 64 columns of the workgroup's share only: exp overflows on the rows whose maximum sits elsewhere
    # (softmax is invariant to the value subtracted until exp overflows: only the rows with a maximum 100 above the rest can show it)
    s = R.softmax_input("peaks", 5, 8192, 8192, scale, seed=1)
    ref = R.ref_softmax_rows(s, 8192, 8192, scale)
    assert not _passes(R.emu_softmax_rows(s, 8192, 8192, scale, max_first64=True), ref, R.bound_softmax_rows(ref))
    # a cross-wave maximum that drops one wave: each of the four is caught by the row whose peak sits in it
    s = R.softmax_input("peaks", 5, 8192, 8192, scale, seed=2)
    ref = R.ref_softmax_rows(s, 8192, 8192, scale)
    for wv in range(4):
        assert not _passes(R.emu_softmax_rows(s, 8192, 8192, scale, drop_wave=wv), ref, R.bound_softmax_rows(ref)), wv
    # pad columns not zeroed
    s = R.softmax_input("random", 3, 100, 100, scale, seed=3)
    ref = R.ref_softmax_rows(s, 100, 256, scale)
    assert _passes(R.emu_softmax_rows(s, 100, 256, scale), ref, R.bound_softmax_rows(ref))
    assert not _passes(R.emu_softmax_rows(s, 100, 256, scale, pad_garbage=True), ref, R.bound_softmax_rows(ref))


@pytest.mark.parametrize("zc,ldm", [(4, 8), (4, 16), (3, 8), (1, 2)])
def test_gaussian_sample_emulation_and_defects(zc, ldm):
    for frames, h, w in ((1, 1, 1), (3, 5, 7), (1, 64, 96)):
        for scale in (1.0, 0.18215):
            wide, mom, noise = R.gaussian_inputs(frames, zc, h, w, ldm, seed=h)
            ref, mag = R.ref_gaussian_sample(mom, noise, zc, scale)
            assert _passes(R.emu_gaussian_sample(mom, noise, zc, scale), ref, R.bound_terms(mag))
            # the lower clamp alone: every call has logvar = -45 (over a zero mean), also the single-element one
            assert not _passes(R.emu_gaussian_sample(mom, noise, zc, scale, clamp_low=False), ref, R.bound_terms(mag))
            if frames * h * w * zc >= 16:                                # every kind of logvar is present from 16 elements on
                assert not _passes(R.emu_gaussian_sample(mom, noise, zc, scale, clamp_high=False), ref, R.bound_terms(mag))
                assert not _passes(R.emu_gaussian_sample(mom, noise, zc, scale, clamp=False), ref, R.bound_terms(mag))
            if ldm > 2 * zc and frames * h * w > 1:
                assert not _passes(R.emu_gaussian_sample(wide, noise, zc, scale, ld_tight=True), ref, R.bound_terms(mag))


def test_gaussian_sample_clamp_shows_even_in_the_smallest_call():
    """1 x 1 pixel, one frame, zc = 4: four logvar values — the first four of the cycle, two of which clamp."""
    wide, mom, noise = R.gaussian_inputs(1, 4, 1, 1, 8, seed=1)
    ref, mag = R.ref_gaussian_sample(mom, noise, 4, 1.0)
    assert not _passes(R.emu_gaussian_sample(mom, noise, 4, 1.0, clamp=False), ref, R.bound_terms(mag))


def test_fp32_blend_kernels_emulation_and_defects():
    n = 1000
    x, z = R.rnd_f32(n, seed=30), R.rnd_f32(n, seed=31)
    m = torch.rand(n, generator=torch.Generator().manual_seed(32))
    ref, mag = R.ref_mask_blend(x, z, m)
    assert _passes(R.emu_mask_blend(x, z, m), ref, R.bound_terms(mag))
    assert not _passes(R.emu_mask_blend(x, z, m, swap=True), ref, R.bound_terms(mag))
    mb = (m > 0.5).float()                                               # binary masks: bit-equal to torch.where
    R.assert_bits_equal(R.emu_mask_blend(x, z, mb), torch.where(mb == 1, x, z), "mask_blend, binary mask")
    e2 = torch.stack([R.rnd_f32(n, seed=33), R.rnd_f32(n, seed=34)])
    for sigma in (14.6146, 1.0, 0.0292):
        for scale in (1.0, 7.5):
            ref, mag = R.ref_cfg_denoise(x, e2, sigma, scale)
            assert _passes(R.emu_cfg_denoise(x, e2, sigma, scale), ref, R.bound_terms(mag))
            # scale = 1 keeps only the conditional half, which the exchange turns into the unconditional one: it fails there too
            assert not _passes(R.emu_cfg_denoise(x, e2, sigma, scale, swap=True), ref, R.bound_terms(mag)), (sigma, scale)
    for a, b in ((0.3, -1.7), (1.0, 0.0), (0.0, 1.0), (1.0, -1.0)):
        zz = x * (1 + 2.0 ** -12) if (a, b) == (1.0, -1.0) else z       # cancellation: nearly equal inputs
        ref, mag = R.ref_axpby(x, zz, a, b)
        assert _passes(R.emu_axpby(x, zz, a, b), ref, R.bound_terms(mag))
        assert not _passes(R.emu_axpby(x, zz, a, b, swap=True), ref, R.bound_terms(mag))
    R.assert_bits_equal(R.emu_axpby(x, z, 1.0, 0.0), x, "axpby (1, 0)")
    R.assert_bits_equal(R.emu_axpby(x, z, 0.0, 1.0), z, "axpby (0, 1)")


def test_unwritten_tail_after_the_first_grid_pass_is_caught():
    """A grid-stride loop that stops after one pass leaves everything from item 2 097 152 on as it was.  The sentinel check sees it
    whatever the values would have been; so does the comparison (the sentinel is not a value the operation produces)."""
    n, guard = R.WRAP_ITEMS, 64
    assert n > R.GRID_ITEMS and n % 256 != 0 and (n - R.GRID_ITEMS) > 256
    written = torch.zeros(n + guard, dtype=torch.bool)
    written[:n] = True
    for dtype in (BF, F32):
        buf = R.sentinel_fill(n + guard, dtype)
        buf[:n] = 0                                                      # a complete launch: passes
        R.assert_sentinels(buf, written, "complete")
        buf[R.GRID_ITEMS:n] = R.sentinel_fill(1, dtype)[0]               # the defect
        with pytest.raises(AssertionError, match="never written"):
            R.assert_sentinels(buf, written, "one pass only")
        buf[:n] = 0
        buf[n] = 0                                                       # and one element too many
        with pytest.raises(AssertionError, match="outside the output"):
            R.assert_sentinels(buf, written, "overrun")
    x = R.rnd_f32(n, seed=40)
    ref, mag = R.ref_axpby(x, x, 0.5, 0.25)
    got = R.emu_axpby(x, x, 0.5, 0.25)
    got[R.GRID_ITEMS:] = 0.0                                             # an unwritten tail that happens to hold zeros
    assert not _passes(got, ref, R.bound_terms(mag))


def test_copy_2d_blocks_destination_pitch_defect_fails():
    rows, c, world = 6, 64, 4
    cw = c // world
    o = R.rnd_bf(world * rows, cw, seed=41).to(BF)
    want = R.sentinel_fill(rows * c, BF).view(rows, c)
    blocks = R.from_heads_blocks(rows, c, world)
    _as_strided_copy(o, want, blocks, rows, cw)
    src = o.view(torch.int16).numpy().view(np.uint8).reshape(-1)
    bb = [(2 * a, 2 * b) for a, b in blocks]
    sent = np.frombuffer(R.sentinel_fill(rows * c, BF).view(torch.int16).numpy().tobytes(), dtype=np.uint8)
    good = R.emu_copy_2d_blocks(src, sent.copy(), bb, rows, 2 * cw, 2 * cw, 2 * c)
    assert good.tobytes() == want.view(torch.int16).numpy().tobytes()
    bad = R.emu_copy_2d_blocks(src, sent.copy(), bb, rows, 2 * cw, 2 * cw, 2 * c, dst_uses_src_pitch=True)
    assert bad.tobytes() != want.view(torch.int16).numpy().tobytes()


def test_comparison_helpers_refuse_what_they_should():
    ref = torch.tensor([1.0, 0.0, -2.0], dtype=F64)
    bound = torch.tensor([0.1, 0.0, 0.1], dtype=F64)
    assert R.excess(ref.clone(), ref, bound) == 0.0
    assert R.excess(torch.tensor([1.0, 1e-30, -2.0]), ref, bound) == math.inf                  # zero bound: exact or nothing
    assert R.excess(torch.tensor([1.0, math.nan, -2.0]), ref, bound) == math.inf
    with pytest.raises(AssertionError, match="outside their bound"):
        R.assert_within(torch.tensor([1.2, 0.0, -2.0]), ref, bound, "x")
    with pytest.raises(AssertionError, match="differ in bits"):
        R.assert_bits_equal(torch.tensor([0.0]), torch.tensor([-0.0]), "signed zero")
    # two elements of similar size exchanged pass a global-max norm and fail here
    a = torch.tensor([1.00, 1.05, 3.0], dtype=F64)
    assert R.excess(a[[1, 0, 2]], a, 2.0 ** -8 * a.abs()) > 1.0


# ------------------------------------------------------------------------------------------
# 4. wrapper refusals that need no device: the check comes before anything touches the library
# ------------------------------------------------------------------------------------------
def test_wrappers_refuse_host_tensors_and_wrong_sizes_before_any_launch(monkeypatch):
    from ccedit_amd import hip, ops

    def no_library():
        raise AssertionError("the wrapper reached the kernel library")
    monkeypatch.setattr(hip, "lib", no_library)
    x, z = torch.zeros(12), torch.zeros(12)
    out = R.sentinel_fill(12, F32)
    for call in (lambda: ops.axpby(x, z, 1.0, 1.0, out=out),
                 lambda: ops.axpby(x, torch.zeros(11), 1.0, 1.0, out=out),
                 lambda: ops.axpby(x, z.double(), 1.0, 1.0, out=out),
                 lambda: ops.axpby(x, z, 1.0, 1.0, out=out[:11]),
                 lambda: ops.cfg_denoise(x, torch.zeros(2, 12), 1.0, 7.5),
                 lambda: ops.cfg_denoise(x, torch.zeros(2, 11), 1.0, 7.5),
                 lambda: ops.gaussian_sample(torch.zeros(6, 8), torch.zeros(1, 4, 2, 3), 4),
                 lambda: ops.gaussian_sample(torch.zeros(6, 7), torch.zeros(1, 4, 2, 3), 4)):
        with pytest.raises(ValueError):
            call()
    assert bool(R.is_sentinel(out).all())
