"""Every entry point of csrc/elementwise.hip on the device, element by element against the float64 references of
tests/_elementwise_ref.py (tests/test_elementwise_ref.py shows on the CPU that these checks pass a correct fp32 evaluation and miss
on each planted defect).

Each output goes into a buffer one guard region longer than needed, pre-filled with a sentinel (NaN bit patterns no kernel produces:
bf16 0x7FC0, fp32 0x7FC5A5A5): after the call no element of the output still holds it and every element outside the output still does.
Most kernels are called through the C ABI for that (caller's buffer, ld / ldp / pitch wider than the data) and again through the ops
wrapper, whose result must have the same bits; add and axpby go through their wrappers' out=, copy_2d_blocks through
RowShard._col_blocks, cat_add_gn through the C ABI alone.

"wrap" = just above 8192 * 256 = 2 097 152 work items and no multiple of 256: grid_for() caps the grid there, so every thread runs
a second pass of its grid-stride loop and the last workgroup is ragged.

  entry point                  test                          wrap  ragged  ld / pitch > data        clamps / edges                refusals
  ccedit_ncthw_to_nhwc         test_ncthw_to_nhwc[_wrap]     yes   yes     Cpad > C (zero pad)      scale_per_b, (1,0) bit-equal  -
  ccedit_nhwc_to_ncthw <bf16>  test_nhwc_to_ncthw[_wrap]     yes   yes     ld > c (NaN beyond c)    bit-equal                     wrapper: b*t, c > ld
  ccedit_nhwc_to_ncthw <fp32>  test_nhwc_to_ncthw[_wrap]     yes   yes     ld > c (NaN beyond c)    bit-equal                     wrapper: b*t, c > ld
  ccedit_cat_add               test_cat_add[_wrap]           yes   yes     -                        c = None, one rounding        -
  ccedit_cat_add_gn            test_cat_add_gn_output        -     yes     -                        RS 4 / 4 / 1, 64-thread floor -
  ccedit_add                   test_add                      yes   yes     -                        out = a (in place)            n % 8
  ccedit_silu                  test_silu                     yes   yes     -                        exp overflow, +-0, +-1e4      -
  ccedit_timestep_embedding    test_timestep_embedding       -     half 1 / 125 / 129  ld > dim     t = 0 .. 999                  odd dim
  ccedit_embedding_lookup      test_embedding_lookup[_wrap]  yes   yes     -                        ids 0 and vocab - 1           wrapper: id range
  ccedit_gaussian_sample       test_gaussian_sample[_wrap]   yes   yes     ldm > 2 zc (NaN beyond)  logvar < -30, = -30, = 20, > 20  wrapper: columns, device
  ccedit_mask_blend            test_mask_blend               yes   yes     -                        m in {0, 1} bit-equal         -
  ccedit_cfg_denoise           test_cfg_denoise              yes   yes     -                        schedule ends, scale 1        wrapper: numel, device
  ccedit_axpby                 test_axpby                    yes   yes     -                        (1,0) (0,1) bit-equal, cancellation, out = x  wrapper: numel, dtype, device
  ccedit_softmax_rows          test_softmax_rows             -     cols 1 .. 8192  lds > cols (inf / NaN), ldp > cols_pad  +-80 span, peak per wave  cols_pad > 8192; wrapper: columns
  ccedit_copy_2d_blocks        test_copy_2d_blocks[_grid_cap]  yes (137 workgroups x several passes; 1024-workgroup cap)  yes  both pitches > row  16-byte rows, fp32  row_bytes / pitch % 16, pitch < row
  ccedit_copy_row_blocks       tests/test_ops_gpu.py: test_copy_row_blocks_pack_unpack_add (bit-equal already)
"""
import math
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _elementwise_ref as R  # noqa: E402
from _elementwise_ref import BF, F32, F64, WRAP_ITEMS  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 4096            # elements behind every output


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _call(name, *args):
    from ccedit_amd import hip, ops
    hip.check(getattr(hip.lib(), name)(*args, ops._stream()), name)


def _refused(name, *args):
    from ccedit_amd import hip
    with pytest.raises(hip.HipLibraryError):
        _call(name, *args)


def _out(numel, dtype):
    return R.sentinel_fill(numel + GUARD, dtype, "cuda")


def _take(buf, numel, what, written=None):
    """The first `numel` elements of a guarded buffer on the CPU, after the sentinel check (written: mask over those elements)."""
    host = buf.cpu()
    mask = torch.zeros(buf.numel(), dtype=torch.bool)
    mask[:numel] = True if written is None else written.reshape(-1)
    R.assert_sentinels(host, mask, what)
    return host[:numel]


def _untouched(buf, what):
    R.assert_sentinels(buf.cpu(), torch.zeros(buf.numel(), dtype=torch.bool), what)


def _p(t):
    return None if t is None else t.data_ptr()


# ------------------------------------------------------------------------------------------
# layout changes
# ------------------------------------------------------------------------------------------
def _ncthw_case(x, cpad, spb, scale, shift, what):
    from ccedit_amd import ops
    b, c, t, h, w = x.shape
    n = b * t * h * w * cpad
    xd, sd = x.cuda(), None if spb is None else spb.cuda()
    buf = _out(n, BF)
    _call("ccedit_ncthw_to_nhwc", xd.data_ptr(), buf.data_ptr(), b, c, t, h, w, cpad, _p(sd), scale, shift)
    got = _take(buf, n, what).view(b * t, h, w, cpad)
    ref = R.ref_ncthw_to_nhwc(x, cpad, spb, scale, shift)
    if spb is None and (scale, shift) == (1.0, 0.0):
        R.assert_bits_equal(got, ref.to(BF), what + " (no arithmetic: the rounded input)")
    R.assert_within(got, ref, R.bound_ncthw_to_nhwc(x, cpad, spb, scale, shift), what)
    assert not bool(got[..., c:].contiguous().view(torch.int16).any()), what + ": pad channels are not +0"
    R.assert_bits_equal(ops.ncthw_to_nhwc(xd, cpad, sd, scale, shift).cpu(), got, what + " (wrapper)")


@pytest.mark.parametrize("c,cpad", [(4, 8), (3, 8), (8, 8), (1, 1), (5, 16)])
@pytest.mark.parametrize("per_b", [False, True])
@pytest.mark.parametrize("scale,shift", [(1.0, 0.0), (-0.5, 0.5)])
def test_ncthw_to_nhwc(c, cpad, per_b, scale, shift):
    _dev()
    x = R.rnd_f32(2, c, 3, 5, 7, seed=c)
    _ncthw_case(x, cpad, torch.tensor([0.7, -1.3]) if per_b else None, scale, shift, f"ncthw_to_nhwc C={c} Cpad={cpad}")


def test_ncthw_to_nhwc_wrap():
    _dev()
    x = R.rnd_f32(2, 3, 3, 600, 584, seed=1)
    assert 2 * 3 * 600 * 584 > R.GRID_ITEMS + 256 and (2 * 3 * 600 * 584) % 256
    _ncthw_case(x, 8, torch.tensor([0.7, -1.3]), -0.5, 0.5, "ncthw_to_nhwc wrap")


def _nhwc_case(f32_in, b, t, h, w, c, ld, what):
    from ccedit_amd import ops
    x = R.rnd_f32(b * t, h, w, ld, seed=ld + c) if f32_in else R.rnd_bf(b * t, h, w, ld, seed=ld + c)
    x[..., c:] = math.nan                                    # a read of an unused channel shows
    x = x if f32_in else x.to(BF)
    n = b * c * t * h * w
    xd = x.cuda()
    buf = _out(n, F32)
    _call("ccedit_nhwc_to_ncthw", xd.data_ptr(), int(f32_in), ld, buf.data_ptr(), b, c, t, h, w)
    got = _take(buf, n, what).view(b, c, t, h, w)
    R.assert_bits_equal(got, R.ref_nhwc_to_ncthw(x, b, t, c), what)
    R.assert_bits_equal(ops.nhwc_to_ncthw(xd, b, t, c).cpu(), got, what + " (wrapper)")


@pytest.mark.parametrize("f32_in", [False, True], ids=["bf16", "fp32"])
@pytest.mark.parametrize("c,ld", [(8, 8), (4, 8), (3, 16)])
@pytest.mark.parametrize("b,t", [(2, 3), (1, 1)])
def test_nhwc_to_ncthw(f32_in, c, ld, b, t):
    _dev()
    _nhwc_case(f32_in, b, t, 5, 7, c, ld, f"nhwc_to_ncthw {'fp32' if f32_in else 'bf16'} c={c} ld={ld} b={b} t={t}")


@pytest.mark.parametrize("f32_in", [False, True], ids=["bf16", "fp32"])
def test_nhwc_to_ncthw_wrap(f32_in):
    _dev()
    b, t, h, w, c = 1, 3, 1, 233_103, 3
    assert b * c * t * h * w > R.GRID_ITEMS + 256 and (b * c * t * h * w) % 256
    _nhwc_case(f32_in, b, t, h, w, c, 4, "nhwc_to_ncthw wrap")


# ------------------------------------------------------------------------------------------
# concatenation and adds: exact (one fp32 add, one rounding)
# ------------------------------------------------------------------------------------------
def _cat_add_case(rows, c1, c2, with_c, what):
    from ccedit_amd import ops
    a, b = R.rnd_bf(rows, c1, seed=1).to(BF), R.rnd_bf(rows, c2, seed=2).to(BF)
    c = R.rnd_bf(rows, c2, seed=3).to(BF) if with_c else None
    ad, bd, cd = a.cuda(), b.cuda(), None if c is None else c.cuda()
    n = rows * (c1 + c2)
    buf = _out(n, BF)
    _call("ccedit_cat_add", ad.data_ptr(), bd.data_ptr(), _p(cd), buf.data_ptr(), rows, c1, c2)
    got = _take(buf, n, what).view(rows, c1 + c2)
    R.assert_bits_equal(got[:, :c1].contiguous(), a, what + ": the a half")
    R.assert_bits_equal(got, R.exact_cat_add(a, b, c), what)
    ref = R.ref_cat_add(a, b, c)
    R.assert_within(got, ref, R.bound_bf16_exact_arith(ref), what)
    R.assert_bits_equal(ops.cat_add(ad, bd, cd).cpu(), got, what + " (wrapper)")


@pytest.mark.parametrize("c1,c2", [(64, 32), (8, 8), (320, 320), (640, 320), (24, 40)])
@pytest.mark.parametrize("with_c", [True, False])
def test_cat_add(c1, c2, with_c):
    _dev()
    _cat_add_case(5 * 4 * 6 + 1, c1, c2, with_c, f"cat_add {c1}+{c2} c={with_c}")


def test_cat_add_wrap():
    _dev()
    rows = 26_225
    assert rows * 80 > R.GRID_ITEMS + 256 and (rows * 80) % 256
    _cat_add_case(rows, 320, 320, True, "cat_add wrap")


@pytest.mark.parametrize("c1,c2,hw", [(32, 32, 9), (320, 320, 48 * 2 + 1), (1280, 1280, 70)])
def test_cat_add_gn_output(c1, c2, hw):
    """The tensor the fused kernel writes is the one the plain kernel writes (its statistics are tests/test_ops_gpu.py's and
    tests/test_exact_gpu.py's business): RS = 4 / 4 / 1 rows side by side, the 64-thread floor at 64 channels, the
    four-rows-in-flight loop and its remainder.  Through the C ABI, so no policy setting decides whether the kernel runs."""
    _dev()
    frames = 2
    rows, n = frames * hw, frames * hw * (c1 + c2)
    a, b, c = (R.rnd_bf(rows, ch, seed=s).to(BF) for ch, s in ((c1, 1), (c2, 2), (c2, 3)))
    ad, bd, cd = a.cuda(), b.cuda(), c.cuda()
    for cc, ccd in ((c, cd), (None, None)):
        what = f"cat_add_gn {c1}+{c2} hw={hw} c={cc is not None}"
        stats = torch.zeros(frames, 64, dtype=F64, device="cuda")
        buf = _out(n, BF)
        _call("ccedit_cat_add_gn", ad.data_ptr(), bd.data_ptr(), _p(ccd), buf.data_ptr(), stats.data_ptr(), frames, hw, c1, c2)
        got = _take(buf, n, what).view(rows, c1 + c2)
        plain = _out(n, BF)
        _call("ccedit_cat_add", ad.data_ptr(), bd.data_ptr(), _p(ccd), plain.data_ptr(), rows, c1, c2)
        R.assert_bits_equal(got, _take(plain, n, what + " (plain kernel)").view(rows, c1 + c2), what + " against ccedit_cat_add")
        R.assert_bits_equal(got, R.exact_cat_add(a, b, cc), what)
        # the statistics belong to other tests; here only that they are those of the tensor written: per frame the 32 sums and the total
        sums = stats.cpu().view(frames, 32, 2)[:, :, 0].sum(dim=1)
        want = got.to(F64).view(frames, -1).sum(dim=1)
        assert bool(((sums - want).abs() <= 1e-4 * got.to(F64).abs().view(frames, -1).sum(dim=1)).all()), what + ": statistics of another tensor"


@pytest.mark.parametrize("n", [8, 8 * 255, 8 * 257, 8 * (R.GRID_ITEMS + 77)], ids=["8", "8x255", "8x257", "wrap"])
def test_add(n):
    _dev()
    from ccedit_amd import ops
    a, b = R.rnd_bf(n, seed=1).to(BF), R.rnd_bf(n, seed=2).to(BF)
    ad, bd = a.cuda(), b.cuda()
    want = R.exact_add(a, b)
    buf = _out(n, BF)
    out = buf[:n]
    assert ops.add(ad, bd, out=out) is out
    got = _take(buf, n, f"add n={n}")
    R.assert_bits_equal(got, want, f"add n={n}")
    ref = a.to(F64) + b.to(F64)
    R.assert_within(got, ref, R.bound_bf16_exact_arith(ref), f"add n={n}")
    R.assert_bits_equal(ops.add(ad, bd).cpu(), want, "add, fresh output")
    ops.add(ad, bd, out=ad)                                                   # in place
    R.assert_bits_equal(ad.cpu(), want, "add, out = a")


def test_add_refuses_a_ragged_length():
    _dev()
    from ccedit_amd import hip, ops
    a = R.rnd_bf(20, seed=1).to(BF).cuda()
    buf = _out(20, BF)
    with pytest.raises(hip.HipLibraryError, match="multiple of 8"):
        ops.add(a[:12], a[:12], out=buf[:12])
    _untouched(buf, "add n=12")


@pytest.mark.parametrize("n", [1, 255, 257, WRAP_ITEMS], ids=["1", "255", "257", "wrap"])
def test_silu(n):
    _dev()
    from ccedit_amd import ops
    x = R.rnd_bf(n, seed=n % 1000, scale=3.0)
    got = _silu_case(x, f"silu n={n}")
    R.assert_bits_equal(ops.silu(x.to(BF).cuda()).cpu(), got, "silu (wrapper)")


def _silu_case(x, what):
    n = x.numel()
    xd = x.to(BF).cuda()
    buf = _out(n, BF)
    _call("ccedit_silu", xd.data_ptr(), buf.data_ptr(), n)
    got = _take(buf, n, what)
    assert bool(torch.isfinite(got.float()).all()), what + ": non-finite output"
    R.assert_within(got, R.ref_silu(x), R.bound_silu(x), what)
    over = R.silu_exp_overflows(x)
    assert not bool(got.float()[over].any()), what + ": not a zero where exp(-x) overflows fp32"
    return got


def test_silu_edges_and_every_bf16_value_up_to_20():
    _dev()
    edges = torch.tensor([0.0, -0.0, 88.0, -88.0, 100.0, -100.0, 1e4, -1e4, 3e38, -3e38]).to(BF).float()
    x = torch.cat([edges, R.all_bf16_in(-20.0, 20.0)])
    assert bool(R.silu_exp_overflows(x).any())
    got = _silu_case(x, "silu sweep")
    assert got[0].view(torch.int16).item() == 0 and got[1].view(torch.int16).item() == -32768, "silu(+-0) is not +-0"


@pytest.mark.parametrize("dim", [2, 6, 250, 258, 320, 1280])
def test_timestep_embedding(dim):
    """half = 1 (smallest), 125 (idle threads), 129 (one thread loops twice), 160, 640; every t of the schedule in one call."""
    _dev()
    from ccedit_amd import ops
    t = torch.arange(1000, dtype=torch.int64)
    td = t.cuda()
    ref = R.ref_timestep_embedding(t, dim)
    buf = _out(1000 * dim, BF)
    _call("ccedit_timestep_embedding", td.data_ptr(), buf.data_ptr(), 1000, dim, dim)
    got = _take(buf, 1000 * dim, f"timestep_embedding dim={dim}").view(1000, dim)
    R.assert_within(got, ref, R.bound_timestep_embedding(ref), f"timestep_embedding dim={dim}")
    R.assert_bits_equal(ops.timestep_embedding(td, dim).cpu(), got, "timestep_embedding (wrapper)")


def test_timestep_embedding_wide_rows_and_odd_dim():
    _dev()
    t = torch.arange(1000, dtype=torch.int64)
    td = t.cuda()
    dim, ld = 320, 384
    buf = _out(1000 * ld, BF)
    _call("ccedit_timestep_embedding", td.data_ptr(), buf.data_ptr(), 1000, dim, ld)
    written = torch.zeros(1000, ld, dtype=torch.bool)
    written[:, :dim] = True
    got = _take(buf, 1000 * ld, "timestep_embedding ld=384", written).view(1000, ld)[:, :dim]
    ref = R.ref_timestep_embedding(t, dim)
    R.assert_within(got, ref, R.bound_timestep_embedding(ref), "timestep_embedding ld=384")
    buf = _out(1000 * 321, BF)
    _refused("ccedit_timestep_embedding", td.data_ptr(), buf.data_ptr(), 1000, 321, 321)
    _untouched(buf, "timestep_embedding odd dim")


def _embedding_case(vocab, l, c, b, what):
    from ccedit_amd import ops
    g = torch.Generator().manual_seed(vocab + b)
    tok, pos = R.rnd_f32(vocab, c, seed=1), R.rnd_f32(l, c, seed=2)
    ids = torch.randint(0, vocab, (b, l), generator=g)
    ids[0, 0], ids[-1, -1] = vocab - 1, 0
    if l > 1:
        ids[0, 1] = 0
        ids[-1, 0] = vocab - 1
    idd, tokd, posd = ids.cuda(), tok.cuda(), pos.cuda()
    n = b * l * c
    buf = _out(n, BF)
    _call("ccedit_embedding_lookup", idd.data_ptr(), tokd.data_ptr(), posd.data_ptr(), buf.data_ptr(), b * l, l, c, vocab)
    got = _take(buf, n, what).view(b * l, c)
    R.assert_bits_equal(got, R.exact_embedding_lookup(ids, tok, pos), what)
    R.assert_bits_equal(got, (tok[ids] + pos).to(BF).view(b * l, c), what)
    R.assert_bits_equal(ops.embedding_lookup(idd, tokd, posd).cpu(), got, what + " (wrapper)")
    return idd, tokd, posd


@pytest.mark.parametrize("vocab,l,c", [(100, 7, 64), (49408, 77, 768), (5, 1, 8)])
@pytest.mark.parametrize("b", [1, 3])
def test_embedding_lookup(vocab, l, c, b):
    _dev()
    _embedding_case(vocab, l, c, b, f"embedding_lookup vocab={vocab} L={l} C={c} B={b}")


def test_embedding_lookup_wrap_and_id_range(monkeypatch):
    _dev()
    from ccedit_amd import hip, ops
    assert 286 * 77 * 96 > R.GRID_ITEMS + 256 and (286 * 77 * 96) % 256
    idd, tokd, posd = _embedding_case(100, 77, 768, 286, "embedding_lookup wrap")

    def no_library():
        raise AssertionError("the wrapper reached the kernel library")
    monkeypatch.setattr(hip, "lib", no_library)
    for bad in (-1, 100):
        ids = idd.clone()
        ids[3, 5] = bad
        with pytest.raises(ValueError, match="token id"):
            ops.embedding_lookup(ids, tokd, posd)


# ------------------------------------------------------------------------------------------
# fp32 kernels
# ------------------------------------------------------------------------------------------
def _gaussian_case(frames, zc, h, w, ldm, scale, what):
    from ccedit_amd import ops
    wide, mom, noise = R.gaussian_inputs(frames, zc, h, w, ldm, seed=h + frames)
    wd, nd = wide.cuda(), noise.cuda()
    n = noise.numel()
    buf = _out(n, F32)
    _call("ccedit_gaussian_sample", wd.data_ptr(), nd.data_ptr(), buf.data_ptr(), frames, zc, h * w, ldm, scale)
    got = _take(buf, n, what).view(noise.shape)
    ref, mag = R.ref_gaussian_sample(mom, noise, zc, scale)
    R.assert_within(got, ref, R.bound_terms(mag), what)
    R.assert_bits_equal(ops.gaussian_sample(wd[:, :2 * zc], nd, zc, scale).cpu(), got, what + " (wrapper, column-slice view)")


@pytest.mark.parametrize("zc,ldm", [(4, 8), (4, 16), (3, 8), (1, 2)])
def test_gaussian_sample(zc, ldm):
    _dev()
    for frames in (1, 3):
        for h, w in ((1, 1), (5, 7), (64, 96)):
            for scale in (1.0, 0.18215):
                _gaussian_case(frames, zc, h, w, ldm, scale, f"gaussian_sample zc={zc} ldm={ldm} frames={frames} {h}x{w} scale={scale}")


def test_gaussian_sample_wrap():
    _dev()
    assert 3 * 4 * 419 * 419 > R.GRID_ITEMS + 256 and (3 * 4 * 419 * 419) % 256
    _gaussian_case(3, 4, 419, 419, 8, 0.18215, "gaussian_sample wrap")


def _rand01(n, seed):
    return torch.rand(n, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("n", [1, 1000, WRAP_ITEMS], ids=["1", "1000", "wrap"])
def test_mask_blend(n):
    _dev()
    from ccedit_amd import ops
    x, z = R.rnd_f32(n, seed=1), R.rnd_f32(n, seed=2)
    xd, zd = x.cuda(), z.cuda()
    for kind in ("binary", "fractional"):
        m = (_rand01(n, 3) > 0.5).float() if kind == "binary" else _rand01(n, 4)
        if kind == "fractional" and n >= 4:
            m[:4] = torch.tensor([0.0, 1.0, 2.0 ** -24, 1.0 - 2.0 ** -24])
        md = m.cuda()
        buf = _out(n, F32)
        _call("ccedit_mask_blend", xd.data_ptr(), zd.data_ptr(), md.data_ptr(), buf.data_ptr(), n)
        got = _take(buf, n, f"mask_blend n={n} {kind}")
        if kind == "binary":
            R.assert_bits_equal(got, torch.where(m == 1, x, z), f"mask_blend n={n}, m in {{0, 1}}")
        ref, mag = R.ref_mask_blend(x, z, m)
        R.assert_within(got, ref, R.bound_terms(mag), f"mask_blend n={n} {kind}")
        R.assert_bits_equal(ops.mask_blend(xd, zd, md).cpu(), got, "mask_blend (wrapper)")


def test_mask_blend_broadcast_mask_of_a_latent():
    """The call of the inpainting sampler: a (B, 1, T, H, W) mask, expand_as(x).contiguous(), against a (B, 4, T, H, W) latent."""
    _dev()
    from ccedit_amd import ops
    b, t, h, w = 2, 3, 5, 7
    x, z = R.rnd_f32(b, 4, t, h, w, seed=1), R.rnd_f32(b, 4, t, h, w, seed=2)
    m1 = (_rand01(b * t * h * w, 3) > 0.4).float().view(b, 1, t, h, w)
    got = ops.mask_blend(x.cuda(), z.cuda(), m1.cuda().expand_as(x).contiguous()).cpu()
    R.assert_bits_equal(got, torch.where(m1.expand_as(x) == 1, x, z), "mask_blend, broadcast binary mask")


@pytest.mark.parametrize("n", [1, 1000, WRAP_ITEMS], ids=["1", "1000", "wrap"])
def test_cfg_denoise(n):
    _dev()
    from ccedit_amd import ops
    x = R.rnd_f32(n, seed=1)
    e2 = torch.stack([R.rnd_f32(n, seed=2), R.rnd_f32(n, seed=3)])            # two seeds: exchanged halves differ
    xd, ed = x.cuda(), e2.cuda()
    for sigma in (14.6146, 1.0, 0.0292):
        for scale in (1.0, 7.5):
            what = f"cfg_denoise n={n} sigma={sigma} scale={scale}"
            buf = _out(n, F32)
            _call("ccedit_cfg_denoise", xd.data_ptr(), ed.data_ptr(), buf.data_ptr(), n, sigma, scale)
            got = _take(buf, n, what)
            ref, mag = R.ref_cfg_denoise(x, e2, sigma, scale)
            R.assert_within(got, ref, R.bound_terms(mag), what)
            if n <= 1000 or (sigma, scale) == (14.6146, 7.5):
                R.assert_bits_equal(ops.cfg_denoise(xd, ed, sigma, scale).cpu(), got, what + " (wrapper)")


@pytest.mark.parametrize("n", [1, 1000, WRAP_ITEMS], ids=["1", "1000", "wrap"])
def test_axpby(n):
    _dev()
    from ccedit_amd import ops
    x, z = R.rnd_f32(n, seed=1), R.rnd_f32(n, seed=2)
    near = x * (1 + 2.0 ** -12)                                               # (1, -1): cancellation
    xd, zd, neard = x.cuda(), z.cuda(), near.cuda()
    for a, b in ((0.3, -1.7), (1.0, 0.0), (0.0, 1.0), (1.0, -1.0)):
        what = f"axpby n={n} a={a} b={b}"
        zz, zzd = (near, neard) if (a, b) == (1.0, -1.0) else (z, zd)
        buf = _out(n, F32)
        out = buf[:n]
        assert ops.axpby(xd, zzd, a, b, out=out) is out
        got = _take(buf, n, what)
        ref, mag = R.ref_axpby(x, zz, a, b)
        R.assert_within(got, ref, R.bound_terms(mag), what)
        if (a, b) == (1.0, 0.0):
            R.assert_bits_equal(got, x, what)
        if (a, b) == (0.0, 1.0):
            R.assert_bits_equal(got, z, what)
        R.assert_bits_equal(ops.axpby(xd, zzd, a, b).cpu(), got, what + ", fresh output")
    xa = xd.clone()
    ops.axpby(xa, zd, 0.3, -1.7, out=xa)                                      # in place
    ref, mag = R.ref_axpby(x, z, 0.3, -1.7)
    R.assert_within(xa.cpu(), ref, R.bound_terms(mag), f"axpby n={n}, out = x")


# ------------------------------------------------------------------------------------------
# softmax_rows (bf16 out)
# ------------------------------------------------------------------------------------------
def _ceil64(n):
    return (n + 63) // 64 * 64


@pytest.mark.parametrize("cols,cols_pad", [(c, _ceil64(c)) for c in (1, 63, 64, 65, 255, 256, 257, 1000, 4096, 8191, 8192)]
                         + [(100, 256), (300, 1024)])
def test_softmax_rows(cols, cols_pad):
    _dev()
    from ccedit_amd import ops
    lds, ldp = cols + 5, cols_pad + 64
    for rows in (1, 3, 70):
        for scale in (512 ** -0.5, 0.37):
            for kind in R.SOFTMAX_KINDS:
                what = f"softmax_rows {kind} rows={rows} cols={cols} cols_pad={cols_pad} scale={scale:.4g}"
                s = R.softmax_input(kind, rows, cols, lds, scale, seed=rows + cols)
                sd = s.cuda()
                buf = _out(rows * ldp, BF)
                _call("ccedit_softmax_rows", sd.data_ptr(), buf.data_ptr(), rows, cols, cols_pad, lds, ldp, scale)
                written = torch.zeros(rows, ldp, dtype=torch.bool)
                written[:, :cols_pad] = True
                got = _take(buf, rows * ldp, what, written).view(rows, ldp)[:, :cols_pad]
                ref = R.ref_softmax_rows(s, cols, cols_pad, scale)
                R.assert_within(got, ref, R.bound_softmax_rows(ref), what)
                assert not bool(got[:, cols:].contiguous().view(torch.int16).any()), what + ": pad columns are not +0"
                dev = (got.to(F64).sum(dim=1) - 1.0).abs().max().item()
                assert dev <= 2.0 ** -8, f"{what}: a row sums to 1 -+ {dev:.3g}"
                if kind == "constant":
                    R.assert_bits_equal(got[:, :cols].contiguous(), torch.full((rows, cols), 1.0 / cols, dtype=F32).to(BF), what)
                if rows == 3:
                    R.assert_bits_equal(ops.softmax_rows(sd, cols, cols_pad, scale).cpu(), got.contiguous(), what + " (wrapper)")


def test_softmax_rows_refuses_more_than_8192_columns():
    _dev()
    s = R.rnd_f32(2, 8256, seed=1).cuda()
    buf = _out(2 * 8256, BF)
    _refused("ccedit_softmax_rows", s.data_ptr(), buf.data_ptr(), 2, 8192, 8256, 8256, 8256, 1.0)
    _refused("ccedit_softmax_rows", s.data_ptr(), buf.data_ptr(), 2, 8256, 8256, 8256, 8256, 1.0)
    _untouched(buf, "softmax_rows cols_pad=8256")


# ------------------------------------------------------------------------------------------
# copy_2d_blocks: the column gather / scatter of RowShard.to_heads / from_heads
# ------------------------------------------------------------------------------------------
def _col_blocks(src, dst, blocks, rows, row_elems):
    """RowShard._col_blocks itself: the kernel with a plan of byte offsets for device tensors, as_strided copies for host tensors."""
    from ccedit_amd.parallel import RowShard
    return RowShard._col_blocks(types.SimpleNamespace(_plans={}), src, dst, blocks, "plan", rows, row_elems)


def _guarded_2d(rows, cols, dtype, device):
    buf = R.sentinel_fill(rows * cols + GUARD, dtype, device)
    return buf, buf[:rows * cols].view(rows, cols)


def _both_arms(src, dst_shape, plans, rows, row_elems, what):
    """The same plans through the kernel and through the as_strided arm, into sentinel-filled destinations: equal bits everywhere,
    the bytes outside every block and the guard region included."""
    bufs = []
    for device in ("cuda", "cpu"):
        buf, dst = _guarded_2d(*dst_shape, src.dtype, device)
        s = src.to(device)
        for blocks in plans:
            _col_blocks(s, dst, blocks, rows, row_elems)
        bufs.append(buf.cpu())
    R.assert_bits_equal(bufs[0], bufs[1], what)
    return bufs[1][:dst_shape[0] * dst_shape[1]].view(dst_shape)


@pytest.mark.parametrize("rows,c,world,dtype", [(34 * 12, 320, 4, BF), (1, 64, 8, BF), (2051, 640, 2, BF), (7001, 640, 2, BF), (37, 64, 4, F32)],
                         ids=["408x320/4", "1x64/8-one-granule", "2051x640/2", "7001x640/2-wrap", "fp32"])
def test_copy_2d_blocks(rows, c, world, dtype):
    _dev()
    cw = c // world
    if (rows, c, world) == (1, 64, 8):
        assert cw * 2 == 16                                                  # row_bytes = 16: one granule
    if rows == 7001:
        # 280 040 granules: 137 workgroups (about 8 granules per thread), eight passes of the loop and a ragged last one.  The cap of
        # 1024 workgroups is not reached here: test_copy_2d_blocks_grid_cap
        assert rows * (cw * 2 // 16) > 1024 * 256
    qkv = R.rnd_bf(rows, 3 * c, seed=1).to(dtype)
    # to_heads: [rows, 3C] -> contiguous [world * 3 * rows, cw]
    send = _both_arms(qkv, (world * 3 * rows, cw), R.to_heads_blocks(rows, c, world), rows, cw, "to_heads gather")
    assert not bool(R.is_sentinel(send).any())
    for r in range(world):
        for j in range(3):
            R.assert_bits_equal(send[(r * 3 + j) * rows:(r * 3 + j + 1) * rows].contiguous(),
                                qkv[:, j * c + r * cw: j * c + (r + 1) * cw].contiguous(), f"to_heads rank {r} part {j}")
    # and back: the inverse plans scatter the buffers into the columns of [rows, 3C]
    back = _both_arms(send, (rows, 3 * c), [[(b, a) for a, b in blocks] for blocks in R.to_heads_blocks(rows, c, world)], rows, cw, "scatter back")
    R.assert_bits_equal(back, qkv, "to_heads and back")
    # from_heads: [world * rows, cw] -> the columns of [rows, C]; only the first world - 1 blocks, so that columns stay unwritten
    o = R.rnd_bf(world * rows, cw, seed=2).to(dtype)
    out = _both_arms(o, (rows, c), [R.from_heads_blocks(rows, c, world)[:-1]], rows, cw, "from_heads scatter")
    assert bool(R.is_sentinel(out[:, (world - 1) * cw:]).all()) and not bool(R.is_sentinel(out[:, :(world - 1) * cw]).any())
    R.assert_bits_equal(out[:, :cw].contiguous(), o[:rows], "from_heads rank 0")


def test_copy_2d_blocks_grid_cap():
    """More than 1024 * 2048 granules in a block: ceil(rows * row_gran / 2048) workgroups would be 1026, the launch is capped at
    1024, and every thread runs a ninth pass for the rest.  The from_heads scatter at 640-byte rows."""
    _dev()
    rows, c, world = 52_501, 640, 2
    cw = c // world
    assert rows * (cw * 2 // 16) > 1024 * 2048 and (rows * (cw * 2 // 16)) % 256
    o = R.rnd_bf(world * rows, cw, seed=3).to(BF)
    out = _both_arms(o, (rows, c), [R.from_heads_blocks(rows, c, world)], rows, cw, "from_heads scatter, capped grid")
    assert not bool(R.is_sentinel(out).any())
    for r in range(world):
        R.assert_bits_equal(out[:, r * cw:(r + 1) * cw].contiguous(), o[r * rows:(r + 1) * rows], f"from_heads rank {r}")


def test_copy_2d_blocks_refusals():
    _dev()
    src = R.rnd_bf(8, 64, seed=1).to(BF).cuda()
    buf = _out(8 * 64, BF)
    plan = torch.tensor([[0, 0]], dtype=torch.int64, device="cuda")
    for row_bytes, sp, dp in ((24, 128, 128), (32, 120, 128), (32, 128, 120), (64, 48, 128), (64, 128, 48)):
        _refused("ccedit_copy_2d_blocks", src.data_ptr(), buf.data_ptr(), plan.data_ptr(), 1, 8, row_bytes, sp, dp)
    _untouched(buf, "copy_2d_blocks refusals")


# ------------------------------------------------------------------------------------------
# wrapper refusals: ValueError before any launch
# ------------------------------------------------------------------------------------------
@pytest.fixture
def no_launch(monkeypatch):
    """The kernel library is out of reach, and every device tensor a wrapper allocates comes pre-filled with the sentinel and is
    recorded: whatever would have been the target of the refused call is there to be inspected."""
    from ccedit_amd import hip
    made = []
    real_empty, real_like = torch.empty, torch.empty_like

    def fill(t):
        if t.is_cuda and t.dtype in (BF, F32):
            t.copy_(R.sentinel_fill(t.numel(), t.dtype, t.device).view(t.shape))
            made.append(t)
        return t

    def no_library():
        raise AssertionError("the wrapper reached the kernel library")
    monkeypatch.setattr(torch, "empty", lambda *a, **k: fill(real_empty(*a, **k)))
    monkeypatch.setattr(torch, "empty_like", lambda *a, **k: fill(real_like(*a, **k)))
    monkeypatch.setattr(hip, "lib", no_library)
    yield made
    for t in made:
        assert bool(R.is_sentinel(t.cpu()).all()), "a refused call wrote to its output"


def _raises(call, *words):
    with pytest.raises(ValueError) as e:
        call()
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_nhwc_to_ncthw_refuses_wrong_frames_and_channels(no_launch):
    _dev()
    from ccedit_amd import ops
    x = torch.zeros(6, 5, 7, 8, device="cuda")
    _raises(lambda: ops.nhwc_to_ncthw(x, 2, 4, 4), "(6, 5, 7, 8)", "2 * 4")
    _raises(lambda: ops.nhwc_to_ncthw(x, 2, 3, 9), "(6, 5, 7, 8)", "c = 9")
    _raises(lambda: ops.nhwc_to_ncthw(x.to(BF), 1, 3, 4), "(6, 5, 7, 8)")


def test_cfg_denoise_refuses_wrong_sizes_and_host_tensors(no_launch):
    _dev()
    from ccedit_amd import ops
    x = torch.zeros(2, 4, 3, 5, 7, device="cuda")
    _raises(lambda: ops.cfg_denoise(x, torch.zeros(2, 2, 4, 3, 5, 6, device="cuda"), 1.0, 7.5), "(2, 4, 3, 5, 7)", "(2, 2, 4, 3, 5, 6)")
    _raises(lambda: ops.cfg_denoise(x, torch.zeros(x.numel(), device="cuda"), 1.0, 7.5), "(2, 4, 3, 5, 7)")
    _raises(lambda: ops.cfg_denoise(x, torch.zeros(2, x.numel()), 1.0, 7.5), "cpu")
    _raises(lambda: ops.cfg_denoise(x.cpu(), torch.zeros(2, x.numel(), device="cuda"), 1.0, 7.5), "cpu")


def test_axpby_refuses_mismatched_and_host_tensors(no_launch):
    _dev()
    from ccedit_amd import ops
    x, z = torch.zeros(1000, device="cuda"), torch.zeros(1000, device="cuda")
    out = R.sentinel_fill(1000, F32, "cuda")
    _raises(lambda: ops.axpby(x, z[:999], 1.0, 1.0, out=out), "(999,)", "(1000,)")
    _raises(lambda: ops.axpby(x, z.to(BF), 1.0, 1.0, out=out), "bfloat16")
    _raises(lambda: ops.axpby(x, z, 1.0, 1.0, out=out[:999]), "out", "(999,)")
    _raises(lambda: ops.axpby(x, z, 1.0, 1.0, out=out.double()), "out", "float64")
    _raises(lambda: ops.axpby(x, z.cpu(), 1.0, 1.0, out=out), "z", "cpu")
    _raises(lambda: ops.axpby(x.cpu(), z, 1.0, 1.0, out=out), "x", "cpu")
    _raises(lambda: ops.axpby(x, z, 1.0, 1.0, out=torch.zeros(1000)), "out", "cpu")
    assert bool(R.is_sentinel(out.cpu()).all())


def test_gaussian_sample_refuses_narrow_moments_and_host_tensors(no_launch):
    _dev()
    from ccedit_amd import ops
    noise = torch.zeros(1, 4, 5, 7, device="cuda")
    _raises(lambda: ops.gaussian_sample(torch.zeros(35, 7, device="cuda"), noise, 4), "(35, 7)", "8")
    _raises(lambda: ops.gaussian_sample(torch.zeros(35, 16, device="cuda")[:, :6], noise, 4), "(35, 6)")
    _raises(lambda: ops.gaussian_sample(torch.zeros(35, 8), noise, 4), "cpu")
    _raises(lambda: ops.gaussian_sample(torch.zeros(35, 8, device="cuda"), noise.cpu(), 4), "cpu")


def test_softmax_rows_refuses_fewer_columns_than_cols(no_launch):
    _dev()
    from ccedit_amd import ops
    _raises(lambda: ops.softmax_rows(torch.zeros(3, 100, device="cuda"), 101, 128, 1.0), "(3, 100)", "101")
