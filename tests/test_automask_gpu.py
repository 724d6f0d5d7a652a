"""Automatic edit masks on a real MI355X (ccedit_amd/automask.py, csrc/automask.hip, --mask_auto).

Everything is exact (bits, no tolerance): the four kernels against the numpy restatement of their definition (tests/_automask_numpy.py),
both access-width arms, misaligned buffers, signed zeros, NaN, cells equal to the threshold; every invalid-argument arm of the C ABI;
AutoMask on the reduced synthetic network against the same closure calls made by hand, plain and through windows, with every RNG
state, cache, reservation and graph of the wrapper as found and the sampler run after it bit-equal to the run without it; the entry
point, whose saved masks given back as --mask_root reproduce the run's bytes."""
import ctypes
import glob
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _automask_numpy as AN  # noqa: E402

pytestmark = pytest.mark.gpu

G160 = dict(model_channels=160, num_heads=4, context_dim=128)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _bits(t):
    if torch.is_tensor(t):
        t = t.detach().cpu().contiguous().numpy()
    return np.ascontiguousarray(t).view(np.int32)


def _offset_view(src: np.ndarray, offset_bytes: int):
    """`src` copied into a device buffer `offset_bytes` past a 16-byte boundary (a contiguous view)."""
    item = src.dtype.itemsize
    buf = torch.zeros(src.size + 16 // item, dtype=torch.from_numpy(src).dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[offset_bytes // item: offset_bytes // item + src.size].view(src.shape)
    v.copy_(torch.from_numpy(src))
    assert v.data_ptr() % 16 == offset_bytes % 16 and v.is_contiguous()
    return v


# ---- 1. the kernels ------------------------------------------------------------------------------
def _halves(b, c, t, h, w, seed):
    """A doubled batch with signed zeros in both halves (equal and opposite signs) among ordinary values."""
    rs = np.random.RandomState(seed)
    y = rs.standard_normal((2 * b, c, t, h, w)).astype(np.float32)
    flat = y.reshape(2, -1)
    n = flat.shape[1]
    for j, (u, v) in enumerate(((0.0, -0.0), (-0.0, 0.0), (-0.0, -0.0), (0.0, 0.0))):
        if j < n:
            flat[0, (j * 7) % n], flat[1, (j * 7) % n] = u, v
    return y


SHAPES = [(2, 4, 3, 16, 24), (1, 4, 2, 9, 13), (1, 1, 1, 1, 1), (2, 16, 1, 8, 8)]


@pytest.mark.parametrize("b,c,t,h,w", SHAPES)
def test_accumulate_is_exact(b, c, t, h, w):
    """16 x 24 and 8 x 8: P % 4 == 0, the 16-byte arm; 9 x 13 and 1 x 1: one element per access.  `first`, then two further adds."""
    _need_gpu()
    from ccedit_amd import ops
    ys = [_halves(b, c, t, h, w, 10 * c + k) for k in range(3)]
    want = got = None
    for k, y in enumerate(ys):
        want = AN.accumulate(y, want)
        got = ops.automask_accumulate(torch.from_numpy(y).cuda(), got)
        assert got.shape == (b, t, h, w) and got.dtype == torch.float32 and got.is_contiguous()
        diff = _bits(got) != _bits(want)
        assert not diff.any(), f"sample {k}: {int(diff.sum())} of {diff.size} cells differ, first at {np.argwhere(diff)[0]}"
    one = ops.automask_accumulate(torch.from_numpy(ys[0]).cuda())
    assert not np.signbit(one.cpu().numpy()).any(), "a difference of signed zeros is +0"


@pytest.mark.parametrize("off_y,off_acc", [(4, 0), (8, 0), (0, 4), (0, 8), (4, 8)])
def test_accumulate_of_buffers_that_are_not_16_byte_aligned(off_y, off_acc):
    """P % 4 == 0 but y or acc 4 / 8 bytes off a 16-byte boundary: the one-element arm, stored and added in place."""
    _need_gpu()
    from ccedit_amd import ops
    y0, y1 = _halves(2, 4, 3, 16, 24, 1), _halves(2, 4, 3, 16, 24, 2)
    acc = _offset_view(np.full((2, 3, 16, 24), 7.0, np.float32), off_acc)
    out = ops.automask_accumulate(_offset_view(y0, off_y), acc, first=True)
    assert out is acc and np.array_equal(_bits(acc), _bits(AN.accumulate(y0)))
    ops.automask_accumulate(_offset_view(y1, off_y), acc)
    assert np.array_equal(_bits(acc), _bits(AN.accumulate(y1, AN.accumulate(y0))))


@pytest.mark.parametrize("h,w", [(16, 24), (9, 13)])
def test_accumulate_carries_nan(h, w):
    _need_gpu()
    from ccedit_amd import ops
    y = _halves(1, 4, 2, h, w, 3)
    y[0, 1, 0, 2, 3] = np.nan                                       # in the source half
    y[1, 3, 1, h - 1, w - 1] = np.nan                               # in the target half
    y[1, 0, 1, 0, 0] = np.inf
    y[0, 0, 1, 0, 0] = np.inf                                       # inf - inf
    want = AN.accumulate(y)
    got = ops.automask_accumulate(torch.from_numpy(y).cuda()).cpu().numpy()
    assert np.isnan(want).sum() == 3 and np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(_bits(got[~np.isnan(want)]), _bits(want[~np.isnan(want)]))


@pytest.mark.parametrize("t,h,w", [(3, 16, 24), (2, 9, 13), (1, 1, 1)])
def test_binarize_is_strict_and_reads_the_scale_per_clip(t, h, w):
    """acc on a grid of multiples of 0.25, so that acc == threshold occurs: such cells stay clear.  B = 2 with different scales; scale 0."""
    _need_gpu()
    from ccedit_amd import ops
    rs = np.random.RandomState(t)
    acc = (rs.randint(0, 17, (2, t, h, w)) * 0.25).astype(np.float32)
    acc[0].flat[0], acc[1].flat[0] = 1.0, 1.5                       # (a cell on each clip's threshold whatever the draw)
    for scales, theta in (((2.0, 3.0), 0.5), ((0.0, 1.0), 0.5), ((4.0, 0.25), 1.0), ((1.0, 1.0), 0.0)):
        thr = np.float32(theta) * np.array(scales, np.float32)
        want = (acc > thr[:, None, None, None]).astype(np.uint8)
        got = ops.automask_binarize(torch.from_numpy(acc).cuda(), torch.tensor(scales, dtype=torch.float32).cuda(), theta)
        assert got.dtype == torch.uint8 and got.shape == acc.shape
        assert np.array_equal(got.cpu().numpy(), want), (scales, theta)
        on_thr = acc == thr[:, None, None, None]
        assert not got.cpu().numpy()[on_thr].any(), "a cell equal to the threshold was set"
    thr = np.float32(0.5) * np.array((2.0, 3.0), np.float32)
    assert (acc == thr[:, None, None, None]).reshape(2, -1).any(axis=1).all(), "the grid never meets the threshold: the test shows nothing"
    # the scale of the restatement: the whole of binarize against numpy, the k-th value on the device
    from ccedit_amd import automask
    n = t * h * w
    dev = torch.from_numpy(acc).cuda()
    scale = ops.kth_values(dev.view(2, n), [automask.rank_of(0.9, n)]).view(2)
    assert np.array_equal(ops.automask_binarize(dev, scale, 0.5).cpu().numpy(), AN.binarize(acc, 0.9, 0.5))
    nan = acc.copy()
    nan[1].flat[-1] = np.nan
    got = ops.automask_binarize(torch.from_numpy(nan).cuda(), torch.tensor((2.0, 3.0)).cuda(), 0.5).cpu().numpy()
    assert got[1].flat[-1] == 0, "a NaN compares false"


def test_binarize_of_a_misaligned_mask():
    _need_gpu()
    from ccedit_amd import ops
    acc = (np.random.RandomState(0).randint(0, 17, (2, 3, 16, 24)) * 0.25).astype(np.float32)
    got = ops.automask_binarize(_offset_view(acc, 4), torch.tensor((2.0, 3.0)).cuda(), 0.5).cpu().numpy()
    assert np.array_equal(got, (acc > np.array((1.0, 1.5), np.float32)[:, None, None, None]).astype(np.uint8))


@pytest.mark.parametrize("t", [1, 2, 5])
@pytest.mark.parametrize("h,w", [(1, 1), (3, 5), (9, 13), (16, 24)])
def test_vote_is_exact(t, h, w):
    _need_gpu()
    from ccedit_amd import ops
    rs = np.random.RandomState(100 * t + h)
    for name, m in [(f"density {d}", (rs.rand(2, t, h, w) < d).astype(np.uint8)) for d in (0.1, 0.5, 0.9)] + [
            ("all clear", np.zeros((2, t, h, w), np.uint8)), ("all set", np.ones((2, t, h, w), np.uint8))]:
        dev = torch.from_numpy(m).cuda()
        for v in (1, 14, 27):
            got = ops.automask_vote(dev, v)
            assert got.dtype == torch.uint8 and got.data_ptr() != dev.data_ptr()
            diff = got.cpu().numpy() != AN.vote(m, v)
            assert not diff.any(), f"{name}, V = {v}: {int(diff.sum())} cells differ, first at {np.argwhere(diff)[0]}"
        assert np.array_equal(dev.cpu().numpy(), m), "the vote wrote to its input"
    mixed = (rs.rand(2, t, h, w) < 0.6).astype(np.uint8)
    assert np.array_equal(ops.automask_vote(torch.from_numpy(mixed * 200).cuda(), 14).cpu().numpy(), AN.vote(mixed, 14)), "any non-zero byte is set"


@pytest.mark.parametrize("h,w", [(9, 13), (16, 24)])
def test_expand_is_exact_and_mask_latent_gives_the_input_back(h, w):
    _need_gpu()
    from ccedit_amd import ops
    m = (np.random.RandomState(w).rand(2, 3, h, w) < 0.4).astype(np.uint8)
    px = ops.automask_expand(torch.from_numpy(m).cuda())
    assert px.shape == (2, 3, 8 * h, 8 * w) and px.dtype == torch.uint8 and px.is_contiguous()
    assert np.array_equal(px.cpu().numpy(), AN.expand(m))
    assert np.array_equal(ops.mask_latent(px).cpu().numpy(), m), "ops.mask_latent(expand(m)) != m"
    assert np.array_equal(ops.automask_expand(torch.from_numpy(m * 3).cuda()).cpu().numpy(), AN.expand(m))


def test_mask_from_is_the_restatement():
    """The rectangle of tests/test_automask.py on the device: kth value, binarize, vote, expand."""
    _need_gpu()
    from ccedit_amd import automask, ops
    rs = np.random.RandomState(4)
    src = rs.standard_normal((2, 4, 5, 16, 24)).astype(np.float32)
    delta = rs.uniform(-0.1, 0.1, src.shape).astype(np.float32)
    delta[0, :, :, 4:10, 6:16] = 1.0
    delta[1, :, 1:, 2:7, 3:20] = -1.0
    y = np.concatenate([src, (src + delta).astype(np.float32)])
    acc = ops.automask_accumulate(torch.from_numpy(y).cuda())
    assert np.array_equal(_bits(acc), _bits(AN.accumulate(y)))
    for q, theta, v in ((0.99, 0.5, 14), (0.99, 0.5, 0), (0.5, 1.0, 1), (1.0, 0.25, 27), (0.0, 2.0, 14)):
        got = automask.mask_from(acc, q, theta, v)
        want = AN.mask_from(AN.accumulate(y), q, theta, v)
        assert got.shape == (2, 5, 128, 192) and np.array_equal(got.cpu().numpy(), want), (q, theta, v)
    lat = automask.mask_from(acc, 0.99, 0.5, 0, latent=True).cpu().numpy()
    assert lat[0, :, 4:10, 6:16].all() and lat[0].sum() == 5 * 60, "V = 0: the rectangle exactly"
    bad = acc.clone()
    bad[1, 2, 3, 4] = float("nan")
    with pytest.raises(ValueError, match="horse.*not finite"):
        automask.mask_from(bad, names=["clips/zebra", "clips/horse"])


def test_invalid_arguments_return_their_code_and_launch_nothing():
    _need_gpu()
    from ccedit_amd import hip, ops
    lib = hip.lib()
    y = torch.full((2, 4, 1, 4, 4), 3.0, device="cuda")
    acc = torch.full((1, 1, 4, 4), 5.0, device="cuda")
    scale = torch.full((1,), 1.0, device="cuda")
    m = torch.full((1, 1, 4, 4), 9, dtype=torch.uint8, device="cuda")
    m2 = torch.full((1, 1, 4, 4), 8, dtype=torch.uint8, device="cuda")
    px = torch.full((1, 1, 32, 32), 7, dtype=torch.uint8, device="cuda")
    p = lambda t: t.data_ptr()                                      # noqa: E731
    f = ctypes.c_float
    cases = [
        (lib.ccedit_automask_accumulate, (None, p(acc), 1, 4, 16, 1), b"null pointer"),
        (lib.ccedit_automask_accumulate, (p(y), None, 1, 4, 16, 1), b"null pointer"),
        (lib.ccedit_automask_accumulate, (p(y), p(acc), 0, 4, 16, 1), b"B=0"),
        (lib.ccedit_automask_accumulate, (p(y), p(acc), 1, 4, 0, 1), b"P=0"),
        (lib.ccedit_automask_accumulate, (p(y), p(acc), 1, 0, 16, 1), b"C=0"),
        (lib.ccedit_automask_accumulate, (p(y), p(acc), 1, 17, 16, 1), b"C=17"),
        (lib.ccedit_automask_accumulate, (p(y), p(acc), 1, 4, 2 ** 33, 1), b"2^33"),
        (lib.ccedit_automask_accumulate, (p(y), p(acc), 1, 4, 16, 2), b"first=2"),
        (lib.ccedit_automask_accumulate, (p(y) + 2, p(acc), 1, 4, 16, 1), b"4-byte aligned"),
        (lib.ccedit_automask_binarize, (None, p(scale), f(0.5), p(m), 1, 16), b"null pointer"),
        (lib.ccedit_automask_binarize, (p(acc), None, f(0.5), p(m), 1, 16), b"null pointer"),
        (lib.ccedit_automask_binarize, (p(acc), p(scale), f(0.5), None, 1, 16), b"null pointer"),
        (lib.ccedit_automask_binarize, (p(acc), p(scale), f(0.5), p(m), 0, 16), b"B=0"),
        (lib.ccedit_automask_binarize, (p(acc), p(scale), f(0.5), p(m), 1, 0), b"P=0"),
        (lib.ccedit_automask_binarize, (p(acc), p(scale), f(-0.5), p(m), 1, 16), b"theta"),
        (lib.ccedit_automask_binarize, (p(acc), p(scale), f(float("nan")), p(m), 1, 16), b"theta"),
        (lib.ccedit_automask_binarize, (p(acc), p(scale), f(float("inf")), p(m), 1, 16), b"theta"),
        (lib.ccedit_automask_binarize, (p(acc) + 1, p(scale), f(0.5), p(m), 1, 16), b"4-byte aligned"),
        (lib.ccedit_automask_vote, (None, p(m2), 1, 1, 4, 4, 14), b"null pointer"),
        (lib.ccedit_automask_vote, (p(m), None, 1, 1, 4, 4, 14), b"null pointer"),
        (lib.ccedit_automask_vote, (p(m), p(m2), 0, 1, 4, 4, 14), b"B=0"),
        (lib.ccedit_automask_vote, (p(m), p(m2), 1, 0, 4, 4, 14), b"T=0"),
        (lib.ccedit_automask_vote, (p(m), p(m2), 1, 1, 0, 4, 14), b"0x4"),
        (lib.ccedit_automask_vote, (p(m), p(m2), 1, 1, 4, 0, 14), b"4x0"),
        (lib.ccedit_automask_vote, (p(m), p(m2), 1, 1, 4, 4, 0), b"votes=0"),
        (lib.ccedit_automask_vote, (p(m), p(m2), 1, 1, 4, 4, 28), b"votes=28"),
        (lib.ccedit_automask_vote, (p(m), p(m2), 2 ** 15, 2 ** 15, 4, 4, 14), b"2^31"),
        (lib.ccedit_automask_vote, (p(m), p(m), 1, 1, 4, 4, 14), b"alias"),
        (lib.ccedit_automask_vote, (p(m), p(m) + 8, 1, 1, 4, 4, 14), b"alias"),
        (lib.ccedit_automask_expand, (None, p(px), 1, 4, 4), b"null pointer"),
        (lib.ccedit_automask_expand, (p(m), None, 1, 4, 4), b"null pointer"),
        (lib.ccedit_automask_expand, (p(m), p(px), 0, 4, 4), b"N=0"),
        (lib.ccedit_automask_expand, (p(m), p(px), 1, 0, 4), b"0x4"),
        (lib.ccedit_automask_expand, (p(m), p(px), 1, 4, 0), b"4x0"),
        (lib.ccedit_automask_expand, (p(m), p(px), 2 ** 30, 4, 4), b"2^33"),
        (lib.ccedit_automask_expand, (p(m), p(px) + 4, 1, 4, 4), b"8-byte aligned"),
    ]
    for fn, args, words in cases:
        rc = fn(*args, None)
        assert rc == -1 and words in lib.ccedit_last_error(), (fn.__name__, args, rc, lib.ccedit_last_error())
    torch.cuda.synchronize()
    for t, v in ((y, 3.0), (acc, 5.0), (scale, 1.0), (m, 9), (m2, 8), (px, 7)):
        assert bool((t == v).all()), "a refused call wrote to a buffer"
    with pytest.raises(ValueError):
        ops.automask_accumulate(y.half())
    with pytest.raises(ValueError):
        ops.automask_accumulate(y[:1])
    with pytest.raises(ValueError):
        ops.automask_accumulate(y, acc[:, :, :2].contiguous())
    with pytest.raises(ValueError):
        ops.automask_binarize(acc, scale.cpu(), 0.5)
    with pytest.raises(ValueError):
        ops.automask_binarize(acc, torch.ones(2, device="cuda"), 0.5)
    with pytest.raises(ValueError):
        ops.automask_vote(m.float(), 14)
    with pytest.raises(hip.HipLibraryError, match="votes=0"):
        ops.automask_vote(m, 0)
    with pytest.raises(ValueError):
        ops.automask_expand(m[0, 0])


# ---- 2. AutoMask on the reduced synthetic network -----------------------------------------------
@pytest.fixture(scope="module")
def g160_wrapper():
    _need_gpu()
    from ccedit_amd.sgm_compat import build_network
    from ccedit_amd.utils.synth import fill_module_
    w = build_network("cpu", **G160)
    fill_module_(w, prefix="model.")
    w.diffusion_model.pack("cuda")
    return w


def _make_sampler_and_denoiser(steps=3):
    from ccedit_amd.config import instantiate_from_config
    dd = "sgm.modules.diffusionmodules."
    denoiser = instantiate_from_config(dict(
        target=dd + "denoiser.DiscreteDenoiser",
        params=dict(num_idx=1000, weighting_config=dict(target=dd + "denoiser_weighting.EpsWeighting"),
                    scaling_config=dict(target=dd + "denoiser_scaling.EpsScaling"),
                    discretization_config=dict(target=dd + "discretizer.LegacyDDPMDiscretization"))))
    sampler = instantiate_from_config(dict(
        target=dd + "sampling.DPMPP2SAncestralSampler",
        params=dict(num_steps=steps, eta=1.0, s_noise=1.0, verbose=False,
                    discretization_config=dict(target=dd + "discretizer.LegacyDDPMDiscretization"),
                    guider_config=dict(target=dd + "guiders.VanillaCFGTV2V", params=dict(scale=7.5)))))
    return sampler, denoiser


def _clip_inputs(seed, n, steps=3):
    """The reduced shape of the committed goldens (latent 16 x 24, context 77 x 128) with n keyframes; a third context: the source prompt's."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(1, 4, n, 16, 24, generator=g)
    cc, cuc, csrc = (torch.randn(1, 77, 128, generator=g) for _ in range(3))
    hint = (torch.rand(1, 1, n, 128, 192, generator=g) * 2 - 1).repeat(1, 3, 1, 1, 1)
    noises = [torch.randn(1, 4, n, 16, 24, generator=g) for _ in range(steps)]
    return x, cc, cuc, csrc, hint, noises


def _closure(wrapper, window=None):
    from ccedit_amd.windows import WindowedDenoiser
    _, denoiser = _make_sampler_and_denoiser()

    def denoise(inp, sigma, cond):          # the closure of scripts/sampling/sampling_tv2v.py: make_closure
        return denoiser(wrapper, inp, sigma, cond)
    return denoise if window is None else WindowedDenoiser(denoise, window, None, wrapper=wrapper)


def _sample(wrapper, x, cc, cuc, hint, noises, reset=True, steps=3):
    """One plain clip through a fresh sampler, per-step noise injected; `reset=False`: from the caches as they are."""
    sampler, _ = _make_sampler_and_denoiser(steps)
    it = iter([v.cuda() for v in noises])
    sampler.noise_sampler = lambda xx: next(it)
    c = dict(crossattn=cc.cuda(), control_hint=hint.cuda())
    uc = dict(crossattn=cuc.cuda(), control_hint=hint.clone().cuda())
    if reset:
        wrapper.reserve_windows(0)
        wrapper.reset_caches()
    return sampler(_closure(wrapper), x.clone().cuda(), c, uc=uc).cpu()


def _restore(w):
    w.reserve_windows(0)
    w.reset_caches()


def _by_hand(wrapper, z, sigma, c_src, c_tgt, samples, seed, window=None):
    """The closure calls AutoMask makes, made here, and the restatement applied to their outputs."""
    from ccedit_amd import automask, ops
    from ccedit_amd.config import instantiate_from_config
    guider = instantiate_from_config(dict(target=automask.GUIDER, params=dict(scale=1.0)))
    closure = _closure(wrapper, window)
    gen = torch.Generator().manual_seed(seed)
    want = None
    for _ in range(samples):
        e = torch.randn(z.shape, generator=gen)
        x = ops.axpby(z, e.cuda(), 1.0, sigma)
        y = closure(*guider.prepare_inputs(x, torch.full((z.shape[0],), sigma), c_tgt, c_src)).float().cpu().numpy()
        assert y.shape[0] == 2 * z.shape[0]
        want = AN.accumulate(y, want)
    return want


def _rng_states():
    return torch.get_rng_state().clone(), torch.cuda.get_rng_state().clone(), np.random.get_state()[1].copy()


@pytest.mark.parametrize("n,window", [(3, None), (5, 3)])
def test_automask_is_the_restatement_of_its_own_closure_calls(g160_wrapper, n, window):
    """2 samples at T = 3 through the plain closure, and at 5 frames through WindowedDenoiser (window 3): acc bit for bit; no global RNG
    stream moves; the wrapper's reservations are as found."""
    from ccedit_amd import automask
    w = g160_wrapper
    x, cc, cuc, csrc, hint, _ = _clip_inputs(61 + n, n)
    z, sigma = x.cuda(), 2.5
    h = hint.cuda()
    c_tgt = dict(crossattn=cc.cuda(), control_hint=h)
    c_src = dict(c_tgt, crossattn=csrc.cuda())
    try:
        _restore(w)
        before = _rng_states()
        acc = automask.AutoMask(_closure(w, window), wrapper=w)(z, sigma, c_src, c_tgt, 2, 11)
        torch.cuda.synchronize()
        after = _rng_states()
        assert all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(before, after)), "a global RNG stream moved"
        assert (w._windows, w._contexts, w._graph_slots, w._hint_slots, w._tkv_slots, w._graph_pool) == (1, 1, 2, 4, 6, None)
        assert len(w._graphs) == len(w._hint_val) == len(w._tkv_val) == 0, "the guest left cache entries behind"
        _restore(w)
        want = _by_hand(w, z, sigma, c_src, c_tgt, 2, 11, window)
    finally:
        _restore(w)
    assert acc.shape == (1, n, 16, 24) and bool(torch.isfinite(acc).all()) and float(acc.max()) > 0
    assert np.array_equal(_bits(acc), _bits(want))
    again = None
    try:
        again = automask.AutoMask(_closure(w, window), wrapper=w)(z, sigma, c_src, c_tgt, 2, torch.Generator().manual_seed(11))
    finally:
        _restore(w)
    assert np.array_equal(_bits(again), _bits(acc)), "an int seed and a generator of that seed draw the same noise"


def test_a_sampler_run_after_an_automask_call_is_the_run_without_it(g160_wrapper):
    """Caches and graphs filled by a clip's run are as found after the guest; the next run from them is bit-equal to a fresh one."""
    from ccedit_amd import automask
    w = g160_wrapper
    x, cc, cuc, csrc, hint, noises = _clip_inputs(71, 3)
    h = hint.cuda()
    c_tgt = dict(crossattn=cc.cuda(), control_hint=h)
    c_src = dict(c_tgt, crossattn=csrc.cuda())
    try:
        plain = _sample(w, x, cc, cuc, hint, noises)
        found = ([list(c) for c in w._caches()], [id(v) for v in w._graphs.values()], dict(w.graph_counts or {}),
                 (w._windows, w._contexts, w._graph_slots, w._hint_slots, w._tkv_slots, w._graph_pool))
        acc = automask.AutoMask(_closure(w), wrapper=w)(x.cuda(), 2.5, c_src, c_tgt, 2, 3)
        left = ([list(c) for c in w._caches()], [id(v) for v in w._graphs.values()], dict(w.graph_counts or {}),
                (w._windows, w._contexts, w._graph_slots, w._hint_slots, w._tkv_slots, w._graph_pool))
        assert left == found, "caches, graphs, counters or reservations are not as found"
        after = _sample(w, x, cc, cuc, hint, noises, reset=False)
        _restore(w)
        acc2 = automask.AutoMask(_closure(w), wrapper=w)(x.cuda(), 2.5, c_src, c_tgt, 2, 3)
        fresh = _sample(w, x, cc, cuc, hint, noises, reset=False)
    finally:
        _restore(w)
    assert bool(torch.isfinite(plain).all()) and plain.shape == (1, 4, 3, 16, 24)
    assert np.array_equal(_bits(after), _bits(plain)) and np.array_equal(_bits(fresh), _bits(plain))
    assert np.array_equal(_bits(acc), _bits(acc2)), "the guest's own result depends on the caches it found"


# ---- 3. entry point ------------------------------------------------------------------------------
def _write_config(tmp_path):
    import yaml
    from ccedit_amd.sgm_compat import engine_config
    cfg = os.path.join(str(tmp_path), "tv2v.yaml")
    with open(cfg, "w") as f:
        yaml.safe_dump(dict(model=engine_config(crossframe=False, vae_ch=32, model_channels=64, num_heads=2, context_dim=64)), f)
    return cfg


@pytest.fixture()
def clip(tmp_path):
    """The clip of the region tests: a 64 x 128 frame directory of 9 frames (3 keyframes at 9 -> 3 fps), 2 steps, --noise_seed 1."""
    from PIL import Image
    rs = np.random.RandomState(8)
    vdir = tmp_path / "clips" / "bear"
    vdir.mkdir(parents=True)
    for i in range(9):
        Image.fromarray(rs.randint(0, 256, (64, 128, 3)).astype(np.uint8)).save(str(vdir / f"{i:03d}.png"))
    base = ["--config_path", _write_config(tmp_path), "--synthetic", "--H", "64", "--W", "128", "--num_keyframes", "3", "--sample_steps", "2",
            "--sampler_name", "DPMPP2SAncestralSampler", "--original_fps", "9", "--target_fps", "3", "--noise_seed", "1", "--prompt", "a panda",
            "--video_path", str(vdir), "--batch_size", "1", "--save_type", "npy"]
    return tmp_path, base


def _job(monkeypatch, base, out, *extra):
    """The job through scripts.sampling.sampling_tv2v.main in this process -> (result frames, log_info)."""
    from scripts.sampling import sampling_tv2v as S
    monkeypatch.setattr(sys, "argv", ["sampling_tv2v.py", *base, "--save_path", out, *extra])
    S.main()
    files = sorted(glob.glob(os.path.join(out, "default", "result", "npy", "frames-*.npy")))
    assert len(files) == 1, files
    with open(os.path.join(out, "default", "log_info.json")) as f:
        return np.load(files[0]), json.load(f)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("extra", [(), ("--mask_auto_strength", "1.0")], ids=["default strength", "strength 1"])
def test_saved_masks_given_back_as_mask_root_reproduce_the_run(clip, monkeypatch, extra):
    """Run A computes the mask and saves it; run B reads it back through --mask_root: the same result bytes.  At the default strength the
    2-step schedule starts at sigma 0 (the latent is not noised, announced on stderr); at strength 1 it starts at the largest sigma and the
    mask is neither empty nor full."""
    _need_gpu()
    from PIL import Image
    tmp_path, base = clip
    d = str(tmp_path / "D")
    res_a, log = _job(monkeypatch, base, str(tmp_path / "a"), "--inpainting_mode", "--mask_auto", "--source_prompt", "a bear", "--mask_auto_save", d,
                      *extra)
    assert res_a.shape == (3, 64, 128, 3) and np.isfinite(res_a).all()
    saved = os.path.join(d, "bear")
    assert sorted(os.listdir(saved)) == [f"{f:05d}.png" for f in range(9)], "one PNG per source frame"
    frames = [np.array(Image.open(os.path.join(saved, f"{f:05d}.png"))) for f in range(9)]
    assert all(m.shape == (64, 128) and m.dtype == np.uint8 and set(np.unique(m)) <= {0, 255} for m in frames)
    for f, k in enumerate([0, 0, 1, 1, 1, 2, 2, 2, 2]):
        assert np.array_equal(frames[f], frames[3 * k]), "a frame holds its nearest keyframe's mask"
    assert len(glob.glob(os.path.join(str(tmp_path / "a"), "default", "mask", "npy", "*.npy"))) == 1, "mask/ was not written"
    auto = log["mask_auto"]
    assert auto["source_prompt"] == "a bear" and (auto["samples"], auto["quantile"], auto["threshold"], auto["vote"]) == (4, 0.99, 0.5, 14)
    assert auto["seed"] == 42 and auto["strength"] == (1.0 if extra else 0.5) and len(auto["fractions"]) == 1
    set_cells = np.mean([(frames[3 * k][::8, ::8] != 0).mean() for k in range(3)])
    assert abs(auto["fractions"][0] - set_cells) < 1e-6, "the logged fraction is not the saved masks'"
    if extra:
        assert auto["sigma"] > 1.0 and 0.0 < auto["fractions"][0] < 1.0, auto
    else:
        assert auto["sigma"] == 0.0, auto
    res_b, log_b = _job(monkeypatch, base, str(tmp_path / "b"), "--inpainting_mode", "--mask_root", d)
    assert "mask_auto" not in log_b
    assert res_b.tobytes() == res_a.tobytes()


@pytest.mark.timeout(900)
def test_no_vote_sets_no_fewer_cells_than_a_unanimous_one(clip, monkeypatch):
    _need_gpu()
    tmp_path, base = clip
    flags = ["--inpainting_mode", "--mask_auto", "--source_prompt", "a bear", "--mask_auto_strength", "1.0"]
    _, none = _job(monkeypatch, base, str(tmp_path / "v0"), *flags, "--mask_auto_vote", "0")
    _, all27 = _job(monkeypatch, base, str(tmp_path / "v27"), *flags, "--mask_auto_vote", "27")
    f0, f27 = none["mask_auto"]["fractions"][0], all27["mask_auto"]["fractions"][0]
    print(f"fraction of latent cells set: vote 0 {f0:.4f}, vote 27 {f27:.4f}")
    assert none["mask_auto"]["vote"] == 0 and all27["mask_auto"]["vote"] == 27
    assert f0 > 0.0, "an empty mask before the vote: the test shows nothing"
    assert f0 >= f27
