"""Region prompts on a real MI355X (ccedit_amd/regions.py, csrc/region.hip, --region_prompt / --region_mask).

Exact (no tolerance): the two kernels against the numpy restatement of their definition (tests/_regions_numpy.py); all-black masks and a
frame-filling region against the plain sampler; a hard split against the per-cell select of two plain evaluations; the network wrapper's
evaluation counts; graphed against eager.  Against the fp32 CPU oracle: one clip with a feathered half-frame region at the reduced size
of the committed goldens, with the budget of the plain sampler trajectory (tests/test_network_gpu.py: TRAJ_TOL)."""
import ctypes
import glob
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _regions_numpy as RN  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
G160 = dict(model_channels=160, num_heads=4, context_dim=128)
TRAJ_TOL = 8e-2      # relative RMS of the final latent: the plain trajectory's budget (test_sampler_trajectory_vs_reference_golden)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt()).item()


def _bits(t):
    if torch.is_tensor(t):
        t = t.detach().cpu().contiguous().numpy()
    return np.ascontiguousarray(t).view(np.int32)


# ---- 1. the kernels ------------------------------------------------------------------------------
def _mask_sets(k, t, hh, ww, seed):
    """The mask kinds of the issue, each uint8 (K, T, H, W)."""
    rs = np.random.RandomState(seed)
    out = {}
    out["random bytes"] = rs.randint(0, 256, (k, t, hh, ww)).astype(np.uint8)
    out["all white"] = np.full((k, t, hh, ww), 255, np.uint8)
    out["all black"] = np.zeros((k, t, hh, ww), np.uint8)
    one = np.zeros((k, t, hh, ww), np.uint8)
    for r in range(k):
        for f in range(t):
            one[r, f, rs.randint(hh), rs.randint(ww)] = 128          # the smallest byte that counts
    out["one white pixel"] = one
    rect = np.full((k, t, hh, ww), 127, np.uint8)                     # the largest byte that does not
    for r in range(k):
        y0, x0 = (r * hh) // (2 * k), (r * ww) // (3 * k)
        rect[r, :, y0:y0 + max(hh // 2, 3), x0:x0 + max(ww // 2, 5)] = 200
    out["overlapping rectangles"] = rect
    fill = rs.randint(0, 256, (k, t, hh, ww)).astype(np.uint8)
    fill[k - 1] = 255
    out["a frame-filling region"] = fill
    return out


# (K, T, H, W, F)
WEIGHT_CASES = [(1, 1, 64, 64, 0), (1, 3, 72, 104, 1), (2, 2, 128, 192, 1), (4, 1, 72, 104, 8), (7, 2, 64, 128, 3), (2, 1, 8, 8, 2)]


@pytest.mark.parametrize("k,t,hh,ww,f", WEIGHT_CASES)
def test_region_weights_are_exact(k, t, hh, ww, f):
    _need_gpu()
    from ccedit_amd import ops
    for name, masks in _mask_sets(k, t, hh, ww, 100 * k + 10 * t + f).items():
        want = RN.region_weights(masks, f)
        got = ops.region_weights(torch.from_numpy(masks).cuda(), f)
        assert got.shape == (k + 1, t, hh // 8, ww // 8) and got.dtype == torch.float32 and got.is_contiguous()
        diff = _bits(got) != _bits(want)
        assert not diff.any(), f"{name}: {int(diff.sum())} of {diff.size} coefficients differ, first at {np.argwhere(diff)[0]}"
        g = got.cpu().numpy()
        assert (g >= 0).all() and (g <= 1).all() and ((g != 0).sum(axis=0) >= 1).all(), name
        if name == "all black":
            assert (g[0] == 1.0).all() and (g[1:] == 0.0).all()
        if name == "a frame-filling region" and k == 1:
            assert (g[1] == 1.0).all() and (g[0] == 0.0).all()


def test_region_weights_of_masks_that_are_not_16_byte_aligned():
    """W % 16 == 0 but the masks 8 bytes off a 16-byte boundary: the 8-byte row loads."""
    _need_gpu()
    from ccedit_amd import ops
    masks = np.random.RandomState(3).randint(0, 256, (2, 2, 32, 48)).astype(np.uint8)
    buf = torch.zeros(masks.size + 16, dtype=torch.uint8, device="cuda")
    v = buf[8:8 + masks.size].view(masks.shape)
    v.copy_(torch.from_numpy(masks))
    assert v.data_ptr() % 16 == 8 and v.is_contiguous()
    assert np.array_equal(_bits(ops.region_weights(v, 2)), _bits(RN.region_weights(masks, 2)))


def _fuse_inputs(b, c, t, h, w, seed, poison=True):
    """K = 2: coefficients from feathered rectangles (cells owned by one region, shared cells, cells region 2 never reaches); NaN in
    region 1 and Inf in region 2 wherever their coefficient is 0."""
    rs = np.random.RandomState(seed)
    masks = np.zeros((2, t, 8 * h, 8 * w), np.uint8)
    masks[0, :, : 8 * h // 2 + 3, : 8 * w // 2 + 5] = 255
    masks[1, :, 8 * h // 3:, 8 * w // 3: 8 * w - 16] = 255
    masks[1, -1] = 0
    coef = RN.region_weights(masks, 1)
    assert (coef == 0).any() and (coef == 1).any() and ((coef > 0) & (coef < 1)).any()
    ys = [rs.standard_normal((b, c, t, h, w)).astype(np.float32) for _ in range(3)]
    if poison:
        ys[1][np.broadcast_to((coef[1] == 0)[None, None], ys[1].shape)] = np.nan
        ys[2][np.broadcast_to((coef[2] == 0)[None, None], ys[2].shape)] = np.inf
    return ys, coef


@pytest.mark.parametrize("b,c,h,w", [(2, 4, 16, 24), (2, 4, 9, 13), (1, 1, 16, 24), (1, 1, 9, 13)])
def test_region_fuse_is_exact_and_skips_zero_coefficients(b, c, h, w):
    """16 x 24: P % 4 == 0, 16-byte accesses; 9 x 13: one element per access.  B C = 8 and 1."""
    _need_gpu()
    from ccedit_amd import ops
    ys, coef = _fuse_inputs(b, c, 2, h, w, 7 * h + b)
    want = RN.region_fuse(ys, coef)
    assert np.isfinite(want).all()
    got = ops.region_fuse([torch.from_numpy(y).cuda() for y in ys], torch.from_numpy(coef).cuda())
    assert got.shape == (b, c, 2, h, w) and bool(torch.isfinite(got).all())
    assert np.array_equal(_bits(got), _bits(want)), f"{int((_bits(got) != _bits(want)).sum())} elements differ"
    # a cell owned by one region is a bit copy of that region's evaluation
    for r in range(3):
        own = np.broadcast_to((coef[r] == 1.0)[None, None], want.shape)
        assert own.any() and np.array_equal(_bits(got.cpu().numpy()[own]), _bits(ys[r][own]))


@pytest.mark.parametrize("h,w", [(16, 24), (9, 13)])
def test_region_fuse_reads_regions_that_are_not_16_byte_aligned(h, w):
    """The evaluations are read where they lie: a tensor 4 / 8 / 12 bytes off a 16-byte boundary takes the element-wise loads."""
    _need_gpu()
    from ccedit_amd import ops
    ys, coef = _fuse_inputs(2, 4, 2, h, w, 11)
    dev = []
    for k, y in enumerate(ys):
        buf = torch.empty(y.size + 4, dtype=torch.float32, device="cuda")
        off = k + 1 if k else 0                                # region 0 aligned, the others 4 / 8 bytes off
        v = buf[off:off + y.size].view(y.shape)
        v.copy_(torch.from_numpy(y))
        assert v.is_contiguous() and (v.data_ptr() % 16 == 0) == (off == 0)
        dev.append(v)
    got = ops.region_fuse(dev, torch.from_numpy(coef).cuda())
    assert np.array_equal(_bits(got), _bits(RN.region_fuse(ys, coef)))


def test_region_entry_points_refuse_bad_arguments():
    """A status and a message, no launch: null pointers, K = 0 or 8, F = 9, H not a multiple of 8; a wrong dtype or shape through ops."""
    _need_gpu()
    from ccedit_amd import hip, ops
    lib = hip.lib()
    m = torch.zeros(1, 1, 16, 16, dtype=torch.uint8, device="cuda")
    cf = torch.full((2, 1, 2, 2), 7.0, device="cuda")
    y = torch.zeros(1, 4, 1, 2, 2, device="cuda")
    table = torch.tensor([y.data_ptr(), y.data_ptr()], dtype=torch.int64, device="cuda")
    out = torch.full_like(y, 5.0)
    p = lambda v: ctypes.c_void_p(v.data_ptr())
    for args, words in (((None, p(cf), 1, 1, 16, 16, 0), b"null pointer"), ((p(m), None, 1, 1, 16, 16, 0), b"null pointer"),
                        ((p(m), p(cf), 0, 1, 16, 16, 0), b"K=0"), ((p(m), p(cf), 8, 1, 16, 16, 0), b"K=8"),
                        ((p(m), p(cf), 1, 1, 16, 16, 9), b"F=9"), ((p(m), p(cf), 1, 1, 16, 16, -1), b"F=-1"),
                        ((p(m), p(cf), 1, 1, 12, 16, 0), b"multiples of 8"), ((p(m), p(cf), 1, 0, 16, 16, 0), b"T=0")):
        assert lib.ccedit_region_weights(*args, None) == -1 and words in lib.ccedit_last_error(), (args, lib.ccedit_last_error())
    for args, words in (((None, p(out), p(cf), 1, 1, 4, 1, 4), b"null pointer"), ((p(table), None, p(cf), 1, 1, 4, 1, 4), b"null pointer"),
                        ((p(table), p(out), None, 1, 1, 4, 1, 4), b"null pointer"), ((p(table), p(out), p(cf), 0, 1, 4, 1, 4), b"K=0"),
                        ((p(table), p(out), p(cf), 8, 1, 4, 1, 4), b"K=8"), ((p(table), p(out), p(cf), 1, 1, 4, 0, 4), b"T=0"),
                        ((p(table), p(out), p(cf), 1, 1, 4, 1, 0), b"P=0")):
        assert lib.ccedit_region_fuse(*args, None) == -1 and words in lib.ccedit_last_error(), (args, lib.ccedit_last_error())
    torch.cuda.synchronize()
    assert bool((cf == 7.0).all()) and bool((out == 5.0).all()), "a refused call wrote to its output"
    with pytest.raises(ValueError):
        ops.region_weights(m.float(), 0)
    with pytest.raises(ValueError):
        ops.region_weights(m[0], 0)
    with pytest.raises(hip.HipLibraryError, match="F=9"):
        ops.region_weights(m, 9)
    with pytest.raises(hip.HipLibraryError, match="multiples of 8"):
        ops.region_weights(torch.zeros(1, 1, 12, 16, dtype=torch.uint8, device="cuda"), 0)
    with pytest.raises(ValueError):
        ops.region_fuse([y, y.half()], cf)
    with pytest.raises(ValueError):
        ops.region_fuse([y, y], cf[:, :, :1].contiguous())
    with pytest.raises(ValueError):
        ops.region_fuse([y, y], cf.double())
    with pytest.raises(hip.HipLibraryError, match="K=0"):
        ops.region_fuse([y], cf[:1].contiguous())


# ---- 2. the region closure in the sampler ------------------------------------------------------
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
    """The reduced shape of the committed goldens (latent 16 x 24, context 77 x 128) with n keyframes."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(1, 4, n, 16, 24, generator=g)
    cc, cuc = torch.randn(1, 77, 128, generator=g), torch.randn(1, 77, 128, generator=g)
    hint = (torch.rand(1, 1, n, 128, 192, generator=g) * 2 - 1).repeat(1, 3, 1, 1, 1)
    noises = [torch.randn(1, 4, n, 16, 24, generator=g) for _ in range(steps)]
    return x, cc, cuc, hint, noises


def _contexts(seed, k):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(1, 77, 128, generator=g) for _ in range(k)]


def _half_masks(n, k=1, right_from=96):
    """K masks over n frames of 128 x 192: region 1 the columns from `right_from` on, further regions horizontal bands."""
    m = np.zeros((k, n, 128, 192), np.uint8)
    m[0, :, :, right_from:] = 255
    for r in range(1, k):
        m[r, :, 16 * r:16 * r + 40, :] = 255
    return m


def _run(wrapper, x, cc, cuc, hint, noises, region_ctx=None, masks=None, feather=1, window=None, overlap=None, steps=3):
    """One clip through a fresh sampler: plain, or through the region closure (contexts [cc] + region_ctx, coefficients from the device
    kernel) around the plain or the windowed closure; per-step noise injected."""
    from ccedit_amd import regions
    from ccedit_amd.windows import WindowedDenoiser
    sampler, denoiser = _make_sampler_and_denoiser(steps)
    it = iter([v.cuda() for v in noises])
    sampler.noise_sampler = lambda xx: next(it)

    def denoise(inp, sigma, cond):          # the closure of scripts/sampling/sampling_tv2v.py: sample_latent
        return denoiser(wrapper, inp, sigma, cond)

    c = dict(crossattn=cc.cuda(), control_hint=hint.cuda())
    uc = dict(crossattn=cuc.cuda(), control_hint=hint.clone().cuda())
    closure = denoise if window is None else WindowedDenoiser(denoise, window, overlap, wrapper=wrapper)
    if region_ctx is not None:
        coef = regions.weights(torch.from_numpy(masks).cuda(), feather)
        closure = regions.RegionDenoiser(closure, [c["crossattn"]] + [v.cuda() for v in region_ctx], coef, wrapper=wrapper)
    wrapper.reset_caches()
    return sampler(closure, x.clone().cuda(), c, uc=uc).cpu()


def _restore(w):
    w.reserve_windows(0)
    w.reset_caches()


def test_black_region_masks_are_the_plain_sampler_bit_for_bit(g160_wrapper):
    """All-black masks: the region's evaluations run (with NaN-free but different text) and the fuse skips them — coef[0] is 1.0."""
    inputs = _clip_inputs(41, 3)
    try:
        plain = _run(g160_wrapper, *inputs)
        got = _run(g160_wrapper, *inputs, region_ctx=_contexts(1, 1), masks=np.zeros((1, 3, 128, 192), np.uint8))
    finally:
        _restore(g160_wrapper)
    assert bool(torch.isfinite(plain).all()) and plain.shape == (1, 4, 3, 16, 24)
    assert np.array_equal(_bits(got), _bits(plain)), _rel(got, plain)


def test_a_frame_filling_region_is_a_plain_run_with_its_prompt(g160_wrapper):
    x, cc, cuc, hint, noises = _clip_inputs(42, 3)
    c1 = _contexts(2, 1)[0]
    try:
        plain = _run(g160_wrapper, x, c1, cuc, hint, noises)
        base = _run(g160_wrapper, x, cc, cuc, hint, noises)
        got = _run(g160_wrapper, x, cc, cuc, hint, noises, region_ctx=[c1], masks=np.full((1, 3, 128, 192), 255, np.uint8))
    finally:
        _restore(g160_wrapper)
    assert np.array_equal(_bits(got), _bits(plain)), _rel(got, plain)
    assert not np.array_equal(_bits(base), _bits(plain)), "the two prompts give the same clip: the test shows nothing"


def test_hard_split_is_the_per_cell_select_of_two_plain_calls(g160_wrapper):
    """F = 0, left half / right half at a cell boundary: ONE call of the closure against two plain calls of the wrapped closure."""
    from ccedit_amd import ops, regions
    w = g160_wrapper
    x, cc, cuc, hint, _ = _clip_inputs(43, 3)
    c1 = _contexts(3, 1)[0].cuda()
    _, denoiser = _make_sampler_and_denoiser()

    def denoise(inp, sigma, cond):
        return denoiser(w, inp, sigma, cond)

    x2 = torch.cat([x, x]).cuda()
    ops.set_mark(x2, "_cfg_twin_halves", True)
    sigma = torch.tensor([3.0, 3.0])
    h2 = torch.cat([hint, hint]).cuda()
    cond = dict(crossattn=torch.cat([cuc, cc]).cuda(), control_hint=h2)
    coef = regions.weights(torch.from_numpy(_half_masks(3)).cuda(), 0)
    try:
        w.reset_caches()
        got = regions.RegionDenoiser(denoise, [cc.cuda(), c1], coef, wrapper=w)(x2, sigma, cond).cpu()
        _restore(w)
        y0 = denoise(x2, sigma, cond).cpu()
        y1 = denoise(x2, sigma, dict(crossattn=torch.cat([cuc.cuda(), c1]), control_hint=h2)).cpu()
    finally:
        _restore(w)
    right = torch.zeros(16, 24, dtype=torch.bool)
    right[:, 12:] = True
    want = torch.where(right, y1, y0)
    assert np.array_equal(_bits(got), _bits(want)), _rel(got, want)
    assert not np.array_equal(_bits(y0), _bits(y1))


@pytest.mark.parametrize("k", [2, 3])
def test_region_contexts_replay_their_graphs_and_keep_the_caches(g160_wrapper, k):
    """K + 1 contexts, 3 steps = 5 sampler evaluations = 5 (K + 1) network evaluations: each context's key is evaluated eagerly once,
    captured once and replayed for the rest; the CFG marks reach the network (`_twin_val` stays empty); ONE hint-stem entry; the text
    K / V projection of each network ran once per context (K = 3: 8 entries, above the plain clip's limit of 6 — no eviction)."""
    w = g160_wrapper
    if not w.use_graph:
        pytest.skip("HIP graphs are switched off by policy")
    nets = (w.diffusion_model, w.diffusion_model.controlnet)
    calls = {id(n): 0 for n in nets}

    def counting(net):
        inner = type(net).text_kv.__get__(net)

        def text_kv(ctx2d):
            calls[id(net)] += int(torch.is_tensor(ctx2d))      # (run() hands a finished TextKV through the same method: no projection)
            return inner(ctx2d)
        return text_kv

    try:
        for n in nets:
            n.text_kv = counting(n)
        out = _run(w, *_clip_inputs(44 + k, 3), region_ctx=_contexts(4, k), masks=_half_masks(3, k))
        counts = dict(w.graph_counts)
        assert counts == dict(eager=k + 1, capture=k + 1, replay=3 * (k + 1)), counts
        assert not w._twin_val, "the network compared CFG halves on the device: a mark was lost on the way through the regions"
        assert len(w._graphs) == k + 1 and all(e.captured for e in w._graphs.values())
        assert len(w._hint_val) == 1, "the hint tensor is the same object for all regions: one cached stem output"
        assert [calls[id(n)] for n in nets] == [k + 1, k + 1], [calls[id(n)] for n in nets]
        assert len(w._tkv_val) == 2 * (k + 1)
        assert bool(torch.isfinite(out).all()) and out.shape == (1, 4, 3, 16, 24)
        # the limits of a plain clip come back with reserve_windows(0)
        w.reserve_windows(0)
        assert (w._graph_slots, w._hint_slots, w._graph_pool) == (2, 4, None) and w._tkv_slots == 6
    finally:
        for n in nets:
            n.__dict__.pop("text_kv", None)
        _restore(w)


def test_graphed_regions_equal_eager_regions(g160_wrapper):
    w = g160_wrapper
    inputs = _clip_inputs(47, 3)
    kw = dict(region_ctx=_contexts(5, 2), masks=_half_masks(3, 2))
    saved = w.use_graph
    try:
        graphed = _run(w, *inputs, **kw)
        w.use_graph = False
        eager = _run(w, *inputs, **kw)
    finally:
        w.use_graph = saved
        _restore(w)
    assert np.array_equal(_bits(graphed), _bits(eager)), _rel(graphed, eager)


def test_regions_outside_windows(g160_wrapper):
    """N = 6, T = 3, overlap 1 (3 windows), K = 1: 2 x 3 graph keys in one pool, all replayed after their capture."""
    w = g160_wrapper
    if not w.use_graph:
        pytest.skip("HIP graphs are switched off by policy")
    try:
        out = _run(w, *_clip_inputs(48, 6), region_ctx=_contexts(6, 1), masks=_half_masks(6), window=3, overlap=1)
        counts = dict(w.graph_counts)
        assert counts == dict(eager=6, capture=6, replay=18), counts
        assert w._graph_slots == 6 and len(w._graphs) == 6 and all(e.captured for e in w._graphs.values())
        assert w._graph_pool is not None and len(w._hint_val) == 3
        assert bool(torch.isfinite(out).all()) and out.shape == (1, 4, 6, 16, 24)
    finally:
        _restore(w)


# ---- 3. against the fp32 oracle ------------------------------------------------------------------
def test_region_clip_vs_oracle(g160_wrapper):
    """K = 1 with a feathered half-frame mask (F = 1), 3 steps of DPMPP2SAncestral + VanillaCFGTV2V(7.5) + DiscreteDenoiser with injected
    noise, against the CPU oracle: the region closure restated in torch around oracle.discrete_denoise / network_forward, coefficients
    from the numpy restatement.  Budget: TRAJ_TOL, the plain trajectory's own — the fusion is a convex combination of the regions'
    outputs, one fp32 rounding per term.  Measured on an MI355X: see DESIGN.md section 3.22."""
    from ccedit_amd.sgm_compat import build_network_spec
    from ccedit_amd.utils.synth import synth_state_dict
    from oracle import ccedit_oracle as O
    n, steps = 3, 3
    x, cc, cuc, hint, noises = _clip_inputs(49, n, steps)
    c1 = _contexts(7, 1)[0]
    masks = _half_masks(n)
    try:
        got = _run(g160_wrapper, x, cc, cuc, hint, noises, region_ctx=[c1], masks=masks, feather=1, steps=steps)
    finally:
        _restore(g160_wrapper)

    cfg = O.NetConfig(**G160)
    sd = synth_state_dict(build_network_spec(G160))
    table = O.denoiser_sigmas(1000)
    coef_t = torch.from_numpy(RN.region_weights(masks, 1))
    assert bool(((coef_t > 0) & (coef_t < 1)).any())

    def network(xx, idx, cond):
        return O.network_forward(sd, cfg, xx, idx, cond)

    def regioned(xx, sigma, cond):
        out = torch.zeros_like(xx)
        for r, ctx in enumerate((cc, c1)):
            ci = dict(cond, crossattn=torch.cat((cond["crossattn"][:1], ctx), 0))
            out += coef_t[r][None, None] * O.discrete_denoise(network, table, xx, sigma, ci)
        return out

    it = iter(noises)
    with torch.no_grad():
        ref = O.dpmpp2s_ancestral_sample(regioned, x.clone(), dict(crossattn=cc, control_hint=hint), dict(crossattn=cuc, control_hint=hint.clone()),
                                         num_steps=steps, scale=7.5, noise_fn=lambda v: next(it))
    r = _rel(got, ref)
    print(f"region clip (K=1, feathered half frame, 3 frames, 3 steps): final latent rel rms err vs fp32 oracle: {r:.4f}")
    assert bool(torch.isfinite(got).all())
    assert r < TRAJ_TOL, r


# ---- 4. entry point ------------------------------------------------------------------------------
def _write_config(tmp_path):
    import yaml
    from ccedit_amd.sgm_compat import engine_config
    cfg = os.path.join(str(tmp_path), "tv2v.yaml")
    with open(cfg, "w") as f:
        yaml.safe_dump(dict(model=engine_config(crossframe=False, vae_ch=32, model_channels=64, num_heads=2, context_dim=64)), f)
    return cfg


@pytest.fixture()
def clip(tmp_path):
    """A 64 x 128 frame directory of 9 frames (3 keyframes at 9 -> 3 fps), a half-frame mask image and a black one."""
    from PIL import Image
    rs = np.random.RandomState(8)
    vdir = tmp_path / "clips" / "bear"
    vdir.mkdir(parents=True)
    for i in range(9):
        Image.fromarray(rs.randint(0, 256, (64, 128, 3)).astype(np.uint8)).save(str(vdir / f"{i:03d}.png"))
    half = np.zeros((64, 128), np.uint8)
    half[:, 64:] = 255
    Image.fromarray(half).save(str(tmp_path / "half.png"))
    Image.fromarray(np.zeros((64, 128), np.uint8)).save(str(tmp_path / "black.png"))
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
def test_entry_point_edits_a_region_and_logs_it(clip, monkeypatch):
    _need_gpu()
    tmp_path, base = clip
    half = str(tmp_path / "half.png")
    res, log = _job(monkeypatch, base, str(tmp_path / "region"), "--region_prompt", "a snow field", "--region_mask", half)
    assert res.shape == (3, 64, 128, 3) and np.isfinite(res).all() and len({res[f].tobytes() for f in range(3)}) == 3
    assert log["regions"] == [dict(prompt="a snow field", mask=half, feather=1, tracked=False)]
    plain, plog = _job(monkeypatch, base, str(tmp_path / "plain"))
    assert "regions" not in plog and not np.array_equal(res, plain), "the region prompt changed nothing"


@pytest.mark.timeout(900)
def test_entry_point_with_a_black_region_writes_the_plain_bytes(clip, monkeypatch):
    _need_gpu()
    tmp_path, base = clip
    res, log = _job(monkeypatch, base, str(tmp_path / "black"), "--region_prompt", "a snow field", "--region_mask", str(tmp_path / "black.png"),
                    "--region_feather", "0")
    plain, _ = _job(monkeypatch, base, str(tmp_path / "plain"))
    assert log["regions"][0]["feather"] == 0
    assert res.tobytes() == plain.tobytes()


@pytest.mark.timeout(900)
def test_entry_point_tracks_a_region_mask(clip, monkeypatch):
    _need_gpu()
    tmp_path, base = clip
    half = str(tmp_path / "half.png")
    res, log = _job(monkeypatch, base, str(tmp_path / "tracked"), "--region_prompt", "a snow field", "--region_mask", half, "--region_track",
                    "--region_frame", "4")
    assert res.shape == (3, 64, 128, 3) and np.isfinite(res).all()
    assert log["regions"] == [dict(prompt="a snow field", mask=half, feather=1, tracked=True)]
