"""Large frames on a real MI355X (ccedit_amd/tiles.py, csrc/tile.hip, --tile_h / --tile_w / --tile_overlap).

Exact (no tolerance): the two kernels against the numpy float32 restatement of their definition (tests/_tiles_numpy.py); a frame of
one tile and the tiles of an overlap-free frame against the plain sampler; first-stage encode / decode in groups against the single
call; the network wrapper's evaluation counts; graphed against eager.  Against the fp32 CPU oracle: one tiled clip at the reduced size
of the committed goldens, with the budget of the plain sampler trajectory (tests/test_network_gpu.py: TRAJ_TOL)."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _tiles_numpy as TN  # noqa: E402

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
    return t.detach().cpu().contiguous().numpy().view(np.int32)


def _same(got, want):
    g, w = _bits(got), np.ascontiguousarray(want).view(np.int32)
    assert g.shape == w.shape, (g.shape, w.shape)
    assert np.array_equal(g, w), f"{int((g != w).sum())} of {g.size} elements differ"


# ---- 1. the kernels ------------------------------------------------------------------------------
def _planned(h, w, th, tw, oh, ow):
    return TN.plan2d(h, w, th, tw, oh, ow)


def _by_hand(h, w, th, tw, starts):
    return list(starts), TN.tables(h, w, th, tw, starts)


# name -> (B, C, N, h, w, th, tw, starts, coef)
KERNEL_CASES = {
    "vector": (2, 4, 3, 24, 40, 16, 24, *_planned(24, 40, 16, 24, 8, 8)),
    # odd widths, no multiple of 8 anywhere (the kernels do not need one, only the plan does): tables by hand, by the same formula
    "scalar": (1, 3, 2, 11, 13, 8, 8, *_by_hand(11, 13, 8, 8, [(sy, sx) for sy in TN.axis_starts(11, 8, 3) for sx in TN.axis_starts(13, 8, 3)])),
    "one_tile": (1, 4, 2, 16, 24, 16, 24, *_planned(16, 24, 16, 24, 0, 0)),
    "no_overlap": (2, 4, 2, 32, 48, 16, 24, *_planned(32, 48, 16, 24, 0, 0)),
    # tw % 4 == 0 and w % 4 == 0, but tiles start at column 7: rows of those tiles fall back to element-wise accesses
    "row_fallback": (1, 2, 2, 12, 28, 8, 12, *_by_hand(12, 28, 8, 12, [(sy, sx) for sy in (0, 4) for sx in (0, 7, 16)])),
    "pulled_back": (1, 4, 1, 90, 160, 64, 96, *_planned(90, 160, 64, 96, 16, 24)),        # 720 x 1280: starts 26 and 64
}


def test_kernel_cases_are_what_they_claim():
    assert KERNEL_CASES["scalar"][7] == [(0, 0), (0, 5), (3, 0), (3, 5)]
    assert len(KERNEL_CASES["one_tile"][7]) == 1 and np.all(KERNEL_CASES["one_tile"][8] == 1.0)
    assert len(KERNEL_CASES["no_overlap"][7]) == 4 and np.all(KERNEL_CASES["no_overlap"][8] == 1.0)
    assert any(sx % 4 for _, sx in KERNEL_CASES["row_fallback"][7]) and KERNEL_CASES["row_fallback"][6] % 4 == 0


@pytest.mark.parametrize("name", list(KERNEL_CASES))
def test_tile_gather_and_fuse_are_exact(name):
    _need_gpu()
    from ccedit_amd import ops
    b, c, n, h, w, th, tw, starts, coef = KERNEL_CASES[name]
    g = torch.Generator().manual_seed(100 * h + w)
    x = torch.randn(b, c, n, h, w, generator=g)
    sd = torch.tensor(starts, dtype=torch.int32).reshape(-1, 2).cuda()
    xt = ops.tile_gather(x.cuda(), sd, th, tw)
    assert xt.shape == (len(starts), b, c, n, th, tw) and xt.is_contiguous()
    _same(xt, TN.gather(x.numpy(), starts, th, tw))
    ys = [torch.randn(b, c, n, th, tw, generator=g) for _ in starts]
    want = TN.fuse([y.numpy() for y in ys], starts, coef, h, w)
    got = ops.tile_fuse([y.cuda() for y in ys], sd, torch.from_numpy(coef).cuda(), h, w)
    assert got.shape == (b, c, n, h, w)
    _same(got, want)
    # an element covered by one tile is that tile's element, bit for bit
    cover = np.zeros((h, w), np.int64)
    for sy, sx in starts:
        cover[sy:sy + th, sx:sx + tw] += 1
    assert cover.min() >= 1
    gb = _bits(got)
    for i, (sy, sx) in enumerate(starts):
        one = cover[sy:sy + th, sx:sx + tw] == 1
        assert np.array_equal(gb[..., sy:sy + th, sx:sx + tw][..., one], _bits(ys[i])[..., one])


def test_tile_fuse_reads_tiles_that_are_not_16_byte_aligned():
    """The tiles' outputs are read where they lie: a tensor 4, 8 or 12 bytes off a 16-byte boundary takes the element-wise loads; so
    does a source frame or an output that is off the boundary."""
    _need_gpu()
    from ccedit_amd import ops
    b, c, n, h, w, th, tw, starts, coef = KERNEL_CASES["vector"]
    g = torch.Generator().manual_seed(5)
    ys = [torch.randn(b, c, n, th, tw, generator=g) for _ in starts]

    def off_view(t, off):
        buf = torch.empty(t.numel() + 4, dtype=torch.float32, device="cuda")
        v = buf[off:off + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.is_contiguous() and (v.data_ptr() % 16 == 0) == (off == 0)
        return v

    dev = [off_view(y, k) for k, y in enumerate(ys)]                     # tile 0 aligned, the others 4 / 8 / 12 bytes off
    sd = torch.tensor(starts, dtype=torch.int32).reshape(-1, 2).cuda()
    want = TN.fuse([y.numpy() for y in ys], starts, coef, h, w)
    _same(ops.tile_fuse(dev, sd, torch.from_numpy(coef).cuda(), h, w), want)
    out = off_view(torch.zeros(b, c, n, h, w), 1)
    _same(ops.tile_fuse(dev, sd, torch.from_numpy(coef).cuda(), h, w, out=out), want)
    x = torch.randn(b, c, n, h, w, generator=g)
    _same(ops.tile_gather(off_view(x, 3), sd, th, tw), TN.gather(x.numpy(), starts, th, tw))


def test_bad_device_tables_stay_inside_the_tensor():
    """A start below 0 or past h - th / w - tw is clamped by the kernels: the result is the restatement's with the clamped starts (and
    the given coefficients)."""
    _need_gpu()
    from ccedit_amd import ops
    b, c, n, h, w, th, tw = 1, 2, 2, 24, 40, 16, 24
    bad = [(-5, 0), (0, 99), (1000, -1), (8, 16)]
    good = TN.clamp_starts(bad, h, w, th, tw)
    assert good == [(0, 0), (0, 16), (8, 0), (8, 16)]
    coef = TN.tables(h, w, th, tw, good)
    g = torch.Generator().manual_seed(6)
    x = torch.randn(b, c, n, h, w, generator=g)
    sd = torch.tensor(bad, dtype=torch.int32).reshape(-1, 2).cuda()
    _same(ops.tile_gather(x.cuda(), sd, th, tw), TN.gather(x.numpy(), good, th, tw))
    ys = [torch.randn(b, c, n, th, tw, generator=g) for _ in bad]
    _same(ops.tile_fuse([y.cuda() for y in ys], sd, torch.from_numpy(coef).cuda(), h, w), TN.fuse([y.numpy() for y in ys], good, coef, h, w))
    # an element no tile covers is 0: one tile in a corner of the frame
    one = torch.tensor([[0, 0]], dtype=torch.int32).cuda()
    got = ops.tile_fuse([ys[0].cuda()], one, torch.ones(1, th, tw).cuda(), h, w)
    want = np.zeros((b, c, n, h, w), np.float32)
    want[..., :th, :tw] = ys[0].numpy()
    _same(got, want)


def test_tile_entry_points_refuse_bad_arguments():
    _need_gpu()
    from ccedit_amd import hip, ops
    lib = hip.lib()
    x = torch.zeros(1, 4, 3, 16, 24, device="cuda")
    xt = torch.zeros(1, 12, 16, 24, device="cuda")
    sd = torch.zeros(1, 2, dtype=torch.int32, device="cuda")
    cf = torch.ones(1, 16, 24, device="cuda")
    tab = torch.tensor([xt.data_ptr()], dtype=torch.int64).cuda()
    ok = (x.data_ptr(), xt.data_ptr(), sd.data_ptr(), 1, 12, 16, 24, 16, 24, None)
    assert lib.ccedit_tile_gather(*ok) == 0
    bad_gather = [(None,) + ok[1:], ok[:1] + (None,) + ok[2:], ok[:2] + (None,) + ok[3:],            # null pointers
                  ok[:3] + (0,) + ok[4:], ok[:3] + (65,) + ok[4:], ok[:4] + (0,) + ok[5:],           # tiles 0, 65; planes 0
                  ok[:7] + (17, 24, None), ok[:7] + (16, 25, None), ok[:7] + (0, 24, None), ok[:7] + (16, -4, None)]
    for args in bad_gather:
        assert lib.ccedit_tile_gather(*args) != 0, args
    okf = (tab.data_ptr(), x.data_ptr(), sd.data_ptr(), cf.data_ptr(), 1, 12, 16, 24, 16, 24, None)
    assert lib.ccedit_tile_fuse(*okf) == 0
    bad_fuse = [(None,) + okf[1:], okf[:1] + (None,) + okf[2:], okf[:2] + (None,) + okf[3:], okf[:3] + (None,) + okf[4:],
                okf[:4] + (65,) + okf[5:], okf[:4] + (0,) + okf[5:], okf[:5] + (-1,) + okf[6:], okf[:8] + (17, 24, None), okf[:8] + (16, 32, None),
                (tab.data_ptr() + 4,) + okf[1:]]
    for args in bad_fuse:
        assert lib.ccedit_tile_fuse(*args) != 0, args
    torch.cuda.synchronize()
    with pytest.raises(hip.HipLibraryError, match="h >= th"):
        ops.tile_gather(x, sd, 17, 24)                                     # a tile taller than the frame
    with pytest.raises(hip.HipLibraryError, match="1 ... 64"):
        ops.tile_gather(x, torch.zeros(65, 2, dtype=torch.int32, device="cuda"), 8, 8)
    with pytest.raises(hip.HipLibraryError, match="w >= tw"):
        ops.tile_fuse([xt.view(1, 4, 3, 16, 24)], sd, cf, 16, 16)
    with pytest.raises(ValueError):
        ops.tile_gather(x.half(), sd, 16, 24)
    with pytest.raises(ValueError):
        ops.tile_gather(x, sd.view(2), 16, 24)
    with pytest.raises(ValueError):
        ops.tile_fuse([xt.view(1, 4, 3, 16, 24)], sd, cf[:, :8].contiguous(), 16, 24)


# ---- 2. the tiled closure in the sampler -------------------------------------------------------
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


def _clip_inputs(seed, n, lh=16, lw=24, steps=3):
    """The reduced shape of the committed goldens (context 77 x 128) with n keyframes of a latent lh x lw."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(1, 4, n, lh, lw, generator=g)
    cc, cuc = torch.randn(1, 77, 128, generator=g), torch.randn(1, 77, 128, generator=g)
    hint = (torch.rand(1, 1, n, 8 * lh, 8 * lw, generator=g) * 2 - 1).repeat(1, 3, 1, 1, 1)
    noises = [torch.randn(1, 4, n, lh, lw, generator=g) for _ in range(steps)]
    return x, cc, cuc, hint, noises


def _crop(inputs, sy, sx, th, tw):
    x, cc, cuc, hint, noises = inputs
    lat = lambda v: v[..., sy:sy + th, sx:sx + tw].contiguous()
    return lat(x), cc, cuc, hint[..., 8 * sy:8 * (sy + th), 8 * sx:8 * (sx + tw)].contiguous(), [lat(v) for v in noises]


def _run(wrapper, x, cc, cuc, hint, noises, tile=None, overlap=None, window=0, window_overlap=None, steps=3):
    """One clip through a fresh sampler: plain (tile None) or through the tiled closure; per-step noise injected."""
    from ccedit_amd.tiles import TiledDenoiser
    sampler, denoiser = _make_sampler_and_denoiser(steps)
    it = iter([v.cuda() for v in noises])
    sampler.noise_sampler = lambda xx: next(it)

    def denoise(inp, sigma, cond):          # the closure of scripts/sampling/sampling_tv2v.py: sample_latent
        return denoiser(wrapper, inp, sigma, cond)

    closure = denoise if tile is None else TiledDenoiser(denoise, tile, overlap, wrapper=wrapper, window=window, window_overlap=window_overlap)
    c = dict(crossattn=cc.cuda(), control_hint=hint.cuda())
    uc = dict(crossattn=cuc.cuda(), control_hint=hint.clone().cuda())
    wrapper.reset_caches()
    return sampler(closure, x.clone().cuda(), c, uc=uc).cpu()


def _restore(w):
    w.reserve_windows(0)
    w.reset_caches()


def test_one_tile_is_the_plain_sampler_bit_for_bit(g160_wrapper):
    """Frame == tile through the tiled closure: gather and fuse are bit copies, the sampled latent is the plain sampler's."""
    inputs = _clip_inputs(41, 3)
    try:
        plain = _run(g160_wrapper, *inputs)
        tiled = _run(g160_wrapper, *inputs, tile=(16, 24), overlap=(8, 8))
    finally:
        _restore(g160_wrapper)
    assert bool(torch.isfinite(plain).all()) and plain.shape == (1, 4, 3, 16, 24)
    assert np.array_equal(_bits(tiled), _bits(plain)), _rel(tiled, plain)


def test_tiles_without_overlap_are_plain_runs_on_their_crops(g160_wrapper):
    """Latent 16 x 48, tile 16 x 24, overlap 0: the two tiles do not interact, so each half is what a plain run gives on that crop of
    the initial latent, the hint and the noises."""
    inputs = _clip_inputs(42, 3, 16, 48)
    try:
        tiled = _run(g160_wrapper, *inputs, tile=(16, 24), overlap=(0, 0))
        left = _run(g160_wrapper, *_crop(inputs, 0, 0, 16, 24))
        right = _run(g160_wrapper, *_crop(inputs, 0, 24, 16, 24))
    finally:
        _restore(g160_wrapper)
    assert tiled.shape == (1, 4, 3, 16, 48) and bool(torch.isfinite(tiled).all())
    assert np.array_equal(_bits(tiled[..., :24]), _bits(left)), _rel(tiled[..., :24], left)
    assert np.array_equal(_bits(tiled[..., 24:]), _bits(right)), _rel(tiled[..., 24:], right)


def test_four_tiles_replay_four_graphs_and_equal_the_eager_run(g160_wrapper):
    """Four tiles (latent 24 x 40, tile 16 x 24, overlap 8; 3 steps = 5 sampler evaluations = 20 network evaluations): each tile's key is
    evaluated eagerly once, captured once and replayed for the rest; the CFG marks reach the network (no device compare: `_twin_val`
    stays empty); the hint stem is computed once per tile; the graphed clip is the eager clip, bit for bit."""
    w = g160_wrapper
    if not w.use_graph:
        pytest.skip("HIP graphs are switched off by policy")
    inputs = _clip_inputs(43, 3, 24, 40)
    saved = w.use_graph
    try:
        graphed = _run(w, *inputs, tile=(16, 24), overlap=(8, 8))
        counts = dict(w.graph_counts)
        assert counts == dict(eager=4, capture=4, replay=12), counts
        assert not w._twin_val, "the network compared CFG halves on the device: a mark was lost on the way through the tiles"
        assert len(w._graphs) == 4 and all(e.captured for e in w._graphs.values())
        assert len(w._hint_val) == 4, "one cached hint-stem output per tile"
        assert bool(torch.isfinite(graphed).all()) and graphed.shape == (1, 4, 3, 24, 40)
        w.reserve_windows(0)                                   # the limits of a plain clip come back
        assert (w._graph_slots, w._hint_slots, w._graph_pool) == (2, 4, None)
        w.use_graph = False
        eager = _run(w, *inputs, tile=(16, 24), overlap=(8, 8))
    finally:
        w.use_graph = saved
        _restore(w)
    assert np.array_equal(_bits(graphed), _bits(eager)), _rel(graphed, eager)


def test_tiles_times_windows(g160_wrapper):
    """N = 6 through windows of 3 (overlap 1: 3 windows) inside each of the four tiles: 12 conditioning keys, 12 graphs in one pool; the
    clip is finite, of the frame's shape, and the graphed run is the eager run bit for bit."""
    w = g160_wrapper
    inputs = _clip_inputs(44, 6, 24, 40)
    saved = w.use_graph
    kw = dict(tile=(16, 24), overlap=(8, 8), window=3, window_overlap=1)
    try:
        graphed = _run(w, *inputs, **kw)
        if saved:
            assert w._graph_slots == 12 and len(w._graphs) == 12 and all(e.captured for e in w._graphs.values()), len(w._graphs)
            assert dict(w.graph_counts) == dict(eager=12, capture=12, replay=36), w.graph_counts
            assert not w._twin_val
        w.use_graph = False
        eager = _run(w, *inputs, **kw)
    finally:
        w.use_graph = saved
        _restore(w)
    assert graphed.shape == (1, 4, 6, 24, 40) and bool(torch.isfinite(graphed).all())
    assert np.array_equal(_bits(graphed), _bits(eager)), _rel(graphed, eager)


# ---- 3. against the fp32 oracle ------------------------------------------------------------------
def test_tiled_clip_vs_oracle(g160_wrapper):
    """Four tiles (latent 24 x 40, tile 16 x 24, overlap 8), N = 3, 3 steps of DPMPP2SAncestral + VanillaCFGTV2V(7.5) + DiscreteDenoiser
    with injected noise, against the CPU oracle: the tiled closure restated in torch around oracle.discrete_denoise / network_forward,
    handed to oracle.dpmpp2s_ancestral_sample.  Budget: TRAJ_TOL, the plain trajectory's own — the fusion is a convex combination of
    the tiles' outputs and cannot widen the worst tile's error."""
    from ccedit_amd.sgm_compat import build_network_spec
    from ccedit_amd.tiles import plan2d
    from ccedit_amd.utils.synth import synth_state_dict
    from oracle import ccedit_oracle as O
    n, steps, lh, lw, th, tw = 3, 3, 24, 40, 16, 24
    x, cc, cuc, hint, noises = _clip_inputs(45, n, lh, lw, steps)
    try:
        got = _run(g160_wrapper, x, cc, cuc, hint, noises, tile=(th, tw), overlap=(8, 8), steps=steps)
    finally:
        _restore(g160_wrapper)

    cfg = O.NetConfig(**G160)
    sd = synth_state_dict(build_network_spec(G160))
    table = O.denoiser_sigmas(1000)
    starts, coef = plan2d(lh, lw, th, tw, 8, 8)
    assert starts == [(0, 0), (0, 16), (8, 0), (8, 16)]
    coef_t = torch.from_numpy(coef)

    def network(xx, idx, cond):
        return O.network_forward(sd, cfg, xx, idx, cond)

    def tiled(xx, sigma, cond):
        out = torch.zeros_like(xx)
        for i, (sy, sx) in enumerate(starts):
            ci = dict(cond, control_hint=cond["control_hint"][..., 8 * sy:8 * (sy + th), 8 * sx:8 * (sx + tw)])
            y = O.discrete_denoise(network, table, xx[..., sy:sy + th, sx:sx + tw], sigma, ci)
            out[..., sy:sy + th, sx:sx + tw] += coef_t[i].view(1, 1, 1, th, tw) * y
        return out

    it = iter(noises)
    with torch.no_grad():
        ref = O.dpmpp2s_ancestral_sample(tiled, x.clone(), dict(crossattn=cc, control_hint=hint), dict(crossattn=cuc, control_hint=hint.clone()),
                                         num_steps=steps, scale=7.5, noise_fn=lambda v: next(it))
    r = _rel(got, ref)
    print(f"tiled clip (24x40 in four tiles of 16x24, 3 steps): final latent rel rms err vs fp32 oracle: {r:.4f}")
    assert bool(torch.isfinite(got).all())
    assert r < TRAJ_TOL, r


# ---- 4. first stage in groups, entry point -------------------------------------------------------
def _write_config(tmp_path):
    import yaml
    from ccedit_amd.sgm_compat import engine_config
    cfg = os.path.join(str(tmp_path), "tv2v.yaml")
    with open(cfg, "w") as f:
        yaml.safe_dump(dict(model=engine_config(crossframe=False, vae_ch=32, model_channels=64, num_heads=2, context_dim=64)), f)
    return cfg


@pytest.mark.timeout(900)
def test_first_stage_in_groups_equals_the_single_call_at_two_tiles(tmp_path):
    """A frame of two tiles (64 x 128 px with a tile of 64 x 64), T_plain = 4: first_stage_group gives 2 frames per call; encode (given
    noise) and decode of 5 frames in groups of 2 (2 + 2 + 1) have the single call's bits."""
    _need_gpu()
    from ccedit_amd.tiles import first_stage_group
    from ccedit_amd.windows import GroupedFirstStage
    from scripts.sampling import sampling_tv2v as S
    args = S.parse_args(["--config_path", _write_config(tmp_path), "--synthetic", "--H", "64", "--W", "128", "--tile_h", "64", "--tile_w", "64",
                         "--num_keyframes", "4"])
    assert S.tiling(args) and S.first_stage_frames(args) == first_stage_group(4, 8, 8, 8, 16) == 2
    torch.set_grad_enabled(False)
    model, dev = S.build_model(args)
    g = torch.Generator().manual_seed(9)
    frames = (torch.rand(1, 3, 5, 64, 128, generator=g) * 2 - 1).to(dev)
    noise = torch.randn(5, 4, 8, 16, generator=g)
    grouped = GroupedFirstStage(model, S.first_stage_frames(args))
    z = model.encode_first_stage(frames, noise=noise)
    zg = grouped.encode_first_stage(frames, noise=noise)
    assert z.shape == zg.shape == (1, 4, 5, 8, 16) and np.array_equal(_bits(zg), _bits(z)), _rel(zg, z)
    d = model.decode_first_stage(z)
    dg = grouped.decode_first_stage(z)
    assert d.shape == dg.shape == (1, 3, 5, 64, 128) and np.array_equal(_bits(dg), _bits(d)), _rel(dg, d)


def _script(*argv):
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "sampling", "sampling_tv2v.py"), *argv]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=450, cwd=ROOT)


def _animation(save_dir):
    """The animated PNG perform_save_locally_video wrote under `save_dir` (png/animation-XXXX.png; grid/ holds a still)."""
    files = sorted(glob.glob(os.path.join(save_dir, "png", "animation-*.png")))
    assert len(files) == 1, (save_dir, files)
    return files[0]


def _apng_frames(path):
    from PIL import Image, ImageSequence
    with Image.open(path) as im:
        return np.stack([np.array(f.convert("RGB")) for f in ImageSequence.Iterator(im)])


@pytest.mark.timeout(1500)
def test_entry_point_writes_large_frames(tmp_path):
    """scripts/sampling/sampling_tv2v.py with --tile_h 64 --tile_w 64 on the tiny config.  Run 1: 128 x 192 frames, --gpu_io --save_type
    png: result/ decodes to 3 frames of 128 x 192.  Run 2: the same through job mode with --inpainting_mode --mask_composite, a mask and
    --window_frames 2: outside the mask the result is original/ byte for byte.  Run 3: 72 x 104 runs with the tile flags and is refused
    with the network's multiple-of-64 error without them."""
    _need_gpu()
    from PIL import Image
    cfg = _write_config(tmp_path)
    common = ["--config_path", cfg, "--synthetic", "--num_keyframes", "3", "--sample_steps", "2", "--sampler_name", "DPMPP2SAncestralSampler",
              "--noise_seed", "1", "--gpu_io", "--save_type", "png"]
    tile = ["--tile_h", "64", "--tile_w", "64"]
    # run 1
    out = str(tmp_path / "plain")
    r = _script(*common, *tile, "--H", "128", "--W", "192", "--save_path", out)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    fr = _apng_frames(_animation(os.path.join(out, "result")))
    assert fr.shape == (3, 128, 192, 3) and len({f.tobytes() for f in fr}) == 3, fr.shape
    # run 2
    rs = np.random.RandomState(6)
    vdir = tmp_path / "clips" / "fox"
    vdir.mkdir(parents=True)
    for i in range(9):
        Image.fromarray(rs.randint(0, 256, (128, 192, 3)).astype(np.uint8)).save(str(vdir / f"{i:03d}.png"))
    mask = np.zeros((128, 192), np.uint8)
    mask[:, 96:] = 255                                                            # left half black: keep
    Image.fromarray(mask).save(str(tmp_path / "clips" / "fox.mask.png"))
    keep = mask == 0
    out = str(tmp_path / "masked")
    r = _script(*common, *tile, "--H", "128", "--W", "192", "--save_path", out, "--inpainting_mode", "--mask_composite", "--window_frames", "2",
                "--original_fps", "9", "--target_fps", "3", "--prompt", "a red fox", "--video_path", str(vdir), "--batch_size", "1")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    orig = _apng_frames(_animation(os.path.join(out, "default", "original")))
    res = _apng_frames(_animation(os.path.join(out, "default", "result")))
    assert orig.shape == res.shape == (3, 128, 192, 3), (orig.shape, res.shape)
    k = np.broadcast_to(keep[None, ..., None], res.shape)
    assert np.array_equal(res[k], orig[k]), f"{int((res[k] != orig[k]).sum())} kept bytes differ"
    assert (res[~k] != orig[~k]).mean() > 0.5, "the edited region equals the original"
    # run 3
    out = str(tmp_path / "odd")
    r = _script(*common, *tile, "--H", "72", "--W", "104", "--save_path", out)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    fr = _apng_frames(_animation(os.path.join(out, "result")))
    assert fr.shape == (3, 72, 104, 3), fr.shape
    r = _script(*common, "--H", "72", "--W", "104", "--save_path", str(tmp_path / "odd_plain"))
    assert r.returncode != 0 and "multiples of 64" in r.stderr, r.stderr[-3000:]
