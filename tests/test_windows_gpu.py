"""Long clips on a real MI355X (ccedit_amd/windows.py, csrc/window.hip, --window_frames).

Exact (no tolerance): the two kernels against torch slicing / the numpy float32 loop of their definition; a clip of one window and the
first window of an overlap-free clip against the plain sampler; first-stage encode / decode in groups against the single call; the
network wrapper's evaluation counts.  Against the fp32 CPU oracle: one windowed clip at the reduced size of the committed goldens,
with the budget of the plain sampler trajectory (tests/test_network_gpu.py: TRAJ_TOL)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

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


# ---- 1. the kernels ------------------------------------------------------------------------------
def _fuse_reference(ys, starts, coef, n):
    """The definition, in numpy float32: per frame the windows in ascending order; the first term is the product alone, every further
    term one multiply (rounded) then one add (rounded)."""
    b, c, t, h, w = ys[0].shape
    out = np.zeros((b, c, n, h, w), np.float32)
    for f in range(n):
        first = True
        for i, s in enumerate(starts):
            j = f - s
            if 0 <= j < t:
                term = (coef[i, j] * ys[i][:, :, j]).astype(np.float32)
                out[:, :, f] = term if first else (out[:, :, f] + term).astype(np.float32)
                first = False
        assert not first, f"frame {f} is covered by no window"
    return out


# (B, C, N, T, overlap, h, w)
KERNEL_CASES = [
    (2, 4, 10, 4, 2, 4, 8),          # P % 4 == 0: 16-byte accesses
    (2, 3, 9, 4, 1, 3, 5),           # odd P: one element per access
    (1, 4, 5, 5, 2, 4, 4),           # W = 1
    (2, 4, 12, 4, 0, 4, 4),          # overlap 0, N a multiple of T: every frame a bit copy
    (2, 4, 14, 4, 0, 2, 6),          # overlap 0, the last window pulled back
    (1, 4, 11, 4, 3, 3, 4),          # overlap T - 1: up to T windows per frame
    (1, 2, 13, 5, 4, 3, 3),          # ... with odd P
    (2, 4, 41, 17, 8, 64, 96),       # production: 41 keyframes at 512 x 768, W = 4
]


@pytest.mark.parametrize("b,c,n,t,overlap,h,w", KERNEL_CASES)
def test_window_gather_and_fuse_are_exact(b, c, n, t, overlap, h, w):
    _need_gpu()
    from ccedit_amd import ops
    from ccedit_amd.windows import plan
    starts, coef = plan(n, t, overlap)
    g = torch.Generator().manual_seed(1000 * n + 10 * t + overlap)
    x = torch.randn(b, c, n, h, w, generator=g)
    sd = torch.tensor(starts, dtype=torch.int32).cuda()
    xw = ops.window_gather(x.cuda(), sd, t)
    assert xw.shape == (len(starts), b, c, t, h, w) and xw.is_contiguous()
    for i, s in enumerate(starts):
        assert np.array_equal(_bits(xw[i]), _bits(x[:, :, s:s + t])), f"window {i}"
    ys = [torch.randn(b, c, t, h, w, generator=g) for _ in starts]
    want = _fuse_reference([y.numpy() for y in ys], starts, coef, n)
    got = ops.window_fuse([y.cuda() for y in ys], sd, torch.from_numpy(coef).cuda(), n)
    assert got.shape == (b, c, n, h, w)
    assert np.array_equal(_bits(got), want.view(np.int32)), f"{int((_bits(got) != want.view(np.int32)).sum())} elements differ"
    # a frame covered by one window is that window's frame, bit for bit
    cover = np.zeros(n, np.int64)
    for s in starts:
        cover[s:s + t] += 1
    for i, s in enumerate(starts):
        for j in range(t):
            if cover[s + j] == 1:
                assert np.array_equal(_bits(got[:, :, s + j]), _bits(ys[i][:, :, j]))


def test_window_fuse_reads_windows_that_are_not_16_byte_aligned():
    """The windows' outputs are read where they lie: a tensor 4 bytes off a 16-byte boundary takes the element-wise loads."""
    _need_gpu()
    from ccedit_amd import ops
    from ccedit_amd.windows import plan
    b, c, n, t, h, w = 2, 4, 7, 3, 4, 8
    starts, coef = plan(n, t, 1)
    g = torch.Generator().manual_seed(5)
    ys = [torch.randn(b, c, t, h, w, generator=g) for _ in starts]
    dev = []
    for k, y in enumerate(ys):
        buf = torch.empty(y.numel() + 4, dtype=torch.float32, device="cuda")
        off = (k % 3) + 1 if k else 0                         # window 0 aligned, the others 4 / 8 / 12 bytes off
        v = buf[off:off + y.numel()].view(y.shape)
        v.copy_(y)
        assert v.is_contiguous() and (v.data_ptr() % 16 == 0) == (off == 0)
        dev.append(v)
    got = ops.window_fuse(dev, torch.tensor(starts, dtype=torch.int32).cuda(), torch.from_numpy(coef).cuda(), n)
    want = _fuse_reference([y.numpy() for y in ys], starts, coef, n)
    assert np.array_equal(_bits(got), want.view(np.int32))


def test_window_entry_points_refuse_bad_arguments():
    _need_gpu()
    from ccedit_amd import hip, ops
    x = torch.zeros(1, 4, 3, 4, 4, device="cuda")
    sd = torch.zeros(1, dtype=torch.int32, device="cuda")
    with pytest.raises(hip.HipLibraryError, match="N >= T"):
        ops.window_gather(x, sd, 4)                           # a window longer than the clip
    with pytest.raises(ValueError):
        ops.window_gather(x.half(), sd, 3)


# ---- 2. the windowed closure in the sampler ----------------------------------------------------
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


def _run(wrapper, x, cc, cuc, hint, noises, window=None, overlap=None, steps=3):
    """One clip through a fresh sampler: plain (window None) or through the windowed closure; per-step noise injected."""
    from ccedit_amd.windows import WindowedDenoiser
    sampler, denoiser = _make_sampler_and_denoiser(steps)
    it = iter([v.cuda() for v in noises])
    sampler.noise_sampler = lambda xx: next(it)

    def denoise(inp, sigma, cond):          # the closure of scripts/sampling/sampling_tv2v.py: sample_latent
        return denoiser(wrapper, inp, sigma, cond)

    closure = denoise if window is None else WindowedDenoiser(denoise, window, overlap, wrapper=wrapper)
    c = dict(crossattn=cc.cuda(), control_hint=hint.cuda())
    uc = dict(crossattn=cuc.cuda(), control_hint=hint.clone().cuda())
    wrapper.reset_caches()
    return sampler(closure, x.clone().cuda(), c, uc=uc).cpu()


def test_one_window_is_the_plain_sampler_bit_for_bit(g160_wrapper):
    """N == T through the windowed closure: gather and fuse are bit copies, the sampled latent is the plain sampler's."""
    inputs = _clip_inputs(31, 3)
    try:
        plain = _run(g160_wrapper, *inputs)
        windowed = _run(g160_wrapper, *inputs, window=3, overlap=1)
    finally:
        g160_wrapper.reserve_windows(0)
        g160_wrapper.reset_caches()
    assert bool(torch.isfinite(plain).all()) and plain.shape == (1, 4, 3, 16, 24)
    assert np.array_equal(_bits(windowed), _bits(plain)), _rel(windowed, plain)


def test_first_window_without_overlap_is_a_plain_run_on_its_frames(g160_wrapper):
    """overlap 0, N = 2 T: the windows do not interact, so frames [0, T) are what a plain run on the first T frames gives from the
    same initial latent, hint and noise slices."""
    t = 3
    x, cc, cuc, hint, noises = _clip_inputs(32, 2 * t)
    try:
        windowed = _run(g160_wrapper, x, cc, cuc, hint, noises, window=t, overlap=0)
        head = _run(g160_wrapper, x[:, :, :t].contiguous(), cc, cuc, hint[:, :, :t].contiguous(), [v[:, :, :t].contiguous() for v in noises])
        tail = _run(g160_wrapper, x[:, :, t:].contiguous(), cc, cuc, hint[:, :, t:].contiguous(), [v[:, :, t:].contiguous() for v in noises])
    finally:
        g160_wrapper.reserve_windows(0)
        g160_wrapper.reset_caches()
    assert windowed.shape == (1, 4, 2 * t, 16, 24) and bool(torch.isfinite(windowed).all())
    assert np.array_equal(_bits(windowed[:, :, :t]), _bits(head)), _rel(windowed[:, :, :t], head)
    assert np.array_equal(_bits(windowed[:, :, t:]), _bits(tail)), _rel(windowed[:, :, t:], tail)


def test_three_windows_replay_three_graphs_without_host_compares(g160_wrapper):
    """W = 3 (N = 6, T = 3, overlap 1; 3 steps = 5 sampler evaluations = 15 network evaluations): each window's key is evaluated eagerly
    once, captured once and replayed for the rest; the CFG marks reach the network (no device compare: `_twin_val` stays empty); the
    hint stem is computed once per window."""
    w = g160_wrapper
    if not w.use_graph:
        pytest.skip("HIP graphs are switched off by policy")
    from ccedit_amd.windows import plan
    assert plan(6, 3, 1)[0] == [0, 2, 3]
    try:
        out = _run(w, *_clip_inputs(33, 6), window=3, overlap=1)
        counts = dict(w.graph_counts)
        assert counts == dict(eager=3, capture=3, replay=9), counts
        assert not w._twin_val, "the network compared CFG halves on the device: a mark was lost on the way through the windows"
        assert len(w._graphs) == 3 and all(e.captured for e in w._graphs.values())
        assert len(w._hint_val) == 3, "one cached hint-stem output per window"
        assert bool(torch.isfinite(out).all()) and out.shape == (1, 4, 6, 16, 24)
        # the limits of a plain clip come back with reserve_windows(0)
        w.reserve_windows(0)
        assert (w._graph_slots, w._hint_slots, w._graph_pool) == (2, 4, None)
    finally:
        w.reserve_windows(0)
        w.reset_caches()


def test_graphed_windows_equal_eager_windows(g160_wrapper):
    """The W graphs share one memory pool and replay in turn: the clip equals the same clip evaluated eagerly, bit for bit."""
    w = g160_wrapper
    inputs = _clip_inputs(34, 6)
    saved = w.use_graph
    try:
        graphed = _run(w, *inputs, window=3, overlap=1)
        w.use_graph = False
        eager = _run(w, *inputs, window=3, overlap=1)
    finally:
        w.use_graph = saved
        w.reserve_windows(0)
        w.reset_caches()
    assert np.array_equal(_bits(graphed), _bits(eager)), _rel(graphed, eager)


# ---- 3. against the fp32 oracle ------------------------------------------------------------------
def test_windowed_clip_vs_oracle(g160_wrapper):
    """N = 6, T = 3, overlap 1 (starts [0, 2, 3]), 3 steps of DPMPP2SAncestral + VanillaCFGTV2V(7.5) + DiscreteDenoiser with injected
    noise, against the CPU oracle: the windowed closure restated in torch around oracle.discrete_denoise / network_forward, handed to
    oracle.dpmpp2s_ancestral_sample.  Budget: TRAJ_TOL, the plain trajectory's own (5.5-6.0e-2 measured there over 5 steps) — the fusion
    is a convex combination of the windows' outputs and cannot widen the worst window's error."""
    from ccedit_amd.sgm_compat import build_network_spec
    from ccedit_amd.utils.synth import synth_state_dict
    from ccedit_amd.windows import plan
    from oracle import ccedit_oracle as O
    n, t, overlap, steps = 6, 3, 1, 3
    x, cc, cuc, hint, noises = _clip_inputs(35, n, steps)
    try:
        got = _run(g160_wrapper, x, cc, cuc, hint, noises, window=t, overlap=overlap, steps=steps)
    finally:
        g160_wrapper.reserve_windows(0)
        g160_wrapper.reset_caches()

    cfg = O.NetConfig(**G160)
    sd = synth_state_dict(build_network_spec(G160))
    table = O.denoiser_sigmas(1000)
    starts, coef = plan(n, t, overlap)
    assert starts == [0, 2, 3]
    coef_t = torch.from_numpy(coef)

    def network(xx, idx, cond):
        return O.network_forward(sd, cfg, xx, idx, cond)

    def windowed(xx, sigma, cond):
        out = torch.zeros_like(xx)
        for i, s in enumerate(starts):
            ci = dict(cond, control_hint=cond["control_hint"][:, :, s:s + t])
            y = O.discrete_denoise(network, table, xx[:, :, s:s + t], sigma, ci)
            out[:, :, s:s + t] += coef_t[i].view(1, 1, t, 1, 1) * y
        return out

    it = iter(noises)
    with torch.no_grad():
        ref = O.dpmpp2s_ancestral_sample(windowed, x.clone(), dict(crossattn=cc, control_hint=hint), dict(crossattn=cuc, control_hint=hint.clone()),
                                         num_steps=steps, scale=7.5, noise_fn=lambda v: next(it))
    r = _rel(got, ref)
    print(f"windowed clip (N=6, T=3, overlap 1, 3 steps): final latent rel rms err vs fp32 oracle: {r:.4f}")
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
def test_first_stage_in_groups_equals_the_single_call(tmp_path):
    """Encode (given noise, and the default draw from the CPU generator) and decode of 7 frames in groups of 3 (3 + 3 + 1)."""
    _need_gpu()
    from ccedit_amd.windows import GroupedFirstStage
    from scripts.sampling import sampling_tv2v as S
    args = S.parse_args(["--config_path", _write_config(tmp_path), "--synthetic", "--H", "64", "--W", "128"])
    torch.set_grad_enabled(False)
    model, dev = S.build_model(args)
    g = torch.Generator().manual_seed(9)
    frames = (torch.rand(2, 3, 7, 64, 128, generator=g) * 2 - 1).to(dev)
    noise = torch.randn(2 * 7, 4, 8, 16, generator=g)
    grouped = GroupedFirstStage(model, 3)
    assert grouped.scale_factor == model.scale_factor
    z = model.encode_first_stage(frames, noise=noise)
    zg = grouped.encode_first_stage(frames, noise=noise)
    assert z.shape == zg.shape == (2, 4, 7, 8, 16) and np.array_equal(_bits(zg), _bits(z)), _rel(zg, z)
    torch.manual_seed(77)
    z2 = model.encode_first_stage(frames)
    torch.manual_seed(77)
    z2g = grouped.encode_first_stage(frames)
    assert np.array_equal(_bits(z2g), _bits(z2)) and not np.array_equal(_bits(z2), _bits(z))
    d = model.decode_first_stage(z)
    dg = grouped.decode_first_stage(z)
    assert d.shape == dg.shape == (2, 3, 7, 64, 128) and np.array_equal(_bits(dg), _bits(d)), _rel(dg, d)


@pytest.mark.timeout(1500)
def test_entry_point_writes_a_long_clip(tmp_path):
    """scripts/sampling/sampling_tv2v.py --window_frames 3 --num_keyframes 6 on a frame directory of 18 frames (6 keyframes), --synthetic:
    N frames are written; with --inpainting_mode --mask_composite the pixels outside the mask are the input frames exactly, inside
    they are not.  (--save_type npy: the fp32 frames themselves, original/ and result/ through the same clamp.)"""
    _need_gpu()
    from PIL import Image
    cfg = _write_config(tmp_path)
    rs = np.random.RandomState(6)
    vdir = tmp_path / "clips" / "fox"
    vdir.mkdir(parents=True)
    for i in range(18):
        Image.fromarray(rs.randint(0, 256, (90, 150, 3)).astype(np.uint8)).save(str(vdir / f"{i:03d}.png"))
    mask = np.zeros((90, 150), np.uint8)
    mask[:, 75:] = 255                                                            # left half black: keep
    Image.fromarray(mask).save(str(tmp_path / "clips" / "fox.mask.png"))
    keep = np.array(Image.fromarray(mask).resize((128, 64), Image.NEAREST)) == 0
    base = ["--config_path", cfg, "--synthetic", "--H", "64", "--W", "128", "--num_keyframes", "6", "--window_frames", "3",
            "--sample_steps", "2", "--sampler_name", "DPMPP2SAncestralSampler", "--original_fps", "9", "--target_fps", "3", "--noise_seed", "1",
            "--prompt", "a red fox", "--video_path", str(vdir), "--batch_size", "1", "--save_type", "npy"]
    for tag, extra in (("plain", []), ("masked", ["--inpainting_mode", "--mask_composite"])):
        out = str(tmp_path / tag)
        cmd = [sys.executable, os.path.join(ROOT, "scripts", "sampling", "sampling_tv2v.py"), *base, "--save_path", out, *extra]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=450, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        orig = np.load(os.path.join(out, "default", "original", "npy", "frames-0000.npy"))
        res = np.load(os.path.join(out, "default", "result", "npy", "frames-0000.npy"))
        assert orig.shape == res.shape == (6, 64, 128, 3) and np.isfinite(res).all(), (tag, res.shape)
        assert len({res[f].tobytes() for f in range(6)}) == 6, "frames repeat"
        if extra:
            k = np.broadcast_to(keep[None, ..., None], res.shape)
            assert np.array_equal(res[k].view(np.int32), orig[k].view(np.int32)), f"{tag}: {int((res[k] != orig[k]).sum())} kept values differ"
            assert (res[~k] != orig[~k]).mean() > 0.5, f"{tag}: the edited region equals the original"
            assert os.path.isdir(os.path.join(out, "default", "mask"))
