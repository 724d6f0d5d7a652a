"""Edit-mask kernels (csrc/mask.hip) and the `--inpainting_mode` route of the entry points on a real MI355X.  Every reference is the
reference project's own expression evaluated with torch on the CPU at test time (F.interpolate(mode="area") + round + clamp, the
re-injection formula of sampling.py:150-153, torch.where, Pillow's NEAREST) or a fixture recorded from the reference
(tests/golden/samplers_toy.npz) — never the kernels themselves."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from ccedit_amd import hip
    hip.lib()


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float(((a - b) ** 2).mean().sqrt() / (b ** 2).mean().sqrt())


# ---- 4. pixel mask -> latent mask -------------------------------------------------------------
def _area_reference(m_u8):
    """The reference's rule (sampling_tv2v.py:391-394) on the binary mask (B, T, H, W) -> uint8 (B, T, H / 8, W / 8)."""
    m = (m_u8 >= 128).float()[:, None]
    b, _, t, h, w = m.shape
    r = torch.clamp(torch.round(torch.nn.functional.interpolate(m, size=(t, h // 8, w // 8), mode="area")), 0, 1)
    return r[:, 0].to(torch.uint8)


def _latent_cases():
    g = torch.Generator().manual_seed(3)
    rnd = lambda *s: (torch.rand(*s, generator=g) > 0.5).to(torch.uint8) * 255
    yield "random 17x512x768", rnd(1, 17, 512, 768)
    yield "random 3x40x72 (odd cell count)", rnd(2, 3, 40, 72)
    yield "coarse blobs", rnd(1, 5, 8, 12).repeat_interleave(16, 2).repeat_interleave(16, 3)
    counts = torch.zeros(1, 1, 24, 40, dtype=torch.uint8)          # 3 x 5 cells holding exactly 0, 1, 31, 32, 33, 63, 64 ... set pixels
    for i, k in enumerate((0, 1, 31, 32, 33, 63, 64, 32, 31, 33, 32, 16, 48, 32, 33)):
        cell = torch.zeros(64, dtype=torch.uint8)
        cell[torch.randperm(64, generator=g)[:k]] = 255
        counts[0, 0, 8 * (i // 5): 8 * (i // 5) + 8, 8 * (i % 5): 8 * (i % 5) + 8] = cell.view(8, 8)
    yield "31 / 32 / 33 of 64", counts
    yield "all 0", torch.zeros(1, 2, 16, 24, dtype=torch.uint8)
    yield "all 1", torch.full((1, 2, 16, 24), 255, dtype=torch.uint8)
    thr = torch.zeros(1, 1, 8, 24, dtype=torch.uint8)              # three cells of 127s, 128s and 255s: the threshold is >= 128
    thr[..., 0:8], thr[..., 8:16], thr[..., 16:24] = 127, 128, 255
    yield "bytes 127 / 128 / 255", thr
    mixed = torch.randint(0, 256, (1, 3, 64, 80), generator=g).to(torch.uint8)          # any byte value, both load widths (W % 16 == 0)
    yield "grey values", mixed


def test_mask_latent_equals_area_round_clamp():
    _need_gpu()
    from ccedit_amd import ops
    for name, m in _latent_cases():
        want = _area_reference(m)
        got = ops.mask_latent(m.cuda()).cpu()
        assert got.dtype == torch.uint8 and got.shape == want.shape, name
        assert torch.equal(got, want), f"{name}: {int((got != want).sum())} of {want.numel()} cells differ"
    thr = ops.mask_latent(next(m for n, m in _latent_cases() if n.startswith("bytes")).cuda()).cpu()
    assert thr.flatten().tolist() == [0, 1, 1]
    # the rule itself, spelled out: a cell with exactly 32 set pixels is 0 (round half to even), 33 is 1
    name, counts = next((n, m) for n, m in _latent_cases() if n.startswith("31"))
    k = (counts >= 128).view(3, 8, 5, 8).sum(dim=(1, 3))
    assert torch.equal(ops.mask_latent(counts.cuda()).cpu()[0, 0], (k > 32).to(torch.uint8))


@pytest.mark.parametrize("n,hs,ws,h,w", [(3, 40, 56, 64, 96), (2, 270, 480, 128, 192), (2, 37, 53, 61, 53), (1, 6, 9, 9, 6),
                                          (17, 135, 240, 512, 768)])
def test_mask_resize_nearest_equals_pillow(n, hs, ws, h, w):
    _need_gpu()
    from PIL import Image
    from ccedit_amd import ops
    src = np.random.RandomState(ws).randint(0, 256, (n, hs, ws)).astype(np.uint8)
    want = np.stack([np.array(Image.fromarray(f).resize((w, h), Image.NEAREST)) for f in src])
    got = ops.mask_resize_nearest(torch.from_numpy(src).cuda(), (h, w)).cpu().numpy()
    assert np.array_equal(got, want)


def test_load_video_mask_device_route_gives_identical_bytes(tmp_path):
    _need_gpu()
    from PIL import Image
    from scripts.sampling.util import load_video_mask
    rs = np.random.RandomState(2)
    d = tmp_path / "m"
    d.mkdir()
    for i in range(9):
        Image.fromarray(rs.randint(0, 256, (90, 150)).astype(np.uint8)).save(str(d / f"{i:03d}.png"))
    Image.fromarray(rs.randint(0, 256, (48, 64, 3)).astype(np.uint8)).save(str(tmp_path / "one.png"))
    for path, n_all in ((str(d), 9), (str(tmp_path / "one.png"), None)):
        for size in ((64, 128), (90, 150), (512, 768)):
            host = load_video_mask(path, 9, 3, 3, size, n_all)
            dev = load_video_mask(path, 9, 3, 3, size, n_all, device=torch.device("cuda:0"))
            assert dev.is_cuda and dev.dtype == torch.uint8 and torch.equal(dev.cpu(), host), (path, size)


# ---- 5. the re-injection ------------------------------------------------------------------------
def _blend_inputs(shape, seed):
    g = torch.Generator().manual_seed(seed)
    x, x0, n = (torch.randn(shape, generator=g) for _ in range(3))
    flat = [t.view(-1) for t in (x, x0, n)]
    pos = torch.randperm(flat[0].numel(), generator=g)[:24]
    for j, p in enumerate(pos.tolist()):          # a handful of very small and very large NORMAL numbers in every operand
        flat[j % 3][p] = (1e-30 if (j // 3) % 2 == 0 else 1e30) * (-1.0 if j % 5 == 0 else 1.0)
    b, c, t, h, w = shape
    m = (torch.rand(b, t, h, w, generator=g) > 0.5).to(torch.uint8)
    return x, x0, n, m


def _same_bits(a, b):
    """torch.equal on the int32 view, except that +0.0 == -0.0 is accepted."""
    ai, bi = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return bool(((ai == bi) | ((a == 0) & (b == 0))).all())


@pytest.mark.parametrize("shape", [(1, 4, 17, 64, 96), (2, 4, 5, 8, 8), (1, 4, 3, 5, 7)])
def test_inpaint_blend_is_bit_equal_to_the_reference_expression(shape):
    """x * m + ((x0 + n * sigma) / sqrt(1 + sigma^2)) * (1 - m) in torch fp32 on the CPU, binary m, for every sigma of the 30-step
    LegacyDDPMDiscretization schedule.  ((1, 4, 3, 5, 7): T h w not a multiple of 4, the one-element variant of the kernel.)"""
    _need_gpu()
    from ccedit_amd import ops
    from ccedit_amd.sampling import LegacyDDPMDiscretization
    sigmas = LegacyDDPMDiscretization()(30)
    assert len(sigmas) == 31 and float(sigmas[-1]) == 0.0
    x, x0, n, m = _blend_inputs(shape, 17 + shape[2])
    mf = m[:, None].float()
    xd, x0d, nd, md = x.cuda(), x0.cuda(), n.cuda(), m.cuda()
    worst = 0
    for i in range(len(sigmas) - 1):          # the loop re-injects before steps 0 ... 29: sigmas[i] > 0
        sigma = sigmas[i]
        s = torch.sqrt(1 + sigma ** 2)
        want = x * mf + ((x0 + n * sigma) / s) * (1 - mf)
        got = ops.inpaint_blend(xd, x0d, nd, md, float(sigma), float(s)).cpu()
        ulp = (got.view(torch.int32).long() - want.view(torch.int32).long()).abs()
        ulp[(got == 0) & (want == 0)] = 0
        worst = max(worst, int(ulp.max()))
        assert _same_bits(got, want), f"sigma[{i}] = {float(sigma)}: {int((ulp > 0).sum())} elements differ, up to {int(ulp.max())} ulp"
        alias = xd.clone()
        out = ops.inpaint_blend(alias, x0d, nd, md, float(sigma), float(s), out=alias)
        assert out is alias and torch.equal(alias.cpu().view(torch.int32), got.view(torch.int32)), f"sigma[{i}]: y = x aliasing changes the bytes"
    print(f"inpaint_blend {shape}: largest ulp distance to the CPU expression over 30 sigmas: {worst}")


# ---- 6. the put-back ----------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 3, 17, 512, 768), (2, 3, 3, 40, 72), (1, 3, 2, 5, 7)])
def test_mask_composite_equals_where(shape):
    _need_gpu()
    from ccedit_amd import ops
    g = torch.Generator().manual_seed(shape[3])
    res, orig = (torch.rand(shape, generator=g) * 2.4 - 1.2 for _ in range(2))
    b, _, t, h, w = shape
    m = torch.randint(0, 256, (b, t, h, w), generator=g).to(torch.uint8)
    m[..., : w // 2] = torch.where(m[..., : w // 2] >= 128, 255, 0).to(torch.uint8)          # half of it black / white, half any byte
    want = torch.where((m >= 128)[:, None], res, orig)
    got = ops.mask_composite(res.cuda(), orig.cuda(), m.cuda())
    assert torch.equal(got.cpu().view(torch.int32), want.view(torch.int32))
    alias = res.cuda()
    assert ops.mask_composite(alias, orig.cuda(), m.cuda(), out=alias) is alias and torch.equal(alias.cpu().view(torch.int32), want.view(torch.int32))


# ---- 7. the loops -------------------------------------------------------------------------------
def test_inpainting_loops_on_the_fused_path_match_the_reference_goldens(golden_dir):
    """tests/golden/samplers_toy.npz (recorded from the reference's sample_inpainting) replayed with the mask as a uint8 latent mask:
    the fused kernel route must meet the goldens at the tolerance of tests/test_network_gpu.py (1e-4) and agree with the fp32-mask
    route (axpby + mask_blend) to the same bound."""
    _need_gpu()
    from ccedit_amd import ops
    from scripts.sampling.util import get_discretization, get_guider, get_sampler
    z = np.load(os.path.join(golden_dir, "samplers_toy.npz"))
    c = {"crossattn": torch.from_numpy(z["cross_c"]).cuda()}
    uc = {"crossattn": torch.from_numpy(z["cross_uc"]).cuda()}

    def toy_denoiser(x, sigma, cond):
        s = sigma.to(x.device).reshape(-1, *([1] * (x.dim() - 1)))
        return x / (1.0 + s * s) + 0.1 * torch.tanh(cond["crossattn"].mean()) * s / (1.0 + s)

    guider = get_guider("sgm.modules.diffusionmodules.guiders.VanillaCFG", scale=3.0)
    x, x0, mask_f = (torch.from_numpy(z[k]).cuda() for k in ("inp_x", "inp_x0", "inp_mask"))
    assert tuple(mask_f.shape) == (1, 1, 5, 8, 8) and set(mask_f.unique().tolist()) <= {0.0, 1.0}
    mask_u8 = mask_f[:, 0].to(torch.uint8).contiguous()
    noise = torch.from_numpy(z["inp_noise"]).cuda()
    calls = []
    real = ops.inpaint_blend
    ops.inpaint_blend = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        for name in ("EulerEDMSampler", "EulerAncestralSampler", "DPMPP2SAncestralSampler"):
            outs = []
            for m in (mask_u8, mask_f):
                smp = get_sampler(name, 7, get_discretization("LegacyDDPMDiscretization"), guider)
                smp.verbose = False
                it = iter(noise)
                smp.noise_sampler = lambda t: next(it)
                n0 = len(calls)
                outs.append(smp.sample_inpainting(toy_denoiser, x.clone(), c, x0, m, uc))
                assert len(calls) - n0 == (7 if m is mask_u8 else 0), "the uint8 mask must take the fused kernel, the fp32 mask must not"
            r_fused, r_unfused = (_rel(o, torch.from_numpy(z[f"inpaint_{name}"])) for o in outs)
            d = _rel(outs[0], outs[1])
            print(f"inpaint_{name}: fused vs golden {r_fused:.3e}, unfused vs golden {r_unfused:.3e}, fused vs unfused {d:.3e}")
            assert r_fused < 1e-4 and d < 1e-4, (name, r_fused, d)
    finally:
        ops.inpaint_blend = real


# ---- 8. end to end ------------------------------------------------------------------------------
def _write_config(tmp_path):
    import yaml
    from ccedit_amd.sgm_compat import engine_config
    cfg = os.path.join(str(tmp_path), "tv2v.yaml")
    with open(cfg, "w") as f:
        yaml.safe_dump(dict(model=engine_config(crossframe=False, vae_ch=32, model_channels=64, num_heads=2, context_dim=64)), f)
    return cfg


def _gif_frames(path):
    from PIL import Image, ImageSequence
    return np.stack([np.array(fr.convert("RGB")) for fr in ImageSequence.Iterator(Image.open(path))])


@pytest.mark.timeout(1200)
def test_job_with_a_mask_keeps_the_original_outside_it(tmp_path):
    """A frame-directory job with `<video>.mask.png` (left half black), --inpainting_mode --mask_composite --gpu_io --save_type gif
    --noise_seed 1.  (a) outside the mask result/ holds the bytes of original/, (b) inside it differs, (c) mask/ is written, (d) the
    same command without --gpu_io writes byte-identical gif files.
    (a) and (b) are checked on the uint8 frames as they are handed to the gif writer, not on pixels decoded from the files: Pillow's
    gif encoder quantises every frame to an adaptive 256-colour palette of that frame, so equal RGB bytes in original/ and result/ do
    not stay equal inside the files.  The job is therefore run once more in this process with the writer's input recorded; that this
    run IS the one that wrote the files is itself asserted (its gif files are byte-identical to the subprocess's)."""
    _need_gpu()
    from PIL import Image
    cfg = _write_config(tmp_path)
    rs = np.random.RandomState(4)
    vdir = tmp_path / "clips" / "fox"
    vdir.mkdir(parents=True)
    for i in range(9):
        Image.fromarray(rs.randint(0, 256, (90, 150, 3)).astype(np.uint8)).save(str(vdir / f"{i:03d}.png"))
    mask = np.zeros((90, 150), np.uint8)
    mask[:, 75:] = 255                                                            # left half black: keep
    Image.fromarray(mask).save(str(tmp_path / "clips" / "fox.mask.png"))
    base = ["--config_path", cfg, "--synthetic", "--H", "64", "--W", "128", "--num_keyframes", "3", "--sample_steps", "2",
            "--sampler_name", "DPMPP2SAncestralSampler", "--original_fps", "9", "--target_fps", "3", "--noise_seed", "1",
            "--prompt", "a red fox", "--video_path", str(vdir), "--batch_size", "1", "--save_type", "gif",
            "--inpainting_mode", "--mask_composite"]
    outs = []
    for tag, extra in (("gpu", ["--gpu_io"]), ("host", [])):
        out = str(tmp_path / tag)
        cmd = [sys.executable, os.path.join(ROOT, "scripts", "sampling", "sampling_tv2v.py"), *base, "--save_path", out, *extra]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=500, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        outs.append(os.path.join(out, "default"))
    # (c) + (d)
    for kind in ("original", "result", "control_hint", "mask"):
        names = sorted(os.listdir(os.path.join(outs[0], kind, "gif")))
        assert names == sorted(os.listdir(os.path.join(outs[1], kind, "gif"))) == ["animation-0000.gif"], kind
        a, b = (open(os.path.join(o, kind, "gif", names[0]), "rb").read() for o in outs)
        assert a == b, f"{kind}/{names[0]} differs between --gpu_io and the host route"
    m = _gif_frames(os.path.join(outs[0], "mask", "gif", "animation-0000.gif"))          # two colours: the gif holds them exactly
    assert m.shape[1:] == (64, 128, 3) and set(np.unique(m)) == {0, 255}                 # (the writer merges identical frames: 1 ... 3 of them)
    keep = m[0, ..., 0] == 0
    assert all(np.array_equal(f[..., 0] == 0, keep) for f in m)
    want_keep = np.array(Image.fromarray(mask).resize((128, 64), Image.NEAREST)) == 0
    assert np.array_equal(keep, want_keep) and keep[:, :64].all() and not keep[:, 64:].any()
    # (a) + (b): the frames handed to the gif writer, reproduced in this process by the same functions from the same inputs
    got = _run_job_in_process(base + ["--gpu_io", "--save_path", str(tmp_path / "inproc")])
    for kind in ("original", "result"):          # ... which are the frames of the files: re-encoding them gives the subprocess's bytes
        assert got[kind + "_gif"] == open(os.path.join(outs[0], kind, "gif", "animation-0000.gif"), "rb").read(), kind
    orig, res = got["original"], got["result"]
    assert orig.shape == res.shape == (1, 3, 64, 128, 3) and orig.dtype == res.dtype == np.uint8
    k = np.broadcast_to(keep[None, None, ..., None], res.shape)
    assert np.array_equal(res[k], orig[k]), f"{int((res[k] != orig[k]).sum())} kept bytes differ from the original"
    assert (res[~k] != orig[~k]).mean() > 0.5, "the edited region equals the original"


def _run_job_in_process(argv):
    """The job through scripts.sampling.sampling_tv2v.run_jobs in this process, recording the uint8 frames perform_save_locally_video
    hands to the gif writer (Image.fromarray is what it calls on each of them) -> {kind: (B, T, H, W, 3) uint8, kind_gif: file bytes}."""
    import PIL.Image
    from scripts.sampling import sampling_tv2v as S
    from scripts.sampling import util as U
    args = S.parse_args(argv)
    torch.manual_seed(args.seed)
    rec, real_save, real_from = {}, U.perform_save_locally_video, PIL.Image.fromarray
    state = {"kind": None}

    def fromarray(a, *aa, **kk):
        if state["kind"] is not None:
            rec.setdefault(state["kind"], []).append(np.array(a))
        return real_from(a, *aa, **kk)

    def save(save_path, samples, *a, **k):
        state["kind"] = os.path.basename(save_path)
        try:
            return real_save(save_path, samples, *a, **k)
        finally:
            state["kind"] = None
    U.perform_save_locally_video, PIL.Image.fromarray = save, fromarray
    try:
        with torch.no_grad():
            S.run_jobs(args)
    finally:
        U.perform_save_locally_video, PIL.Image.fromarray = real_save, real_from
    out = {}
    for kind, frames in rec.items():
        out[kind] = np.stack(frames)[None]
        out[kind + "_gif"] = open(os.path.join(args.save_path, "default", kind, "gif", "animation-0000.gif"), "rb").read()
    return out


@pytest.mark.timeout(900)
def test_masked_branch_of_the_script_is_the_samplers_own_loop(tmp_path):
    """sample_latent's masked branch with an all-ones latent mask against sampler.sample_inpainting called directly with the same
    seeded noise_sampler, start, conditioning and known latent: the script adds nothing of its own to the reference's loop.  Both
    --sdedit_denoise_strength branches.  (Not compared with the unmasked run: the masked loop draws one more noise tensor per step.)"""
    _need_gpu()
    from scripts.sampling import sampling_tv2v as S
    from scripts.sampling.util import init_sampling, sdedit_start
    cfg = _write_config(tmp_path)
    for extra in ([], ["--sdedit_denoise_strength", "0.7"]):
        args = S.parse_args(["--config_path", cfg, "--synthetic", "--H", "64", "--W", "128", "--num_keyframes", "3", "--sample_steps", "3",
                             "--sampler_name", "DPMPP2SAncestralSampler", "--noise_seed", "11", "--inpainting_mode", *extra])
        torch.manual_seed(args.seed)
        torch.set_grad_enabled(False)
        model, dev = S.build_model(args)
        g = torch.Generator().manual_seed(args.seed)
        cond = S.conditioning_tensors(args, g, True)
        hint = cond["control_hint"].to(dev)
        txt, txt_uc = S.text_inputs(cond, dev, args)
        c, uc = model.conditioner.get_unconditional_conditioning({"txt": txt, "control_hint": hint}, batch_uc={"txt": txt_uc, "control_hint": hint.clone()})
        keyframes = cond["keyframes"].to(dev)
        randn = torch.randn(1, 4, 3, 8, 16, generator=g).to(dev)
        ones = torch.ones(1, 3, 8, 16, dtype=torch.uint8, device=dev)
        torch.manual_seed(123)
        got = S.sample_latent(args, model, dev, c, uc, randn.clone(), keyframes=keyframes, mask=ones)

        torch.manual_seed(123)          # the same draws of the posterior sample / the SDEdit start, in the script's order
        strength = args.sdedit_denoise_strength
        sampler = init_sampling(sample_steps=3, sampler_name=args.sampler_name, discretization_name=args.discretization_name,
                                guider_config_target=S.GUIDER, cfg_scale=args.cfg_scale, **({"img2img_strength": strength} if strength else {}))
        gen = torch.Generator().manual_seed(11)
        sampler.noise_sampler = lambda v: torch.randn(v.shape, generator=gen).to(v.device)
        start = sdedit_start(model, sampler, keyframes) if strength else randn.clone()
        z = model.encode_first_stage(keyframes)
        want = sampler.sample_inpainting(lambda inp, sigma, cc: model.denoiser(model.model, inp, sigma, cc), start, c, uc=uc, x0=z, mask=ones)
        r = _rel(got, want)
        print(f"sample_latent (masked, {extra or 'no sdedit'}) vs sample_inpainting called directly: rel rms {r:.3e}")
        assert got.shape == want.shape == (1, 4, 3, 8, 16) and bool(torch.isfinite(got).all())
        assert torch.equal(got, want), r
