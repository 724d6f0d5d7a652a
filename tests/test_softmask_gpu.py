"""Graded edit masks on a real MI355X (csrc/softmask.hip, the level launcher of csrc/mask.hip, the samplers' strength= route and the
`--mask_graded` / `--mask_feather` route of the entry point).  Exact, no tolerance anywhere: every kernel against the numpy
restatement (tests/_softmask_numpy.py), the sampler walk against a loop of the existing binary re-injection, the graded route on
binary masks against the binary route."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _softmask_numpy as ref  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from ccedit_amd import hip
    hip.lib()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ---- 1. feather -------------------------------------------------------------------------------
def _feather_maps(shape, seed):
    rs = np.random.RandomState(seed)
    yield "random bytes", rs.randint(0, 256, shape).astype(np.uint8)
    yield "0 / 255", (rs.rand(*shape) > 0.5).astype(np.uint8) * 255
    blob = np.zeros(shape, np.uint8)
    blob[..., shape[-2] // 4: shape[-2] // 2 + 3, 1: shape[-1] // 2] = 255
    yield "a box at the border", blob
    yield "all 255", np.full(shape, 255, np.uint8)


@pytest.mark.parametrize("shape,radii", [((2, 24, 40), (1, 3, 64)), ((1, 8, 12), (1, 3, 64)), ((3, 40, 72), (2, 17))],
                         ids=["2x24x40", "1x8x12 (4-byte variant)", "3x40x72"])
def test_mask_feather_equals_numpy(shape, radii):
    _need_gpu()
    from ccedit_amd import ops
    for name, m in _feather_maps(shape, shape[-1]):
        d = torch.from_numpy(m).cuda()
        for r in radii:
            got = ops.mask_feather(d, r).cpu().numpy()
            want = ref.feather(m, r)
            assert got.dtype == np.uint8 and np.array_equal(got, want), f"{name}, R={r}: {int((got != want).sum())} of {want.size} bytes differ"
        assert np.array_equal(d.cpu().numpy(), m), "the source was written"
    four = torch.from_numpy(next(_feather_maps((1, 2) + shape, 9))[1]).cuda()          # (B, T, H, W): per frame
    assert np.array_equal(ops.mask_feather(four, 3).cpu().numpy(), ref.feather(four.cpu().numpy(), 3))


# ---- 2. latent strengths ------------------------------------------------------------------------
def _boundary_cells():
    """3 x 6 cells whose byte sums are 64 g + d for d in -33, -32, -31, 31, 32, 33 around several g (the rounding boundary lies between
    64 g + 31 -> g and 64 g + 32 -> g + 1), the bytes spread over the cell at random."""
    rs = np.random.RandomState(11)
    sums = [64 * g + d for g in (1, 100, 254) for d in (-33, -32, -31, 31, 32, 33)]
    m = np.zeros((1, 1, 24, 48), np.uint8)
    for i, s in enumerate(sums):
        cell = np.full(64, s // 64, np.int64)
        cell[rs.permutation(64)[: s % 64]] += 1
        assert cell.sum() == s and cell.max() <= 255
        m[0, 0, 8 * (i // 6): 8 * (i // 6) + 8, 8 * (i % 6): 8 * (i % 6) + 8] = rs.permutation(cell).reshape(8, 8)
    return m, np.array(sums).reshape(3, 6)


def test_mask_latent_graded_equals_numpy():
    _need_gpu()
    from ccedit_amd import ops
    rs = np.random.RandomState(2)
    cases = {"random 2x3x40x72 (odd cell count: the one-cell variant)": rs.randint(0, 256, (2, 3, 40, 72)).astype(np.uint8),
             "random 1x3x64x80 (W % 16 == 0)": rs.randint(0, 256, (1, 3, 64, 80)).astype(np.uint8),
             "all 255": np.full((1, 2, 16, 32), 255, np.uint8), "all 0": np.zeros((1, 2, 16, 24), np.uint8)}
    for name, m in cases.items():
        got = ops.mask_latent_graded(torch.from_numpy(m).cuda()).cpu().numpy()
        assert got.dtype == np.uint8 and np.array_equal(got, ref.latent_strength(m)), name
    m, sums = _boundary_cells()
    want = (sums + 32) >> 6
    assert want.tolist()[0] == [0, 1, 1, 1, 2, 2] and want[2, 3:].tolist() == [254, 255, 255]
    for variant in (m, np.concatenate([m, m[..., :8]], axis=-1)):                        # 6 cells a row: the pair variant; 7: the one-cell variant
        got = ops.mask_latent_graded(torch.from_numpy(np.ascontiguousarray(variant)).cuda()).cpu().numpy()
        assert np.array_equal(got[0, 0, :, :6], want) and np.array_equal(got, ref.latent_strength(variant))
    cells = (rs.rand(1, 2, 4, 6) > 0.5)
    binary = np.ascontiguousarray((cells.repeat(8, axis=2).repeat(8, axis=3) * 255).astype(np.uint8))
    d = torch.from_numpy(binary).cuda()
    assert torch.equal(ops.mask_latent_graded(d), ops.mask_latent(d) * 255)              # cell-aligned 0 / 255: 255 x the binary route


# ---- 3. the level re-injection --------------------------------------------------------------------
def _blend_inputs(shape, seed):
    """tests/test_mask_gpu.py's operands: normal deviates with a handful of +-1e-30 and +-1e30 entries in every operand."""
    g = torch.Generator().manual_seed(seed)
    x, x0, n = (torch.randn(shape, generator=g) for _ in range(3))
    flat = [t.view(-1) for t in (x, x0, n)]
    pos = torch.randperm(flat[0].numel(), generator=g)[:24]
    for j, p in enumerate(pos.tolist()):
        flat[j % 3][p] = (1e-30 if (j // 3) % 2 == 0 else 1e30) * (-1.0 if j % 5 == 0 else 1.0)
    return x, x0, n, g


@pytest.mark.parametrize("shape", [(2, 4, 5, 8, 8), (1, 4, 3, 5, 7)], ids=["16-byte variant", "odd P: one-element variant"])
def test_inpaint_blend_level_equals_numpy_and_the_binary_route(shape):
    _need_gpu()
    from ccedit_amd import ops
    x, x0, n, g = _blend_inputs(shape, 5 + shape[2])
    b, _, t, h, w = shape
    xd, x0d, nd = x.cuda(), x0.cuda(), n.cuda()
    sigma = torch.tensor(3.0369)
    s = torch.sqrt(1 + sigma ** 2)
    for thr in (1, 2, 128, 254, 255):
        L = torch.randint(0, 256, (b, t, h, w), generator=g).to(torch.uint8)
        L.view(-1)[:8] = torch.tensor([0, thr - 1, thr, 255, thr, thr - 1, 255, 0], dtype=torch.uint8)
        Ld = L.cuda()
        want = torch.from_numpy(ref.blend_level(x.numpy(), x0.numpy(), n.numpy(), L.numpy(), thr, float(sigma), float(s)))
        got = ops.inpaint_blend_level(xd, x0d, nd, Ld, thr, float(sigma), float(s))
        assert torch.equal(_bits(got), _bits(want)), f"thr={thr}: {int((_bits(got) != _bits(want)).sum())} elements differ from numpy"
        binary = ops.inpaint_blend(xd, x0d, nd, (Ld >= thr).to(torch.uint8), float(sigma), float(s))
        assert torch.equal(_bits(got), _bits(binary)), f"thr={thr}: differs from inpaint_blend with the mask (strength >= thr)"
        alias = xd.clone()
        out = ops.inpaint_blend_level(alias, x0d, nd, Ld, thr, float(sigma), float(s), out=alias)
        assert out is alias and torch.equal(_bits(alias), _bits(got)), f"thr={thr}: y = x aliasing changes the bytes"
    for bad in (0, 256):
        with pytest.raises(ValueError, match=r"1 \.\.\. 255"):
            ops.inpaint_blend_level(xd, x0d, nd, Ld, bad, 1.0, 1.5)


# ---- 4. the graded composite ----------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 3, 2, 16, 24), (1, 3, 1, 5, 7)], ids=["16-byte variant", "odd P: one-element variant"])
def test_mask_composite_graded_equals_numpy_and_the_binary_route(shape):
    _need_gpu()
    from ccedit_amd import ops
    g = torch.Generator().manual_seed(shape[3])
    res, orig = (torch.rand(shape, generator=g) * 2.4 - 1.2 for _ in range(2))
    b, _, t, h, w = shape
    m = torch.randint(0, 256, (b, t, h, w), generator=g).to(torch.uint8)
    m.view(-1)[:12] = torch.tensor([0, 1, 127, 128, 254, 255, 255, 255, 255, 255, 0, 0], dtype=torch.uint8)
    m.view(-1)[12:20] = torch.tensor([0, 0, 0, 0, 255, 255, 255, 255], dtype=torch.uint8)          # whole words of 0 and of 255
    want = torch.from_numpy(ref.composite_graded(res.numpy(), orig.numpy(), m.numpy()))
    got = ops.mask_composite_graded(res.cuda(), orig.cuda(), m.cuda())
    assert torch.equal(_bits(got), _bits(want)), f"{int((_bits(got) != _bits(want)).sum())} of {want.numel()} elements differ from numpy"
    alias = res.cuda()
    assert ops.mask_composite_graded(alias, orig.cuda(), m.cuda(), out=alias) is alias and torch.equal(_bits(alias), _bits(want))
    hard = torch.where(m >= 128, 255, 0).to(torch.uint8).cuda()
    assert torch.equal(_bits(ops.mask_composite_graded(res.cuda(), orig.cuda(), hard)), _bits(ops.mask_composite(res.cuda(), orig.cuda(), hard)))


# ---- 5. the sampler walk --------------------------------------------------------------------------
def _stub(x, sigma, cond):
    """A fixed device function of (x, sigma) in place of the network."""
    s = sigma.to(x.device).reshape(-1, *([1] * (x.dim() - 1)))
    return x / (1.0 + s * s) + 0.05 * torch.sin(3.0 * x) * s / (1.0 + s)


def _sampler(name, seed):
    from ccedit_amd import sampling
    kw = dict(s_churn=0.8) if name == "EulerEDMSampler" else {}          # (churn: the EDM step draws noise of its own, after the re-injection's)
    smp = getattr(sampling, name)(discretization_config={"target": "ccedit_amd.sampling.LegacyDDPMDiscretization"}, num_steps=6, **kw)
    gen = torch.Generator().manual_seed(seed)
    smp.noise_sampler = lambda v: torch.randn(v.shape, generator=gen).to(v.device)
    return smp


def _loop(smp, x, x0, strength, start):
    """The walk restated with the EXISTING binary re-injection: before walked step j the mask is (strength >= thr(j, n))."""
    from ccedit_amd import ops
    x, s_in, sigmas, num_sigmas, cond, uc = smp.prepare_sampling_loop(x, {}, None, None)
    n = num_sigmas - 1 - start
    for i in range(start, num_sigmas - 1):
        m = (strength >= ref.threshold(i - start, n)).to(torch.uint8)
        noise = smp.noise_sampler(x0).float().contiguous()
        x = ops.inpaint_blend(x, x0, noise, m, float(sigmas[i]), float(torch.sqrt(1.0 + sigmas[i] ** 2)))
        extra = smp._churn(i, sigmas, num_sigmas) if hasattr(smp, "_churn") else {}
        x = smp.sampler_step(s_in * sigmas[i], s_in * sigmas[i + 1], _stub, x, cond, uc, **extra)
    return x


@pytest.mark.parametrize("name", ["DPMPP2SAncestralSampler", "EulerEDMSampler"])
def test_sample_inpainting_with_strengths_is_the_binary_loop_with_a_threshold_per_step(name):
    _need_gpu()
    g = torch.Generator().manual_seed(8)
    shape = (1, 4, 3, 8, 8)
    x, x0 = torch.randn(shape, generator=g).cuda(), torch.randn(shape, generator=g).cuda()
    levels = torch.tensor([0, 64, 128, 200, 255], dtype=torch.uint8)
    strength = levels[torch.randint(0, 5, (1, 3, 8, 8), generator=g)].cuda()
    assert set(strength.unique().tolist()) == {0, 64, 128, 200, 255}
    for denoise_steps, start in ((None, 0), (4, 2)):                      # the whole schedule; an SDEdit start that skips the first two steps
        kw = {} if denoise_steps is None else dict(denoise_steps=denoise_steps)
        got = _sampler(name, 21).sample_inpainting(_stub, x.clone(), {}, x0, strength=strength, **kw)
        want = _loop(_sampler(name, 21), x.clone(), x0, strength, start)
        assert bool(torch.isfinite(got).all()) and torch.equal(_bits(got), _bits(want)), (name, denoise_steps)
        for value in (255, 0):                                            # all 255: mask = ones; all 0: mask = zeros
            flat = torch.full((1, 3, 8, 8), value, dtype=torch.uint8).cuda()
            a = _sampler(name, 22).sample_inpainting(_stub, x.clone(), {}, x0, strength=flat, **kw)
            b = _sampler(name, 22).sample_inpainting(_stub, x.clone(), {}, x0, mask=(flat // 255), **kw)
            assert torch.equal(_bits(a), _bits(b)), (name, denoise_steps, value)
    assert not torch.equal(_bits(got), _bits(b))                          # (the strengths do something)


# ---- 6. the entry point ---------------------------------------------------------------------------
def _write_config(tmp_path):
    import yaml
    from ccedit_amd.sgm_compat import engine_config
    cfg = os.path.join(str(tmp_path), "tv2v.yaml")
    with open(cfg, "w") as f:
        yaml.safe_dump(dict(model=engine_config(crossframe=False, vae_ch=32, model_channels=64, num_heads=2, context_dim=64)), f)
    return cfg


def _clip(tmp_path, mask):
    from PIL import Image
    rs = np.random.RandomState(4)
    vdir = tmp_path / "clips" / "fox"
    vdir.mkdir(parents=True)
    for i in range(9):
        Image.fromarray(rs.randint(0, 256, (90, 150, 3)).astype(np.uint8)).save(str(vdir / f"{i:03d}.png"))
    Image.fromarray(mask).save(str(tmp_path / "one.png"))
    return str(vdir), str(tmp_path / "one.png")


def _job(argv):
    """One job through run_jobs in this process -> <save_path>/default."""
    from scripts.sampling import sampling_tv2v as S
    args = S.parse_args(argv)
    torch.manual_seed(args.seed)
    with torch.no_grad():
        S.run_jobs(args)
    return os.path.join(args.save_path, "default")


def _png_frames(out, kind):
    """The frames of <out>/<kind>/png/animation-0000.png (lossless: the bytes handed to the writer) -> (frames, H, W, 3) uint8, file bytes."""
    from PIL import Image, ImageSequence
    path = os.path.join(out, kind, "png", "animation-0000.png")
    assert sorted(os.listdir(os.path.dirname(path))) == ["animation-0000.png"], kind
    return np.stack([np.array(fr.convert("RGB")) for fr in ImageSequence.Iterator(Image.open(path))]), open(path, "rb").read()


def _base(tmp_path, vdir, mpath):
    return ["--config_path", _write_config(tmp_path), "--synthetic", "--H", "64", "--W", "128", "--num_keyframes", "3", "--sample_steps", "2",
            "--sampler_name", "DPMPP2SAncestralSampler", "--original_fps", "9", "--target_fps", "3", "--noise_seed", "1", "--prompt", "a red fox",
            "--video_path", vdir, "--batch_size", "1", "--save_type", "png", "--inpainting_mode", "--mask_path", mpath, "--mask_composite"]


@pytest.mark.timeout(600)
def test_feathered_job_writes_the_strength_map_and_keeps_the_original_at_strength_0(tmp_path):
    _need_gpu()
    import json
    from PIL import Image
    mask = np.zeros((90, 150), np.uint8)
    mask[:, 75:] = 255                                                    # left half black: keep
    vdir, mpath = _clip(tmp_path, mask)
    base = _base(tmp_path, vdir, mpath) + ["--mask_feather", "8"]
    out = _job(base + ["--save_path", str(tmp_path / "plain")])
    want = ref.feather(np.array(Image.fromarray(mask).resize((128, 64), Image.NEAREST)), 8)
    assert set(np.unique(want)) > {0, 255} and (want[:, :56] == 0).all() and (want[:, 72:] == 255).all()
    m, _ = _png_frames(out, "mask")
    assert m.shape[1:] == (64, 128, 3) and all(np.array_equal(f[..., c], want) for f in m for c in range(3)), "mask/ is not the feathered mask"
    orig, _ = _png_frames(out, "original")
    res, _ = _png_frames(out, "result")
    assert orig.shape == res.shape == (3, 64, 128, 3)
    keep = np.broadcast_to((want == 0)[None, ..., None], res.shape)
    assert np.array_equal(res[keep], orig[keep]), f"{int((res[keep] != orig[keep]).sum())} bytes of strength 0 differ from the original"
    free = np.broadcast_to((want == 255)[None, ..., None], res.shape)
    assert (res[free] != orig[free]).mean() > 0.5, "the edited region equals the original"
    log = json.load(open(os.path.join(out, "log_info.json")))
    assert log["mask_graded"] is False and log["mask_feather"] == 8
    # composes with windows: fewer frames per evaluation than keyframes
    out_w = _job(base + ["--window_frames", "2", "--window_overlap", "1", "--save_path", str(tmp_path / "windows")])
    res_w, _ = _png_frames(out_w, "result")
    assert res_w.shape == res.shape and np.array_equal(res_w[keep], orig[keep])
    assert np.array_equal(_png_frames(out_w, "mask")[0], m)


@pytest.mark.timeout(600)
def test_graded_route_on_a_cell_aligned_binary_mask_writes_the_binary_routes_files(tmp_path):
    _need_gpu()
    import json
    mask = np.zeros((64, 128), np.uint8)
    mask[16:48, 64:] = 255                                                # edges on the 8-pixel cell grid
    vdir, mpath = _clip(tmp_path, mask)
    base = _base(tmp_path, vdir, mpath)
    binary = _job(base + ["--save_path", str(tmp_path / "binary")])
    graded = _job(base + ["--mask_graded", "--save_path", str(tmp_path / "graded")])
    for kind in ("original", "result", "control_hint", "mask"):
        assert _png_frames(binary, kind)[1] == _png_frames(graded, kind)[1], f"{kind}/ differs between the binary and the graded route"
    log_b, log_g = (json.load(open(os.path.join(o, "log_info.json"))) for o in (binary, graded))
    assert "mask_graded" not in log_b and "mask_feather" not in log_b                    # without the flags: the log as before
    assert log_g["mask_graded"] is True and log_g["mask_feather"] == 0
