"""Pixel I/O kernels (csrc/pixel.hip) on a real MI355X, each against what the reference calls — Pillow, F.interpolate, torch.kthvalue,
the depth encoders' own `normalize`, the numpy expressions of perform_save_locally_video — evaluated on the CPU at test time."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from ccedit_amd import hip
    hip.lib()
    return torch.device("cuda:0")


def _frames(n=23, h=40, w=56):           # == tests/test_video_io.py::_frames
    rs = np.random.RandomState(5)
    yy, xx = np.mgrid[0:h, 0:w]
    return [np.stack([(xx * 4 + 7 * i) % 256, (yy * 5 + 3 * i) % 256, rs.randint(0, 256, (h, w))], -1).astype(np.uint8)
            for i in range(n)]


def _pil(frames, h, w):
    from PIL import Image
    return np.stack([np.array(Image.fromarray(f).resize((w, h), Image.BICUBIC)) for f in frames])


def _as_float(u8):          # load_img's arithmetic: (N, H, W, 3) uint8 -> (N, 3, H, W) fp32
    t = torch.from_numpy(u8).permute(0, 3, 1, 2).float() / 255.0
    return torch.clamp(t * 2.0 - 1.0, -1.0, 1.0)


@pytest.mark.parametrize("n,hs,ws,h,w", [(3, 270, 480, 128, 192),      # shrink
                                          (2, 64, 96, 128, 192),       # enlargement
                                          (2, 40, 56, 40, 32),         # height unchanged
                                          (2, 37, 53, 61, 53),         # width unchanged (no horizontal pass), W odd
                                          (3, 101, 67, 33, 97),        # nothing a multiple of anything
                                          (1, 33, 47, 50, 70)])        # W even, not a multiple of 4
def test_resize_u8_pil_equals_pillow(dev, n, hs, ws, h, w):
    from ccedit_amd import ops
    src = np.random.RandomState(ws).randint(0, 256, (n, hs, ws, 3)).astype(np.uint8)
    src[:, : hs // 3, : ws // 2] = np.where(src[:, : hs // 3, : ws // 2] > 127, 255, 0)
    want = _pil(src, h, w)
    x = torch.from_numpy(src).to(dev)
    assert np.array_equal(ops.resize_u8_pil(x, (h, w)).cpu().numpy(), want)
    got = ops.resize_u8_pil(x, (h, w), to_float=True).cpu()                      # (3, N, H, W)
    assert torch.equal(got.permute(1, 0, 2, 3), _as_float(want))


def test_resize_u8_pil_production_shape(dev):
    """17 keyframes 1080 x 1920 -> 512 x 768 in one launch per pass."""
    from ccedit_amd import ops
    rs = np.random.RandomState(11)
    small = rs.randint(0, 256, (17, 135, 240, 3)).astype(np.uint8)
    src = np.ascontiguousarray(np.repeat(np.repeat(small, 8, axis=1), 8, axis=2))          # blocky: hard edges everywhere
    src[:, ::7, ::5] = rs.randint(0, 256, src[:, ::7, ::5].shape).astype(np.uint8)
    want = _pil(src, 512, 768)
    x = torch.from_numpy(src).to(dev)
    assert np.array_equal(ops.resize_u8_pil(x, (512, 768)).cpu().numpy(), want)
    assert torch.equal(ops.resize_u8_pil(x, (512, 768), to_float=True).cpu().permute(1, 0, 2, 3), _as_float(want))


def test_loaders_on_device_equal_the_reference_goldens(dev, golden_dir, tmp_path):
    from PIL import Image
    from scripts.sampling.util import load_img, load_video_keyframes
    z = np.load(os.path.join(golden_dir, "video_io.npz"))
    for i, fr in enumerate(_frames()):
        Image.fromarray(fr).save(os.path.join(tmp_path, f"frame_{i:04d}.png"))
    d = str(tmp_path)
    got = load_video_keyframes(d, 20, 3, 5, size=(32, 48), device=dev)
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), z["dir_20_3_5_resized"])
    assert np.array_equal(load_video_keyframes(d, 20, 10, 9, device=dev).cpu().numpy(), z["dir_20_10_9"])          # no resize: scale only
    assert np.array_equal(load_img(os.path.join(d, "frame_0003.png"), (24, 40), device=dev).cpu().numpy(), z["img_resized"])
    assert torch.equal(load_img(os.path.join(d, "frame_0003.png"), device=dev).cpu(), load_img(os.path.join(d, "frame_0003.png")))


@pytest.mark.parametrize("shape,size", [((17, 3, 40, 56), (64, 96)), ((5, 1, 135, 240), (64, 96)), ((2, 3, 37, 53), (61, 53)),
                                        ((17, 1, 384, 512), (512, 768)), ((3, 3, 20, 30), (31, 45))])
def test_resize_bicubic_vs_interpolate(dev, shape, size):
    """Bound 1e-5 absolute on inputs in [-1, 1]: 16 products, sum |w| <= 1.6 per axis, fp32 rounding 2^-24 per operation gives
    < 3e-6; the rest is margin for a different contraction of multiply-adds on the two sides."""
    from ccedit_amd import ops
    x = torch.rand(*shape, generator=torch.Generator().manual_seed(shape[2])) * 2 - 1
    want = torch.nn.functional.interpolate(x, size=size, mode="bicubic", align_corners=False)
    got = ops.resize_bicubic(x.to(dev), size).cpu()
    err = (got - want).abs().max().item()
    print(f"resize_bicubic {shape} -> {size}: max abs err {err:.3e}")
    assert got.shape == want.shape and err <= 1e-5


def _kth_case(dev, x, ranks):
    from ccedit_amd import ops
    got = ops.kth_values(x.to(dev), ranks).cpu()
    want = torch.stack([torch.kthvalue(x, k, dim=1).values for k in ranks], dim=1)
    assert torch.equal(got, want), (got, want)
    mm = ops.minmax(x.to(dev)).cpu()
    assert torch.equal(mm[:, 0], x.min(dim=1).values) and torch.equal(mm[:, 1], x.max(dim=1).values)


def test_kth_values_and_minmax_are_exact(dev):
    g = torch.Generator().manual_seed(4)
    n = 17 * 512 * 768
    x = torch.randn(2, n, generator=g) * 3.0 + 1.0                    # negative values, two rows with different contents
    x[1] = torch.rand(n, generator=g) * 80.0 - 20.0
    _kth_case(dev, x, [int(0.02 * n), int(0.85 * n)])
    _kth_case(dev, x, [1, n, n // 2, 12345])                          # ranks 1 and n, four ranks in one call
    q = (torch.round(x[:, : n // 8] * 4.0).clamp(-32, 31) / 4.0).contiguous()          # heavy ties: 64 levels
    assert q.unique().numel() <= 64
    _kth_case(dev, q, [1, int(0.02 * q.shape[1]), int(0.85 * q.shape[1]), q.shape[1]])
    odd = x[:, :1000003].contiguous()                                 # n not a multiple of the block or of 4
    _kth_case(dev, odd, [int(0.02 * 1000003), int(0.85 * 1000003)])
    _kth_case(dev, odd[:1, :777].contiguous(), [1, 777])
    _kth_case(dev, torch.full((1, 4096), -2.5), [1, 2048, 4096])      # one value only


@pytest.mark.parametrize("shape", [(2, 1, 3, 8, 12), (2, 1, 17, 64, 96), (1, 1, 3, 7, 9)])
def test_depth_hint_vs_encoders(dev, shape):
    """Both forms against the encoders' own `normalize` on the CPU: within 2^-22 (two roundings at magnitude <= 1); the measured
    difference is printed — 0 means bit-equal (measured: bit-equal, both forms, all three shapes)."""
    from sgm.modules.encoders.modules import DepthMidasEncoder, DepthZoeEncoder
    raw = torch.rand(*shape, generator=torch.Generator().manual_seed(1)) * 7 + 1
    raw[0, 0, 0, 0, 0], raw[-1, 0, -1, -1, -1] = 0.25, 9.5
    for cls in (DepthMidasEncoder, DepthZoeEncoder):
        want = cls.normalize(raw)
        got = cls.normalize_gpu(raw.to(dev)).cpu()
        err = (got - want).abs().max().item()
        print(f"{cls.__name__} {shape}: max abs diff {err:.3e}, bit-equal {torch.equal(got, want)}")
        assert got.shape == want.shape == (shape[0], 3) + shape[2:] and err <= 2.0 ** -22
        assert torch.equal(got[:, 0], got[:, 1]) and torch.equal(got[:, 1], got[:, 2])


def test_depth_hint_constant_depth_is_nan_like_the_reference(dev):
    from sgm.modules.encoders.modules import DepthMidasEncoder
    raw = torch.full((1, 1, 2, 4, 4), 3.0)
    assert torch.isnan(DepthMidasEncoder.normalize(raw)).all()
    assert torch.isnan(DepthMidasEncoder.normalize_gpu(raw.to(dev)).cpu()).all()


@pytest.mark.parametrize("shape", [(2, 3, 3, 16, 24), (1, 3, 2, 7, 9), (1, 3, 17, 64, 96)])
def test_frames_to_u8_equals_numpy(dev, shape):
    from ccedit_amd import ops
    g = torch.Generator().manual_seed(2)
    x = torch.rand(*shape, generator=g) * 2.4 - 1.2                                  # beyond +-1 on both sides
    flat = x.view(-1)
    grid = torch.arange(256, dtype=torch.float32) / 255.0 * 2.0 - 1.0               # the k / 255 grid points
    special = torch.cat([torch.tensor([-1.0, 1.0, -1.5, 1.5]), grid, torch.nextafter(grid, torch.full_like(grid, 2.0)),
                         torch.nextafter(grid, torch.full_like(grid, -2.0))])
    m = min(special.numel(), flat.numel())          # (the smallest case holds the first 374 of them)
    flat[:m] = special[:m]
    frames01 = torch.clamp((x + 1.0) / 2.0, 0.0, 1.0)
    frames_f = frames01.permute(0, 2, 3, 4, 1).numpy()                               # (B, T, H, W, C) as perform_save_locally_video
    want_trunc = (255.0 * frames_f).astype(np.uint8)
    want_round = np.clip(frames_f * 255.0 + 0.5, 0, 255).astype(np.uint8)
    xd = x.to(dev)
    assert np.array_equal(ops.frames_to_u8(xd).cpu().numpy(), want_trunc)
    assert np.array_equal(ops.frames_to_u8(xd, rounding=True).cpu().numpy(), want_round)
    assert np.array_equal(ops.frames_to_u8(frames01.to(dev), unit_range=True).cpu().numpy(), want_trunc)
    assert np.array_equal(ops.frames_to_u8(frames01.to(dev), rounding=True, unit_range=True).cpu().numpy(), want_round)


def test_save_on_device_writes_the_same_files(dev, tmp_path):
    from scripts.sampling.util import perform_save_locally_video
    x = torch.rand(2, 3, 4, 16, 24, generator=torch.Generator().manual_seed(3)) * 2.2 - 1.1
    a, b = str(tmp_path / "host"), str(tmp_path / "dev")
    pa = perform_save_locally_video(a, torch.clamp((x + 1.0) / 2.0, 0.0, 1.0), fps=3, return_savepaths=True)
    pb = perform_save_locally_video(b, x.to(dev), fps=3, return_savepaths=True, gpu_io=True, signed=True)
    assert [os.path.relpath(p, a) for p in pa] == [os.path.relpath(p, b) for p in pb]
    for sub in ("gif", "grid"):
        names = sorted(os.listdir(os.path.join(a, sub)))
        assert names == sorted(os.listdir(os.path.join(b, sub))) and len(names) == 2
        for nm in names:
            assert open(os.path.join(a, sub, nm), "rb").read() == open(os.path.join(b, sub, nm), "rb").read()


@pytest.mark.timeout(1200)
def test_job_mode_with_gpu_io_writes_identical_files(dev, tmp_path):
    """The job-mode entry point on a directory-of-images job, with and without --gpu_io: every step on that route is exact, so the
    frame files are byte-identical and log_info.json holds the same entries."""
    import yaml
    from PIL import Image
    from ccedit_amd.sgm_compat import engine_config
    cfg = os.path.join(str(tmp_path), "tv2v.yaml")
    with open(cfg, "w") as f:
        yaml.safe_dump(dict(model=engine_config(crossframe=False, vae_ch=32, model_channels=64, num_heads=2, context_dim=64)), f)
    rs = np.random.RandomState(1)
    vids = []
    for name in ("a", "b"):
        d = tmp_path / "clips" / name
        d.mkdir(parents=True)
        for i in range(9):
            Image.fromarray(rs.randint(0, 256, (90, 150, 3)).astype(np.uint8)).save(str(d / f"{i:03d}.png"))
        vids.append(str(d))
    (tmp_path / "prompts.txt").write_text("a red fox\na blue bird\n")
    (tmp_path / "videos.txt").write_text("\n".join(vids) + "\n")
    base = ["--config_path", cfg, "--synthetic", "--H", "64", "--W", "128", "--num_keyframes", "3", "--sample_steps", "2",
            "--sampler_name", "DPMPP2SAncestralSampler", "--original_fps", "9", "--target_fps", "3", "--noise_seed", "5",
            "--prompt_listpath", str(tmp_path / "prompts.txt"), "--video_listpath", str(tmp_path / "videos.txt"), "--batch_size", "2",
            "--save_type", "gif"]
    outs = []
    for tag, extra in (("host", []), ("gpu", ["--gpu_io"])):
        out = str(tmp_path / tag)
        cmd = [sys.executable, os.path.join(ROOT, "scripts", "sampling", "sampling_tv2v.py"), *base, "--save_path", out, *extra]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=500, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        outs.append(out)
    logs = [json.load(open(os.path.join(o, "default", "log_info.json"))) for o in outs]
    assert logs[0]["video_paths"] == logs[1]["video_paths"] == vids
    assert [os.path.relpath(p, outs[0]) for p in logs[0]["keyframes_paths"]] == [os.path.relpath(p, outs[1]) for p in logs[1]["keyframes_paths"]]
    assert {k: v for k, v in logs[0].items() if k != "keyframes_paths"} == {k: v for k, v in logs[1].items() if k != "keyframes_paths"}
    for kind in ("original", "control_hint", "result"):
        names = sorted(os.listdir(os.path.join(outs[0], "default", kind, "gif")))
        assert names == sorted(os.listdir(os.path.join(outs[1], "default", kind, "gif"))) and len(names) == 2
        for nm in names:
            a = open(os.path.join(outs[0], "default", kind, "gif", nm), "rb").read()
            b = open(os.path.join(outs[1], "default", kind, "gif", nm), "rb").read()
            assert a == b, f"{kind}/{nm} differs between the host route and --gpu_io"
