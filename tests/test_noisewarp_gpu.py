"""Motion-following noise on a real MI355X (ccedit_amd/noisewarp.py, csrc/noisewarp.hip, --noise_warp).

Exact (no tolerance anywhere, everything compared through int32 views): every entry point and noisewarp.build as a whole against the
numpy restatement (tests/_noisewarp_numpy.py, whose own properties tests/test_noisewarp.py checks) on matched vector fields of
scenes and of random bytes at 64 x 64, 64 x 128 and 128 x 192 with keyframes every frame, every third frame and unevenly spaced, and
on hand-made fields: zero, a pure cell shift, components beyond the clamp, the forward-backward limit between 4 and 5, every cell
arriving at one sample.  The gather on NaN and inf bit patterns, both store widths, and its refusals; the wrap around a noise source
(draw counts, the mix at rho < 1, the samplers' walks); and the entry point on PNG frame directories."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _noisewarp_numpy as ref  # noqa: E402
from _masktrack_scenes import random_frames, scene  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [(64, 64), (64, 128), (128, 192)]
SPACINGS = {"every frame": tuple(range(13)), "every third": (0, 3, 6, 9, 12), "uneven": (0, 1, 5, 12)}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from ccedit_amd import hip
    hip.lib()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same(got, want):
    """A device tensor against a numpy array, through int32 views."""
    want = torch.from_numpy(np.ascontiguousarray(want))
    return got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape) and torch.equal(_bits(got), want.view(torch.int32))


@functools.lru_cache(maxsize=None)
def _clip(kind, h, w):
    """(13 frames, the matcher's vectors of all 24 pairs) — computed once, shared and never written to."""
    src = random_frames(h, w, 13, 11) if kind == "random" else scene(h, w, 13, 3, bg=(1, -2), obj=(-2, 3))[0]
    return src, ref.vectors(src)


def _pair_field(h, w, v, r):
    """The vectors of a clip of two frames: v everywhere for 1 -> 0, r everywhere for 0 -> 1."""
    vec = np.zeros((2, h // 8, w // 8, 2), np.int32)
    vec[0], vec[1] = v, r
    return vec


def _target(h, w):
    """The centre of a cell next to the middle of the frame: up to 128 x 128 no cell is further from it than the clamp's 64 pixels,
    at W = 192 the vectors of the outer columns are clamped short of it (the kernel against numpy all the same)."""
    return 8 * (h // 16 - 1) + 4, 8 * (w // 16 - 1) + 4


def _hand_made(h, w):
    yield "zero", _pair_field(h, w, (0, 0), (0, 0)), ref.FB_LIMIT
    yield "a cell shift", _pair_field(h, w, (8, -16), (-8, 16)), ref.FB_LIMIT
    yield "beyond the clamp", _pair_field(h, w, (200, -200), (-200, 200)), ref.FB_LIMIT
    yield "any int32", np.random.RandomState(3).randint(-2 ** 31, 2 ** 31, (2, h // 8, w // 8, 2), dtype=np.int64).astype(np.int32), ref.FB_LIMIT
    yield "disagree by 5", _pair_field(h, w, (1, -1), (2, -1)), ref.FB_LIMIT           # v + r = (3, -2)
    yield "disagree by 4", _pair_field(h, w, (1, -1), (1, -1)), ref.FB_LIMIT           # v + r = (2, -2)
    cy, cx = ref.centres(h // 8, w // 8)                             # every vector points at the centre of the cell _target names
    ty, tx = _target(h, w)
    one = np.zeros((2, h // 8, w // 8, 2), np.int32)
    one[0] = np.stack([ty - cy, tx - cx], axis=1).reshape(h // 8, w // 8, 2)
    yield "one cell", one, 10 ** 6


# ---- 1. track ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", SIZES)
@pytest.mark.parametrize("kind", ["random", "scene"])
def test_track_is_exact_on_matched_fields(h, w, kind):
    _need_gpu()
    from ccedit_amd import ops
    _, vec = _clip(kind, h, w)
    dvec = _dev(vec)
    for name, key in SPACINGS.items():
        got = ops.noisewarp_track(dvec, key, h, w, ref.FB_LIMIT)
        want = ref.track(vec, key, h, w)
        assert _same(got, want), (kind, h, w, name, int((got.cpu().numpy() != want).any(axis=-1).sum()))


@pytest.mark.parametrize("h,w", SIZES)
def test_track_is_exact_on_hand_made_fields(h, w):
    _need_gpu()
    from ccedit_amd import ops
    cy, cx = ref.centres(h // 8, w // 8)
    got = {}
    for name, vec, limit in _hand_made(h, w):
        want = ref.track(vec, (0, 1), h, w, limit)
        got[name] = ops.noisewarp_track(_dev(vec), (0, 1), h, w, limit)
        assert _same(got[name], want), (name, h, w)
        got[name] = got[name].cpu().numpy()
    assert not got["zero"][0].any() and got["zero"][1, :, 0].all(), "row 0 is zero, a still clip keeps every cell"
    assert np.array_equal(got["zero"][1, :, 1], cy) and np.array_equal(got["zero"][1, :, 2], cx)
    inside = (cy + 8 < h) & (cx - 16 >= 0)
    assert np.array_equal(got["a cell shift"][1, :, 0] != 0, inside) and 0 < inside.sum() < inside.size, "border cells go invalid"
    clamped = ops.noisewarp_track(_dev(_pair_field(h, w, (64, -64), (-64, 64))), (0, 1), h, w, ref.FB_LIMIT).cpu().numpy()
    assert np.array_equal(got["beyond the clamp"], clamped), "+-200 is read as +-64"
    assert not got["disagree by 5"][1, :, 0].any() and got["disagree by 4"][1, :, 0].all()
    if w <= 128:
        assert got["one cell"][1, :, 0].all() and (got["one cell"][1, :, 1:] == _target(h, w)).all()


def test_track_refuses_bad_arguments():
    _need_gpu()
    from ccedit_amd import ops
    vec = _dev(np.zeros((4, 8, 8, 2), np.int32))
    for key in ((0,), (1, 2), (0, 2, 2), (0, 3)):
        with pytest.raises(ValueError, match="keyframes"):
            ops.noisewarp_track(vec, key, 64, 64, 4)
    with pytest.raises(ValueError, match="vec"):
        ops.noisewarp_track(vec[:3], (0, 1), 64, 64, 4)
    with pytest.raises(ValueError, match="int32"):
        ops.noisewarp_track(vec, (0, 2), 64, 128, 4)


# ---- 2. claim and resolve ------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", SIZES)
def test_origins_are_exact_and_do_not_depend_on_arrival_order(h, w):
    _need_gpu()
    from ccedit_amd import ops
    cells = (h // 8) * (w // 8)
    fields = [(f"{kind} {name}", ref.track(_clip(kind, h, w)[1], key, h, w)) for kind in ("random", "scene") for name, key in SPACINGS.items()]
    fields += [(name, ref.track(vec, (0, 1), h, w, limit)) for name, vec, limit in _hand_made(h, w)]
    for name, trk in fields:
        want = ref.origins(trk, h, w)
        runs = [ops.noisewarp_origins(_dev(trk), h, w) for _ in range(2)]
        for org, src, inherited in runs:
            assert _same(org, want[0]) and _same(src, want[1]), (name, h, w)
            assert inherited.cpu().tolist() == want[2].tolist(), (name, h, w)
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(*runs)), "two runs are bit-equal"
        src = runs[0][1].cpu().numpy()
        assert all(len(np.unique(row)) == cells for row in src), f"{name}: a frame reads a sample twice"
        if name == "one cell" and w <= 128:
            ty, tx = _target(h, w)
            assert want[2].tolist() == [0, 1] and src[1, 0] == (ty >> 3) * (w // 8) + (tx >> 3), "exactly one cell wins: the smallest index"
            assert np.array_equal(src[1, 1:], cells + np.arange(1, cells))
        if name == "zero":
            assert np.array_equal(src[1], np.arange(cells))


# ---- 3. the gather -------------------------------------------------------------------------------------
def _raw(b, k, h, w, seed):
    """fp32 (b, 4, k, h, w) of any bit patterns, NaNs of several payloads and both infinities among them."""
    rs = np.random.RandomState(seed)
    bits = rs.randint(-2 ** 31, 2 ** 31, (b, 4, k, h, w), dtype=np.int64).astype(np.int32)
    flat = bits.reshape(-1)
    flat[:6] = np.asarray([0x7fc00000, 0x7fc00001, 0xffc12345, 0x7f800000, 0xff800000, 0x80000000], np.uint32).view(np.int32)
    return bits.view(np.float32)


@pytest.mark.parametrize("b", [1, 2])
@pytest.mark.parametrize("h,w", [(8, 8), (8, 16), (3, 5)])
def test_gather_is_numpy_fancy_indexing(b, h, w):
    """(3, 5): 75 samples per plane, no multiple of 4 — the 4-byte arm; the others take 16-byte stores on a fresh tensor and the 4-byte
    arm on a view one element into a buffer."""
    _need_gpu()
    from ccedit_amd import ops
    k, n = 5, 5 * h * w
    raw = _raw(b, k, h, w, 7 + b)
    rs = np.random.RandomState(b)
    src = np.stack([rs.permutation(n) if i == 0 else rs.randint(0, n, n) for i in range(b)]).astype(np.int32).reshape(b, k, h * w)
    want = ref.gather(raw, src)
    draw, dsrc = _dev(raw), _dev(src)
    assert draw.data_ptr() % 16 == 0 and dsrc.data_ptr() % 16 == 0
    got = ops.noise_warp(draw, dsrc)
    assert _same(got, want), (b, h, w)
    assert torch.equal(_bits(draw), torch.from_numpy(raw).view(torch.int32)), "the input is left alone"
    buf = torch.zeros(raw.size + 5, dtype=torch.float32, device="cuda")
    view = buf[1:1 + raw.size].view(raw.shape)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    assert ops.noise_warp(draw, dsrc, out=view, checked=True) is view and _same(view, want)
    assert _bits(buf)[0] == 0 and not _bits(buf)[1 + raw.size:].any(), "nothing is written outside the view"
    ident = _dev(np.arange(b * n, dtype=np.int32).reshape(b, k, h * w) % n)
    assert _same(ops.noise_warp(draw, ident), raw)


def test_gather_refuses_an_index_out_of_range_and_wrong_shapes():
    _need_gpu()
    from ccedit_amd import hip, ops
    raw = _dev(_raw(2, 5, 8, 8, 1))
    good = np.tile(np.arange(320, dtype=np.int32), 2).reshape(2, 5, 64)
    for at, value in (((0, 0, 0), 320), ((1, 4, 63), -1), ((1, 2, 3), 2 ** 31 - 1)):
        bad = good.copy()
        bad[at] = value
        out = torch.full_like(raw, 3.0)
        with pytest.raises(hip.HipLibraryError, match="outside 0 ... 319"):
            ops.noise_warp(raw, _dev(bad), out=out)
        assert bool((out == 3.0).all()), "an error status, not a launch"
        flag, dbad = torch.zeros(1, dtype=torch.int32, device="cuda"), _dev(bad)
        assert hip.lib().ccedit_noisewarp_check(dbad.data_ptr(), 2, 320, flag.data_ptr(), None) == -1
    ops.noisewarp_check(_dev(good))
    for src in (_dev(good[:1]), _dev(good.reshape(2, 64, 5)), _dev(good).long(), _dev(good).cpu()):
        with pytest.raises(ValueError, match="src"):
            ops.noise_warp(raw, src)
    with pytest.raises(ValueError, match="raw"):
        ops.noise_warp(raw[:, :, :, :, ::2], _dev(good))
    with pytest.raises(ValueError, match="out"):
        ops.noise_warp(raw, _dev(good), out=torch.empty(2, 4, 5, 64, device="cuda"))
    lib, p, dgood = hip.lib(), raw.data_ptr(), _dev(good)
    assert lib.ccedit_noise_warp(p, dgood.data_ptr(), p, 2, 4, 320, None) == -1 and b"two buffers" in lib.ccedit_last_error()
    assert lib.ccedit_noise_warp(p, dgood.data_ptr(), p + 2, 2, 4, 320, None) == -1 and b"aligned" in lib.ccedit_last_error()


# ---- 4. build ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", SIZES)
@pytest.mark.parametrize("kind", ["random", "scene"])
def test_build_is_the_restatement_end_to_end(h, w, kind):
    _need_gpu()
    from ccedit_amd import noisewarp
    frames, _ = _clip(kind, h, w)
    dframes = _dev(frames)
    for key in ((0, 3, 6, 9, 12), (1, 2, 6, 11)):                    # (the second: the clip starts at frame 1, uneven spacing)
        want_src, want_shares = ref.build(frames, key)
        src, shares = noisewarp.build(dframes, key)
        assert _same(src, want_src), (kind, h, w, key)
        assert shares == want_shares.tolist() and shares[0] == 0.0
    one, share = noisewarp.build(dframes, (4,))
    assert _same(one, np.arange((h // 8) * (w // 8), dtype=np.int32)[None]) and share == [0.0]
    with pytest.raises(ValueError, match="strictly increasing"):
        noisewarp.build(dframes, (0, 3, 3))
    with pytest.raises(ValueError, match="multiples of 64"):
        noisewarp.build(dframes[:, :56], (0, 3))


# ---- 5. the wrap and the samplers ----------------------------------------------------------------------
class _Source:
    """A seeded noise source that counts its draws and keeps them."""

    def __init__(self, seed):
        self.gen, self.draws = torch.Generator().manual_seed(seed), []

    def __call__(self, x):
        self.draws.append(torch.randn(x.shape, generator=self.gen).to(x.device))
        return self.draws[-1]


def _all_from_frame_0(b, k, cells):
    return _dev(np.tile(np.arange(cells, dtype=np.int32), (b, k, 1)))


def test_wrap_draws_once_at_rho_1_and_mixes_a_second_draw_below():
    _need_gpu()
    from ccedit_amd import noisewarp, ops
    b, k, h, w = 2, 3, 8, 8
    src = _all_from_frame_0(b, k, h * w)
    x = torch.empty(b, 4, k, h, w, device="cuda")
    raw = _Source(5)
    got = noisewarp.wrap(raw, src, 1.0)(x)
    assert len(raw.draws) == 1 and torch.equal(_bits(got), _bits(ops.noise_warp(raw.draws[0], src)))
    assert all(torch.equal(_bits(got[:, :, f]), _bits(raw.draws[0][:, :, 0])) for f in range(k)), "every keyframe carries keyframe 0's noise"
    raw = _Source(5)
    got = noisewarp.wrap(raw, src, 0.5)(x)
    assert len(raw.draws) == 2
    want = ops.axpby(ops.noise_warp(raw.draws[0], src), raw.draws[1], 0.5, float(np.sqrt(1.0 - 0.25)))
    assert torch.equal(_bits(got), _bits(want))
    raw = _Source(5)
    got = noisewarp.wrap(raw, src, 0.0)(x)
    assert len(raw.draws) == 2 and torch.equal(_bits(got), _bits(raw.draws[1])), "rho = 0: the second, independent draw"
    raw = _Source(5)
    wrapped = noisewarp.wrap(raw, src, 1.0)
    for other in (torch.empty(b, 4, h, w, device="cuda"), torch.empty(b, 4, k + 1, h, w, device="cuda"), torch.empty(1, 4, k, h, w, device="cuda")):
        assert wrapped(other) is raw.draws[-1], "what is not the maps' shape passes through unchanged"
    assert len(raw.draws) == 3
    with pytest.raises(ValueError, match="--noise_warp_rho"):
        noisewarp.wrap(raw, src, 1.5)
    from ccedit_amd import hip
    with pytest.raises(hip.HipLibraryError, match="outside"):
        noisewarp.wrap(raw, src + 64 * k, 1.0)


def _stub(x, sigma, cond):
    """A fixed device function of (x, sigma) in place of the network."""
    s = sigma.to(x.device).reshape(-1, *([1] * (x.dim() - 1)))
    return x / (1.0 + s * s) + 0.05 * torch.sin(3.0 * x) * s / (1.0 + s)


def _sampler(name, source):
    from ccedit_amd import sampling
    smp = getattr(sampling, name)(discretization_config={"target": "ccedit_amd.sampling.LegacyDDPMDiscretization"}, num_steps=4)
    smp.noise_sampler = source
    return smp


@pytest.mark.parametrize("name", ["DPMPP2SAncestralSampler", "EulerAncestralSampler"])
def test_the_samplers_draw_as_often_with_the_wrap_and_an_identity_map_changes_nothing(name):
    _need_gpu()
    from ccedit_amd import noisewarp
    b, k, h, w = 1, 3, 8, 8
    g = torch.Generator().manual_seed(8)
    x, x0 = torch.randn(b, 4, k, h, w, generator=g).cuda(), torch.randn(b, 4, k, h, w, generator=g).cuda()
    mask = (torch.rand(b, k, h, w, generator=g) > 0.5).to(torch.uint8).cuda()
    ident = _dev(np.arange(k * h * w, dtype=np.int32).reshape(1, k, h * w))
    carried = _all_from_frame_0(b, k, h * w)

    def walk(src, inpaint):
        raw = _Source(21)
        smp = _sampler(name, raw if src is None else noisewarp.wrap(raw, src, 1.0))
        out = smp.sample_inpainting(_stub, x.clone(), {}, x0, mask=mask) if inpaint else smp(_stub, x.clone(), {})
        return out, len(raw.draws)

    for inpaint in (False, True):
        plain, n_plain = walk(None, inpaint)
        same, n_same = walk(ident, inpaint)
        moved, n_moved = walk(carried, inpaint)
        assert n_plain == n_same == n_moved == (8 if inpaint else 4), (name, inpaint, n_plain, n_same, n_moved)
        assert bool(torch.isfinite(moved).all()) and torch.equal(_bits(plain), _bits(same)), (name, inpaint)
        assert not torch.equal(_bits(plain), _bits(moved)), "the carried noise does something"


# ---- 6. the entry point --------------------------------------------------------------------------------
def _write_config(tmp_path):
    import yaml
    from ccedit_amd.sgm_compat import engine_config
    cfg = os.path.join(str(tmp_path), "tv2v.yaml")
    with open(cfg, "w") as f:
        yaml.safe_dump(dict(model=engine_config(crossframe=False, vae_ch=32, model_channels=64, num_heads=2, context_dim=64)), f)
    return cfg


def _frame_dir(tmp_path, name, frames):
    from PIL import Image
    vdir = tmp_path / "clips" / name
    vdir.mkdir(parents=True)
    for i, f in enumerate(frames):
        Image.fromarray(f).save(str(vdir / f"{i:03d}.png"))
    return str(vdir)


def _job(argv):
    """One job through run_jobs in this process -> <save_path>/default."""
    from scripts.sampling import sampling_tv2v as S
    args = S.parse_args(argv)
    torch.manual_seed(args.seed)
    with torch.no_grad():
        S.run_jobs(args)
    return os.path.join(args.save_path, "default")


def _result(out):
    path = os.path.join(out, "result", "png", "animation-0000.png")
    assert sorted(os.listdir(os.path.dirname(path))) == ["animation-0000.png"]
    return open(path, "rb").read()


def _base(tmp_path, vdir):
    return ["--config_path", _write_config(tmp_path), "--synthetic", "--H", "128", "--W", "192", "--num_keyframes", "5", "--sample_steps", "2",
            "--sampler_name", "DPMPP2SAncestralSampler", "--original_fps", "9", "--target_fps", "3", "--prompt", "a red fox",
            "--video_path", vdir, "--batch_size", "1", "--save_type", "png"]


@pytest.mark.timeout(600)
def test_a_job_whose_map_is_the_identity_writes_the_plain_runs_bytes(tmp_path):
    """Random bytes match nowhere: the restatement's map is the identity, so the carried run must be the plain run — the start latent,
    the ancestral draws (--noise_seed's CPU generator stays the raw source) and, in the second pair, windows and the re-injection draws
    of --inpainting_mode."""
    _need_gpu()
    from PIL import Image
    from scripts.sampling.util import load_video_frames_u8
    frames = random_frames(128, 192, 13, 5)
    src, shares = ref.build(frames, (0, 3, 6, 9, 12))
    assert np.array_equal(src.reshape(-1), np.arange(src.size)) and not np.any(shares)
    vdir = _frame_dir(tmp_path, "static", frames)
    assert np.array_equal(load_video_frames_u8(vdir, (128, 192), torch.device("cuda")).cpu().numpy(), frames)
    Image.fromarray(np.where(np.arange(192)[None, :] >= 96, 255, 0).astype(np.uint8).repeat(128, axis=0)).save(str(tmp_path / "mask.png"))
    base = _base(tmp_path, vdir) + ["--noise_seed", "1"]
    extras = {"plain": [], "windows": ["--window_frames", "3", "--window_overlap", "1", "--inpainting_mode", "--mask_path", str(tmp_path / "mask.png")]}
    for tag, extra in extras.items():
        plain = _job(base + extra + ["--save_path", str(tmp_path / f"{tag}_off")])
        warped = _job(base + extra + ["--noise_warp", "--save_path", str(tmp_path / f"{tag}_on")])
        assert _result(plain) == _result(warped), f"{tag}: an identity map changed the result"
        log_off, log_on = (json.load(open(os.path.join(o, "log_info.json"))) for o in (plain, warped))
        assert "noise_warp" not in log_off                                   # without the flag: the log as before
        assert log_on["noise_warp"]["rho"] == 1.0 and log_on["noise_warp"]["inherited"] == [0.0] * 5


@pytest.mark.timeout(600)
def test_a_job_on_a_still_clip_inherits_everything_and_differs_from_the_plain_run(tmp_path):
    _need_gpu()
    frames = np.repeat(random_frames(128, 192, 1, 6), 13, axis=0)
    vdir = _frame_dir(tmp_path, "still", frames)
    base = _base(tmp_path, vdir)                                             # (no --noise_seed: the device generator is the raw source)
    plain = _job(base + ["--save_path", str(tmp_path / "off")])
    warped = _job(base + ["--noise_warp", "--save_path", str(tmp_path / "on")])
    log = json.load(open(os.path.join(warped, "log_info.json")))
    assert log["noise_warp"] == dict(rho=1.0, inherited=[0.0, 1.0, 1.0, 1.0, 1.0], clips=[[0.0, 1.0, 1.0, 1.0, 1.0]])
    assert _result(plain) != _result(warped)
    mixed = _job(base + ["--noise_warp", "--noise_warp_rho", "0.5", "--save_path", str(tmp_path / "half")])
    assert json.load(open(os.path.join(mixed, "log_info.json")))["noise_warp"]["rho"] == 0.5
    assert _result(mixed) not in (_result(plain), _result(warped))
