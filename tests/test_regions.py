"""Region prompts without a GPU (ccedit_amd/regions.py, --region_prompt / --region_mask): the properties of the numpy restatement the
kernels are held to (tests/_regions_numpy.py), every refusal of the command line before a model is built, log_info.json, the nesting
order of the wrappers in sample_latent, the per-clip cache limits of the network wrapper."""
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _regions_numpy as RN  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _args(*argv, ref=False):
    from scripts.sampling import sampling_tv2v as S
    from scripts.sampling import sampling_tv2v_ref as R
    return (R if ref else S).parse_args(list(argv))


# ---- 1. the restatement ----------------------------------------------------------------------------
def _random_masks(k, t, hh, ww, seed):
    rs = np.random.RandomState(seed)
    m = rs.randint(0, 256, (k, t, hh, ww)).astype(np.uint8)
    for r in range(k):                                             # blocks of solid colour, so that cells are owned, shared and empty
        y0, x0 = rs.randint(hh // 2), rs.randint(ww // 2)
        m[r, :, y0:y0 + hh // 2, x0:x0 + ww // 2] = 255
        m[r, :, :8, :] = 0
    return m


@pytest.mark.parametrize("k,t,hh,ww,f", [(1, 1, 64, 64, 0), (2, 2, 72, 104, 1), (7, 1, 64, 128, 3), (3, 1, 72, 104, 8), (2, 1, 8, 8, 2)])
def test_coefficients_are_a_partition_of_one(k, t, hh, ww, f):
    coef = RN.region_weights(_random_masks(k, t, hh, ww, 5 * k + f), f)
    assert coef.dtype == np.float32 and coef.shape == (k + 1, t, hh // 8, ww // 8)
    assert (coef >= 0).all() and (coef <= 1).all()
    assert np.abs(coef.astype(np.float64).sum(axis=0) - 1.0).max() <= 2.0 ** -22
    assert ((coef != 0).sum(axis=0) >= 1).all(), "a cell without a non-zero coefficient"
    # where one region has everything its coefficient is exactly 1.0 and all others exactly 0.0
    one = coef == 1.0
    assert (np.where(one.any(axis=0)[None], (coef == 0.0) | one, True)).all()


@pytest.mark.parametrize("f", [0, 1, 8])
def test_black_masks_and_a_frame_filling_region(f):
    black = RN.region_weights(np.zeros((3, 2, 72, 104), np.uint8), f)
    assert (black[0] == 1.0).all() and (black[1:] == 0.0).all()
    masks = np.zeros((2, 2, 72, 104), np.uint8)
    masks[1] = 255
    full = RN.region_weights(masks, f)
    assert (full[2] == 1.0).all(), "a frame-filling region loses weight at the border"          # (clamping replicates the edge)
    assert (full[0] == 0.0).all() and (full[1] == 0.0).all()
    masks[1, :, 3, 5] = 127                                         # below the threshold: one pixel short in one cell
    assert (RN.region_weights(masks, f)[2] < 1.0).any()


def test_identical_masks_share_half_and_half():
    m = _random_masks(1, 2, 64, 96, 3)
    coef = RN.region_weights(np.concatenate([m, m]), 1)
    s = RN.box_sums(RN.cell_counts(m), 1)[0]
    shared = 2 * s >= 64 * 9                                        # tot >= S: the base prompt has nothing left
    assert shared.any() and (coef[1][shared] == 0.5).all() and (coef[2][shared] == 0.5).all() and (coef[0][shared] == 0.0).all()
    assert np.array_equal(coef[1], coef[2])


def test_hard_split_is_exact_on_a_cell_boundary():
    masks = np.zeros((2, 1, 64, 128), np.uint8)
    masks[0, :, :, :64] = 255
    masks[1, :, :, 64:] = 255
    coef = RN.region_weights(masks, 0)
    assert (coef[0] == 0.0).all()
    assert (coef[1][..., :8] == 1.0).all() and (coef[1][..., 8:] == 0.0).all()
    assert (coef[2][..., 8:] == 1.0).all() and (coef[2][..., :8] == 0.0).all()
    # a boundary inside a cell: that column of cells is shared by its pixel counts, 3 / 8 and 5 / 8
    masks = np.zeros((2, 1, 64, 128), np.uint8)
    masks[0, :, :, :67] = 255
    masks[1, :, :, 67:] = 255
    coef = RN.region_weights(masks, 0)
    assert (coef[1][..., 8] == np.float32(24.0 / 64.0)).all() and (coef[2][..., 8] == np.float32(40.0 / 64.0)).all()


def test_fuse_restatement_skips_zero_terms_and_copies_owned_cells():
    rs = np.random.RandomState(1)
    masks = np.zeros((1, 1, 32, 64), np.uint8)
    masks[0, :, :, 32:] = 255
    coef = RN.region_weights(masks, 1)
    ys = [rs.standard_normal((2, 4, 1, 4, 8)).astype(np.float32) for _ in range(2)]
    ys[1][..., :3] = np.nan                                         # where region 1's coefficient is exactly 0
    assert (coef[1][..., :3] == 0).all()
    out = RN.region_fuse(ys, coef)
    assert np.isfinite(out).all()
    assert np.array_equal(out[..., :3].view(np.int32), ys[0][..., :3].view(np.int32))
    assert np.array_equal(out[..., 5:].view(np.int32), ys[1][..., 5:].view(np.int32))
    mid = (coef[0][0, :, 3] * ys[0][..., 3]).astype(np.float32) + (coef[1][0, :, 3] * ys[1][..., 3]).astype(np.float32)
    assert np.array_equal(out[..., 3].view(np.int32), mid.astype(np.float32).view(np.int32))


def test_constants_live_in_regions_alone():
    from ccedit_amd import regions
    assert (regions.MAX_REGIONS, regions.MAX_FEATHER, regions.DEFAULT_FEATHER, regions.CELL, regions.THRESHOLD) == (7, 8, 1, 8, 128)
    assert _args().region_feather == regions.DEFAULT_FEATHER


# ---- 2. the command line ---------------------------------------------------------------------------
@pytest.fixture()
def mask_png(tmp_path):
    from PIL import Image
    p = str(tmp_path / "m.png")
    Image.fromarray(np.zeros((64, 128), np.uint8)).save(p)
    return p


def test_without_region_flags_nothing_is_imported_or_checked(monkeypatch):
    from scripts.sampling import sampling_tv2v as S
    monkeypatch.delitem(sys.modules, "ccedit_amd.regions", raising=False)
    a = _args("--H", "100", "--W", "77", "--batch_size", "4")
    assert not S.regions_on(a) and a.region_prompt is None and a.region_mask is None
    S.check_region_options(a, with_ref=True)
    S.check_region_jobs(a, 5)
    assert S.region_setup(a, None, None, None, None, None, "") == {}
    assert "ccedit_amd.regions" not in sys.modules


def test_region_flag_refusals(mask_png, tmp_path):
    many = []
    for i in range(8):
        many += ["--region_prompt", f"p{i}", "--region_mask", mask_png]
    seq = tmp_path / "seq"
    seq.mkdir()
    cases = [
        (["--region_prompt", "a"], "give one mask per prompt"),
        (["--region_mask", mask_png], "give one mask per prompt"),
        (["--region_prompt", "a", "--region_prompt", "b", "--region_mask", mask_png], "2 --region_prompt and 1 --region_mask"),
        (many, "at most 7"),
        (["--region_prompt", "a", "--region_mask", mask_png, "--region_feather", "9"], "0 ... 8"),
        (["--region_prompt", "a", "--region_mask", mask_png, "--region_feather", "-1"], "0 ... 8"),
        (["--region_prompt", "a", "--region_mask", str(tmp_path / "missing.png")], "does not exist"),
        (["--region_prompt", "a", "--region_mask", mask_png, "--region_track", "--H", "64", "--W", "128"], "give --video_path"),
        (["--region_prompt", "a", "--region_mask", mask_png, "--region_track", "--H", "72", "--W", "128", "--video_path", "v"], "multiples of 64"),
        (["--region_prompt", "a", "--region_mask", mask_png, "--region_track", "--H", "64", "--W", "128", "--video_path", "v", "--region_frame", "-2"],
         "outside the video"),
        (["--region_prompt", "a", "--region_mask", str(seq), "--region_track", "--H", "64", "--W", "128", "--video_path", "v"], "is a mask sequence"),
    ]
    for argv, words in cases:
        with pytest.raises(ValueError, match=re.escape(words)):
            _args(*argv)
    ok = _args("--region_prompt", "a", "--region_mask", mask_png, "--region_prompt", "b", "--region_mask", mask_png, "--region_feather", "0")
    assert ok.region_prompt == ["a", "b"] and ok.region_mask == [mask_png, mask_png] and ok.region_feather == 0


def test_more_than_one_clip_is_refused_before_a_model_is_built(mask_png, tmp_path, monkeypatch):
    from scripts.sampling import sampling_tv2v as S
    monkeypatch.setattr(S, "build_model", lambda *a, **k: pytest.fail("a model was built"))
    plist, vlist = tmp_path / "p.txt", tmp_path / "v.txt"
    plist.write_text("a fox\na dog\n")
    vlist.write_text("x\ny\n")
    region = ["--region_prompt", "snow", "--region_mask", mask_png, "--synthetic", "--config_path", "none.yaml"]
    with pytest.raises(ValueError, match="one video"):
        S.run_jobs(_args("--prompt_listpath", str(plist), "--video_listpath", str(vlist), *region))
    with pytest.raises(ValueError, match="--batch_size 1"):
        S.run_jobs(_args("--prompt", "a fox", "--video_path", "x", "--num_samples", "2", "--batch_size", "2", *region))
    S.check_region_jobs(_args("--prompt", "a fox", "--video_path", "x", "--num_samples", "2", "--batch_size", "1", *region), 1)
    S.check_region_jobs(_args("--prompt", "a fox", "--video_path", "x", "--batch_size", "4", *region), 1)


def test_regions_are_refused_with_a_reference_image(mask_png, tmp_path, monkeypatch):
    from scripts.sampling import sampling_tv2v as S
    from scripts.sampling import sampling_tv2v_ref as R
    flags = ["--region_prompt", "snow", "--region_mask", mask_png]
    with pytest.raises(NotImplementedError, match="reference image"):
        S.check_region_options(_args(*flags), with_ref=True)
    monkeypatch.setattr(R, "build_model", lambda *a, **k: pytest.fail("a model was built"))
    monkeypatch.setattr(sys, "argv", ["sampling_tv2v_ref.py", "--config_path", "none.yaml", "--synthetic", *flags])
    with pytest.raises(NotImplementedError, match="region_prompt"):
        R.main()


# ---- 3. log_info.json ------------------------------------------------------------------------------
def test_log_info_records_the_regions(mask_png, tmp_path, monkeypatch):
    """run_jobs with the model, the sampler and the region table stubbed: the job's log_info.json gains `regions`."""
    from PIL import Image
    from scripts.sampling import sampling_tv2v as S
    vdir = tmp_path / "clips" / "bear"
    vdir.mkdir(parents=True)
    rs = np.random.RandomState(2)
    for i in range(9):
        Image.fromarray(rs.randint(0, 256, (64, 128, 3)).astype(np.uint8)).save(str(vdir / f"{i:03d}.png"))

    class Conditioner:
        def get_unconditional_conditioning(self, batch, batch_uc=None):
            return (dict(crossattn=batch["txt"].float(), control_hint=batch["control_hint"]),
                    dict(crossattn=batch_uc["txt"].float(), control_hint=batch_uc["control_hint"]))

    class Model:
        conditioner = Conditioner()

    seen = {}

    def sample_one(args, model, dev, c, uc, randn, keyframes=None, regions=None, **kw):
        seen["regions"] = regions
        return torch.zeros_like(keyframes)

    def weights(masks, feather):
        seen["masks"], seen["feather"] = masks, feather
        return torch.zeros(masks.shape[0] + 1, masks.shape[1], masks.shape[2] // 8, masks.shape[3] // 8)

    from ccedit_amd import regions
    monkeypatch.setattr(S, "build_model", lambda a: (setattr(a, "context_dim", 64), (Model(), torch.device("cpu")))[1])
    monkeypatch.setattr(S, "sample_one", sample_one)
    monkeypatch.setattr(regions, "weights", weights)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    out = str(tmp_path / "out")
    args = _args("--synthetic", "--config_path", "none.yaml", "--H", "64", "--W", "128", "--num_keyframes", "3", "--original_fps", "9",
                 "--target_fps", "3", "--prompt", "a panda", "--video_path", str(vdir), "--save_path", out, "--save_type", "npy",
                 "--region_prompt", "a snow field", "--region_mask", mask_png, "--region_prompt", "a red scarf", "--region_mask", mask_png,
                 "--region_feather", "2")
    S.run_jobs(args)
    with open(os.path.join(out, "default", "log_info.json")) as f:
        log = json.load(f)
    assert log["regions"] == [dict(prompt="a snow field", mask=mask_png, feather=2, tracked=False),
                              dict(prompt="a red scarf", mask=mask_png, feather=2, tracked=False)]
    assert log["video_paths"] == [str(vdir)] and len(log["keyframes_paths"]) == 1
    # what the sampler was handed: the base context first, a context per region prompt (seeded by the text with its --add_prompt
    # prefix, like the main prompt), the masks with the clip's geometry
    r = seen["regions"]
    assert len(r["contexts"]) == 3 and all(tuple(v.shape) == (1, 77, 64) for v in r["contexts"]) and tuple(r["coef"].shape) == (3, 3, 8, 16)
    want, _ = S.job_text(args, ["a snow field"], torch.device("cpu"), 64)
    assert torch.equal(r["contexts"][1], want.float()) and not torch.equal(r["contexts"][1], r["contexts"][2])
    assert tuple(seen["masks"].shape) == (2, 3, 64, 128) and seen["masks"].dtype == torch.uint8 and seen["feather"] == 2


# ---- 4. nesting and cache limits ---------------------------------------------------------------------
class _Wrapper:
    frame_shard = row_shard = None

    def __init__(self):
        self.calls = []

    def reserve_windows(self, n):
        self.calls.append(("windows", n))

    def reserve_contexts(self, n):
        self.calls.append(("contexts", n))


@pytest.mark.parametrize("extra,inner", [
    ([], "plain"),
    (["--num_keyframes", "6", "--window_frames", "3"], "windows"),
    (["--H", "128", "--W", "192", "--tile_h", "64", "--tile_w", "64", "--num_keyframes", "6", "--window_frames", "3"], "tiles"),
])
def test_regions_are_the_outermost_wrapper(extra, inner, mask_png, monkeypatch):
    from ccedit_amd import regions, tiles, windows
    from scripts.sampling import sampling_tv2v as S
    from scripts.sampling import util

    class Model:
        model = _Wrapper()

        @staticmethod
        def denoiser(network, inp, sigma, cc):
            return inp

    monkeypatch.setattr(util, "init_sampling", lambda **kw: (lambda denoiser, start, c, uc=None: denoiser))
    args = _args("--region_prompt", "snow", "--region_mask", mask_png, *(extra or ["--H", "64", "--W", "128", "--num_keyframes", "3"]))
    t, h, w = args.num_keyframes, args.H // 8, args.W // 8
    c = dict(crossattn=torch.zeros(1, 77, 64), control_hint=torch.zeros(1, 3, t, args.H, args.W))
    reg = dict(contexts=[c["crossattn"], torch.ones(1, 77, 64)], coef=torch.zeros(2, t, h, w))
    outer = S.sample_latent(args, Model(), None, c, dict(c), torch.zeros(1, 4, t, h, w), regions=reg)
    assert isinstance(outer, regions.RegionDenoiser) and outer.wrapper is Model.model and outer.coef is reg["coef"]
    assert tuple(outer.coef.shape[1:]) == (t, h, w), "the coefficient table has the full latent's shape"
    if inner == "plain":
        assert not isinstance(outer.denoiser, (windows.WindowedDenoiser, tiles.TiledDenoiser)) and callable(outer.denoiser)
    elif inner == "windows":
        assert isinstance(outer.denoiser, windows.WindowedDenoiser) and outer.denoiser.window == 3
    else:
        assert isinstance(outer.denoiser, tiles.TiledDenoiser) and outer.denoiser.window == 3 and (outer.denoiser.th, outer.denoiser.tw) == (8, 8)
    # without regions the chain is what it was
    plain = S.sample_latent(args, Model(), None, c, dict(c), torch.zeros(1, 4, t, h, w))
    assert not isinstance(plain, regions.RegionDenoiser)


def test_region_denoiser_builds_its_contexts_once_per_clip():
    from ccedit_amd import regions
    w = _Wrapper()
    ctx = [torch.full((1, 77, 8), float(i)) for i in range(3)]
    rd = regions.RegionDenoiser(lambda x, s, c: x, ctx, torch.zeros(3, 2, 4, 4), wrapper=w)
    ca = torch.cat([torch.full((1, 77, 8), -1.0), ctx[0]])
    first = rd._region_contexts(ca)
    assert rd._region_contexts(ca) is first and w.calls == [("contexts", 3)]
    for r, d in enumerate(first):
        assert tuple(d.shape) == (2, 77, 8) and torch.equal(d[:1], ca[:1]) and torch.equal(d[1:], ctx[r])
    ca.add_(1.0)                                                    # written in place: another version, the entry is rebuilt
    again = rd._region_contexts(ca)
    assert again is not first and torch.equal(again[2][:1], ca[:1]) and len(w.calls) == 2
    with pytest.raises(ValueError, match="one clip"):
        rd._region_contexts(torch.zeros(4, 77, 8))
    with pytest.raises(ValueError):
        regions.RegionDenoiser(lambda x, s, c: x, ctx[:1], torch.zeros(1, 2, 4, 4))
    with pytest.raises(ValueError):
        regions.RegionDenoiser(lambda x, s, c: x, ctx, torch.zeros(2, 2, 4, 4))
    with pytest.raises(ValueError, match="table's T, h, w"):
        rd(torch.zeros(2, 4, 2, 4, 5), torch.ones(2), dict(crossattn=ca))


def test_network_wrapper_limits_follow_windows_times_contexts():
    from ccedit_amd.network import OpenAIWrapperControlLDM3DTV2V as W
    w = W.__new__(W)
    assert (w._graph_slots, w._hint_slots, w._tkv_slots, w._graph_pool) == (2, 4, 6, None)
    w.reserve_contexts(3)                                           # K = 2 on a plain clip
    assert (w._graph_slots, w._hint_slots, w._tkv_slots) == (3, 4, 6)
    w.reserve_contexts(4)                                           # K = 3: eight text K / V entries
    assert (w._graph_slots, w._hint_slots, w._tkv_slots) == (4, 4, 8)
    w.reserve_windows(6)                                            # ... around tiles x windows = 6: the region wrapper reserved first
    assert (w._graph_slots, w._hint_slots, w._tkv_slots) == (24, 12, 8)
    assert w.graph_counts == dict(eager=0, capture=0, replay=0)
    w.reserve_windows(0)                                            # a plain clip's limits, the contexts' too
    assert (w._graph_slots, w._hint_slots, w._tkv_slots, w._graph_pool, w._contexts, w._windows) == (2, 4, 6, None, 1, 1)
    w.reserve_windows(3)                                            # windows alone: what they were
    assert (w._graph_slots, w._hint_slots, w._tkv_slots) == (3, 6, 6)
    w.reserve_windows(0)


def test_header_names_the_region_functions_and_keeps_the_abi():
    with open(os.path.join(ROOT, "include", "ccedit_hip.h")) as f:
        text = f.read()
    assert re.search(r"#define\s+CCEDIT_ABI_VERSION\s+12\b", text)
    assert re.search(r"\bint ccedit_region_weights\(", text) and re.search(r"\bint ccedit_region_fuse\(", text)
    from ccedit_amd import hip
    assert "ccedit_region_weights" in hip.EXPORTS and "ccedit_region_fuse" in hip.EXPORTS
    from ccedit_amd.csrc import build
    assert "region.hip" in build.SOURCES and "-ffp-contract=off" in build.EXTRA_FLAGS["region.hip"]
    assert not any("fast" in f for f in build.EXTRA_FLAGS["region.hip"])
