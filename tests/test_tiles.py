"""Large frames (ccedit_amd/tiles.py, --tile_h / --tile_w / --tile_overlap): the host side — the tile plan, the flags, what is refused,
the numpy restatement of the kernels against itself.  No GPU."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _tiles_numpy as TN  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EPS = 2.0 ** -24


def _cover_and_sum(starts, coef, lh, lw):
    th, tw = coef.shape[1:]
    cover = np.zeros((lh, lw), np.int64)
    total = np.zeros((lh, lw), np.float64)
    for t, (sy, sx) in enumerate(starts):
        cover[sy:sy + th, sx:sx + tw] += 1
        total[sy:sy + th, sx:sx + tw] += coef[t].astype(np.float64)
    return cover, total


def _check_plan(lh, lw, th, tw, oh, ow):
    """The properties every plan has: float32 (tiles, th, tw); every pixel covered; single-covered pixels exactly 1.0; sums within
    2^-24 of 1; each coefficient raw / D from integers, rounded once; the numpy restatement gives the same tables."""
    from ccedit_amd.tiles import plan2d
    starts, coef = plan2d(lh, lw, th, tw, oh, ow)
    assert isinstance(coef, np.ndarray) and coef.dtype == np.float32 and coef.shape == (len(starts), th, tw)
    assert starts == sorted(starts) and len(set(starts)) == len(starts), starts            # y major, x minor, ascending
    assert all(0 <= sy <= lh - th and 0 <= sx <= lw - tw for sy, sx in starts), starts
    cover, total = _cover_and_sum(starts, coef, lh, lw)
    assert cover.min() >= 1, "a pixel no tile covers"
    assert np.abs(total - 1.0).max() <= EPS, np.abs(total - 1.0).max()
    for t, (sy, sx) in enumerate(starts):
        one = cover[sy:sy + th, sx:sx + tw] == 1
        assert np.all(coef[t][one] == np.float32(1.0))
    if oh <= th // 2 and ow <= tw // 2:
        assert cover.max() <= 4, cover.max()
    rs, rc = TN.plan2d(lh, lw, th, tw, oh, ow)
    assert rs == starts and np.array_equal(rc.view(np.int32), coef.view(np.int32))
    return starts, coef, cover


def test_plan_small_frame_with_and_without_overlap():
    from ccedit_amd.tiles import plan2d
    from ccedit_amd.windows import plan
    for o in ((8, 8), (0, 0)):
        starts, coef, cover = _check_plan(24, 40, 16, 24, *o)
        assert sorted({s[0] for s in starts}) == [0, 8] and sorted({s[1] for s in starts}) == [0, 16]
        assert starts == [(0, 0), (0, 16), (8, 0), (8, 16)]
        # the starts are windows.plan's, per axis
        assert plan(24, 16, o[0])[0] == [0, 8] and plan(40, 24, o[1])[0] == [0, 16]
        assert cover.max() == 4, "the pulled-back last tile overlaps the first even at overlap 0"
    # one coefficient by hand: pixel (8, 16) at overlap 0 is (8, 16) of tile 0, (8, 0) of tile 1, (0, 16) of tile 2, (0, 0) of tile 3
    starts, coef = plan2d(24, 40, 16, 24, 0, 0)
    r = lambda k, t: min(k + 1, t - k)
    raws = [r(8, 16) * r(16, 24), r(8, 16) * r(0, 24), r(0, 16) * r(16, 24), r(0, 16) * r(0, 24)]
    got = [coef[0, 8, 16], coef[1, 8, 0], coef[2, 0, 16], coef[3, 0, 0]]
    assert got == [np.float32(np.float64(v) / np.float64(sum(raws))) for v in raws]
    # a frame of exactly one tile
    starts, coef = plan2d(16, 24, 16, 24, 4, 6)
    assert starts == [(0, 0)] and np.array_equal(coef, np.ones((1, 16, 24), np.float32))


@pytest.mark.parametrize("lh,lw", [(128, 192), (136, 200)])
def test_plan_full_size(lh, lw):
    starts, coef, cover = _check_plan(lh, lw, 64, 96, 16, 24)
    if (lh, lw) == (128, 192):
        assert starts == [(sy, sx) for sy in (0, 48, 64) for sx in (0, 72, 96)]
    assert (cover == 1).any(), "no single-covered pixel: the exact-1.0 property was not exercised"


def test_plan_covers_a_frame_the_network_refuses_directly():
    """720 x 1280: a latent of 90 x 160, no multiple of 8 — refused by the network at its own size, covered by tiles of 64 x 96."""
    starts, coef, cover = _check_plan(90, 160, 64, 96, 16, 24)
    assert all(sy >= 0 and sx >= 0 and sy + 64 <= 90 and sx + 96 <= 160 for sy, sx in starts)
    assert sorted({s[0] for s in starts}) == [0, 26] and sorted({s[1] for s in starts}) == [0, 64]


@pytest.mark.parametrize("args,words", [
    ((24, 40, 12, 24, 4, 8), "multiple of 64"),            # tile not a multiple of 8 latent
    ((24, 40, 16, 20, 4, 4), "multiple of 64"),
    ((24, 40, 16, 24, 16, 8), "0 <= overlap < tile"),
    ((24, 40, 16, 24, 8, -1), "0 <= overlap < tile"),
    ((8, 40, 16, 24, 8, 8), "does not fill one tile"),
    ((24, 16, 16, 24, 8, 8), "does not fill one tile"),
    ((80, 80, 8, 8, 0, 0), "more than 64"),                # 10 x 10 tiles
])
def test_plan_refusals(args, words):
    from ccedit_amd.tiles import plan2d
    with pytest.raises(ValueError, match=re.escape(words)):
        plan2d(*args)


def test_plan_accepts_sixty_four_tiles():
    from ccedit_amd.tiles import plan2d
    assert len(plan2d(64, 64, 8, 8, 0, 0)[0]) == 64


def test_restatement_gather_and_fuse_agree_with_their_definitions():
    """The numpy restatement itself: the gather of a fused constant field is the field; a fuse of gathered tiles gives the frame back to
    within one rounding per term; a single-covered element is a bit copy."""
    rs = np.random.RandomState(3)
    h, w, th, tw = 24, 40, 16, 24
    starts, coef = TN.plan2d(h, w, th, tw, 8, 8)
    x = rs.randn(2, 3, h, w).astype(np.float32)
    xt = TN.gather(x, starts, th, tw)
    assert xt.shape == (4, 2, 3, th, tw) and np.array_equal(xt[3], x[..., 8:, 16:])
    back = TN.fuse(list(xt), starts, coef, h, w)
    assert np.abs(back - x).max() <= 4 * 2.0 ** -23 * np.abs(x).max()
    assert np.array_equal(back[..., :8, :16].view(np.int32), x[..., :8, :16].view(np.int32))        # covered by tile 0 alone
    assert TN.clamp_starts([(-3, 50)], h, w, th, tw) == [(0, 16)]


# ---- flags -------------------------------------------------------------------------------------------
def _args(*extra):
    from scripts.sampling import sampling_tv2v as S
    return S.parse_args(list(extra))


def test_tile_flags_parse_and_decide():
    from scripts.sampling import sampling_tv2v as S
    a = _args()
    assert a.tile_h == 0 and a.tile_w == 0 and a.tile_overlap is None and not S.tiling(a)
    a = _args("--H", "1024", "--W", "1536", "--tile_h", "512", "--tile_w", "768")
    assert S.tiling(a) and S.tile_overlap_px(a) == (128, 192) and S.tile_plan_args(a) == (128, 192, 64, 96, 16, 24)
    a = _args("--H", "128", "--W", "192", "--tile_h", "64", "--tile_w", "64")
    assert S.tile_overlap_px(a) == (16, 16)
    a = _args("--H", "1024", "--W", "1536", "--tile_h", "512", "--tile_w", "768", "--tile_overlap", "64")
    assert S.tile_overlap_px(a) == (64, 64)
    a = _args("--H", "320", "--W", "320", "--tile_h", "320", "--tile_w", "320")
    assert S.tile_overlap_px(a) == (80, 80)                                     # a quarter, rounded down to a multiple of 8
    assert not S.tiling(_args("--H", "512", "--W", "768", "--tile_h", "512", "--tile_w", "768"))        # one tile: the plain path
    assert S.tiling(_args("--H", "512", "--W", "776", "--tile_h", "512", "--tile_w", "768"))
    helps = {act.dest: act.help for act in S.make_parser()._actions}
    for k in ("tile_h", "tile_w", "tile_overlap"):
        assert "(not in the reference script)" in helps[k]
    for bad in (["--tile_h", "512"], ["--tile_w", "768"], ["--tile_overlap", "64"], ["--tile_h", "-64", "--tile_w", "64"]):
        with pytest.raises(SystemExit):
            S.parse_args(bad)


def test_check_tiling_passes_everything_with_tiles_off():
    from scripts.sampling import sampling_tv2v as S
    S.check_tiling(_args("--H", "100", "--W", "77"))
    S.check_tiling(_args("--H", "100", "--W", "77"), with_ref=True)
    S.check_tiling(_args("--H", "64", "--W", "64", "--tile_h", "100", "--tile_w", "100", "--tile_overlap", "3"), with_ref=True)     # frame <= tile: off


BIG = ["--H", "1024", "--W", "1536", "--num_keyframes", "17"]


@pytest.mark.parametrize("extra,exc,words", [
    (BIG + ["--tile_h", "500", "--tile_w", "768"], ValueError, "multiples of 64"),
    (BIG + ["--tile_h", "512", "--tile_w", "768", "--tile_overlap", "12"], ValueError, "multiple of 8"),
    (BIG + ["--tile_h", "512", "--tile_w", "768", "--tile_overlap", "512"], ValueError, "not smaller than the tile"),
    (["--H", "1020", "--W", "1536", "--tile_h", "512", "--tile_w", "768"], ValueError, "multiples of 8"),
    (["--H", "1024", "--W", "1540", "--tile_h", "512", "--tile_w", "768"], ValueError, "multiples of 8"),
    (["--H", "256", "--W", "1536", "--tile_h", "512", "--tile_w", "768"], ValueError, "does not fill one tile"),
    (["--H", "640", "--W", "640", "--tile_h", "64", "--tile_w", "64", "--tile_overlap", "0"], ValueError, "more than 64"),
    (["--H", "720", "--W", "1280", "--tile_h", "512", "--tile_w", "768", "--propagate", "--prompt", "a fox", "--video_path", "x",
      "--save_type", "png"], ValueError, "pyramid"),
    (["--H", "2048", "--W", "3072", "--num_keyframes", "17", "--tile_h", "512", "--tile_w", "768"], ValueError, "score matrix"),
])
def test_check_tiling_refusals(extra, exc, words):
    from scripts.sampling import sampling_tv2v as S
    with pytest.raises(exc, match=re.escape(words)):
        S.check_tiling(_args(*extra))


def test_check_tiling_accepts_the_common_sizes():
    from scripts.sampling import sampling_tv2v as S
    for hw in (("720", "1280"), ("1080", "1920"), ("1024", "1536")):
        a = _args("--H", hw[0], "--W", hw[1], "--num_keyframes", "17", "--tile_h", "512", "--tile_w", "768")
        S.check_tiling(a)
        lh, lw = int(hw[0]) // 8, int(hw[1]) // 8
        assert S.first_stage_frames(a) == max(1, 17 * 64 * 96 // (lh * lw))
    # --window_frames is T_plain when set
    a = _args("--H", "1024", "--W", "1536", "--num_keyframes", "41", "--window_frames", "17", "--tile_h", "512", "--tile_w", "768")
    assert S.first_stage_frames(a) == 4
    # --propagate at a multiple of 64 passes
    S.check_tiling(_args("--H", "1024", "--W", "1536", "--num_keyframes", "17", "--tile_h", "512", "--tile_w", "768", "--propagate", "--prompt", "a fox",
                         "--video_path", "x", "--save_type", "png"))


def test_tiles_are_refused_with_a_reference_image(tmp_path, monkeypatch):
    import yaml
    from ccedit_amd.sgm_compat import engine_config
    from scripts.sampling import sampling_tv2v as S
    from scripts.sampling import sampling_tv2v_ref as R
    flags = ["--H", "128", "--W", "192", "--tile_h", "64", "--tile_w", "64", "--num_keyframes", "3"]
    with pytest.raises(NotImplementedError, match="reference image"):
        S.check_tiling(_args(*flags), with_ref=True)
    cfg = os.path.join(str(tmp_path), "cfg.yaml")
    with open(cfg, "w") as f:
        yaml.safe_dump(dict(model=engine_config(crossframe=True, vae_ch=32, model_channels=64, num_heads=2, context_dim=64)), f)
    monkeypatch.setattr(sys, "argv", ["sampling_tv2v_ref.py", "--config_path", cfg, "--synthetic", *flags])
    with pytest.raises(NotImplementedError, match="tile_h"):
        R.main()                                                             # before a model is built (no GPU here)
    monkeypatch.setattr(sys, "argv", ["sampling_tv2v.py", "--config_path", cfg, "--synthetic", *flags])
    with pytest.raises(NotImplementedError, match="cond_feat"):
        S.main()


def test_tiled_denoiser_refusals_and_reserve_count():
    import torch
    from ccedit_amd import tiles
    from ccedit_amd.windows import plan

    class Sharded:
        frame_shard, row_shard = object(), None

    class Rows:
        frame_shard, row_shard = None, object()

    for wr in (Sharded(), Rows()):
        with pytest.raises(NotImplementedError, match="sharded"):
            tiles.TiledDenoiser(lambda x, s, c: x, (16, 24), (8, 8), wrapper=wr)
    with pytest.raises(NotImplementedError, match="cond_feat"):
        tiles.check_supported(cond=dict(crossattn=torch.zeros(1), control_hint=torch.zeros(1), cond_feat=torch.zeros(1)))
    tiles.check_supported(cond=dict(crossattn=torch.zeros(1), control_hint=torch.zeros(1)))
    with pytest.raises(ValueError):
        tiles.TiledDenoiser(lambda x, s, c: x, (16, 24), (16, 8))
    assert (tiles.TiledDenoiser(lambda x, s, c: x, (64, 96)).oh, tiles.TiledDenoiser(lambda x, s, c: x, (64, 96)).ow) == (16, 24)

    class Wrapper:
        frame_shard = row_shard = None
        reserved = []

        def reserve_windows(self, n):
            self.reserved.append(n)

    # nested with windows: 9 tiles x the windows of plan(34, 17, 8), reserved once per clip
    w = Wrapper()
    td = tiles.TiledDenoiser(lambda x, s, c: x, (64, 96), (16, 24), wrapper=w, window=17, window_overlap=8)
    nwin = len(plan(34, 17, 8)[0])
    assert nwin == 3 and tiles.window_count(34, 17, 8) == 3 and tiles.window_count(17, 17, 8) == 1 and tiles.window_count(34) == 1
    starts, sd, cd = td.tables(128, 192, 34, torch.device("cpu"))
    td.tables(128, 192, 34, torch.device("cpu"))
    assert len(starts) == 9 and w.reserved == [9 * nwin]
    assert sd.dtype == torch.int32 and tuple(sd.shape) == (9, 2) and cd.dtype == torch.float32 and tuple(cd.shape) == (9, 64, 96)
    w2 = Wrapper()
    w2.reserved = []
    tiles.TiledDenoiser(lambda x, s, c: x, (64, 96), (16, 24), wrapper=w2).tables(128, 192, 34, torch.device("cpu"))
    assert w2.reserved == [9]


def test_first_stage_group_and_frame_cap():
    from ccedit_amd import tiles
    assert tiles.first_stage_group(17, 64, 96, 128, 192) == 4
    assert tiles.first_stage_group(17, 64, 96, 64, 96) == 17
    assert tiles.first_stage_group(3, 8, 8, 16, 24) == 1
    for lh, lw in ((128, 192), (135, 240)):
        g = tiles.first_stage_group(17, 64, 96, lh, lw)
        assert g * lh * lw <= 17 * 64 * 96 < (g + 1) * lh * lw
    tiles.check_frame_cap(135, 240)
    with pytest.raises(ValueError, match="score matrix"):
        tiles.check_frame_cap(216, 216)
    assert tiles.MAX_FRAME_LATENT * (tiles.MAX_FRAME_LATENT + 3) < 2 ** 31 <= (tiles.MAX_FRAME_LATENT + 1) * (tiles.MAX_FRAME_LATENT + 4)


def test_header_names_the_tile_functions_and_keeps_the_abi():
    with open(os.path.join(ROOT, "include", "ccedit_hip.h")) as f:
        text = f.read()
    assert re.search(r"#define\s+CCEDIT_ABI_VERSION\s+12\b", text)
    assert re.search(r"\bint ccedit_tile_gather\(", text) and re.search(r"\bint ccedit_tile_fuse\(", text)
    from ccedit_amd import hip
    assert "ccedit_tile_gather" in hip._SIGS and "ccedit_tile_fuse" in hip._SIGS
